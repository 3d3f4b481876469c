// The box stage of a renderer with box labels: the ids tensor the caller sees (the segmask of
// S9 / S11) -> per view and label the tight 2-D bounding box and the pixel count, i32 [views][K][5] =
// (xmin, ymin, xmax, ymax, count).  One reduction kernel per step behind the render, the resolve and the unprojection
// on the same stream, preceded by a small fill kernel when a view is split over several workgroups (boxes.hip).
#pragma once

#include <cstdint>

#include <hip/hip_runtime_api.h>

namespace mrx {

constexpr uint32_t kBoxMaxLabels = 1024;
// how many native pixels the stage can address (its work items are counted in 32 bits)
constexpr uint64_t kBoxMaxPixels = 0xFFFFFFFFull;

// ids is [views][nslow][nfast] int32, NATIVE (on a supersampled renderer the resolved tensor); out is [views][K][5].
struct BoxParams {
    const int32_t *ids;
    int32_t *out;
    uint32_t numViews, nfast, nslow;
    uint32_t K;                     // 1 ... kBoxMaxLabels: ids with (uint32_t)id < K are counted
    int32_t transposed;             // Raytracer-mode [x][y] storage: the slow index is the column
    uint32_t numCUs;
    uint32_t forcedParts;           // MRX_BOX_PARTS; 0: the automatic rule
};

// The workgroups per view the stage would launch with: 1 when views >= 2 * numCUs, otherwise the smallest count that
// gives 2 * numCUs workgroups; forcedParts, when not zero, instead; either capped at ceil(nslow / 4).
uint32_t boxParts(uint32_t numViews, uint32_t nslow, uint32_t numCUs, uint32_t forcedParts);

// What launchBoxes answers before it enqueues anything (host only, no HIP call): hipErrorInvalidValue for K outside
// 1 ... kBoxMaxLabels, a null pointer, no CU or more pixels than kBoxMaxPixels.
hipError_t checkBoxes(const BoxParams &p);

// Enqueues the stage on `stream`: nothing for zero views, one kernel at one workgroup per view, a fill kernel and the
// kernel otherwise.
hipError_t launchBoxes(const BoxParams &p, hipStream_t stream);

}  // namespace mrx
