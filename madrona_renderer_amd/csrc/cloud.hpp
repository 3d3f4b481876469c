// The compaction stage of a renderer with the point-cloud output: the depth tensor the caller
// sees -> N points per view, the valid pixels of a view in storage order, evenly thinned where there are more than N
// and zero-padded where there are fewer, each unprojected as the position stage would (S13); beside them the image
// pixel every point came from and the number of valid pixels.  One kernel per step behind everything else on the
// render's stream, two where a view is split over several workgroups (cloud.hip).  The arithmetic is cloud_core.hpp's,
// shared with the host entry.
#pragma once

#include <algorithm>
#include <cstdint>

#include <hip/hip_runtime_api.h>

#include "cloud_core.hpp"

namespace mrx {

// depth is [views][nslow][nfast] floats, NATIVE (on a supersampled renderer the resolved depth); points is
// [views][N][4] floats, pixel [views][N] int32, count [views] int32; sx ox sz oz / viewProj are the constants the render
// used, those of the SAMPLE image.  Pose and projection are read when the kernel runs.
struct CloudParams {
    const float *depth;
    float *points;                  // 16-byte aligned
    int32_t *pixel;
    int32_t *count;
    uint32_t *scratch;              // [views][parts] counts of a split view's parts; not read at one part per view
    uint64_t scratchCount;          // its elements
    const float *camPos;            // [views][3]
    const float *camRot;            // [views][4] w, x, y, z
    const ViewProj *viewProj;       // [views], or null: the uniform constants below
    float sx, ox, sz, oz;
    uint32_t numViews, nfast, nslow;
    uint32_t N;                     // 1 ... kCloudMaxPoints
    uint32_t s, half;               // supersampling factor (1 without) and s / 2
    int32_t frame;                  // kFrameWorld (1) or kFrameView (2): mrx_positions' values
    int32_t transposed;             // Raytracer-mode [x][y] storage
    float maxDepth;                 // 0: none
    uint32_t numCUs;
    uint32_t forcedParts;           // MRX_CLOUD_PARTS; 0: the automatic rule
};

// how many native pixels the stage can address (its pixels are counted in 32 bits), and how many one view may have
// (MRX_BUF_CLOUD_PIXEL is an int32)
constexpr uint64_t kCloudMaxPixels = 0xFFFFFFFFull;
constexpr uint64_t kCloudMaxViewPixels = 0x7FFFFFFFull;

// The workgroups per view the stage launches with.  Automatic: 1 when views >= 2 * numCUs, otherwise the smallest
// count that gives 2 * numCUs workgroups, no more than one per whole span of the view (4096 pixels: a smaller part
// would not keep its four waves busy) and no more than kCloudMaxParts.  Forced: that number, no more than one per
// segment and no more than kCloudMaxParts.
inline uint32_t cloudParts(uint32_t numViews, uint64_t pxPerView, uint32_t numCUs, uint32_t forcedParts)
{
    const uint64_t segs = (pxPerView + kCloudSeg - 1u) / kCloudSeg;
    if (forcedParts)
        return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({ forcedParts, segs, kCloudMaxParts }));
    const uint64_t want = 2ull * numCUs;
    if (numViews == 0 || numViews >= want)
        return 1;
    const uint64_t cap = std::max<uint64_t>(1, std::min<uint64_t>(segs / kCloudSpanSegs, kCloudMaxParts));
    return (uint32_t)std::min<uint64_t>((want + numViews - 1) / numViews, cap);
}

// whether the slot rule runs in 64 bits: pxPerView * N reaches 2^32
inline bool cloudWide(uint64_t pxPerView, uint32_t N) { return pxPerView * N >= (1ull << 32); }

// What launchCloud answers before it enqueues anything (host only, no HIP call): hipErrorInvalidValue for a null or
// unaligned tensor, N outside 1 ... kCloudMaxPoints, a frame other than the two, a factor outside 1 ... 4, a maxDepth
// that is negative or not finite, no CU, more pixels than kCloudMaxPixels, a view of more than kCloudMaxViewPixels,
// views * N at 2^31 or more, or a split without room for its counts.
inline hipError_t checkCloud(const CloudParams &p)
{
    const uint64_t pxPerView = (uint64_t)p.nfast * p.nslow;
    if (p.N < 1 || p.N > kCloudMaxPoints || (p.frame != 1 && p.frame != 2) || p.s < 1 || p.s > 4 || p.half != p.s / 2 ||
        p.numCUs == 0 || (uint64_t)p.numCUs * 8u >= (1ull << 31))
        return hipErrorInvalidValue;
    if (!(p.maxDepth >= 0.0f) || p.maxDepth > 3.4028234663852886e38f)
        return hipErrorInvalidValue;
    if (!p.depth || !p.points || !p.pixel || !p.count || (reinterpret_cast<uintptr_t>(p.points) & 15u) != 0 ||
        (reinterpret_cast<uintptr_t>(p.depth) & 3u) != 0 || (reinterpret_cast<uintptr_t>(p.pixel) & 3u) != 0 ||
        (reinterpret_cast<uintptr_t>(p.count) & 3u) != 0 || (p.frame == 1 && (!p.camPos || !p.camRot)))
        return hipErrorInvalidValue;
    if (pxPerView > kCloudMaxViewPixels || pxPerView * p.numViews > kCloudMaxPixels ||
        (uint64_t)p.numViews * p.N >= (1ull << 31))
        return hipErrorInvalidValue;
    const uint32_t parts = cloudParts(p.numViews, pxPerView, p.numCUs, p.forcedParts);
    if (parts > 1 && pxPerView * p.numViews != 0 && (!p.scratch || (uint64_t)p.numViews * parts > p.scratchCount))
        return hipErrorInvalidValue;
    return hipSuccess;
}

// Enqueues the stage on `stream`: nothing for zero pixels, the select kernel at one workgroup per view, the count
// kernel and the select kernel otherwise.
hipError_t launchCloud(const CloudParams &p, hipStream_t stream);

// The same source on the CPU, part by part, span by span and segment by segment as the kernels walk them
// (mrx_cloud_host): no device is touched.  `scratch` as the device's.
void cloudHost(const CloudParams &p);

}  // namespace mrx
