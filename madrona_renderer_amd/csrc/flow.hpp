// The flow stage of a renderer with the optical-flow output: per native pixel the image-space
// displacement, since the snapshot was taken, of the surface point the pixel sees -- from the depth and the visibility
// ids the caller sees, the live pose, scale and camera columns, the projection constants and the snapshot of all of
// them.  Two kernels behind everything else on the render's stream (flow.hip): the flow, then the snapshot that copies
// the live state for the next step.  The arithmetic is flow_core.hpp's, shared with the host entry.
#pragma once

#include <cstdint>

#include <hip/hip_runtime_api.h>

#include "flow_core.hpp"

namespace mrx {

// depth is [views][nslow][nfast] floats, ids the same of int32, flow [views][nslow][nfast][4], all NATIVE (on a
// supersampled renderer the resolved tensors); sx ox sz oz / viewProj are the constants the render used, those of the
// SAMPLE image.  prevProj is the snapshot's [views][4].  Pose, projection and snapshot are read when the kernel runs.
struct FlowParams {
    const float *depth;
    const int32_t *ids;             // visibility ids, -1: background
    float *flow;                    // 16-byte aligned
    const uint32_t *instKBase;      // [I], non-decreasing within a world
    const uint32_t *worldInstStart; // [worlds + 1]
    const uint32_t *viewWorld;      // [views]
    FlowPose live, prev;
    const ViewProj *viewProj;       // [views], or null: the uniform constants below
    float sx, ox, sz, oz;
    const float *prevProj;          // [views][4]: the snapshot's constants
    float *snapshot;                // the allocation prev and prevProj lie in (flowBindSnapshot); null: no snapshot stage
    uint32_t numViews, numInstances, nfast, nslow;
    uint32_t s, half;               // supersampling factor (1 without) and s / 2
    int32_t transposed;             // Raytracer-mode [x][y] storage
    uint32_t numCUs;
    uint32_t passRows;              // MRX_FLOW_PASS_ROWS; 0: kFlowPassRows
};

// how many native pixels the stage can address (its pixels are counted in 32 bits)
constexpr uint64_t kFlowMaxPixels = 0xFFFFFFFFull;

// dwords of a snapshot of `instances` rows and `views` views: position, rotation, scale; camera position, rotation;
// the four constants -- in this order, each slice a multiple of 4 dwords long from a 16-byte aligned base
struct FlowSnapshotLayout {
    uint64_t instPos, instRot, instScale, camPos, camRot, proj, total;     // dword offsets
};
inline FlowSnapshotLayout flowSnapshotLayout(uint64_t instances, uint64_t views)
{
    const auto up = [](uint64_t n) { return (n + 3u) & ~(uint64_t)3u; };
    FlowSnapshotLayout l;
    l.instPos = 0;
    l.instRot = l.instPos + up(3 * instances);
    l.instScale = l.instRot + up(4 * instances);
    l.camPos = l.instScale + up(3 * instances);
    l.camRot = l.camPos + up(3 * views);
    l.proj = l.camRot + up(4 * views);
    l.total = l.proj + up(4 * views);
    return l;
}
// points snapshot, prev and prevProj of `p` into a snapshot allocation (numInstances and numViews are set)
inline void flowBindSnapshot(float *base, FlowParams &p)
{
    const FlowSnapshotLayout l = flowSnapshotLayout(p.numInstances, p.numViews);
    p.snapshot = base;
    p.prev.instPos = base + l.instPos;
    p.prev.instRot = base + l.instRot;
    p.prev.instScale = base + l.instScale;
    p.prev.camPos = base + l.camPos;
    p.prev.camRot = base + l.camRot;
    p.prevProj = base + l.proj;
}

// hipErrorInvalidValue for a factor outside 1 ... 4, a null or unaligned tensor, no CU or more pixels than
// kFlowMaxPixels -- there is no other path.
hipError_t checkFlow(const FlowParams &p);

// Enqueues the flow kernel on `stream` (nothing for zero pixels).
hipError_t launchFlow(const FlowParams &p, hipStream_t stream);

// Enqueues the snapshot kernel on `stream`: the live columns and the constants the render used -> prev / prevProj.
hipError_t launchFlowSnapshot(const FlowParams &p, hipStream_t stream);

// The same source on the CPU, pixel by pixel (mrx_flow_host): no device is touched.
void flowHost(const FlowParams &p);

}  // namespace mrx
