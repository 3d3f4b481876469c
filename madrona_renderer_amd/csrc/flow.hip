// Flow stage of a renderer with the optical-flow output: two kernels.
//
// flowKernel.  A work item is (view, block of 256 pixels of that view); a workgroup of 256 lanes takes items by a grid
// stride, a lane one pixel of the item: one dword of depth and one of ids in, one 16-byte store out.  The view, and with
// it the world, is the same for the whole workgroup: lane 0 reads both cameras and both sets of constants and leaves
// R(q_c), R(q_c'), c, c' and the constants in LDS, where every lane reads them by broadcast when it needs them -- 32
// values that would otherwise live in every lane's registers.  No wave ever straddles two views.
//
// The workgroup stages the rows of the view's world into LDS, kFlowPassRows at a time (flow_core.hpp flowStageRow):
// kBase, R(q_r), 1 / s_r, p_r from the live columns, R(q'_r), s'_r, p'_r from the snapshot -- computed once per row, not
// once per pixel, which gives the same bits.  A record is 33 dwords, an odd stride: lanes whose pixels belong to
// different rows read different banks, lanes of one row are served by a broadcast.  The bases of a world do not
// decrease, so a pixel's row lies in the first pass whose successor starts past the pixel's id; the lane finds it there
// by bisection and computes S17 from the record in LDS.  A world of more rows than one pass restages; a pixel is
// computed once, in its own pass.
//
// flowSnapshotKernel copies the live columns and the constants the render used into the snapshot, dword by dword.
//
// Arithmetic: S17's order, one rounding per operation, no fma (the build has -ffp-contract=off), IEEE divisions (no
// fast-math flag): NumPy float32 reproduces every bit (tests/flow_oracle.py).  The zeros of a pixel that is not valid
// are chosen by a select, never computed.
#include <algorithm>

#include <hip/hip_runtime.h>

#include "flow.hpp"

namespace mrx {

namespace {

// what the kernels read
struct FlowArgs {
    const float *depth;
    const int32_t *ids;
    float *flow;
    const uint32_t *instKBase, *worldInstStart, *viewWorld;
    FlowPose live, prev;
    const ViewProj *viewProj;
    const float *prevProj;
    float uniform[4];               // sx ox sz oz (viewProj == null)
    uint32_t nfast, pxPerView;
    uint32_t blocksPerView, items;
    uint32_t s, half;
    uint32_t passRows;
};

// (left alone the compiler loads a row's record and the view's at once and takes 114 VGPRs, four waves per SIMD; asked
// for six to eight it takes 59, with no spill: all eight workgroups a CU is sent are resident)
template <bool TRANSPOSED>
__global__ __launch_bounds__(kFlowBlock) __attribute__((amdgpu_waves_per_eu(6, 8))) void flowKernel(const FlowArgs a)
{
    __shared__ FlowRow rows[kFlowPassRows];
    __shared__ FlowView sview;

    // (the grid has at most a.items workgroups)
    for (uint32_t item = blockIdx.x;;) {
        const uint32_t view = item / a.blocksPerView, block = item - view * a.blocksPerView;
        // (a view within 255 pixels of 2^32 wraps the last block's index: the test is made in 64 bits)
        const uint32_t p = block * kFlowBlock + threadIdx.x;
        const bool inside = (uint64_t)block * kFlowBlock + threadIdx.x < a.pxPerView;
        const size_t pixel = (size_t)view * a.pxPerView + p;        // < 2^32 (checkFlow)
        float d = 0.0f;
        int32_t k = -1;
        if (inside) {
            d = a.depth[pixel];
            k = a.ids[pixel];
        }
        const uint32_t slow = p / a.nfast, fast = p - slow * a.nfast;
        const uint32_t x = TRANSPOSED ? slow : fast, y = TRANSPOSED ? fast : slow;

        __syncthreads();                // the item before is still being read
        if (threadIdx.x == 0)
            flowLoadView(view, a.live, a.prev, a.viewProj, a.uniform, a.prevProj, sview);
        const uint32_t world = a.viewWorld[view];
        const uint32_t rowLo = a.worldInstStart[world], rowHi = a.worldInstStart[world + 1];

        float out[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
        bool pending = !(d == 0.0f) && k >= 0;                      // S17 step 1
        for (uint32_t base = rowLo; base < rowHi; base += a.passRows) {
            const uint32_t n = min(a.passRows, rowHi - base);
            if (base != rowLo)
                __syncthreads();        // the pass before is still being read
            for (uint32_t i = threadIdx.x; i < n; i += kFlowBlock)
                flowStageRow(base + i, a.instKBase[base + i], a.live, a.prev, rows[i]);
            __syncthreads();
            // the first base behind this pass: an id below it has its row here (or, below the world's first base, nowhere)
            const uint32_t next = base + n < rowHi ? a.instKBase[base + n] : kFlowNoBase;
            if (pending && (uint32_t)k < next) {
                const uint32_t i = flowFindRow(rows, n, (uint32_t)k);
                if (i < n)
                    flowPixel(sview, rows[i], a.s, a.half, x, y, d, out);
                pending = false;
            }
        }
        if (inside)
            *reinterpret_cast<float4 *>(a.flow + 4 * pixel) = make_float4(out[0], out[1], out[2], out[3]);
        // (a sum that wrapped would be smaller than the item it came from)
        const uint32_t nextItem = item + gridDim.x;
        if (nextItem <= item || nextItem >= a.items)
            break;
        item = nextItem;
    }
}

struct SnapshotArgs {
    FlowPose live;
    const ViewProj *viewProj;
    float uniform[4];
    float *dst;
    uint32_t n[6];                  // dwords of the six slices
    uint32_t off[6];                // ... and where each starts in dst
};

__global__ __launch_bounds__(256) void flowSnapshotKernel(const SnapshotArgs a)
{
    uint32_t total = 0;
#pragma unroll
    for (int c = 0; c < 6; ++c)
        total += a.n[c];
    const uint32_t stride = gridDim.x * 256u;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += stride) {
        uint32_t j = i;
        if (j < a.n[0]) { a.dst[a.off[0] + j] = a.live.instPos[j]; continue; }
        j -= a.n[0];
        if (j < a.n[1]) { a.dst[a.off[1] + j] = a.live.instRot[j]; continue; }
        j -= a.n[1];
        if (j < a.n[2]) { a.dst[a.off[2] + j] = a.live.instScale[j]; continue; }
        j -= a.n[2];
        if (j < a.n[3]) { a.dst[a.off[3] + j] = a.live.camPos[j]; continue; }
        j -= a.n[3];
        if (j < a.n[4]) { a.dst[a.off[4] + j] = a.live.camRot[j]; continue; }
        j -= a.n[4];
        // sx ox sz oz of view j / 4: the first four dwords of its ViewProj record (flow_core.hpp asserts the layout)
        const uint32_t c = j & 3u;
        a.dst[a.off[5] + j] = a.viewProj ? reinterpret_cast<const float *>(a.viewProj + (j >> 2))[c]
                                         : (c == 0 ? a.uniform[0] : c == 1 ? a.uniform[1] : c == 2 ? a.uniform[2] : a.uniform[3]);
    }
}

bool posesSet(const FlowPose &q) { return q.instPos && q.instRot && q.instScale && q.camPos && q.camRot; }

}  // namespace

hipError_t checkFlow(const FlowParams &p)
{
    const uint64_t px = (uint64_t)p.nfast * p.nslow * p.numViews;
    if (px > kFlowMaxPixels || p.numCUs == 0 || (uint64_t)p.numCUs * 8u >= (1ull << 31))
        return hipErrorInvalidValue;
    if (p.s < 1 || p.s > 4 || p.half != p.s / 2)
        return hipErrorInvalidValue;
    if (!p.depth || !p.ids || !p.flow || (reinterpret_cast<uintptr_t>(p.flow) & 15u) != 0 || !p.instKBase ||
        !p.worldInstStart || !p.viewWorld || !posesSet(p.live) || !posesSet(p.prev) || !p.prevProj)
        return hipErrorInvalidValue;
    // (the snapshot's slices are counted in 32 bits)
    if (flowSnapshotLayout(p.numInstances, p.numViews).total >= (1ull << 31))
        return hipErrorInvalidValue;
    return hipSuccess;
}

hipError_t launchFlow(const FlowParams &p, hipStream_t stream)
{
    {
        const hipError_t e = checkFlow(p);
        if (e != hipSuccess)
            return e;
    }
    const uint64_t pxPerView = (uint64_t)p.nfast * p.nslow;
    if (pxPerView * p.numViews == 0)
        return hipSuccess;
    FlowArgs a;
    a.depth = p.depth;
    a.ids = p.ids;
    a.flow = p.flow;
    a.instKBase = p.instKBase;
    a.worldInstStart = p.worldInstStart;
    a.viewWorld = p.viewWorld;
    a.live = p.live;
    a.prev = p.prev;
    a.viewProj = p.viewProj;
    a.prevProj = p.prevProj;
    a.uniform[0] = p.sx; a.uniform[1] = p.ox; a.uniform[2] = p.sz; a.uniform[3] = p.oz;
    a.nfast = p.nfast;
    a.pxPerView = (uint32_t)pxPerView;
    a.blocksPerView = (uint32_t)((pxPerView + kFlowBlock - 1u) / kFlowBlock);
    // (views * blocksPerView <= (pixels + 255 * views) / 256 < 2^32 / 256 + 2^32: counted in 64 bits, refused past 2^32)
    const uint64_t items = (uint64_t)p.numViews * a.blocksPerView;
    if (items > 0xFFFFFFFFull)
        return hipErrorInvalidValue;
    a.items = (uint32_t)items;
    a.s = p.s;
    a.half = p.half;
    a.passRows = p.passRows ? std::min(p.passRows, kFlowPassRows) : kFlowPassRows;
    // as many workgroups as are resident at once (8 of 256 lanes per CU), the rest by stride
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(items, (uint64_t)p.numCUs * 8u);
    if (p.transposed)
        hipLaunchKernelGGL(flowKernel<true>, dim3(blocks), dim3(kFlowBlock), 0, stream, a);
    else
        hipLaunchKernelGGL(flowKernel<false>, dim3(blocks), dim3(kFlowBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launchFlowSnapshot(const FlowParams &p, hipStream_t stream)
{
    if (!p.snapshot || !posesSet(p.live) || p.numCUs == 0 || (uint64_t)p.numCUs * 8u * 256u >= (1ull << 31))
        return hipErrorInvalidValue;
    const FlowSnapshotLayout l = flowSnapshotLayout(p.numInstances, p.numViews);
    if (l.total >= (1ull << 31))          // (the kernel's index and its stride are both below 2^31: their sum does not wrap)
        return hipErrorInvalidValue;
    SnapshotArgs a;
    a.live = p.live;
    a.viewProj = p.viewProj;
    a.uniform[0] = p.sx; a.uniform[1] = p.ox; a.uniform[2] = p.sz; a.uniform[3] = p.oz;
    a.dst = p.snapshot;
    const uint64_t n[6] = { 3ull * p.numInstances, 4ull * p.numInstances, 3ull * p.numInstances,
                            3ull * p.numViews, 4ull * p.numViews, 4ull * p.numViews };
    const uint64_t off[6] = { l.instPos, l.instRot, l.instScale, l.camPos, l.camRot, l.proj };
    uint64_t total = 0;
    for (int c = 0; c < 6; ++c) {
        a.n[c] = (uint32_t)n[c];
        a.off[c] = (uint32_t)off[c];
        total += n[c];
    }
    if (total == 0)
        return hipSuccess;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((total + 255u) / 256u, (uint64_t)p.numCUs * 8u);
    hipLaunchKernelGGL(flowSnapshotKernel, dim3(blocks), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace mrx
