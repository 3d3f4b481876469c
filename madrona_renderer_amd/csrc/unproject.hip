// Unprojection stage of a renderer with the position output: one streaming kernel that turns
// the depth tensor the caller sees into one xyzw point per pixel.  Per pixel 4 bytes are read and 16 written.
//
// An item is one native pixel, a lane owns one item at a time: a wave loads 256 contiguous bytes of depth and stores
// 1 KiB of contiguous positions, one 16-byte store per lane.  The tensor base is 16-byte aligned and every pixel's
// offset a multiple of 16, so there is one form and no tail.
//
// Indexing: a lane splits its FIRST item into (view, slow, fast) with two integer divisions; from then on the grid
// stride, split the same way on the host, is added digit by digit with a carry -- no division inside the loop.
//
// Per-view values (the camera's quaternion and position, sx ox sz oz): a wave whose active lanes all lie in one view
// -- every wave of a view of 64 pixels or more that does not straddle a boundary -- reads them through a
// readfirstlane'd index, that is with scalar loads; any other wave (views smaller than a wave, boundaries) reads them
// per lane.  Both paths run the same arithmetic.
//
// Arithmetic: S13's order, one rounding per operation, no fma (the build has -ffp-contract=off): NumPy float32
// reproduces every bit (tests/position_oracle.py).  A background pixel (depth == 0) stores four zero dwords chosen by
// a select, never a product with the depth: 0 * inf would be NaN.
#include <algorithm>

#include <hip/hip_runtime.h>

#include "stage_core.hpp"
#include "unproject.hpp"

namespace mrx {

namespace {

// what the kernel reads beside its pointers
struct UnprojectArgs {
    float sx, ox, sz, oz;           // the uniform constants (viewProj == null)
    uint32_t nfast, nslow;
    uint32_t items, pxPerView;
    uint32_t s, half;
    uint32_t dView, dSlow, dFast;   // the grid stride as (views, rows, pixels): stride = (dView * nslow + dSlow) * nfast + dFast
};

struct ViewVals {
    float sx, ox, sz, oz;
    float qw, qx, qy, qz;
    float cx, cy, cz;
};

template <bool WORLD>
__device__ __forceinline__ ViewVals loadView(const float *__restrict__ camRot, const float *__restrict__ camPos,
                                             const ViewProj *__restrict__ viewProj, const UnprojectArgs &a, uint32_t v)
{
    ViewVals o;
    if (viewProj) {
        const float4 c = *reinterpret_cast<const float4 *>(&viewProj[v]);   // sx ox sz oz: the record's first 16 bytes
        o.sx = c.x; o.ox = c.y; o.sz = c.z; o.oz = c.w;
    } else {
        o.sx = a.sx; o.ox = a.ox; o.sz = a.sz; o.oz = a.oz;
    }
    if constexpr (WORLD) {
        const float4 q = *reinterpret_cast<const float4 *>(camRot + 4 * (size_t)v);
        o.qw = q.x; o.qx = q.y; o.qy = q.z; o.qz = q.w;
        o.cx = camPos[3 * (size_t)v]; o.cy = camPos[3 * (size_t)v + 1]; o.cz = camPos[3 * (size_t)v + 2];
    } else {
        o.qw = o.qx = o.qy = o.qz = o.cx = o.cy = o.cz = 0.0f;
    }
    return o;
}

// S13 for one pixel: (x, y) = the native pixel, d = its depth
template <bool WORLD>
__device__ __forceinline__ float4 unprojectPixel(const ViewVals &v, const UnprojectArgs &a, uint32_t x, uint32_t y,
                                                 float d)
{
    const ViewPoint p = viewPoint(v.sx, v.ox, v.sz, v.oz, a.s, a.half, x, y, d);
    float o[3] = { p.v[0], p.v[1], p.v[2] };
    if constexpr (WORLD) {
        const float q[4] = { v.qw, v.qx, v.qy, v.qz }, c[3] = { v.cx, v.cy, v.cz };
        float R[9];
        quatRotation(q, R);
        rotateAdd(R, p.v, c, o);
    }
    const bool hit = !(d == 0.0f);
    return make_float4(hit ? o[0] : 0.0f, hit ? o[1] : 0.0f, hit ? o[2] : 0.0f, hit ? 1.0f : 0.0f);
}

template <bool WORLD, bool TRANSPOSED>
__global__ __launch_bounds__(256) void unprojectKernel(const float *__restrict__ depth, float *__restrict__ pos,
                                                       const float *__restrict__ camRot,
                                                       const float *__restrict__ camPos,
                                                       const ViewProj *__restrict__ viewProj, const UnprojectArgs a)
{
    uint32_t item = blockIdx.x * 256u + threadIdx.x;
    if (item >= a.items)
        return;
    uint32_t view = item / a.pxPerView;
    const uint32_t rem = item - view * a.pxPerView;
    uint32_t slow = rem / a.nfast;
    uint32_t fast = rem - slow * a.nfast;
    for (;;) {
        const float d = depth[item];
        const uint32_t x = TRANSPOSED ? slow : fast, y = TRANSPOSED ? fast : slow;
        const uint32_t v0 = __builtin_amdgcn_readfirstlane(view);
        float4 out;
        if (__builtin_amdgcn_ballot_w64(view != v0) == 0)      // one view in this wave: a uniform index, scalar loads
            out = unprojectPixel<WORLD>(loadView<WORLD>(camRot, camPos, viewProj, a, v0), a, x, y, d);
        else
            out = unprojectPixel<WORLD>(loadView<WORLD>(camRot, camPos, viewProj, a, view), a, x, y, d);
        *reinterpret_cast<float4 *>(pos + 4 * (size_t)item) = out;
        // (the stride is below 2^31: a wrapped sum would be smaller than the item it came from)
        const uint32_t next = item + gridDim.x * 256u;
        if (next <= item || next >= a.items)
            break;
        item = next;
        // fast < nfast and dFast < nfast, slow < nslow and dSlow < nslow: one conditional subtraction per digit
        fast += a.dFast;
        const uint32_t c0 = fast >= a.nfast ? 1u : 0u;
        fast -= c0 ? a.nfast : 0u;
        slow += a.dSlow + c0;
        const uint32_t c1 = slow >= a.nslow ? 1u : 0u;
        slow -= c1 ? a.nslow : 0u;
        view += a.dView + c1;
    }
}

}  // namespace

hipError_t launchUnproject(const UnprojectParams &p, hipStream_t stream)
{
    const uint64_t pxPerView = (uint64_t)p.nfast * p.nslow;
    const uint64_t px = pxPerView * p.numViews;
    if (px == 0)
        return hipSuccess;
    if (px > kUnprojectMaxPixels || p.numCUs == 0 || (uint64_t)p.numCUs * 8u * 256u >= (1ull << 31))
        return hipErrorInvalidValue;
    if ((p.frame != kFrameWorld && p.frame != kFrameView) || p.s < 1 || p.s > 4 || p.half != p.s / 2 || !p.depth ||
        !p.pos || (reinterpret_cast<uintptr_t>(p.pos) & 15u) != 0 || (p.frame == kFrameWorld && (!p.camPos || !p.camRot)))
        return hipErrorInvalidValue;
    UnprojectArgs a;
    a.sx = p.sx; a.ox = p.ox; a.sz = p.sz; a.oz = p.oz;
    a.nfast = p.nfast; a.nslow = p.nslow;
    a.items = (uint32_t)px;
    a.pxPerView = (uint32_t)pxPerView;
    a.s = p.s; a.half = p.half;
    // a streaming kernel: as many workgroups as are resident at once (8 of 256 lanes per CU), the rest by stride
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((px + 255u) / 256u, (uint64_t)p.numCUs * 8u);
    const uint64_t stride = (uint64_t)blocks * 256u;
    a.dView = (uint32_t)(stride / pxPerView);
    a.dSlow = (uint32_t)(stride % pxPerView / p.nfast);
    a.dFast = (uint32_t)(stride % pxPerView % p.nfast);
    const bool world = p.frame == kFrameWorld, tr = p.transposed != 0;
    const auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, stream, p.depth, p.pos, p.camRot, p.camPos, p.viewProj, a);
        return hipGetLastError();
    };
    return world ? (tr ? go(unprojectKernel<true, true>) : go(unprojectKernel<true, false>))
                 : (tr ? go(unprojectKernel<false, true>) : go(unprojectKernel<false, false>));
}

}  // namespace mrx
