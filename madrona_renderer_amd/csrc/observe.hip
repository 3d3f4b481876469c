// Observation stage of a renderer with the packed observation output: one streaming kernel that
// turns the rgb and depth tensors the caller sees into the channel-first tensor a policy takes, [views][S * C][H][W],
// and keeps a stack of the last S frames in it.
//
// One entry, a template on the element type and the form; layout and S are arguments.  A lane owns its pixels across
// all S * C planes: it converts the current frame's C channel values, then moves frames 1 ... S-1 down to 0 ... S-2 --
// reading frame f + 1 before it writes frame f, in ascending f, so the shift is in place -- and writes the current
// frame to S-1.  In a view whose reset byte is not zero nothing is read: every frame is the current one.
//
// Forms.  x-fast storage (Rasterizer mode) is the image itself, so a pixel's offset in its view is its offset in every
// plane:
//   narrow  one pixel per lane, a dword load of rgb and one of depth, element stores; every size;
//   wide    four consecutive pixels per lane, one 16-byte load of rgb and one of depth and one 4 * e-byte access per
//           plane (16 B for f32, 8 B for the halves, 4 B for u8); legal when H * W % 4 == 0 -- every plane offset is
//           then a multiple of 4 * e -- and the tensors are 16-byte aligned.
// x-slow storage (Raytracer mode, [x][y]) goes through LDS in 32 x 32 tiles:
//   tile    a workgroup of 256 lanes loads a tile's rgb and depth words coalesced on y, four rows of x per lane, into
//           two tiles of rows of 33 dwords, and after a barrier reads them back by columns, coalesced on x: the row
//           write xr * 33 + l and the column read l * 33 + c both touch 32 different banks per 32-lane half.  The
//           output side, conversion and stack shift, is the narrow form's.  Edge tiles are guarded on both sides.
//
// Indexing (narrow, wide): a lane splits its FIRST item into (view, item of the view) with one integer division; the
// grid stride, split the same way on the host, is added digit by digit with a carry.  The tile form divides per tile,
// on wave-uniform values.
//
// The reset byte: a wave whose active lanes all lie in one view reads it through a readfirstlane'd index, that is
// with a scalar load; any other wave (views smaller than a wave, boundaries) reads it per lane.  A workgroup of the
// tile form lies in one view.  The kernel never writes the column -- other workgroups still read it -- the host
// enqueues a memset behind the kernel.
//
// Arithmetic: S15's, one rounding per operation, no fma (the build has -ffp-contract=off); clamps are selects
// (t > 0 ? t : 0), so a negative zero becomes +0 whatever the hardware's max does.  NumPy reproduces every bit
// (tests/observation_oracle.py).
#include <algorithm>

#include <hip/hip_runtime.h>

#include "observe.hpp"

namespace mrx {

namespace {

// what the kernel reads beside its pointers
struct ObserveArgs {
    uint32_t items;                 // pixels (narrow), groups of 4 pixels (wide), tiles (tile)
    uint32_t perView;               // items of one view
    uint32_t plane;                 // accesses of one output plane: H * W (narrow, tile), H * W / 4 (wide)
    uint32_t res, tiles;            // tile form: the view's side, tiles per side
    uint32_t layout, C, S;
    uint32_t hasRange;
    float lo, inv;
    uint32_t dView, dRem;           // the grid stride as (views, items of a view): stride = dView * perView + dRem
};

constexpr float kInv255 = 1.0f / 255.0f;    // S8's constant

// the element of one pixel and of four consecutive pixels (the compiler's own vector types: values, not structs)
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
template <uint32_t DT> struct Elem { using One = uint16_t; using Four = u32x2; };
template <> struct Elem<kObsF32> { using One = uint32_t; using Four = u32x4; };
template <> struct Elem<kObsU8> { using One = uint8_t; using Four = uint32_t; };

template <uint32_t DT>
__device__ __forceinline__ typename Elem<DT>::Four pack4(uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    if constexpr (DT == kObsF32)
        return u32x4 { a, b, c, d };
    else if constexpr (DT == kObsU8)
        return a | (b << 8) | (c << 16) | (d << 24);
    else
        return u32x2 { a | (b << 16), c | (d << 16) };
}

// a float32 value in the element type, as bits: IEEE round to nearest even (f16: subnormals kept, overflow to inf)
template <uint32_t DT>
__device__ __forceinline__ uint32_t floatBits(float v)
{
    if constexpr (DT == kObsF32) {
        return __float_as_uint(v);
    } else if constexpr (DT == kObsF16) {
        return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)v);
    } else {
        const uint32_t u = __float_as_uint(v);
        return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
    }
}

template <uint32_t DT>
__device__ __forceinline__ uint32_t colourBits(uint32_t b)
{
    if constexpr (DT == kObsU8)
        return b;
    else
        return floatBits<DT>((float)b * kInv255);
}

template <uint32_t DT>
__device__ __forceinline__ uint32_t depthBits(float o)
{
    if constexpr (DT == kObsU8) {
        const float lo = o > 0.0f ? o : 0.0f;
        const float c = lo < 1.0f ? lo : 1.0f;
        return (uint32_t)(c * 255.0f + 0.5f);
    } else {
        return floatBits<DT>(o);
    }
}

// S15 for one pixel: w = its RGBA8 word, d = its depth; ch = the C channel values of the layout as element bits
template <uint32_t DT>
__device__ __forceinline__ void channels(const ObserveArgs &a, uint32_t w, float d, uint32_t (&ch)[4])
{
    const uint32_t r = w & 255u, g = (w >> 8) & 255u, b = (w >> 16) & 255u;
    float o = d;
    if (a.hasRange) {
        const float t = (d - a.lo) * a.inv;
        const float t0 = t > 0.0f ? t : 0.0f;
        const float t1 = t0 < 1.0f ? t0 : 1.0f;
        o = d == 0.0f ? 1.0f : t1;                  // the background is as far as it gets: a select, not arithmetic
    }
    const uint32_t D = depthBits<DT>(o);
    const uint32_t y = (77u * r + 150u * g + 29u * b + 128u) >> 8;
    const bool rgb = a.layout == kObsRgb || a.layout == kObsRgbd;
    ch[0] = rgb ? colourBits<DT>(r) : a.layout == kObsD ? D : colourBits<DT>(y);
    ch[1] = rgb ? colourBits<DT>(g) : D;
    ch[2] = colourBits<DT>(b);
    ch[3] = D;
}

// the lane's access px of plane 0 of its view, planes `plane` accesses apart: shift the stack and store the current
// frame (the channel loops are unrolled over 4 with a guard: no indexed register array)
template <typename P>
__device__ __forceinline__ void pushFrame(P *px, size_t plane, const P (&cur)[4], uint32_t C, uint32_t S, bool reset)
{
    for (uint32_t f = 0; f + 1u < S; ++f) {
        P v[4];
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c) {
            v[c] = cur[c];
            if (c < C && !reset)
                v[c] = px[(size_t)((f + 1u) * C + c) * plane];
        }
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c)
            if (c < C)
                px[(size_t)(f * C + c) * plane] = v[c];
    }
#pragma unroll
    for (uint32_t c = 0; c < 4; ++c)
        if (c < C)
            px[(size_t)((S - 1u) * C + c) * plane] = cur[c];
}

template <uint32_t DT, uint32_t FORM>
__global__ __launch_bounds__(256) void observeKernel(const uint32_t *__restrict__ rgb, const float *__restrict__ depth,
                                                     void *__restrict__ obs, const uint8_t *__restrict__ reset,
                                                     const ObserveArgs a)
{
    using One = typename Elem<DT>::One;
    using Four = typename Elem<DT>::Four;
    const size_t planesPerView = (size_t)a.S * a.C;
    if constexpr (FORM == kObsTile) {
        __shared__ uint32_t tileRgb[32 * 33];
        __shared__ float tileDepth[32 * 33];
        const uint32_t tx = threadIdx.x & 31u, ty = threadIdx.x >> 5;
        for (uint32_t unit = blockIdx.x;;) {
            const uint32_t view = unit / a.perView, t = unit - view * a.perView;
            const uint32_t tileX = t / a.tiles, tileY = t - tileX * a.tiles;
            const uint32_t x0 = tileX * 32u, y0 = tileY * 32u;
            const size_t base = (size_t)view * a.plane;
            // in: rows of x, coalesced on y
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                const uint32_t xr = ty + 8u * k, x = x0 + xr, y = y0 + tx;
                if (x < a.res && y < a.res) {
                    const size_t i = base + (size_t)x * a.res + y;
                    if (rgb)
                        tileRgb[xr * 33u + tx] = rgb[i];
                    if (depth)
                        tileDepth[xr * 33u + tx] = depth[i];
                }
            }
            __syncthreads();
            const bool rs = reset ? reset[view] != 0 : false;
            // out: rows of y, coalesced on x
            for (uint32_t k = 0; k < 4; ++k) {
                const uint32_t yr = ty + 8u * k, oy = y0 + yr, ox = x0 + tx;
                if (ox < a.res && oy < a.res) {
                    const uint32_t w = rgb ? tileRgb[tx * 33u + yr] : 0u;
                    const float d = depth ? tileDepth[tx * 33u + yr] : 0.0f;
                    uint32_t ch[4];
                    channels<DT>(a, w, d, ch);
                    const One cur[4] = { (One)ch[0], (One)ch[1], (One)ch[2], (One)ch[3] };
                    One *px = static_cast<One *>(obs) + (size_t)view * planesPerView * a.plane + (size_t)oy * a.res + ox;
                    pushFrame<One>(px, a.plane, cur, a.C, a.S, rs);
                }
            }
            // (units < 2^32: a wrapped sum would be no larger than the unit it came from)
            const uint32_t next = unit + gridDim.x;
            if (next <= unit || next >= a.items)
                break;
            unit = next;
            __syncthreads();            // the tiles are read above and written again below
        }
    } else {
        uint32_t item = blockIdx.x * 256u + threadIdx.x;
        if (item >= a.items)
            return;
        uint32_t view = item / a.perView;
        uint32_t rem = item - view * a.perView;
        for (;;) {
            bool rs = false;
            if (reset) {
                const uint32_t v0 = __builtin_amdgcn_readfirstlane(view);
                if (__builtin_amdgcn_ballot_w64(view != v0) == 0)   // one view in this wave: a uniform index, a scalar load
                    rs = reset[v0] != 0;
                else
                    rs = reset[view] != 0;
            }
            if constexpr (FORM == kObsWide) {
                u32x4 w = { 0u, 0u, 0u, 0u };
                f32x4 d = { 0.0f, 0.0f, 0.0f, 0.0f };
                if (rgb)
                    w = reinterpret_cast<const u32x4 *>(rgb)[item];
                if (depth)
                    d = reinterpret_cast<const f32x4 *>(depth)[item];
                uint32_t c0[4], c1[4], c2[4], c3[4];
                channels<DT>(a, w.x, d.x, c0);
                channels<DT>(a, w.y, d.y, c1);
                channels<DT>(a, w.z, d.z, c2);
                channels<DT>(a, w.w, d.w, c3);
                const Four cur[4] = { pack4<DT>(c0[0], c1[0], c2[0], c3[0]), pack4<DT>(c0[1], c1[1], c2[1], c3[1]),
                                      pack4<DT>(c0[2], c1[2], c2[2], c3[2]), pack4<DT>(c0[3], c1[3], c2[3], c3[3]) };
                Four *px = static_cast<Four *>(obs) + (size_t)view * planesPerView * a.plane + rem;
                pushFrame<Four>(px, a.plane, cur, a.C, a.S, rs);
            } else {
                const uint32_t w = rgb ? rgb[item] : 0u;
                const float d = depth ? depth[item] : 0.0f;
                uint32_t ch[4];
                channels<DT>(a, w, d, ch);
                const One cur[4] = { (One)ch[0], (One)ch[1], (One)ch[2], (One)ch[3] };
                One *px = static_cast<One *>(obs) + (size_t)view * planesPerView * a.plane + rem;
                pushFrame<One>(px, a.plane, cur, a.C, a.S, rs);
            }
            // (the stride is below 2^31: a wrapped sum would be smaller than the item it came from)
            const uint32_t next = item + gridDim.x * 256u;
            if (next <= item || next >= a.items)
                break;
            item = next;
            // rem < perView and dRem < perView: one conditional subtraction
            rem += a.dRem;
            const uint32_t c = rem >= a.perView ? 1u : 0u;
            rem -= c ? a.perView : 0u;
            view += a.dView + c;
        }
    }
}

template <uint32_t DT>
hipError_t launchTyped(uint32_t form, uint32_t blocks, hipStream_t stream, const uint32_t *rgb, const float *depth,
                       void *obs, const uint8_t *reset, const ObserveArgs &a)
{
    if (form == kObsTile)
        hipLaunchKernelGGL((observeKernel<DT, kObsTile>), dim3(blocks), dim3(256), 0, stream, rgb, depth, obs, reset, a);
    else if (form == kObsWide)
        hipLaunchKernelGGL((observeKernel<DT, kObsWide>), dim3(blocks), dim3(256), 0, stream, rgb, depth, obs, reset, a);
    else
        hipLaunchKernelGGL((observeKernel<DT, kObsNarrow>), dim3(blocks), dim3(256), 0, stream, rgb, depth, obs, reset, a);
    return hipGetLastError();
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

uint32_t observeForm(const ObserveParams &p)
{
    if (p.transposed)
        return kObsTile;
    const bool colour = observeReadsColour(p.layout), dep = observeReadsDepth(p.layout);
    const bool wide = ((uint64_t)p.nfast * p.nslow) % 4u == 0 && aligned16(p.obs) && (!colour || aligned16(p.rgb)) &&
                      (!dep || aligned16(p.depth));
    return wide ? kObsWide : kObsNarrow;
}

hipError_t launchObserve(const ObserveParams &p, hipStream_t stream)
{
    const uint32_t C = observeChannels(p.layout);
    if (C == 0 || p.dtype > kObsU8 || p.stack < 1 || p.stack > kObsMaxStack)
        return hipErrorInvalidValue;
    const uint64_t pxPerView = (uint64_t)p.nfast * p.nslow;
    const uint64_t px = pxPerView * p.numViews;
    if (px == 0)
        return hipSuccess;
    if (px > kObserveMaxPixels || p.numCUs == 0 || (uint64_t)p.numCUs * 8u * 256u >= (1ull << 31))
        return hipErrorInvalidValue;
    const bool colour = observeReadsColour(p.layout), dep = observeReadsDepth(p.layout);
    if ((colour && !p.rgb) || (dep && !p.depth) || !p.obs || !aligned16(p.obs) || (p.stack > 1 && !p.reset) ||
        (p.transposed && p.nfast != p.nslow))
        return hipErrorInvalidValue;
    const uint32_t form = observeForm(p);
    ObserveArgs a {};
    a.layout = p.layout; a.C = C; a.S = p.stack;
    a.hasRange = p.hasRange && dep ? 1u : 0u;
    a.lo = p.lo; a.inv = p.inv;
    a.res = p.nfast;
    a.tiles = (p.nfast + 31u) / 32u;
    a.plane = (uint32_t)(form == kObsWide ? pxPerView / 4u : pxPerView);
    // a streaming kernel: as many workgroups as are resident at once (8 of 256 lanes per CU), the rest by stride
    const uint64_t resident = (uint64_t)p.numCUs * 8u;
    uint32_t blocks;
    if (form == kObsTile) {
        a.perView = a.tiles * a.tiles;                          // (at most 512 * 512)
        a.items = a.perView * p.numViews;                       // (no more than there are pixels)
        blocks = (uint32_t)std::min<uint64_t>(a.items, resident);
    } else {
        a.perView = a.plane;
        a.items = (uint32_t)(form == kObsWide ? px / 4u : px);
        blocks = (uint32_t)std::min<uint64_t>(((uint64_t)a.items + 255u) / 256u, resident);
        const uint64_t stride = (uint64_t)blocks * 256u;
        a.dView = (uint32_t)(stride / a.perView);
        a.dRem = (uint32_t)(stride % a.perView);
    }
    const uint32_t *rgb = colour ? p.rgb : nullptr;
    const float *depth = dep ? p.depth : nullptr;
    const uint8_t *reset = p.stack > 1 ? p.reset : nullptr;
    hipError_t e;
    switch (p.dtype) {
    case kObsF32: e = launchTyped<kObsF32>(form, blocks, stream, rgb, depth, p.obs, reset, a); break;
    case kObsF16: e = launchTyped<kObsF16>(form, blocks, stream, rgb, depth, p.obs, reset, a); break;
    case kObsBf16: e = launchTyped<kObsBf16>(form, blocks, stream, rgb, depth, p.obs, reset, a); break;
    default: e = launchTyped<kObsU8>(form, blocks, stream, rgb, depth, p.obs, reset, a); break;
    }
    if (e != hipSuccess || p.stack == 1)
        return e;
    // the flags are consumed by exactly this run: cleared behind the kernel, whose workgroups all read them
    return hipMemsetAsync(p.reset, 0, p.numViews, stream);
}

}  // namespace mrx
