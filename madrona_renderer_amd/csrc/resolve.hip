// Resolve stage of a supersampled renderer: one streaming kernel that turns the s x s sample
// tensors into the native ones.  rgb: box filter, (sum + s*s/2) / (s*s) per byte.  depth, ids, normals: the sample
// (s/2, s/2) of the footprint, unfiltered.
//
// A lane of the vector form owns FOUR native pixels of a row: per sample row it loads 4*S consecutive dwords as S
// 16-byte loads (S*S loads in flight per lane) and stores 16 bytes per output.  That needs every row pitch to be a
// multiple of 16 bytes -- nfast % 4 == 0, whatever S -- and 16-byte aligned tensors; everything else takes the
// scalar form, one native pixel per lane with dword loads.
//
// Summing: the four bytes of a sample are summed two at a time in the 16-bit halves of a dword -- (x & 0x00FF00FF)
// holds bytes 0 and 2, ((x >> 8) & 0x00FF00FF) bytes 1 and 3; 16 samples of 255 make 4080, plus the rounding term
// 4088 < 65536, so no half ever carries into the other.
// Rounding: S = 2, 4: (h + S*S/2) >> {2, 4}, the neighbour half's bits masked off.
// S = 3: h <= 9 * 255 + 4 = 2299 and q = (h * 7282) >> 16 = floor(h / 9) for every h < 32768:
// 7282 = 65536 / 9 + 2/9, so h * 7282 / 65536 = h / 9 + h * (2/9) / 65536, and the excess is below 1/9 -- the
// distance from h / 9 to the next integer at the least -- while h * 2 < 65536.  (tests/test_supersample_cpu.py runs
// all 2300 values.)
#include <algorithm>

#include <hip/hip_runtime.h>

#include "resolve.hpp"

namespace mrx {

namespace {

constexpr uint32_t kHalves = 0x00FF00FFu;

// the sums of bytes (0, 2) in `e` and (1, 3) in `o` -> the resolved pixel
template <int S>
__device__ __forceinline__ uint32_t boxFinish(uint32_t e, uint32_t o)
{
    constexpr uint32_t rnd = (uint32_t)(S * S / 2) * 0x00010001u;
    e += rnd;
    o += rnd;
    if constexpr (S == 3) {
        const uint32_t q0 = ((e & 0xFFFFu) * 7282u) >> 16, q2 = ((e >> 16) * 7282u) & 0x00FF0000u;
        const uint32_t q1 = ((o & 0xFFFFu) * 7282u) >> 16, q3 = ((o >> 16) * 7282u) & 0x00FF0000u;
        return q0 | q2 | ((q1 | q3) << 8);
    } else {
        constexpr int sh = S == 2 ? 2 : 4;
        return ((e >> sh) & kHalves) | (((o >> sh) & kHalves) << 8);
    }
}

__device__ __forceinline__ void boxAdd(uint32_t x, uint32_t &e, uint32_t &o)
{
    e += x & kHalves;
    o += (x >> 8) & kHalves;
}

// vector form: item = (native row, group of 4 native pixels); groups = nfast / 4
template <int S>
__global__ __launch_bounds__(256) void resolveVecKernel(const ResolveParams p, uint32_t groups, uint32_t items)
{
    const size_t pitch = (size_t)p.nfast * S;           // dwords of a sample row
    for (uint32_t item = blockIdx.x * 256u + threadIdx.x; item < items;) {
        const uint32_t row = item / groups, g = item - row * groups;
        const size_t in0 = (size_t)row * S * pitch + (size_t)g * (4 * S);
        const size_t out = (size_t)row * p.nfast + (size_t)g * 4;
        if (p.rgbIn) {
            uint4 v[S][S];
#pragma unroll
            for (int j = 0; j < S; ++j)
#pragma unroll
                for (int q = 0; q < S; ++q)
                    v[j][q] = *reinterpret_cast<const uint4 *>(p.rgbIn + in0 + (size_t)j * pitch + 4 * q);
            uint32_t e[4] = { 0, 0, 0, 0 }, o[4] = { 0, 0, 0, 0 };
#pragma unroll
            for (int j = 0; j < S; ++j)
#pragma unroll
                for (int q = 0; q < S; ++q) {
                    // dword 4 * q + c of the row belongs to native pixel (4 * q + c) / S
                    boxAdd(v[j][q].x, e[(4 * q + 0) / S], o[(4 * q + 0) / S]);
                    boxAdd(v[j][q].y, e[(4 * q + 1) / S], o[(4 * q + 1) / S]);
                    boxAdd(v[j][q].z, e[(4 * q + 2) / S], o[(4 * q + 2) / S]);
                    boxAdd(v[j][q].w, e[(4 * q + 3) / S], o[(4 * q + 3) / S]);
                }
            *reinterpret_cast<uint4 *>(p.rgbOut + out) =
                make_uint4(boxFinish<S>(e[0], o[0]), boxFinish<S>(e[1], o[1]), boxFinish<S>(e[2], o[2]),
                           boxFinish<S>(e[3], o[3]));
        }
        // point samples: sample (S/2, S/2) of each of the four footprints
        const size_t pt = in0 + (size_t)(S / 2) * pitch;
        const auto gather = [&](const uint32_t *in, uint32_t *dst) {
            uint4 r;
            if constexpr (S == 2) {
                const uint4 a = *reinterpret_cast<const uint4 *>(in + pt);
                const uint4 b = *reinterpret_cast<const uint4 *>(in + pt + 4);
                r = make_uint4(a.y, a.w, b.y, b.w);
            } else {
                r = make_uint4(in[pt + S / 2], in[pt + S + S / 2], in[pt + 2 * S + S / 2], in[pt + 3 * S + S / 2]);
            }
            *reinterpret_cast<uint4 *>(dst + out) = r;
        };
        if (p.depthIn)
            gather(p.depthIn, p.depthOut);
        if (p.idsIn)
            gather(p.idsIn, p.idsOut);
        if (p.normalIn)
            gather(p.normalIn, p.normalOut);
        // (the stride is below 2^32 / 2: a wrapped sum would be smaller than the item it came from)
        const uint32_t next = item + gridDim.x * 256u;
        if (next <= item)
            break;
        item = next;
    }
}

// scalar form: item = one native pixel (unaligned pitches: nfast % 4 != 0)
template <int S>
__global__ __launch_bounds__(256) void resolveScalarKernel(const ResolveParams p, uint32_t items)
{
    const size_t pitch = (size_t)p.nfast * S;
    for (uint32_t item = blockIdx.x * 256u + threadIdx.x; item < items;) {
        const uint32_t row = item / p.nfast, x = item - row * p.nfast;
        const size_t in0 = (size_t)row * S * pitch + (size_t)x * S;
        if (p.rgbIn) {
            uint32_t v[S][S];
#pragma unroll
            for (int j = 0; j < S; ++j)
#pragma unroll
                for (int i = 0; i < S; ++i)
                    v[j][i] = p.rgbIn[in0 + (size_t)j * pitch + i];
            uint32_t e = 0, o = 0;
#pragma unroll
            for (int j = 0; j < S; ++j)
#pragma unroll
                for (int i = 0; i < S; ++i)
                    boxAdd(v[j][i], e, o);
            p.rgbOut[item] = boxFinish<S>(e, o);
        }
        const size_t pt = in0 + (size_t)(S / 2) * pitch + S / 2;
        if (p.depthIn)
            p.depthOut[item] = p.depthIn[pt];
        if (p.idsIn)
            p.idsOut[item] = p.idsIn[pt];
        if (p.normalIn)
            p.normalOut[item] = p.normalIn[pt];
        const uint32_t next = item + gridDim.x * 256u;
        if (next <= item)
            break;
        item = next;
    }
}

template <int S>
hipError_t launchResolveS(const ResolveParams &p, bool vec, hipStream_t stream)
{
    const uint64_t px = (uint64_t)p.rows * p.nfast;
    const uint32_t items = (uint32_t)(vec ? px / 4 : px);
    // a streaming kernel: as many workgroups as are resident at once (8 of 256 lanes per CU), the rest by stride
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(((uint64_t)items + 255u) / 256u, (uint64_t)p.numCUs * 8u);
    if (vec)
        hipLaunchKernelGGL(resolveVecKernel<S>, dim3(blocks), dim3(256), 0, stream, p, p.nfast / 4, items);
    else
        hipLaunchKernelGGL(resolveScalarKernel<S>, dim3(blocks), dim3(256), 0, stream, p, items);
    return hipGetLastError();
}

}  // namespace

hipError_t launchResolve(const ResolveParams &p, int s, hipStream_t stream)
{
    const uint64_t px = (uint64_t)p.rows * p.nfast;
    if (px == 0)
        return hipSuccess;
    if (px > kResolveMaxPixels || p.numCUs == 0 || (uint64_t)p.numCUs * 8u * 256u >= (1ull << 31))
        return hipErrorInvalidValue;
    const auto aligned = [](const void *a) { return (reinterpret_cast<uintptr_t>(a) & 15u) == 0; };
    const bool vec = p.nfast % 4 == 0 && aligned(p.rgbIn) && aligned(p.depthIn) && aligned(p.idsIn) &&
                     aligned(p.normalIn) && aligned(p.rgbOut) && aligned(p.depthOut) && aligned(p.idsOut) &&
                     aligned(p.normalOut);
    switch (s) {
    case 2: return launchResolveS<2>(p, vec, stream);
    case 3: return launchResolveS<3>(p, vec, stream);
    case 4: return launchResolveS<4>(p, vec, stream);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace mrx
