// Box stage of a renderer with box labels: one reduction kernel that turns the ids tensor the
// caller sees into per-view, per-label bounding boxes and pixel counts.  Per native pixel 4 bytes are read; per view
// K rows of 20 bytes are written.
//
// An item is one row segment -- (view, slow index, 64 consecutive fast pixels) -- and a wave owns one item at a time:
// it loads up to 256 contiguous bytes, and every active lane of the item shares the slow index.  A workgroup of four
// waves belongs to one view, or to one part of a view (a contiguous range of rows); its waves take the rows
// round-robin.  Loads run one batch of items ahead of the accumulation, so a wave waits for memory once per batch.
//
// Accumulation (label peeling): lanes past the row's end and ids outside 0 ... K-1 -- one unsigned compare -- drop
// out of `valid`.  While ballot(valid) is not empty the label of its first lane is read with readlane, a second ballot
// gives the lanes that hold it, and popcount / ctz / clz of that mask are the segment's count and its lowest and
// highest fast index: scalar bit operations, no cross-lane reduction.  One lane applies them and the slow index to
// the workgroup's table in LDS with integer atomics (the four waves share the table).  An all-background segment
// costs one ballot.
//
// Table: K x (fast min, slow min, fast max, slow max, count), initialised to the identities (nfast, nslow, -1, -1, 0).
// After a barrier the workgroup's lanes write it out, element by element, swapping the fast and slow bounds into
// (x, y) order on transposed storage.  With one workgroup per view these are plain stores of all K rows; with several
// a fill kernel has written the identities first and each part merges its non-empty rows with global integer
// atomics.  Min, max and add of integers: the result does not depend on the order, both forms give the same tensor.
#include <algorithm>

#include <hip/hip_runtime.h>

#include "boxes.hpp"

namespace mrx {

namespace {

constexpr uint32_t kBatch = 4;      // items a wave has in flight

struct BoxArgs {
    uint32_t nfast, nslow;
    uint32_t segs;                  // 64-pixel segments per row
    uint32_t K;
    uint32_t parts, units;          // workgroups per view; views * parts
    uint32_t transposed;
};

// a wave's place in its part: the row and the segment of the next item; rows round-robin over the four waves
struct Cursor {
    uint32_t row, seg;
    __device__ __forceinline__ void advance(uint32_t segs)
    {
        if (++seg == segs) {
            seg = 0;
            row += 4;
        }
    }
};

// the identity of table column c: (nfast, nslow, -1, -1, 0)
__device__ __forceinline__ int32_t identity(const BoxArgs &a, uint32_t c)
{
    return c == 0 ? (int32_t)a.nfast : c == 1 ? (int32_t)a.nslow : c == 4 ? 0 : -1;
}

// one item: `id` is the lane's id, or -1 on a lane past the row's end
__device__ __forceinline__ void accumulate(int32_t *tab, const BoxArgs &a, int32_t id, uint32_t slow, uint32_t fastBase,
                                           uint32_t lane)
{
    uint64_t valid = __builtin_amdgcn_ballot_w64((uint32_t)id < a.K);
    while (valid) {
        const int32_t l0 = __builtin_amdgcn_readlane(id, (int)__builtin_ctzll(valid));
        const uint64_t m = __builtin_amdgcn_ballot_w64(id == l0);      // (l0 < K: every lane of m is one of valid)
        if (lane == 0) {
            int32_t *row = tab + 5 * l0;
            atomicMin(row + 0, (int32_t)(fastBase + (uint32_t)__builtin_ctzll(m)));
            atomicMin(row + 1, (int32_t)slow);
            atomicMax(row + 2, (int32_t)(fastBase + 63u - (uint32_t)__builtin_clzll(m)));
            atomicMax(row + 3, (int32_t)slow);
            atomicAdd(row + 4, (int32_t)__builtin_popcountll(m));
        }
        valid &= ~m;
    }
}

__global__ __launch_bounds__(256) void boxKernel(const int32_t *__restrict__ ids, int32_t *__restrict__ out,
                                                 const BoxArgs a)
{
    __shared__ int32_t tab[kBoxMaxLabels * 5];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t cells = a.K * 5u;
    for (uint32_t unit = blockIdx.x;;) {
        const uint32_t view = unit / a.parts, part = unit - view * a.parts;
        const uint32_t rowLo = (uint32_t)((uint64_t)part * a.nslow / a.parts);
        const uint32_t rowHi = (uint32_t)((uint64_t)(part + 1u) * a.nslow / a.parts);
        for (uint32_t i = threadIdx.x; i < cells; i += 256u)
            tab[i] = identity(a, i % 5u);
        __syncthreads();

        const int32_t *base = ids + (size_t)view * a.nslow * a.nfast;
        const auto load = [&](int32_t (&dst)[kBatch], Cursor &c) {
#pragma unroll
            for (uint32_t k = 0; k < kBatch; ++k) {
                int32_t v = -1;
                if (c.row < rowHi) {
                    const uint32_t fast = c.seg * 64u + lane;
                    if (fast < a.nfast)
                        v = base[(size_t)c.row * a.nfast + fast];
                    c.advance(a.segs);
                }
                dst[k] = v;
            }
        };
        Cursor lc { rowLo + wave, 0u }, pc = lc;
        int32_t cur[kBatch], nxt[kBatch];
        load(cur, lc);
        while (pc.row < rowHi) {
            load(nxt, lc);
#pragma unroll
            for (uint32_t k = 0; k < kBatch; ++k) {
                if (pc.row < rowHi) {
                    accumulate(tab, a, cur[k], pc.row, pc.seg * 64u, lane);
                    pc.advance(a.segs);
                }
            }
#pragma unroll
            for (uint32_t k = 0; k < kBatch; ++k)
                cur[k] = nxt[k];
        }
        __syncthreads();

        // table cell (l, c) -> out[view][l][c]; on transposed storage x is the slow index: columns 0 <-> 1, 2 <-> 3
        int32_t *o = out + (size_t)view * cells;
        for (uint32_t i = threadIdx.x; i < cells; i += 256u) {
            const uint32_t l = i / 5u, c = i - 5u * l;
            const int32_t v = tab[5u * l + ((a.transposed && c < 4u) ? (c ^ 1u) : c)];
            if (a.parts == 1u)
                o[i] = v;
            else if (tab[5u * l + 4u] > 0) {
                if (c < 2u)
                    atomicMin(o + i, v);
                else if (c < 4u)
                    atomicMax(o + i, v);
                else
                    atomicAdd(o + i, v);
            }
        }
        // (units < 2^32: a wrapped sum would be no larger than the unit it came from)
        const uint32_t next = unit + gridDim.x;
        if (next <= unit || next >= a.units)
            break;
        unit = next;
        __syncthreads();            // the table is read above and initialised again below
    }
}

// the identities into every row: what the parts of a split view merge into
__global__ __launch_bounds__(256) void boxFillKernel(int32_t *__restrict__ out, uint64_t cells, int32_t w, int32_t h)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < cells; i += (uint64_t)gridDim.x * 256u) {
        const uint32_t c = (uint32_t)(i % 5u);
        out[i] = c == 0 ? w : c == 1 ? h : c == 4 ? 0 : -1;
    }
}

}  // namespace

uint32_t boxParts(uint32_t numViews, uint32_t nslow, uint32_t numCUs, uint32_t forcedParts)
{
    const uint32_t cap = std::max(1u, (nslow + 3u) / 4u);           // every part has a row per wave
    if (forcedParts)
        return std::min(forcedParts, cap);
    const uint64_t want = 2ull * numCUs;
    if (numViews == 0 || numViews >= want)
        return 1;
    return (uint32_t)std::min<uint64_t>((want + numViews - 1) / numViews, cap);
}

hipError_t checkBoxes(const BoxParams &p)
{
    if (p.K < 1 || p.K > kBoxMaxLabels || !p.ids || !p.out || p.numCUs == 0 ||
        (uint64_t)p.numCUs * 8u >= (1ull << 31))
        return hipErrorInvalidValue;
    if ((uint64_t)p.nfast * p.nslow * p.numViews > kBoxMaxPixels)
        return hipErrorInvalidValue;
    return hipSuccess;
}

hipError_t launchBoxes(const BoxParams &p, hipStream_t stream)
{
    {
        const hipError_t e = checkBoxes(p);
        if (e != hipSuccess)
            return e;
    }
    if ((uint64_t)p.nfast * p.nslow * p.numViews == 0)
        return hipSuccess;
    BoxArgs a;
    a.nfast = p.nfast; a.nslow = p.nslow;
    a.segs = (p.nfast + 63u) / 64u;
    a.K = p.K;
    a.parts = boxParts(p.numViews, p.nslow, p.numCUs, p.forcedParts);
    a.units = p.numViews * a.parts;                                 // parts <= nslow: no more than there are pixels
    a.transposed = p.transposed ? 1u : 0u;
    // as many workgroups as are resident at once (8 of 256 lanes per CU), the rest by stride
    const uint32_t resident = p.numCUs * 8u;
    if (a.parts > 1) {
        const uint64_t cells = (uint64_t)p.numViews * p.K * 5u;
        const uint32_t blocks = (uint32_t)std::min<uint64_t>((cells + 255u) / 256u, resident);
        const int32_t w = (int32_t)(p.transposed ? p.nslow : p.nfast), h = (int32_t)(p.transposed ? p.nfast : p.nslow);
        hipLaunchKernelGGL(boxFillKernel, dim3(blocks), dim3(256), 0, stream, p.out, cells, w, h);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    hipLaunchKernelGGL(boxKernel, dim3(std::min(a.units, resident)), dim3(256), 0, stream, p.ids, p.out, a);
    return hipGetLastError();
}

}  // namespace mrx
