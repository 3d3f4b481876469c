// Compaction stage of a renderer with the point-cloud output: the depth tensor the caller sees ->
// N points per view.  Per native pixel 4 bytes are read; per view N * 20 + 4 bytes are written.
//
// A segment is 64 consecutive pixels of a view in storage order, one wave's coalesced load of 256 bytes.  The ballot of
// `valid` is the segment's mask, its popcount the segment's count, and the mbcnt of the mask below a lane that lane's
// rank inside the segment: no cross-lane reduction.  A span is 64 consecutive segments, 4096 pixels: a workgroup of
// eight waves loads a span at once, 8 segments per wave round-robin, and keeps the depths in registers -- 8 loads in
// flight per lane, each depth read from memory once.  The 64 counts of a span go to LDS; behind one barrier every wave
// scans them itself, one count per lane, and has every segment's base and the span's total.  Consecutive spans use the
// two halves of the count array in turn, so a span costs one barrier.
//
// A unit is (view, part): a part is a contiguous range of the view's segments (cloud_core.hpp cloudPartSeg), walked
// span by span.  A valid lane's rank is (valid pixels of the view ahead of the part) + (total of the part's spans
// before this one) + (base of its segment) + (its mbcnt); with the view's count M the slot rule (cloudSlot) tells the
// lane on its own whether it is selected and where it goes: no search, no atomics on the outputs.  A selected lane
// unprojects its pixel (S13, cloud_core.hpp) and stores 16 bytes of point and 4 of pixel index.  Slots from M on are
// zero-filled by a strided loop over the unit's lanes, the parts of a view taking turns.
//
// Where M comes from.  One part per view and a view of one span (the headline's 64 x 64): the span's own scan gives it;
// nothing is read twice.  One part per view and more spans: the workgroup counts the view first (countRange), then
// walks it -- the second read comes out of L2.  Several parts per view: cloudCountKernel leaves every part's count in
// a [views][parts] scratch column, and a unit of the select kernel sums the column and its own prefix of it through
// two LDS words.  Integer sums: the result does not depend on the number of parts.
//
// Per-view values (quaternion, camera position, sx ox sz oz) are read through the unit's view index, which is uniform:
// scalar loads, as in unproject.hip.
#include <algorithm>

#include <hip/hip_runtime.h>

#include "cloud.hpp"

namespace mrx {

namespace {

// what the kernels read
struct CloudArgs {
    const float *depth;
    float *points;
    int32_t *pixel;
    int32_t *count;
    uint32_t *scratch;
    const float *camRot, *camPos;
    const ViewProj *viewProj;
    float uniform[4];               // sx ox sz oz (viewProj == null)
    float maxDepth;
    uint32_t nfast, pxPerView, segs;
    uint32_t N, parts, units;
    uint32_t s, half;
    uint32_t transposed, imgW;      // imgW: the image's width, y * imgW + x the pixel index
};

// lane `lane`'s depth of segment `seg` of the view at `base`; 0 -- not valid -- past the view's or the range's end
__device__ __forceinline__ float loadDepth(const float *__restrict__ base, const CloudArgs &a, uint32_t seg,
                                           uint32_t segHi, uint32_t lane)
{
    // (a view within 63 pixels of 2^32 would wrap the last segment's index: the test is made in 64 bits)
    const uint64_t i = (uint64_t)seg * kCloudSeg + lane;
    return seg < segHi && i < a.pxPerView ? base[i] : 0.0f;
}

// the valid pixels of segments segLo ... segHi - 1, on every lane of the workgroup.  Waves take the segments
// round-robin, eight loads in flight each.  Two barriers: `red` is free again when it returns.
__device__ __forceinline__ uint32_t countRange(const float *__restrict__ base, const CloudArgs &a, uint32_t segLo,
                                               uint32_t segHi, uint32_t wave, uint32_t lane, CloudLds &lds)
{
    constexpr uint32_t kBatch = 8;
    uint32_t c = 0;
    // (segHi <= 2^26: the sums below do not wrap)
    for (uint32_t s0 = segLo + wave; s0 < segHi; s0 += kCloudWaves * kBatch) {
        float d[kBatch];
#pragma unroll
        for (uint32_t j = 0; j < kBatch; ++j)
            d[j] = loadDepth(base, a, s0 + kCloudWaves * j, segHi, lane);
#pragma unroll
        for (uint32_t j = 0; j < kBatch; ++j)
            c += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(cloudValid(d[j], a.maxDepth)));
    }
    if (lane == 0)
        lds.red[wave] = c;
    __syncthreads();
    const uint32_t total = lds.red[0] + lds.red[1] + lds.red[2] + lds.red[3] + lds.red[4] + lds.red[5] + lds.red[6] + lds.red[7];
    __syncthreads();
    return total;
}

// scratch[view][part] = the valid pixels of the part
__global__ __launch_bounds__(kCloudBlock) void cloudCountKernel(const CloudArgs a)
{
    __shared__ CloudLds lds;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint32_t unit = blockIdx.x;;) {
        const uint32_t view = unit / a.parts, part = unit - view * a.parts;
        const float *base = a.depth + (size_t)view * a.pxPerView;
        const uint32_t c = countRange(base, a, cloudPartSeg(part, a.parts, a.segs), cloudPartSeg(part + 1u, a.parts, a.segs),
                                      wave, lane, lds);
        if (threadIdx.x == 0)
            a.scratch[unit] = c;
        // (units < 2^31: the sum does not wrap)
        unit += gridDim.x;
        if (unit >= a.units)
            break;
    }
}

template <bool WORLD, typename W>
__global__ __launch_bounds__(kCloudBlock) void cloudSelectKernel(const CloudArgs a)
{
    __shared__ CloudLds lds;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint32_t unit = blockIdx.x;;) {
        const uint32_t view = unit / a.parts, part = unit - view * a.parts;
        const float *base = a.depth + (size_t)view * a.pxPerView;
        const uint32_t segLo = cloudPartSeg(part, a.parts, a.segs), segHi = cloudPartSeg(part + 1u, a.parts, a.segs);
        const CloudView cv = cloudLoadView<WORLD>(a.camRot, a.camPos, a.viewProj, a.uniform, view);
        float4 *points = reinterpret_cast<float4 *>(a.points) + (size_t)view * a.N;
        int32_t *pixel = a.pixel + (size_t)view * a.N;

        // M, and the valid pixels ahead of this part
        uint32_t M = 0, run = 0;
        const bool fromScan = a.parts == 1u && a.segs <= kCloudSpanSegs;    // the only span's scan gives M
        if (a.parts > 1u) {
            if (threadIdx.x < 2u)
                lds.sum[threadIdx.x] = 0u;
            __syncthreads();
            if (threadIdx.x < a.parts) {                                    // (parts <= kCloudMaxParts <= kCloudBlock)
                const uint32_t c = a.scratch[(size_t)view * a.parts + threadIdx.x];
                atomicAdd(&lds.sum[0], c);
                if (threadIdx.x < part)
                    atomicAdd(&lds.sum[1], c);
            }
            __syncthreads();
            M = lds.sum[0];
            run = lds.sum[1];
        } else if (!fromScan) {
            M = countRange(base, a, 0u, a.segs, wave, lane, lds);
        }

        uint32_t parity = 0;
        for (uint32_t spanLo = segLo; spanLo < segHi; spanLo += kCloudSpanSegs, parity ^= 1u) {
            float d[kCloudWaveSegs];
#pragma unroll
            for (uint32_t j = 0; j < kCloudWaveSegs; ++j)
                d[j] = loadDepth(base, a, spanLo + kCloudWaves * j + wave, segHi, lane);
            // segment 8 * j + wave of the span: its count is left on lane j, and the eight are stored at once
            uint32_t mine = 0;
#pragma unroll
            for (uint32_t j = 0; j < kCloudWaveSegs; ++j) {
                const uint32_t c = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(cloudValid(d[j], a.maxDepth)));
                mine = lane == j ? c : mine;
            }
            if (lane < kCloudWaveSegs)
                lds.cnt[parity][kCloudWaves * lane + wave] = mine;
            __syncthreads();
            // every wave scans the span's 64 counts itself: inclusive, then exclusive
            const uint32_t c = lds.cnt[parity][lane];
            uint32_t incl = c;
#pragma unroll
            for (uint32_t step = 1; step < 64u; step <<= 1) {
                const uint32_t up = (uint32_t)__shfl_up((int)incl, step);
                incl += lane >= step ? up : 0u;
            }
            const uint32_t excl = incl - c;
            const uint32_t spanTotal = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            if (fromScan)
                M = spanTotal;
            // (a loop, not eight copies of its body: the depth of segment j is picked by a chain of selects on the
            // uniform j, which keeps d[] in registers without indexing it)
#pragma unroll 1
            for (uint32_t j = 0; j < kCloudWaveSegs; ++j) {
                float dj = d[0];
#pragma unroll
                for (uint32_t q = 1; q < kCloudWaveSegs; ++q)
                    dj = j == q ? d[q] : dj;
                const uint32_t seg = spanLo + kCloudWaves * j + wave;
                const uint32_t segBase = run + (uint32_t)__builtin_amdgcn_readlane((int)excl, (int)(kCloudWaves * j + wave));
                const bool valid = cloudValid(dj, a.maxDepth);
                const uint64_t mask = __builtin_amdgcn_ballot_w64(valid);
                if (valid) {
                    const uint32_t rho = segBase + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                                                             __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
                    const uint32_t slot = cloudSlot<W>(rho, M, a.N);
                    if (slot < a.N) {                                       // (kCloudNoSlot is not)
                        const uint32_t i = seg * kCloudSeg + lane;          // (valid: inside the view, below 2^31)
                        const uint32_t slow = i / a.nfast, fast = i - slow * a.nfast;
                        const uint32_t x = a.transposed ? slow : fast, y = a.transposed ? fast : slow;
                        float o[4];
                        cloudUnproject<WORLD>(cv, a.s, a.half, x, y, dj, o);
                        points[slot] = make_float4(o[0], o[1], o[2], o[3]);
                        pixel[slot] = (int32_t)(y * a.imgW + x);
                    }
                }
            }
            run += spanTotal;
        }

        // the empty slots, the parts of the view taking turns; the count
        for (uint64_t k = (uint64_t)M + part * kCloudBlock + threadIdx.x; k < a.N; k += (uint64_t)a.parts * kCloudBlock) {
            points[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            pixel[k] = -1;
        }
        if (part == 0u && threadIdx.x == 0u)
            a.count[view] = (int32_t)M;

        // (units < 2^31: the sum does not wrap)
        unit += gridDim.x;
        if (unit >= a.units)
            break;
        __syncthreads();            // the count array and the sums are written again above
    }
}

}  // namespace

hipError_t launchCloud(const CloudParams &p, hipStream_t stream)
{
    {
        const hipError_t e = checkCloud(p);
        if (e != hipSuccess)
            return e;
    }
    const uint64_t pxPerView = (uint64_t)p.nfast * p.nslow;
    if (pxPerView * p.numViews == 0)
        return hipSuccess;
    CloudArgs a;
    a.depth = p.depth;
    a.points = p.points;
    a.pixel = p.pixel;
    a.count = p.count;
    a.scratch = p.scratch;
    a.camRot = p.camRot;
    a.camPos = p.camPos;
    a.viewProj = p.viewProj;
    a.uniform[0] = p.sx; a.uniform[1] = p.ox; a.uniform[2] = p.sz; a.uniform[3] = p.oz;
    a.maxDepth = p.maxDepth;
    a.nfast = p.nfast;
    a.pxPerView = (uint32_t)pxPerView;
    a.segs = (uint32_t)((pxPerView + kCloudSeg - 1u) / kCloudSeg);
    a.N = p.N;
    a.parts = cloudParts(p.numViews, pxPerView, p.numCUs, p.forcedParts);
    // (views * parts <= views * segs <= pixels + 63 * views; views * N < 2^31 with N >= 1: below 2^31 + 2^32, counted in
    // 64 bits and refused at 2^31)
    const uint64_t units = (uint64_t)p.numViews * a.parts;
    if (units >= (1ull << 31))
        return hipErrorInvalidValue;
    a.units = (uint32_t)units;
    a.s = p.s;
    a.half = p.half;
    a.transposed = p.transposed ? 1u : 0u;
    a.imgW = p.transposed ? p.nslow : p.nfast;
    // as many workgroups as are resident at once (4 of 512 lanes per CU), the rest by stride
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(units, (uint64_t)p.numCUs * 4u);
    if (a.parts > 1) {
        hipLaunchKernelGGL(cloudCountKernel, dim3(blocks), dim3(kCloudBlock), 0, stream, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    const bool world = p.frame == 1, wide = cloudWide(pxPerView, p.N);
    const auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kCloudBlock), 0, stream, a);
        return hipGetLastError();
    };
    return world ? (wide ? go(cloudSelectKernel<true, uint64_t>) : go(cloudSelectKernel<true, uint32_t>))
                 : (wide ? go(cloudSelectKernel<false, uint64_t>) : go(cloudSelectKernel<false, uint32_t>));
}

}  // namespace mrx
