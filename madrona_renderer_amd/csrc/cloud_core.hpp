// The arithmetic of the point-cloud output, written once for the device kernels (cloud.hip) and
// for the host entry (mrx_cloud_host): which depth is valid, which slot the valid pixel of a rank takes, how a view's
// segments are split over parts, and S13's unprojection of one pixel in exactly unproject.hip's operation order --
// binary32, every operation rounded on its own, no fma written and both compilers run with contraction off, the zeros
// of a background pixel chosen by a select -- so that a filled slot holds the bits MRX_BUF_POSITION holds at its pixel.
#pragma once

#include <cstdint>

#include "stage_core.hpp"

namespace mrx {

constexpr uint32_t kCloudBlock = 512;           // lanes of a workgroup: eight waves
constexpr uint32_t kCloudWaves = 8;
constexpr uint32_t kCloudSeg = 64;              // pixels of a segment: one per lane of a wave
constexpr uint32_t kCloudSpanSegs = 64;         // segments of a span: 8 per wave, one count per lane of the scan
constexpr uint32_t kCloudWaveSegs = kCloudSpanSegs / kCloudWaves;
constexpr uint32_t kCloudMaxPoints = 65536;     // N
constexpr uint32_t kCloudMaxParts = 256;        // workgroups per view: no more than a workgroup has lanes
constexpr uint32_t kCloudNoSlot = 0xFFFFFFFFu;

// what a workgroup of the select kernel keeps in LDS: the counts of a span's segments, twice (consecutive spans
// alternate, one barrier per span), one count per wave, and the two sums over a split view's parts
struct CloudLds {
    uint32_t cnt[2][kCloudSpanSegs];
    uint32_t red[kCloudWaves];
    uint32_t sum[2];
};
constexpr uint32_t kCloudLdsBytes = (uint32_t)sizeof(CloudLds);

// S18: a depth that is a point of the cloud.  False for a NaN.
MRX_HD inline bool cloudValid(float d, float maxDepth) { return d > 0.0f && (maxDepth == 0.0f || d <= maxDepth); }

// S18's slot rule as a scatter: the slot of the valid pixel of rank rho < M among M valid pixels and N slots, or
// kCloudNoSlot.  M < N: slot rho.  M >= N: slot k takes rank floor(k * M / N), so rho is taken iff k0 = ceil(rho * N / M)
// is below N and floor(k0 * M / N) == rho, and then by k0 alone.  W: uint32_t where pxPerView * N < 2^32 -- rho * N
// and k0 * M are both below it --, uint64_t otherwise.
template <typename W>
MRX_HD inline uint32_t cloudSlot(uint32_t rho, uint32_t M, uint32_t N)
{
    if (M < N)
        return rho;
    const W num = (W)rho * (W)N;
    const W q = num / (W)M;
    const W k0 = q * (W)M != num ? q + 1u : q;
    if (k0 >= (W)N)
        return kCloudNoSlot;
    return (k0 * (W)M) / (W)N == (W)rho ? (uint32_t)k0 : kCloudNoSlot;
}

// the first segment of part `part` of `parts` over `segs` segments (part == parts: segs)
MRX_HD inline uint32_t cloudPartSeg(uint32_t part, uint32_t parts, uint32_t segs)
{
    return (uint32_t)((uint64_t)part * segs / parts);
}

// a view's camera and constants: R(q) (S1, the quaternion used as given), c, sx ox sz oz
struct CloudView {
    float sx, ox, sz, oz;
    float R[9], c[3];
};

template <bool WORLD>
MRX_HD inline CloudView cloudLoadView(const float *camRot, const float *camPos, const ViewProj *viewProj,
                                      const float *uniform, uint32_t v)
{
    CloudView o;
    loadProjection(viewProj, uniform, v, o.sx, o.ox, o.sz, o.oz);
    if constexpr (WORLD) {
        quatRotation(camRot + 4 * (size_t)v, o.R);
        for (int i = 0; i < 3; ++i)
            o.c[i] = camPos[3 * (size_t)v + i];
    } else {
        for (int i = 0; i < 9; ++i)
            o.R[i] = 0.0f;
        o.c[0] = o.c[1] = o.c[2] = 0.0f;
    }
    return o;
}

// S13 for one pixel: (x, y) = the native pixel, d = its depth; s the supersampling factor, half = s / 2
template <bool WORLD>
MRX_HD inline void cloudUnproject(const CloudView &v, uint32_t s, uint32_t half, uint32_t x, uint32_t y, float d,
                                  float *out)
{
    const ViewPoint q = viewPoint(v.sx, v.ox, v.sz, v.oz, s, half, x, y, d);
    float o[3] = { q.v[0], q.v[1], q.v[2] };
    if constexpr (WORLD)
        rotateAdd(v.R, q.v, v.c, o);
    const bool hit = !(d == 0.0f);
    out[0] = hit ? o[0] : 0.0f;
    out[1] = hit ? o[1] : 0.0f;
    out[2] = hit ? o[2] : 0.0f;
    out[3] = hit ? 1.0f : 0.0f;
}

}  // namespace mrx
