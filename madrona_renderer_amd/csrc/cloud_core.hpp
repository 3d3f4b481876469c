// The arithmetic of the point-cloud output, written once for the device kernels (cloud.hip) and
// for the host entry (mrx_cloud_host): which depth is valid, which slot the valid pixel of a rank takes, how a view's
// segments are split over parts, and S13's unprojection of one pixel in exactly unproject.hip's operation order --
// binary32, every operation rounded on its own, no fma written and both compilers run with contraction off, the zeros
// of a background pixel chosen by a select -- so that a filled slot holds the bits MRX_BUF_POSITION holds at its pixel.
#pragma once

#include <cstddef>
#include <cstdint>

#include "raster.hpp"

namespace mrx {

static_assert(offsetof(ViewProj, sx) == 0 && offsetof(ViewProj, ox) == 4 && offsetof(ViewProj, sz) == 8 &&
              offsetof(ViewProj, oz) == 12, "ViewProj begins with sx ox sz oz");

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
    if (viewProj) {
        o.sx = viewProj[v].sx; o.ox = viewProj[v].ox; o.sz = viewProj[v].sz; o.oz = viewProj[v].oz;
    } else {
        o.sx = uniform[0]; o.ox = uniform[1]; o.sz = uniform[2]; o.oz = uniform[3];
    }
    if constexpr (WORLD) {
        const float *q = camRot + 4 * (size_t)v;
        const float w = q[0], x = q[1], y = q[2], z = q[3];
        const float x2 = x + x, y2 = y + y, z2 = z + z;
        const float xx = x * x2, yy = y * y2, zz = z * z2;
        const float xy = x * y2, xz = x * z2, yz = y * z2;
        const float wx = w * x2, wy = w * y2, wz = w * z2;
        o.R[0] = 1.0f - (yy + zz); o.R[1] = xy - wz;          o.R[2] = xz + wy;
        o.R[3] = xy + wz;          o.R[4] = 1.0f - (xx + zz); o.R[5] = yz - wx;
        o.R[6] = xz - wy;          o.R[7] = yz + wx;          o.R[8] = 1.0f - (xx + yy);
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
    const float px = (float)(s * x + half);
    const float py = (float)(s * y + half);
    const float rx = px * v.sx + v.ox;
    const float rz = py * v.sz + v.oz;
    const float vx = d * rx, vy = d, vz = d * rz;
    float ox = vx, oy = vy, oz = vz;
    if constexpr (WORLD) {
        ox = ((v.R[0] * vx + v.R[1] * vy) + v.R[2] * vz) + v.c[0];
        oy = ((v.R[3] * vx + v.R[4] * vy) + v.R[5] * vz) + v.c[1];
        oz = ((v.R[6] * vx + v.R[7] * vy) + v.R[8] * vz) + v.c[2];
    }
    const bool hit = !(d == 0.0f);
    out[0] = hit ? ox : 0.0f;
    out[1] = hit ? oy : 0.0f;
    out[2] = hit ? oz : 0.0f;
    out[3] = hit ? 1.0f : 0.0f;
}

}  // namespace mrx
