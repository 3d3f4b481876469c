// The arithmetic of the optical-flow output, written once for the device kernel (flow.hip) and for
// the host entry (mrx_flow_host): a row's staging, the row search, the current point, its way through the instance's
// frame into the previous pose and the previous view, and the select of the result.  binary32, every operation rounded
// on its own: no fma is written and both compilers run with contraction off, so NumPy float32 reproduces every bit
// (tests/flow_oracle.py).  The divisions are IEEE divisions: no fast-math flag on either compile line.
#pragma once

#include <cstdint>

#include "stage_core.hpp"

namespace mrx {

constexpr uint32_t kFlowBlock = 256;        // pixels of one work item, one per lane
constexpr uint32_t kFlowPassRows = 64;      // staged rows of one pass (MRX_FLOW_PASS_ROWS forces fewer)
constexpr uint32_t kFlowNoBase = 0xFFFFFFFFu;

// One row as a pass stages it: 31 dwords and two of padding -- an odd stride, so that lanes that read the same field of
// different rows read different LDS banks.
struct FlowRow {
    uint32_t kBase;             // first world-local triangle index of the row
    float R[9];                 // R(q_r), row major, live
    float is[3];                // 1.0f / s_r, live
    float p[3];                 // p_r, live
    float Rp[9];                // R(q'_r), the snapshot's
    float sp[3];                // s'_r
    float pp[3];                // p'_r
    uint32_t pad[2];
};
static_assert(sizeof(FlowRow) == 33 * 4, "FlowRow is 33 dwords");

// the live columns of a renderer, or its snapshot of them
struct FlowPose {
    const float *instPos, *instRot, *instScale;     // [I][3], [I][4] w x y z, [I][3]
    const float *camPos, *camRot;                   // [views][3], [views][4]
};

// both cameras and both sets of constants of one view
struct FlowView {
    float R[9], c[3];           // R(q_c), c: live
    float Rp[9], cp[3];         // R(q_c'), c': the snapshot's
    float sx, ox, sz, oz;       // the constants the render used
    float sxp, oxp, szp, ozp;   // the snapshot's
};

MRX_HD inline void flowStageRow(uint32_t row, uint32_t kBase, const FlowPose &live, const FlowPose &prev, FlowRow &out)
{
    out.kBase = kBase;
    quatRotation(live.instRot + 4 * (size_t)row, out.R);
    quatRotation(prev.instRot + 4 * (size_t)row, out.Rp);
    for (int c = 0; c < 3; ++c) {
        out.is[c] = 1.0f / live.instScale[3 * (size_t)row + c];
        out.p[c] = live.instPos[3 * (size_t)row + c];
        out.sp[c] = prev.instScale[3 * (size_t)row + c];
        out.pp[c] = prev.instPos[3 * (size_t)row + c];
    }
    out.pad[0] = out.pad[1] = 0u;
}

MRX_HD inline void flowLoadView(uint32_t v, const FlowPose &live, const FlowPose &prev, const ViewProj *viewProj,
                                const float *uniform, const float *prevProj, FlowView &o)
{
    quatRotation(live.camRot + 4 * (size_t)v, o.R);
    quatRotation(prev.camRot + 4 * (size_t)v, o.Rp);
    for (int c = 0; c < 3; ++c) {
        o.c[c] = live.camPos[3 * (size_t)v + c];
        o.cp[c] = prev.camPos[3 * (size_t)v + c];
    }
    // (stage_core.hpp's loadProjection, written out: `o` is in LDS, and through the call the kernel's stores to it change)
    if (viewProj) {
        o.sx = viewProj[v].sx; o.ox = viewProj[v].ox; o.sz = viewProj[v].sz; o.oz = viewProj[v].oz;
    } else {
        o.sx = uniform[0]; o.ox = uniform[1]; o.sz = uniform[2]; o.oz = uniform[3];
    }
    o.sxp = prevProj[4 * (size_t)v]; o.oxp = prevProj[4 * (size_t)v + 1];
    o.szp = prevProj[4 * (size_t)v + 2]; o.ozp = prevProj[4 * (size_t)v + 3];
}

// step 3 among n staged rows whose bases do not decrease: the index of the last one with kBase <= k, n where there is
// none.  `rows` may be LDS.
MRX_HD inline uint32_t flowFindRow(const FlowRow *rows, uint32_t n, uint32_t k)
{
    uint32_t lo = 0, hi = n;            // rows below lo qualify, rows from hi on do not
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (rows[mid].kBase <= k)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo ? lo - 1 : n;
}

// steps 2 and 4 - 7 for one hit pixel (x, y) of depth d whose row is `row`; `s` the supersampling factor, half = s / 2.
// out = (dx, dy, dz, 1) where valid, four selected zeros elsewhere.
MRX_HD inline void flowPixel(const FlowView &v, const FlowRow &row, uint32_t s, uint32_t half, uint32_t x, uint32_t y,
                             float d, float *out)
{
    // (S13's view-space point, written out: through stage_core.hpp's viewPoint the kernel's instructions come in another
    // order)
    const float px = (float)(s * x + half);
    const float py = (float)(s * y + half);
    const float rx = px * v.sx + v.ox;
    const float rz = py * v.sz + v.oz;
    const float pv[3] = { d * rx, d, d * rz };
    float P[3];
    rotateAdd(v.R, pv, v.c, P);
    // into the instance's frame, out again with the previous pose
    const float u[3] = { P[0] - row.p[0], P[1] - row.p[1], P[2] - row.p[2] };
    float l[3];
    rotateT(row.R, u, l);
    const float n[3] = { (l[0] * row.is[0]) * row.sp[0], (l[1] * row.is[1]) * row.sp[1], (l[2] * row.is[2]) * row.sp[2] };
    float Pp[3];
    rotateAdd(row.Rp, n, row.pp, Pp);
    // into the previous view
    const float up[3] = { Pp[0] - v.cp[0], Pp[1] - v.cp[1], Pp[2] - v.cp[2] };
    float pvp[3];
    rotateT(v.Rp, up, pvp);
    const float Y = pvp[1];
    const bool valid = Y > 0.0f;        // false for a NaN
    const float pxp = (pvp[0] / Y - v.oxp) / v.sxp;
    const float pyp = (pvp[2] / Y - v.ozp) / v.szp;
    const float fs = (float)s;
    const float dx = (px - pxp) / fs, dy = (py - pyp) / fs, dz = d - Y;
    out[0] = valid ? dx : 0.0f;
    out[1] = valid ? dy : 0.0f;
    out[2] = valid ? dz : 0.0f;
    out[3] = valid ? 1.0f : 0.0f;
}

}  // namespace mrx
