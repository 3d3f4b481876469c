// The arithmetic of the shadow stage, written once for the device kernel (shadow.hip) and for
// the host entry (mrx_shadow_host): the shadow ray of a pixel, a row's staging, the any-hit BLAS traversal and the
// darkening of an occluded pixel.  Everything that decides a result is written elsewhere: the pixel's point is S13 as
// stage_core.hpp and cloud_core.hpp have it, the row's frame, the transform into it, the triangle test and the slab test
// are rays_core.hpp's S16.  binary32, every operation rounded on its own: no fma is written and both compilers run with contraction off,
// so NumPy float32 reproduces every bit (tests/shadow_oracle.py).
//
// The answer is an OR over a world's candidate triangles: no order of the tests, no cull and no early return changes it.
#pragma once

#include <cstdint>

#include "cloud_core.hpp"
#include "rays_core.hpp"

namespace mrx {

constexpr uint32_t kShadowBlock = 256;          // pixels of one workgroup, one per lane
constexpr uint32_t kShadowPassRows = 64;        // staged rows of one pass (MRX_SHADOW_PASS_ROWS forces fewer)
constexpr uint32_t kShadowPrepTris = 32;        // triangle records of a wave: kBvhFlatMax, a flat object in one go
constexpr float kShadowDefaultBias = 1.0f / 1024.0f;
constexpr float kShadowNoMaxDistance = 3.402823466e+38f;    // FLT_MAX: the tmax of a stage without a max_distance

// One row as the stage keeps it: rayStageFrame's record (kBase and id unused) and, because every ray of a view has one
// direction, that direction in the row's frame and its reciprocals -- computed once per row, never per pixel.
struct ShadowRow {
    RayRow r;
    float d[3], id[3];
};

// the light of a view: the unit vector towards it in world space and S7's two constants
struct ShadowLight {
    float toLight[3];
    float ambient, diffuse;
};

MRX_HD inline ShadowLight shadowLoadLight(const ViewLight *viewLight, const float *uniform, uint32_t v)
{
    ShadowLight o;
    if (viewLight) {
        o.toLight[0] = viewLight[v].toLight[0]; o.toLight[1] = viewLight[v].toLight[1];
        o.toLight[2] = viewLight[v].toLight[2];
        o.ambient = viewLight[v].ambient; o.diffuse = viewLight[v].diffuse;
    } else {
        o.toLight[0] = uniform[0]; o.toLight[1] = uniform[1]; o.toLight[2] = uniform[2];
        o.ambient = uniform[3]; o.diffuse = uniform[4];
    }
    return o;
}

// S19: is the pixel a hit pixel (false for a NaN), and its shadow ray -- o = S13's world point, d = toLight,
// tmin = bias * z, tmax = max_distance
MRX_HD inline bool shadowHit(float z) { return z > 0.0f; }

MRX_HD inline Ray shadowRay(const CloudView &cv, uint32_t s, uint32_t half, uint32_t x, uint32_t y, float z,
                            const float *toLight, float bias, float maxDistance)
{
    float p[4];
    cloudUnproject<true>(cv, s, half, x, y, z, p);
    Ray r;
    for (int c = 0; c < 3; ++c) {
        r.o[c] = p[c];
        r.d[c] = toLight[c];
    }
    r.tmin = bias * z;
    r.tmax = maxDistance;
    return r;
}

// row `row` of the instance tables -> its record for rays of direction toLight
MRX_HD inline void shadowStageRow(uint32_t row, const RayTables &s, const float *toLight, ShadowRow &out)
{
    rayStageFrame(row, s, out.r);
    Ray r;
    for (int c = 0; c < 3; ++c) {
        r.o[c] = 0.0f;
        r.d[c] = toLight[c];
    }
    float o[3];
    rayToInstance(out.r, r, o, out.d);
    rayInvDir(out.d, out.id);
}

// a pixel's origin in the row's frame (the direction is the row's own)
MRX_HD inline void shadowOrigin(const RayRow &row, const Ray &r, float *o)
{
    float d[3];
    rayToInstance(row, r, o, d);
}

// The BLAS of one object, any hit: true at the first accepted triangle.  `Stack` as rayTraverse's; the stretch of the
// slab tests is tmin ... tmax throughout, nothing shortens it.
template <typename Stack>
MRX_HD inline bool shadowTraverse(const RayRow &row, const RayTables &s, const float *o, const float *d, const float *id,
                                  float tmin, float tmax, Stack &stack)
{
    uint32_t node = (uint32_t)row.root;
    for (;;) {
        const BvhNode &n = s.nodes[node];
        for (uint32_t c = 0; c < kBvhWidth; ++c) {
            const uint32_t ch = n.child[c];
            if (ch == kBvhEmpty)
                continue;
            if (!raySlabKeeps(n.bmin[c], n.bmax[c], o, id, tmin, tmax))
                continue;
            if (ch & kBvhLeafBit) {
                const uint32_t start = ch & ((1u << kBvhLeafStartBits) - 1u);
                const uint32_t count = ((ch & ~kBvhLeafBit) >> kBvhLeafStartBits) + 1u;
                for (uint32_t i = 0; i < count; ++i) {
                    float t;
                    if (rayTriangleTest(s.tris[s.leafTris[start + i]].p, o, d, tmin, tmax, t))
                        return true;
                }
            } else if (!stack.push(ch)) {
                return false;       // (cannot happen: the stack holds 1 + 7 * depth entries)
            }
        }
        if (!stack.pop(node))
            return false;
    }
}

// One row, one ray, plain loops: the host's form of the row loop.  `brute`: no cull at all.
template <typename Stack>
MRX_HD inline bool shadowRowOccludes(const ShadowRow &row, const RayTables &s, const Ray &r, bool brute, Stack &stack)
{
    if (row.r.numTris == 0)
        return false;
    float o[3];
    shadowOrigin(row.r, r, o);
    if (!brute) {
        if (!raySlabKeeps(row.r.bbMin, row.r.bbMax, o, row.id, r.tmin, r.tmax))
            return false;
        if (row.r.root >= 0)
            return shadowTraverse(row.r, s, o, row.d, row.id, r.tmin, r.tmax, stack);
    }
    for (uint32_t i = 0; i < row.r.numTris; ++i) {
        float t;
        if (rayTriangleTest(s.tris[row.r.firstTri + i].p, o, row.d, r.tmin, r.tmax, t))
            return true;
    }
    return false;
}

// S19's application to an occluded pixel: its colour scaled down to the ambient term where the diffuse term had lit it,
// otherwise as it is.  lv: the light of the view in view space, Rc^T * toLight (S2's axes); rgb and normal are the
// packed pixels (r, nx lowest); alpha is kept.
MRX_HD inline uint32_t shadowApply(uint32_t rgb, uint32_t normal, const float *lv, float ambient, float diffuse)
{
    float c[3];
    for (int i = 0; i < 3; ++i)
        c[i] = ((float)((normal >> (8 * i)) & 255u) - 128.0f) / 127.0f;
    const float ndl = rayDot(c, lv);
    const float lit = diffuse * (ndl > 0.0f ? ndl : 0.0f) + ambient;
    if (!(lit > ambient))
        return rgb;
    const float f = ambient / lit;
    uint32_t out = rgb & 0xFF000000u;
    for (int i = 0; i < 3; ++i)
        out |= (uint32_t)((float)((rgb >> (8 * i)) & 255u) * f + 0.5f) << (8 * i);
    return out;
}

}  // namespace mrx
