// The arithmetic of the ray-cast sensor, written once for the device kernel (rays.hip) and for the
// host entry (mrx_trace_rays_host): the frame transform, a row's staging, the transform into an instance's frame, the
// triangle test, the slab test and the BLAS traversal.  binary32, every operation rounded on its own: no fma is written
// and both compilers run with contraction off, so NumPy float32 reproduces every bit (tests/ray_oracle.py).
//
// Only the triangle test decides a result.  The slab tests (instance box, BLAS nodes) reject what the triangle test
// would reject anyway: their boxes are padded (slabKeeps) and every comparison is written so that a NaN keeps the box.
#pragma once

#include <cstdint>

#include "stage_core.hpp"

namespace mrx {

constexpr uint32_t kRayMaxPerWorld = 65536;
constexpr uint32_t kRayBlock = 256;         // rays of one workgroup, one per lane
constexpr uint32_t kRayPassRows = 64;       // staged rows of one pass (MRX_RAY_PASS_ROWS forces fewer)
constexpr uint32_t kRayNoHit = 0xFFFFFFFFu;

// One candidate row as phase A stages it: 26 dwords.  numTris == 0: not a candidate.
struct RayRow {
    float R[9];                 // R(q_i), row major
    float is[3];                // 1.0f / scale
    float t[3];                 // position
    uint32_t firstTri, numTris;
    int32_t root;               // BLAS root, -1: flat
    float bbMin[3], bbMax[3];
    uint32_t kBase;             // first world-local triangle index of the row
    int32_t id;                 // what a hit stores: S9 / S11's segmask value
};

// the live columns and the geometry tables of a renderer, as the render kernels read them
struct RayTables {
    const ObjTri *tris;
    const BvhNode *nodes;
    const uint32_t *leafTris;
    const ObjInfo *instInfo;            // [I]
    const uint32_t *instKBase;          // [I]
    const int32_t *boundObj;            // [I]: the object each row is bound to
    const uint32_t *worldInstStart;     // [worlds + 1]
    const float *instPos, *instRot, *instScale;
    const int32_t *instObj;
    const int32_t *instLabel;           // null: no label column
};

struct RayBest {
    float t;
    uint32_t k;                 // kRayNoHit: nothing accepted yet
    int32_t id;
};

struct Ray {
    float o[3], d[3];
    float tmin, tmax;
};

MRX_HD inline float rayDot(const float *a, const float *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
MRX_HD inline void rayCross(const float *a, const float *b, float *c)
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

MRX_HD inline bool rayFinite(float v) { return v - v == 0.0f; }

// The ray of world `w` as the caller wrote it, (ox, oy, oz, tmin, dx, dy, dz, tmax), taken out of the frame of the
// world's mount row: frame in 0 ... n_w - 1 -> o = Rf * ol + p, d = Rf * dl, pose read live; any other frame -> as given.
MRX_HD inline Ray rayFromFrame(const float *in, int32_t frame, uint32_t rowLo, uint32_t rowHi, const RayTables &s)
{
    Ray r;
    r.tmin = in[3];
    r.tmax = in[7];
    if (frame >= 0 && (uint32_t)frame < rowHi - rowLo) {
        const uint32_t row = rowLo + (uint32_t)frame;
        float Rf[9];
        quatRotation(s.instRot + 4 * (size_t)row, Rf);
        const float *p = s.instPos + 3 * (size_t)row;
        for (int c = 0; c < 3; ++c) {
            r.o[c] = ((Rf[3 * c] * in[0] + Rf[3 * c + 1] * in[1]) + Rf[3 * c + 2] * in[2]) + p[c];
            r.d[c] = (Rf[3 * c] * in[4] + Rf[3 * c + 1] * in[5]) + Rf[3 * c + 2] * in[6];
        }
    } else {
        for (int c = 0; c < 3; ++c) {
            r.o[c] = in[c];
            r.d[c] = in[4 + c];
        }
    }
    return r;
}

// Phase A: row `row` of the instance tables -> its staged record.  A candidate has a live ObjectID >= 0, a bound object
// that is drawn and holds triangles, and a scale whose components are all finite and not zero.  rayStageFrame: the
// record without kBase and id, which only a stage that names what it hit reads (the shadow stage does not: S19).
MRX_HD inline void rayStageFrame(uint32_t row, const RayTables &s, RayRow &out)
{
    const ObjInfo info = s.instInfo[row];
    const float *sc = s.instScale + 3 * (size_t)row;
    const bool scaleOk = sc[0] != 0.0f && sc[1] != 0.0f && sc[2] != 0.0f && rayFinite(sc[0]) && rayFinite(sc[1]) &&
                         rayFinite(sc[2]);
    const bool cand = s.instObj[row] >= 0 && info.numTris > 0 && scaleOk;
    quatRotation(s.instRot + 4 * (size_t)row, out.R);
    for (int c = 0; c < 3; ++c) {
        out.is[c] = 1.0f / sc[c];
        out.t[c] = s.instPos[3 * (size_t)row + c];
        out.bbMin[c] = info.bbMin[c];
        out.bbMax[c] = info.bbMax[c];
    }
    out.firstTri = info.firstTri;
    out.numTris = cand ? info.numTris : 0u;
    out.root = info.root;
}

MRX_HD inline void rayStageRow(uint32_t row, const RayTables &s, RayRow &out)
{
    rayStageFrame(row, s, out);
    out.kBase = s.instKBase[row];
    const int32_t lab = s.instLabel ? s.instLabel[row] : kLabelObject;
    out.id = lab == kLabelObject ? s.boundObj[row] : lab;
}

// o'_c = ((Ri[0][c] * wv.x + Ri[1][c] * wv.y) + Ri[2][c] * wv.z) * is_c with wv = o - t_i; d' the same from d
MRX_HD inline void rayToInstance(const RayRow &row, const Ray &r, float *o, float *d)
{
    const float wv[3] = { r.o[0] - row.t[0], r.o[1] - row.t[1], r.o[2] - row.t[2] };
    for (int c = 0; c < 3; ++c) {
        o[c] = ((row.R[c] * wv[0] + row.R[3 + c] * wv[1]) + row.R[6 + c] * wv[2]) * row.is[c];
        d[c] = ((row.R[c] * r.d[0] + row.R[3 + c] * r.d[1]) + row.R[6 + c] * r.d[2]) * row.is[c];
    }
}

// Moeller-Trumbore, two-sided, on the vertices as stored; a NaN anywhere fails a comparison and rejects.  The winner
// is the smallest t, among equal t the lowest k: no order of the calls changes it.  rayTriangleTest: is the triangle
// accepted, and at which t -- all an any-hit query asks (S19).  The test in two halves: what the triangle and the
// direction give alone (RayTriPrep: 16 dwords, one 64-byte record), and the rest, which needs the origin.  Rays of one
// direction share the first half (the shadow stage computes it once per triangle); the operations and their order are
// the same however the halves are called.
struct alignas(16) RayTriPrep {
    float v0[3], e1[3], e2[3], p[3];
    float det, inv;
    float pad[2];
};
static_assert(sizeof(RayTriPrep) == 64, "RayTriPrep is four 16-byte loads");

MRX_HD inline void rayTrianglePrep(const float *v, const float *d, RayTriPrep &k)
{
    for (int c = 0; c < 3; ++c) {
        k.v0[c] = v[c];
        k.e1[c] = v[3 + c] - v[c];
        k.e2[c] = v[6 + c] - v[c];
    }
    rayCross(d, k.e2, k.p);
    k.det = rayDot(k.e1, k.p);
    k.inv = 1.0f / k.det;
    k.pad[0] = k.pad[1] = 0.0f;
}

MRX_HD inline bool rayTrianglePrepped(const RayTriPrep &k, const float *o, const float *d, float tmin, float tmax,
                                      float &t)
{
    float q[3];
    const float sv[3] = { o[0] - k.v0[0], o[1] - k.v0[1], o[2] - k.v0[2] };
    const float u = rayDot(sv, k.p) * k.inv;
    rayCross(sv, k.e1, q);
    const float w = rayDot(d, q) * k.inv;
    t = rayDot(k.e2, q) * k.inv;
    return k.det != 0.0f && u >= 0.0f && w >= 0.0f && u + w <= 1.0f && t > tmin && t <= tmax;
}

MRX_HD inline bool rayTriangleTest(const float *v, const float *o, const float *d, float tmin, float tmax, float &t)
{
    RayTriPrep k;
    rayTrianglePrep(v, d, k);
    return rayTrianglePrepped(k, o, d, tmin, tmax, t);
}

MRX_HD inline void rayTriangle(const float *v, const float *o, const float *d, float tmin, float tmax, uint32_t k,
                               int32_t id, RayBest &best)
{
    float t;
    const bool hit = rayTriangleTest(v, o, d, tmin, tmax, t);
    if (hit && (best.k == kRayNoHit || t < best.t || (t == best.t && k < best.k))) {
        best.t = t;
        best.k = k;
        best.id = id;
    }
}

// S16's degenerate rays, which miss whatever the scene: a direction that is all zero, and tmin >= tmax (or a NaN in
// either: no t passes t > tmin && t <= tmax).  A NaN direction misses through the triangle test.
MRX_HD inline bool rayDegenerate(const Ray &r)
{
    return (r.d[0] == 0.0f && r.d[1] == 0.0f && r.d[2] == 0.0f) || !(r.tmin < r.tmax);
}

// 1 / d per axis for the slab tests (inf on a zero component: handled there)
MRX_HD inline void rayInvDir(const float *d, float *id)
{
    for (int c = 0; c < 3; ++c)
        id[c] = 1.0f / d[c];
}

// Does the ray's stretch tLo ... tHi come near the box?  False only when it certainly does not.  The box is padded by
// kRaySlabPad times the largest distance, per axis, from the origin to a face of it: the triangle test's result is the
// exact one of a ray moved by a few ulps of |o' - v0|, which this bounds from above, box size and distance both.  An
// axis whose quotients are NaN (0 * inf: a zero direction component with the origin on the padded face, a NaN in
// the ray) does not narrow the stretch, and a NaN in tLo / tHi fails the last comparison: the box is kept.
constexpr float kRaySlabPad = 1.0f / 32768.0f;
MRX_HD inline bool raySlabKeeps(const float *bmin, const float *bmax, const float *o, const float *id, float tLo, float tHi)
{
    float reach = 0.0f;
    for (int c = 0; c < 3; ++c) {
        const float a = bmin[c] - o[c], b = bmax[c] - o[c];
        const float fa = a < 0.0f ? -a : a, fb = b < 0.0f ? -b : b;
        reach = fa > reach ? fa : reach;
        reach = fb > reach ? fb : reach;
    }
    const float pad = reach * kRaySlabPad;
    float tE = tLo, tX = tHi;
    for (int c = 0; c < 3; ++c) {
        const float a = ((bmin[c] - pad) - o[c]) * id[c], b = ((bmax[c] + pad) - o[c]) * id[c];
        if (a == a && b == b) {
            const float lo = a < b ? a : b, hi = a < b ? b : a;
            tE = lo > tE ? lo : tE;
            tX = hi < tX ? hi : tX;
        }
    }
    return !(tE > tX);
}

// The BLAS of one object, per ray.  `Stack` has push(uint32_t) -> bool and pop(uint32_t &) -> bool; leaves are tested
// where they are met, inner nodes pushed, so 1 + 7 * depth entries bound it (bvh.cpp).  Once something is accepted the
// stretch ends at its t (equal t stays inside: the lowest k still has to be found).
template <typename Stack>
MRX_HD inline void rayTraverse(const RayRow &row, const RayTables &s, const float *o, const float *d, const float *id,
                               float tmin, float tmax, Stack &stack, RayBest &best)
{
    uint32_t node = (uint32_t)row.root;
    for (;;) {
        const BvhNode &n = s.nodes[node];
        for (uint32_t c = 0; c < kBvhWidth; ++c) {
            const uint32_t ch = n.child[c];
            if (ch == kBvhEmpty)
                continue;
            const float tHi = best.k == kRayNoHit ? tmax : (best.t < tmax ? best.t : tmax);
            if (!raySlabKeeps(n.bmin[c], n.bmax[c], o, id, tmin, tHi))
                continue;
            if (ch & kBvhLeafBit) {
                const uint32_t start = ch & ((1u << kBvhLeafStartBits) - 1u);
                const uint32_t count = ((ch & ~kBvhLeafBit) >> kBvhLeafStartBits) + 1u;
                for (uint32_t i = 0; i < count; ++i) {
                    const uint32_t tri = s.leafTris[start + i];
                    rayTriangle(s.tris[tri].p, o, d, tmin, tmax, row.kBase + (tri - row.firstTri), row.id, best);
                }
            } else if (!stack.push(ch)) {
                return;         // (cannot happen: the stack holds 1 + 7 * depth entries)
            }
        }
        if (!stack.pop(node))
            return;
    }
}

// One row, one ray, plain loops: the host's form of phase B.  `brute`: no cull at all.
template <typename Stack>
MRX_HD inline void rayRow(const RayRow &row, const RayTables &s, const Ray &r, bool brute, Stack &stack, RayBest &best)
{
    if (row.numTris == 0)
        return;
    float o[3], d[3], id[3];
    rayToInstance(row, r, o, d);
    if (!brute) {
        rayInvDir(d, id);
        const float tHi = best.k == kRayNoHit ? r.tmax : (best.t < r.tmax ? best.t : r.tmax);
        if (!raySlabKeeps(row.bbMin, row.bbMax, o, id, r.tmin, tHi))
            return;
        if (row.root >= 0) {
            rayTraverse(row, s, o, d, id, r.tmin, r.tmax, stack, best);
            return;
        }
    }
    for (uint32_t i = 0; i < row.numTris; ++i)
        rayTriangle(s.tris[row.firstTri + i].p, o, d, r.tmin, r.tmax, row.kBase + i, row.id, best);
}

}  // namespace mrx
