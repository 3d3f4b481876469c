// What the post-render stages share, written once for their device kernels and their host entries:
// the rotation of a quaternion, R * v + t and R^T * v, the view-space point of a pixel, the read of a view's projection
// constants and the host's traversal stack; for device code also the traversal stack in LDS and the wave-uniform reads.
// binary32, every operation rounded on its own: no fma is written and both compilers run with contraction off, so NumPy
// float32 reproduces every bit.  The stages' own arithmetic is in rays_core.hpp, flow_core.hpp, cloud_core.hpp and
// shadow_core.hpp.  Two places keep a copy because their kernels' code changes through the call: unproject.hip's load of
// a view's values (vector loads of the records) and flow_core.hpp's projection read and view-space point.
#pragma once

#include <cstddef>
#include <cstdint>

#include "bvh.hpp"

namespace mrx {

// the kernels and the host entries take sx ox sz oz as the first 16 bytes of a view's record
static_assert(offsetof(ViewProj, sx) == 0 && offsetof(ViewProj, ox) == 4 && offsetof(ViewProj, sz) == 8 &&
              offsetof(ViewProj, oz) == 12, "ViewProj begins with sx ox sz oz");

// S1, the quaternion (w, x, y, z) used as given; R row major
MRX_HD inline void quatRotation(const float *q, float *R)
{
    const float w = q[0], x = q[1], y = q[2], z = q[3];
    const float x2 = x + x, y2 = y + y, z2 = z + z;
    const float xx = x * x2, yy = y * y2, zz = z * z2;
    const float xy = x * y2, xz = x * z2, yz = y * z2;
    const float wx = w * x2, wy = w * y2, wz = w * z2;
    R[0] = 1.0f - (yy + zz); R[1] = xy - wz;          R[2] = xz + wy;
    R[3] = xy + wz;          R[4] = 1.0f - (xx + zz); R[5] = yz - wx;
    R[6] = xz - wy;          R[7] = yz + wx;          R[8] = 1.0f - (xx + yy);
}

// R * v + t, S13's order
MRX_HD inline void rotateAdd(const float *R, const float *v, const float *t, float *out)
{
    for (int i = 0; i < 3; ++i)
        out[i] = ((R[3 * i] * v[0] + R[3 * i + 1] * v[1]) + R[3 * i + 2] * v[2]) + t[i];
}

// R^T * v
MRX_HD inline void rotateT(const float *R, const float *v, float *out)
{
    for (int j = 0; j < 3; ++j)
        out[j] = (R[j] * v[0] + R[3 + j] * v[1]) + R[6 + j] * v[2];
}

// sx ox sz oz of view `v`: its record of the per-view table, else the four uniform constants
MRX_HD inline void loadProjection(const ViewProj *viewProj, const float *uniform, uint32_t v, float &sx, float &ox,
                                  float &sz, float &oz)
{
    if (viewProj) {
        sx = viewProj[v].sx; ox = viewProj[v].ox; sz = viewProj[v].sz; oz = viewProj[v].oz;
    } else {
        sx = uniform[0]; ox = uniform[1]; sz = uniform[2]; oz = uniform[3];
    }
}

// S13's view-space point of the native pixel (x, y) of depth d; s the supersampling factor, half = s / 2.  px, py: the
// index of the sample the depth was taken from, as the render kernels form it -- S5's ox / oz carry the half pixel that
// makes it the sample's centre.
struct ViewPoint {
    float px, py;
    float v[3];
};
MRX_HD inline ViewPoint viewPoint(float sx, float ox, float sz, float oz, uint32_t s, uint32_t half, uint32_t x,
                                  uint32_t y, float d)
{
    ViewPoint o;
    o.px = (float)(s * x + half);
    o.py = (float)(s * y + half);
    const float rx = o.px * sx + ox;
    const float rz = o.py * sz + oz;
    o.v[0] = d * rx; o.v[1] = d; o.v[2] = d * rz;
    return o;
}

// the traversal stack of a host entry (rayTraverse's `Stack`); in an unnamed namespace, so that what an entry
// instantiates with it stays local to its unit: the library exports no symbol for it
namespace {
struct HostStack {
    uint32_t v[kBvhStackCap];
    uint32_t sp = 0;
    bool push(uint32_t x)
    {
        if (sp >= kBvhStackCap)
            return false;
        v[sp++] = x;
        return true;
    }
    bool pop(uint32_t &x)
    {
        if (sp == 0)
            return false;
        x = v[--sp];
        return true;
    }
};
}  // namespace

#if defined(__HIPCC__)
// the traversal stack of one lane of a workgroup of BLOCK lanes: entry e lies at base[e * BLOCK], the lanes of an entry
// side by side
template <uint32_t BLOCK>
struct LaneStack {
    uint32_t *base;
    uint32_t sp, cap;
    __device__ __forceinline__ bool push(uint32_t v)
    {
        if (sp >= cap)
            return false;
        base[sp * BLOCK] = v;
        ++sp;
        return true;
    }
    __device__ __forceinline__ bool pop(uint32_t &v)
    {
        if (sp == 0)
            return false;
        --sp;
        v = base[sp * BLOCK];
        return true;
    }
};

typedef __attribute__((address_space(4))) float ConstFloat;

// a value that is the same in every lane, moved to an SGPR
__device__ __forceinline__ float uniformF(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}
__device__ __forceinline__ uint32_t uniformU(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
#endif

}  // namespace mrx
