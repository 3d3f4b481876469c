// The shadow stage of a renderer with cast shadows: per native pixel of the depth tensor the
// caller sees one any-hit ray from the pixel's world point towards the light of the view's world, through the rows of
// that world -- the ObjTri pool, the per-object BLAS, the per-row ObjInfo table and the live pose, scale and ObjectID
// columns, as the trace stage reads them.  It writes a u8 mask (0 occluded, 255 otherwise) and, in its applying form,
// darkens the rgb of occluded pixels to the ambient term.  One kernel per step behind the unprojection on the render's
// stream (shadow.hip); the arithmetic is shadow_core.hpp's, shared with the host entry.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>

#include <hip/hip_runtime_api.h>

#include "shadow_core.hpp"

namespace mrx {

struct ShadowParams {
    RayTables s;                    // boundObj, instKBase and instLabel are not read
    const uint32_t *viewWorld;      // [views]
    const float *depth;             // [views][nslow][nfast], native
    uint8_t *mask;                  // [views][nslow][nfast]
    uint32_t *rgb;                  // apply: [views][nslow][nfast] packed pixels, native, 4-byte aligned
    const uint32_t *normal;         // apply: the same of the normal tensor
    const float *camPos;            // [views][3]
    const float *camRot;            // [views][4] w, x, y, z
    const ViewProj *viewProj;       // [views], or null: the uniform constants below
    float sx, ox, sz, oz;
    const ViewLight *viewLight;     // [views], or null: the uniform light below
    float toLight[3], ambient, diffuse;
    uint32_t numViews, nfast, nslow;
    uint32_t ss, half;              // supersampling factor (1 without) and ss / 2
    int32_t transposed;             // Raytracer-mode [x][y] storage
    int32_t apply;                  // darken rgb (needs rgb and normal)
    float bias, maxDistance;
    uint32_t bvhDepth;              // deepest BLAS of the scene: the traversal stack holds 1 + 7 * depth entries
    uint32_t numCUs;
    uint32_t passRows;              // MRX_SHADOW_PASS_ROWS; 0: kShadowPassRows
    int32_t brute;                  // MRX_SHADOW_BRUTE=1: the form without any cull
};

// What launchShadow would launch (host only, no HIP call).
struct ShadowPlan {
    uint32_t blocksPerView, workgroups;
    uint32_t stackEntries, passRows;
    uint32_t ldsBytes;              // dynamic LDS: the traversal stacks
};

// how many native pixels the stage can address
constexpr uint64_t kShadowMaxPixels = 0xFFFFFFFFull;

// hipErrorInvalidValue for a null or misaligned tensor, more than kShadowMaxPixels native pixels (or so many that
// the workgroups pass 2^31 - 1), s outside 1 ... 4, a BLAS deeper than kBvhStackCap allows, no CU, a bias that is not
// finite and >= 0 or a max_distance that is neither FLT_MAX nor finite and > 0; otherwise the plan (workgroups == 0:
// no pixel, nothing to enqueue).
inline hipError_t planShadow(const ShadowParams &p, ShadowPlan &plan)
{
    plan = ShadowPlan {};
    const uint64_t pxPerView = (uint64_t)p.nfast * p.nslow, px = pxPerView * p.numViews;
    if (px > kShadowMaxPixels || p.numCUs == 0 || p.ss < 1 || p.ss > 4 || p.half != p.ss / 2)
        return hipErrorInvalidValue;
    if (!(std::isfinite(p.bias) && p.bias >= 0.0f) || !(std::isfinite(p.maxDistance) && p.maxDistance > 0.0f))
        return hipErrorInvalidValue;
    const auto aligned4 = [](const void *q) { return (reinterpret_cast<uintptr_t>(q) & 3u) == 0; };
    if (!p.depth || !aligned4(p.depth) || !p.mask || !p.viewWorld || !p.camPos || !p.camRot || !p.s.tris ||
        !p.s.instInfo || !p.s.worldInstStart || !p.s.instPos || !p.s.instRot || !p.s.instScale || !p.s.instObj)
        return hipErrorInvalidValue;
    if (p.apply && (!p.rgb || !aligned4(p.rgb) || !p.normal || !aligned4(p.normal)))
        return hipErrorInvalidValue;
    const uint32_t entries = 1u + 7u * p.bvhDepth;
    if (p.bvhDepth > kBvhStackCap || entries > kBvhStackCap)
        return hipErrorInvalidValue;
    if (p.bvhDepth && (!p.s.nodes || !p.s.leafTris))
        return hipErrorInvalidValue;
    const uint64_t blocksPerView = (pxPerView + kShadowBlock - 1u) / kShadowBlock;
    if (blocksPerView * p.numViews >= (1ull << 31))
        return hipErrorInvalidValue;
    plan.blocksPerView = (uint32_t)blocksPerView;
    plan.workgroups = px ? (uint32_t)(blocksPerView * p.numViews) : 0u;
    plan.stackEntries = entries;
    plan.passRows = p.passRows ? std::min(p.passRows, kShadowPassRows) : kShadowPassRows;
    plan.ldsBytes = entries * kShadowBlock * 4u;
    return hipSuccess;
}

// Once per device, with the device current, before the first launch there (mrx_shadow_create): lets the kernels take
// the dynamic LDS the deepest traversal stack needs.
hipError_t prepareShadow();

// Enqueues the stage on `stream`: nothing for zero pixels, one kernel otherwise.
hipError_t launchShadow(const ShadowParams &p, hipStream_t stream);

// The same source on the CPU, pixel by pixel (mrx_shadow_host): no device is touched.
void shadowHost(const ShadowParams &p);

}  // namespace mrx
