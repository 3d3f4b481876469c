// The trace stage of a renderer with a ray-cast sensor: caller-supplied rays, R per world, traced
// through the world's instance rows -- the ObjTri pool, the per-object BLAS, the per-row ObjInfo table and the live pose,
// scale, ObjectID and label columns, as the render kernels read them.  Per ray the parameter t of the nearest hit (the
// ray's own tmax on a miss) and the segmask value of the row that was hit (-1 on a miss).  One kernel per step, last on
// the render's stream (rays.hip); the arithmetic is rays_core.hpp's, shared with the host entry.
#pragma once

#include <cstdint>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../include/mrx.h"
#include "rays_core.hpp"

namespace mrx {

struct RayParams {
    RayTables s;
    const float *rays;              // [worlds][R][8]: (ox, oy, oz, tmin, dx, dy, dz, tmax)
    const int32_t *frame;           // [worlds]: world-local mount row, anything outside 0 ... n_w - 1 = world frame
    float *outT;                    // [worlds][R]
    int32_t *outId;                 // [worlds][R]
    uint32_t numWorlds, R;
    uint32_t bvhDepth;              // deepest BLAS of the scene: the traversal stack holds 1 + 7 * depth entries
    uint32_t numCUs;
    uint32_t passRows;              // MRX_RAY_PASS_ROWS; 0: kRayPassRows
    int32_t brute;                  // MRX_RAYS_BRUTE=1: the form without any cull
};

// What launchRays would launch (host only, no HIP call).
struct RayPlan {
    uint32_t blocksPerWorld, workgroups;
    uint32_t stackEntries, passRows;
    uint32_t ldsBytes;              // dynamic LDS: the traversal stacks
};

// hipErrorInvalidValue for R outside 1 ... kRayMaxPerWorld, worlds * R >= 2^31, a null pointer, no CU or a BLAS deeper
// than kBvhStackCap allows; otherwise the plan (workgroups == 0: zero worlds, nothing to enqueue).
hipError_t planRays(const RayParams &p, RayPlan &plan);

// Once per device, with the device current, before the first launch there (mrx_rays_create): lets the kernels take the
// dynamic LDS the deepest traversal stack needs.
hipError_t prepareRays();

// Enqueues the stage on `stream`: nothing for zero rays, one kernel otherwise.
hipError_t launchRays(const RayParams &p, hipStream_t stream);

// The same source on the CPU, ray by ray (mrx_trace_rays_host): no device is touched.
void traceRaysHost(const RayParams &p);

// What the host entries (mrx_trace_rays_host, mrx_shadow_host) make of the geometry a caller hands them: the pool, the
// BLAS buildBlas gives it, the columns and per-row tables as bindGeometry lays them out, and `tables` pointing at them
// (instLabel null).  MRX_E_INVALID for ranges that do not fit, MRX_E_UNSUPPORTED for a BLAS deeper than the stack.
struct RayHostScene {
    std::vector<ObjTri> tris;
    BlasSet blas;
    std::vector<float> pos, rot, scale;
    std::vector<int32_t> obj, bound;
    std::vector<uint32_t> kBase;
    std::vector<ObjInfo> info;
    RayTables tables;
};
int rayHostScene(const float *tri_pos, uint32_t num_tris, const int32_t *obj_first, const int32_t *obj_count,
                 uint32_t num_objects, const mrx_instance *instances, uint32_t num_instances,
                 const uint32_t *world_inst_start, uint32_t num_worlds, RayHostScene &g);

}  // namespace mrx
