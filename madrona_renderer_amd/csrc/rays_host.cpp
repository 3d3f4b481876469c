// The ray-cast sensor on the CPU: rays_core.hpp run ray by ray over host arrays.  Host code only --
// no HIP call, no device -- so that tests can hold the kernel's source against tests/ray_oracle.py without a GPU and a
// sanitizer build can run it (rays_host_driver.cpp).
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/mrx.h"
#include "rays.hpp"

namespace mrx {

void traceRaysHost(const RayParams &p)
{
    std::vector<RayRow> rows;
    for (uint32_t w = 0; w < p.numWorlds; ++w) {
        const uint32_t rowLo = p.s.worldInstStart[w], rowHi = p.s.worldInstStart[w + 1];
        rows.resize(rowHi - rowLo);
        for (uint32_t row = rowLo; row < rowHi; ++row)
            rayStageRow(row, p.s, rows[row - rowLo]);
        for (uint32_t i = 0; i < p.R; ++i) {
            const size_t slot = (size_t)w * p.R + i;
            const float *in = p.rays + 8 * slot;
            const Ray ray = rayFromFrame(in, p.frame ? p.frame[w] : -1, rowLo, rowHi, p.s);
            RayBest best { 0.0f, kRayNoHit, -1 };
            const bool dead = !p.brute && rayDegenerate(ray);
            for (const RayRow &row : rows) {
                if (dead)
                    break;
                HostStack stack;
                rayRow(row, p.s, ray, p.brute != 0, stack, best);
            }
            if (best.k == kRayNoHit) {
                std::memcpy(p.outT + slot, in + 7, sizeof(float));      // tmax as given, NaN payload included
                p.outId[slot] = -1;
            } else {
                p.outT[slot] = best.t;
                p.outId[slot] = best.id;
            }
        }
    }
}

}  // namespace mrx

namespace mrx {

int rayHostScene(const float *tri_pos, uint32_t num_tris, const int32_t *obj_first, const int32_t *obj_count,
                 uint32_t num_objects, const mrx_instance *instances, uint32_t num_instances,
                 const uint32_t *world_inst_start, uint32_t num_worlds, RayHostScene &g)
{
    if (!world_inst_start || (num_tris && !tri_pos) || (num_objects && (!obj_first || !obj_count)) ||
        (num_instances && !instances))
        return MRX_E_INVALID;
    std::vector<int32_t> first(num_objects), count(num_objects);
    for (uint32_t o = 0; o < num_objects; ++o) {
        if (obj_first[o] < 0 || obj_count[o] < 0 || (uint64_t)obj_first[o] + (uint64_t)obj_count[o] > num_tris)
            return MRX_E_INVALID;
        first[o] = obj_first[o];
        count[o] = obj_count[o];
    }
    for (uint32_t w = 0; w < num_worlds; ++w)
        if (world_inst_start[w] > world_inst_start[w + 1] || world_inst_start[w + 1] > num_instances)
            return MRX_E_INVALID;
    g.tris.resize(num_tris);
    for (uint32_t t = 0; t < num_tris; ++t) {
        std::memset(&g.tris[t], 0, sizeof(ObjTri));
        std::memcpy(g.tris[t].p, tri_pos + 9 * (size_t)t, sizeof g.tris[t].p);
        g.tris[t].mat = -1;
    }
    buildBlas(g.tris.data(), first, count, g.blas);
    if (1u + 7u * g.blas.maxDepth > kBvhStackCap)
        return MRX_E_UNSUPPORTED;
    // the columns and per-row tables as bindGeometry lays them out: a row draws the object its id names
    const size_t n = num_instances;
    g.pos.assign(3 * n + 1, 0.0f); g.rot.assign(4 * n + 1, 0.0f); g.scale.assign(3 * n + 1, 0.0f);
    g.obj.assign(n + 1, 0); g.bound.assign(n + 1, 0);
    g.kBase.assign(n + 1, 0u);
    g.info.assign(n + 1, ObjInfo {});
    for (size_t i = 0; i < n; ++i) {
        std::memcpy(&g.pos[3 * i], instances[i].position, 12);
        std::memcpy(&g.rot[4 * i], instances[i].rotation, 16);
        std::memcpy(&g.scale[3 * i], instances[i].scale, 12);
        g.obj[i] = g.bound[i] = instances[i].object_id;
        ObjInfo oi {};
        oi.root = -1;
        if (g.obj[i] >= 0 && (uint32_t)g.obj[i] < num_objects)
            oi = g.blas.objects[g.obj[i]];
        g.info[i] = oi;
    }
    for (uint32_t w = 0; w < num_worlds; ++w) {
        uint32_t k = 0;
        for (uint32_t row = world_inst_start[w]; row < world_inst_start[w + 1]; ++row) {
            g.kBase[row] = k;
            k += g.info[row].numTris;
        }
    }
    g.tables = RayTables {};
    g.tables.tris = g.tris.data();
    g.tables.nodes = g.blas.nodes.data();
    g.tables.leafTris = g.blas.leafTris.data();
    g.tables.instInfo = g.info.data();
    g.tables.instKBase = g.kBase.data();
    g.tables.boundObj = g.bound.data();
    g.tables.worldInstStart = world_inst_start;
    g.tables.instPos = g.pos.data();
    g.tables.instRot = g.rot.data();
    g.tables.instScale = g.scale.data();
    g.tables.instObj = g.obj.data();
    return MRX_OK;
}

}  // namespace mrx

extern "C" int mrx_trace_rays_host(const float *tri_pos, uint32_t num_tris, const int32_t *obj_first,
                                   const int32_t *obj_count, uint32_t num_objects, const mrx_instance *instances,
                                   uint32_t num_instances, const int32_t *labels_or_null,
                                   const uint32_t *world_inst_start, uint32_t num_worlds, const int32_t *frame_or_null,
                                   const float *rays, uint32_t rays_per_world, int brute, float *out_t, int32_t *out_id)
{
    using namespace mrx;
    if (rays_per_world < 1 || rays_per_world > kRayMaxPerWorld || (uint64_t)num_worlds * rays_per_world >= (1ull << 31))
        return MRX_E_INVALID;
    if (!rays || !out_t || !out_id)
        return MRX_E_INVALID;
    RayHostScene g;
    if (const int rc = rayHostScene(tri_pos, num_tris, obj_first, obj_count, num_objects, instances, num_instances,
                                    world_inst_start, num_worlds, g))
        return rc;
    RayParams p {};
    p.s = g.tables;
    p.s.instLabel = labels_or_null;
    p.rays = rays;
    p.frame = frame_or_null;
    p.outT = out_t;
    p.outId = out_id;
    p.numWorlds = num_worlds;
    p.R = rays_per_world;
    p.bvhDepth = g.blas.maxDepth;
    p.numCUs = 1;
    p.brute = brute;
    traceRaysHost(p);
    return MRX_OK;
}
