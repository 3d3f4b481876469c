// The ray-cast sensor on the CPU: rays_core.hpp run ray by ray over host arrays.  Host code only --
// no HIP call, no device -- so that tests can hold the kernel's source against tests/ray_oracle.py without a GPU and a
// sanitizer build can run it (rays_host_driver.cpp).
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/mrx.h"
#include "rays.hpp"

namespace mrx {

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

extern "C" int mrx_trace_rays_host(const float *tri_pos, uint32_t num_tris, const int32_t *obj_first,
                                   const int32_t *obj_count, uint32_t num_objects, const mrx_instance *instances,
                                   uint32_t num_instances, const int32_t *labels_or_null,
                                   const uint32_t *world_inst_start, uint32_t num_worlds, const int32_t *frame_or_null,
                                   const float *rays, uint32_t rays_per_world, int brute, float *out_t, int32_t *out_id)
{
    using namespace mrx;
    if (rays_per_world < 1 || rays_per_world > kRayMaxPerWorld || (uint64_t)num_worlds * rays_per_world >= (1ull << 31))
        return MRX_E_INVALID;
    if (!world_inst_start || !rays || !out_t || !out_id || (num_tris && !tri_pos) ||
        (num_objects && (!obj_first || !obj_count)) || (num_instances && !instances))
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
    std::vector<ObjTri> tris(num_tris);
    for (uint32_t t = 0; t < num_tris; ++t) {
        std::memset(&tris[t], 0, sizeof(ObjTri));
        std::memcpy(tris[t].p, tri_pos + 9 * (size_t)t, sizeof tris[t].p);
        tris[t].mat = -1;
    }
    BlasSet blas;
    buildBlas(tris.data(), first, count, blas);
    if (1u + 7u * blas.maxDepth > kBvhStackCap)
        return MRX_E_UNSUPPORTED;
    // the columns and per-row tables as bindGeometry lays them out: a row draws the object its id names
    const size_t n = num_instances;
    std::vector<float> pos(3 * n + 1), rot(4 * n + 1), scale(3 * n + 1);
    std::vector<int32_t> obj(n + 1), bound(n + 1);
    std::vector<uint32_t> kBase(n + 1, 0);
    std::vector<ObjInfo> info(n + 1);
    for (size_t i = 0; i < n; ++i) {
        std::memcpy(&pos[3 * i], instances[i].position, 12);
        std::memcpy(&rot[4 * i], instances[i].rotation, 16);
        std::memcpy(&scale[3 * i], instances[i].scale, 12);
        obj[i] = bound[i] = instances[i].object_id;
        ObjInfo oi {};
        oi.root = -1;
        if (obj[i] >= 0 && (uint32_t)obj[i] < num_objects)
            oi = blas.objects[obj[i]];
        info[i] = oi;
    }
    for (uint32_t w = 0; w < num_worlds; ++w) {
        uint32_t k = 0;
        for (uint32_t row = world_inst_start[w]; row < world_inst_start[w + 1]; ++row) {
            kBase[row] = k;
            k += info[row].numTris;
        }
    }
    RayParams p {};
    p.s.tris = tris.data();
    p.s.nodes = blas.nodes.data();
    p.s.leafTris = blas.leafTris.data();
    p.s.instInfo = info.data();
    p.s.instKBase = kBase.data();
    p.s.boundObj = bound.data();
    p.s.worldInstStart = world_inst_start;
    p.s.instPos = pos.data();
    p.s.instRot = rot.data();
    p.s.instScale = scale.data();
    p.s.instObj = obj.data();
    p.s.instLabel = labels_or_null;
    p.rays = rays;
    p.frame = frame_or_null;
    p.outT = out_t;
    p.outId = out_id;
    p.numWorlds = num_worlds;
    p.R = rays_per_world;
    p.bvhDepth = blas.maxDepth;
    p.numCUs = 1;
    p.brute = brute;
    traceRaysHost(p);
    return MRX_OK;
}
