// The shadow stage on the CPU: shadow_core.hpp run over host arrays in the kernel's own structure
// -- view by view, the rows of the view's world staged pass by pass, every pixel walked over the staged rows.  Host code
// only -- no HIP call, no device -- so that tests can hold the kernel's source against tests/shadow_oracle.py without a
// GPU and a sanitizer build can run it (shadow_host_driver.cpp).
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/mrx.h"
#include "rays.hpp"
#include "shadow.hpp"

namespace mrx {

void shadowHost(const ShadowParams &p)
{
    const uint64_t pxPerView = (uint64_t)p.nfast * p.nslow;
    if (pxPerView * p.numViews == 0)
        return;
    const uint32_t passRows = p.passRows ? std::min(p.passRows, kShadowPassRows) : kShadowPassRows;
    const float proj[4] = { p.sx, p.ox, p.sz, p.oz };
    const float light[5] = { p.toLight[0], p.toLight[1], p.toLight[2], p.ambient, p.diffuse };
    std::vector<ShadowRow> rows(passRows);
    std::vector<uint8_t> occluded((size_t)pxPerView);
    for (uint32_t view = 0; view < p.numViews; ++view) {
        const uint32_t world = p.viewWorld[view];
        const uint32_t rowLo = p.s.worldInstStart[world], rowHi = p.s.worldInstStart[world + 1];
        const CloudView cv = cloudLoadView<true>(p.camRot, p.camPos, p.viewProj, proj, view);
        const ShadowLight lt = shadowLoadLight(p.viewLight, light, view);
        const float *depth = p.depth + (size_t)view * pxPerView;
        std::fill(occluded.begin(), occluded.end(), (uint8_t)0);
        const auto rayOf = [&](uint64_t pix) {
            const uint32_t slow = (uint32_t)(pix / p.nfast), fast = (uint32_t)(pix - (uint64_t)slow * p.nfast);
            const uint32_t x = p.transposed ? slow : fast, y = p.transposed ? fast : slow;
            return shadowRay(cv, p.ss, p.half, x, y, depth[pix], lt.toLight, p.bias, p.maxDistance);
        };
        for (uint32_t base = rowLo; base < rowHi; base += passRows) {
            const uint32_t n = std::min(passRows, rowHi - base);
            for (uint32_t i = 0; i < n; ++i)
                shadowStageRow(base + i, p.s, lt.toLight, rows[i]);
            for (uint64_t pix = 0; pix < pxPerView; ++pix) {
                if (!shadowHit(depth[pix]) || (!p.brute && occluded[pix]))
                    continue;
                const Ray ray = rayOf(pix);
                if (!p.brute && rayDegenerate(ray))
                    continue;
                for (uint32_t i = 0; i < n; ++i) {
                    HostStack stack;
                    if (shadowRowOccludes(rows[i], p.s, ray, p.brute != 0, stack)) {
                        occluded[pix] = 1;
                        if (!p.brute)
                            break;
                    }
                }
            }
        }
        for (uint64_t pix = 0; pix < pxPerView; ++pix) {
            const size_t item = (size_t)view * pxPerView + pix;
            const bool dark = shadowHit(depth[pix]) && occluded[pix];
            p.mask[item] = dark ? (uint8_t)0 : (uint8_t)255;
            if (p.apply && dark) {
                float Rc[9], lv[3];
                quatRotation(p.camRot + 4 * (size_t)view, Rc);
                rotateT(Rc, lt.toLight, lv);
                p.rgb[item] = shadowApply(p.rgb[item], p.normal[item], lv, lt.ambient, lt.diffuse);
            }
        }
    }
}

}  // namespace mrx

extern "C" int mrx_shadow_host(const float *tri_pos, uint32_t num_tris, const int32_t *obj_first,
                               const int32_t *obj_count, uint32_t num_objects, const mrx_instance *instances,
                               uint32_t num_instances, const uint32_t *world_inst_start, uint32_t num_worlds,
                               const float *depth, uint32_t views, uint32_t nfast, uint32_t nslow, int transposed,
                               uint32_t s, const float *consts, const float *cam_pos, const float *cam_rot,
                               const uint32_t *view_world, const float *lights, float bias, float max_distance,
                               uint32_t pass_rows, int brute, uint32_t *rgb_or_null, const uint32_t *normal_or_null,
                               uint8_t *out_mask)
{
    using namespace mrx;
    const uint64_t pxPerView = (uint64_t)nfast * nslow;
    if (pxPerView * views == 0)
        return MRX_OK;
    if (!consts || !lights || !view_world || (rgb_or_null != nullptr) != (normal_or_null != nullptr))
        return MRX_E_INVALID;
    for (uint32_t v = 0; v < views; ++v)
        if (view_world[v] >= num_worlds)
            return MRX_E_INVALID;
    RayHostScene g;
    if (const int rc = rayHostScene(tri_pos, num_tris, obj_first, obj_count, num_objects, instances, num_instances,
                                    world_inst_start, num_worlds, g))
        return rc;
    // per-view constants and lights as the device tables hold them
    std::vector<ViewProj> proj(views);
    std::vector<ViewLight> light(views);
    for (uint32_t v = 0; v < views; ++v) {
        std::memset(&proj[v], 0, sizeof(ViewProj));
        std::memcpy(&proj[v], consts + 4 * (size_t)v, 16);
        std::memset(&light[v], 0, sizeof(ViewLight));
        std::memcpy(&light[v], lights + 5 * (size_t)v, 20);
    }
    ShadowParams p {};
    p.s = g.tables;
    p.viewWorld = view_world;
    p.depth = depth;
    p.mask = out_mask;
    p.rgb = rgb_or_null;
    p.normal = normal_or_null;
    p.camPos = cam_pos;
    p.camRot = cam_rot;
    p.viewProj = proj.data();
    p.viewLight = light.data();
    p.numViews = views;
    p.nfast = nfast;
    p.nslow = nslow;
    p.ss = s;
    p.half = s / 2;
    p.transposed = transposed;
    p.apply = rgb_or_null ? 1 : 0;
    p.bias = bias;
    p.maxDistance = max_distance;
    p.bvhDepth = g.blas.maxDepth;
    p.numCUs = 1;
    p.passRows = pass_rows;
    p.brute = brute;
    ShadowPlan plan;
    if (planShadow(p, plan) != hipSuccess)
        return MRX_E_INVALID;
    shadowHost(p);
    return MRX_OK;
}
