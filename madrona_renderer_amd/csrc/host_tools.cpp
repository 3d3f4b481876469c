// The C-ABI entries that take no renderer: asset readers and decoders, the constants, dispatch rules and launch plans
// a test compares against, the BLAS check.  Host work only.
#include "renderer.hpp"

#include "assets.hpp"
#include "boxes.hpp"
#include "rays.hpp"

extern "C" {

int mrx_projection_constants(uint32_t width, uint32_t height, int render_mode, mrx_projection proj, float out[6])
{
    if (!out)
        return fail(MRX_E_INVALID, "null output");
    if (render_mode != MRX_MODE_RASTERIZER && render_mode != MRX_MODE_RAYTRACER)
        return fail(MRX_E_INVALID, "bad render_mode");
    const bool rt = render_mode == MRX_MODE_RAYTRACER;
    mrx::ViewProj c;
    const int rc = projectionConstants(width, rt ? width : height, rt, proj, c);
    if (rc != MRX_OK)
        return rc;
    out[0] = c.sx; out[1] = c.ox; out[2] = c.sz; out[3] = c.oz; out[4] = c.invNear; out[5] = c.s6bPad;
    return MRX_OK;
}

int mrx_light_constants(mrx_light light, float out[5])
{
    if (!out)
        return fail(MRX_E_INVALID, "null output");
    mrx::ViewLight c;
    const int rc = lightConstants(light, c);
    if (rc != MRX_OK)
        return rc;
    out[0] = c.toLight[0]; out[1] = c.toLight[1]; out[2] = c.toLight[2]; out[3] = c.ambient; out[4] = c.diffuse;
    return MRX_OK;
}

int mrx_box_plan(uint32_t views, uint32_t nfast, uint32_t nslow, uint32_t k, uint32_t num_cus, uint32_t forced_parts,
                 int null_pointers)
{
    static const int32_t in = 0;
    static int32_t outCell = 0;             // (never dereferenced: checkBoxes looks at the pointers' values only)
    mrx::BoxParams q {};
    q.ids = null_pointers ? nullptr : &in;
    q.out = null_pointers ? nullptr : &outCell;
    q.numViews = views; q.nfast = nfast; q.nslow = nslow;
    q.K = k;
    q.numCUs = num_cus;
    q.forcedParts = forced_parts;
    if (mrx::checkBoxes(q) != hipSuccess)
        return fail(MRX_E_INVALID, "the box stage refuses these arguments");
    if ((uint64_t)views * nfast * nslow == 0)
        return 0;
    return (int)mrx::boxParts(views, nslow, num_cus, forced_parts);
}

int mrx_cloud_plan(uint32_t views, uint32_t nfast, uint32_t nslow, uint32_t n, uint32_t num_cus, uint32_t forced_parts,
                   int null_pointers, uint32_t out[3])
{
    // (never dereferenced: checkCloud looks at the pointers' values only)
    alignas(16) static float f[4] = {};
    static int32_t i = 0;
    static uint32_t u = 0;
    const uint64_t pxPerView = (uint64_t)nfast * nslow;
    mrx::CloudParams q {};
    if (!null_pointers) {
        q.depth = f;
        q.points = f;
        q.pixel = &i;
        q.count = &i;
        q.scratch = &u;
        q.camPos = q.camRot = f;
    }
    q.scratchCount = (uint64_t)views * mrx::kCloudMaxParts;     // (the renderer sizes the column by the same rule)
    q.numViews = views; q.nfast = nfast; q.nslow = nslow;
    q.N = n;
    q.s = 1; q.half = 0;
    q.frame = 1;
    q.numCUs = num_cus;
    q.forcedParts = forced_parts;
    if (mrx::checkCloud(q) != hipSuccess)
        return fail(MRX_E_INVALID, "the compaction stage refuses these arguments");
    const uint32_t parts = mrx::cloudParts(views, pxPerView, num_cus, forced_parts);
    const uint64_t units = pxPerView * views == 0 ? 0 : (uint64_t)views * parts;
    if (units >= (1ull << 31))
        return fail(MRX_E_INVALID, "the compaction stage refuses these arguments");
    if (out) {
        out[0] = parts;
        out[1] = mrx::kCloudLdsBytes;
        out[2] = mrx::cloudWide(pxPerView, n) ? 1u : 0u;
    }
    return (int)std::min<uint64_t>(units, (uint64_t)num_cus * 4u);
}

int mrx_ray_plan(uint32_t worlds, uint32_t rays_per_world, uint32_t bvh_depth, uint32_t num_cus, uint32_t pass_rows,
                 int null_pointers, uint32_t out[4])
{
    // (never dereferenced: planRays looks at the pointers' values only)
    static float f = 0.0f;
    static int32_t i = 0;
    static uint32_t u = 0;
    mrx::RayParams q {};
    if (!null_pointers) {
        q.s.tris = reinterpret_cast<const mrx::ObjTri *>(&f);
        q.s.nodes = reinterpret_cast<const mrx::BvhNode *>(&f);
        q.s.leafTris = &u;
        q.s.instInfo = reinterpret_cast<const mrx::ObjInfo *>(&f);
        q.s.instKBase = &u;
        q.s.boundObj = &i;
        q.s.worldInstStart = &u;
        q.s.instPos = q.s.instRot = q.s.instScale = &f;
        q.s.instObj = &i;
        q.rays = &f;
        q.frame = &i;
        q.outT = &f;
        q.outId = &i;
    }
    q.numWorlds = worlds;
    q.R = rays_per_world;
    q.bvhDepth = bvh_depth;
    q.numCUs = num_cus;
    q.passRows = pass_rows;
    mrx::RayPlan plan;
    if (mrx::planRays(q, plan) != hipSuccess)
        return fail(MRX_E_INVALID, "the trace stage refuses these arguments");
    if (out) {
        out[0] = plan.blocksPerWorld;
        out[1] = plan.stackEntries;
        out[2] = plan.passRows;
        out[3] = plan.ldsBytes;
    }
    return (int)plan.workgroups;
}

int mrx_shadow_plan(uint32_t views, uint32_t nfast, uint32_t nslow, uint32_t s, uint32_t bvh_depth, uint32_t num_cus,
                    uint32_t pass_rows, int apply, float bias, float max_distance, int bad_pointers, uint32_t out[4])
{
    // (never dereferenced: planShadow looks at the pointers' values only)
    alignas(4) static char bytes[8] = {};
    static float f = 0.0f;
    static int32_t i = 0;
    static uint32_t u = 0;
    static uint8_t b = 0;
    mrx::ShadowParams q {};
    if (bad_pointers != 1) {
        q.s.tris = reinterpret_cast<const mrx::ObjTri *>(&f);
        q.s.nodes = reinterpret_cast<const mrx::BvhNode *>(&f);
        q.s.leafTris = &u;
        q.s.instInfo = reinterpret_cast<const mrx::ObjInfo *>(&f);
        q.s.worldInstStart = &u;
        q.s.instPos = q.s.instRot = q.s.instScale = &f;
        q.s.instObj = &i;
        q.viewWorld = &u;
        q.depth = bad_pointers == 2 ? reinterpret_cast<const float *>(bytes + 1) : &f;
        q.mask = &b;
        q.rgb = bad_pointers == 3 ? reinterpret_cast<uint32_t *>(bytes + 2) : &u;
        q.normal = &u;
        q.camPos = q.camRot = &f;
    }
    q.numViews = views; q.nfast = nfast; q.nslow = nslow;
    q.ss = s; q.half = s / 2;
    q.apply = apply;
    q.bias = bias;
    q.maxDistance = max_distance;
    q.bvhDepth = bvh_depth;
    q.numCUs = num_cus;
    q.passRows = pass_rows;
    mrx::ShadowPlan plan;
    if (mrx::planShadow(q, plan) != hipSuccess)
        return fail(MRX_E_INVALID, "the shadow stage refuses these arguments");
    if (out) {
        out[0] = plan.blocksPerView;
        out[1] = plan.stackEntries;
        out[2] = plan.passRows;
        out[3] = plan.ldsBytes;
    }
    return (int)plan.workgroups;
}

int mrx_load_obj(const char *path, float **tri_pos, float **tri_uv, uint32_t *num_tris)
{
    if (!path || !tri_pos || !tri_uv || !num_tris)
        return fail(MRX_E_INVALID, "null argument");
    mrx::TriSoup soup;
    std::string err;
    if (!mrx::loadOBJ(path, soup, err))
        return fail(MRX_E_ASSET, err);
    *num_tris = soup.numTris();
    *tri_pos = (float *)std::malloc(soup.pos.size() * sizeof(float) + 4);
    *tri_uv = (float *)std::malloc(soup.uv.size() * sizeof(float) + 4);
    std::memcpy(*tri_pos, soup.pos.data(), soup.pos.size() * sizeof(float));
    std::memcpy(*tri_uv, soup.uv.data(), soup.uv.size() * sizeof(float));
    return MRX_OK;
}

int mrx_obj_objects(const char *path, uint32_t *first_tri, uint32_t capacity)
{
    if (!path || (!first_tri && capacity))
        return fail(MRX_E_INVALID, "null argument");
    mrx::TriSoup soup;
    std::string err;
    if (!mrx::loadOBJ(path, soup, err))
        return fail(MRX_E_ASSET, err);
    for (size_t o = 0; o < soup.objStart.size() && o < capacity; ++o)
        first_tri[o] = soup.objStart[o];
    return (int)soup.objStart.size();
}

int mrx_decode_png(const char *path, uint8_t **rgba, uint32_t *width, uint32_t *height)
{
    if (!path || !rgba || !width || !height)
        return fail(MRX_E_INVALID, "null argument");
    mrx::Image img;
    std::string err;
    if (!mrx::decodePNG(path, img, err))
        return fail(MRX_E_ASSET, err);
    *width = img.width;
    *height = img.height;
    *rgba = (uint8_t *)std::malloc(img.rgba.size() + 4);
    std::memcpy(*rgba, img.rgba.data(), img.rgba.size());
    return MRX_OK;
}

int mrx_decode_texture(const char *path, uint8_t **rgba, uint32_t *width, uint32_t *height)
{
    if (!path || !rgba || !width || !height)
        return fail(MRX_E_INVALID, "null argument");
    mrx::Image img;
    std::string err;
    if (!mrx::decodeTexture(path, img, err))
        return fail(MRX_E_ASSET, err);
    *width = img.width;
    *height = img.height;
    *rgba = (uint8_t *)std::malloc(img.rgba.size() + 4);
    std::memcpy(*rgba, img.rgba.data(), img.rgba.size());
    return MRX_OK;
}

int mrx_decode_bc7(const uint8_t *blocks, uint32_t num_blocks, uint8_t *rgba)
{
    if ((!blocks || !rgba) && num_blocks)
        return fail(MRX_E_INVALID, "null argument");
    for (uint32_t b = 0; b < num_blocks; ++b)
        mrx::decodeBC7Block(blocks + 16 * (size_t)b, reinterpret_cast<uint8_t (*)[4]>(rgba + 64 * (size_t)b));
    return MRX_OK;
}

int64_t mrx_describe_obj_materials(const char *path, char *json, uint64_t capacity)
{
    if (!path || !json)
        return fail(MRX_E_INVALID, "null argument");
    mrx::TriSoup soup;
    std::string err;
    if (!mrx::loadOBJ(path, soup, err))
        return fail(MRX_E_ASSET, err);
    auto quote = [](const std::string &s) {
        std::string o = "\"";
        for (char c : s) {
            if (c == '"' || c == '\\') o += '\\';
            o += c;
        }
        return o + "\"";
    };
    std::string out = "{\"num_tris\":" + std::to_string(soup.numTris()) + ",\"tri_mtl\":[";
    for (size_t i = 0; i < soup.triMtl.size(); ++i)
        out += (i ? "," : "") + std::to_string(soup.triMtl[i]);
    out += "],\"names\":[";
    for (size_t i = 0; i < soup.mtlNames.size(); ++i)
        out += (i ? "," : "") + quote(soup.mtlNames[i]);
    out += "],\"libs\":[";
    for (size_t i = 0; i < soup.mtlLibs.size(); ++i)
        out += (i ? "," : "") + quote(soup.mtlLibs[i]);
    out += "],\"materials\":[";
    std::vector<mrx::MtlMaterial> lib;
    for (const std::string &ml : soup.mtlLibs) {
        std::string merr;
        (void)mrx::loadMTL(ml, lib, merr);
    }
    for (size_t i = 0; i < lib.size(); ++i) {
        char kd[96];
        std::snprintf(kd, sizeof kd, "[%.9g,%.9g,%.9g]", lib[i].kd[0], lib[i].kd[1], lib[i].kd[2]);
        out += std::string(i ? "," : "") + "{\"name\":" + quote(lib[i].name) + ",\"kd\":" + kd +
               ",\"map_kd\":" + quote(lib[i].mapKd) + "}";
    }
    out += "]}";
    if (out.size() + 1 > capacity)
        return fail(MRX_E_INVALID, "buffer too small");
    std::memcpy(json, out.c_str(), out.size() + 1);
    return (int64_t)out.size();
}

uint32_t mrx_dispatch_min_tris(uint32_t base, uint32_t num_views, int textured, uint32_t width, uint32_t height,
                               uint32_t num_cus)
{
    return mrx::bvhDispatchMinTris(base ? base : mrx::kBvhMinTris, num_views, textured != 0, width, height, num_cus);
}

uint32_t mrx_group_fill(uint32_t num_cus) { return mrx::groupFill(num_cus); }

int mrx_dispatch_flat(int raytracer, uint32_t num_views, uint32_t width, uint32_t height, uint32_t max_world_triangles,
                      uint32_t max_world_instances, uint32_t num_cus)
{
    // (Raytracer storage is square: res = width)
    return mrx::bvhDispatchFlat(raytracer != 0, num_views, width, raytracer ? width : height, max_world_triangles,
                                max_world_instances, num_cus) ? 1 : 0;
}

int mrx_group_plan(const mrx_group_plan_in *in, mrx_group_plan_t *out)
{
    if (!in || !out)
        return fail(MRX_E_INVALID, "null argument");
    if (in->max_world_triangles > 256u)
        return fail(MRX_E_INVALID, "the group kernel renders worlds of at most 256 triangles");
    if (in->uni_instances > 4u)
        return fail(MRX_E_INVALID, "uniform worlds have at most 4 instances");
    if (in->group_views < 0 || in->group_tiles < 0 || in->debug_slots < 0 || in->xcd_skew < -1 || in->xcd_rotate < -1)
        return fail(MRX_E_INVALID, "override out of range");
    // (never dereferenced: groupPlan looks at the pointers' values only)
    static const char block = 0;
    static uint32_t word = 0;
    static unsigned long long stamp = 0;
    mrx::RasterParams p {};
    p.numViews = in->views; p.nfast = in->nfast; p.nslow = in->nslow;
    p.tilesFast = (in->nfast + 63u) / 64u;
    p.tilesSlow = (in->nslow + 63u) / 64u;
    p.anyTextured = in->textured != 0;
    p.numCUs = in->num_cus;
    p.uniInstances = in->uni_instances;
    p.uniCamsPerWorld = in->uni_cams_per_world;
    std::memcpy(p.uniPrefix, in->uni_prefix, sizeof p.uniPrefix);
    std::memcpy(p.uniFirstTri, in->uni_first_tri, sizeof p.uniFirstTri);
    p.poseBlock = p.geomBlock = in->has_blocks ? &block : nullptr;
    // (any non-zero value is "on": 2 the stamps alone, every other value a MRX_DEBUG_SKIP switch, with bit 1 the stamps too)
    p.debugSkip = (in->diagnostics & ~2) ? 1u : 0u;
    p.debugStamps = (in->diagnostics & 2) ? &stamp : nullptr;
    p.grpViewsWanted = in->group_views;
    p.grpTilesWanted = in->group_tiles;
    p.xcdSkewWanted = in->xcd_skew;
    p.xcdRotateWanted = in->xcd_rotate;
    p.debugSlots = in->debug_slots;
    p.xcdPhase = in->xcd_phase;
    p.xccReport = in->has_report ? &word : nullptr;
    *out = mrx_group_plan_t {};
    if ((uint64_t)p.numViews * p.tilesFast * p.tilesSlow == 0)
        return MRX_ENTRY_NONE;
    const mrx::GroupPlan plan = mrx::groupPlan(p, in->max_world_triangles, in->fast_allowed != 0);
    out->slots = plan.slots;
    out->group_views = plan.grpViews;
    out->chunk_tiles = plan.grpChunkTiles;
    out->groups_per_view = plan.grpPerView;
    out->workgroups = plan.workgroups;
    out->threads = plan.threads;
    out->xcd_skew = plan.xcdSkew;
    out->xcd_rotate = plan.xcdRotate;
    out->xmode = plan.xmode;
    out->fast = plan.fast ? 1 : 0;
    out->shape = plan.header.shape;
    out->prefix = plan.header.prefix;
    out->first01 = plan.header.first01;
    out->first23 = plan.header.first23;
    return plan.fast ? MRX_ENTRY_GROUP_FAST : MRX_ENTRY_GROUP;
}

int mrx_blas_check(const float *tri_pos, uint32_t num_tris, uint32_t *num_nodes, uint32_t *depth,
                   uint32_t *num_leaves)
{
    if ((!tri_pos && num_tris) || !num_nodes || !depth || !num_leaves)
        return fail(MRX_E_INVALID, "null argument");
    using namespace mrx;
    std::vector<ObjTri> tris(num_tris);
    for (uint32_t t = 0; t < num_tris; ++t)
        std::memcpy(tris[t].p, tri_pos + 9 * (size_t)t, 36);
    BlasSet b;
    buildBlas(tris.data(), { 0 }, { (int32_t)num_tris }, b);
    *num_nodes = (uint32_t)b.nodes.size();
    *depth = b.maxDepth;
    *num_leaves = 0;
    const ObjInfo &o = b.objects[0];
    if (o.root < 0)
        return num_tris <= kBvhFlatMax && b.nodes.empty() ? MRX_OK
                                                          : fail(MRX_E_INVALID, "large object without a hierarchy");
    if (1 + 7 * b.maxDepth > kBvhStackCap)
        return fail(MRX_E_INVALID, "hierarchy too deep for the traversal stack");
    std::vector<uint32_t> seen(num_tris, 0);
    // (node, box that must contain everything below it)
    struct Item { uint32_t node; float lo[3], hi[3]; };
    std::vector<Item> todo;
    {
        Item root {};
        root.node = (uint32_t)o.root;
        std::memcpy(root.lo, o.bbMin, 12);
        std::memcpy(root.hi, o.bbMax, 12);
        todo.push_back(root);
    }
    while (!todo.empty()) {
        const Item it = todo.back();
        todo.pop_back();
        if (it.node >= b.nodes.size())
            return fail(MRX_E_INVALID, "child index out of range");
        const BvhNode &n = b.nodes[it.node];
        for (uint32_t c = 0; c < kBvhWidth; ++c) {
            const uint32_t ref = n.child[c];
            if (ref == kBvhEmpty)
                continue;
            for (int a = 0; a < 3; ++a)
                if (n.bmin[c][a] < it.lo[a] || n.bmax[c][a] > it.hi[a])
                    return fail(MRX_E_INVALID, "child box sticks out of its parent's");
            if (ref & kBvhLeafBit) {
                const uint32_t cnt = ((ref >> kBvhLeafStartBits) & 15u) + 1u;
                const uint32_t start = ref & ((1u << kBvhLeafStartBits) - 1u);
                if (cnt > kBvhLeafMax || start + cnt > b.leafTris.size())
                    return fail(MRX_E_INVALID, "bad leaf");
                ++*num_leaves;
                for (uint32_t i = 0; i < cnt; ++i) {
                    const uint32_t t = b.leafTris[start + i];
                    if (t >= num_tris || seen[t]++)
                        return fail(MRX_E_INVALID, "triangle missing from or repeated in the leaves");
                    for (int v = 0; v < 3; ++v)
                        for (int a = 0; a < 3; ++a) {
                            const float x = tris[t].p[3 * v + a];
                            if (x < n.bmin[c][a] || x > n.bmax[c][a])
                                return fail(MRX_E_INVALID, "triangle outside its leaf's box");
                        }
                }
            } else {
                Item ch {};
                ch.node = ref;
                std::memcpy(ch.lo, n.bmin[c], 12);
                std::memcpy(ch.hi, n.bmax[c], 12);
                todo.push_back(ch);
            }
        }
    }
    for (uint32_t t = 0; t < num_tris; ++t)
        if (seen[t] != 1)
            return fail(MRX_E_INVALID, "triangle missing from the leaves");
    return MRX_OK;
}

void mrx_free(void *p) { std::free(p); }

}  // extern "C"
