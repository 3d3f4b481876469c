// Scene ingestion and world assembly (mrx_create): the view and light constants, the object pool and its BLAS, the
// geometry binding and its dispatch decisions, the per-view tables.
#include "renderer.hpp"

#include <array>
#include <map>
#include <utility>

#include "assets.hpp"

// Build-defined constants of the rendering spec.
constexpr double kVfovDeg = 90.0;      // /root/reference/src/sim.cpp:170
constexpr float kRasterZNear = 0.001f; // /root/reference/src/sim.cpp:170
constexpr float kRtZNear = 0.1f;       // /root/reference/src/mgr.cpp:477
constexpr float kRtZFar = 1000.f;      // /root/reference/src/mgr.cpp:478

// DESIGN.md S5 for one projection (mrx_projection_constants): checks it and works out the view constants in double,
// rounded once to float, in the order the oracle uses (oracle.projection_constants).  H is the height as rendered
// (Raytracer mode: = W).  `resolved` receives the projection with the mode's default znear filled in.
int projectionConstants(uint32_t W, uint32_t H, bool rt, const mrx_projection &in, mrx::ViewProj &out,
                        mrx_projection *resolved)
{
    if (!(std::isfinite(in.vfov_deg) && in.vfov_deg > 0.0f && in.vfov_deg < 180.0f))
        return fail(MRX_E_INVALID, "vfov_deg " + std::to_string(in.vfov_deg) + " is not in (0, 180)");
    const float znear = in.znear == 0.0f ? (rt ? kRtZNear : kRasterZNear) : in.znear;
    if (!(std::isfinite(znear) && znear > 0.0f))
        return fail(MRX_E_INVALID, "znear " + std::to_string(in.znear) + " is not > 0");
    if (rt && !(znear < kRtZFar))
        return fail(MRX_E_INVALID, "znear " + std::to_string(in.znear) + " is not below the Raytracer far plane (1000)");
    if (W == 0 || H == 0)
        return fail(MRX_E_INVALID, "bad view size");
    const float th = (float)std::tan((double)in.vfov_deg * M_PI / 360.0);
    const double asp = (double)W / (double)H;
    out.sx = (float)(2.0 * (double)th * asp / (double)W);
    out.ox = (float)((1.0 / (double)W - 1.0) * (double)th * asp);
    out.sz = (float)(-2.0 * (double)th / (double)H);
    out.oz = (float)((1.0 - 1.0 / (double)H) * (double)th);
    out.invNear = 1.0f / znear;
    // S6b pad: a surface point nearer than znear along +Y that still projects
    // into the image lies within znear * |longest ray| of the eye
    out.s6bPad = (float)((double)znear * std::sqrt(1.0 + (double)th * (double)th * (1.0 + asp * asp)) * 1.001);
    out.pad[0] = out.pad[1] = 0.0f;
    if (resolved)
        *resolved = mrx_projection{ in.vfov_deg, znear };
    return MRX_OK;
}
// the light every world has unless it is given one (mgr.cpp:357; S7's constants).  The reference's direction is
// written in double, and -0.05 is not a float: resolved from its float rounding, the z component of the unit vector
// comes out one ulp off.  A light whose direction equals the float rounding of the default IS the default
// (lightConstants resolves it from the doubles), so that the default given explicitly keeps every bit.
constexpr double kLightDir[3] = { 1.0, -1.0, -0.05 };
constexpr mrx_light kDefaultLight = { { (float)kLightDir[0], (float)kLightDir[1], (float)kLightDir[2] }, 0.25f, 0.75f };

// DESIGN.md S4 / S7 for one light (mrx_light_constants): checks it and resolves the unit vector towards the light in
// double, rounded once to float, in the order the oracle uses (oracle.to_light_vector).
int lightConstants(const mrx_light &in, mrx::ViewLight &out)
{
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(in.direction[c]))
            return fail(MRX_E_INVALID, "light direction is not finite");
    if (in.direction[0] == 0.0f && in.direction[1] == 0.0f && in.direction[2] == 0.0f)
        return fail(MRX_E_INVALID, "light direction is zero");
    if (!(std::isfinite(in.ambient) && in.ambient >= 0.0f))
        return fail(MRX_E_INVALID, "light ambient " + std::to_string(in.ambient) + " is not a finite value >= 0");
    if (!(std::isfinite(in.diffuse) && in.diffuse >= 0.0f))
        return fail(MRX_E_INVALID, "light diffuse " + std::to_string(in.diffuse) + " is not a finite value >= 0");
    double d[3] = { (double)in.direction[0], (double)in.direction[1], (double)in.direction[2] };
    if (in.direction[0] == kDefaultLight.direction[0] && in.direction[1] == kDefaultLight.direction[1] &&
        in.direction[2] == kDefaultLight.direction[2])
        for (int c = 0; c < 3; ++c)
            d[c] = kLightDir[c];
    const double ln = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    for (int c = 0; c < 3; ++c)
        out.toLight[c] = (float)(-d[c] / ln);
    out.ambient = in.ambient;
    out.diffuse = in.diffuse;
    out.pad[0] = out.pad[1] = out.pad[2] = 0.0f;
    return MRX_OK;
}

// S6b support.  An object may hold several shells (edge-connected components);
// each is judged on its own: closed and consistently wound <=> every directed
// edge of the component occurs once and so does its reverse (vertices welded
// by exact position).  Per triangle: orient = the sign of its component's
// enclosed volume (+1 outward winding, -1 inward; 0 when the component is
// open / inconsistent, which leaves its triangles two-sided) and the
// component's bounding box, padded by 1e-4 of its extent + 1e-6.
static void shellOrientation(const mrx::ObjTri *tris, uint32_t n, mrx::TriMat *mats)
{
    std::map<std::array<uint32_t, 3>, uint32_t> ids;
    std::vector<std::array<uint32_t, 3>> tv(n);
    for (uint32_t t = 0; t < n; ++t)
        for (int c = 0; c < 3; ++c) {
            std::array<uint32_t, 3> key;
            std::memcpy(key.data(), tris[t].p + 3 * c, 12);
            for (uint32_t &w : key)
                if (w == 0x80000000u) w = 0;            // -0 == +0
            auto it = ids.find(key);
            if (it == ids.end())
                it = ids.emplace(key, (uint32_t)ids.size()).first;
            tv[t][c] = it->second;
        }
    // components: triangles joined through a shared (undirected) edge
    std::vector<uint32_t> parent(n);
    for (uint32_t t = 0; t < n; ++t)
        parent[t] = t;
    auto find = [&](uint32_t x) {
        while (parent[x] != x)
            x = parent[x] = parent[parent[x]];
        return x;
    };
    std::map<std::pair<uint32_t, uint32_t>, uint32_t> firstOnEdge;
    for (uint32_t t = 0; t < n; ++t)
        for (int c = 0; c < 3; ++c) {
            uint32_t a = tv[t][c], b = tv[t][(c + 1) % 3];
            if (a > b) std::swap(a, b);
            auto ins = firstOnEdge.emplace(std::make_pair(a, b), t);
            if (!ins.second)
                parent[find(t)] = find(ins.first->second);
        }
    struct Shell {
        std::map<std::pair<uint32_t, uint32_t>, int> edges;
        double vol = 0.0;
        bool bad = false;
        uint32_t count = 0;
        float lo[3], hi[3];
    };
    std::map<uint32_t, Shell> shells;
    for (uint32_t t = 0; t < n; ++t) {
        Shell &sh = shells[find(t)];
        const uint32_t *v = tv[t].data();
        if (v[0] == v[1] || v[1] == v[2] || v[2] == v[0])
            sh.bad = true;
        for (int c = 0; c < 3; ++c)
            if (++sh.edges[{ v[c], v[(c + 1) % 3] }] > 1)
                sh.bad = true;
        const float *a = tris[t].p, *b = a + 3, *c3 = a + 6;
        sh.vol += (double)a[0] * ((double)b[1] * c3[2] - (double)b[2] * c3[1]) +
                  (double)a[1] * ((double)b[2] * c3[0] - (double)b[0] * c3[2]) +
                  (double)a[2] * ((double)b[0] * c3[1] - (double)b[1] * c3[0]);
        for (int c = 0; c < 3; ++c)
            for (int ax = 0; ax < 3; ++ax) {
                const float x = tris[t].p[3 * c + ax];
                if ((sh.count == 0 && c == 0) || x < sh.lo[ax]) sh.lo[ax] = x;
                if ((sh.count == 0 && c == 0) || x > sh.hi[ax]) sh.hi[ax] = x;
            }
        sh.count++;
    }
    for (auto &kv : shells) {
        Shell &sh = kv.second;
        if (sh.count < 4)
            sh.bad = true;
        for (const auto &e : sh.edges)
            if (!sh.bad && sh.edges.find({ e.first.second, e.first.first }) == sh.edges.end())
                sh.bad = true;
        for (int ax = 0; ax < 3; ++ax) {
            const float pad = 1e-4f * (sh.hi[ax] - sh.lo[ax]) + 1e-6f;
            sh.lo[ax] -= pad;
            sh.hi[ax] += pad;
        }
    }
    for (uint32_t t = 0; t < n; ++t) {
        const Shell &sh = shells[find(t)];
        mats[t].orient = sh.bad ? 0.0f : sh.vol > 0.0 ? 1.0f : sh.vol < 0.0 ? -1.0f : 0.0f;
        std::memcpy(mats[t].bbMin, sh.lo, 12);
        std::memcpy(mats[t].bbMax, sh.hi, 12);
    }
}

// One-tile views whose worlds fit one pass: two views per workgroup, their TLASes built side by side (bvh.hip,
// MULTI) -- phase I is as long as the latency of its pose loads whether one wave works in it or two, and the
// texel loads at the end of the first view's tile overlap the traversal of the second.  As long as the groups
// still fill the chip (two resident workgroups per CU) and two TLASes leave room for two workgroups in a CU's
// LDS: untextured worlds of up to 104 instances, textured ones of up to 64 (profiles/r03_bvh_group_views.txt).
// Called whenever the bound geometry changes (textured or not decides the kernel's tables).
static int chooseBvhGroups(mrx_renderer &r)
{
    using namespace mrx;
    RasterParams &p = r.params;
    const uint32_t nviews = p.numViews, maxWorldInst = r.info.max_world_instances;
    p.bvhGroupViews = 1;
    // worlds that fit one 64-lane set-up take the flat kernel (bvh.hip): 64x64 tiles, one view per workgroup
    p.bvhFlat = (p.bvhTile == 0 && r.info.max_world_triangles <= 64u && maxWorldInst <= 64u) ? 1u : 0u;
    if (const char *dbg = std::getenv("MRX_BVH_FLAT"))
        p.bvhFlat = p.bvhFlat && std::atoi(dbg) != 0;
    p.bvhGroupTiles = r.bvhGroupTilesGeneral;
    if (p.bvhFlat) {
        // Tiles of a view per workgroup for the flat kernel (three workgroups per CU: 46 KB of LDS each).  A group pays
        // one set-up of the view (S) and then a tile time (T) per tile, and the launch runs in ceil(groups / resident)
        // generations: the run length -- the view's tiles divided by a power of two, at most 16 -- that minimises
        // generations x (S + tiles x T).  S / T = 2.5 / 3.0 from the stamps (profiles/r04_flat_stamps.txt); measured
        // (profiles/r04_flat_zbufs_ab.txt): 1024 x 128^2 picks 2 (39.0 us against 41.4 at 4 and 48.3 at 1), 4096 x 128^2
        // picks 4 (115 against 137 / 166), configs[4] (4096 views of 16 tiles) picks 8.
        const uint32_t tpvF = ((p.nfast + 63u) / 64u) * ((p.nslow + 63u) / 64u);
        const uint32_t residentF = 3u * std::max(p.numCUs, 1u);
        uint32_t best = 1;
        double bestCost = 1e300;
        for (uint32_t g = std::min(tpvF, 16u); g >= 1u; g = (g + 1u) / 2u) {
            const uint64_t groups = (uint64_t)nviews * ((tpvF + g - 1) / g);
            const double cost = (double)((groups + residentF - 1) / residentF) * (2.5 + 3.0 * (double)g);
            if (cost < bestCost) {
                bestCost = cost;
                best = g;
            }
            if (g == 1u)
                break;
        }
        p.bvhGroupTiles = best;
        if (const char *dbg = std::getenv("MRX_BVH_GROUP_TILES"))
            p.bvhGroupTiles = (uint32_t)std::max(1, std::min((int)tpvF, std::atoi(dbg)));
        return MRX_OK;
    }
    const uint32_t resident = 2u * std::max(p.numCUs, 1u);
    const uint32_t tpv = ((p.nfast + 63u) / 64u) * ((p.nslow + 63u) / 64u);
    if (tpv == 1 && p.bvhTile == 0 && maxWorldInst <= p.bvhPassInst) {
        const bool tex = p.anyTextured != 0;
        // (by view count, profiles/r03_bvh_group_views.txt: two views per workgroup win where the pairs fit the chip at
        // once and fill at least three quarters of it -- 768 ... 1024 views on 256 CUs -- and again from four
        // generations of single views on; in between, two generations of single views beat one and a bit of pairs)
        // Between one and two views per resident workgroup the launch is as many workgroups as the chip holds, pairs
        // on the first nviews - resident of them and single views on the others (bit 16; bvh.hip): one generation
        // for 513 ... 1024 views.
        // (worlds of more than 64 instances: only from three quarters of the chip in pairs on -- 576 ... 700 views of
        // 101-instance worlds lose 4 % to two generations of single views, profiles/r03_bvh_group_views.txt)
        const bool mixed = nviews > resident && nviews <= 2u * resident &&
                           (maxWorldInst <= 64u || 2u * nviews >= 3u * resident);
        const bool pairsPay = mixed || nviews >= 4u * resident;
        // (textured: pairs as long as two TLAS blocks leave room for 256 records)
        // (a textured renderer with the normals output: its dword per record slot counts, as below)
        p.bvhGroupViews = pairsPay && bvhLdsBytes(p.bvhPassInst, tex, p.bvhClassify != 0, 2u, 256u) +
                                          ((tex && p.normal) ? 256u * 4u : 0u) <= 80u * 1024u ? 2u : 1u;
        if (p.bvhGroupViews == 2u && mixed && !std::getenv("MRX_BVH_NO_MIXED"))
            p.bvhGroupViews |= 0x10000u;
        if (const char *dbg = std::getenv("MRX_BVH_GROUP_VIEWS")) {
            const int want = std::atoi(dbg);
            if (want == 1 || want == 2 || want == 4 || want == 8)
                p.bvhGroupViews = (uint32_t)want | (want == 2 ? (p.bvhGroupViews & 0x10000u) : 0u);
        }
    }
    // Launches of one-tile views whose workgroups all run at once (more than one per CU, at most two): the
    // workgroup dispatched second to a CU runs the first part of its work at wave priority 1 (bvh.hip: the arbiters
    // serve the older workgroup first, and the launch ends with the younger half).  MRX_BVH_PRIO: 0 off, 1 / 2 / 3
    // the modes measured there.  (Views of several tiles, one generation of workgroups: 256 x 128^2 gains 4 - 6 %,
    // 128 x 128^2 of 100 cubes loses 7 %, C5 / 8 loses 1 % -- tiles of a view differ too much in what they hold;
    // left alone.  profiles/r03_bvh_priority.txt)
    int prio = 2;
    if (const char *dbg = std::getenv("MRX_BVH_PRIO"))
        prio = std::max(0, std::min(3, std::atoi(dbg)));
    const uint32_t tw = p.bvhTile == 2 ? 32 : 64, th = p.bvhTile == 0 ? 64 : 32;
    const uint32_t tiles = ((p.nfast + tw - 1) / tw) * ((p.nslow + th - 1) / th);
    const uint32_t groupTiles = std::max(1u, std::min(p.bvhGroupTiles, tiles));
    const uint32_t gv = p.bvhGroupViews & 0xFFFFu;
    const uint32_t wgs = (p.bvhGroupViews & 0x10000u) ? resident
                         : gv > 1 ? (nviews + gv - 1) / gv : nviews * ((tiles + groupTiles - 1) / groupTiles);
    // textured worlds: as many 48-byte shading records per round as fit the half CU beside the TLAS block(s), in 32s
    // (profiles/r04_bvh_textured.txt; MRX_BVH_TEX_CAP overrides).  With the normals output a record
    // costs 52 bytes -- the normals forms keep a dword per record slot behind everything else -- so the cap is smaller
    // and the workgroup stays within the half CU: two per CU, as the launch shape and the priority scheme assume.
    {
        const uint32_t perSlot = p.normal ? 4u : 0u;
        uint32_t cap = 64;
        while (cap + 32u <= 1008u &&
               bvhLdsBytes(p.bvhPassInst, true, p.bvhClassify != 0, gv, cap + 32u) + perSlot * (cap + 32u) <= 80u * 1024u)
            cap += 32u;
        if (const char *dbg = std::getenv("MRX_BVH_TEX_CAP"))
            cap = (uint32_t)std::max(64, std::min((int)cap, std::atoi(dbg)));
        p.bvhTexCap = cap;
    }
    p.bvhGroupViews |= std::min(resident / 2u, 4095u) << 20;      // (the first index of a CU's second workgroup)
    if (prio && p.bvhTile == 0 && tiles == 1 && wgs <= resident && wgs > resident / 2u)
        p.bvhGroupViews |= (uint32_t)prio << 17;
    return MRX_OK;
}

// Everything that follows from which object each instance row is bound to (r.boundObj):
// the world-local triangle numbering, the per-view draw lists of the raster kernels, the
// per-instance BLAS records of the BVH path, which kernel renders, the uniform-world fast
// paths.  Runs at creation and again from mrx_refresh_objects; the pose tensors, the
// outputs and the object pool are untouched.
// [I] the object each row is bound to, as the trace stage reads it (one spare word: idle lanes read row 0)
hipError_t uploadRayBound(mrx_renderer &r)
{
    std::vector<int32_t> bound(r.boundObj);
    if (bound.empty())
        bound.push_back(-1);
    return r.rayBound.reupload(bound);
}

int bindGeometry(mrx_renderer &r)
{
    using namespace mrx;
    const std::vector<int32_t> &bound = r.boundObj;
    const std::vector<uint32_t> &worldInstStart = r.worldInstStartHost, &viewWorld = r.viewWorldHost;
    const uint32_t numWorlds = (uint32_t)worldInstStart.size() - 1u;
    auto drawn = [&](int32_t o) { return o >= 0 && (size_t)o < r.objFirst.size(); };
    std::vector<uint32_t> worldTriStart(1, 0), instKBase(bound.size(), 0);
    std::vector<WorldTri> worldTris;   // per world; expanded per view below
    uint32_t maxWorldTris = 0;
    for (uint32_t w = 0; w < numWorlds; ++w) {
        for (uint32_t row = worldInstStart[w]; row < worldInstStart[w + 1]; ++row) {
            // first world-local triangle index of the instance (the visibility id space)
            instKBase[row] = (uint32_t)worldTris.size() - worldTriStart[w];
            if (drawn(bound[row])) {
                const uint32_t f = (uint32_t)r.objFirst[bound[row]];
                const uint32_t n = (uint32_t)r.objCount[bound[row]];
                for (uint32_t t = 0; t < n; ++t)
                    worldTris.push_back(WorldTri { row, f + t });
            }
        }
        worldTriStart.push_back((uint32_t)worldTris.size());
        maxWorldTris = std::max(maxWorldTris, worldTriStart[w + 1] - worldTriStart[w]);
    }
    // Which kernel renders: the group kernel (raster.hip) wins while a world fits its
    // 128-slot instantiation, the BVH path (bvh.hip) as soon as the 256-slot one
    // would be needed (measured at 1024 worlds x 64x64: 122 triangles 20.9 against
    // 25.7 us, 134 triangles 28.6 against 27.0, 482 triangles 83 against 31.4 --
    // profiles/r02_bvh_crossover.txt); it serves both render modes.
    // MRX_BVH_MIN_TRIS moves the threshold; kernel_variant 2 / 3 force the BVH /
    // the raster kernels.
    //   Small batches of one-tile views cross over earlier: up to two workgroups per CU the BVH kernel's
    // launch costs what its slowest workgroup costs, while the raster kernels' 128-slot shape pays for its slots
    // (profiles/r03_bvh_threshold.txt: 512 views of 74 triangles 10.7 against 12.3 us, 1024 views of 98 triangles
    // 18.0 against 18.6; 2048 views and more cross at 122 ... 129).
    uint32_t minTris = r.bvhMinTris;
    {
        // (a renderer that shades with the material column: a textured material of the table may come to be drawn)
        bool anyTex = r.params.instMat && r.anyMatTextured;
        for (const WorldTri &wt : worldTris)
            if (r.triMatsHost[wt.tri].tex >= 0) {
                anyTex = true;
                break;
            }
        const uint32_t nviews = (uint32_t)viewWorld.size();
        // (textured worlds: the same up to 2.5 views per CU -- 512 views of 74 triangles 13.0 against 15.5 us -- and at
        // 4 per CU only from ~115 triangles on, left at the general threshold; raster.hpp bvhDispatchMinTris)
        if (!std::getenv("MRX_BVH_MIN_TRIS"))
            minTris = bvhDispatchMinTris(minTris, nviews, anyTex, r.params.nfast, r.params.nslow, r.params.numCUs);
    }
    // (Raytracer-mode batches of many large views of small worlds: the BVH path's flat kernel -- what BASELINE configs[4]
    // names -- is ahead of the raster kernel there; raster.hpp bvhDispatchFlat.  MRX_BVH_FLAT=0 / MRX_BVH_MIN_TRIS: off)
    bool rtFlat = bvhDispatchFlat(r.mode == MRX_MODE_RAYTRACER, (uint32_t)viewWorld.size(), r.params.nfast, r.params.nslow,
                                  maxWorldTris, r.info.max_world_instances, r.params.numCUs) &&
                  !std::getenv("MRX_BVH_MIN_TRIS") && r.params.bvhTile == 0;
    if (const char *dbg = std::getenv("MRX_BVH_FLAT"))
        rtFlat = rtFlat && std::atoi(dbg) != 0;
    r.useBvh = r.variant == kVariantBvh || (r.variant == kVariantDefault && (maxWorldTris >= minTris || rtFlat));
    if (r.useBvh && maxWorldTris > kBvhMaxWorldTris)
        return fail(MRX_E_UNSUPPORTED, "more than 2M triangles in one world");
    // per-view draw lists with a fixed stride (one load level in the kernel);
    // the BVH path walks the world's instances instead and needs none
    const uint32_t stride = maxWorldTris ? maxWorldTris : 1u;
    {
        const size_t nv = r.useBvh ? 0 : viewWorld.size();
        std::vector<WorldTri> viewTris(nv * stride, WorldTri { 0, 0 });
        std::vector<uint32_t> viewTriCount(nv);
        for (size_t v = 0; v < nv; ++v) {
            const uint32_t w = viewWorld[v];
            const uint32_t b = worldTriStart[w], n = worldTriStart[w + 1] - b;
            viewTriCount[v] = n;
            std::memcpy(viewTris.data() + v * stride, worldTris.data() + b, n * sizeof(WorldTri));
        }
        MRX_HIP(r.viewTris.reupload(viewTris));
        MRX_HIP(r.viewTriCount.reupload(viewTriCount));
    }
    // per instance: range, root and box of its bound object, so the per-step TLAS build has
    // no load that depends on another
    std::vector<ObjInfo> instInfo(bound.size());
    for (size_t i = 0; i < bound.size(); ++i) {
        ObjInfo info {};
        info.root = -1;
        if (drawn(bound[i]))
            info = r.blas.objects[bound[i]];
        instInfo[i] = info;
    }
    if (instInfo.empty())
        instInfo.emplace_back();                      // idle lanes read row 0
    MRX_HIP(r.objInfo.reupload(instInfo));
    MRX_HIP(r.instKBase.reupload(instKBase));
    // the ray-cast sensor stores the bound object's id of the row it hits
    if (r.raysPerWorld)
        MRX_HIP(uploadRayBound(r));

    RasterParams &p = r.params;
    // (the material column, DESIGN.md 4.14: decided here, never by what the column holds)
    p.anyTextured = (p.instMat && r.anyMatTextured) ? 1 : 0;
    for (const mrx::WorldTri &wt : worldTris)
        if (r.triMatsHost[wt.tri].tex >= 0) {
            p.anyTextured = 1;
            break;
        }
    p.viewTris = r.viewTris.ptr;
    p.viewTriCount = r.viewTriCount.ptr;
    p.viewTriStride = stride;
    p.instInfo = r.objInfo.ptr;
    p.instKBase = r.instKBase.ptr;
    // uniform worlds -> arithmetic draw list (raster.hpp): every world the same 1..4 bound
    // objects in the same order, the same camera count
    p.uniInstances = 0;
    p.uniCamsPerWorld = 0;
    if (numWorlds > 0) {
        const uint32_t n0 = worldInstStart[1] - worldInstStart[0], c0 = r.worldCams[0];
        bool uni = n0 >= 1 && n0 <= 4 && c0 >= 1;
        for (uint32_t w = 0; uni && w < numWorlds; ++w) {
            uni = worldInstStart[w + 1] - worldInstStart[w] == n0 && r.worldCams[w] == c0;
            for (uint32_t i = 0; uni && i < n0; ++i) {
                const int32_t oa = bound[worldInstStart[w] + i], ob = bound[worldInstStart[0] + i];
                uni = oa == ob && drawn(oa);
            }
        }
        if (uni) {
            p.uniInstances = n0;
            p.uniCamsPerWorld = c0;
            uint32_t acc = 0;
            for (uint32_t i = 0; i < 4; ++i) {
                p.uniPrefix[i] = acc;
                p.uniFirstTri[i] = 0;
                if (i < n0) {
                    const int32_t o = bound[worldInstStart[0] + i];
                    p.uniFirstTri[i] = (uint32_t)r.objFirst[o];
                    acc += (uint32_t)r.objCount[o];
                }
            }
            p.uniPrefix[4] = acc;
        }
    }
    r.info.max_world_triangles = maxWorldTris;
    r.info.render_path = r.useBvh ? 1 : 0;
    return chooseBvhGroups(r);
}

// The launch form of the projections in r.proj and the lights in r.lights.  Every view the
// same projection and every world the same light: the constants go in the kernel arguments and params.viewProj /
// viewLight are null (the uniform form -- a renderer of default cameras and lights launches exactly what it always
// did).  Views or worlds that differ: both tables, one record per view, are copied to the device on the renderer's
// stream, behind every render enqueued so far and ahead of every later one, and the kernels' per-view instantiations
// read them; the table of whichever does not vary holds the uniform values.
// A renderer that shades with the colour column (params.instColor) or the material column
// (params.instMat, 4.14) or the label column (params.instLabel, 4.16) always launches with the tables: the chunked, brute and BVH kernels read the columns in their
// per-view instantiations.  params.tablesVary tells the
// group kernels, which have a colour form over the uniform constants, whether the tables hold anything else.
int applyViewTables(mrx_renderer &r)
{
    mrx::RasterParams &p = r.params;
    const bool rt = r.mode == MRX_MODE_RAYTRACER;
    const uint32_t W = rt ? p.nslow : p.nfast, H = rt ? p.nfast : p.nslow;
    const mrx_projection dflt = { (float)kVfovDeg, 0.0f };
    const mrx_projection &first = r.proj.empty() ? dflt : r.proj[0];
    const mrx_light &firstLight = r.lights.empty() ? kDefaultLight : r.lights[0];
    bool uniform = true, sameLight = true;
    for (const mrx_projection &q : r.proj)
        uniform = uniform && std::memcmp(&q, &first, sizeof q) == 0;
    for (const mrx_light &l : r.lights)
        sameLight = sameLight && std::memcmp(&l, &firstLight, sizeof l) == 0;
    uniform = uniform && sameLight;
    mrx::ViewProj c;
    int rc = projectionConstants(W, H, rt, first, c);
    if (rc != MRX_OK)
        return rc;
    mrx::ViewLight lc;
    rc = lightConstants(firstLight, lc);
    if (rc != MRX_OK)
        return rc;
    p.sx = c.sx; p.ox = c.ox; p.sz = c.sz; p.oz = c.oz;
    p.invNear = c.invNear;
    p.s6bPad = c.s6bPad;
    for (int k = 0; k < 3; ++k)
        p.toLight[k] = lc.toLight[k];
    p.ambient = lc.ambient;
    p.diffuse = lc.diffuse;
    const size_t n = r.proj.size();
    p.tablesVary = uniform ? 0u : 1u;
    if (uniform && !((p.instColor || p.instMat || p.instLabel) && n)) {
        p.viewProj = nullptr;
        p.viewLight = nullptr;
        p.lightTable = 0;
        return MRX_OK;
    }
    MRX_HIP(hipSetDevice(r.device));
    if (!r.projDev.ptr) {
        MRX_HIP(r.projDev.alloc(n, 256));
        MRX_HIP(r.lightDev.alloc(n, 256));
        MRX_HIP(hipHostMalloc((void **)&r.projStage, n * sizeof(mrx::ViewProj), hipHostMallocDefault));
        MRX_HIP(hipHostMalloc((void **)&r.lightStage, n * sizeof(mrx::ViewLight), hipHostMallocDefault));
        MRX_HIP(hipEventCreateWithFlags(&r.projEv, hipEventDisableTiming));
    }
    // the staging is what the last copies read: it is overwritten only once they have run
    if (r.projCopyPending)
        MRX_HIP(hipEventSynchronize(r.projEv));
    for (size_t v = 0; v < n; ++v) {
        rc = projectionConstants(W, H, rt, r.proj[v], r.projStage[v]);
        if (rc != MRX_OK)
            return rc;
        rc = lightConstants(r.lights[r.viewWorldHost[v]], r.lightStage[v]);
        if (rc != MRX_OK)
            return rc;
    }
    MRX_HIP(hipMemcpyAsync(r.projDev.ptr, r.projStage, n * sizeof(mrx::ViewProj), hipMemcpyHostToDevice, r.stream));
    MRX_HIP(hipMemcpyAsync(r.lightDev.ptr, r.lightStage, n * sizeof(mrx::ViewLight), hipMemcpyHostToDevice, r.stream));
    MRX_HIP(hipEventRecord(r.projEv, r.stream));
    r.projCopyPending = true;
    p.viewProj = r.projDev.ptr;
    p.viewLight = r.lightDev.ptr;
    p.lightTable = sameLight ? 0u : 1u;
    return MRX_OK;
}

int buildScene(const mrx_config &cfg, mrx_renderer &r)
{
    using namespace mrx;
    // ---- objects: disk assets in path order, then one object per raw mesh
    //      (/root/reference/src/mgr.cpp:267-270, scripts/test.py:7-10)
    std::vector<ObjTri> &tris = r.hostTris;
    const uint32_t maxInstancesPerWorld = cfg.max_instances_per_world;
    auto appendObject = [&](const float *pos, const float *uv, uint32_t n, int32_t mat) {
        r.objFirst.push_back((int32_t)tris.size());
        r.objCount.push_back((int32_t)n);
        for (uint32_t t = 0; t < n; ++t) {
            ObjTri o {};
            std::memcpy(o.p, pos + 9 * (size_t)t, sizeof(o.p));
            std::memcpy(o.uv, uv + 6 * (size_t)t, sizeof(o.uv));
            o.mat = mat;
            tris.push_back(o);
        }
    };
    // File materials (MTL) are appended after the API materials and textures:
    // an asset with mat_id >= 0 is drawn with that API material; with mat_id
    // -1 each face keeps the material its OBJ names through mtllib / usemtl
    // (Kd colour, map_Kd PNG texture), or the default when it names none.
    struct FileMat { float kd[3]; std::string mapKd; };
    std::vector<FileMat> fileMats;
    std::vector<std::string> fileTexPaths;
    for (uint32_t a = 0; a < cfg.num_asset_paths; ++a) {
        TriSoup soup;
        std::string err;
        if (!loadOBJ(cfg.asset_paths[a], soup, err))
            return fail(MRX_E_ASSET, "Failed to load render assets: " + err);
        // The reference carries a per-asset material id through its API
        // (bindings.cpp:26-36) but applies it only inside a disabled block
        // (mgr.cpp:339-349); the block's evident intent is implemented here.
        int32_t mat = -1;
        if (cfg.mat_assignments && a < cfg.num_mat_assignments)
            mat = cfg.mat_assignments[a];
        // One object per asset FILE: the reference imports with one_object_per_asset
        // (the `true` of importFromDisk, mgr.cpp:301-303) and addresses objects[i] by asset
        // path i (mgr.cpp:340-345), so the `o` / `g` blocks of a file are the meshes of one
        // object and later assets / raw meshes keep the ids the reference gives them.
        // MRX_OBJ_SPLIT_BLOCKS=1 opts into one object per block instead.
        const char *split = std::getenv("MRX_OBJ_SPLIT_BLOCKS");
        if (split && split[0] == '1') {
            for (size_t o = 0; o < soup.objStart.size(); ++o) {
                const uint32_t t0 = soup.objStart[o];
                const uint32_t t1 = o + 1 < soup.objStart.size() ? soup.objStart[o + 1] : soup.numTris();
                appendObject(soup.pos.data() + 9 * (size_t)t0, soup.uv.data() + 6 * (size_t)t0, t1 - t0, mat);
            }
        } else {
            appendObject(soup.pos.data(), soup.uv.data(), soup.numTris(), mat);
        }
        if (mat < 0 && !soup.mtlNames.empty()) {
            std::vector<MtlMaterial> lib;
            for (const std::string &ml : soup.mtlLibs) {
                std::string merr;
                (void)loadMTL(ml, lib, merr);       // a missing library leaves faces on the default
            }
            std::vector<int32_t> nameToMat(soup.mtlNames.size(), -1);
            for (size_t n = 0; n < soup.mtlNames.size(); ++n)
                for (const MtlMaterial &mm : lib)
                    if (mm.name == soup.mtlNames[n]) {
                        nameToMat[n] = (int32_t)(cfg.num_materials + fileMats.size());
                        fileMats.push_back(FileMat { { mm.kd[0], mm.kd[1], mm.kd[2] }, mm.mapKd });
                        break;
                    }
            const size_t first = tris.size() - soup.numTris();
            for (uint32_t t = 0; t < soup.numTris(); ++t)
                if (soup.triMtl[t] >= 0)
                    tris[first + t].mat = nameToMat[soup.triMtl[t]];
        }
    }
    const mrx_geometry &g = cfg.geo;
    for (uint32_t m = 0; m < g.num_meshes; ++m) {   // mgr.cpp:214-272
        const uint32_t v0 = g.mesh_vertex_offsets[m];
        const uint32_t v1 = m + 1 < g.num_meshes ? g.mesh_vertex_offsets[m + 1] : g.num_vertices;
        const uint32_t i0 = g.mesh_index_offsets[m];
        const uint32_t i1 = m + 1 < g.num_meshes ? g.mesh_index_offsets[m + 1] : g.num_indices;
        if (v1 < v0 || v1 > g.num_vertices || i1 < i0 || i1 > g.num_indices)
            return fail(MRX_E_INVALID, "raw mesh offsets out of range");
        const uint32_t nt = (i1 - i0) / 3;
        std::vector<float> pos(9 * (size_t)nt), uv(6 * (size_t)nt);
        for (uint32_t t = 0; t < nt; ++t)
            for (int c = 0; c < 3; ++c) {
                const uint32_t vi = g.indices[i0 + 3 * t + c];
                if (vi >= v1 - v0)
                    return fail(MRX_E_INVALID, "raw mesh index out of range");
                std::memcpy(&pos[9 * (size_t)t + 3 * c], g.vertices + 3 * (size_t)(v0 + vi), 12);
                std::memcpy(&uv[6 * (size_t)t + 2 * c], g.uvs + 2 * (size_t)(v0 + vi), 8);
            }
        appendObject(pos.data(), uv.data(), nt, g.mesh_materials[m]);
    }

    // ---- textures and materials (mgr.cpp:316-337; no disk textures or
    //      materials exist, so the index shift there is zero)
    std::vector<TexDesc> texDescs;
    std::vector<uint32_t> texels;
    for (uint32_t t = 0; t < cfg.num_textures; ++t) {
        Image img;
        std::string err;
        if (!decodeTexture(cfg.texture_paths[t], img, err))
            return fail(MRX_E_ASSET, "Failed to load texture: " + err);
        // (the BVH kernels' shading records hold width | height << 16)
        if (img.width == 0 || img.height == 0 || img.width > 65535u || img.height > 65535u)
            return fail(MRX_E_UNSUPPORTED, std::string("texture ") + cfg.texture_paths[t] +
                                               ": sides of 1 ... 65535 texels are supported");
        TexDesc d {};
        d.offset = (uint32_t)texels.size();
        d.width = img.width;
        d.height = img.height;
        texDescs.push_back(d);
        const size_t n = (size_t)img.width * img.height;
        texels.resize(texels.size() + n);
        std::memcpy(texels.data() + d.offset, img.rgba.data(), n * 4);
    }
    // combined material table: API materials, then file materials whose map_Kd
    // textures (PNG or KTX2; anything unreadable means untextured) follow the API textures
    std::vector<mrx_material> allMats(cfg.materials, cfg.materials + cfg.num_materials);
    for (const FileMat &fm : fileMats) {
        mrx_material m {};
        m.color[0] = fm.kd[0]; m.color[1] = fm.kd[1]; m.color[2] = fm.kd[2]; m.color[3] = 1.0f;
        m.texture_idx = -1;
        m.roughness = 0.8f;
        m.metalness = 0.2f;
        if (!fm.mapKd.empty()) {
            int32_t found = -1;
            for (size_t i = 0; i < fileTexPaths.size(); ++i)
                if (fileTexPaths[i] == fm.mapKd)
                    found = (int32_t)(cfg.num_textures + i);
            if (found < 0) {
                Image img;
                std::string terr;
                if (decodeTexture(fm.mapKd, img, terr) && img.width >= 1 && img.height >= 1 && img.width <= 65535u &&
                    img.height <= 65535u) {
                    TexDesc d {};
                    d.offset = (uint32_t)texels.size();
                    d.width = img.width;
                    d.height = img.height;
                    texDescs.push_back(d);
                    const size_t n = (size_t)img.width * img.height;
                    texels.resize(texels.size() + n);
                    std::memcpy(texels.data() + d.offset, img.rgba.data(), n * 4);
                    found = (int32_t)(cfg.num_textures + fileTexPaths.size());
                    fileTexPaths.push_back(fm.mapKd);
                }
            }
            m.texture_idx = found;
        }
        allMats.push_back(m);
    }
    // resolve every object triangle's material once: mesh material if it
    // exists, else the default colour (white, untextured); a texture index
    // with no texture behind it means untextured
    std::vector<TriMat> triMats(tris.size());
    for (size_t t = 0; t < tris.size(); ++t) {
        TriMat &tm = triMats[t];
        tm.color[0] = tm.color[1] = tm.color[2] = tm.color[3] = 1.0f;
        tm.tex = -1;
        const int32_t m = tris[t].mat;
        if (m >= 0 && (size_t)m < allMats.size()) {
            std::memcpy(tm.color, allMats[m].color, 16);
            tm.tex = allMats[m].texture_idx;
        }
        if (tm.tex < 0 || (uint32_t)tm.tex >= (uint32_t)texDescs.size())
            tm.tex = -1;
        if (tm.tex >= 0) {
            // the texture's descriptor rides along (BVH path: no second load level per pixel)
            tm.texDesc[0] = (int32_t)texDescs[tm.tex].offset;
            tm.texDesc[1] = (int32_t)texDescs[tm.tex].width;
            tm.texDesc[2] = (int32_t)texDescs[tm.tex].height;
        }
    }
    // the table the material override reads: rgb and the texture index validated the same way, and
    // one spare record past the end in a colour no test material has -- a missing range guard shows, it does not stray
    std::vector<MatRec> matRecs;
    const bool wantMats = (cfg.flags & MRX_FLAG_INSTANCE_MATERIALS) != 0;
    const bool wantLabels = (cfg.flags & MRX_FLAG_INSTANCE_LABELS) != 0;
    r.anyMatTextured = false;
    if (wantMats) {
        for (const mrx_material &m : allMats) {
            MatRec rec = { m.color[0], m.color[1], m.color[2], m.texture_idx };
            if (rec.tex < 0 || (uint32_t)rec.tex >= (uint32_t)texDescs.size())
                rec.tex = -1;
            r.anyMatTextured = r.anyMatTextured || rec.tex >= 0;
            matRecs.push_back(rec);
        }
        matRecs.push_back(MatRec { 0.8125f, 0.0625f, 0.6875f, -1 });
    }
    // the object a triangle belongs to rides in the alpha slot (segmask label, raster.hpp)
    for (size_t o = 0; o < r.objFirst.size(); ++o)
        for (int32_t t = 0; t < r.objCount[o]; ++t) {
            const int32_t id = (int32_t)o;
            std::memcpy(&triMats[(size_t)r.objFirst[o] + t].color[3], &id, 4);
        }
    // S6b: orientation and padded bounding box of every triangle's shell
    for (size_t o = 0; o < r.objFirst.size(); ++o)
        shellOrientation(tris.data() + r.objFirst[o], (uint32_t)r.objCount[o],
                         triMats.data() + r.objFirst[o]);

    // ---- world assembly: per-world copies of the table rows, world-major
    //      (/root/reference/src/sim.cpp:143-175).  With max_instances_per_world a world owns
    //      that many rows at least (the reference sizes its renderer by maxInstancesPerWorld,
    //      src/mgr.cpp:378-388, and creates renderables at run time, src/sim.inl:5-8): the
    //      spare rows start hidden and unbound (ObjectID -1, identity pose) and are bound to
    //      an object by writing its id and calling mrx_refresh_objects.
    std::vector<float> instPos, instRot, instScale, camPos, camRot;
    std::vector<int32_t> instObj;
    // (the colour column, with the flag: a row's four bytes, or zero for all of them and for spare rows)
    const bool wantColors = (cfg.flags & MRX_FLAG_INSTANCE_COLORS) != 0;
    std::vector<uint32_t> instColor;
    // (the material column, with its flag: spare rows -1; the initial ids come through mrx_set_instance_materials)
    std::vector<int32_t> instMat;
    std::vector<uint32_t> &worldInstStart = r.worldInstStartHost, &viewWorld = r.viewWorldHost;
    worldInstStart.assign(1, 0u);
    viewWorld.clear();
    r.worldCams.clear();
    r.proj.clear();
    // (checked by mrx_create)
    r.lights.assign(cfg.num_worlds, kDefaultLight);
    if (cfg.world_lights)
        r.lights.assign(cfg.world_lights, cfg.world_lights + cfg.num_worlds);
    uint32_t maxWorldInst = 0;
    for (uint32_t w = 0; w < cfg.num_worlds; ++w) {
        const mrx_world_init &wi = cfg.worlds[w];
        if ((uint64_t)wi.instances_offset + wi.num_instances > cfg.num_instances ||
            (uint64_t)wi.cameras_offset + wi.num_cameras > cfg.num_cameras)
            return fail(MRX_E_INVALID, "world " + std::to_string(w) +
                                           " addresses rows outside the tables");
        const uint32_t rows = std::max(wi.num_instances, maxInstancesPerWorld);
        for (uint32_t i = 0; i < rows; ++i) {
            if (i < wi.num_instances) {
                const mrx_instance &in = cfg.instances[wi.instances_offset + i];
                instPos.insert(instPos.end(), in.position, in.position + 3);
                instRot.insert(instRot.end(), in.rotation, in.rotation + 4);
                instScale.insert(instScale.end(), in.scale, in.scale + 3);
                instObj.push_back(in.object_id);
                uint32_t packed = 0;
                if (cfg.instance_colors)
                    std::memcpy(&packed, cfg.instance_colors + 4 * (size_t)(wi.instances_offset + i), 4);
                instColor.push_back(packed);
            } else {
                const float zero[3] = { 0.f, 0.f, 0.f }, ident[4] = { 1.f, 0.f, 0.f, 0.f }, one[3] = { 1.f, 1.f, 1.f };
                instPos.insert(instPos.end(), zero, zero + 3);
                instRot.insert(instRot.end(), ident, ident + 4);
                instScale.insert(instScale.end(), one, one + 3);
                instObj.push_back(-1);
                instColor.push_back(0u);
            }
        }
        worldInstStart.push_back((uint32_t)instObj.size());
        maxWorldInst = std::max(maxWorldInst, rows);
        r.worldCams.push_back(wi.num_cameras);
        for (uint32_t c = 0; c < wi.num_cameras; ++c) {
            const mrx_camera &cam = cfg.cameras[wi.cameras_offset + c];
            camPos.insert(camPos.end(), cam.position, cam.position + 3);
            camRot.insert(camRot.end(), cam.rotation, cam.rotation + 4);
            viewWorld.push_back(w);
            // (checked by mrx_create; the mode's default znear resolved below)
            r.proj.push_back(cfg.camera_projections ? cfg.camera_projections[wi.cameras_offset + c]
                                                    : mrx_projection{ (float)kVfovDeg, 0.0f });
        }
    }
    // the object each row draws: bound here, re-bound by mrx_refresh_objects
    r.boundObj = instObj;

    // ---- upload what never changes shape
    {
        // geometry block: ObjTri[pool], then TriMat[pool] at the next 256-byte boundary
        const uint32_t pool = (uint32_t)tris.size();
        const size_t matsOff = geomMatsOffset(pool);
        MRX_HIP(r.geomBlock.alloc(matsOff + (size_t)pool * sizeof(TriMat) + 256));
        r.tris.view(r.geomBlock.ptr, pool);
        r.triMats.view(r.geomBlock.ptr + matsOff, pool);
        if (pool) {
            MRX_HIP(hipMemcpy(r.tris.ptr, tris.data(), (size_t)pool * sizeof(ObjTri), hipMemcpyHostToDevice));
            MRX_HIP(hipMemcpy(r.triMats.ptr, triMats.data(), (size_t)pool * sizeof(TriMat), hipMemcpyHostToDevice));
        }
    }
    MRX_HIP(r.textures.upload(texDescs));
    MRX_HIP(r.texels.upload(texels));
    r.triMatsHost = triMats;
    r.bvhMinTris = kBvhMinTris;
    if (const char *dbg = std::getenv("MRX_BVH_MIN_TRIS"))
        r.bvhMinTris = (uint32_t)std::max(0, std::atoi(dbg));
    // BLAS per object (the reference builds them at load too: mgr.cpp:472-473)
    buildBlas(tris.data(), r.objFirst, r.objCount, r.blas);
    const BlasSet &blas = r.blas;
    if (blas.leafTris.size() >= (1u << kBvhLeafStartBits))
        return fail(MRX_E_UNSUPPORTED, "too many triangles in BLAS leaves");
    // (the kernel's traversal stack is kBvhStackCap entries of LDS per wave: a deeper tree
    // would write past it -- bvh.cpp rebuilds such trees balanced, which bounds the depth
    // by about log8 of the triangle count; refuse what still does not fit)
    if (1 + 7 * blas.maxDepth > kBvhStackCap)
        return fail(MRX_E_UNSUPPORTED, "a BLAS is too deep for the traversal stack (" +
                                           std::to_string(blas.maxDepth) + " levels)");
    MRX_HIP(r.bvhNodes.upload(blas.nodes));
    MRX_HIP(r.bvhLeafTris.upload(blas.leafTris));
    MRX_HIP(r.worldInstStart.upload(worldInstStart));
    MRX_HIP(r.viewWorld.upload(viewWorld));
    {
        // pose block (the exported, user-mutable tensors are slices of it)
        const uint32_t nv = (uint32_t)viewWorld.size(), ni = (uint32_t)instObj.size();
        const PoseLayout lay = poseLayout(nv, ni);
        // (the colour column, where there is one, behind the layout the FAST prologue relies on; the material column
        // behind the colour column's slot, which a renderer with the material column alone has zero-filled)
        // (the label column behind the slots of both, whichever of them the renderer has)
        const size_t poseBytes = (size_t)lay.total +
                                 (wantLabels ? 3u : wantMats ? 2u : wantColors ? 1u : 0u) * (size_t)mrxAlign256(ni * 4u) + 256;
        MRX_HIP(r.poseBlock.alloc(poseBytes));
        MRX_HIP(hipMemset(r.poseBlock.ptr, 0, poseBytes));
        uint8_t *b = r.poseBlock.ptr;
        r.camRot.view(b + lay.camRot, camRot.size());
        r.camPos.view(b + lay.camPos, camPos.size());
        r.instRot.view(b + lay.instRot, instRot.size());
        r.instPos.view(b + lay.instPos, instPos.size());
        r.instScale.view(b + lay.instScale, instScale.size());
        r.instObj.view(b + lay.instObj, instObj.size());
        auto up = [](void *dst, const void *src, size_t bytes) {
            return bytes ? hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) : hipSuccess;
        };
        MRX_HIP(up(r.camRot.ptr, camRot.data(), camRot.size() * 4));
        MRX_HIP(up(r.camPos.ptr, camPos.data(), camPos.size() * 4));
        MRX_HIP(up(r.instRot.ptr, instRot.data(), instRot.size() * 4));
        MRX_HIP(up(r.instPos.ptr, instPos.data(), instPos.size() * 4));
        MRX_HIP(up(r.instScale.ptr, instScale.data(), instScale.size() * 4));
        MRX_HIP(up(r.instObj.ptr, instObj.data(), instObj.size() * 4));
        if (wantColors) {
            r.instColor.view(b + poseColorOffset(nv, ni), instColor.size());
            MRX_HIP(up(r.instColor.ptr, instColor.data(), instColor.size() * 4));
        }
        if (wantMats) {
            instMat.assign(ni, -1);
            r.instMat.view(b + poseMaterialOffset(nv, ni), instMat.size());
            MRX_HIP(up(r.instMat.ptr, instMat.data(), instMat.size() * 4));
            MRX_HIP(r.matTable.upload(matRecs));
            MRX_HIP(hipHostMalloc((void **)&r.matStage, (size_t)(ni ? ni : 1u) * sizeof(int32_t), hipHostMallocDefault));
            MRX_HIP(hipEventCreateWithFlags(&r.matEv, hipEventDisableTiming));
        }
        if (wantLabels) {
            // (every row at the sentinel: the segmask of S9 until a caller writes the column)
            const std::vector<int32_t> labels(ni, MRX_LABEL_OBJECT);
            r.instLabel.view(b + poseLabelOffset(nv, ni), labels.size());
            MRX_HIP(up(r.instLabel.ptr, labels.data(), labels.size() * 4));
            MRX_HIP(hipHostMalloc((void **)&r.labelStage, (size_t)(ni ? ni : 1u) * sizeof(int32_t), hipHostMallocDefault));
            MRX_HIP(hipEventCreateWithFlags(&r.labelEv, hipEventDisableTiming));
        }
    }

    const bool rt = cfg.render_mode == MRX_MODE_RAYTRACER;
    const uint32_t W = cfg.view_width;
    // Raytracer output is square, res = view width (mgr.cpp:130,443)
    const uint32_t H = rt ? cfg.view_width : cfg.view_height;
    const uint32_t nviews = (uint32_t)viewWorld.size();
    // storage [view][slow][fast]: raster fast = image x; Raytracer fast =
    // image y (callers read it as [x][y]: scripts/test.py:160, dump.cpp:9-21)
    const uint32_t nfast = rt ? H : W, nslow = rt ? W : H;
    const size_t px = (size_t)nviews * nfast * nslow;
    {
        // diagnostic: a block allocated ahead of the outputs (MRX_OUT_PRE_MB), freed
        // again right after them unless MRX_OUT_PRE_HOLD=1
        DevBuf<uint8_t> pre;
        if (const char *dbg = std::getenv("MRX_OUT_PRE_MB"))
            if (pre.alloc((size_t)std::atoll(dbg) << 20) != hipSuccess)
                (void)hipGetLastError();
        MRX_HIP(allocOutputs(px, !(cfg.flags & MRX_FLAG_NO_RGB), !(cfg.flags & MRX_FLAG_NO_DEPTH),
                             rt || wantLabels || (cfg.flags & MRX_FLAG_VISIBILITY_IDS), firstKindIsOneBlock(px), r.rgb, r.depth,
                             r.ids,
                             (cfg.flags & MRX_FLAG_NORMALS) != 0, r.normal));
        const char *hold = std::getenv("MRX_OUT_PRE_HOLD");
        if (!(hold && hold[0] == '1'))
            pre.release();
    }
    // (the label column brings the ids tensor to Rasterizer mode too: S11's segmask)
    const bool wantIds = rt || wantLabels || (cfg.flags & MRX_FLAG_VISIBILITY_IDS);

    RasterParams &p = r.params;
    p.tris = r.tris.ptr;
    p.triMats = r.triMats.ptr;
    p.textures = r.textures.ptr;
    p.texels = r.texels.ptr;
    p.poseBlock = reinterpret_cast<const char *>(r.poseBlock.ptr);
    p.geomBlock = reinterpret_cast<const char *>(r.geomBlock.ptr);
    p.numInstances = (uint32_t)instObj.size();
    p.poolTris = (uint32_t)tris.size();
    p.instPos = r.instPos.ptr;
    p.instRot = r.instRot.ptr;
    p.instScale = r.instScale.ptr;
    p.instObj = r.instObj.ptr;
    // (a depth-only renderer never reads the column: it launches what a renderer without one does)
    p.instColor = (cfg.flags & MRX_FLAG_NO_RGB) ? nullptr : r.instColor.ptr;
    p.instMat = (cfg.flags & MRX_FLAG_NO_RGB) ? nullptr : r.instMat.ptr;
    p.matTable = r.matTable.ptr;
    p.numMaterials = wantMats ? (uint32_t)allMats.size() : 0u;
    // (read under every output selection; never where the ids tensor holds visibility ids, which win over the segmask:
    // such a renderer keeps the column and launches what one without it does)
    p.instLabel = (cfg.flags & MRX_FLAG_VISIBILITY_IDS) ? nullptr : r.instLabel.ptr;
    p.camPos = r.camPos.ptr;
    p.camRot = r.camRot.ptr;
    p.rgb = r.rgb.ptr;
    p.depth = r.depth.ptr;
    p.ids = wantIds ? r.ids.ptr : nullptr;
    p.normal = r.normal.ptr;
    p.numViews = nviews;
    {
        int cus = 0;
        MRX_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, r.device));
        p.numCUs = (uint32_t)std::max(cus, 1);
        if (const char *dbg = std::getenv("MRX_FAKE_CUS"))      // tests: the launch shapes of a smaller device
            p.numCUs = (uint32_t)std::max(1, std::atoi(dbg));
    }
    p.nfast = nfast;
    p.nslow = nslow;
    p.tilesFast = (nfast + 63) / 64;
    p.tilesSlow = (nslow + 63) / 64;
    // S5: pixel -> ray constants, double math rounded once to float -- per view (projectionConstants): the
    // uniform ones in the kernel arguments, or the per-view table (applyViewTables, with the worlds' lights: S4, S7)
    for (mrx_projection &q : r.proj) {
        mrx::ViewProj c;
        if (projectionConstants(W, H, rt, q, c, &q) != MRX_OK)
            return MRX_E_INVALID;
    }
    p.invFar = rt ? 1.0f / kRtZFar : 0.0f;
    {
        const int rc = applyViewTables(r);
        if (rc != MRX_OK)
            return rc;
    }
    p.transposed = rt ? 1 : 0;
    // Raytracer ids are the segmask unless the caller asked for visibility ids
    p.idsAreSegmask = ((rt || wantLabels) && !(cfg.flags & MRX_FLAG_VISIBILITY_IDS)) ? 1 : 0;
    p.debugSkip = 0;
    if (const char *dbg = std::getenv("MRX_DEBUG_SKIP"))
        p.debugSkip = (uint32_t)std::atoi(dbg);
    p.debugStamps = nullptr;
    if (const char *dbg = std::getenv("MRX_DEBUG_STAMPS"))
        if (std::atoi(dbg) != 0) {
            // (x4: the BVH kernel's 32x32 tile shape launches four workgroups per 64x64 tile)
            const size_t n = ((size_t)nviews * p.tilesFast * p.tilesSlow * 4 + 64) * 4 * 8;
            MRX_HIP(r.stamps.alloc(n));
            MRX_HIP(hipMemset(r.stamps.ptr, 0, n * sizeof(unsigned long long)));
            p.debugStamps = r.stamps.ptr;
        }
    p.writeThrough = 1;
    if (const char *dbg = std::getenv("MRX_WRITE_THROUGH"))
        p.writeThrough = std::atoi(dbg) != 0;
    p.grpViews = p.grpChunkTiles = p.grpPerView = 0;
    p.grpViewsWanted = p.grpTilesWanted = 0;
    if (const char *dbg = std::getenv("MRX_GROUP_VIEWS"))
        p.grpViewsWanted = std::atoi(dbg);
    if (const char *dbg = std::getenv("MRX_GROUP_TILES"))
        p.grpTilesWanted = std::atoi(dbg);
    p.xcdRotate = 0;
    p.xcdRotateWanted = -1;
    if (const char *dbg = std::getenv("MRX_XCD_ROTATE"))
        p.xcdRotateWanted = std::atoi(dbg);
    p.xccReport = nullptr;
    p.xcdPhase = 0;
    if (hipHostMalloc((void **)&r.xccHost, 64, hipHostMallocMapped) == hipSuccess &&
        hipHostGetDevicePointer((void **)&r.xccDev, r.xccHost, 0) == hipSuccess) {
        *r.xccHost = 0;
        p.xccReport = r.xccDev;
    } else {
        (void)hipGetLastError();                  // no feedback: the split assumes an even start
        r.xccHost = nullptr;
    }
    if (const char *dbg = std::getenv("MRX_XCD_PHASE"))
        r.xcdPhaseForced = std::atoi(dbg) & 1;
    p.xcdSkew = 0;
    p.xcdSkewWanted = -1;
    if (const char *dbg = std::getenv("MRX_XCD_SKEW"))
        p.xcdSkewWanted = std::atoi(dbg);
    p.debugSlots = 0;
    if (const char *dbg = std::getenv("MRX_DEBUG_SLOTS"))
        p.debugSlots = std::atoi(dbg);
    p.bvhNodes = r.bvhNodes.ptr;
    p.bvhLeafTris = r.bvhLeafTris.ptr;
    p.numObjects = (uint32_t)r.objFirst.size();
    p.bvhUniInst = p.bvhUniCams = 0;
    if (cfg.num_worlds > 0) {
        bool uni = true;
        const uint32_t rows0 = worldInstStart[1] - worldInstStart[0];
        for (uint32_t w = 1; uni && w < cfg.num_worlds; ++w)
            uni = worldInstStart[w + 1] - worldInstStart[w] == rows0 &&
                  cfg.worlds[w].num_cameras == cfg.worlds[0].num_cameras;
        if (uni && rows0 > 0 && cfg.worlds[0].num_cameras > 0) {
            p.bvhUniInst = rows0;
            p.bvhUniCams = cfg.worlds[0].num_cameras;
        }
    }
    p.worldInstStart = r.worldInstStart.ptr;
    p.viewWorld = r.viewWorld.ptr;
    // TLAS records of up to 128 instances stay in LDS at once (two workgroups
    // per CU); larger worlds take several passes
    // (as many as the largest world has, in eights: what the records do not take leaves room for a second TLAS block)
    p.bvhPassInst = std::min<uint32_t>(128u, std::max<uint32_t>(8u, (maxWorldInst + 7u) / 8u * 8u));
    p.bvhTile = 0;
    if (const char *dbg = std::getenv("MRX_BVH_TILE"))
        p.bvhTile = std::max(0, std::min(2, std::atoi(dbg)));
    // scenes with meshes large enough for a BLAS get the instantiation that classifies the
    // listed large triangles per strip (bvh.hip, CLS): close-ups of such meshes are where
    // long lists of large triangles come from
    p.bvhClassify = blas.nodes.empty() ? 0 : 1;
    if (const char *dbg = std::getenv("MRX_BVH_CLASSIFY"))
        p.bvhClassify = std::atoi(dbg) != 0;
    // (swept on the round's final kernel, 16 ... 4096: a plateau from 192 to 1024 -- only triangles that cover a good
    // part of the tile are worth the shared list and its barrier; profiles/r02_bvh_perf.txt)
    p.bvhSmallArea = 256;
    if (const char *dbg = std::getenv("MRX_BVH_SMALL_AREA"))
        p.bvhSmallArea = std::max(0, std::min(4096, std::atoi(dbg)));
    if (const char *dbg = std::getenv("MRX_BVH_PASS_INST"))
        p.bvhPassInst = std::min<uint32_t>(512u, std::max<uint32_t>(8u, (uint32_t)std::atoi(dbg) / 8u * 8u));
    // Views of several tiles whose world fits one TLAS pass: a workgroup renders a run of the view's
    // tiles over one TLAS build (bvh.hip).  As long a run as leaves one full generation of resident
    // workgroups (two per CU: 512 on 256 CUs) -- measured, profiles/r03_bvh_group_tiles.txt: 512 views of 256x256
    // cube+plane 155 -> 119 us at 16 tiles per group, 1024 views of 128x128 73 -> 62 us at 4, and
    // every shape loses as soon as the groups no longer fill the chip.
    p.bvhGroupTiles = 1;
    if (maxWorldInst <= p.bvhPassInst) {
        const uint32_t tw = p.bvhTile == 2 ? 32 : 64, thh = p.bvhTile == 0 ? 64 : 32;
        const uint32_t tpv = ((nfast + tw - 1) / tw) * ((nslow + thh - 1) / thh);
        uint32_t g = 1;
        while (g < 16u && g * 2u <= tpv && (uint64_t)nviews * ((tpv + 2u * g - 1) / (2u * g)) >= 2u * p.numCUs)
            g *= 2;
        p.bvhGroupTiles = std::max(1u, g);
        if (const char *dbg = std::getenv("MRX_BVH_GROUP_TILES"))
            p.bvhGroupTiles = (uint32_t)std::max(1, std::min((int)tpv, std::atoi(dbg)));
    }
    r.bvhGroupTilesGeneral = p.bvhGroupTiles;         // (the flat kernel chooses its own: chooseBvhGroups)
    mrx_info_t &inf = r.info;
    inf.num_worlds = cfg.num_worlds;
    inf.num_views = nviews;
    inf.num_instances = (uint32_t)instObj.size();
    inf.num_objects = (uint32_t)r.objFirst.size();
    inf.num_triangles = (uint32_t)tris.size();
    inf.num_materials = (uint32_t)allMats.size();
    inf.num_textures = (uint32_t)texDescs.size();
    inf.storage_fast = nfast;
    inf.storage_slow = nslow;
    inf.device_id = r.device;
    inf.kernel_variant = r.variant;
    inf.bvh_nodes = (uint32_t)blas.nodes.size();
    inf.bvh_depth = blas.maxDepth;
    inf.max_world_instances = maxWorldInst;
    inf.num_shards = 1;
    inf.bytes_per_step = (uint64_t)px * (4u * ((r.rgb.ptr ? 1u : 0u) + (r.depth.ptr ? 1u : 0u) + (r.normal.ptr ? 1u : 0u)) +
                                         (wantIds ? 4u : 0u)) +
                         (44ull + (r.instColor.ptr ? 4ull : 0ull) + (r.instMat.ptr ? 4ull : 0ull) +
                          (r.instLabel.ptr ? 4ull : 0ull)) * inf.num_instances +
                         28ull * nviews;
    return bindGeometry(r);
}
