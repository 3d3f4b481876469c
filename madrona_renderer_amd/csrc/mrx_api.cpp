// C-ABI implementation (include/mrx.h): creation and destruction, the step, setters and getters, buffers, info, timing
// and output placement.  HIP only -- no CPU rendering path.  Scene ingestion is scene.cpp, the post-render stages
// stages.cpp, the device threads of a multi-device renderer shards.cpp, the entries without a renderer host_tools.cpp.
#include "renderer.hpp"

#include <chrono>
#include <utility>

#include "boxes.hpp"
#include "observe.hpp"

// The output tensors of a renderer normally live in ONE allocation, rgb first.  A lane
// stores the same pixels of every tensor back to back, and when two tensors
// lie a multiple of 512 KiB apart those stores collide in the memory system
// (measured: a 64 MiB + 64 MiB render takes 24.1 us at distance = 0 mod 512 KiB
// and 22.5 us at 256 KiB mod 512 KiB, profiles/r01_placement.txt).  Separate
// hipMalloc blocks are 2 MiB-aligned -- the bad case -- and their physical
// distance is anybody's guess; inside one allocation the distance is ours:
// depth starts at phase 256 KiB of the 512 KiB period, ids at phase 64 KiB.
constexpr size_t kOutPeriod = 512u << 10;
static size_t outPhase(const char *env, size_t dflt)
{
    if (const char *dbg = std::getenv(env))
        return (size_t)std::atoll(dbg) << 10;
    return dflt;
}
// Which kind of candidate the placement search starts with: tensors of 64 MiB
// were reliably fast in one block, tensors of 256 MiB and 1 GiB one block each.
bool firstKindIsOneBlock(size_t px)
{
    if (const char *dbg = std::getenv("MRX_OUT_KIND"))      // "one" | "split": diagnostic override
        return dbg[0] == 'o';
    return px * 4 < (128ull << 20);
}

// Output selection (MRX_FLAG_NO_RGB / MRX_FLAG_NO_DEPTH): a tensor that is not selected is
// not allocated, and its slab drops out of the layout -- the first tensor present owns the block.
// Normals (MRX_FLAG_NORMALS): one more slab behind everything above -- every other tensor keeps its
// offset and phase -- at a phase of its own (MRX_OUT_SKEW_NORMAL_KB, 384 KiB: neither rgb's 0, depth's 256 nor the
// ids' 64; measured against 128 KiB, profiles/r12_normals_placement.txt: level on 64 MiB and 256 MiB tensors, and on
// 1 GiB ones the four tensors reach a faster placement mode from it more often).
hipError_t allocOutputs(size_t px, bool wantRgb, bool wantDepth, bool wantIds, bool oneAllocation,
                        DevBuf<uint32_t> &rgb, DevBuf<float> &depth, DevBuf<int32_t> &ids,
                        bool wantNormal, DevBuf<uint32_t> &normal)
{
    const size_t depthPhase = outPhase("MRX_OUT_SKEW_DEPTH_KB", 256u << 10);
    const size_t idsPhase = outPhase("MRX_OUT_SKEW_IDS_KB", 64u << 10);
    const size_t normalPhase = outPhase("MRX_OUT_SKEW_NORMAL_KB", 384u << 10);
    if (!oneAllocation) {
        // One allocation per tensor, made back to back, the phases applied
        // inside the (2 MiB-aligned) blocks.  Whether that yields the intended
        // distance is up to the allocator -- this is the other kind of
        // candidate of the placement search: half-GiB outputs were only ever
        // fast this way, 128 MiB ones reliably only in one allocation.
        hipError_t e = wantRgb ? rgb.alloc(px) : hipSuccess;
        size_t gapBytes = 0;
        if (const char *dbg = std::getenv("MRX_OUT_GAP_MB"))    // diagnostic: a held allocation between the tensors
            gapBytes = (size_t)std::atoll(dbg) << 20;
        static std::vector<DevBuf<uint8_t>> heldGaps;            // (only ever filled by the diagnostic knob)
        auto gap = [&]() {
            DevBuf<uint8_t> sp;
            if (gapBytes && sp.alloc(gapBytes) == hipSuccess)
                heldGaps.push_back(sp);
        };
        if (e == hipSuccess && wantDepth) {
            if (wantRgb)
                gap();
            e = depth.alloc(px, depthPhase);
            depth.ptr = reinterpret_cast<float *>(static_cast<char *>(depth.base) + depthPhase);
        }
        if (e == hipSuccess && wantIds) {
            gap();
            e = ids.alloc(px, idsPhase);
            ids.ptr = reinterpret_cast<int32_t *>(static_cast<char *>(ids.base) + idsPhase);
        }
        if (e == hipSuccess && wantNormal) {
            gap();
            e = normal.alloc(px, normalPhase);
            normal.ptr = reinterpret_cast<uint32_t *>(static_cast<char *>(normal.base) + normalPhase);
        }
        if (e != hipSuccess) {
            rgb.release(); depth.release(); ids.release(); normal.release();
        }
        return e;
    }
    // the first tensor present at offset 0; depth at phase 256 KiB of the period after the rgb slab, ids at
    // phase 64 KiB of the period after the slab before them
    const size_t tb = (px * 4 + kOutPeriod - 1) / kOutPeriod * kOutPeriod;
    const size_t depthOff = wantRgb ? tb + depthPhase : 0;
    const size_t idsOff = wantDepth ? depthOff + tb + kOutPeriod - (depthOff % kOutPeriod) + idsPhase
                                    : wantRgb ? tb + idsPhase : 0;
    const size_t end = (wantIds ? idsOff : wantDepth ? depthOff : 0) + px * 4;
    // normals: at their phase of the first period that starts behind the last slab
    const size_t normalOff = (end + kOutPeriod - 1) / kOutPeriod * kOutPeriod + normalPhase;
    const size_t total = wantNormal ? normalOff + px * 4 : end;
    const char *how = std::getenv("MRX_OUT_ALLOC");
    int dev = 0;
    (void)hipGetDevice(&dev);
    auto own = [&](auto &buf) {
        return (how && how[0] == 'v') ? buf.allocVmm(px, total - px * 4, dev) : buf.alloc(px, total - px * 4);
    };
    const hipError_t e = wantRgb ? own(rgb) : wantDepth ? own(depth) : own(ids);
    if (e != hipSuccess)
        return e;
    char *base = static_cast<char *>(wantRgb ? rgb.base : wantDepth ? depth.base : ids.base);
    if (wantRgb && wantDepth)
        depth.view(base + depthOff, px);
    if (wantIds && (wantRgb || wantDepth))
        ids.view(base + idsOff, px);
    if (wantNormal)
        normal.view(base + normalOff, px);
    return hipSuccess;
}

hipError_t mrx_renderer::launchRender()
{
    // the parity workgroup 0 reported some launches ago (the word is written by the
    // device without synchronisation: any value it ever held is a valid prediction)
    if (xcdPhaseForced >= 0)
        params.xcdPhase = (uint32_t)xcdPhaseForced;
    else if (xccHost)
        params.xcdPhase = *(volatile uint32_t *)xccHost & 1u;
    // (the report is a write over PCIe: asked for in the first launches and then in
    // every 32nd -- the phase of a queue changes rarely)
    ++launches;
    params.xccReport = (xccDev && (launches <= 4 || (launches & 31u) == 0)) ? xccDev : nullptr;
    if (useBvh) {
        lastEntry = mrx::kEntryBvh;
        return mrx::launchBvh(params, stream, &lastForm);
    }
    return mrx::launchRaster(params, info.max_world_triangles, variant, stream, &lastEntry, &lastForm);
}

mrx_renderer::~mrx_renderer()
{
    stopShardWorkers(shardSet);
    for (mrx_renderer *sh : shards)
        delete sh;
    if (!shards.empty())
        return;
    (void)hipSetDevice(device);
    tris.release(); triMats.release(); textures.release(); texels.release();
    viewTris.release(); viewTriCount.release();
    instPos.release(); instRot.release(); instScale.release();
    camPos.release(); camRot.release(); instObj.release(); instColor.release(); instMat.release();
    instLabel.release();
    matTable.release();
    projDev.release();
    lightDev.release();
    if (projStage)
        (void)hipHostFree(projStage);
    if (lightStage)
        (void)hipHostFree(lightStage);
    if (projEv)
        (void)hipEventDestroy(projEv);
    if (matStage)
        (void)hipHostFree(matStage);
    if (matEv)
        (void)hipEventDestroy(matEv);
    if (labelStage)
        (void)hipHostFree(labelStage);
    if (labelEv)
        (void)hipEventDestroy(labelEv);
    poseBlock.release(); geomBlock.release();
    rgb.release(); depth.release(); ids.release(); normal.release(); stamps.release();
    outRgb.release(); outDepth.release(); outIds.release(); outNormal.release();
    position.release();
    boxes.release();
    obs.release(); obsReset.release();
    releaseAttached(*this);
    if (xccHost) (void)hipHostFree(xccHost);
    bvhNodes.release(); bvhLeafTris.release(); worldInstStart.release();
    viewWorld.release(); instKBase.release(); objInfo.release();
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
}

int wantsShard(const char *what)
{
    return fail(MRX_E_UNSUPPORTED, std::string(what) + ": this renderer spans several devices -- "
                                   "address one shard (mrx_shard / mrx_buffer_shard)");
}

int infoFull(mrx_renderer *r, mrx_info_t *out)
{
    if (!r || !out)
        return fail(MRX_E_INVALID, "null argument");
    if (!r->shards.empty()) {
        // the shards share the scene: counts of what is per world add up, the rest is shard 0's
        mrx_info_t sum = r->shards[0]->info;
        for (size_t i = 1; i < r->shards.size(); ++i) {
            const mrx_info_t &o = r->shards[i]->info;
            sum.num_worlds += o.num_worlds;
            sum.num_views += o.num_views;
            sum.num_instances += o.num_instances;
            sum.bytes_per_step += o.bytes_per_step;
            sum.max_world_triangles = std::max(sum.max_world_triangles, o.max_world_triangles);
            sum.max_world_instances = std::max(sum.max_world_instances, o.max_world_instances);
            sum.render_path = std::max(sum.render_path, o.render_path);
        }
        sum.num_shards = (uint32_t)r->shards.size();
        *out = sum;
        return MRX_OK;
    }
    *out = r->info;
    return MRX_OK;
}

extern "C" {

int mrx_abi_version(void) { return MRX_ABI_VERSION; }

const char *mrx_last_error(void) { return g_err.c_str(); }

// the renderers that hold views [first, first + count) of the job, with the first job view of each
static std::vector<std::pair<mrx_renderer *, uint32_t>> viewOwners(mrx_renderer *r)
{
    std::vector<std::pair<mrx_renderer *, uint32_t>> out;
    uint32_t base = 0;
    if (r->shards.empty()) {
        out.emplace_back(r, 0u);
        return out;
    }
    for (mrx_renderer *sh : r->shards) {
        out.emplace_back(sh, base);
        base += (uint32_t)sh->proj.size();
    }
    return out;
}

static int viewRange(mrx_renderer *r, uint32_t first, uint32_t count, const void *ptr)
{
    size_t total = 0;
    for (const auto &o : viewOwners(r))
        total += o.first->proj.size();
    if ((uint64_t)first + count > total)
        return fail(MRX_E_INVALID, "views [" + std::to_string(first) + ", " + std::to_string((uint64_t)first + count) +
                                       ") outside the renderer's " + std::to_string(total));
    if (count && !ptr)
        return fail(MRX_E_INVALID, "null projection array");
    return MRX_OK;
}

int mrx_set_view_projection(mrx_renderer *r, uint32_t first_view, uint32_t count, const mrx_projection *proj)
{
    if (const int src = settle(r))
        return src;
    if (!r)
        return fail(MRX_E_INVALID, "null renderer");
    int rc = viewRange(r, first_view, count, proj);
    if (rc != MRX_OK)
        return rc;
    // every value first: a bad one leaves every view as it was
    const bool rt = r->mode == MRX_MODE_RAYTRACER;
    std::vector<mrx_projection> resolved(count);
    for (uint32_t i = 0; i < count; ++i) {
        mrx::ViewProj vp;
        if (projectionConstants(16, 16, rt, proj[i], vp, &resolved[i]) != MRX_OK)
            return fail(MRX_E_INVALID, "view " + std::to_string((uint64_t)first_view + i) + ": " + g_err);
    }
    for (const auto &o : viewOwners(r)) {
        mrx_renderer &sh = *o.first;
        const uint64_t lo = std::max<uint64_t>(first_view, o.second);
        const uint64_t hi = std::min<uint64_t>((uint64_t)first_view + count, (uint64_t)o.second + sh.proj.size());
        if (lo >= hi)
            continue;
        for (uint64_t v = lo; v < hi; ++v)
            sh.proj[v - o.second] = resolved[v - first_view];
        rc = applyViewTables(sh);
        if (rc != MRX_OK)
            return rc;
    }
    return MRX_OK;
}

int mrx_view_projection(mrx_renderer *r, uint32_t first_view, uint32_t count, mrx_projection *out)
{
    if (const int src = settle(r))
        return src;
    if (!r)
        return fail(MRX_E_INVALID, "null renderer");
    const int rc = viewRange(r, first_view, count, out);
    if (rc != MRX_OK)
        return rc;
    for (const auto &o : viewOwners(r))
        for (size_t v = 0; v < o.first->proj.size(); ++v) {
            const uint64_t job = (uint64_t)o.second + v;
            if (job >= first_view && job < (uint64_t)first_view + count)
                out[job - first_view] = o.first->proj[v];
        }
    return MRX_OK;
}

// the renderers that hold the worlds of the job, with the first job world of each
static std::vector<std::pair<mrx_renderer *, uint32_t>> worldOwners(mrx_renderer *r)
{
    std::vector<std::pair<mrx_renderer *, uint32_t>> out;
    if (r->shards.empty()) {
        out.emplace_back(r, 0u);
        return out;
    }
    for (size_t i = 0; i < r->shards.size(); ++i)
        out.emplace_back(r->shards[i], r->shardFirstWorld[i]);
    return out;
}

static int worldRange(mrx_renderer *r, uint32_t first, uint32_t count, const void *ptr)
{
    size_t total = 0;
    for (const auto &o : worldOwners(r))
        total += o.first->lights.size();
    if ((uint64_t)first + count > total)
        return fail(MRX_E_INVALID, "worlds [" + std::to_string(first) + ", " + std::to_string((uint64_t)first + count) +
                                       ") outside the renderer's " + std::to_string(total));
    if (count && !ptr)
        return fail(MRX_E_INVALID, "null light array");
    return MRX_OK;
}

int mrx_set_world_light(mrx_renderer *r, uint32_t first_world, uint32_t count, const mrx_light *lights)
{
    if (const int src = settle(r))
        return src;
    if (!r)
        return fail(MRX_E_INVALID, "null renderer");
    int rc = worldRange(r, first_world, count, lights);
    if (rc != MRX_OK)
        return rc;
    // every value first: a bad one leaves every world as it was
    for (uint32_t i = 0; i < count; ++i) {
        mrx::ViewLight vl;
        if (lightConstants(lights[i], vl) != MRX_OK)
            return fail(MRX_E_INVALID, "world " + std::to_string((uint64_t)first_world + i) + ": " + g_err);
    }
    for (const auto &o : worldOwners(r)) {
        mrx_renderer &sh = *o.first;
        const uint64_t lo = std::max<uint64_t>(first_world, o.second);
        const uint64_t hi = std::min<uint64_t>((uint64_t)first_world + count, (uint64_t)o.second + sh.lights.size());
        if (lo >= hi)
            continue;
        for (uint64_t w = lo; w < hi; ++w)
            sh.lights[w - o.second] = lights[w - first_world];
        rc = applyViewTables(sh);
        if (rc != MRX_OK)
            return rc;
    }
    return MRX_OK;
}

int mrx_world_light(mrx_renderer *r, uint32_t first_world, uint32_t count, mrx_light *out)
{
    if (const int src = settle(r))
        return src;
    if (!r)
        return fail(MRX_E_INVALID, "null renderer");
    const int rc = worldRange(r, first_world, count, out);
    if (rc != MRX_OK)
        return rc;
    for (const auto &o : worldOwners(r))
        for (size_t w = 0; w < o.first->lights.size(); ++w) {
            const uint64_t job = (uint64_t)o.second + w;
            if (job >= first_world && job < (uint64_t)first_world + count)
                out[job - first_world] = o.first->lights[w];
        }
    return MRX_OK;
}

// the renderers that hold the instance rows of the job, with the first job row of each
static std::vector<std::pair<mrx_renderer *, uint64_t>> rowOwners(mrx_renderer *r)
{
    std::vector<std::pair<mrx_renderer *, uint64_t>> out;
    uint64_t base = 0;
    if (r->shards.empty()) {
        out.emplace_back(r, 0u);
        return out;
    }
    for (mrx_renderer *sh : r->shards) {
        out.emplace_back(sh, base);
        base += sh->info.num_instances;
    }
    return out;
}

// One int32 column of the instance rows with a host-side setter: the device slice, the pinned staging of the setter (one
// word per row), the event behind its last copy, and the words of its error messages.
struct RowColumn {
    DevBuf<int32_t> mrx_renderer::*dev;
    int32_t *mrx_renderer::*stage;
    hipEvent_t mrx_renderer::*ev;
    bool mrx_renderer::*pending;
    const char *nullMsg, *noneMsg;
};
static const RowColumn kMaterialColumn = {
    &mrx_renderer::instMat, &mrx_renderer::matStage, &mrx_renderer::matEv, &mrx_renderer::matCopyPending, "null material array",
    "no instance materials: this renderer was created without MRX_FLAG_INSTANCE_MATERIALS" };
static const RowColumn kLabelColumn = {
    &mrx_renderer::instLabel, &mrx_renderer::labelStage, &mrx_renderer::labelEv, &mrx_renderer::labelCopyPending,
    "null label array", "no instance labels: this renderer was created without MRX_FLAG_INSTANCE_LABELS" };

static int rowRange(mrx_renderer *r, const RowColumn &col, uint32_t first, uint32_t count, const void *ptr)
{
    uint64_t total = 0;
    bool column = true;
    for (const auto &o : rowOwners(r)) {
        total += o.first->info.num_instances;
        column = column && (o.first->*col.dev).ptr;
    }
    if (!ptr)
        return fail(MRX_E_INVALID, col.nullMsg);
    if ((uint64_t)first + count > total)
        return fail(MRX_E_INVALID, "rows [" + std::to_string(first) + ", " + std::to_string((uint64_t)first + count) +
                                       ") outside the renderer's " + std::to_string(total));
    if (!column)
        return fail(MRX_E_UNSUPPORTED, col.noneMsg);
    return MRX_OK;
}

static int setRows(mrx_renderer *r, const RowColumn &col, uint32_t first_row, uint32_t count, const int32_t *values)
{
    if (const int src = settle(r))
        return src;
    if (!r)
        return fail(MRX_E_INVALID, "null renderer");
    const int rc = rowRange(r, col, first_row, count, values);
    if (rc != MRX_OK)
        return rc;
    for (const auto &o : rowOwners(r)) {
        mrx_renderer &sh = *o.first;
        const uint64_t lo = std::max<uint64_t>(first_row, o.second);
        const uint64_t hi = std::min<uint64_t>((uint64_t)first_row + count, o.second + sh.info.num_instances);
        if (lo >= hi)
            continue;
        // (through the pinned staging: the copy runs on the stream behind every render enqueued so far, and the caller's
        // array is free when the call returns; the staging is overwritten only once the last copy from it has run)
        MRX_HIP(hipSetDevice(sh.device));
        if (sh.*col.pending)
            MRX_HIP(hipEventSynchronize(sh.*col.ev));
        int32_t *stage = sh.*col.stage + (lo - o.second);
        std::memcpy(stage, values + (lo - first_row), (hi - lo) * sizeof(int32_t));
        MRX_HIP(hipMemcpyAsync((sh.*col.dev).ptr + (lo - o.second), stage, (hi - lo) * sizeof(int32_t), hipMemcpyHostToDevice,
                               sh.stream));
        MRX_HIP(hipEventRecord(sh.*col.ev, sh.stream));
        sh.*col.pending = true;
    }
    return MRX_OK;
}

static int getRows(mrx_renderer *r, const RowColumn &col, uint32_t first_row, uint32_t count, int32_t *out)
{
    if (const int src = settle(r))
        return src;
    if (!r)
        return fail(MRX_E_INVALID, "null renderer");
    const int rc = rowRange(r, col, first_row, count, out);
    if (rc != MRX_OK)
        return rc;
    for (const auto &o : rowOwners(r)) {
        mrx_renderer &sh = *o.first;
        const uint64_t lo = std::max<uint64_t>(first_row, o.second);
        const uint64_t hi = std::min<uint64_t>((uint64_t)first_row + count, o.second + sh.info.num_instances);
        if (lo >= hi)
            continue;
        MRX_HIP(hipSetDevice(sh.device));
        MRX_HIP(hipStreamSynchronize(sh.stream));
        MRX_HIP(hipMemcpy(out + (lo - first_row), (sh.*col.dev).ptr + (lo - o.second), (hi - lo) * sizeof(int32_t),
                          hipMemcpyDeviceToHost));
    }
    return MRX_OK;
}

int mrx_set_instance_materials(mrx_renderer *r, uint32_t first_row, uint32_t count, const int32_t *materials)
{
    return setRows(r, kMaterialColumn, first_row, count, materials);
}

int mrx_instance_materials(mrx_renderer *r, uint32_t first_row, uint32_t count, int32_t *out)
{
    return getRows(r, kMaterialColumn, first_row, count, out);
}

int mrx_set_instance_labels(mrx_renderer *r, uint32_t first_row, uint32_t count, const int32_t *labels)
{
    return setRows(r, kLabelColumn, first_row, count, labels);
}

int mrx_instance_labels(mrx_renderer *r, uint32_t first_row, uint32_t count, int32_t *out)
{
    return getRows(r, kLabelColumn, first_row, count, out);
}

int mrx_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        return 0;
    return n;
}

// Where LARGE output tensors land in HBM matters on some boxes: with tensors of
// 256 MiB and more the same launch streams its stores ~20 % faster into some
// allocations than into others, steadily for the life of the allocation
// (profiles/r02_placement.txt).  Nothing visible from user space
// predicts which -- not the layout, not the distance between the tensors, not
// the address, not the XCD phase of the queue; some boxes offer no fast
// allocation at all -- so for such outputs a few candidates are allocated one
// after another (alternately all tensors in one block and one block per
// tensor), each timed with a few renders, and the fastest kept.  Bounded: at
// most two candidates (the best so far and the current one) plus one small
// spacer are alive at any time, two are tried by default (round 3: a pure
// two-tensor fill shows the same modes from allocation to allocation --
// profiles/r03_placement.txt -- so this is a property of the platform, not
// something a longer search could fix), and nothing is tried when two more
// copies of the outputs would not fit a quarter of the free memory.  Outputs below 256 MiB (every 64x64 batch up to 8192 views) are laid
// out deterministically in one block -- depth at phase 256 KiB of the 512 KiB
// period -- and need no search (what looked like a placement lottery for them
// in round 1 was the XCD phase of the stream: raster.hip, xcdPhase).
// MRX_PLACEMENT_TRIES=1 switches the search off.
static int choosePlacement(mrx_renderer *r)
{
    const bool wantRgb = r->rgb.ptr != nullptr, wantDepth = r->depth.ptr != nullptr;
    const bool wantIds = r->ids.ptr != nullptr, wantNormal = r->normal.ptr != nullptr;
    const size_t px = wantRgb ? r->rgb.count : r->depth.count;
    // (keyed on the bytes actually allocated: an output that is not selected has no tensor)
    const size_t bytes = px * 4 * ((wantRgb ? 1 : 0) + (wantDepth ? 1 : 0) + (wantIds ? 1 : 0) + (wantNormal ? 1 : 0));
    int maxTries = (bytes >= (256ull << 20) && bytes <= (16ull << 30)) ? 2 : 1;
    if (const char *dbg = std::getenv("MRX_PLACEMENT_TRIES"))
        maxTries = std::max(1, std::min(16, std::atoi(dbg)));
    if (maxTries > 1) {
        size_t freeB = 0, totalB = 0;
        if (hipMemGetInfo(&freeB, &totalB) != hipSuccess || 2 * bytes + (256ull << 20) > freeB / 4) {
            (void)hipGetLastError();
            maxTries = 1;
        }
    }
    if (maxTries <= 1)
        return MRX_OK;
    const bool trace = std::getenv("MRX_PLACEMENT_TRACE") != nullptr;
    struct Cand { DevBuf<uint32_t> rgb; DevBuf<float> depth; DevBuf<int32_t> ids; DevBuf<uint32_t> normal; float us = 0.0f; };
    auto bind = [&](const Cand &c) {
        r->params.rgb = c.rgb.ptr;
        r->params.depth = c.depth.ptr;
        r->params.ids = wantIds ? c.ids.ptr : nullptr;
        r->params.normal = c.normal.ptr;
    };
    auto freeCand = [](Cand &c) { c.rgb.release(); c.depth.release(); c.ids.release(); c.normal.release(); };
    auto launch = [&]() { return r->launchRender(); };     // (the sample render alone: the resolve reads whatever is kept)
    auto timeBatch = [&](int n, float &ms) -> hipError_t {
        hipError_t e = hipEventRecord(r->ev0, r->stream);
        for (int i = 0; i < n && e == hipSuccess; ++i)
            e = launch();
        if (e == hipSuccess) e = hipEventRecord(r->ev1, r->stream);
        if (e == hipSuccess) e = hipEventSynchronize(r->ev1);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, r->ev0, r->ev1);
        return e;
    };
    Cand best;
    best.rgb = r->rgb; best.depth = r->depth; best.ids = r->ids; best.normal = r->normal;   // what buildScene allocated
    // a render takes ~0.1 - 1 ms here: batches of ~0.5 ms, ~40 ms of warm-up (clocks)
    hipError_t st = hipSuccess;                   // first error; the cleanup below always runs
    bind(best);
    float one = 0.0f;
    st = launch();
    if (st == hipSuccess) st = timeBatch(1, one);
    one = std::max(one, 1e-3f);
    const int batch = std::max(3, std::min(64, (int)(0.5f / one)));
    float scratch = 0.0f;
    if (st == hipSuccess) st = timeBatch(std::max(8, std::min(4000, (int)(40.0f / one))), scratch);
    auto measure = [&](Cand &c) -> hipError_t {
        bind(c);
        hipError_t e = launch();
        float bestMs = 1e30f, ms = 0.0f;
        for (int rep = 0; rep < 3 && e == hipSuccess; ++rep) {
            e = timeBatch(batch, ms);
            bestMs = std::min(bestMs, ms);
        }
        c.us = bestMs / (float)batch * 1000.0f;
        return e;
    };
    if (st == hipSuccess) st = measure(best);
    float tmax = best.us;
    r->placementUs.push_back(best.us);
    std::string log;
    char buf[64];
    std::snprintf(buf, sizeof buf, " %.2f", best.us);
    log += buf;
    for (int k = 1; k < maxTries && st == hipSuccess; ++k) {
        // a spacer of 2 ... 128 MiB steps the next candidate on in the address space;
        // the best candidate so far stays allocated, so the new one cannot reuse its block
        DevBuf<uint8_t> sp;
        if (sp.alloc((size_t)(2 * ((k * 37) % 64 + 1)) << 20) != hipSuccess)
            (void)hipGetLastError();
        Cand c;
        const hipError_t ae = allocOutputs(px, wantRgb, wantDepth, wantIds, ((k & 1) == 0) == firstKindIsOneBlock(px),
                                           c.rgb, c.depth, c.ids, wantNormal, c.normal);
        sp.release();
        if (ae != hipSuccess) {
            (void)hipGetLastError();                  // out of memory: make do with what there is
            break;
        }
        st = measure(c);
        if (st != hipSuccess) {
            freeCand(c);
            break;
        }
        std::snprintf(buf, sizeof buf, " %.2f", c.us);
        log += buf;
        r->placementUs.push_back(c.us);
        tmax = std::max(tmax, c.us);
        if (c.us < best.us) {
            freeCand(best);
            best = c;
        } else {
            freeCand(c);
        }
        // the two modes lie 5 - 7 % (outputs below 256 MiB) to ~20 % apart; candidates of
        // one mode scatter by +-0.5 % (small) to +-4 % (large)
        if (best.us <= (bytes < (256ull << 20) ? 0.965f : 0.88f) * tmax)
            break;                                    // a fast placement
    }
    if (trace)
        std::fprintf(stderr, "mrx: output placement, us/render:%s -> %.2f (rgb %p depth %p)\n", log.c_str(),
                     best.us, (void *)best.rgb.ptr, (void *)best.depth.ptr);
    r->rgb = best.rgb; r->depth = best.depth; r->ids = best.ids; r->normal = best.normal;
    r->placementKeptUs = best.us;
    bind(best);
    if (st != hipSuccess)
        return fail(MRX_E_HIP, std::string("output placement: ") + hipGetErrorString(st));
    return MRX_OK;
}

// one renderer on one device (mrx_create proper, or one shard of a multi-device renderer)
static int createOne(const mrx_config &cfg, mrx_renderer **out)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(MRX_E_NO_DEVICE,
                    "no HIP device: this library renders on MI355X only (no CPU path)");
    if (cfg.gpu_id < 0 || cfg.gpu_id >= ndev)
        return fail(MRX_E_NO_DEVICE, "gpu_id " + std::to_string(cfg.gpu_id) +
                                         " out of range (" + std::to_string(ndev) + " devices)");
    MRX_HIP(hipSetDevice(cfg.gpu_id));

    mrx_renderer *r = new mrx_renderer();
    r->device = cfg.gpu_id;
    r->stream = (hipStream_t)cfg.stream;
    r->mode = cfg.render_mode;
    r->flags = cfg.flags;
    r->variant = cfg.kernel_variant;
    // S12: a supersampled renderer is the renderer of the sample image -- buildScene sees ss * W x ss * H views, and
    // everything it decides (constants, dispatch, placement) is that renderer's -- plus the native tensors behind it
    decodeStageFlags(cfg.flags, *r);
    mrx_config sampleCfg = cfg;
    sampleCfg.view_width *= r->ss;
    sampleCfg.view_height *= r->ss;
    int rc = buildScene(sampleCfg, *r);
    if (rc == MRX_OK)
        rc = allocStages(*r);
    if (rc == MRX_OK) {
        hipError_t e = hipEventCreate(&r->ev0);
        if (e == hipSuccess) e = hipEventCreate(&r->ev1);
        if (e != hipSuccess)
            rc = fail(MRX_E_HIP, std::string("hipEventCreate: ") + hipGetErrorString(e));
    }
    if (rc == MRX_OK)
        rc = choosePlacement(r);
    // the reference renders the first frame inside the constructor (mgr.cpp:524)
    if (rc == MRX_OK)
        rc = mrx_step(r);
    if (rc == MRX_OK)
        rc = mrx_sync(r);
    if (rc != MRX_OK) {
        delete r;
        return rc;
    }
    *out = r;
    return MRX_OK;
}

// contiguous world range of shard i of n: sizes differ by at most one (scenes.shard_range)
static uint32_t shardFirstWorld(uint32_t numWorlds, uint32_t i, uint32_t n)
{
    const uint32_t base = numWorlds / n, rem = numWorlds % n;
    return i * base + std::min(i, rem);
}

int mrx_create(const mrx_config *cfgIn, mrx_renderer **out)
{
    if (!cfgIn || !out)
        return fail(MRX_E_INVALID, "null argument");
    *out = nullptr;
    // ABI 2 callers pass the struct without its trailing ABI 3 fields: those read as zero
    // (ABI 4 callers: the struct without camera_projections, MRX_CONFIG_V4_SIZE -- every camera the default -- or
    // without world_lights, MRX_CONFIG_V4_PROJ_SIZE -- every world the default light -- or without instance_colors,
    // MRX_CONFIG_V4_LIGHT_SIZE -- no initial colours)
    if (cfgIn->struct_size != sizeof(mrx_config) && cfgIn->struct_size != MRX_CONFIG_V2_SIZE &&
        cfgIn->struct_size != MRX_CONFIG_V4_SIZE && cfgIn->struct_size != MRX_CONFIG_V4_PROJ_SIZE &&
        cfgIn->struct_size != MRX_CONFIG_V4_LIGHT_SIZE)
        return fail(MRX_E_INVALID, "mrx_config size mismatch (ABI)");
    mrx_config full;
    std::memset(&full, 0, sizeof full);
    std::memcpy(&full, cfgIn, cfgIn->struct_size);
    full.struct_size = sizeof(mrx_config);
    if (full.reserved0 != 0)
        return fail(MRX_E_INVALID, "mrx_config.reserved0 must be zero");
    if (full.instance_colors)
        full.flags |= MRX_FLAG_INSTANCE_COLORS;
    const mrx_config *cfg = &full;
    if (cfg->render_mode != MRX_MODE_RASTERIZER && cfg->render_mode != MRX_MODE_RAYTRACER)
        return fail(MRX_E_INVALID, "bad render_mode");
    if (cfg->view_width == 0 || cfg->view_height == 0 || cfg->view_width > 16384 ||
        cfg->view_height > 16384)
        return fail(MRX_E_INVALID, "bad view size");
    {
        const uint64_t s = supersampleOf(cfg->flags);
        if (s * cfg->view_width > 16384 || s * cfg->view_height > 16384)
            return fail(MRX_E_INVALID, "bad view size: the sample image of supersampling factor " + std::to_string(s) +
                                           " is larger than 16384 pixels a side");
    }
    if (cfg->num_worlds && !cfg->worlds)
        return fail(MRX_E_INVALID, "worlds is null");
    if ((cfg->num_instances && !cfg->instances) || (cfg->num_cameras && !cfg->cameras) ||
        (cfg->num_asset_paths && !cfg->asset_paths) || (cfg->num_materials && !cfg->materials) ||
        (cfg->num_textures && !cfg->texture_paths))
        return fail(MRX_E_INVALID, "a table pointer is null while its count is not zero");
    if (cfg->geo.num_meshes &&
        (!cfg->geo.vertices || !cfg->geo.uvs || !cfg->geo.indices || !cfg->geo.mesh_vertex_offsets ||
         !cfg->geo.mesh_index_offsets || !cfg->geo.mesh_materials))
        return fail(MRX_E_INVALID, "raw geometry arrays are null while num_meshes is not zero");
    if (cfg->kernel_variant < 0 || cfg->kernel_variant >= mrx::kNumVariants)
        return fail(MRX_E_INVALID, "bad kernel_variant");
    if ((cfg->flags & MRX_FLAG_NO_RGB) && (cfg->flags & MRX_FLAG_NO_DEPTH))
        return fail(MRX_E_INVALID, "no output selected: MRX_FLAG_NO_RGB and MRX_FLAG_NO_DEPTH together leave "
                                   "neither rgb nor depth to render");
    if (positionsOf(cfg->flags) && (cfg->flags & MRX_FLAG_NO_DEPTH))
        return fail(MRX_E_INVALID, "MRX_FLAG_POSITIONS and MRX_FLAG_NO_DEPTH together: the position output is computed "
                                   "from the depth tensor, which an rgb-only renderer does not have");
    // the pixels of the job at the native size (Raytracer storage is square), against the limit of each stage that is on
    uint64_t nativePx = 0;
    for (uint32_t w = 0; w < cfg->num_worlds; ++w)
        nativePx += cfg->worlds[w].num_cameras;
    nativePx *= (uint64_t)cfg->view_width * (cfg->render_mode == MRX_MODE_RAYTRACER ? cfg->view_width : cfg->view_height);
    if (const uint32_t k = boxLabelsOf(cfg->flags)) {
        if (k > mrx::kBoxMaxLabels)
            return fail(MRX_E_INVALID, "MRX_FLAG_BOX_LABELS: " + std::to_string(k) + " labels, more than 1024");
        if (cfg->flags & MRX_FLAG_VISIBILITY_IDS)
            return fail(MRX_E_INVALID, "MRX_FLAG_BOX_LABELS and MRX_FLAG_VISIBILITY_IDS together: the box stage reads "
                                       "the segmask, and the ids tensor of this renderer holds visibility ids");
        if (cfg->render_mode == MRX_MODE_RASTERIZER && !(cfg->flags & MRX_FLAG_INSTANCE_LABELS))
            return fail(MRX_E_INVALID, "MRX_FLAG_BOX_LABELS in Rasterizer mode needs MRX_FLAG_INSTANCE_LABELS: the box "
                                       "stage reads the segmask, which this renderer does not have");
        // (mrx_info's storage is the native size: the resolved tensor is what the stage reads)
        if (nativePx > mrx::kBoxMaxPixels)
            return fail(MRX_E_INVALID, "MRX_FLAG_BOX_LABELS: more than 2^32 - 1 native pixels");
    }
    if (const uint32_t layout = obsLayoutOf(cfg->flags)) {
        if (mrx::observeChannels(layout) == 0)
            return fail(MRX_E_INVALID, "MRX_FLAG_OBSERVATIONS: layout " + std::to_string(layout) + " is not one of "
                                       "MRX_OBS_RGB ... MRX_OBS_YD (1 ... 5)");
        if (mrx::observeReadsColour(layout) && (cfg->flags & MRX_FLAG_NO_RGB))
            return fail(MRX_E_INVALID, "MRX_FLAG_OBSERVATIONS with a colour layout and MRX_FLAG_NO_RGB together: the "
                                       "observation stage reads the rgb tensor, which a depth-only renderer does not have");
        if (mrx::observeReadsDepth(layout) && (cfg->flags & MRX_FLAG_NO_DEPTH))
            return fail(MRX_E_INVALID, "MRX_FLAG_OBSERVATIONS with a depth layout and MRX_FLAG_NO_DEPTH together: the "
                                       "observation stage reads the depth tensor, which an rgb-only renderer does not have");
        // (as the unprojection stage limits it: mrx_info's storage is the native size)
        if (nativePx > mrx::kObserveMaxPixels)
            return fail(MRX_E_INVALID, "MRX_FLAG_OBSERVATIONS: more than 2^32 - 1 native pixels");
    } else if (cfg->flags & MRX_FLAG_OBS_MASK) {
        return fail(MRX_E_INVALID, "MRX_FLAG_OBSERVATIONS: element type or stack bits without a layout");
    }
    if (cfg->max_instances_per_world > (1u << 20))
        return fail(MRX_E_INVALID, "max_instances_per_world out of range");
    if (cfg->camera_projections)
        for (uint32_t c = 0; c < cfg->num_cameras; ++c) {
            mrx::ViewProj vp;
            const bool rt = cfg->render_mode == MRX_MODE_RAYTRACER;
            if (projectionConstants(cfg->view_width, rt ? cfg->view_width : cfg->view_height, rt,
                                    cfg->camera_projections[c], vp) != MRX_OK)
                return fail(MRX_E_INVALID, "camera " + std::to_string(c) + ": " + g_err);
        }
    if (cfg->world_lights)
        for (uint32_t w = 0; w < cfg->num_worlds; ++w) {
            mrx::ViewLight vl;
            if (lightConstants(cfg->world_lights[w], vl) != MRX_OK)
                return fail(MRX_E_INVALID, "world " + std::to_string(w) + ": " + g_err);
        }
    if (cfg->num_devices > 1 && !cfg->device_ids)
        return fail(MRX_E_INVALID, "device_ids is null while num_devices is not zero");
    if (cfg->num_devices > 64)
        return fail(MRX_E_INVALID, "more than 64 devices");
    if (cfg->num_devices > 1 && cfg->num_devices > cfg->num_worlds)
        return fail(MRX_E_INVALID, "more devices (" + std::to_string(cfg->num_devices) + ") than worlds (" +
                                       std::to_string(cfg->num_worlds) + "): a shard would own no world");
    if (cfg->num_devices <= 1) {
        if (cfg->num_devices == 1 && cfg->device_ids)
            full.gpu_id = cfg->device_ids[0];
        full.num_devices = 0;
        full.device_ids = nullptr;
        return createOne(full, out);
    }
    // ---- one shard per listed device, each a renderer of its own over a contiguous world range
    if (cfg->stream)
        return fail(MRX_E_INVALID, "a renderer of several devices launches on each device's null stream: "
                                   "mrx_config.stream must be null (mrx_set_stream on a shard sets its stream)");
    mrx_renderer *top = new mrx_renderer();
    top->mode = cfg->render_mode;
    top->flags = cfg->flags;
    top->variant = cfg->kernel_variant;
    decodeStageFlags(cfg->flags, *top);
    top->device = cfg->device_ids[0];
    const uint32_t n = cfg->num_devices;
    for (uint32_t i = 0; i < n; ++i) {
        mrx_config sub = full;
        const uint32_t lo = shardFirstWorld(cfg->num_worlds, i, n), hi = shardFirstWorld(cfg->num_worlds, i + 1, n);
        sub.gpu_id = cfg->device_ids[i];
        sub.worlds = cfg->worlds ? cfg->worlds + lo : nullptr;
        sub.world_lights = cfg->world_lights ? cfg->world_lights + lo : nullptr;
        sub.num_worlds = hi - lo;
        sub.num_devices = 0;
        sub.device_ids = nullptr;
        mrx_renderer *sh = nullptr;
        const int rc = createOne(sub, &sh);
        if (rc != MRX_OK) {
            const std::string why = g_err;
            delete top;                               // (destroys the shards made so far)
            return fail(rc, "shard " + std::to_string(i) + " (device " + std::to_string(sub.gpu_id) + "): " + why);
        }
        sh->parent = top;
        top->shards.push_back(sh);
        top->shardFirstWorld.push_back(lo);
    }
    top->shardFirstWorld.push_back(cfg->num_worlds);
    startShardWorkers(top);
    *out = top;
    return MRX_OK;
}

void mrx_destroy(mrx_renderer *r)
{
    if (!r)
        return;
    stopShardWorkers(r->shardSet);
    for (mrx_renderer *sh : r->shards) {
        (void)hipSetDevice(sh->device);
        (void)hipStreamSynchronize(sh->stream);
    }
    if (r->shards.empty()) {
        (void)hipSetDevice(r->device);
        (void)hipStreamSynchronize(r->stream);
    }
    delete r;
}

int mrx_render(mrx_renderer *r)
{
    if (r && r->parent)                               // (a shard stepped on its own: behind what its renderer posted)
        if (const int src = settle(r))
            return src;
    if (!r)
        return fail(MRX_E_INVALID, "null renderer");
    // several devices: one launch each, enqueued concurrently by the shards' host threads
    // (shardsRun); on return every device has its kernel queued, nothing waits for a render
    if (!r->shards.empty())
        return shardsRun(r, kCmdRender);
    MRX_HIP(hipSetDevice(r->device));
    MRX_HIP(r->launch());
    return MRX_OK;
}

int mrx_step(mrx_renderer *r)
{
    // Manager::step = Step graph + Render graphs (mgr.cpp:177-185).  The Step
    // graph only advances a per-world clock nothing reads (sim.cpp:73-77) and
    // re-sorts static entities; what remains observable is the render.
    if (!r)
        return fail(MRX_E_INVALID, "null renderer");
    r->stepCount++;
    return mrx_render(r);
}

int mrx_sync(mrx_renderer *r)
{
    if (r && r->parent)
        if (const int src = settle(r))
            return src;
    if (!r)
        return fail(MRX_E_INVALID, "null renderer");
    if (!r->shards.empty())
        return shardsRun(r, kCmdSync);
    MRX_HIP(hipSetDevice(r->device));
    MRX_HIP(hipStreamSynchronize(r->stream));
    return MRX_OK;
}

void *mrx_stream(mrx_renderer *r) { return r ? (void *)r->stream : nullptr; }

static_assert(mrx::kEntryNone == MRX_ENTRY_NONE && mrx::kEntryGroupFast == MRX_ENTRY_GROUP_FAST &&
                  mrx::kEntryGroup == MRX_ENTRY_GROUP && mrx::kEntryChunked == MRX_ENTRY_CHUNKED &&
                  mrx::kEntryBrute == MRX_ENTRY_BRUTE && mrx::kEntryBvh == MRX_ENTRY_BVH,
              "raster.hpp RasterEntry and mrx.h MRX_ENTRY_* disagree");

int mrx_raster_entry(mrx_renderer *r)
{
    if (!r)
        return fail(MRX_E_INVALID, "null renderer");
    return r->shards.empty() ? r->lastEntry : r->shards[0]->lastEntry;
}

#define MRX_FORM_SAME(name, NAME) ((int)mrx::KernelForm::name == MRX_FORM_##NAME)
static_assert(MRX_FORM_SAME(Uniform, UNIFORM) && MRX_FORM_SAME(PV, PV) && MRX_FORM_SAME(PVL, PVL) && MRX_FORM_SAME(C, C) &&
                  MRX_FORM_SAME(PVLC, PVLC) && MRX_FORM_SAME(M, M) && MRX_FORM_SAME(PVLM, PVLM) && MRX_FORM_SAME(N, N) &&
                  MRX_FORM_SAME(NPV, NPV) && MRX_FORM_SAME(L, L) && MRX_FORM_SAME(LN, LN) && MRX_FORM_SAME(PVM, PVM),
              "raster.hpp KernelForm and mrx.h MRX_FORM_* disagree");
#undef MRX_FORM_SAME

int mrx_kernel_form(mrx_renderer *r, mrx_kernel_form_t *out)
{
    if (!r)
        return fail(MRX_E_INVALID, "null renderer");
    if (!out)
        return fail(MRX_E_INVALID, "null output");
    const mrx_renderer &sh = r->shards.empty() ? *r : *r->shards[0];
    out->form = sh.lastForm.form;
    out->slots = sh.lastForm.slots;
    return MRX_OK;
}

int mrx_bvh_launch(mrx_renderer *r, mrx_bvh_launch_t *out)
{
    if (!r)
        return fail(MRX_E_INVALID, "null renderer");
    if (!out)
        return fail(MRX_E_INVALID, "null output");
    const mrx_renderer &sh = r->shards.empty() ? *r : *r->shards[0];
    const mrx::BvhLaunchShape s = mrx::bvhLaunchShape(sh.params);
    mrx_bvh_launch_t o = {};
    o.kernel = !sh.useBvh ? MRX_BVH_KERNEL_NONE : s.flat ? MRX_BVH_KERNEL_FLAT : MRX_BVH_KERNEL_TILE;
    o.tile_w = s.tileW;
    o.tile_h = s.tileH;
    o.classify = s.classify;
    o.textured = s.textured;
    o.record_cap = s.recordCap;
    o.record_usable = s.recordUsable;
    o.tex_cap = s.texCap;
    o.big_cap = s.bigCap;
    o.pass_inst = s.passInst;
    o.group_views = s.groupViews;
    o.mixed = s.mixed;
    o.priority = s.priority;
    o.group_tiles = s.groupTiles;
    o.small_area = s.smallArea;
    o.workgroups = s.workgroups;
    *out = o;
    return MRX_OK;
}

int mrx_num_shards(mrx_renderer *r) { return !r ? 0 : r->shards.empty() ? 1 : (int)r->shards.size(); }

mrx_renderer *mrx_shard(mrx_renderer *r, int shard)
{
    if (!r || shard < 0 || shard >= mrx_num_shards(r)) {
        fail(MRX_E_INVALID, "no such shard");
        return nullptr;
    }
    return r->shards.empty() ? r : r->shards[shard];
}

void *mrx_buffer_shard(mrx_renderer *r, int shard, int which, int64_t dims[4], int *ndim, int *dtype,
                       int *device)
{
    mrx_renderer *sh = mrx_shard(r, shard);
    return sh ? mrx_buffer(sh, which, dims, ndim, dtype, device) : nullptr;
}

int64_t mrx_shard_split(uint32_t num_worlds, uint32_t shard, uint32_t num_shards)
{
    if (num_shards == 0 || shard > num_shards)
        return fail(MRX_E_INVALID, "bad shard");
    return (int64_t)shardFirstWorld(num_worlds, shard, num_shards);
}

int64_t mrx_shard_first_world(mrx_renderer *r, int shard)
{
    if (!r || shard < 0 || shard > mrx_num_shards(r))
        return fail(MRX_E_INVALID, "no such shard");
    if (r->shards.empty())
        return shard == 0 ? 0 : (int64_t)r->info.num_worlds;
    return (int64_t)r->shardFirstWorld[shard];
}

int mrx_refresh_objects(mrx_renderer *r)
{
    if (const int src = settle(r))
        return src;
    if (!r)
        return fail(MRX_E_INVALID, "null renderer");
    for (mrx_renderer *sh : r->shards) {
        const int rc = mrx_refresh_objects(sh);
        if (rc != MRX_OK)
            return rc;
    }
    if (!r->shards.empty())
        return MRX_OK;
    MRX_HIP(hipSetDevice(r->device));
    // renders in flight read the tables that are about to change
    MRX_HIP(hipStreamSynchronize(r->stream));
    std::vector<int32_t> live(r->boundObj.size());
    if (!live.empty())
        MRX_HIP(hipMemcpy(live.data(), r->instObj.ptr, live.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    // an id that names no object cannot be bound: refuse it before anything changes
    for (size_t i = 0; i < live.size(); ++i)
        if (live[i] >= 0 && (size_t)live[i] >= r->objFirst.size())
            return fail(MRX_E_INVALID, "instance row " + std::to_string(i) + " holds object id " +
                                           std::to_string(live[i]) + ", the scene has " +
                                           std::to_string(r->objFirst.size()) + " objects");
    bool changed = false;
    for (size_t i = 0; i < live.size(); ++i)
        if (live[i] >= 0 && live[i] != r->boundObj[i]) {
            r->boundObj[i] = live[i];
            changed = true;
        }
    if (!changed)
        return MRX_OK;
    return bindGeometry(*r);
}

int mrx_set_stream(mrx_renderer *r, void *stream)
{
    if (const int src = settle(r))
        return src;
    if (!r)
        return fail(MRX_E_INVALID, "null renderer");
    if (!r->shards.empty())
        return wantsShard("mrx_set_stream");
    MRX_HIP(hipSetDevice(r->device));
    if ((hipStream_t)stream == r->stream)
        return MRX_OK;
    // renders already enqueued on the old stream finish before anything that
    // is enqueued on the new one can start
    MRX_HIP(hipStreamSynchronize(r->stream));
    r->stream = (hipStream_t)stream;
    return MRX_OK;
}

// mrx_buffer and mrx_sample_buffer: the tensor of `which` the caller sees (on a supersampled renderer the resolved one),
// or, `sample`, the s * W x s * H tensor the render writes
static void *bufferOf(mrx_renderer *r, int which, int64_t dims[4], int *ndim, int *dtype, int *device, bool sample)
{
    if (settle(r) != MRX_OK)
        return nullptr;
    if (!r || !dims || !ndim || !dtype) {
        fail(MRX_E_INVALID, "null argument");
        return nullptr;
    }
    if (!r->shards.empty()) {
        wantsShard(sample ? "mrx_sample_buffer" : "mrx_buffer");
        return nullptr;
    }
    if (sample && r->ss == 1) {
        fail(MRX_E_UNSUPPORTED, "no sample tensors: this renderer was created without supersampling");
        return nullptr;
    }
    if (sample && which != MRX_BUF_RGB && which != MRX_BUF_DEPTH && which != MRX_BUF_SEGMASK &&
        which != MRX_BUF_VISIBILITY && which != MRX_BUF_NORMAL) {
        fail(which >= 0 && which < MRX_NUM_BUFFERS_EXT10 ? MRX_E_UNSUPPORTED : MRX_E_INVALID,
             "not a rendered output: only rgb, depth, normals and the ids tensor have samples");
        return nullptr;
    }
    const bool rt = r->mode == MRX_MODE_RAYTRACER;
    const int64_t V = r->info.num_views, I = r->info.num_instances;
    const int64_t S = (int64_t)r->info.storage_slow * (sample ? r->ss : 1u);
    const int64_t F = (int64_t)r->info.storage_fast * (sample ? r->ss : 1u);
    // (what the caller sees of a supersampled renderer are the resolved tensors; each exists exactly when its sample
    // tensor does)
    const bool resolved = r->ss > 1 && !sample;
    void *const rgbPtr = resolved ? (void *)r->outRgb.ptr : (void *)r->rgb.ptr;
    void *const depthPtr = resolved ? (void *)r->outDepth.ptr : (void *)r->depth.ptr;
    void *const idsPtr = resolved ? (void *)r->outIds.ptr : (void *)r->ids.ptr;
    void *const normalPtr = resolved ? (void *)r->outNormal.ptr : (void *)r->normal.ptr;
    void *ptr = nullptr;
    const char *off = nullptr;                  // the MRX_E_UNSUPPORTED text of a tensor this renderer lacks
    if (device)
        *device = r->device;
    switch (which) {
    case MRX_BUF_RGB:       // mgr.cpp:547-568
        dims[0] = V; dims[1] = S; dims[2] = F; dims[3] = 4;
        *ndim = 4; *dtype = MRX_DTYPE_U8; ptr = rgbPtr;
        off = "rgb not rendered: this renderer was created depth-only (MRX_FLAG_NO_RGB)";
        break;
    case MRX_BUF_NORMAL:    // the surface-normal output: storage as rgb's
        dims[0] = V; dims[1] = S; dims[2] = F; dims[3] = 4;
        *ndim = 4; *dtype = MRX_DTYPE_U8; ptr = normalPtr;
        off = "normals not rendered: this renderer was created without MRX_FLAG_NORMALS";
        break;
    case MRX_BUF_POSITION:  // the position output: native size whatever the factor, no samples
        dims[0] = V; dims[1] = r->info.storage_slow; dims[2] = r->info.storage_fast; dims[3] = 4;
        *ndim = 4; *dtype = MRX_DTYPE_F32; ptr = r->position.ptr;
        off = "positions not computed: this renderer was created without MRX_FLAG_POSITIONS";
        break;
    case MRX_BUF_BOXES:     // box labels: (xmin, ymin, xmax, ymax, count) per view and label
        dims[0] = V; dims[1] = r->boxLabels; dims[2] = 5;
        *ndim = 3; *dtype = MRX_DTYPE_I32; ptr = r->boxes.ptr;
        off = "boxes not computed: this renderer was created without MRX_FLAG_BOX_LABELS";
        break;
    case MRX_BUF_OBSERVATION: {   // the packed observation: channel first, image order in both modes
        const int64_t H = rt ? r->info.storage_fast : r->info.storage_slow, W = rt ? r->info.storage_slow : r->info.storage_fast;
        dims[0] = V; dims[1] = (int64_t)r->obsStack * mrx::observeChannels(r->obsLayout); dims[2] = H; dims[3] = W;
        *ndim = 4;
        *dtype = r->obsDtype == MRX_OBS_F32 ? MRX_DTYPE_F32 : r->obsDtype == MRX_OBS_F16 ? MRX_DTYPE_F16
               : r->obsDtype == MRX_OBS_BF16 ? MRX_DTYPE_BF16 : MRX_DTYPE_U8;
        ptr = r->obs.ptr;
        off = "observations not packed: this renderer was created without MRX_FLAG_OBSERVATIONS";
        break;
    }
    case MRX_BUF_OBSERVATION_RESET:   // the reset column: a non-zero byte restarts the view's stack at the next run
        dims[0] = V; *ndim = 1; *dtype = MRX_DTYPE_U8; ptr = r->obsReset.ptr;
        off = r->obsLayout ? "no reset column: this renderer's MRX_FLAG_OBSERVATIONS field has a stack of 1"
                           : "no reset column: this renderer was created without MRX_FLAG_OBSERVATIONS";
        break;
    case MRX_BUF_RAYS:          // the ray-cast sensor: indexed by world
    case MRX_BUF_RAY_FRAME:
    case MRX_BUF_RAY_DISTANCE:
    case MRX_BUF_RAY_ID:
        if (!r->raysPerWorld) {
            fail(MRX_E_UNSUPPORTED, "no ray-cast sensor: mrx_rays_create was not called on this renderer");
            return nullptr;
        }
        dims[0] = r->info.num_worlds; dims[1] = r->raysPerWorld; dims[2] = 8;
        *ndim = which == MRX_BUF_RAYS ? 3 : which == MRX_BUF_RAY_FRAME ? 1 : 2;
        *dtype = which == MRX_BUF_RAYS || which == MRX_BUF_RAY_DISTANCE ? MRX_DTYPE_F32 : MRX_DTYPE_I32;
        ptr = which == MRX_BUF_RAYS ? (void *)r->rays.ptr : which == MRX_BUF_RAY_FRAME ? (void *)r->rayFrame.ptr
            : which == MRX_BUF_RAY_DISTANCE ? (void *)r->rayT.ptr : (void *)r->rayId.ptr;
        break;
    case MRX_BUF_FLOW:      // the optical-flow output: native size whatever the factor, no samples
        dims[0] = V; dims[1] = r->info.storage_slow; dims[2] = r->info.storage_fast; dims[3] = 4;
        *ndim = 4; *dtype = MRX_DTYPE_F32; ptr = r->flowOut.ptr;
        off = "no optical flow: mrx_flow_create was not called on this renderer";
        break;
    case MRX_BUF_CLOUD:         // the point-cloud output: indexed by view and slot, no samples
    case MRX_BUF_CLOUD_PIXEL:
    case MRX_BUF_CLOUD_COUNT:
        if (!r->cloudPoints) {
            fail(MRX_E_UNSUPPORTED, "no point cloud: mrx_cloud_create was not called on this renderer");
            return nullptr;
        }
        dims[0] = V; dims[1] = r->cloudPoints; dims[2] = 4;
        *ndim = which == MRX_BUF_CLOUD ? 3 : which == MRX_BUF_CLOUD_PIXEL ? 2 : 1;
        *dtype = which == MRX_BUF_CLOUD ? MRX_DTYPE_F32 : MRX_DTYPE_I32;
        ptr = which == MRX_BUF_CLOUD ? (void *)r->cloudOut.ptr : which == MRX_BUF_CLOUD_PIXEL ? (void *)r->cloudPixel.ptr
                                                               : (void *)r->cloudCount.ptr;
        break;
    case MRX_BUF_SHADOW:    // the shadow mask: stored exactly like depth, native size, no samples
        dims[0] = V; dims[1] = r->info.storage_slow; dims[2] = r->info.storage_fast;
        *ndim = 3; *dtype = MRX_DTYPE_U8; ptr = r->shadowMask.ptr;
        off = "no shadow mask: mrx_shadow_create was not called on this renderer";
        break;
    case MRX_BUF_DEPTH:     // mgr.cpp:570-590
        dims[0] = V; dims[1] = S; dims[2] = F; dims[3] = 1;
        *ndim = rt ? 3 : 4; *dtype = MRX_DTYPE_F32; ptr = depthPtr;
        off = "depth not rendered: this renderer was created rgb-only (MRX_FLAG_NO_DEPTH)";
        break;
    case MRX_BUF_SEGMASK:   // mgr.cpp:592-605; with the label column S11's segmask, in both modes
        if (!rt && !r->instLabel.ptr) {
            fail(MRX_E_UNSUPPORTED, "Segmask not implemented for rasterizer");
            return nullptr;
        }
        if (!r->params.idsAreSegmask) {
            fail(MRX_E_UNSUPPORTED, "ids buffer holds visibility ids (MRX_FLAG_VISIBILITY_IDS)");
            return nullptr;
        }
        dims[0] = V; dims[1] = S; dims[2] = F;
        *ndim = 3; *dtype = MRX_DTYPE_I32; ptr = idsPtr;
        break;
    case MRX_BUF_VISIBILITY:
        if (!r->ids.ptr || r->params.idsAreSegmask) {
            fail(MRX_E_UNSUPPORTED, "visibility ids need MRX_FLAG_VISIBILITY_IDS");
            return nullptr;
        }
        dims[0] = V; dims[1] = S; dims[2] = F;
        *ndim = 3; *dtype = MRX_DTYPE_I32; ptr = idsPtr;
        break;
    case MRX_BUF_INSTANCE_POSITION:   // mgr.cpp:627-635
        dims[0] = I; dims[1] = 3; *ndim = 2; *dtype = MRX_DTYPE_F32; ptr = r->instPos.ptr;
        break;
    case MRX_BUF_INSTANCE_ROTATION:   // mgr.cpp:637-645
        dims[0] = I; dims[1] = 4; *ndim = 2; *dtype = MRX_DTYPE_F32; ptr = r->instRot.ptr;
        break;
    case MRX_BUF_INSTANCE_SCALE:
        dims[0] = I; dims[1] = 3; *ndim = 2; *dtype = MRX_DTYPE_F32; ptr = r->instScale.ptr;
        break;
    case MRX_BUF_INSTANCE_OBJECT:     // ObjectID column (sim.cpp:152-156); negative = hidden
        dims[0] = I; *ndim = 1; *dtype = MRX_DTYPE_I32; ptr = r->instObj.ptr;
        break;
    case MRX_BUF_INSTANCE_MATERIAL:   // the material override column; outside the table = no override
        dims[0] = I; *ndim = 1; *dtype = MRX_DTYPE_I32; ptr = r->instMat.ptr;
        off = "no instance materials: this renderer was created without MRX_FLAG_INSTANCE_MATERIALS";
        break;
    case MRX_BUF_INSTANCE_LABEL:      // the label column; MRX_LABEL_OBJECT = the bound object's id
        dims[0] = I; *ndim = 1; *dtype = MRX_DTYPE_I32; ptr = r->instLabel.ptr;
        off = "no instance labels: this renderer was created without MRX_FLAG_INSTANCE_LABELS";
        break;
    case MRX_BUF_INSTANCE_COLOR:      // the colour override column; a == 0 = no override
        dims[0] = I; dims[1] = 4; *ndim = 2; *dtype = MRX_DTYPE_U8; ptr = r->instColor.ptr;
        off = "no instance colours: this renderer was created without MRX_FLAG_INSTANCE_COLORS";
        break;
    // The reference sizes the camera tensors with totalNumInstances
    // (mgr.cpp:652,662); the rows that exist are one per camera, exported so.
    case MRX_BUF_CAMERA_POSITION:
        dims[0] = V; dims[1] = 3; *ndim = 2; *dtype = MRX_DTYPE_F32; ptr = r->camPos.ptr;
        break;
    case MRX_BUF_CAMERA_ROTATION:
        dims[0] = V; dims[1] = 4; *ndim = 2; *dtype = MRX_DTYPE_F32; ptr = r->camRot.ptr;
        break;
    default:
        fail(MRX_E_INVALID, "unknown buffer id");
        return nullptr;
    }
    if (!ptr && off)
        fail(MRX_E_UNSUPPORTED, off);
    return ptr;
}

void *mrx_buffer(mrx_renderer *r, int which, int64_t dims[4], int *ndim, int *dtype, int *device)
{
    return bufferOf(r, which, dims, ndim, dtype, device, false);
}

void *mrx_sample_buffer(mrx_renderer *r, int which, int64_t dims[4], int *ndim, int *dtype, int *device)
{
    return bufferOf(r, which, dims, ndim, dtype, device, true);
}

int mrx_copy_to_host(mrx_renderer *r, int which, void *dst, uint64_t bytes)
{
    if (const int src = settle(r))
        return src;
    if (!r || !dst)
        return fail(MRX_E_INVALID, "null argument");
    if (!r->shards.empty())
        return wantsShard("mrx_copy_to_host");
    int64_t dims[4] = { 1, 1, 1, 1 };
    int nd = 0, dt = 0, dev = 0;
    void *src = mrx_buffer(r, which, dims, &nd, &dt, &dev);
    if (!src)
        return MRX_E_UNSUPPORTED;
    uint64_t total = dt == MRX_DTYPE_U8 ? 1 : dt == MRX_DTYPE_F16 || dt == MRX_DTYPE_BF16 ? 2 : 4;
    for (int i = 0; i < nd; ++i)
        total *= (uint64_t)dims[i];
    if (bytes > total)
        return fail(MRX_E_INVALID, "readback larger than the buffer");
    MRX_HIP(hipSetDevice(r->device));
    MRX_HIP(hipStreamSynchronize(r->stream));
    MRX_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return MRX_OK;
}

int mrx_info(mrx_renderer *r, mrx_info_t *out)
{
    // the ABI-2 entry point: its callers allocated the struct as it was then
    return mrx_info_sized(r, out, MRX_INFO_V2_SIZE);
}

int mrx_info_sized(mrx_renderer *r, void *out, size_t size)
{
    if (!r || !out)
        return fail(MRX_E_INVALID, "null argument");
    if (size < MRX_INFO_V2_SIZE)
        return fail(MRX_E_INVALID, "mrx_info_t size mismatch (ABI)");
    mrx_info_t full;
    const int rc = infoFull(r, &full);
    if (rc != MRX_OK)
        return rc;
    std::memcpy(out, &full, std::min(size, sizeof full));
    return MRX_OK;
}

int mrx_time_steps_host(mrx_renderer *r, int steps, double *us_per_step)
{
    if (!r || !us_per_step || steps <= 0)
        return fail(MRX_E_INVALID, "bad argument");
    shardTraceReset();
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < steps; ++i) {
        const int rc = mrx_step(r);
        if (rc != MRX_OK)
            return rc;
    }
    const auto t1 = std::chrono::steady_clock::now();
    *us_per_step = std::chrono::duration<double, std::micro>(t1 - t0).count() / (double)steps;
    shardTraceReport();
    return mrx_sync(r);
}

int mrx_time_renders(mrx_renderer *r, int steps, float *ms_total)
{
    if (r && r->parent)
        if (const int src = settle(r))
            return src;
    if (!r || !ms_total || steps < 0)
        return fail(MRX_E_INVALID, "bad argument");
    if (!r->shards.empty()) {
        // every device runs its `steps` launches between its own two events, all enqueued
        // before anything is waited for: the job takes as long as the slowest device
        {
            const int rc = shardsRun(r, kCmdTimed, steps);    // every device's launches from its own thread
            if (rc != MRX_OK)
                return rc;
        }
        *ms_total = 0.0f;
        for (mrx_renderer *sh : r->shards) {
            float ms = 0.0f;
            MRX_HIP(hipSetDevice(sh->device));
            MRX_HIP(hipEventSynchronize(sh->ev1));
            MRX_HIP(hipEventElapsedTime(&ms, sh->ev0, sh->ev1));
            *ms_total = std::max(*ms_total, ms);
        }
        return MRX_OK;
    }
    MRX_HIP(hipSetDevice(r->device));
    MRX_HIP(hipEventRecord(r->ev0, r->stream));
    for (int i = 0; i < steps; ++i)
        MRX_HIP(r->launch());
    MRX_HIP(hipEventRecord(r->ev1, r->stream));
    MRX_HIP(hipEventSynchronize(r->ev1));
    MRX_HIP(hipEventElapsedTime(ms_total, r->ev0, r->ev1));
    return MRX_OK;
}

int64_t mrx_debug_stamps(mrx_renderer *r, uint64_t *dst, int64_t capacity)
{
    if (settle(r) != MRX_OK)
        return 0;
    if (r && !r->shards.empty())
        r = r->shards[0];
    if (!r || !dst || !r->stamps.ptr)
        return 0;
    const int64_t n = (int64_t)r->stamps.count < capacity ? (int64_t)r->stamps.count : capacity;
    if (hipSetDevice(r->device) != hipSuccess || hipStreamSynchronize(r->stream) != hipSuccess ||
        hipMemcpy(dst, r->stamps.ptr, (size_t)n * 8, hipMemcpyDeviceToHost) != hipSuccess)
        return 0;
    return n;
}

int mrx_mark(mrx_renderer *r, int which)
{
    if (const int src = settle(r))
        return src;
    if (!r || (which != 0 && which != 1))
        return fail(MRX_E_INVALID, "bad argument");
    for (mrx_renderer *sh : r->shards) {
        const int rc = mrx_mark(sh, which);
        if (rc != MRX_OK)
            return rc;
    }
    if (!r->shards.empty())
        return MRX_OK;
    MRX_HIP(hipSetDevice(r->device));
    MRX_HIP(hipEventRecord(which ? r->ev1 : r->ev0, r->stream));
    return MRX_OK;
}

int mrx_elapsed_ms(mrx_renderer *r, float *ms)
{
    if (const int src = settle(r))
        return src;
    if (!r || !ms)
        return fail(MRX_E_INVALID, "null argument");
    if (!r->shards.empty()) {                     // the slowest device
        *ms = 0.0f;
        for (mrx_renderer *sh : r->shards) {
            float one = 0.0f;
            const int rc = mrx_elapsed_ms(sh, &one);
            if (rc != MRX_OK)
                return rc;
            *ms = std::max(*ms, one);
        }
        return MRX_OK;
    }
    MRX_HIP(hipSetDevice(r->device));
    MRX_HIP(hipEventSynchronize(r->ev1));
    MRX_HIP(hipEventElapsedTime(ms, r->ev0, r->ev1));
    return MRX_OK;
}

int mrx_placement(mrx_renderer *r, float *cand_us, int capacity, float *kept_us)
{
    if (r && !r->shards.empty())
        r = r->shards[0];
    if (!r || (!cand_us && capacity > 0))
        return fail(MRX_E_INVALID, "bad argument");
    for (size_t i = 0; i < r->placementUs.size() && (int)i < capacity; ++i)
        cand_us[i] = r->placementUs[i];
    if (kept_us)
        *kept_us = r->placementKeptUs;
    return (int)r->placementUs.size();
}

int mrx_copy_triangles(mrx_renderer *r, float *tri_pos, float *tri_uv, int32_t *tri_mat,
                       int32_t *obj_first, int32_t *obj_count)
{
    if (r && !r->shards.empty())
        r = r->shards[0];                         // every shard holds the whole object pool
    if (!r)
        return fail(MRX_E_INVALID, "null renderer");
    for (size_t t = 0; t < r->hostTris.size(); ++t) {
        if (tri_pos) std::memcpy(tri_pos + 9 * t, r->hostTris[t].p, 36);
        if (tri_uv) std::memcpy(tri_uv + 6 * t, r->hostTris[t].uv, 24);
        if (tri_mat) tri_mat[t] = r->hostTris[t].mat;
    }
    for (size_t o = 0; o < r->objFirst.size(); ++o) {
        if (obj_first) obj_first[o] = r->objFirst[o];
        if (obj_count) obj_count[o] = r->objCount[o];
    }
    return MRX_OK;
}

}  // extern "C"
