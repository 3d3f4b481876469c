// The post-render stages: what each launches, the table that lists them once in step order (kStages) and everything
// that goes through it -- the step's stage loop, the shards' "run stage i" command, the stage entry points and the
// tensors a creation flag allocates -- and the stages attached later (mrx_rays_create, mrx_flow_create,
// mrx_cloud_create, mrx_shadow_create), which share one life cycle (Attached, attachPrologue, attachAll).
//
// A new attached stage supplies: its launch filler (the blocks every stage has come from fillImage / fillCamera), its
// entry in kStages, its create / release / bytes functions and its Attached record, its mrx_*_create -- the texts of
// the prologue, its own argument and size checks --, its fields in the renderer and its tensors in bufferOf.  The
// arithmetic the stages share is in stage_core.hpp.
#include "renderer.hpp"

#include "resolve.hpp"
#include "unproject.hpp"
#include "boxes.hpp"
#include "rays.hpp"
#include "observe.hpp"

// What the stages' parameter blocks have in common, under the same names, filled once.  The image as the caller sees
// it: the native size, whichever the sample render's.
template <typename P>
static void fillImage(const mrx_renderer &r, P &q)
{
    q.numViews = r.params.numViews;
    q.nfast = r.info.storage_fast;
    q.nslow = r.info.storage_slow;
    q.transposed = r.params.transposed;
    q.numCUs = r.params.numCUs;
}

// ... of a stage that works out which sample a native pixel's value was taken from: the supersampling factor, too
template <typename P>
static void fillSampledImage(const mrx_renderer &r, P &q, uint32_t P::*s)
{
    fillImage(r, q);
    q.*s = r.ss;
    q.half = r.ss / 2;
}

// the projection constants of the views: the per-view table, else the uniform four
template <typename P>
static void fillProjection(const mrx_renderer &r, P &q)
{
    q.viewProj = r.params.viewProj;
    q.sx = r.params.sx; q.ox = r.params.ox; q.sz = r.params.sz; q.oz = r.params.oz;
}

template <typename P>
static void fillCamera(const mrx_renderer &r, P &q)
{
    q.camPos = r.params.camPos;
    q.camRot = r.params.camRot;
    fillProjection(r, q);
}

// (depth, ids, the constants and every table pointer are read from the render's parameters at every launch: the
// placement search re-binds the first two, mrx_set_view_projection the constants, bindGeometry the tables; pose,
// table and snapshot CONTENTS are read by the kernel)
mrx::FlowParams mrx_renderer::flowParams()
{
    mrx::FlowParams q {};
    q.depth = seenDepth();
    q.ids = seenIds();
    q.flow = flowOut.ptr;
    q.instKBase = params.instKBase;
    q.worldInstStart = params.worldInstStart;
    q.viewWorld = params.viewWorld;
    q.live.instPos = params.instPos;
    q.live.instRot = params.instRot;
    q.live.instScale = params.instScale;
    q.live.camPos = params.camPos;
    q.live.camRot = params.camRot;
    fillProjection(*this, q);
    fillSampledImage(*this, q, &mrx::FlowParams::s);
    q.numInstances = info.num_instances;
    q.passRows = flowPassRows;
    mrx::flowBindSnapshot(flowSnap.ptr, q);
    return q;
}
hipError_t mrx_renderer::launchFlow() { return mrx::launchFlow(flowParams(), stream); }
hipError_t mrx_renderer::launchFlowSnapshot() { return mrx::launchFlowSnapshot(flowParams(), stream); }

// (depth, the constants and the table pointer are read from the render's parameters at every launch: the placement
// search re-binds the first, mrx_set_view_projection the others; pose and table CONTENTS are read by the kernel)
hipError_t mrx_renderer::launchCloud()
{
    mrx::CloudParams q {};
    q.depth = seenDepth();
    q.points = cloudOut.ptr;
    q.pixel = cloudPixel.ptr;
    q.count = cloudCount.ptr;
    q.scratch = cloudScratch.ptr;
    q.scratchCount = cloudScratch.count;
    fillCamera(*this, q);
    fillSampledImage(*this, q, &mrx::CloudParams::s);
    q.N = cloudPoints;
    q.frame = (int32_t)cloudFrame;
    q.maxDepth = cloudMaxDepth;
    q.forcedParts = cloudForcedParts;
    return mrx::launchCloud(q, stream);
}

// (depth, rgb, normals, the constants, the light and every table pointer are read from the render's parameters at every
// launch: the placement search re-binds the tensors, mrx_set_view_projection / mrx_set_world_light the constants and
// the light tables, bindGeometry the geometry tables; pose, scale, ObjectID, camera and table CONTENTS are read by the
// kernel)
hipError_t mrx_renderer::launchShadow(bool apply)
{
    mrx::ShadowParams q {};
    q.s.tris = params.tris;
    q.s.nodes = params.bvhNodes;
    q.s.leafTris = params.bvhLeafTris;
    q.s.instInfo = params.instInfo;
    q.s.worldInstStart = params.worldInstStart;
    q.s.instPos = params.instPos;
    q.s.instRot = params.instRot;
    q.s.instScale = params.instScale;
    q.s.instObj = params.instObj;
    q.viewWorld = params.viewWorld;
    q.depth = seenDepth();
    q.mask = shadowMask.ptr;
    q.rgb = seenRgb();
    q.normal = seenNormal();
    fillCamera(*this, q);
    fillSampledImage(*this, q, &mrx::ShadowParams::ss);
    q.viewLight = params.viewLight;
    for (int k = 0; k < 3; ++k)
        q.toLight[k] = params.toLight[k];
    q.ambient = params.ambient;
    q.diffuse = params.diffuse;
    q.apply = apply ? 1 : 0;
    q.bias = shadowBias;
    q.maxDistance = shadowMaxDistance;
    q.bvhDepth = info.bvh_depth;
    q.passRows = shadowPassRows;
    q.brute = shadowBrute ? 1 : 0;
    return mrx::launchShadow(q, stream);
}

// (every table pointer is read from the render's parameters at every launch: bindGeometry re-binds them; pose, scale,
// ObjectID, label, ray and frame CONTENTS are read by the kernel)
hipError_t mrx_renderer::launchRays()
{
    mrx::RayParams q {};
    q.s.tris = params.tris;
    q.s.nodes = params.bvhNodes;
    q.s.leafTris = params.bvhLeafTris;
    q.s.instInfo = params.instInfo;
    q.s.instKBase = params.instKBase;
    q.s.boundObj = rayBound.ptr;
    q.s.worldInstStart = params.worldInstStart;
    q.s.instPos = params.instPos;
    q.s.instRot = params.instRot;
    q.s.instScale = params.instScale;
    q.s.instObj = params.instObj;
    q.s.instLabel = instLabel.ptr;
    q.rays = rays.ptr;
    q.frame = rayFrame.ptr;
    q.outT = rayT.ptr;
    q.outId = rayId.ptr;
    q.numWorlds = info.num_worlds;
    q.R = raysPerWorld;
    q.bvhDepth = info.bvh_depth;
    q.numCUs = params.numCUs;
    q.passRows = rayPassRows;
    q.brute = rayBrute ? 1 : 0;
    return mrx::launchRays(q, stream);
}

// (rgb and depth are read from the render's parameters at every launch: the placement search re-binds them)
hipError_t mrx_renderer::launchObserve()
{
    mrx::ObserveParams q {};
    q.rgb = seenRgb();
    q.depth = seenDepth();
    q.obs = obs.ptr;
    q.reset = obsReset.ptr;
    fillImage(*this, q);
    q.layout = obsLayout;
    q.dtype = obsDtype;
    q.stack = obsStack;
    q.hasRange = obsHi > 0.0f ? 1 : 0;
    q.lo = obsLo;
    q.inv = obsInv;
    return mrx::launchObserve(q, stream);
}

// every view's stack restarts at the next run of the stage
hipError_t mrx_renderer::markObservationsReset()
{
    return obsReset.ptr ? hipMemsetAsync(obsReset.ptr, 1, params.numViews, stream) : hipSuccess;
}

// (the ids pointer is read from the render's parameters at every launch: the placement search re-binds it)
hipError_t mrx_renderer::launchBoxes()
{
    mrx::BoxParams q {};
    q.ids = seenIds();
    q.out = boxes.ptr;
    fillImage(*this, q);
    q.K = boxLabels;
    q.forcedParts = boxParts;
    return mrx::launchBoxes(q, stream);
}

// (depth, the constants and the table pointer are read from the render's parameters at every launch: the placement
// search re-binds the first, mrx_set_view_projection the others; pose and table CONTENTS are read by the kernel)
hipError_t mrx_renderer::launchUnproject()
{
    mrx::UnprojectParams q {};
    q.depth = seenDepth();
    q.pos = position.ptr;
    fillCamera(*this, q);
    fillSampledImage(*this, q, &mrx::UnprojectParams::s);
    q.frame = positions == 2 ? mrx::kFrameView : mrx::kFrameWorld;
    return mrx::launchUnproject(q, stream);
}

// (the sample pointers are read from the render's parameters at every launch: the placement search re-binds them)
hipError_t mrx_renderer::launchResolve()
{
    mrx::ResolveParams q {};
    q.rgbIn = params.rgb;
    q.depthIn = reinterpret_cast<const uint32_t *>(params.depth);
    q.idsIn = reinterpret_cast<const uint32_t *>(params.ids);
    q.normalIn = params.normal;
    q.rgbOut = outRgb.ptr;
    q.depthOut = reinterpret_cast<uint32_t *>(outDepth.ptr);
    q.idsOut = reinterpret_cast<uint32_t *>(outIds.ptr);
    q.normalOut = outNormal.ptr;
    q.rows = params.numViews * info.storage_slow;
    q.nfast = info.storage_fast;
    q.numCUs = params.numCUs;
    return mrx::launchResolve(q, (int)ss, stream);
}

// The test knobs: an environment variable read as an integer where it is set.  envCount: a count, never below 0, and
// `absent` where the variable is not set.
static int envInt(const char *name, int absent)
{
    const char *v = std::getenv(name);
    return v ? std::atoi(v) : absent;
}
static uint32_t envCount(const char *name, uint32_t absent) { return (uint32_t)std::max(0, envInt(name, (int)absent)); }

uint32_t supersampleOf(uint32_t flags) { return 1u + ((flags & MRX_FLAG_SUPERSAMPLE_MASK) >> MRX_FLAG_SUPERSAMPLE_SHIFT); }

// the native tensors of a supersampled renderer, one per sample tensor, laid out as the outputs of a plain renderer of
// the native size are; info then describes what the caller sees: native storage, and the resolve's bytes on top of the
// sample render's -- s * s * 4 read per native pixel of rgb, 4 per point-sampled tensor, 4 written per tensor
static int allocResolved(mrx_renderer &r)
{
    const uint32_t s = r.ss;
    const uint32_t nfast = r.params.nfast / s, nslow = r.params.nslow / s;
    const uint64_t px = (uint64_t)r.params.numViews * nfast * nslow;
    if (px > mrx::kResolveMaxPixels)
        return fail(MRX_E_INVALID, "supersampling: more than 2^32 - 1 native pixels");
    MRX_HIP(allocOutputs((size_t)px, r.rgb.ptr != nullptr, r.depth.ptr != nullptr, r.ids.ptr != nullptr,
                         firstKindIsOneBlock((size_t)px), r.outRgb, r.outDepth, r.outIds, r.normal.ptr != nullptr,
                         r.outNormal));
    r.info.storage_fast = nfast;
    r.info.storage_slow = nslow;
    const uint64_t points = (r.depth.ptr ? 1u : 0u) + (r.ids.ptr ? 1u : 0u) + (r.normal.ptr ? 1u : 0u);
    r.info.bytes_per_step += px * ((r.rgb.ptr ? 4ull * s * s + 4ull : 0ull) + 8ull * points);
    return MRX_OK;
}

uint32_t positionsOf(uint32_t flags) { return (flags & MRX_FLAG_POSITIONS_VIEW) ? 2u : (flags & MRX_FLAG_POSITIONS) ? 1u : 0u; }

// the position tensor of a renderer with the position output: one allocation of its own (hipMalloc: 16-byte aligned
// and more), [views][storage_slow][storage_fast][4] floats of the NATIVE size; the stage's bytes on top of the rest:
// 4 read and 16 written per native pixel
static int allocPositions(mrx_renderer &r)
{
    const uint64_t px = (uint64_t)r.params.numViews * r.info.storage_fast * r.info.storage_slow;
    if (px > mrx::kUnprojectMaxPixels)
        return fail(MRX_E_INVALID, "positions: more than 2^32 - 1 native pixels");
    MRX_HIP(r.position.alloc((size_t)px * 4));
    r.info.bytes_per_step += px * (4ull + 16ull);
    return MRX_OK;
}

uint32_t boxLabelsOf(uint32_t flags) { return (flags & MRX_FLAG_BOX_LABELS_MASK) >> MRX_FLAG_BOX_LABELS_SHIFT; }

// the box tensor of a renderer with box labels: one allocation of its own, [views][K][5] int32; the stage's bytes on
// top of the rest: 4 read per native pixel and the tensor written
static int allocBoxes(mrx_renderer &r)
{
    const uint64_t px = (uint64_t)r.params.numViews * r.info.storage_fast * r.info.storage_slow;
    if (px > mrx::kBoxMaxPixels)
        return fail(MRX_E_INVALID, "box labels: more than 2^32 - 1 native pixels");
    const uint64_t cells = (uint64_t)r.params.numViews * r.boxLabels * 5u;
    MRX_HIP(r.boxes.alloc((size_t)cells));
    r.info.bytes_per_step += px * 4ull + cells * 4ull;
    r.boxParts = envCount("MRX_BOX_PARTS", r.boxParts);     // tests: the merge path at tiny sizes
    return MRX_OK;
}

uint32_t obsLayoutOf(uint32_t flags) { return (flags & MRX_FLAG_OBS_LAYOUT_MASK) >> MRX_FLAG_OBS_SHIFT; }
static uint32_t obsDtypeOf(uint32_t flags) { return (flags & MRX_FLAG_OBS_DTYPE_MASK) >> MRX_FLAG_OBS_DTYPE_SHIFT; }
static uint32_t obsStackOf(uint32_t flags) { return 1u + ((flags & MRX_FLAG_OBS_STACK_MASK) >> MRX_FLAG_OBS_STACK_SHIFT); }

static_assert(MRX_OBS_RGB == mrx::kObsRgb && MRX_OBS_RGBD == mrx::kObsRgbd && MRX_OBS_D == mrx::kObsD &&
                  MRX_OBS_Y == mrx::kObsY && MRX_OBS_YD == mrx::kObsYd && MRX_OBS_F32 == mrx::kObsF32 &&
                  MRX_OBS_F16 == mrx::kObsF16 && MRX_OBS_BF16 == mrx::kObsBf16 && MRX_OBS_U8 == mrx::kObsU8,
              "observe.hpp and mrx.h MRX_OBS_* disagree");

// the tensors of a renderer with the packed observation output: the [views][S * C][H][W] tensor, zeroed, and with
// S > 1 the reset column, which starts at 1 -- the first frame fills every stack; the stage's bytes on top of the
// rest, per native pixel: the inputs the layout reads (4 for rgb, 4 for depth), the current frame written (C * e) and
// S - 1 frames read and written (2 * (S - 1) * C * e)
static int allocObservations(mrx_renderer &r)
{
    const uint64_t px = (uint64_t)r.params.numViews * r.info.storage_fast * r.info.storage_slow;
    if (px > mrx::kObserveMaxPixels)
        return fail(MRX_E_INVALID, "observations: more than 2^32 - 1 native pixels");
    const uint64_t C = mrx::observeChannels(r.obsLayout), e = mrx::observeElemBytes(r.obsDtype), S = r.obsStack;
    const uint64_t bytes = px * S * C * e;
    MRX_HIP(r.obs.alloc((size_t)std::max<uint64_t>(bytes, 1)));
    MRX_HIP(hipMemsetAsync(r.obs.ptr, 0, (size_t)bytes, r.stream));      // (ahead of the first frame, on its stream)
    if (S > 1) {
        MRX_HIP(r.obsReset.alloc((size_t)std::max<uint32_t>(r.params.numViews, 1)));
        MRX_HIP(hipMemsetAsync(r.obsReset.ptr, 1, r.params.numViews, r.stream));
    }
    r.info.bytes_per_step += px * ((mrx::observeReadsColour(r.obsLayout) ? 4ull : 0ull) +
                                   (mrx::observeReadsDepth(r.obsLayout) ? 4ull : 0ull) + (2ull * S - 1ull) * C * e);
    return MRX_OK;
}

static bool flowOn(const mrx_renderer *r)
{
    return r->shards.empty() ? r->flowOut.ptr != nullptr : r->shards[0]->flowOut.ptr != nullptr;
}

void decodeStageFlags(uint32_t flags, mrx_renderer &r)
{
    r.ss = supersampleOf(flags);
    r.positions = positionsOf(flags);
    r.boxLabels = boxLabelsOf(flags);
    r.obsLayout = obsLayoutOf(flags);
    r.obsDtype = obsDtypeOf(flags);
    r.obsStack = obsStackOf(flags);
}

// a post-render stage
struct Stage {
    bool (*on)(const mrx_renderer &r);          // on for this renderer (of a multi-device renderer: for its shards)
    hipError_t (*launch)(mrx_renderer &r);      // on the renderer's stream
    int (*alloc)(mrx_renderer &r);              // at creation, of a stage the flags switch on; null: an attached stage
    const char *call;                           // the launch as a HIP failure's text names it
    const char *off;                            // the MRX_E_UNSUPPORTED text of its entry point
    bool inStep = true;                         // false: an entry point's form of a stage, never part of a step
};
enum : int { kStageResolve = 0, kStageUnproject, kStageShadow, kStageBoxes, kStageObserve, kStageTrace, kStageFlow,
             kStageFlowSnapshot, kStageCloud, kStageShadowMask, kNumStages };

// The stages in the order a step runs them; the snapshot after the flow that reads the one before it; the compaction
// last: it reads the depth the caller sees, behind the resolve, and nothing reads what it writes.  The shadow stage
// runs behind the unprojection and ahead of the boxes and the observation: the observation packs the rgb it has
// darkened, and neither the flow nor the cloud reads rgb.  Its last entry is mrx_shadow's: the mask-only form whatever
// the renderer's, which no step runs.
static const Stage kStages[kNumStages] = {
    { [](const mrx_renderer &r) { return r.ss > 1; }, [](mrx_renderer &r) { return r.launchResolve(); }, allocResolved,
      "launchResolve()", "nothing to resolve: this renderer was created without supersampling" },
    { [](const mrx_renderer &r) { return r.positions != 0; }, [](mrx_renderer &r) { return r.launchUnproject(); },
      allocPositions, "launchUnproject()",
      "nothing to unproject: this renderer was created without MRX_FLAG_POSITIONS" },
    { [](const mrx_renderer &r) { return r.shadows != 0; }, [](mrx_renderer &r) { return r.launchShadow(r.shadows == 2); },
      nullptr, "launchShadow()", "no shadows to cast: mrx_shadow_create was not called on this renderer" },
    { [](const mrx_renderer &r) { return r.boxLabels != 0; }, [](mrx_renderer &r) { return r.launchBoxes(); }, allocBoxes,
      "launchBoxes()", "no boxes to compute: this renderer was created without MRX_FLAG_BOX_LABELS" },
    { [](const mrx_renderer &r) { return r.obsLayout != 0; }, [](mrx_renderer &r) { return r.launchObserve(); },
      allocObservations, "launchObserve()",
      "nothing to observe: this renderer was created without MRX_FLAG_OBSERVATIONS" },
    { [](const mrx_renderer &r) { return r.raysPerWorld != 0; }, [](mrx_renderer &r) { return r.launchRays(); }, nullptr,
      "launchRays()", "nothing to trace: mrx_rays_create was not called on this renderer" },
    { [](const mrx_renderer &r) { return flowOn(&r); }, [](mrx_renderer &r) { return r.launchFlow(); }, nullptr,
      "launchFlow()", "no optical flow: mrx_flow_create was not called on this renderer" },
    { [](const mrx_renderer &r) { return flowOn(&r); }, [](mrx_renderer &r) { return r.launchFlowSnapshot(); }, nullptr,
      "launchFlowSnapshot()", "no optical flow: mrx_flow_create was not called on this renderer" },
    { [](const mrx_renderer &r) { return r.cloudPoints != 0; }, [](mrx_renderer &r) { return r.launchCloud(); }, nullptr,
      "launchCloud()", "no point cloud: mrx_cloud_create was not called on this renderer" },
    { [](const mrx_renderer &r) { return r.shadows != 0; }, [](mrx_renderer &r) { return r.launchShadow(false); }, nullptr,
      "launchShadow()", "no shadows to cast: mrx_shadow_create was not called on this renderer", false },
};

int allocStages(mrx_renderer &r)
{
    for (const Stage &s : kStages)
        if (s.alloc && s.on(r))
            if (const int rc = s.alloc(r))
                return rc;
    return MRX_OK;
}

hipError_t mrx_renderer::launch()
{
    hipError_t e = launchRender();
    for (const Stage &s : kStages)
        if (e == hipSuccess && s.inStep && s.on(*this))
            e = s.launch(*this);
    return e;
}

// `who`: how the caller names the renderer ("r->", "sh->")
static int stageLaunch(const Stage &s, mrx_renderer &r, const char *who)
{
    const hipError_t e = s.launch(r);
    return e == hipSuccess ? MRX_OK : fail(MRX_E_HIP, std::string(who) + s.call + ": " + hipGetErrorString(e));
}

// what the shards of one device do for a command, on whichever thread runs it (the shards of a
// group share a device; it is made current here unless the thread is bound to it for good)
int groupRun(const ShardGroup &group, int cmd, int steps, bool bindDevice)
{
    if (group.empty())
        return MRX_OK;
    if (bindDevice)
        MRX_HIP(hipSetDevice(group[0]->device));
    if (cmd >= kCmdStage && cmd < kCmdStage + kNumStages) {
        for (mrx_renderer *sh : group)
            if (const int rc = stageLaunch(kStages[cmd - kCmdStage], *sh, "sh->"))
                return rc;
        return MRX_OK;
    }
    switch (cmd) {
    case kCmdRender:
        for (mrx_renderer *sh : group)
            MRX_HIP(sh->launch());
        return MRX_OK;
    case kCmdObserveRestart:
        for (mrx_renderer *sh : group) {
            MRX_HIP(sh->markObservationsReset());
            MRX_HIP(sh->launchObserve());
        }
        return MRX_OK;
    case kCmdSync:
        for (mrx_renderer *sh : group)
            MRX_HIP(hipStreamSynchronize(sh->stream));
        return MRX_OK;
    case kCmdTimed:
        // every shard's launches between its own two events, the shards of the device interleaved
        // step by step: the slowest shard's interval spans the device's whole job
        for (mrx_renderer *sh : group)
            MRX_HIP(hipEventRecord(sh->ev0, sh->stream));
        for (int i = 0; i < steps; ++i)
            for (mrx_renderer *sh : group)
                MRX_HIP(sh->launch());
        for (mrx_renderer *sh : group)
            MRX_HIP(hipEventRecord(sh->ev1, sh->stream));
        return MRX_OK;
    default:
        return MRX_OK;
    }
}

// a renderer, or the renderer a shard handle belongs to: device threads caught up (MRX_SHARD_ASYNC)
int settle(mrx_renderer *r)
{
    if (r && r->parent)
        r = r->parent;
    if (!r || !r->shardSet.shardAsync)
        return MRX_OK;
    return joinRenders(r->shardSet);
}

// run `cmd` on every shard of a multi-device renderer (shards.cpp where it has device threads); returns the first failure
int shardsRun(mrx_renderer *r, int cmd, int steps)
{
    if (!r->shardSet.workers.empty())
        return shardsRun(r->shardSet, cmd, steps);
    // no threads: device by device from the calling thread (consecutive shards of one device as a group)
    ShardGroup group;
    for (size_t i = 0; i < r->shards.size(); ++i) {
        group.push_back(r->shards[i]);
        if (i + 1 == r->shards.size() || r->shards[i + 1]->device != r->shards[i]->device) {
            const int rc = groupRun(group, cmd, steps, true);
            if (rc != MRX_OK)
                return rc;
            group.clear();
        }
    }
    return MRX_OK;
}

void startShardWorkers(mrx_renderer *r)
{
    std::vector<int> devices;
    for (const mrx_renderer *sh : r->shards)
        devices.push_back(sh->device);
    const ShardBindFn bind = [](const ShardGroup &group) {
        const hipError_t e = hipSetDevice(group[0]->device);
        return e == hipSuccess ? (int)MRX_OK
                               : fail(MRX_E_HIP, std::string("hipSetDevice (shard worker): ") + hipGetErrorString(e));
    };
    startShardWorkers(r->shardSet, r->shards, devices, (r->flags & MRX_FLAG_SHARD_ASYNC) != 0, bind, groupRun);
}

// the one prologue of the stage entry points (mrx_resolve ... mrx_flow_snapshot)
static int runStage(mrx_renderer *r, int stage)
{
    if (const int src = settle(r))
        return src;
    if (!r)
        return fail(MRX_E_INVALID, "null renderer");
    const Stage &s = kStages[stage];
    if (!s.on(*r))
        return fail(MRX_E_UNSUPPORTED, s.off);
    if (!r->shards.empty())
        return shardsRun(r, kCmdStage + stage);
    MRX_HIP(hipSetDevice(r->device));
    return stageLaunch(s, *r, "r->");
}

// ---- the stages attached after creation (mrx_rays_create, mrx_flow_create, mrx_cloud_create, mrx_shadow_create).  Each
// supplies a `create` -- its buffers, their first contents, its test knobs, its "on" field and its first launch, in
// that order --, a `release` -- the buffers freed and the field cleared: the failure path, the way back when a later
// shard fails, the renderer's teardown -- and a `bytes`, what it adds to info.bytes_per_step while it is on.
struct Attached {
    const char *what;                                       // how the text of a HIP failure begins
    hipError_t (*create)(mrx_renderer &r, uint32_t arg);
    void (*release)(mrx_renderer &r);
    uint64_t (*bytes)(const mrx_renderer &r);
    uint32_t mrx_renderer::*on;                             // the field that holds `arg` while the stage is on (null: none)
};

static uint64_t nativePixels(const mrx_info_t &i) { return (uint64_t)i.num_views * i.storage_fast * i.storage_slow; }

// the sensor: the four tensors, the bound-object table, the first trace
static hipError_t raysCreate(mrx_renderer &r, uint32_t R)
{
    const uint64_t worlds = r.info.num_worlds, n = worlds * R;
    hipError_t e = r.rays.alloc((size_t)n * 8u);
    if (e == hipSuccess) e = r.rayT.alloc((size_t)n);
    if (e == hipSuccess) e = r.rayId.alloc((size_t)n);
    if (e == hipSuccess) e = r.rayFrame.alloc((size_t)worlds);
    if (e == hipSuccess) e = uploadRayBound(r);
    if (e == hipSuccess) e = mrx::prepareRays();
    // zero rays, world frame (-1 is all bytes 0xFF), and what the zero ray gives: tmax = 0, id -1
    if (e == hipSuccess) e = hipMemsetAsync(r.rays.ptr, 0, (size_t)n * 32u, r.stream);
    if (e == hipSuccess) e = hipMemsetAsync(r.rayT.ptr, 0, (size_t)n * 4u, r.stream);
    if (e == hipSuccess) e = hipMemsetAsync(r.rayId.ptr, 0xFF, (size_t)n * 4u, r.stream);
    if (e == hipSuccess) e = hipMemsetAsync(r.rayFrame.ptr, 0xFF, (size_t)worlds * 4u, r.stream);
    if (e != hipSuccess)
        return e;
    r.rayBrute = envInt("MRX_RAYS_BRUTE", 0) != 0;
    r.rayPassRows = envCount("MRX_RAY_PASS_ROWS", r.rayPassRows);   // tests: several staging passes at tiny sizes
    r.raysPerWorld = R;
    return r.launchRays();
}
static void raysRelease(mrx_renderer &r)
{
    r.raysPerWorld = 0;
    r.rays.release(); r.rayT.release(); r.rayFrame.release(); r.rayId.release(); r.rayBound.release();
}
// per ray 32 bytes read, 8 written (the tables it walks depend on the rays)
static uint64_t raysBytes(const mrx_renderer &r) { return (uint64_t)r.info.num_worlds * r.raysPerWorld * 40ull; }
static const Attached kRays = { "ray-cast sensor: ", raysCreate, raysRelease, raysBytes, &mrx_renderer::raysPerWorld };

// the flow output: the tensor, the snapshot of the state as it is, the first flow.  The two pointers are the sign of it.
static hipError_t flowCreate(mrx_renderer &r, uint32_t)
{
    const uint64_t px = nativePixels(r.info);
    const uint64_t snap = mrx::flowSnapshotLayout(r.info.num_instances, r.info.num_views).total;
    // (one spare 16 bytes each: a renderer without a pixel or a row still has two pointers)
    hipError_t e = r.flowOut.alloc((size_t)px * 4u + 4u);
    if (e == hipSuccess) e = r.flowSnap.alloc((size_t)snap + 4u);
    if (e == hipSuccess) e = hipMemsetAsync(r.flowOut.ptr, 0, ((size_t)px * 4u + 4u) * 4u, r.stream);
    if (e == hipSuccess) e = hipMemsetAsync(r.flowSnap.ptr, 0, ((size_t)snap + 4u) * 4u, r.stream);
    if (e != hipSuccess)
        return e;
    r.flowPassRows = envCount("MRX_FLOW_PASS_ROWS", r.flowPassRows);    // tests: several staging passes at tiny sizes
    // the initial state is the previous state of the first frame: a still scene
    e = r.launchFlowSnapshot();
    return e == hipSuccess ? r.launchFlow() : e;
}
static void flowRelease(mrx_renderer &r) { r.flowOut.release(); r.flowSnap.release(); }
// per native pixel 4 bytes of depth and 4 of ids read, 16 written
static uint64_t flowBytes(const mrx_renderer &r) { return nativePixels(r.info) * 24ull; }
static const Attached kFlow = { "optical flow: ", flowCreate, flowRelease, flowBytes, nullptr };

// the point cloud: the three tensors, the counts of a split view's parts, the first run of the stage.  Frame and far
// crop are in the renderer already (mrx_cloud_create).
static hipError_t cloudCreate(mrx_renderer &r, uint32_t N)
{
    const uint64_t views = r.info.num_views, slots = views * N;
    const uint64_t pxPerView = (uint64_t)r.info.storage_fast * r.info.storage_slow;
    r.cloudForcedParts = envCount("MRX_CLOUD_PARTS", 0);    // tests: the split at tiny sizes
    const uint64_t parts = mrx::cloudParts(r.info.num_views, pxPerView, r.params.numCUs, r.cloudForcedParts);
    hipError_t e = r.cloudOut.alloc((size_t)slots * 4u);
    if (e == hipSuccess) e = r.cloudPixel.alloc((size_t)slots);
    if (e == hipSuccess) e = r.cloudCount.alloc((size_t)views);
    if (e == hipSuccess) e = r.cloudScratch.alloc((size_t)(views * parts));
    // the empty cloud: zero points, pixel -1 (all bytes 0xFF), count 0
    if (e == hipSuccess) e = hipMemsetAsync(r.cloudOut.ptr, 0, (size_t)slots * 16u, r.stream);
    if (e == hipSuccess) e = hipMemsetAsync(r.cloudPixel.ptr, 0xFF, (size_t)slots * 4u, r.stream);
    if (e == hipSuccess) e = hipMemsetAsync(r.cloudCount.ptr, 0, (size_t)views * 4u, r.stream);
    if (e != hipSuccess)
        return e;
    r.cloudPoints = N;
    return r.launchCloud();
}
static void cloudRelease(mrx_renderer &r)
{
    r.cloudPoints = 0;
    r.cloudOut.release(); r.cloudPixel.release(); r.cloudCount.release(); r.cloudScratch.release();
}
// what the compaction stage reads and writes per step: 4 bytes of depth per native pixel; 20 bytes per slot and a count
static uint64_t cloudBytes(const mrx_renderer &r)
{
    return nativePixels(r.info) * 4ull + (uint64_t)r.info.num_views * ((uint64_t)r.cloudPoints * 20ull + 4ull);
}
static const Attached kCloud = { "point cloud: ", cloudCreate, cloudRelease, cloudBytes, &mrx_renderer::cloudPoints };

// the shadow stage: the mask, the first run in the mask-only form.  Bias and reach are in the renderer already
// (mrx_shadow_create); `mode` is 1 or 2.
static hipError_t shadowCreate(mrx_renderer &r, uint32_t mode)
{
    const uint64_t px = nativePixels(r.info);
    r.shadowBrute = envInt("MRX_SHADOW_BRUTE", 0) != 0;
    r.shadowPassRows = envCount("MRX_SHADOW_PASS_ROWS", 0);     // tests: several staging passes at tiny sizes
    hipError_t e = r.shadowMask.alloc((size_t)px);
    if (e == hipSuccess) e = mrx::prepareShadow();
    if (e == hipSuccess) e = hipMemsetAsync(r.shadowMask.ptr, 0xFF, (size_t)px, r.stream);
    if (e != hipSuccess)
        return e;
    r.shadows = mode;
    return r.launchShadow(false);
}
static void shadowRelease(mrx_renderer &r)
{
    r.shadows = 0;
    r.shadowMask.release();
}
// what the shadow stage reads and writes per step: 4 bytes of depth and the mask's byte per native pixel (what the
// applying form touches on top depends on the image: no fixed term)
static uint64_t shadowBytes(const mrx_renderer &r) { return nativePixels(r.info) * 5ull; }
static const Attached kShadow = { "shadows: ", shadowCreate, shadowRelease, shadowBytes, &mrx_renderer::shadows };

void releaseAttached(mrx_renderer &r)
{
    for (const Attached *a : { &kRays, &kFlow, &kCloud, &kShadow })
        a->release(r);
}

// the stage of one renderer on one device; a failure leaves the renderer without it
static int attachOne(mrx_renderer *r, uint32_t arg, const Attached &a)
{
    MRX_HIP(hipSetDevice(r->device));
    hipError_t e = a.create(*r, arg);
    if (e == hipSuccess) e = hipStreamSynchronize(r->stream);
    if (e != hipSuccess) {
        a.release(*r);
        return fail(MRX_E_HIP, std::string(a.what) + hipGetErrorString(e));
    }
    r->info.bytes_per_step += a.bytes(*r);
    return MRX_OK;
}

// takes the stage off a shard again (a later one failed)
static void detachOne(mrx_renderer *r, const Attached &a)
{
    (void)hipSetDevice(r->device);
    (void)hipStreamSynchronize(r->stream);
    r->info.bytes_per_step -= a.bytes(*r);
    a.release(*r);
}

// an attached stage on the renderer or on every shard of it, all or nothing: a shard that fails takes the stage of the
// shards before it along.  Of a renderer of several devices the parent's "on" field is set, too.
static int attachAll(mrx_renderer *r, uint32_t arg, const Attached &a)
{
    for (size_t i = 0; i < r->shards.size(); ++i) {
        const int rc = attachOne(r->shards[i], arg, a);
        if (rc != MRX_OK) {
            const std::string why = g_err;
            for (size_t k = 0; k < i; ++k)
                detachOne(r->shards[k], a);
            return fail(rc, why);
        }
    }
    if (r->shards.empty())
        if (const int rc = attachOne(r, arg, a))
            return rc;
    if (a.on)
        r->*a.on = arg;
    return MRX_OK;
}

// The prologue of the four mrx_*_create entries, in the order every one of them had it: the device threads caught up,
// the handle, "on a shard", "already attached", the entry's own argument check (made by the caller, who passes the
// text of what failed or an empty string), the tensors the stage needs -- of the first shard: all shards have the same
// --, and the whole renderer's info for the caller's size limits.
struct AttachTexts {
    const char *onShard, *already;
    std::string badArgument;
    const char *needIds = nullptr, *needDepth = nullptr, *needRgb = nullptr, *needNormal = nullptr;    // null: not needed
};
static int attachPrologue(mrx_renderer *r, int stage, const AttachTexts &t, mrx_info_t &whole)
{
    if (const int src = settle(r))
        return src;
    if (!r)
        return fail(MRX_E_INVALID, "null renderer");
    if (r->parent)
        return fail(MRX_E_INVALID, t.onShard);
    if (kStages[stage].on(*r))
        return fail(MRX_E_INVALID, t.already);
    if (!t.badArgument.empty())
        return fail(MRX_E_INVALID, t.badArgument);
    const mrx_renderer *first = r->shards.empty() ? r : r->shards[0];
    if (t.needIds && (!first->ids.ptr || first->params.idsAreSegmask))
        return fail(MRX_E_INVALID, t.needIds);
    if (t.needDepth && !first->depth.ptr)
        return fail(MRX_E_INVALID, t.needDepth);
    if (t.needRgb && !first->rgb.ptr)
        return fail(MRX_E_INVALID, t.needRgb);
    if (t.needNormal && !first->normal.ptr)
        return fail(MRX_E_INVALID, t.needNormal);
    whole = mrx_info_t {};
    return infoFull(r, &whole) != MRX_OK ? (int)MRX_E_INVALID : (int)MRX_OK;
}

// `set` on the renderer and on every shard of it
template <typename F>
static void onAll(mrx_renderer *r, F set)
{
    set(*r);
    for (mrx_renderer *sh : r->shards)
        set(*sh);
}

extern "C" {

int mrx_resolve(mrx_renderer *r) { return runStage(r, kStageResolve); }
int mrx_unproject(mrx_renderer *r) { return runStage(r, kStageUnproject); }
int mrx_boxes(mrx_renderer *r) { return runStage(r, kStageBoxes); }
int mrx_observe(mrx_renderer *r) { return runStage(r, kStageObserve); }
int mrx_trace(mrx_renderer *r) { return runStage(r, kStageTrace); }
int mrx_flow(mrx_renderer *r) { return runStage(r, kStageFlow); }
int mrx_flow_snapshot(mrx_renderer *r) { return runStage(r, kStageFlowSnapshot); }
int mrx_compact(mrx_renderer *r) { return runStage(r, kStageCloud); }
int mrx_shadow(mrx_renderer *r) { return runStage(r, kStageShadowMask); }

int mrx_supersample(mrx_renderer *r)
{
    return r ? (int)r->ss : fail(MRX_E_INVALID, "null renderer");
}

int mrx_positions(mrx_renderer *r)
{
    return r ? (int)r->positions : fail(MRX_E_INVALID, "null renderer");
}

int mrx_box_labels(mrx_renderer *r)
{
    return r ? (int)r->boxLabels : fail(MRX_E_INVALID, "null renderer");
}

int mrx_rays_create(mrx_renderer *r, uint32_t rays_per_world)
{
    AttachTexts t { "mrx_rays_create on a shard: attach the sensor to the renderer it belongs to",
                    "this renderer already has a ray-cast sensor" };
    if (rays_per_world < 1 || rays_per_world > mrx::kRayMaxPerWorld)
        t.badArgument = "rays_per_world " + std::to_string(rays_per_world) + " is not in 1 ... 65536";
    mrx_info_t whole;
    if (const int rc = attachPrologue(r, kStageTrace, t, whole))
        return rc;
    if ((uint64_t)whole.num_worlds * rays_per_world >= (1ull << 31))
        return fail(MRX_E_INVALID, "ray-cast sensor: worlds * rays_per_world reaches 2^31");
    return attachAll(r, rays_per_world, kRays);
}

int mrx_rays(mrx_renderer *r)
{
    return r ? (int)r->raysPerWorld : fail(MRX_E_INVALID, "null renderer");
}

int mrx_set_rays(mrx_renderer *r, uint32_t first_world, uint32_t count, const float *rays)
{
    if (const int src = settle(r))
        return src;
    if (!r || !rays)
        return fail(MRX_E_INVALID, "null argument");
    if (!r->shards.empty())
        return wantsShard("mrx_set_rays");
    if (!r->raysPerWorld)
        return fail(MRX_E_UNSUPPORTED, "no ray-cast sensor: mrx_rays_create was not called on this renderer");
    if ((uint64_t)first_world + count > r->info.num_worlds)
        return fail(MRX_E_INVALID, "mrx_set_rays: worlds past the renderer's last");
    if (count == 0)
        return MRX_OK;
    MRX_HIP(hipSetDevice(r->device));
    const size_t perWorld = (size_t)r->raysPerWorld * 8u;
    MRX_HIP(hipMemcpyAsync(r->rays.ptr + first_world * perWorld, rays, count * perWorld * sizeof(float),
                           hipMemcpyHostToDevice, r->stream));
    MRX_HIP(hipStreamSynchronize(r->stream));
    return MRX_OK;
}

int mrx_flow_create(mrx_renderer *r)
{
    AttachTexts t { "mrx_flow_create on a shard: attach the output to the renderer it belongs to",
                    "this renderer already has the optical-flow output" };
    t.needIds = "optical flow needs visibility ids: create the renderer with MRX_FLAG_VISIBILITY_IDS";
    t.needDepth = "optical flow needs depth: this renderer was created rgb-only (MRX_FLAG_NO_DEPTH)";
    mrx_info_t whole;
    if (const int rc = attachPrologue(r, kStageFlow, t, whole))
        return rc;
    if (nativePixels(whole) > mrx::kFlowMaxPixels)
        return fail(MRX_E_INVALID, "optical flow: more than 2^32 - 1 native pixels");
    return attachAll(r, 0, kFlow);
}

int mrx_flow_enabled(mrx_renderer *r)
{
    if (!r)
        return fail(MRX_E_INVALID, "null renderer");
    return flowOn(r) ? 1 : 0;
}

int mrx_cloud_create(mrx_renderer *r, uint32_t points_per_view, int frame, float max_depth)
{
    AttachTexts t { "mrx_cloud_create on a shard: attach the output to the renderer it belongs to",
                    "this renderer already has the point-cloud output" };
    if (points_per_view < 1 || points_per_view > mrx::kCloudMaxPoints)
        t.badArgument = "points_per_view " + std::to_string(points_per_view) + " is not in 1 ... 65536";
    else if (frame != 1 && frame != 2)
        t.badArgument = "point cloud: frame " + std::to_string(frame) + " is neither 1 (world space) nor 2 (view space)";
    else if (!(max_depth == 0.0f || (std::isfinite(max_depth) && max_depth > 0.0f)))
        t.badArgument = "point cloud: max_depth is 0 (none) or finite and positive";
    t.needDepth = "the point cloud needs depth: this renderer was created rgb-only (MRX_FLAG_NO_DEPTH)";
    mrx_info_t whole;
    if (const int rc = attachPrologue(r, kStageCloud, t, whole))
        return rc;
    if ((uint64_t)whole.num_views * points_per_view >= (1ull << 31))
        return fail(MRX_E_INVALID, "point cloud: views * points_per_view reaches 2^31");
    if ((uint64_t)whole.storage_fast * whole.storage_slow > mrx::kCloudMaxViewPixels ||
        nativePixels(whole) > mrx::kCloudMaxPixels)
        return fail(MRX_E_INVALID, "point cloud: more than 2^32 - 1 native pixels, or more than 2^31 - 1 in a view");
    onAll(r, [&](mrx_renderer &sh) {
        sh.cloudFrame = (uint32_t)frame;
        sh.cloudMaxDepth = max_depth;
    });
    return attachAll(r, points_per_view, kCloud);
}

int mrx_cloud(mrx_renderer *r)
{
    return r ? (int)r->cloudPoints : fail(MRX_E_INVALID, "null renderer");
}

int mrx_shadow_create(mrx_renderer *r, int apply, float bias, float max_distance)
{
    AttachTexts t { "mrx_shadow_create on a shard: attach the stage to the renderer it belongs to",
                    "this renderer already casts shadows" };
    if (!(std::isfinite(bias) && bias >= 0.0f))
        t.badArgument = "shadows: bias is finite and >= 0";
    else if (!(std::isfinite(max_distance) && max_distance > 0.0f))
        t.badArgument = "shadows: max_distance is FLT_MAX (none) or finite and > 0";
    t.needDepth = "shadows need depth: this renderer was created rgb-only (MRX_FLAG_NO_DEPTH)";
    if (apply) {
        t.needRgb = "shadows with apply need rgb: this renderer was created depth-only (MRX_FLAG_NO_RGB)";
        t.needNormal = "shadows with apply need the normal tensor: create the renderer with MRX_FLAG_NORMALS";
    }
    mrx_info_t whole;
    if (const int rc = attachPrologue(r, kStageShadow, t, whole))
        return rc;
    if (nativePixels(whole) > mrx::kShadowMaxPixels)
        return fail(MRX_E_INVALID, "shadows: more than 2^32 - 1 native pixels");
    onAll(r, [&](mrx_renderer &sh) {
        sh.shadowBias = bias;
        sh.shadowMaxDistance = max_distance;
    });
    return attachAll(r, apply ? 2u : 1u, kShadow);
}

int mrx_shadows(mrx_renderer *r)
{
    return r ? (int)r->shadows : fail(MRX_E_INVALID, "null renderer");
}

int mrx_observations(mrx_renderer *r)
{
    if (!r)
        return fail(MRX_E_INVALID, "null renderer");
    return r->obsLayout ? (int)MRX_FLAG_OBSERVATIONS(r->obsLayout, r->obsDtype, r->obsStack) : 0;
}

int mrx_set_observation_depth_range(mrx_renderer *r, float lo, float hi)
{
    if (const int src = settle(r))
        return src;
    if (!r)
        return fail(MRX_E_INVALID, "null renderer");
    if (!r->obsLayout)
        return fail(MRX_E_UNSUPPORTED, "no observation depth range: this renderer was created without MRX_FLAG_OBSERVATIONS");
    const bool unset = lo == 0.0f && hi == 0.0f;
    if (!unset && !(std::isfinite(lo) && std::isfinite(hi) && lo >= 0.0f && lo < hi))
        return fail(MRX_E_INVALID, "observation depth range: 0 <= lo < hi, both finite (0, 0: no range)");
    if (!unset && !mrx::observeReadsDepth(r->obsLayout))
        return fail(MRX_E_INVALID, "observation depth range: this renderer's layout has no depth channel");
    // S15: a float32 subtract and a float32 divide
    const float span = hi - lo;
    const float inv = unset ? 0.0f : 1.0f / span;
    onAll(r, [&](mrx_renderer &sh) {
        sh.obsLo = unset ? 0.0f : lo;
        sh.obsHi = unset ? 0.0f : hi;
        sh.obsInv = inv;
    });
    // frames packed under another range are meaningless: every stack restarts from the frame packed now
    if (!r->shards.empty())
        return shardsRun(r, kCmdObserveRestart);
    MRX_HIP(hipSetDevice(r->device));
    MRX_HIP(r->markObservationsReset());
    MRX_HIP(r->launchObserve());
    return MRX_OK;
}

int mrx_observation_depth_range(mrx_renderer *r, float *lo, float *hi)
{
    if (!r || !lo || !hi)
        return fail(MRX_E_INVALID, "null argument");
    if (!r->obsLayout)
        return fail(MRX_E_UNSUPPORTED, "no observation depth range: this renderer was created without MRX_FLAG_OBSERVATIONS");
    *lo = r->obsLo;
    *hi = r->obsHi;
    return MRX_OK;
}

}  // extern "C"
