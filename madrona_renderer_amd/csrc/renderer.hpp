// What the host units of libmrx_hip.so share (mrx_api.cpp, scene.cpp, stages.cpp, host_tools.cpp): the HIP error
// macro, device buffers, the renderer behind the C ABI's handle and the functions that cross a unit's border.
#pragma once

#include "../../include/mrx.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "bvh.hpp"
#include "raster.hpp"
#include "flow.hpp"
#include "cloud.hpp"
#include "shadow.hpp"
#include "error.hpp"
#include "shards.hpp"

#define MRX_HIP(call)                                                          \
    do {                                                                       \
        hipError_t e_ = (call);                                                \
        if (e_ != hipSuccess)                                                  \
            return fail(MRX_E_HIP, std::string(#call) + ": " +                 \
                                       hipGetErrorString(e_));                 \
    } while (0)

#pragma GCC visibility push(hidden)

template <typename T>
struct DevBuf {
    T *ptr = nullptr;
    size_t count = 0;
    bool owned = true;
    void *base = nullptr;                       // what hipMalloc returned (ptr may sit inside it)
    // diagnostic (MRX_OUT_ALLOC=vmm): the block comes from the virtual-memory API instead --
    // one physical handle mapped at a reserved address
    hipMemGenericAllocationHandle_t vmmHandle {};
    size_t vmmSize = 0;
    hipError_t alloc(size_t n, size_t tailBytes = 0)     // tail: room for slices (view) behind the data
    {
        count = n;
        owned = true;
        const hipError_t e = hipMalloc(&base, (n ? n : 1) * sizeof(T) + tailBytes);
        ptr = e == hipSuccess ? static_cast<T *>(base) : nullptr;
        return e;
    }
    hipError_t allocVmm(size_t n, size_t tailBytes, int device)
    {
        count = n;
        owned = true;
        hipMemAllocationProp prop {};
        prop.type = hipMemAllocationTypePinned;
        prop.location.type = hipMemLocationTypeDevice;
        prop.location.id = device;
        size_t gran = 0;
        hipError_t e = hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended);
        if (e != hipSuccess)
            return e;
        if (const char *dbg = std::getenv("MRX_OUT_VMM_GRAN_MB"))
            gran = std::max<size_t>(gran, (size_t)std::atoll(dbg) << 20);
        const size_t bytes = ((n ? n : 1) * sizeof(T) + tailBytes + gran - 1) / gran * gran;
        e = hipMemCreate(&vmmHandle, bytes, &prop, 0);
        if (e != hipSuccess)
            return e;
        e = hipMemAddressReserve(&base, bytes, gran, nullptr, 0);
        if (e == hipSuccess)
            e = hipMemMap(base, bytes, 0, vmmHandle, 0);
        if (e == hipSuccess) {
            hipMemAccessDesc acc {};
            acc.location = prop.location;
            acc.flags = hipMemAccessFlagsProtReadWrite;
            e = hipMemSetAccess(base, bytes, &acc, 1);
        }
        if (e != hipSuccess) {
            (void)hipMemRelease(vmmHandle);
            base = nullptr;
            return e;
        }
        vmmSize = bytes;
        ptr = static_cast<T *>(base);
        return hipSuccess;
    }
    void view(void *base, size_t n)             // a slice of another allocation (not owned)
    {
        ptr = static_cast<T *>(base);
        this->base = nullptr;
        count = n;
        owned = false;
    }
    hipError_t upload(const std::vector<T> &h)
    {
        hipError_t e = alloc(h.size());
        if (e != hipSuccess || h.empty())
            return e;
        return hipMemcpy(ptr, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
    }
    // upload again after the host table changed (mrx_refresh_objects): in place when the size fits
    hipError_t reupload(const std::vector<T> &h)
    {
        if (ptr && owned && h.size() <= count && !vmmSize) {
            if (h.empty())
                return hipSuccess;
            return hipMemcpy(ptr, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
        }
        release();
        return upload(h);
    }
    void release()
    {
        if (base && owned && vmmSize) {
            (void)hipMemUnmap(base, vmmSize);
            (void)hipMemRelease(vmmHandle);
            (void)hipMemAddressFree(base, vmmSize);
            vmmSize = 0;
        } else if (base && owned) {
            (void)hipFree(base);
        }
        ptr = nullptr;
        base = nullptr;
    }
};

struct mrx_renderer {
    int device = 0;
    hipStream_t stream = nullptr;
    int32_t mode = MRX_MODE_RASTERIZER;
    uint32_t flags = 0;
    int32_t variant = 0;
    uint64_t stepCount = 0;
    mrx_info_t info {};
    mrx::RasterParams params {};
    // host copies kept for mrx_copy_triangles
    std::vector<mrx::ObjTri> hostTris;
    std::vector<int32_t> objFirst, objCount;
    // device state
    DevBuf<mrx::ObjTri> tris;
    DevBuf<mrx::TriMat> triMats;
    DevBuf<mrx::TexDesc> textures;
    DevBuf<uint32_t> texels;
    DevBuf<mrx::WorldTri> viewTris;
    DevBuf<uint32_t> viewTriCount;
    // the pose tensors are slices of one block, the geometry tables of another, at offsets that follow
    // from the counts (raster.hpp poseLayout / geomMatsOffset): the group kernel's fast prologue derives
    // their addresses from two base pointers that reach it preloaded in SGPRs
    DevBuf<uint8_t> poseBlock, geomBlock;
    DevBuf<float> instPos, instRot, instScale, camPos, camRot;
    DevBuf<int32_t> instObj;
    // the colour override column (MRX_FLAG_INSTANCE_COLORS): the slice of the pose block behind
    // instObj; no pointer without the flag
    DevBuf<uint32_t> instColor;
    // the material override column (MRX_FLAG_INSTANCE_MATERIALS): the slice of the pose block behind
    // the colour column's slot; no pointer without the flag.  matTable: the renderer's material table as the kernels
    // read it, one spare record past its end; anyMatTextured: some material of it has a texture
    DevBuf<int32_t> instMat;
    DevBuf<mrx::MatRec> matTable;
    bool anyMatTextured = false;
    // pinned staging of mrx_set_instance_materials, one word per row, and the event behind its last copy
    int32_t *matStage = nullptr;
    hipEvent_t matEv = nullptr;
    bool matCopyPending = false;
    // the label column (MRX_FLAG_INSTANCE_LABELS): the slice of the pose block behind the material
    // column's slot; no pointer without the flag.  Staging and event of mrx_set_instance_labels as the material column's.
    DevBuf<int32_t> instLabel;
    int32_t *labelStage = nullptr;
    hipEvent_t labelEv = nullptr;
    bool labelCopyPending = false;
    DevBuf<uint32_t> rgb;
    DevBuf<float> depth;
    DevBuf<int32_t> ids;
    DevBuf<uint32_t> normal;                    // MRX_FLAG_NORMALS; no pointer without the flag
    // supersampling: with ss > 1 everything above is the renderer of ss * W x ss * H views -- the
    // four tensors hold the samples -- and these are the native tensors the resolve stage writes, the ones a caller
    // sees; info.storage_fast / storage_slow are native.  ss == 1: no pointers, no second launch.
    uint32_t ss = 1;
    DevBuf<uint32_t> outRgb;
    DevBuf<float> outDepth;
    DevBuf<int32_t> outIds;
    DevBuf<uint32_t> outNormal;
    // the tensors the caller sees, as the stages behind the resolve read them (at every launch: the placement search
    // re-binds the render's)
    uint32_t *seenRgb() const { return ss > 1 ? outRgb.ptr : params.rgb; }
    float *seenDepth() const { return ss > 1 ? outDepth.ptr : params.depth; }
    int32_t *seenIds() const { return ss > 1 ? outIds.ptr : params.ids; }
    uint32_t *seenNormal() const { return ss > 1 ? outNormal.ptr : params.normal; }
    // position output: 0 none, 1 world space, 2 view space (mrx_positions); the xyzw tensor the
    // unprojection stage writes from the depth tensor the caller sees -- an allocation of its own, outside allocOutputs
    // and the placement search.  0: no pointer, no further launch.
    uint32_t positions = 0;
    DevBuf<float> position;
    // box labels: K (mrx_box_labels) and the [views][K][5] tensor the box stage writes from the
    // ids tensor the caller sees -- an allocation of its own, outside allocOutputs and the placement search.  0: no
    // pointer, no further launch.  boxParts: MRX_BOX_PARTS, the forced number of workgroups per view (0: automatic).
    uint32_t boxLabels = 0, boxParts = 0;
    DevBuf<int32_t> boxes;
    // packed observation output: the field of the flags (mrx_observations), its parts, the
    // [views][S * C][H][W] tensor the observation stage writes from the rgb and depth tensors the caller sees and, with
    // S > 1, the reset column -- allocations of their own, outside allocOutputs and the placement search.  obsLayout 0:
    // no pointer, no further launch.  obsLo / obsHi: the depth range, both 0 without one; obsInv = 1.0f / (hi - lo).
    uint32_t obsLayout = 0, obsDtype = 0, obsStack = 1;
    float obsLo = 0.0f, obsHi = 0.0f, obsInv = 0.0f;
    DevBuf<uint8_t> obs, obsReset;
    // ray-cast sensor (mrx_rays_create): R rays per world, the two input tensors, the two outputs
    // and the per-row table of bound object ids the stage stores -- allocations of their own, outside allocOutputs and
    // the placement search.  R == 0: no pointer, no further launch.  rayBrute: MRX_RAYS_BRUTE, the form without culls;
    // rayPassRows: MRX_RAY_PASS_ROWS, the forced number of rows per staging pass (0: the default).
    uint32_t raysPerWorld = 0, rayPassRows = 0;
    bool rayBrute = false;
    DevBuf<float> rays, rayT;
    DevBuf<int32_t> rayFrame, rayId, rayBound;
    // optical-flow output (mrx_flow_create): the [views][H][W][4] tensor the flow stage writes and
    // the snapshot of last step's pose, scale and camera columns and projection constants it reads -- allocations of
    // their own, outside allocOutputs and the placement search.  No pointer: no further launch.  flowPassRows:
    // MRX_FLOW_PASS_ROWS, the forced number of rows per staging pass (0: the default).
    DevBuf<float> flowOut, flowSnap;
    uint32_t flowPassRows = 0;
    // point-cloud output (mrx_cloud_create): N points per view, the frame (1 world, 2 view space:
    // mrx_positions' values) and the far crop (0: none); the [views][N][4] points, the [views][N] pixel indices and the
    // [views] counts the compaction stage writes from the depth tensor the caller sees, and the [views][parts] counts of
    // a split view's parts -- allocations of their own, outside allocOutputs and the placement search.  N == 0: no
    // pointer, no further launch.  cloudForcedParts: MRX_CLOUD_PARTS, the forced number of workgroups per view (0: automatic).
    uint32_t cloudPoints = 0, cloudFrame = 0, cloudForcedParts = 0;
    float cloudMaxDepth = 0.0f;
    DevBuf<float> cloudOut;
    DevBuf<int32_t> cloudPixel, cloudCount;
    DevBuf<uint32_t> cloudScratch;
    // cast shadows (mrx_shadow_create): 0 off, 1 the mask, 2 the mask and the darkened rgb
    // (mrx_shadows); the bias and the reach of the shadow rays; the [views][storage_slow][storage_fast] u8 mask the
    // shadow stage writes from the depth tensor the caller sees -- an allocation of its own, outside allocOutputs and
    // the placement search.  0: no pointer, no further launch.  shadowBrute: MRX_SHADOW_BRUTE, the form without culls;
    // shadowPassRows: MRX_SHADOW_PASS_ROWS, the forced number of rows per staging pass (0: the default).
    uint32_t shadows = 0, shadowPassRows = 0;
    bool shadowBrute = false;
    float shadowBias = 0.0f, shadowMaxDistance = 0.0f;
    DevBuf<uint8_t> shadowMask;
    DevBuf<unsigned long long> stamps;
    // XCD phase feedback (raster.hip): a host-mapped word workgroup 0 reports its XCC id to
    uint32_t *xccHost = nullptr, *xccDev = nullptr;
    int32_t xcdPhaseForced = -1;                // MRX_XCD_PHASE: 0 / 1 override (tests)
    uint32_t launches = 0;
    // BVH path: BLAS (built at load) and the tables the per-step TLAS reads
    DevBuf<mrx::BvhNode> bvhNodes;
    DevBuf<uint32_t> bvhLeafTris, worldInstStart, viewWorld, instKBase;
    DevBuf<mrx::ObjInfo> objInfo;
    bool useBvh = false;
    int32_t lastEntry = mrx::kEntryNone;        // the kernel the last launch() ran (mrx_raster_entry)
    mrx::LaunchForm lastForm;                   // ... and its instantiation: form and group slots (mrx_kernel_form)
    // host copies the geometry binding is (re)built from (bindGeometry): the object each
    // instance row is bound to, the world -> row and view -> world tables, the BLAS set
    std::vector<int32_t> boundObj;
    std::vector<uint32_t> worldInstStartHost, viewWorldHost, worldCams;
    std::vector<mrx::TriMat> triMatsHost;
    mrx::BlasSet blas;
    uint32_t bvhMinTris = mrx::kBvhMinTris;
    uint32_t bvhGroupTilesGeneral = 1;          // tiles of a view per workgroup as bvhTileKernel wants them (buildScene)
    // single-process multi-device (mrx_config.device_ids): a renderer that only fans out to
    // one sub-renderer per device, each owning a contiguous range of the worlds
    std::vector<mrx_renderer *> shards;
    std::vector<uint32_t> shardFirstWorld;      // [shards + 1]
    ShardSet shardSet;                          // the host threads that run the shards' commands (shards.hpp)
    mrx_renderer *parent = nullptr;             // of a shard: the renderer it belongs to
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // what choosePlacement measured (mrx_placement): us per render of every candidate
    // output allocation it timed, in order, and of the one it kept
    std::vector<float> placementUs;
    float placementKeptUs = 0.0f;
    // per-view projection: the projection of every view of this renderer (defaults resolved), its
    // device table (launched with only while the views differ: params.viewProj), the pinned staging the table is
    // copied from on the stream, and the event after the last such copy (the staging is reused once it has passed)
    std::vector<mrx_projection> proj;
    DevBuf<mrx::ViewProj> projDev;
    mrx::ViewProj *projStage = nullptr;
    hipEvent_t projEv = nullptr;
    bool projCopyPending = false;
    // per-world light: the light of every world of this renderer as the caller gave it, and the
    // per-view device table with its staging -- filled and copied together with the projection table, behind the
    // same event: the kernels' per-view instantiations read both
    std::vector<mrx_light> lights;
    DevBuf<mrx::ViewLight> lightDev;
    mrx::ViewLight *lightStage = nullptr;

    // a step's launches: the render and behind it, on the same stream, every stage that is on, in the order of the
    // stage table (stages.cpp kStages)
    hipError_t launch();
    hipError_t launchRender();
    // the stages' launches (stages.cpp)
    hipError_t launchResolve();
    hipError_t launchUnproject();
    hipError_t launchBoxes();
    hipError_t launchObserve();
    hipError_t markObservationsReset();
    hipError_t launchRays();
    mrx::FlowParams flowParams();
    hipError_t launchFlow();
    hipError_t launchFlowSnapshot();
    hipError_t launchCloud();
    hipError_t launchShadow(bool apply);        // apply: a step's form of a renderer with shadows == 2

    ~mrx_renderer();
};

// ---- stages.cpp
// the stage fields of a renderer from its creation flags (a single-device renderer, a shard, a multi-device parent)
void decodeStageFlags(uint32_t flags, mrx_renderer &r);
// at creation, behind buildScene: the tensors of the stages the flags switch on
int allocStages(mrx_renderer &r);
// at teardown: the buffers of the stages attached later (mrx_rays_create ... mrx_shadow_create)
void releaseAttached(mrx_renderer &r);
uint32_t supersampleOf(uint32_t flags);
uint32_t positionsOf(uint32_t flags);
uint32_t boxLabelsOf(uint32_t flags);
uint32_t obsLayoutOf(uint32_t flags);
// shards: what a group does for a command, a renderer's device threads caught up, a command on every shard
int groupRun(const ShardGroup &group, int cmd, int steps, bool bindDevice);
int settle(mrx_renderer *r);
int shardsRun(mrx_renderer *r, int cmd, int steps = 0);
void startShardWorkers(mrx_renderer *r);

// ---- scene.cpp
int projectionConstants(uint32_t W, uint32_t H, bool rt, const mrx_projection &in, mrx::ViewProj &out,
                        mrx_projection *resolved = nullptr);
int lightConstants(const mrx_light &in, mrx::ViewLight &out);
hipError_t uploadRayBound(mrx_renderer &r);
int bindGeometry(mrx_renderer &r);
int applyViewTables(mrx_renderer &r);
int buildScene(const mrx_config &cfg, mrx_renderer &r);

// ---- mrx_api.cpp
bool firstKindIsOneBlock(size_t px);
hipError_t allocOutputs(size_t px, bool wantRgb, bool wantDepth, bool wantIds, bool oneAllocation,
                        DevBuf<uint32_t> &rgb, DevBuf<float> &depth, DevBuf<int32_t> &ids,
                        bool wantNormal, DevBuf<uint32_t> &normal);
int wantsShard(const char *what);
int infoFull(mrx_renderer *r, mrx_info_t *out);

#pragma GCC visibility pop
