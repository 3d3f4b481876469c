// madRender::Manager -- the host C++ API of the batch renderer, kept
// member-for-member with the reference's class
// (/root/reference/src/mgr.hpp:29-120) so callers such as
// /root/reference/src/headless.cpp:48-61 and src/bindings.cpp:183-233 keep
// working.  The implementation (madrona_renderer_amd/csrc/manager.cpp) is a
// thin layer over the C-ABI in include/mrx.h; all rendering happens in HIP
// kernels on the MI355X.
#pragma once

#include <memory>
#include <string>

#include "types.hpp"

namespace madRender {

using AdditionalMaterial = madrona::imp::SourceMaterial;

struct ImportedAsset {
    std::string path;
    int32_t matID;   // index into the additional materials, -1 = none
};

class Manager {
public:
    enum class RenderMode { Rasterizer, Raytracer };
    // Which outputs a step renders (the engine's render-config RenderMode RGBD / Depth, plus colour
    // only): an output that is not rendered has no tensor -- its getters fail as segmaskTensor()
    // does in Rasterizer mode.  The segmask (Raytracer mode) is rendered under every setting.
    enum class RenderOutputs { RGBD, Depth, RGB };
    // The projection of a camera (attachEntityToView's vfov / znear, src/sim.cpp:168-171): degrees, 0 < vfov < 180;
    // znear > 0, 0 = the mode's default (Raytracer mode: below its far plane, 1000).  {90, 0} is every view's default.
    struct CameraProjection { float vfovDeg; float znear; };
    // The directional light of a world: the direction the light travels (any length but zero) and the two constants
    // of lit = fma(diffuse, max(n.l, 0), ambient), both >= 0.  {(1, -1, -0.05), 0.25, 0.75} is every world's default.
    struct Light { float direction[3]; float ambient; float diffuse; };

    struct GeometryConfig {
        const madrona::math::Vector3 *vertices;
        const madrona::math::Vector2 *uvs;
        const uint32_t *indices;
        const uint32_t *meshVertexOffsets;
        const uint32_t *meshIndexOffsets;
        const int32_t *meshMaterials;
        uint32_t numVertices;
        uint32_t numIndices;
        uint32_t numMeshes;
    };

    struct Config {
        int gpuID;
        uint32_t numWorlds;
        RenderMode renderMode;
        uint32_t batchRenderViewWidth = 64;
        uint32_t batchRenderViewHeight = 64;
        madrona::render::APIBackend *extRenderAPI = nullptr;  // ignored
        madrona::render::GPUDevice *extRenderDev = nullptr;   // ignored
        bool headlessMode = false;

        struct RenderConfig {
            GeometryConfig geoCfg;
            const char **assetPaths;
            uint32_t numAssetPaths;
            int32_t *matAssignments;
            uint32_t numMatAssignments;
            const AdditionalMaterial *additionalMats;
            uint32_t numAdditionalMats;
            const char **additionalTextures;
            uint32_t numAdditionalTextures;
            ImportedInstance *importedInstances;
            uint32_t numInstances;
            ImportedCamera *cameras;
            uint32_t numCameras;
            Sim::WorldInit *worlds;
        } rcfg;

        // ---- additions (trailing, defaulted: the reference's initialisers keep compiling) ----
        // Single-process multi-device: with numDevices > 1 this one Manager spans deviceIDs[0 ..
        // numDevices) -- the worlds are split into contiguous ranges, one shard (own tensors, own
        // launch) per listed device, step() launches on all of them; gpuID is then ignored.
        const int *deviceIDs = nullptr;
        uint32_t numDevices = 0;
        // Rows per world at least (the reference's maxInstancesPerWorld, src/mgr.cpp:378-388):
        // spare rows start hidden and unbound, see refreshObjects().
        uint32_t maxInstancesPerWorld = 0;
        // Outputs rendered (MRX_FLAG_NO_RGB / MRX_FLAG_NO_DEPTH): RGBD = both, as the reference.
        RenderOutputs renderOutputs = RenderOutputs::RGBD;
        // [numCameras] projections parallel to rcfg.cameras (nullptr: every camera {90, 0}); a view takes its
        // camera row's, as it takes its pose.
        const CameraProjection *cameraProjections = nullptr;
        // [numWorlds] lights (nullptr: every world the default light); every view of a world takes its world's.
        const Light *worldLights = nullptr;
        // Per-instance colour override (MRX_FLAG_INSTANCE_COLORS): [numInstances][4] bytes (r, g, b, a) parallel to
        // rcfg.importedInstances, the initial values of instanceColorTensor(); a == 0 = the material colour.
        // nullptr with instanceColorColumn: a zero-filled column; nullptr without: no column.
        const uint8_t *instanceColors = nullptr;
        bool instanceColorColumn = false;
        // Per-instance material override (MRX_FLAG_INSTANCE_MATERIALS): [numInstances] material ids parallel to
        // rcfg.importedInstances, the initial values of instanceMaterialTensor(); an id outside the material table
        // (-1, say) = the triangles' own materials.  Expanded per world as the poses are: worlds that alias rows
        // share ids, spare rows get -1.  nullptr with instanceMaterialColumn: a column of -1; nullptr without: none.
        const int32_t *instanceMaterials = nullptr;
        bool instanceMaterialColumn = false;
        // Surface-normal output (MRX_FLAG_NORMALS): normalTensor() holds the view-space normal of every pixel's
        // winning triangle, RGBA8-encoded; combines with every renderOutputs setting.
        bool normals = false;
        // Per-instance labels (MRX_FLAG_INSTANCE_LABELS): [numInstances] int32 labels parallel to
        // rcfg.importedInstances, the initial values of instanceLabelTensor(); kLabelObject = the id of the row's bound
        // object.  Expanded per world as the poses are: worlds that alias rows share labels, spare rows get
        // kLabelObject.  nullptr with instanceLabelColumn: a column of kLabelObject; nullptr without: none.  With the
        // column segmaskTensor() exists in Rasterizer mode too and holds the label of the row that wins each pixel.
        const int32_t *instanceLabels = nullptr;
        bool instanceLabelColumn = false;
        // Supersampled antialiasing (MRX_FLAG_SUPERSAMPLE_MASK): 1 ... 4; with s > 1 every view is rendered at s times
        // the width and height and resolved to the configured size -- rgb box-filtered, depth, normals and the ids
        // tensor point-sampled -- so every tensor getter keeps its shape.
        uint32_t supersample = 1;
        // Position output (MRX_FLAG_POSITIONS / _VIEW): 0 none, 1 world space, 2 view space; positionTensor() then holds
        // the point every pixel sees, computed from depth by a stage behind every render.  Needs depth rendered.
        uint32_t positions = 0;
        // Box labels (MRX_FLAG_BOX_LABELS): K in 1 ... 1024, 0 none; boxTensor() then holds the 2-D bounding box and the
        // pixel count of every label 0 ... K-1 in every view, computed from the segmask by a stage behind every render.
        // Needs a segmask: Raytracer mode, or Rasterizer mode with the label column.
        uint32_t boxLabels = 0;
        // Packed observation output (MRX_FLAG_OBSERVATIONS): the field's value, MRX_FLAG_OBSERVATIONS(layout, dtype,
        // stack), 0 none; observationTensor() then holds the channel-first tensor a policy takes -- [views, S * C, H, W]
        // in float32, float16, bfloat16 or uint8 -- packed from rgb and depth by a stage behind every render.  A
        // layout needs the outputs it reads rendered.
        uint32_t observations = 0;
        // Ray-cast sensor (mrx_rays_create): R rays per world in 1 ... 65536, 0 none; rayTensor() / rayFrameTensor() then
        // take the rays and the row they are mounted on, and a trace stage behind every render writes
        // rayDistanceTensor() and rayIdTensor().
        uint32_t raysPerWorld = 0;
        // Optical-flow output (mrx_flow_create): flowTensor() then holds, per native pixel, the image-space displacement
        // since the previous step of the surface point the pixel sees, computed by a stage behind every render from a
        // device snapshot of last step's poses, cameras and projections.  Sets the visibility-ids flag, as
        // MADRONA_MI355_VISIBILITY=1 does: the ids tensor then holds visibility ids, so segmaskTensor() and boxLabels are
        // unavailable.  Needs depth rendered.
        bool flow = false;
    };
    // the label that stands for the id of the object a row is bound to (MRX_LABEL_OBJECT)
    static constexpr int32_t kLabelObject = INT32_MIN;

    // Aborts (FATAL-style, like the reference) when construction fails.
    Manager(const Config &cfg);
    ~Manager();

    void step();     // advance + render, asynchronous on the renderer's stream
    void render();   // the render half of step()
    void sync();     // wait for everything enqueued so far

    // (the tensor getters take the shard of a multi-device Manager; a Manager of one device
    // has shard 0 only, so the reference's argument-less calls are unchanged)
    madrona::py::Tensor rgbTensor(uint32_t shard = 0) const;
    madrona::py::Tensor depthTensor(uint32_t shard = 0) const;
    madrona::py::Tensor segmaskTensor(uint32_t shard = 0) const;

    madrona::py::Tensor instancePositionTensor(uint32_t shard = 0) const;
    madrona::py::Tensor instanceRotationTensor(uint32_t shard = 0) const;

    madrona::py::Tensor cameraPositionTensor(uint32_t shard = 0) const;
    madrona::py::Tensor cameraRotationTensor(uint32_t shard = 0) const;

    uint64_t rgbCudaPtr(uint32_t shard = 0) const;
    uint64_t depthCudaPtr(uint32_t shard = 0) const;
    uint64_t segmaskCudaPtr(uint32_t shard = 0) const;

    // Additions with no counterpart in the reference (measurement / tests).
    madrona::py::Tensor visibilityTensor(uint32_t shard = 0) const;   // needs MADRONA_MI355_VISIBILITY=1
    // i32 [instances], mutable: negative hides the instance from the next step on
    // (the ObjectID column, src/sim.cpp:152-156; src/sim.inl:5-16)
    madrona::py::Tensor instanceObjectTensor(uint32_t shard = 0) const;
    madrona::py::Tensor instanceScaleTensor(uint32_t shard = 0) const;
    // u8 [instances, 4], mutable: the colour override (r, g, b, a) of every row, a == 0 = none (upstream's
    // per-renderable colour override; needs Config::instanceColors or instanceColorColumn)
    madrona::py::Tensor instanceColorTensor(uint32_t shard = 0) const;
    // i32 [instances], mutable: the material override of every row, outside the material table = none (upstream's
    // per-renderable material override; needs Config::instanceMaterials or instanceMaterialColumn)
    madrona::py::Tensor instanceMaterialTensor(uint32_t shard = 0) const;
    // u8 [views, H, W, 4] (Raytracer: [views, res, res, 4] transposed, as rgb): the flat view-space normal of the
    // pixel's winning triangle turned towards the eye, byte = 128 + 127 * component, alpha 255; background
    // (128, 128, 128, 0).  Needs Config::normals.
    madrona::py::Tensor normalTensor(uint32_t shard = 0) const;
    // i32 [instances], mutable: the label of every row, kLabelObject = the id of its bound object; what segmaskTensor()
    // holds on the pixels the row wins (needs Config::instanceLabels or instanceLabelColumn)
    madrona::py::Tensor instanceLabelTensor(uint32_t shard = 0) const;
    // supersampling: the factor; the s * W x s * H tensor the render writes for an output id (MRX_BUF_RGB, _DEPTH,
    // _SEGMASK, _VISIBILITY, _NORMAL; fatal at factor 1 or on an output that is not rendered); the resolve stage alone
    uint32_t supersample() const;
    madrona::py::Tensor sampleTensor(int which, uint32_t shard = 0) const;
    void resolve();
    // position output: 0 none / 1 world / 2 view; f32 [views, H, W, 4] (Raytracer: [views, res, res, 4] transposed, as
    // rgb): (x, y, z, 1) of the point the pixel's depth stands for, (0, 0, 0, 0) on background (fatal without
    // Config::positions); the unprojection stage alone
    uint32_t positions() const;
    madrona::py::Tensor positionTensor(uint32_t shard = 0) const;
    void unproject();
    // box labels: K or 0; i32 [views, K, 5] = (xmin, ymin, xmax, ymax, count) in image coordinates in both modes,
    // (W, H, -1, -1, 0) for a label no pixel holds (fatal without Config::boxLabels); the box stage alone
    uint32_t boxLabels() const;
    madrona::py::Tensor boxTensor(uint32_t shard = 0) const;
    void boxes();
    // packed observation output: the field or 0; [views, S * C, H, W] in the field's element type, image rows and
    // columns in both modes, frame 0 the oldest (fatal without Config::observations); the reset column u8 [views]
    // (fatal with a stack of 1); the observation stage alone -- on a stacked renderer one more frame; the depth range
    // (lo = hi = 0: none), whose setter restarts every stack
    uint32_t observations() const;
    madrona::py::Tensor observationTensor(uint32_t shard = 0) const;
    madrona::py::Tensor observationResetTensor(uint32_t shard = 0) const;
    void observe();
    void setObservationDepthRange(float lo, float hi);
    void observationDepthRange(float *lo, float *hi) const;
    // ray-cast sensor: R or 0; f32 [worlds, R, 8] rays (ox, oy, oz, tmin, dx, dy, dz, tmax) and i32 [worlds] mount rows
    // (-1: world frame), both mutable; f32 [worlds, R] the parameter t of the nearest hit (tmax on a miss) and i32
    // [worlds, R] the segmask value of the row that was hit (-1 on a miss) (fatal without Config::raysPerWorld); the
    // trace stage alone
    uint32_t rays() const;
    madrona::py::Tensor rayTensor(uint32_t shard = 0) const;
    madrona::py::Tensor rayFrameTensor(uint32_t shard = 0) const;
    madrona::py::Tensor rayDistanceTensor(uint32_t shard = 0) const;
    madrona::py::Tensor rayIdTensor(uint32_t shard = 0) const;
    void trace();
    // optical-flow output: whether there is one; f32 [views, H, W, 4] (Raytracer: [views, res, res, 4] transposed, as
    // rgb): (dx, dy, dz, 1) -- the point pixel (x, y) sees was at (x - dx, y - dy) at the previous step, dz the change of
    // depth -- and (0, 0, 0, 0) where there is none (fatal without Config::flow); the flow stage alone, which leaves
    // the snapshot as it is; the snapshot stage alone, which makes the current state the previous one
    bool flows() const;
    madrona::py::Tensor flowTensor(uint32_t shard = 0) const;
    void flow();
    void flowSnapshot();
    // binds every row to the (non-negative) object id its ObjectID column now holds: a spare
    // row gets its geometry, an existing row swaps it (makeEntityRenderable at run time,
    // src/sim.inl:5-8); waits for the device
    void refreshObjects();
    uint32_t numShards() const;                     // devices this Manager spans
    // worlds [shardFirstWorld(i), shardFirstWorld(i + 1)) live on shard i
    uint32_t shardFirstWorld(uint32_t shard) const;
    float timeRenders(int steps);                   // device ms for `steps` renders
    double timeStepsHost(int steps);                // host us per step() call, `steps` calls back to back
    void mark(int which);                           // HIP event 0/1 on the stream
    float elapsedMs();                              // event1 - event0, waits for 1
    uint64_t bytesPerStep() const;                  // algorithmic HBM bytes / render
    void *nativeHandle() const;                     // mrx_renderer *
    // output placement as mrx_placement reports it: candidates timed at creation
    int placement(float *candUs, int capacity, float *keptUs) const;
    void setStream(void *hipStream);                // launch on this stream from now on
    void setShardStream(uint32_t shard, void *hipStream);   // the same for one shard of several
    const char *renderPath() const;                 // "raster" (tiled raster kernels) or "bvh"
    // the kernel the last render launched (mrx_raster_entry): "group-fast", "group", "chunked", "brute",
    // "bvh", or "none" before the first render
    const char *rasterEntry() const;
    // the instantiation of that kernel (mrx_kernel_form): the form's name -- "Uniform", "PV", "PVL", "C", "PVLC", "M",
    // "PVLM", "N", "NPV", "L", "LN", "PVM"  -- and the group kernel's triangle slots per view (0 for
    // every other kernel)
    struct KernelFormInfo {
        const char *form;
        int32_t slots;
    };
    KernelFormInfo kernelForm() const;
    // per-view projection (views of the whole job): set views [first, first + count) -- stream-ordered, the next
    // step renders with them; false (and nothing changed) when a value is out of range -- and read them back
    bool setViewProjection(uint32_t first, uint32_t count, const CameraProjection *proj);
    void viewProjection(uint32_t first, uint32_t count, CameraProjection *out) const;
    uint32_t numViews() const;
    // per-world light (worlds of the whole job): set worlds [first, first + count) -- stream-ordered, the next step
    // renders with them; false (and nothing changed) when a value is refused -- and read back what was set
    bool setWorldLights(uint32_t first, uint32_t count, const Light *lights);
    void worldLights(uint32_t first, uint32_t count, Light *out) const;
    uint32_t numWorlds() const;
    // per-instance material override (rows of the whole job, world-major, spare rows included): write rows
    // [first, first + count) of the column from host memory -- stream-ordered, the next step renders with them; false
    // when the range is outside the renderer -- and read them back (waits for the stream)
    bool setInstanceMaterials(uint32_t first, uint32_t count, const int32_t *materials);
    void instanceMaterials(uint32_t first, uint32_t count, int32_t *out) const;
    uint32_t numInstanceRows() const;
    // per-instance labels, as the material override above: stream-ordered write of rows [first, first + count) from
    // host memory, and the read-back
    bool setInstanceLabels(uint32_t first, uint32_t count, const int32_t *labels);
    void instanceLabels(uint32_t first, uint32_t count, int32_t *out) const;

    uint32_t numAgents;

private:
    struct Impl;
    std::unique_ptr<Impl> impl_;
};

}  // namespace madRender
