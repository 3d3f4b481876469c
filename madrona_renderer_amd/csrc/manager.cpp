// madRender::Manager over the C-ABI (include/mrx.h).  Mirrors the control
// flow of the reference's Manager (/root/reference/src/mgr.cpp:505-665):
// construct -> first frame rendered; step(); tensor getters that wrap device
// pointers without copying.
#include "../../include/madrona_mi355/manager.hpp"
#include "../../include/mrx.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

namespace madRender {

namespace detail {
static bool g_throwOnError = false;
// The reference aborts on every error (FATAL / REQ_CUDA / assert:
// mgr.cpp:306,320,420,595).  Language bindings flip this so the same
// conditions surface as exceptions instead of killing the interpreter.
void setThrowOnError(bool v) { g_throwOnError = v; }

[[noreturn]] static void fatal(const char *msg)
{
    if (g_throwOnError)
        throw std::runtime_error(msg);
    std::fprintf(stderr, "FATAL: %s\n", msg);
    std::fflush(stderr);
    std::abort();
}
[[noreturn]] static void fatal(const std::string &msg) { fatal(msg.c_str()); }
}  // namespace detail

using madrona::py::Tensor;
using madrona::py::TensorElementType;

namespace {
// the status of a C-ABI call: anything but MRX_OK is fatal, with the library's text
void check(int rc)
{
    if (rc != MRX_OK)
        detail::fatal(mrx_last_error());
}

// ... of a setter whose values the caller may get wrong: MRX_E_INVALID is theirs (false, the text in mrx_last_error)
bool accepted(int rc)
{
    if (rc == MRX_E_INVALID)
        return false;
    check(rc);
    return true;
}

mrx_info_t info(mrx_renderer *r)
{
    mrx_info_t i {};
    check(mrx_info_sized(r, &i, sizeof i));
    return i;
}
}  // namespace

struct Manager::Impl {
    mrx_renderer *r = nullptr;
    ~Impl() { mrx_destroy(r); }

    Tensor wrap(int which, uint32_t shard, bool sample = false) const
    {
        int64_t dims[4] = { 0, 0, 0, 0 };
        int ndim = 0, dtype = 0, dev = 0;
        mrx_renderer *sh = sample ? mrx_shard(r, (int)shard) : nullptr;
        void *p = sample ? (sh ? mrx_sample_buffer(sh, which, dims, &ndim, &dtype, &dev) : nullptr)
                         : mrx_buffer_shard(r, (int)shard, which, dims, &ndim, &dtype, &dev);
        if (!p)
            detail::fatal(mrx_last_error());
        TensorElementType t = dtype == MRX_DTYPE_U8 ? TensorElementType::UInt8
                            : dtype == MRX_DTYPE_I32 ? TensorElementType::Int32
                            : dtype == MRX_DTYPE_F16 ? TensorElementType::Float16
                            : dtype == MRX_DTYPE_BF16 ? TensorElementType::BFloat16
                                                      : TensorElementType::Float32;
        return Tensor(p, t, dims, ndim, dev);
    }
};

Manager::Manager(const Config &cfg)
    : impl_(new Impl())
{
    static_assert(sizeof(mrx_instance) == sizeof(ImportedInstance), "instance ABI");
    static_assert(sizeof(mrx_camera) == sizeof(ImportedCamera), "camera ABI");
    static_assert(sizeof(mrx_world_init) == sizeof(Sim::WorldInit), "world ABI");
    static_assert(sizeof(mrx_material) == sizeof(AdditionalMaterial), "material ABI");

    mrx_config c {};
    c.struct_size = sizeof(mrx_config);
    c.gpu_id = cfg.gpuID;
    c.num_worlds = cfg.numWorlds;
    c.render_mode = cfg.renderMode == RenderMode::Raytracer ? MRX_MODE_RAYTRACER
                                                            : MRX_MODE_RASTERIZER;
    c.view_width = cfg.batchRenderViewWidth;
    c.view_height = cfg.batchRenderViewHeight;
    const Config::RenderConfig &rc = cfg.rcfg;
    c.geo.vertices = reinterpret_cast<const float *>(rc.geoCfg.vertices);
    c.geo.uvs = reinterpret_cast<const float *>(rc.geoCfg.uvs);
    c.geo.indices = rc.geoCfg.indices;
    c.geo.mesh_vertex_offsets = rc.geoCfg.meshVertexOffsets;
    c.geo.mesh_index_offsets = rc.geoCfg.meshIndexOffsets;
    c.geo.mesh_materials = rc.geoCfg.meshMaterials;
    c.geo.num_vertices = rc.geoCfg.numVertices;
    c.geo.num_indices = rc.geoCfg.numIndices;
    c.geo.num_meshes = rc.geoCfg.numMeshes;
    c.asset_paths = rc.assetPaths;
    c.num_asset_paths = rc.numAssetPaths;
    c.mat_assignments = rc.matAssignments;
    c.num_mat_assignments = rc.numMatAssignments;
    c.materials = reinterpret_cast<const mrx_material *>(rc.additionalMats);
    c.num_materials = rc.numAdditionalMats;
    c.texture_paths = rc.additionalTextures;
    c.num_textures = rc.numAdditionalTextures;
    c.instances = reinterpret_cast<const mrx_instance *>(rc.importedInstances);
    c.num_instances = rc.numInstances;
    c.cameras = reinterpret_cast<const mrx_camera *>(rc.cameras);
    c.num_cameras = rc.numCameras;
    c.worlds = reinterpret_cast<const mrx_world_init *>(rc.worlds);
    c.stream = nullptr;
    c.device_ids = cfg.deviceIDs;
    c.num_devices = cfg.numDevices;
    c.max_instances_per_world = cfg.maxInstancesPerWorld;
    static_assert(sizeof(mrx_projection) == sizeof(CameraProjection), "projection ABI");
    c.camera_projections = reinterpret_cast<const mrx_projection *>(cfg.cameraProjections);
    static_assert(sizeof(mrx_light) == sizeof(Light), "light ABI");
    c.world_lights = reinterpret_cast<const mrx_light *>(cfg.worldLights);
    c.instance_colors = cfg.instanceColors;
    if (cfg.instanceColorColumn)
        c.flags |= MRX_FLAG_INSTANCE_COLORS;
    if (cfg.instanceMaterialColumn || cfg.instanceMaterials)
        c.flags |= MRX_FLAG_INSTANCE_MATERIALS;
    if (cfg.normals)
        c.flags |= MRX_FLAG_NORMALS;
    if (cfg.instanceLabelColumn || cfg.instanceLabels)
        c.flags |= MRX_FLAG_INSTANCE_LABELS;
    if (cfg.supersample < 1 || cfg.supersample > 4)
        detail::fatal("supersample " + std::to_string(cfg.supersample) + " is not in 1 ... 4");
    c.flags |= MRX_FLAG_SUPERSAMPLE(cfg.supersample);
    if (cfg.positions > 2)
        detail::fatal("positions " + std::to_string(cfg.positions) + " is not 0 (none), 1 (world) or 2 (view)");
    if (cfg.positions)
        c.flags |= cfg.positions == 2 ? MRX_FLAG_POSITIONS | MRX_FLAG_POSITIONS_VIEW : MRX_FLAG_POSITIONS;
    if (cfg.boxLabels > 1024)
        detail::fatal("boxLabels " + std::to_string(cfg.boxLabels) + " is not in 0 ... 1024");
    c.flags |= MRX_FLAG_BOX_LABELS(cfg.boxLabels);
    if (cfg.observations & ~MRX_FLAG_OBS_MASK)
        detail::fatal("observations " + std::to_string(cfg.observations) + " has bits outside MRX_FLAG_OBS_MASK");
    c.flags |= cfg.observations;
    if (cfg.renderOutputs == RenderOutputs::Depth)
        c.flags |= MRX_FLAG_NO_RGB;
    else if (cfg.renderOutputs == RenderOutputs::RGB)
        c.flags |= MRX_FLAG_NO_DEPTH;
    // build-only knobs travel by environment so Config stays field-compatible
    if (const char *v = std::getenv("MADRONA_MI355_VISIBILITY"))
        if (std::atoi(v) != 0)
            c.flags |= MRX_FLAG_VISIBILITY_IDS;
    if (cfg.flow) {
        if (cfg.renderOutputs == RenderOutputs::RGB)
            detail::fatal("flow needs depth: renderOutputs RGB renders none");
        if (cfg.boxLabels)
            detail::fatal("flow and boxLabels exclude each other: under flow the ids tensor holds visibility ids");
        c.flags |= MRX_FLAG_VISIBILITY_IDS;
    }
    if (const char *k = std::getenv("MADRONA_MI355_KERNEL"))
        c.kernel_variant = std::atoi(k);

    if (cfg.raysPerWorld > 65536)
        detail::fatal("raysPerWorld " + std::to_string(cfg.raysPerWorld) + " is not in 0 ... 65536");
    check(mrx_create(&c, &impl_->r));
    // (the flag word is full: the sensor is attached to the renderer once it exists)
    if (cfg.raysPerWorld)
        check(mrx_rays_create(impl_->r, cfg.raysPerWorld));
    if (cfg.flow)
        check(mrx_flow_create(impl_->r));
    // the initial values of an int32 column, world-major as mrx_create lays the rows out (spare rows `spare`)
    const auto expand = [&](const int32_t *perInstance, int32_t spare) {
        std::vector<int32_t> rows;
        for (uint32_t w = 0; w < cfg.numWorlds; ++w) {
            const Sim::WorldInit &wi = rc.worlds[w];
            const uint32_t n = std::max(wi.numInstances, cfg.maxInstancesPerWorld);
            for (uint32_t i = 0; i < n; ++i)
                rows.push_back(i < wi.numInstances ? perInstance[wi.instancesOffset + i] : spare);
        }
        return rows;
    };
    if (cfg.instanceMaterials) {
        const std::vector<int32_t> ids = expand(cfg.instanceMaterials, -1);
        if (!ids.empty())
            check(mrx_set_instance_materials(impl_->r, 0, (uint32_t)ids.size(), ids.data()));
    }
    if (cfg.instanceLabels) {
        const std::vector<int32_t> labels = expand(cfg.instanceLabels, MRX_LABEL_OBJECT);
        if (!labels.empty())
            check(mrx_set_instance_labels(impl_->r, 0, (uint32_t)labels.size(), labels.data()));
    }
    // ... then the first frame again: what a caller reads before its first step() already shows them
    if (cfg.instanceMaterials || cfg.instanceLabels)
        check(mrx_render(impl_->r));

    // vestigial in the reference too (mgr.cpp:516-522)
    const char *num_agents_str = std::getenv("HIDESEEK_NUM_AGENTS");
    numAgents = num_agents_str ? (uint32_t)std::atoi(num_agents_str) : 1u;
    // mrx_create already rendered the first frame (mgr.cpp:524)
}

Manager::~Manager() {}

void Manager::step() { check(mrx_step(impl_->r)); }
void Manager::render() { check(mrx_render(impl_->r)); }
void Manager::sync() { check(mrx_sync(impl_->r)); }

Tensor Manager::rgbTensor(uint32_t shard) const { return impl_->wrap(MRX_BUF_RGB, shard); }
Tensor Manager::depthTensor(uint32_t shard) const { return impl_->wrap(MRX_BUF_DEPTH, shard); }
Tensor Manager::segmaskTensor(uint32_t shard) const { return impl_->wrap(MRX_BUF_SEGMASK, shard); }
Tensor Manager::visibilityTensor(uint32_t shard) const { return impl_->wrap(MRX_BUF_VISIBILITY, shard); }
Tensor Manager::normalTensor(uint32_t shard) const { return impl_->wrap(MRX_BUF_NORMAL, shard); }

Tensor Manager::instanceObjectTensor(uint32_t shard) const { return impl_->wrap(MRX_BUF_INSTANCE_OBJECT, shard); }
Tensor Manager::instanceScaleTensor(uint32_t shard) const { return impl_->wrap(MRX_BUF_INSTANCE_SCALE, shard); }
Tensor Manager::instanceColorTensor(uint32_t shard) const { return impl_->wrap(MRX_BUF_INSTANCE_COLOR, shard); }
Tensor Manager::instanceMaterialTensor(uint32_t shard) const { return impl_->wrap(MRX_BUF_INSTANCE_MATERIAL, shard); }
Tensor Manager::instanceLabelTensor(uint32_t shard) const { return impl_->wrap(MRX_BUF_INSTANCE_LABEL, shard); }
Tensor Manager::instancePositionTensor(uint32_t shard) const { return impl_->wrap(MRX_BUF_INSTANCE_POSITION, shard); }
Tensor Manager::instanceRotationTensor(uint32_t shard) const { return impl_->wrap(MRX_BUF_INSTANCE_ROTATION, shard); }
Tensor Manager::cameraPositionTensor(uint32_t shard) const { return impl_->wrap(MRX_BUF_CAMERA_POSITION, shard); }
Tensor Manager::cameraRotationTensor(uint32_t shard) const { return impl_->wrap(MRX_BUF_CAMERA_ROTATION, shard); }

uint64_t Manager::rgbCudaPtr(uint32_t shard) const { return (uint64_t)rgbTensor(shard).devicePtr(); }
uint64_t Manager::depthCudaPtr(uint32_t shard) const { return (uint64_t)depthTensor(shard).devicePtr(); }
uint64_t Manager::segmaskCudaPtr(uint32_t shard) const { return (uint64_t)segmaskTensor(shard).devicePtr(); }

// the post-render stages: the option the renderer was created with, the stage's tensors, the stage alone
uint32_t Manager::supersample() const { return (uint32_t)mrx_supersample(impl_->r); }
Tensor Manager::sampleTensor(int which, uint32_t shard) const { return impl_->wrap(which, shard, true); }
void Manager::resolve() { check(mrx_resolve(impl_->r)); }

uint32_t Manager::positions() const { return (uint32_t)mrx_positions(impl_->r); }
Tensor Manager::positionTensor(uint32_t shard) const { return impl_->wrap(MRX_BUF_POSITION, shard); }
void Manager::unproject() { check(mrx_unproject(impl_->r)); }

uint32_t Manager::boxLabels() const { return (uint32_t)mrx_box_labels(impl_->r); }
Tensor Manager::boxTensor(uint32_t shard) const { return impl_->wrap(MRX_BUF_BOXES, shard); }
void Manager::boxes() { check(mrx_boxes(impl_->r)); }

uint32_t Manager::observations() const { return (uint32_t)mrx_observations(impl_->r); }
Tensor Manager::observationTensor(uint32_t shard) const { return impl_->wrap(MRX_BUF_OBSERVATION, shard); }
Tensor Manager::observationResetTensor(uint32_t shard) const { return impl_->wrap(MRX_BUF_OBSERVATION_RESET, shard); }
void Manager::observe() { check(mrx_observe(impl_->r)); }
void Manager::setObservationDepthRange(float lo, float hi) { check(mrx_set_observation_depth_range(impl_->r, lo, hi)); }
void Manager::observationDepthRange(float *lo, float *hi) const { check(mrx_observation_depth_range(impl_->r, lo, hi)); }

uint32_t Manager::rays() const { return (uint32_t)mrx_rays(impl_->r); }
Tensor Manager::rayTensor(uint32_t shard) const { return impl_->wrap(MRX_BUF_RAYS, shard); }
Tensor Manager::rayFrameTensor(uint32_t shard) const { return impl_->wrap(MRX_BUF_RAY_FRAME, shard); }
Tensor Manager::rayDistanceTensor(uint32_t shard) const { return impl_->wrap(MRX_BUF_RAY_DISTANCE, shard); }
Tensor Manager::rayIdTensor(uint32_t shard) const { return impl_->wrap(MRX_BUF_RAY_ID, shard); }
void Manager::trace() { check(mrx_trace(impl_->r)); }

bool Manager::flows() const { return mrx_flow_enabled(impl_->r) == 1; }
Tensor Manager::flowTensor(uint32_t shard) const { return impl_->wrap(MRX_BUF_FLOW, shard); }
void Manager::flow() { check(mrx_flow(impl_->r)); }
void Manager::flowSnapshot() { check(mrx_flow_snapshot(impl_->r)); }

void Manager::refreshObjects() { check(mrx_refresh_objects(impl_->r)); }

uint32_t Manager::numShards() const { return (uint32_t)mrx_num_shards(impl_->r); }

uint32_t Manager::shardFirstWorld(uint32_t shard) const
{
    const int64_t w = mrx_shard_first_world(impl_->r, (int)shard);
    if (w < 0)
        detail::fatal(mrx_last_error());
    return (uint32_t)w;
}

float Manager::timeRenders(int steps)
{
    float ms = 0.f;
    check(mrx_time_renders(impl_->r, steps, &ms));
    return ms;
}

double Manager::timeStepsHost(int steps)
{
    double us = 0.0;
    check(mrx_time_steps_host(impl_->r, steps, &us));
    return us;
}

void Manager::mark(int which) { check(mrx_mark(impl_->r, which)); }

float Manager::elapsedMs()
{
    float ms = 0.f;
    check(mrx_elapsed_ms(impl_->r, &ms));
    return ms;
}

uint32_t Manager::numViews() const { return info(impl_->r).num_views; }
uint32_t Manager::numWorlds() const { return info(impl_->r).num_worlds; }
uint32_t Manager::numInstanceRows() const { return info(impl_->r).num_instances; }
uint64_t Manager::bytesPerStep() const { return info(impl_->r).bytes_per_step; }
const char *Manager::renderPath() const { return info(impl_->r).render_path == 1 ? "bvh" : "raster"; }

void *Manager::nativeHandle() const { return impl_->r; }

bool Manager::setViewProjection(uint32_t first, uint32_t count, const CameraProjection *proj)
{
    return accepted(mrx_set_view_projection(impl_->r, first, count, reinterpret_cast<const mrx_projection *>(proj)));
}

void Manager::viewProjection(uint32_t first, uint32_t count, CameraProjection *out) const
{
    check(mrx_view_projection(impl_->r, first, count, reinterpret_cast<mrx_projection *>(out)));
}

bool Manager::setWorldLights(uint32_t first, uint32_t count, const Light *lights)
{
    return accepted(mrx_set_world_light(impl_->r, first, count, reinterpret_cast<const mrx_light *>(lights)));
}

void Manager::worldLights(uint32_t first, uint32_t count, Light *out) const
{
    check(mrx_world_light(impl_->r, first, count, reinterpret_cast<mrx_light *>(out)));
}

bool Manager::setInstanceMaterials(uint32_t first, uint32_t count, const int32_t *materials)
{
    return accepted(mrx_set_instance_materials(impl_->r, first, count, materials));
}

void Manager::instanceMaterials(uint32_t first, uint32_t count, int32_t *out) const
{
    check(mrx_instance_materials(impl_->r, first, count, out));
}

bool Manager::setInstanceLabels(uint32_t first, uint32_t count, const int32_t *labels)
{
    return accepted(mrx_set_instance_labels(impl_->r, first, count, labels));
}

void Manager::instanceLabels(uint32_t first, uint32_t count, int32_t *out) const
{
    check(mrx_instance_labels(impl_->r, first, count, out));
}

int Manager::placement(float *candUs, int capacity, float *keptUs) const
{
    return mrx_placement(impl_->r, candUs, capacity, keptUs);
}

const char *Manager::rasterEntry() const
{
    static const char *const names[] = {"none", "group-fast", "group", "chunked", "brute", "bvh"};
    const int e = mrx_raster_entry(impl_->r);
    if (e < 0 || e >= (int)(sizeof names / sizeof names[0]))
        detail::fatal(mrx_last_error());
    return names[e];
}

Manager::KernelFormInfo Manager::kernelForm() const
{
    static const char *const names[] = {"Uniform", "PV", "PVL", "C", "PVLC", "M", "PVLM", "N", "NPV", "L", "LN", "PVM"};
    mrx_kernel_form_t f {};
    check(mrx_kernel_form(impl_->r, &f));
    if (f.form < 0 || f.form >= (int)(sizeof names / sizeof names[0]))
        detail::fatal("mrx_kernel_form: unknown form");
    return KernelFormInfo { names[f.form], f.slots };
}

void Manager::setStream(void *hipStream) { check(mrx_set_stream(impl_->r, hipStream)); }

void Manager::setShardStream(uint32_t shard, void *hipStream)
{
    mrx_renderer *sh = mrx_shard(impl_->r, (int)shard);
    if (!sh)
        detail::fatal(mrx_last_error());
    check(mrx_set_stream(sh, hipStream));
}

}  // namespace madRender
