// Python module `madrona_renderer` (pybind11): the same classes, keyword
// arguments and methods as the reference's nanobind module
// (/root/reference/src/bindings.cpp:18-236), bound to the MI355X Manager.
// Tensors are exported through DLPack (device type ROCm), so
// `tensor.to_torch()` aliases the renderer's HBM buffers without a copy.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <array>
#include <cmath>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "../../include/madrona_mi355/manager.hpp"
#include "../../include/mrx.h"
#include "obs_names.hpp"

namespace py = pybind11;

namespace madRender {
namespace detail { void setThrowOnError(bool v); }
}

namespace {

using namespace madRender;

namespace {
// a camera as the binding takes it: the reference's ImportedCamera (28 bytes, unchanged) and its projection
struct PyCamera {
    ImportedCamera cam;
    Manager::CameraProjection proj;
};

// the mode-independent half of the projection check (mrx_projection_constants has the rest): ValueError
void checkProjection(const Manager::CameraProjection &q)
{
    if (!(std::isfinite(q.vfovDeg) && q.vfovDeg > 0.0f && q.vfovDeg < 180.0f))
        throw py::value_error("vfov must be finite and in (0, 180) degrees");
    if (!(std::isfinite(q.znear) && q.znear >= 0.0f))
        throw py::value_error("znear must be finite and > 0 (None: the mode's default)");
}
// the light check of the library (mrx_light_constants): ValueError
void checkLight(const Manager::Light &l)
{
    float c[5];
    const mrx_light in = { { l.direction[0], l.direction[1], l.direction[2] }, l.ambient, l.diffuse };
    if (mrx_light_constants(in, c) != MRX_OK)
        throw py::value_error(mrx_last_error());
}
// a znear the caller gave (not None): finite and > 0
float znearOf(float z)
{
    if (!(std::isfinite(z) && z > 0.0f))
        throw py::value_error("znear must be finite and > 0 (None: the mode's default)");
    return z;
}
}  // namespace
using madrona::py::Tensor;
using madrona::py::TensorElementType;

// ---- minimal DLPack (v0.8 ABI) ------------------------------------------
enum { kDLCPU = 1, kDLROCM = 10 };
enum { kDLInt = 0, kDLUInt = 1, kDLFloat = 2, kDLBfloat = 4 };
struct DLDevice { int32_t device_type; int32_t device_id; };
struct DLDataType { uint8_t code; uint8_t bits; uint16_t lanes; };
struct DLTensor {
    void *data;
    DLDevice device;
    int32_t ndim;
    DLDataType dtype;
    int64_t *shape;
    int64_t *strides;
    uint64_t byte_offset;
};
struct DLManagedTensor {
    DLTensor dl_tensor;
    void *manager_ctx;
    void (*deleter)(DLManagedTensor *);
};

struct DLHolder {
    DLManagedTensor managed;
    int64_t shape[4];
    PyObject *owner;   // keeps the renderer alive while torch holds the view
};

void dlDeleter(DLManagedTensor *m)
{
    DLHolder *h = static_cast<DLHolder *>(m->manager_ctx);
    if (h->owner && Py_IsInitialized()) {
        py::gil_scoped_acquire gil;
        Py_DECREF(h->owner);
    }
    delete h;
}

void capsuleDestructor(PyObject *cap)
{
    // consumed capsules are renamed "used_dltensor" and own nothing
    if (PyCapsule_IsValid(cap, "dltensor")) {
        auto *m = static_cast<DLManagedTensor *>(PyCapsule_GetPointer(cap, "dltensor"));
        if (m && m->deleter)
            m->deleter(m);
    }
}

// Python-side tensor handle: the view plus a reference to its renderer.
struct PyTensor {
    Tensor t;
    py::object owner;
};

py::object makeCapsule(const PyTensor &self)
{
    auto *h = new DLHolder();
    const Tensor &t = self.t;
    DLTensor &d = h->managed.dl_tensor;
    d.data = t.devicePtr();
    d.device = DLDevice { kDLROCM, t.gpuID() };
    d.ndim = (int32_t)t.numDims();
    switch (t.type()) {
    case TensorElementType::UInt8: d.dtype = DLDataType { kDLUInt, 8, 1 }; break;
    case TensorElementType::Int32: d.dtype = DLDataType { kDLInt, 32, 1 }; break;
    case TensorElementType::Float16: d.dtype = DLDataType { kDLFloat, 16, 1 }; break;
    case TensorElementType::BFloat16: d.dtype = DLDataType { kDLBfloat, 16, 1 }; break;
    default: d.dtype = DLDataType { kDLFloat, 32, 1 }; break;
    }
    for (int i = 0; i < d.ndim; ++i)
        h->shape[i] = t.dims()[i];
    d.shape = h->shape;
    d.strides = nullptr;
    d.byte_offset = 0;
    h->managed.manager_ctx = h;
    h->managed.deleter = dlDeleter;
    h->owner = self.owner.ptr();
    Py_XINCREF(h->owner);
    PyObject *cap = PyCapsule_New(&h->managed, "dltensor", capsuleDestructor);
    if (!cap) {
        dlDeleter(&h->managed);
        throw py::error_already_set();
    }
    return py::reinterpret_steal<py::object>(cap);
}

// a NumPy argument as a dense array of T, converted where it is not one
template <typename T>
using CArray = py::array_t<T, py::array::c_style | py::array::forcecast>;

PyTensor wrapTensor(py::object self, Tensor t) { return PyTensor { t, std::move(self) }; }

// `shard` of the tensor getters: None means "the renderer's one shard" -- an error when the
// renderer spans several devices (each shard's tensors live on its own device)
uint32_t shardOf(const py::object &self, const py::object &shard)
{
    const uint32_t n = self.cast<Manager &>().numShards();
    if (shard.is_none()) {
        if (n > 1)
            throw py::value_error("this renderer spans " + std::to_string(n) +
                                  " devices: say which shard's tensor (shard=i)");
        return 0;
    }
    const long i = shard.cast<long>();
    if (i < 0 || (unsigned long)i >= n)
        throw py::index_error("shard " + std::to_string(i) + " of " + std::to_string(n));
    return (uint32_t)i;
}

// observations= of the constructor: None / False (no output), a string -- the channels, float32, no stack -- or a dict
// with the keys channels (required), dtype, stack and depth_range
struct ObsArg {
    uint32_t field = 0;             // MRX_FLAG_OBSERVATIONS(...), 0: no output
    bool hasRange = false;
    float lo = 0.0f, hi = 0.0f;
};

// (lo, hi) with 0 <= lo < hi, both finite, as float32
void parseObsRange(const py::object &range, float &lo, float &hi)
{
    const char *msg = "observations: depth_range must be None or (lo, hi) with 0 <= lo < hi, both finite";
    if (!py::isinstance<py::tuple>(range) && !py::isinstance<py::list>(range))
        throw py::value_error(msg);
    const py::sequence seq = range.cast<py::sequence>();
    if (seq.size() != 2)
        throw py::value_error(msg);
    double v[2];
    for (int i = 0; i < 2; ++i) {
        const py::object o = seq[i];
        if (py::isinstance<py::bool_>(o) || (!py::isinstance<py::float_>(o) && !py::isinstance<py::int_>(o)))
            throw py::value_error(msg);
        v[i] = o.cast<double>();
    }
    lo = (float)v[0];
    hi = (float)v[1];
    if (!(std::isfinite(lo) && std::isfinite(hi) && lo >= 0.0f && lo < hi))
        throw py::value_error(msg);
}

ObsArg parseObservations(const py::object &arg, Manager::RenderOutputs outputs)
{
    ObsArg out;
    if (arg.is_none() || (py::isinstance<py::bool_>(arg) && !arg.cast<bool>()))
        return out;
    std::string channels, dtype = "float32";
    long long stack = 1;
    py::object range = py::none();
    if (py::isinstance<py::str>(arg)) {
        channels = arg.cast<std::string>();
    } else if (py::isinstance<py::dict>(arg)) {
        bool haveChannels = false;
        for (const auto &kv : arg.cast<py::dict>()) {
            if (!py::isinstance<py::str>(kv.first))
                throw py::value_error("observations: the keys are channels, dtype, stack and depth_range");
            const std::string key = kv.first.cast<std::string>();
            const py::object val = py::reinterpret_borrow<py::object>(kv.second);
            if (key == "channels" || key == "dtype") {
                if (!py::isinstance<py::str>(val))
                    throw py::value_error("observations: " + key + " must be a string");
                (key == "channels" ? channels : dtype) = val.cast<std::string>();
                haveChannels = haveChannels || key == "channels";
            } else if (key == "stack") {
                if (py::isinstance<py::bool_>(val) || !py::isinstance<py::int_>(val))
                    throw py::value_error("observations: stack must be an int in 1 ... 8");
                stack = val.cast<long long>();
            } else if (key == "depth_range") {
                range = val;
            } else {
                throw py::value_error("observations: unknown key " + key + " (channels, dtype, stack, depth_range)");
            }
        }
        if (!haveChannels)
            throw py::value_error("observations: the dict needs channels (rgb, rgbd, d, y, yd)");
    } else {
        throw py::value_error("observations must be None, a channels string or a dict (channels, dtype, stack, depth_range)");
    }
    const uint32_t layout = obsLayoutOf(channels), dt = obsDtypeOf(dtype);
    if (!layout)
        throw py::value_error("observations: unknown channels " + channels + " (rgb, rgbd, d, y, yd)");
    if (dt == kNumObsDtypes)
        throw py::value_error("observations: unknown dtype " + dtype + " (float32, float16, bfloat16, uint8)");
    if (stack < 1 || stack > 8)
        throw py::value_error("observations: stack must be an int in 1 ... 8");
    const bool colour = layout != MRX_OBS_D, depth = layout == MRX_OBS_RGBD || layout == MRX_OBS_D || layout == MRX_OBS_YD;
    if (colour && outputs == Manager::RenderOutputs::Depth)
        throw py::value_error("observations: channels " + channels + " need rgb: render_outputs Depth renders none");
    if (depth && outputs == Manager::RenderOutputs::RGB)
        throw py::value_error("observations: channels " + channels + " need depth: render_outputs RGB renders none");
    if (!range.is_none()) {
        parseObsRange(range, out.lo, out.hi);
        if (!depth)
            throw py::value_error("observations: depth_range with channels " + channels + ", which have no depth");
        out.hasRange = true;
    }
    out.field = MRX_FLAG_OBSERVATIONS(layout, dt, (uint32_t)stack);
    return out;
}

// a count the constructor takes as None (0) or an int in 1 ... hi; with `orZero`, 0 and False stand for None too.
// Anything else, True included, is refused with `msg`.
uint32_t countOrNone(const py::object &arg, long long hi, bool orZero, const char *msg)
{
    if (arg.is_none() || (orZero && py::isinstance<py::bool_>(arg) && !arg.cast<bool>()))
        return 0;
    if (py::isinstance<py::bool_>(arg) || !py::isinstance<py::int_>(arg))
        throw py::value_error(msg);
    const long long n = arg.cast<long long>();   // (an int beyond long long: pybind's cast error)
    if (n < (orZero ? 0 : 1) || n > hi)
        throw py::value_error(msg);
    return (uint32_t)n;
}

// a per-instance column the constructor takes as None (no column), a bool (True: a column of the default value) or an
// array of `rows` rows -- of `cols` entries each, one-dimensional where cols is 0; anything else is refused with `msg`.
// Sets the Config's switch and pointer; the array returned backs the pointer.
template <typename T>
CArray<T> parseColumn(const py::object &arg, size_t rows, py::ssize_t cols, const char *msg, bool &column, const T *&data)
{
    CArray<T> a;
    if (py::isinstance<py::bool_>(arg)) {
        column = arg.cast<bool>();
    } else if (!arg.is_none()) {
        a = CArray<T>::ensure(arg);
        if (!a || a.ndim() != (cols ? 2 : 1) || (size_t)a.shape(0) != rows || (cols && a.shape(1) != cols))
            throw py::value_error(msg);
        data = a.data();
        column = true;
    }
    return a;
}

// a scalar or a sequence of floats, for set_camera_projection and set_world_light, which broadcast a scalar
std::vector<float> asVec(const py::object &o, bool &scalar)
{
    scalar = !py::isinstance<py::sequence>(o) && !py::hasattr(o, "__len__");
    if (scalar)
        return { o.cast<float>() };
    return CArray<float>(o).cast<std::vector<float>>();
}

// set_instance_labels / set_instance_materials and instance_labels / instance_materials: an int32 column from and to
// host memory through its Manager accessor.  `none` is the column's "no value" (what a call of no rows points at);
// `array` and `values` are the nouns of the two refusals.
void setRows(Manager &self, bool (Manager::*set)(uint32_t, uint32_t, const int32_t *), int32_t none, const std::string &array,
             const std::string &values, const CArray<int32_t> &ids, int64_t first_row)
{
    if (ids.ndim() != 1)
        throw py::value_error(array + " must be a one-dimensional int32 array");
    if (first_row < 0 || first_row + (int64_t)ids.shape(0) > (int64_t)self.numInstanceRows())
        throw py::value_error("more " + values + " than instance rows from first_row on");
    if (!(self.*set)((uint32_t)first_row, (uint32_t)ids.shape(0), ids.shape(0) ? ids.data() : &none))
        throw py::value_error(mrx_last_error());
}

py::array_t<int32_t> getRows(Manager &self, void (Manager::*get)(uint32_t, uint32_t, int32_t *) const, int32_t none)
{
    const uint32_t n = self.numInstanceRows();
    py::array_t<int32_t> out(n);
    (self.*get)(0, n, n ? out.mutable_data() : &none);
    return out;
}

// ---- the constructor, in steps: parse the options, check the scene, fill the Config, construct ----------------------
struct Options {
    ObsArg obs;
    uint32_t raysPerWorld = 0, boxLabels = 0, positionFrame = 0;
};

// step 1: the keyword options that are no plain value, and the combinations that exclude each other
Options parseOptions(Manager::RenderOutputs outputs, int supersample, const py::object &positions, const py::object &boxes,
                     const py::object &observations, const py::object &rays, bool flow)
{
    Options o;
    o.obs = parseObservations(observations, outputs);
    // rays: None (no sensor) or R, an int in 1 ... 65536
    o.raysPerWorld = countOrNone(rays, 65536, false, "rays must be None or an int in 1 ... 65536 (the number of rays per world)");
    // boxes: None / 0 / False (no output) or K, an int in 1 ... 1024
    o.boxLabels = countOrNone(boxes, 1024, true, "boxes must be None or an int in 1 ... 1024 (the number of labels)");
    if (supersample < 1 || supersample > 4)
        throw py::value_error("supersample must be 1, 2, 3 or 4");
    if (flow && outputs == Manager::RenderOutputs::RGB)
        throw py::value_error("flow needs depth: render_outputs RGB renders none");
    if (flow && o.boxLabels)
        throw py::value_error("flow and boxes exclude each other: under flow the ids tensor holds visibility "
                              "ids, the box stage needs a segmask");
    // positions: False / None (no output), True or "world", or "view"
    if (py::isinstance<py::bool_>(positions))
        o.positionFrame = positions.cast<bool>() ? 1u : 0u;
    else if (py::isinstance<py::str>(positions) && positions.cast<std::string>() == "world")
        o.positionFrame = 1;
    else if (py::isinstance<py::str>(positions) && positions.cast<std::string>() == "view")
        o.positionFrame = 2;
    else if (!positions.is_none())
        throw py::value_error("positions must be False, True, \"world\" or \"view\"");
    if (o.positionFrame && outputs == Manager::RenderOutputs::RGB)
        throw py::value_error("positions need depth: render_outputs RGB renders none");
    return o;
}

// step 2: the shapes of the scene's arrays -- the C ABI carries no lengths for the per-mesh arrays and reads uvs
// row-for-row with vertices -- and the cameras against the mode
void checkScene(size_t num_worlds, size_t worlds, Manager::RenderMode mode, const std::vector<PyCamera> &cameras,
                const CArray<float> &vertices, const CArray<float> &uvs, const CArray<uint32_t> &vertexOffsets,
                const CArray<uint32_t> &indexOffsets, const CArray<int32_t> &materials)
{
    if (vertices.size() && (vertices.ndim() != 2 || vertices.shape(1) != 3))
        throw py::value_error("mesh_vertices must have shape [N, 3]");
    if (uvs.size() && (uvs.ndim() != 2 || uvs.shape(1) != 2))
        throw py::value_error("mesh_uvs must have shape [N, 2]");
    if (num_worlds != worlds)
        throw py::value_error("num_worlds does not match len(worlds)");
    if (indexOffsets.size() != vertexOffsets.size() || materials.size() != vertexOffsets.size())
        throw py::value_error("mesh_vertex_offsets, mesh_indices_offsets and "
                              "mesh_materials must have one entry per mesh");
    if ((uvs.size() ? uvs.shape(0) : 0) != (vertices.size() ? vertices.shape(0) : 0))
        throw py::value_error("mesh_uvs must have one row per row of mesh_vertices");
    if (mode == Manager::RenderMode::Raytracer)
        for (const PyCamera &c : cameras)
            if (!(c.proj.znear < 1000.0f))
                throw py::value_error("znear must be below the Raytracer far plane (1000)");
}

// world_lights: [(direction, ambient, diffuse)] per world
std::vector<Manager::Light> parseLights(const py::object &world_lights, int num_worlds)
{
    std::vector<Manager::Light> lights;
    const py::sequence seq = world_lights.cast<py::sequence>();
    if ((int64_t)py::len(seq) != num_worlds)
        throw py::value_error("world_lights needs one (direction, ambient, diffuse) per world");
    for (const py::handle &h : seq) {
        const py::tuple t = py::tuple(py::reinterpret_borrow<py::object>(h));
        if (t.size() != 3)
            throw py::value_error("world_lights entries are (direction, ambient, diffuse)");
        const std::array<float, 3> d = t[0].cast<std::array<float, 3>>();
        const Manager::Light l = { { d[0], d[1], d[2] }, t[1].cast<float>(), t[2].cast<float>() };
        checkLight(l);
        lights.push_back(l);
    }
    return lights;
}

// what a Config points at beside the caller's own arrays: alive until the Manager is constructed
struct ConfigStore {
    std::vector<ImportedCamera> cameras;
    std::vector<Manager::CameraProjection> projections;
    std::vector<const char *> assetPaths, texturePaths;
    std::vector<int32_t> matAssignments;
    std::vector<Manager::Light> lights;
    CArray<uint8_t> colors;
    CArray<int32_t> materials, labels;
};

}  // namespace

PYBIND11_MODULE(madrona_renderer, m)
{
    m.doc() = "MI355X-native batch renderer with the madrona_renderer API";
    madRender::detail::setThrowOnError(true);
    // the C ABI's names of the colour override column (include/mrx.h), as the library was built with them
#define MRX_ATTR(name) m.attr(#name) = py::int_((long long)(name))
    MRX_ATTR(MRX_FLAG_INSTANCE_COLORS); MRX_ATTR(MRX_BUF_INSTANCE_COLOR); MRX_ATTR(MRX_NUM_BUFFERS);
    // ... and of the material override column
    MRX_ATTR(MRX_FLAG_INSTANCE_MATERIALS); MRX_ATTR(MRX_BUF_INSTANCE_MATERIAL); MRX_ATTR(MRX_NUM_BUFFERS_EXT);
    // ... and of the surface-normal output
    MRX_ATTR(MRX_FLAG_NORMALS); MRX_ATTR(MRX_BUF_NORMAL); MRX_ATTR(MRX_NUM_BUFFERS_EXT2);
    // ... and of the label column
    MRX_ATTR(MRX_FLAG_INSTANCE_LABELS); MRX_ATTR(MRX_BUF_INSTANCE_LABEL); MRX_ATTR(MRX_NUM_BUFFERS_EXT3);
    MRX_ATTR(MRX_LABEL_OBJECT);
    // ... and of the supersampling factor
    MRX_ATTR(MRX_FLAG_SUPERSAMPLE_SHIFT); MRX_ATTR(MRX_FLAG_SUPERSAMPLE_MASK);
    // ... and of the position output
    MRX_ATTR(MRX_FLAG_POSITIONS); MRX_ATTR(MRX_FLAG_POSITIONS_VIEW); MRX_ATTR(MRX_BUF_POSITION); MRX_ATTR(MRX_NUM_BUFFERS_EXT4);
    // ... and of the box labels
    MRX_ATTR(MRX_FLAG_BOX_LABELS_SHIFT); MRX_ATTR(MRX_FLAG_BOX_LABELS_MASK); MRX_ATTR(MRX_BUF_BOXES); MRX_ATTR(MRX_NUM_BUFFERS_EXT5);
    // ... and of the packed observation output
    MRX_ATTR(MRX_FLAG_OBS_SHIFT); MRX_ATTR(MRX_FLAG_OBS_MASK); MRX_ATTR(MRX_FLAG_OBS_LAYOUT_MASK);
    MRX_ATTR(MRX_FLAG_OBS_DTYPE_MASK); MRX_ATTR(MRX_FLAG_OBS_STACK_MASK);
    m.def("MRX_FLAG_OBSERVATIONS", [](uint32_t layout, uint32_t dtype, uint32_t stack) {
        return (uint32_t)MRX_FLAG_OBSERVATIONS(layout, dtype, stack);
    });
    MRX_ATTR(MRX_BUF_OBSERVATION); MRX_ATTR(MRX_BUF_OBSERVATION_RESET); MRX_ATTR(MRX_NUM_BUFFERS_EXT6);
    // ... and of the ray-cast sensor
    MRX_ATTR(MRX_BUF_RAYS); MRX_ATTR(MRX_BUF_RAY_FRAME); MRX_ATTR(MRX_BUF_RAY_DISTANCE); MRX_ATTR(MRX_BUF_RAY_ID);
    MRX_ATTR(MRX_NUM_BUFFERS_EXT7);
    // ... and of the optical-flow output
    MRX_ATTR(MRX_BUF_FLOW); MRX_ATTR(MRX_NUM_BUFFERS_EXT8);
    MRX_ATTR(MRX_DTYPE_F16); MRX_ATTR(MRX_DTYPE_BF16); MRX_ATTR(MRX_CONFIG_V4_LIGHT_SIZE);
#undef MRX_ATTR
    m.attr("MRX_CONFIG_SIZE") = (uint32_t)sizeof(mrx_config);

    py::enum_<Manager::RenderMode>(m, "RenderMode")
        .value("Rasterizer", Manager::RenderMode::Rasterizer)
        .value("Raytracer", Manager::RenderMode::Raytracer);
    // which outputs a step renders (not in the reference): rgb_tensor() / depth_tensor() of an
    // output that is not rendered raise RuntimeError
    py::enum_<Manager::RenderOutputs>(m, "RenderOutputs")
        .value("RGBD", Manager::RenderOutputs::RGBD)
        .value("Depth", Manager::RenderOutputs::Depth)
        .value("RGB", Manager::RenderOutputs::RGB);

    py::class_<ImportedAsset>(m, "ImportedAsset")
        .def(py::init([](std::string path, int64_t mat_id) {
                 return ImportedAsset { std::move(path), (int32_t)mat_id };
             }),
             py::arg("path"), py::arg("mat_id"));

    py::class_<AdditionalMaterial>(m, "AdditionalMaterial")
        .def(py::init([](const std::array<float, 4> &color, int64_t texture_id,
                         float roughness, float metalness) {
                 AdditionalMaterial mat {};
                 mat.color = { color[0], color[1], color[2], color[3] };
                 mat.textureIdx = (int32_t)texture_id;
                 mat.roughness = roughness;
                 mat.metalness = metalness;
                 return mat;
             }),
             py::arg("color"), py::arg("texture_id"), py::arg("roughness"),
             py::arg("metalness"));

    py::class_<ImportedInstance>(m, "ImportedInstance")
        .def(py::init([](const std::array<float, 3> &pos, const std::array<float, 4> &rot,
                         const std::array<float, 3> &scale, int64_t object_id) {
                 ImportedInstance i {};
                 i.position = { pos[0], pos[1], pos[2] };
                 i.rotation = { rot[0], rot[1], rot[2], rot[3] };
                 i.scale = { scale[0], scale[1], scale[2] };
                 i.objectID = (int32_t)object_id;
                 return i;
             }),
             py::arg("position"), py::arg("rotation"), py::arg("scale"),
             py::arg("object_id"));

    // (the binding's camera carries the projection beside the 28-byte ImportedCamera; znear None = the mode's default)
    py::class_<PyCamera>(m, "ImportedCamera")
        .def(py::init([](const std::array<float, 3> &pos, const std::array<float, 4> &rot, float vfov, py::object znear) {
                 PyCamera c {};
                 c.cam.position = { pos[0], pos[1], pos[2] };
                 c.cam.rotation = { rot[0], rot[1], rot[2], rot[3] };
                 c.proj.vfovDeg = vfov;
                 c.proj.znear = znear.is_none() ? 0.0f : znearOf(znear.cast<float>());
                 checkProjection(c.proj);
                 return c;
             }),
             py::arg("position"), py::arg("rotation"), py::arg("vfov") = 90.0f, py::arg("znear") = py::none())
        .def_property_readonly("vfov", [](const PyCamera &c) { return c.proj.vfovDeg; })
        .def_property_readonly("znear", [](const PyCamera &c) -> py::object {
            return c.proj.znear == 0.0f ? py::none() : py::cast(c.proj.znear); });

    py::class_<Sim::WorldInit>(m, "WorldInit")
        .def(py::init([](int64_t num_instances, int64_t instance_offset, int64_t num_cameras,
                         int64_t camera_offset) {
                 return Sim::WorldInit { (uint32_t)num_instances, (uint32_t)instance_offset,
                                         (uint32_t)num_cameras, (uint32_t)camera_offset };
             }),
             py::arg("num_instances"), py::arg("instance_offset"), py::arg("num_cameras"),
             py::arg("camera_offset"));

    m.def("inspect", [](py::array_t<uint32_t, py::array::c_style> a) {
        std::printf("Array data pointer : %p\n", (const void *)a.data());
        std::printf("Array dimension : %zu\n", (size_t)a.ndim());
        for (py::ssize_t i = 0; i < a.ndim(); ++i) {
            std::printf("Array dimension [%zu] : %zu\n", (size_t)i, (size_t)a.shape(i));
            std::printf("Array stride    [%zu] : %zd\n", (size_t)i,
                        (ssize_t)(a.strides(i) / (py::ssize_t)sizeof(uint32_t)));
        }
        std::printf("Device ID = 0 (cpu=1, cuda=0)\n");
        std::printf("Array dtype: int16=0, uint32=1, float32=0\n");
    });

    py::class_<PyTensor>(m, "Tensor")
        .def("__dlpack__",
             [](const PyTensor &self, py::kwargs) { return makeCapsule(self); })
        .def("__dlpack_device__",
             [](const PyTensor &self) { return py::make_tuple((int)kDLROCM, self.t.gpuID()); })
        .def("to_torch",
             [](py::object self) {
                 py::object torch = py::module_::import("torch");
                 return torch.attr("from_dlpack")(self);
             })
        .def("device_ptr", [](const PyTensor &self) { return (uint64_t)self.t.devicePtr(); })
        .def_property_readonly("shape",
                               [](const PyTensor &self) {
                                   py::tuple s(self.t.numDims());
                                   for (int i = 0; i < self.t.numDims(); ++i)
                                       s[i] = self.t.dims()[i];
                                   return s;
                               })
        .def_property_readonly("gpu_id", [](const PyTensor &self) { return self.t.gpuID(); });

    py::class_<Manager> renderer(m, "MadronaRenderer");
    renderer
        .def(py::init([](int gpu_id, int num_worlds, Manager::RenderMode render_mode,
                         int batch_render_view_width, int batch_render_view_height,
                         const std::vector<ImportedAsset> &asset_paths, CArray<float> mesh_vertices,
                         CArray<float> mesh_uvs, CArray<uint32_t> mesh_indices, CArray<uint32_t> mesh_vertex_offsets,
                         CArray<uint32_t> mesh_indices_offsets, CArray<int32_t> mesh_materials,
                         const std::vector<AdditionalMaterial> &mats,
                         const std::vector<std::string> &texture_paths,
                         const std::vector<ImportedInstance> &instances,
                         const std::vector<PyCamera> &pycameras,
                         const std::vector<Sim::WorldInit> &worlds,
                         const std::vector<int> &device_ids, int max_instances_per_world,
                         Manager::RenderOutputs render_outputs, py::object world_lights, py::object instance_colors,
                         py::object instance_materials, bool normals, py::object instance_labels, int supersample,
                         py::object positions, py::object boxes, py::object observations, py::object rays,
                         bool flow) {
                 const Options opt = parseOptions(render_outputs, supersample, positions, boxes, observations, rays, flow);
                 checkScene((size_t)num_worlds, worlds.size(), render_mode, pycameras, mesh_vertices, mesh_uvs,
                            mesh_vertex_offsets, mesh_indices_offsets, mesh_materials);

                 // fill the Config: the reference's fields first
                 ConfigStore s;
                 bool anyProjection = false;
                 for (const PyCamera &c : pycameras) {
                     s.cameras.push_back(c.cam);
                     s.projections.push_back(c.proj);
                     anyProjection = anyProjection || c.proj.vfovDeg != 90.0f || c.proj.znear != 0.0f;
                 }
                 for (const ImportedAsset &a : asset_paths) {
                     s.assetPaths.push_back(a.path.c_str());
                     s.matAssignments.push_back(a.matID);
                 }
                 for (const std::string &p : texture_paths)
                     s.texturePaths.push_back(p.c_str());
                 Manager::Config cfg {};
                 cfg.gpuID = gpu_id;
                 cfg.numWorlds = (uint32_t)num_worlds;
                 cfg.renderMode = render_mode;
                 cfg.batchRenderViewWidth = (uint32_t)batch_render_view_width;
                 cfg.batchRenderViewHeight = (uint32_t)batch_render_view_height;
                 auto &g = cfg.rcfg.geoCfg;
                 g.vertices = (const madrona::math::Vector3 *)mesh_vertices.data();
                 g.uvs = (const madrona::math::Vector2 *)mesh_uvs.data();
                 g.indices = mesh_indices.data();
                 g.meshVertexOffsets = mesh_vertex_offsets.data();
                 g.meshIndexOffsets = mesh_indices_offsets.data();
                 g.meshMaterials = mesh_materials.data();
                 g.numVertices = mesh_vertices.size() ? (uint32_t)mesh_vertices.shape(0) : 0;
                 g.numIndices = (uint32_t)mesh_indices.size();
                 g.numMeshes = (uint32_t)mesh_vertex_offsets.size();
                 cfg.rcfg.assetPaths = s.assetPaths.data();
                 cfg.rcfg.numAssetPaths = (uint32_t)s.assetPaths.size();
                 cfg.rcfg.matAssignments = s.matAssignments.data();
                 cfg.rcfg.numMatAssignments = (uint32_t)s.matAssignments.size();
                 cfg.rcfg.additionalMats = mats.data();
                 cfg.rcfg.numAdditionalMats = (uint32_t)mats.size();
                 cfg.rcfg.additionalTextures = s.texturePaths.data();
                 cfg.rcfg.numAdditionalTextures = (uint32_t)s.texturePaths.size();
                 cfg.rcfg.importedInstances = const_cast<ImportedInstance *>(instances.data());
                 cfg.rcfg.numInstances = (uint32_t)instances.size();
                 cfg.rcfg.cameras = s.cameras.data();
                 cfg.rcfg.numCameras = (uint32_t)s.cameras.size();
                 cfg.rcfg.worlds = const_cast<Sim::WorldInit *>(worlds.data());
                 // ... then the additions: one renderer over several devices; spare instance rows
                 cfg.deviceIDs = device_ids.empty() ? nullptr : device_ids.data();
                 cfg.numDevices = (uint32_t)device_ids.size();
                 if (max_instances_per_world < 0)
                     throw py::value_error("max_instances_per_world must not be negative");
                 cfg.maxInstancesPerWorld = (uint32_t)max_instances_per_world;
                 cfg.renderOutputs = render_outputs;
                 cfg.cameraProjections = anyProjection ? s.projections.data() : nullptr;
                 if (!world_lights.is_none()) {
                     s.lights = parseLights(world_lights, num_worlds);
                     cfg.worldLights = s.lights.data();
                 }
                 // instance_colors: None (no column), True (a zero-filled one) or [num_instances, 4] uint8
                 s.colors = parseColumn<uint8_t>(instance_colors, instances.size(), 4,
                                                 "instance_colors must be None, True or a uint8 array of shape [num_instances, 4]",
                                                 cfg.instanceColorColumn, cfg.instanceColors);
                 // instance_materials: None (no column), True (a column of -1) or [num_instances] int32
                 s.materials = parseColumn<int32_t>(instance_materials, instances.size(), 0,
                                                    "instance_materials must be None, True or an int32 array of shape [num_instances]",
                                                    cfg.instanceMaterialColumn, cfg.instanceMaterials);
                 cfg.normals = normals;
                 // instance_labels: None (no column), True (a column of MRX_LABEL_OBJECT) or [num_instances] int32
                 s.labels = parseColumn<int32_t>(instance_labels, instances.size(), 0,
                                                 "instance_labels must be None, True or an int32 array of shape [num_instances]",
                                                 cfg.instanceLabelColumn, cfg.instanceLabels);
                 cfg.supersample = (uint32_t)supersample;
                 cfg.positions = opt.positionFrame;
                 cfg.boxLabels = opt.boxLabels;
                 cfg.observations = opt.obs.field;
                 cfg.raysPerWorld = opt.raysPerWorld;
                 cfg.flow = flow;

                 std::unique_ptr<Manager> mgr(new Manager(cfg));
                 // (mrx_config cannot carry the range: the first frame is packed raw and restarted under it here)
                 if (opt.obs.hasRange)
                     mgr->setObservationDepthRange(opt.obs.lo, opt.obs.hi);
                 return mgr.release();
             }),
             py::arg("gpu_id"), py::arg("num_worlds"), py::arg("render_mode"),
             py::arg("batch_render_view_width"), py::arg("batch_render_view_height"),
             py::arg("asset_paths"), py::arg("mesh_vertices"), py::arg("mesh_uvs"),
             py::arg("mesh_indices"), py::arg("mesh_vertex_offsets"),
             py::arg("mesh_indices_offsets"), py::arg("mesh_materials"), py::arg("materials"),
             py::arg("texture_paths"), py::arg("instances"), py::arg("cameras"),
             py::arg("worlds"),
             // not in the reference (its callers never pass them): device_ids = [d0, d1, ...] makes this
             // one renderer span several devices (gpu_id is then ignored), max_instances_per_world
             // reserves hidden, unbound rows per world (see refresh_objects), render_outputs renders only depth
             // (RenderOutputs.Depth) or only rgb (RenderOutputs.RGB)
             py::arg("device_ids") = std::vector<int>(), py::arg("max_instances_per_world") = 0,
             py::arg("render_outputs") = Manager::RenderOutputs::RGBD,
             // world_lights = [(direction xyz, ambient, diffuse)] per world: the worlds' directional lights
             py::arg("world_lights") = py::none(),
             // instance_colors = True or a [num_instances, 4] uint8 array (r, g, b, a): the colour override column
             py::arg("instance_colors") = py::none(),
             // instance_materials = True or a [num_instances] int32 array: the material override column
             py::arg("instance_materials") = py::none(),
             // normals = True: the surface-normal output, normal_tensor()
             py::arg("normals") = false,
             // instance_labels = True or a [num_instances] int32 array: the label column (the segmask in both modes)
             py::arg("instance_labels") = py::none(),
             // supersample = s: every view rendered at s * width x s * height and resolved (sample_tensor, resolve)
             py::arg("supersample") = 1,
             // positions = True / "world" / "view": the point every pixel sees (position_tensor, unproject)
             py::arg("positions") = false,
             // boxes = K: the bounding box and pixel count of labels 0 ... K-1 in every view (box_tensor, boxes)
             py::arg("boxes") = py::none(),
             // observations = "rgbd" or dict(channels=, dtype=, stack=, depth_range=): the packed channel-first tensor a
             // policy takes (observation_tensor, observation_reset_tensor, observe, set_observation_depth_range)
             py::arg("observations") = py::none(),
             // rays = R: a ray-cast sensor of R rays per world (ray_tensor, ray_frame_tensor, ray_distance_tensor,
             // ray_id_tensor, trace)
             py::arg("rays") = py::none(),
             // flow = True: the optical-flow output (flow_tensor, flow, flow_snapshot); sets the visibility-ids flag
             py::arg("flow") = false)
        .def("step", &Manager::step)
        .def("render", &Manager::render)
        .def("sync", &Manager::sync)
        // supersampling: the factor; the s * W x s * H tensor the render writes for "rgb", "depth", "segmask",
        // "visibility" or "normal" (RuntimeError at factor 1 or on an output that is not rendered); the resolve stage alone
        .def_property_readonly("supersample", &Manager::supersample)
        .def("sample_tensor",
             [](py::object self, const std::string &name, py::object shard) {
                 static const std::pair<const char *, int> ids[] = {
                     { "rgb", MRX_BUF_RGB }, { "depth", MRX_BUF_DEPTH }, { "segmask", MRX_BUF_SEGMASK },
                     { "visibility", MRX_BUF_VISIBILITY }, { "normal", MRX_BUF_NORMAL } };
                 for (const auto &id : ids)
                     if (name == id.first)
                         return wrapTensor(self, self.cast<Manager &>().sampleTensor(id.second, shardOf(self, shard)));
                 throw py::value_error("sample_tensor: no output named " + name +
                                       " (rgb, depth, segmask, visibility, normal)");
             },
             py::arg("name"), py::arg("shard") = py::none())
        .def("resolve", &Manager::resolve)
        // position output: None, "world" or "view"; the unprojection stage alone
        .def_property_readonly("positions",
                               [](const Manager &self) -> py::object {
                                   const uint32_t f = self.positions();
                                   return f == 0 ? py::object(py::none()) : py::object(py::str(f == 2 ? "view" : "world"));
                               })
        .def("unproject", &Manager::unproject)
        // box labels: K or 0; the box stage alone
        .def_property_readonly("box_labels", &Manager::boxLabels)
        .def("boxes", &Manager::boxes)
        // ray-cast sensor: R or 0; the trace stage alone
        .def_property_readonly("rays", &Manager::rays)
        .def("trace", &Manager::trace)
        // optical-flow output: whether there is one; the flow stage alone, which does not advance the snapshot; the
        // snapshot stage alone (after an episode reset wrote the poses)
        .def_property_readonly("flows", &Manager::flows)
        .def("flow", &Manager::flow)
        .def("flow_snapshot", &Manager::flowSnapshot)
        // packed observation output: the option as a dict or None; the observation stage alone -- on a stacked renderer
        // one more frame; the depth range, whose setter restarts every stack
        .def_property_readonly("observations",
                               [](const Manager &self) -> py::object {
                                   const uint32_t f = self.observations();
                                   if (!f)
                                       return py::none();
                                   float lo = 0.0f, hi = 0.0f;
                                   self.observationDepthRange(&lo, &hi);
                                   py::dict d;
                                   d["channels"] = kObsChannels[(f & MRX_FLAG_OBS_LAYOUT_MASK) >> MRX_FLAG_OBS_SHIFT];
                                   d["dtype"] = kObsDtypes[(f & MRX_FLAG_OBS_DTYPE_MASK) >> MRX_FLAG_OBS_DTYPE_SHIFT];
                                   d["stack"] = 1u + ((f & MRX_FLAG_OBS_STACK_MASK) >> MRX_FLAG_OBS_STACK_SHIFT);
                                   d["depth_range"] = hi > 0.0f ? py::object(py::make_tuple(lo, hi)) : py::object(py::none());
                                   return d;
                               })
        .def("observe", &Manager::observe)
        .def("set_observation_depth_range",
             [](Manager &self, py::object lo, py::object hi) {
                 if (lo.is_none() && hi.is_none()) {
                     self.setObservationDepthRange(0.0f, 0.0f);
                     return;
                 }
                 float l = 0.0f, h = 0.0f;
                 parseObsRange(py::make_tuple(lo, hi), l, h);
                 self.setObservationDepthRange(l, h);
             },
             py::arg("lo"), py::arg("hi") = py::none())
        .def("rgb_cuda_ptr", [](py::object self, py::object shard) { return self.cast<Manager &>().rgbCudaPtr(shardOf(self, shard)); },
             py::arg("shard") = py::none())
        .def("depth_cuda_ptr", [](py::object self, py::object shard) { return self.cast<Manager &>().depthCudaPtr(shardOf(self, shard)); },
             py::arg("shard") = py::none())
        .def("segmask_cuda_ptr", [](py::object self, py::object shard) { return self.cast<Manager &>().segmaskCudaPtr(shardOf(self, shard)); },
             py::arg("shard") = py::none())
        // binds rows to the object ids their ObjectID column holds (spare rows: max_instances_per_world)
        .def("refresh_objects", &Manager::refreshObjects)
        .def_property_readonly("num_shards", &Manager::numShards)
        .def("shard_first_world", &Manager::shardFirstWorld, py::arg("shard"))
        .def("time_renders", &Manager::timeRenders, py::arg("steps"))
        .def("time_steps_host", &Manager::timeStepsHost, py::arg("steps"))
        .def("mark", &Manager::mark, py::arg("which"))
        .def("elapsed_ms", &Manager::elapsedMs)
        .def("bytes_per_step", &Manager::bytesPerStep)
        .def("render_path", [](Manager &self) { return std::string(self.renderPath()); })
        .def("raster_entry", [](Manager &self) { return std::string(self.rasterEntry()); })
        .def("kernel_form",
             [](Manager &self) {
                 // mrx_kernel_form: the instantiation the last render launched
                 const Manager::KernelFormInfo f = self.kernelForm();
                 py::dict d;
                 d["form"] = std::string(f.form);
                 d["slots"] = f.slots;
                 return d;
             })
        .def("bvh_launch",
             [](Manager &self) {
                 // mrx_bvh_launch: the BVH path's launch shape for the bound geometry
                 mrx_bvh_launch_t s = {};
                 if (mrx_bvh_launch(static_cast<mrx_renderer *>(self.nativeHandle()), &s) != MRX_OK)
                     throw std::runtime_error(mrx_last_error());
                 static const char *const kernels[] = {"none", "tile", "flat"};
                 py::dict d;
                 d["kernel"] = kernels[s.kernel >= 0 && s.kernel <= 2 ? s.kernel : 0];
                 d["tile"] = py::make_tuple(s.tile_w, s.tile_h);
                 d["classify"] = s.classify != 0;
                 d["textured"] = s.textured != 0;
                 d["record_cap"] = s.record_cap;
                 d["record_usable"] = s.record_usable;
                 d["tex_cap"] = s.tex_cap;
                 d["big_cap"] = s.big_cap;
                 d["pass_inst"] = s.pass_inst;
                 d["group_views"] = s.group_views;
                 d["mixed"] = s.mixed != 0;
                 d["priority"] = s.priority;
                 d["group_tiles"] = s.group_tiles;
                 d["small_area"] = s.small_area;
                 d["workgroups"] = s.workgroups;
                 return d;
             })
        .def("placement",
             [](Manager &self) {
                 float us[16] = {}, kept = 0.f;
                 const int n = self.placement(us, 16, &kept);
                 py::list cands;
                 for (int i = 0; i < n && i < 16; ++i)
                     cands.append(us[i]);
                 py::dict d;
                 d["tries"] = n > 0 ? n : 1;
                 d["candidates_us"] = cands;
                 d["kept_us"] = n > 0 ? py::object(py::float_(kept)) : py::object(py::none());
                 return d;
             })
        .def("native_handle", [](Manager &self) { return (uint64_t)self.nativeHandle(); })
        // per-view projection (views of the whole job from first_view on): vfov / znear are scalars (every view from
        // first_view to the end) or sequences (one entry per view; a scalar beside a sequence is broadcast);
        // znear None = the mode's default.  Stream-ordered: the next step renders with them.
        .def("set_camera_projection",
             [](Manager &self, py::object vfov, py::object znear, int64_t first_view) {
                 const int64_t total = (int64_t)self.numViews();
                 if (first_view < 0 || first_view > total)
                     throw py::value_error("first_view out of range");
                 bool fs = true, zs = true;
                 std::vector<float> fv = asVec(vfov, fs), zv;
                 if (znear.is_none())
                     zv.push_back(0.0f);
                 else {
                     zv = asVec(znear, zs);
                     for (float z : zv)
                         znearOf(z);
                 }
                 if (!fs && !zs && fv.size() != zv.size())
                     throw py::value_error("vfov and znear differ in length");
                 const int64_t n = !fs ? (int64_t)fv.size() : !zs ? (int64_t)zv.size() : total - first_view;
                 if (first_view + n > total)
                     throw py::value_error("more projections than views from first_view on");
                 std::vector<Manager::CameraProjection> proj((size_t)n);
                 for (int64_t i = 0; i < n; ++i) {
                     proj[(size_t)i].vfovDeg = fs ? fv[0] : fv[(size_t)i];
                     proj[(size_t)i].znear = zs ? zv[0] : zv[(size_t)i];
                     checkProjection(proj[(size_t)i]);
                 }
                 if (!self.setViewProjection((uint32_t)first_view, (uint32_t)n, proj.data()))
                     throw py::value_error(mrx_last_error());
             },
             py::arg("vfov"), py::arg("znear") = py::none(), py::arg("first_view") = 0)
        // per-world light (worlds of the whole job from first_world on): direction is one triple (every world from
        // first_world to the end) or an array [n, 3]; ambient / diffuse are None (each world keeps its own), scalars
        // or sequences of n, broadcast as set_camera_projection does.  Stream-ordered: the next step renders with them.
        .def("set_world_light",
             [](Manager &self, py::object direction, py::object ambient, py::object diffuse, int64_t first_world) {
                 const int64_t total = (int64_t)self.numWorlds();
                 if (first_world < 0 || first_world > total)
                     throw py::value_error("first_world out of range");
                 const CArray<float> dir(direction);
                 const bool one = dir.ndim() == 1;
                 if (!((one && dir.shape(0) == 3) || (dir.ndim() == 2 && dir.shape(1) == 3)))
                     throw py::value_error("direction must be one (x, y, z) or an array of shape [n, 3]");
                 bool as = true, ds = true;
                 std::vector<float> av, dv;
                 if (!ambient.is_none())
                     av = asVec(ambient, as);
                 if (!diffuse.is_none())
                     dv = asVec(diffuse, ds);
                 int64_t n = one ? -1 : (int64_t)dir.shape(0);
                 for (const auto &sv : { std::make_pair(as, &av), std::make_pair(ds, &dv) })
                     if (!sv.first) {
                         if (n >= 0 && (int64_t)sv.second->size() != n)
                             throw py::value_error("direction, ambient and diffuse differ in length");
                         n = (int64_t)sv.second->size();
                     }
                 if (n < 0)
                     n = total - first_world;
                 if (first_world + n > total)
                     throw py::value_error("more lights than worlds from first_world on");
                 std::vector<Manager::Light> lights((size_t)n);
                 if (n)
                     self.worldLights((uint32_t)first_world, (uint32_t)n, lights.data());
                 const float *d = dir.data();
                 for (int64_t i = 0; i < n; ++i) {
                     Manager::Light &l = lights[(size_t)i];
                     for (int c = 0; c < 3; ++c)
                         l.direction[c] = d[(one ? 0 : 3 * i) + c];
                     if (!ambient.is_none())
                         l.ambient = as ? av[0] : av[(size_t)i];
                     if (!diffuse.is_none())
                         l.diffuse = ds ? dv[0] : dv[(size_t)i];
                     checkLight(l);
                 }
                 if (!self.setWorldLights((uint32_t)first_world, (uint32_t)n, lights.data()))
                     throw py::value_error(mrx_last_error());
             },
             py::arg("direction"), py::arg("ambient") = py::none(), py::arg("diffuse") = py::none(),
             py::arg("first_world") = 0)
        .def("world_light",
             [](Manager &self) {
                 const uint32_t n = self.numWorlds();
                 std::vector<Manager::Light> lights(n);
                 self.worldLights(0, n, lights.data());
                 py::array_t<float> d({ (py::ssize_t)n, (py::ssize_t)3 }), a(n), f(n);
                 for (uint32_t i = 0; i < n; ++i) {
                     for (int c = 0; c < 3; ++c)
                         d.mutable_at(i, c) = lights[i].direction[c];
                     a.mutable_at(i) = lights[i].ambient;
                     f.mutable_at(i) = lights[i].diffuse;
                 }
                 return py::make_tuple(d, a, f);
             })
        // per-instance material override from host memory (rows of the whole job from first_row on; a renderer of
        // several shards splits them).  Stream-ordered: renders enqueued before keep the old ids.
        // per-instance labels from host memory, as set_instance_materials / instance_materials below
        .def("set_instance_labels",
             [](Manager &self, CArray<int32_t> ids, int64_t first_row) {
                 setRows(self, &Manager::setInstanceLabels, MRX_LABEL_OBJECT, "labels", "labels", ids, first_row);
             },
             py::arg("labels"), py::arg("first_row") = 0)
        .def("instance_labels", [](Manager &self) { return getRows(self, &Manager::instanceLabels, MRX_LABEL_OBJECT); })
        .def("set_instance_materials",
             [](Manager &self, CArray<int32_t> ids, int64_t first_row) {
                 setRows(self, &Manager::setInstanceMaterials, -1, "materials", "material ids", ids, first_row);
             },
             py::arg("materials"), py::arg("first_row") = 0)
        .def("instance_materials", [](Manager &self) { return getRows(self, &Manager::instanceMaterials, -1); })
        .def("camera_projection",
             [](Manager &self) {
                 const uint32_t n = self.numViews();
                 std::vector<Manager::CameraProjection> proj(n);
                 self.viewProjection(0, n, proj.data());
                 py::array_t<float> f(n), z(n);
                 for (uint32_t i = 0; i < n; ++i) {
                     f.mutable_at(i) = proj[i].vfovDeg;
                     z.mutable_at(i) = proj[i].znear;
                 }
                 return py::make_tuple(f, z);
             })
        // e.g. r.set_stream(torch.cuda.current_stream().cuda_stream): pose writes and
        // step() are then ordered on that stream without a host synchronisation
        .def("set_stream",
             [](Manager &self, uint64_t stream, py::object shard) {
                 if (shard.is_none())
                     self.setStream((void *)stream);
                 else
                     self.setShardStream(shard.cast<uint32_t>(), (void *)stream);
             },
             py::arg("stream"), py::arg("shard") = py::none())
        .def_readonly("num_agents", &Manager::numAgents);

    // the tensor getters, NAME(shard=None); one the renderer was created without raises RuntimeError
    const auto tensor = [&renderer](const char *name, Tensor (Manager::*get)(uint32_t) const) {
        renderer.def(name,
                     [get](py::object self, py::object shard) {
                         return wrapTensor(self, (self.cast<Manager &>().*get)(shardOf(self, shard)));
                     },
                     py::arg("shard") = py::none());
    };
    tensor("rgb_tensor", &Manager::rgbTensor);
    tensor("depth_tensor", &Manager::depthTensor);
    tensor("segmask_tensor", &Manager::segmaskTensor);
    tensor("visibility_tensor", &Manager::visibilityTensor);
    // u8 [views, H, W, 4], storage as rgb's: the view-space normal of every pixel's winning triangle (needs normals=True)
    tensor("normal_tensor", &Manager::normalTensor);
    // f32 [views, H, W, 4], (x, y, z, 1) per hit pixel and zeros on background (needs positions=)
    tensor("position_tensor", &Manager::positionTensor);
    // i32 [views, K, 5] = (xmin, ymin, xmax, ymax, count) (needs boxes=)
    tensor("box_tensor", &Manager::boxTensor);
    // f32 [worlds, R, 8] rays and i32 [worlds] mount rows, both written like a pose; f32 [worlds, R] t of the nearest hit
    // and i32 [worlds, R] the id of the row that was hit (need rays=)
    tensor("ray_tensor", &Manager::rayTensor);
    tensor("ray_frame_tensor", &Manager::rayFrameTensor);
    tensor("ray_distance_tensor", &Manager::rayDistanceTensor);
    tensor("ray_id_tensor", &Manager::rayIdTensor);
    // f32 [views, H, W, 4] = (dx, dy, dz, 1) per pixel whose point was in front of the previous camera, zeros elsewhere
    // (needs flow=True)
    tensor("flow_tensor", &Manager::flowTensor);
    // [views, S * C, H, W] in the dtype asked for, frame 0 the oldest (needs observations=); the reset column u8 [views]
    // (RuntimeError with stack 1)
    tensor("observation_tensor", &Manager::observationTensor);
    tensor("observation_reset_tensor", &Manager::observationResetTensor);
    tensor("instance_position_tensor", &Manager::instancePositionTensor);
    tensor("instance_rotation_tensor", &Manager::instanceRotationTensor);
    tensor("instance_scale_tensor", &Manager::instanceScaleTensor);
    tensor("instance_object_tensor", &Manager::instanceObjectTensor);
    // u8 [instances, 4]: the colour override of every row, a == 0 = none (needs instance_colors=)
    tensor("instance_color_tensor", &Manager::instanceColorTensor);
    // i32 [instances]: the label of every row, MRX_LABEL_OBJECT = the bound object's id (needs instance_labels=)
    tensor("instance_label_tensor", &Manager::instanceLabelTensor);
    // i32 [instances]: the material override of every row, outside the table = none (needs instance_materials=)
    tensor("instance_material_tensor", &Manager::instanceMaterialTensor);
    tensor("camera_position_tensor", &Manager::cameraPositionTensor);
    tensor("camera_rotation_tensor", &Manager::cameraRotationTensor);
}
