// renderer_headless -- the reference's command-line front end
// (/root/reference/src/headless.cpp:31-79, src/args.cpp:52-98, src/dump.cpp:45-119)
// over the MI355X Manager:
//
//   renderer_headless NUM_WORLDS NUM_STEPS rt|rast BATCH_WIDTH BATCH_HEIGHT
//                     [--dump-last-frame file_name_without_extension]
//                     [--scene synthetic|demo] [--depth] [--gpus N] [--outputs rgbd|depth|rgb]
//                     [--vfov DEG] [--znear Z]   (every camera's projection; no counterpart upstream)
//                     [--light X,Y,Z[,AMBIENT,DIFFUSE]]   (every world's directional light; no counterpart upstream)
//                     [--instance-colors SEED]   (an opaque colour override per instance row, splitmix64(SEED, row))
//                     [--instance-materials SEED]   (a material override per instance row, rows 1::4 left without)
//                     [--normals]   (the surface-normal output; --dump-last-frame also writes NAME.normals.png)
//                     [--instance-labels SEED]   (a label per instance row, rows 1::4 left at their object's id;
//                                                 --dump-last-frame also writes NAME.labels.png)
//                     [--supersample N]   (1 ... 4: every view rendered at N times the width and height and resolved;
//                                          --dump-last-frame writes the resolved images)
//                     [--positions [world|view]]   (the position output, world space unless `view`; --dump-last-frame
//                                                   also writes NAME.points.ply, the hit pixels' points; needs depth)
//                     [--boxes K]   (1 ... 1024: the bounding box and pixel count of labels 0 ... K-1 in every view;
//                                    --dump-last-frame also writes NAME.boxes.txt, one line
//                                    `view label xmin ymin xmax ymax count` per non-empty row; needs a segmask: rt, or
//                                    rast with --instance-labels)
//                     [--rays R]   (1 ... 65536: a ray-cast sensor of R rays per world, a horizontal fan of unit rays from
//                                   the world's first camera position; --dump-last-frame also writes NAME.rays.txt, one
//                                   line `world ray t id` per ray)
//                     [--flow]   (the optical-flow output: per pixel the image-space motion since the previous step;
//                                 --dump-last-frame also writes NAME.flow.npy, shape (views, H, W, 4), descr <f4; needs
//                                 depth, excludes --boxes and --instance-labels: the ids tensor holds visibility ids)
//                     [--observations CHANNELS[,DTYPE[,STACK]]]   (the packed observation output: rgb, rgbd, d, y or yd;
//                                    float32 (default), float16, bfloat16 or uint8; 1 ... 8 stacked frames;
//                                    --dump-last-frame also writes NAME.obs.npy, shape (views, STACK * C, H, W), descr
//                                    <f4, <f2, |u1 or, for bfloat16, <u2 holding the bit patterns)
//                     [--obs-depth-range LO,HI]   (depth channels normalised to 0 <= LO < HI; needs --observations with d)
//
// --outputs (no counterpart upstream, where the render config's RenderMode is pinned to RGBD)
// renders only depth or only rgb (Config::renderOutputs); --dump-last-frame then writes the
// output that exists -- for depth only, a grey tile of 1/depth (nearest hit of the frame white,
// background black) unless --depth asks for the reference's depth image.
//
// --gpus N (no counterpart upstream: the reference has a single gpuID,
// mgr.hpp:50) renders the worlds on N devices of the node through ONE Manager
// (Config::deviceIDs): contiguous world ranges whose sizes differ by at most
// one, one shard per device, step() launches on all of them, no exchange
// between the devices.  A line per device and the two reference lines for the
// whole node are printed.
//
// It steps the renderer NUM_STEPS times, prints the reference's two lines
// (`FPS`, `Average total step time`) and optionally writes the last frame of
// every world as one tiled PNG.  The reference constructs its Manager without
// a scene (headless.cpp:48-55 passes no rcfg); here the scene is either the
// synthetic cube+plane worlds of the benchmark or the reference's demo scene
// (viewer.cpp:74-164 / scripts/test.py:11-130).
#include <cerrno>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/madrona_mi355/manager.hpp"
#include "../../include/mrx.h"
#include "assets.hpp"
#include "obs_names.hpp"

#ifndef MRX_DATA_DIR
#define MRX_DATA_DIR "data"
#endif

using namespace madRender;
using madrona::math::Quat;
using madrona::math::Vector3;

namespace {

enum class Mode { Rasterizer, Raycaster };

struct Args {
    uint32_t numWorlds = 0, numSteps = 0, width = 64, height = 64;
    Mode mode = Mode::Rasterizer;
    bool dump = false, dumpDepth = false, demo = false;
    uint32_t gpus = 1;
    Manager::RenderOutputs outputs = Manager::RenderOutputs::RGBD;
    std::string outName;
    // --vfov DEG / --znear Z: the projection of every camera (0 = the mode's default near plane)
    float vfov = 90.0f, znear = 0.0f;
    // --light X,Y,Z[,AMBIENT,DIFFUSE]: the light of every world (the direction it travels; ambient, diffuse >= 0)
    bool hasLight = false;
    Manager::Light light = { { 1.0f, -1.0f, -0.05f }, 0.25f, 0.75f };
    // --instance-colors SEED: every instance row overridden with an opaque colour drawn from the seed and the row
    bool hasColors = false;
    uint64_t colorSeed = 0;
    // --instance-materials SEED: every instance row but rows 1::4 overridden with a material drawn from the seed and the row
    bool hasMaterials = false;
    uint64_t materialSeed = 0;
    // --normals: render the surface-normal output too; --dump-last-frame then also writes NAME.normals.png
    bool normals = false;
    // --instance-labels SEED: every instance row but rows 1::4 labelled 1000 + a draw from the seed and the row;
    // --dump-last-frame then also writes NAME.labels.png
    bool hasLabels = false;
    uint64_t labelSeed = 0;
    // --supersample N: the supersampling factor, 1 ... 4 (the sample image at most 16384 pixels a side)
    uint32_t supersample = 1;
    // --positions [world|view]: the position output (0 none, 1 world, 2 view); --dump-last-frame then also writes
    // NAME.points.ply
    uint32_t positions = 0;
    // --boxes K: box labels, 1 ... 1024; --dump-last-frame then also writes NAME.boxes.txt
    uint32_t boxes = 0;
    // --rays R: a ray-cast sensor of R rays per world, 1 ... 65536: a horizontal fan of unit rays from the world's first
    // camera position; --dump-last-frame then also writes NAME.rays.txt
    uint32_t rays = 0;
    // --flow: the optical-flow output; --dump-last-frame then also writes NAME.flow.npy
    bool flow = false;
    // --observations CHANNELS[,DTYPE[,STACK]]: the packed observation output (layout 0: none); --dump-last-frame then
    // also writes NAME.obs.npy.  --obs-depth-range LO,HI: the range its depth channels are normalised to
    uint32_t obsLayout = 0, obsDtype = 0, obsStack = 1;
    bool hasObsRange = false;
    float obsLo = 0.0f, obsHi = 0.0f;
};

// the comma-separated fields of an option's value
std::vector<std::string> splitCommas(const char *s)
{
    std::vector<std::string> fields(1);
    for (const char *ch = s; *ch; ++ch) {
        if (*ch == ',')
            fields.emplace_back();
        else
            fields.back() += *ch;
    }
    return fields;
}

// a refusal: the text on stderr, EXIT_FAILURE
[[noreturn]] __attribute__((format(printf, 1, 2))) void die(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    std::vfprintf(stderr, fmt, ap);
    va_end(ap);
    std::exit(EXIT_FAILURE);
}

// a number of the whole argument, finite
float parseFloat(const char *flag, const char *s)
{
    char *end = nullptr;
    const float v = std::strtof(s, &end);
    if (!*s || *end || !std::isfinite(v))
        die("%s: not a number: %s\n", flag, s);
    return v;
}

// an unsigned integer of the whole argument in `base` (0: strtoull's prefixes), without a sign
bool parseUnsigned(const char *s, int base, unsigned long long &v)
{
    char *end = nullptr;
    errno = 0;
    v = std::strtoull(s, &end, base);
    return *s && *s != '-' && *s != '+' && !*end && errno == 0;
}

// the SEED of --instance-colors, --instance-materials and --instance-labels
uint64_t parseSeed(const char *flag, const char *s)
{
    unsigned long long v = 0;
    if (!parseUnsigned(s, 0, v))
        die("%s: not an unsigned integer seed: %s\n", flag, s);
    return v;
}

// a decimal count in 1 ... hi; `what` is the noun of the refusal ("a factor", "a number of labels")
uint32_t parseCount(const char *flag, const char *what, unsigned long long hi, const char *s)
{
    unsigned long long v = 0;
    if (!parseUnsigned(s, 10, v) || v < 1 || v > hi)
        die("%s: not %s from 1 to %llu: %s\n", flag, what, hi, s);
    return (uint32_t)v;
}

[[noreturn]] void usage(const char *argv0)
{
    die("%s [NUM_WORLDS] [NUM_STEPS] [rt|rast] [BATCH_WIDTH] [BATCH_HEIGHT] "
        "[--dump-last-frame file_name_without_extension] [--scene synthetic|demo] [--depth] [--gpus N] [--outputs rgbd|depth|rgb] [--vfov DEG] [--znear Z] [--light X,Y,Z[,AMBIENT,DIFFUSE]] [--instance-colors SEED] [--instance-materials SEED] [--normals] [--instance-labels SEED] [--supersample N] [--positions [world|view]] [--boxes K] [--rays R] [--flow] [--observations CHANNELS[,DTYPE[,STACK]]] [--obs-depth-range LO,HI]\n",
        argv0);
}

Args parse(int argc, char **argv)
{
    if (argc < 6)
        usage(argv[0]);
    Args a;
    a.numWorlds = (uint32_t)std::atoi(argv[1]);
    a.numSteps = (uint32_t)std::atoi(argv[2]);
    if (!std::strcmp(argv[3], "rt")) a.mode = Mode::Raycaster;
    else if (!std::strcmp(argv[3], "rast")) a.mode = Mode::Rasterizer;
    else usage(argv[0]);
    a.width = (uint32_t)std::atoi(argv[4]);
    a.height = (uint32_t)std::atoi(argv[5]);
    for (int i = 6; i < argc; ++i) {
        // option `name` without a value; and the value of option `name`, null unless argv[i] is it and a value follows
        const auto is = [&](const char *name) { return !std::strcmp(argv[i], name); };
        const auto value = [&](const char *name) -> const char * { return is(name) && i + 1 < argc ? argv[++i] : nullptr; };
        const char *v = nullptr;
        if ((v = value("--dump-last-frame"))) {
            a.dump = true;
            a.outName = v;
        } else if ((v = value("--scene"))) {
            a.demo = !std::strcmp(v, "demo");
        } else if (is("--depth")) {
            a.dumpDepth = true;
        } else if (is("--normals")) {
            a.normals = true;
        } else if ((v = value("--gpus"))) {
            a.gpus = (uint32_t)std::atoi(v);
        } else if ((v = value("--vfov"))) {
            a.vfov = parseFloat("--vfov", v);
            if (!(a.vfov > 0.0f && a.vfov < 180.0f))
                die("--vfov: %s is not in (0, 180) degrees\n", v);
        } else if ((v = value("--light"))) {
            // three or five numbers; the library's own check decides (mrx_light_constants needs no device)
            const std::vector<std::string> fields = splitCommas(v);
            const size_t n = fields.size();
            float l[5] = { 0.0f, 0.0f, 0.0f, a.light.ambient, a.light.diffuse }, c[5];
            for (size_t k = 0; k < n && k < 5; ++k)
                l[k] = parseFloat("--light", fields[k].c_str());
            if (n != 3 && n != 5)
                die("--light: wants X,Y,Z or X,Y,Z,AMBIENT,DIFFUSE, got %s\n", v);
            if (mrx_light_constants(mrx_light { { l[0], l[1], l[2] }, l[3], l[4] }, c) != MRX_OK)
                die("--light: %s\n", mrx_last_error());
            a.light = { { l[0], l[1], l[2] }, l[3], l[4] };
            a.hasLight = true;
        } else if ((v = value("--instance-colors"))) {
            a.colorSeed = parseSeed("--instance-colors", v);
            a.hasColors = true;
        } else if ((v = value("--instance-materials"))) {
            a.materialSeed = parseSeed("--instance-materials", v);
            a.hasMaterials = true;
        } else if ((v = value("--instance-labels"))) {
            a.labelSeed = parseSeed("--instance-labels", v);
            a.hasLabels = true;
        } else if ((v = value("--supersample"))) {
            a.supersample = parseCount("--supersample", "a factor", 4, v);
        } else if ((v = value("--boxes"))) {
            a.boxes = parseCount("--boxes", "a number of labels", 1024, v);
        } else if ((v = value("--rays"))) {
            a.rays = parseCount("--rays", "a number of rays per world", 65536, v);
        } else if (is("--flow")) {
            a.flow = true;
        } else if ((v = value("--observations"))) {
            const std::vector<std::string> f = splitCommas(v);
            const uint32_t layout = obsLayoutOf(f[0]), dtype = f.size() > 1 ? obsDtypeOf(f[1]) : 0u;
            uint32_t stack = 1;
            if (f.size() > 2) {
                const char *t = f[2].c_str();
                stack = t[0] >= '1' && t[0] <= '8' && !t[1] ? (uint32_t)(t[0] - '0') : 0u;
            }
            if (!layout || dtype == kNumObsDtypes || !stack || f.size() > 3)
                die("--observations: wants CHANNELS[,DTYPE[,STACK]] -- rgb|rgbd|d|y|yd, "
                    "float32|float16|bfloat16|uint8, 1 ... 8 -- got: %s\n", v);
            a.obsLayout = layout; a.obsDtype = dtype; a.obsStack = stack;
        } else if ((v = value("--obs-depth-range"))) {
            const std::vector<std::string> f = splitCommas(v);
            if (f.size() != 2)
                die("--obs-depth-range: wants LO,HI, got: %s\n", v);
            a.obsLo = parseFloat("--obs-depth-range", f[0].c_str());
            a.obsHi = parseFloat("--obs-depth-range", f[1].c_str());
            if (!(a.obsLo >= 0.0f && a.obsLo < a.obsHi))
                die("--obs-depth-range: wants 0 <= LO < HI, got: %s\n", v);
            a.hasObsRange = true;
        } else if (is("--positions")) {
            // the frame is optional: the next argument is taken for it unless it is another option
            a.positions = 1;
            if (i + 1 < argc && std::strncmp(argv[i + 1], "--", 2) != 0) {
                const char *f = argv[++i];
                if (!std::strcmp(f, "view"))
                    a.positions = 2;
                else if (std::strcmp(f, "world") != 0)
                    die("--positions: the frame is world or view, not: %s\n", f);
            }
        } else if ((v = value("--znear"))) {
            a.znear = parseFloat("--znear", v);
            if (!(a.znear > 0.0f))
                die("--znear: %s is not > 0\n", v);
        } else if ((v = value("--outputs"))) {
            if (!std::strcmp(v, "rgbd")) a.outputs = Manager::RenderOutputs::RGBD;
            else if (!std::strcmp(v, "depth")) a.outputs = Manager::RenderOutputs::Depth;
            else if (!std::strcmp(v, "rgb")) a.outputs = Manager::RenderOutputs::RGB;
            else usage(argv[0]);
        } else {
            usage(argv[0]);
        }
    }
    const bool noRgb = a.outputs == Manager::RenderOutputs::Depth, noDepth = a.outputs == Manager::RenderOutputs::RGB;
    if (a.numWorlds == 0 || a.width == 0 || a.height == 0 || a.gpus == 0 || a.gpus > a.numWorlds)
        usage(argv[0]);
    if ((uint64_t)a.supersample * a.width > 16384 || (uint64_t)a.supersample * a.height > 16384)
        die("--supersample: %u times %u x %u is more than 16384 pixels a side\n", a.supersample, a.width, a.height);
    if (a.mode == Mode::Raycaster && !(a.znear < 1000.0f))
        die("--znear: must be below the Raytracer far plane (1000)\n");
    if (a.dumpDepth && noDepth)
        die("--depth: depth is not rendered with --outputs rgb\n");
    if (a.positions && noDepth)
        die("--positions: positions are computed from depth, which is not rendered with --outputs rgb\n");
    if (a.flow && noDepth)
        die("--flow: the flow is computed from depth, which is not rendered with --outputs rgb\n");
    if (a.flow && (a.boxes || a.hasLabels))
        die("--flow: the ids tensor holds visibility ids, so there is no segmask for --boxes or --instance-labels\n");
    if (a.boxes && a.mode == Mode::Rasterizer && !a.hasLabels)
        die("--boxes: boxes are computed from the segmask, which rast has only with --instance-labels\n");
    const bool colour = a.obsLayout && a.obsLayout != MRX_OBS_D;
    const bool depth = a.obsLayout == MRX_OBS_RGBD || a.obsLayout == MRX_OBS_D || a.obsLayout == MRX_OBS_YD;
    if (colour && noRgb)
        die("--observations: these channels need rgb, which is not rendered with --outputs depth\n");
    if (depth && noDepth)
        die("--observations: these channels need depth, which is not rendered with --outputs rgb\n");
    if (a.hasObsRange && !depth)
        die("--obs-depth-range: needs --observations with a depth channel (rgbd, d or yd)\n");
    return a;
}

uint64_t splitmix64(uint64_t x)
{
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// u(k) = (splitmix64(seed ^ k) >> 40) * 2^-24
double uniform(uint64_t k)
{
    uint64_t z = (0x4D52584Dull ^ k) + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 40) * 0x1p-24;
}

// camera at `eye` looking at `tgt`: local +Y forward, +X right, +Z up, no roll
Quat lookAt(const float eye[3], const double tgt[3])
{
    double f[3] = { tgt[0] - eye[0], tgt[1] - eye[1], tgt[2] - eye[2] };
    double n = std::sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
    for (double &x : f) x /= n;
    double r[3] = { f[1] * 1.0 - f[2] * 0.0, f[2] * 0.0 - f[0] * 1.0, f[0] * 0.0 - f[1] * 0.0 };
    n = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    for (double &x : r) x /= n;
    double u[3] = { r[1] * f[2] - r[2] * f[1], r[2] * f[0] - r[0] * f[2], r[0] * f[1] - r[1] * f[0] };
    // rotation with columns (right, fwd, up) -> quaternion
    const double m[3][3] = { { r[0], f[0], u[0] }, { r[1], f[1], u[1] }, { r[2], f[2], u[2] } };
    const double tr = m[0][0] + m[1][1] + m[2][2];
    double q[4];
    if (tr > 0) {
        const double s = std::sqrt(tr + 1.0) * 2;
        q[0] = 0.25 * s; q[1] = (m[2][1] - m[1][2]) / s;
        q[2] = (m[0][2] - m[2][0]) / s; q[3] = (m[1][0] - m[0][1]) / s;
    } else if (m[0][0] > m[1][1] && m[0][0] > m[2][2]) {
        const double s = std::sqrt(1.0 + m[0][0] - m[1][1] - m[2][2]) * 2;
        q[0] = (m[2][1] - m[1][2]) / s; q[1] = 0.25 * s;
        q[2] = (m[0][1] + m[1][0]) / s; q[3] = (m[0][2] + m[2][0]) / s;
    } else if (m[1][1] > m[2][2]) {
        const double s = std::sqrt(1.0 + m[1][1] - m[0][0] - m[2][2]) * 2;
        q[0] = (m[0][2] - m[2][0]) / s; q[1] = (m[0][1] + m[1][0]) / s;
        q[2] = 0.25 * s; q[3] = (m[1][2] + m[2][1]) / s;
    } else {
        const double s = std::sqrt(1.0 + m[2][2] - m[0][0] - m[1][1]) * 2;
        q[0] = (m[1][0] - m[0][1]) / s; q[1] = (m[0][2] + m[2][0]) / s;
        q[2] = (m[1][2] + m[2][1]) / s; q[3] = 0.25 * s;
    }
    return Quat { (float)q[0], (float)q[1], (float)q[2], (float)q[3] };
}

struct Scene {
    std::vector<std::string> paths;
    std::vector<const char *> pathPtrs;
    std::vector<int32_t> matAssign;
    std::vector<AdditionalMaterial> mats;
    std::vector<std::string> texPaths;
    std::vector<const char *> texPtrs;
    std::vector<ImportedInstance> instances;
    std::vector<ImportedCamera> cameras;
    std::vector<Sim::WorldInit> worlds;
    std::vector<Vector3> verts;
    std::vector<madrona::math::Vector2> uvs;
    std::vector<uint32_t> indices, vertOff, idxOff;
    std::vector<int32_t> meshMats;
};

// worlds [first, first + n) of the synthetic job: world ids are global, so a
// shard holds exactly the rows it would own of the whole job's scene
void buildSynthetic(Scene &s, uint32_t first, uint32_t n, const std::string &dataDir)
{
    s.paths = { dataDir + "/cube.obj", dataDir + "/plane.obj" };
    s.matAssign = { 0, 0 };
    s.mats = { { { 0.588f, 0.588f, 0.588f, 1.0f }, -1, 0.8f, 0.2f },
               { { 1.0f, 1.0f, 1.0f, 1.0f }, 0, 0.8f, 0.2f } };
    s.texPaths = { dataDir + "/cube.png" };
    const double pi = 3.14159265358979323846;
    for (uint32_t w = 0; w < n; ++w) {
        double u[12];
        for (int j = 0; j < 12; ++j)
            u[j] = uniform((uint64_t)(first + w) * 16 + j);
        const double sc = 1.0 + 2.0 * u[2], th = 2.0 * pi * u[3];
        s.instances.push_back({ { 0.f, 0.f, 0.f }, { 1.f, 0.f, 0.f, 0.f }, { 1.f, 1.f, 1.f }, 1 });
        s.instances.push_back({ { (float)(-4 + 8 * u[0]), (float)(-4 + 8 * u[1]), (float)(0.5 * sc) },
                                { (float)std::cos(th / 2), 0.f, 0.f, (float)std::sin(th / 2) },
                                { (float)sc, (float)sc, (float)sc }, 0 });
        const double r = 10.0 + 6.0 * u[7], hgt = 3.0 + 5.0 * u[8], az = 2.0 * pi * u[9];
        const float eye[3] = { (float)(r * std::cos(az)), (float)(r * std::sin(az)), (float)hgt };
        const double tgt[3] = { 0.0, 0.0, 1.0 };
        s.cameras.push_back({ { eye[0], eye[1], eye[2] }, lookAt(eye, tgt) });
        s.worlds.push_back({ 2, w * 2, 1, w });
    }
}

void buildDemo(Scene &s, uint32_t n, const std::string &dataDir)
{
    s.paths = { dataDir + "/cube.obj" };
    s.matAssign = { 0 };
    s.mats = { { { 1.f, 1.f, 1.f, 1.f }, 0, 0.8f, 0.2f } };
    s.texPaths = { dataDir + "/cube.png" };
    s.verts = { { 0.f, 0.f, 0.f }, { 5.f, 0.f, 10.f }, { 10.f, 0.f, 0.f } };
    s.uvs = { { 0.f, 0.f }, { 0.f, 0.f }, { 0.f, 0.f } };
    s.indices = { 0, 1, 2 };
    s.vertOff = { 0 };
    s.idxOff = { 0 };
    s.meshMats = { -1 };
    s.instances = { { { 0.f, 0.f, 15.f }, { 0.707107f, 0.707107f, 0.f, 0.f }, { 3.f, 3.f, 3.f }, 0 },
                    { { 0.f, 0.f, 15.f }, { 0.707107f, 0.707107f, 0.f, 0.f }, { 10.f, 10.f, 10.f }, 1 } };
    s.cameras = { { { -22.343935f, -21.845375f, 27.061676f },
                    { 0.913407f, -0.112268f, 0.047731f, -0.388336f } } };
    for (uint32_t w = 0; w < n; ++w)
        s.worlds.push_back({ 2, 0, 1, 0 });
}

// Tiled dump, as /root/reference/src/dump.cpp:45-119: ceil(sqrt(N)) rows of
// images; depth as grey 255 * min(d / 255, 1).  Raytracer storage is [x][y]
// and is transposed back (dump.cpp:9-21); rasterizer storage is row-major.
// DumpWhat::InvDepth (a depth-only renderer's default): grey 255 * dmin / d, dmin = the
// nearest depth of the frame, 0 for background.
// DumpWhat::Normal: the surface-normal tensor, in rgb's format (its bytes as they are, alpha included).
// DumpWhat::Labels: the segmask of a renderer with the label column: the low 24 bits of each pixel's label as
// (r, g, b), r lowest, alpha 255; background pixels (-1) are (0, 0, 0, 0).
enum class DumpWhat { Rgb, Depth, InvDepth, Normal, Labels };

// how a dump ends when the library refused a copy: its text on stderr, false
bool libraryError()
{
    std::fprintf(stderr, "%s\n", mrx_last_error());
    return false;
}

// the tail of the dumps below: `head`, then `bodyBytes` of `body`, as the file `path`; false, and a line on stderr,
// unless every byte was written and the file closed
bool writeFile(const std::string &path, const std::string &head, const void *body = nullptr, size_t bodyBytes = 0)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    bool ok = f && std::fwrite(head.data(), 1, head.size(), f) == head.size() &&
              (!bodyBytes || std::fwrite(body, 1, bodyBytes, f) == bodyBytes);
    if (f && std::fclose(f) != 0)
        ok = false;
    if (!ok)
        std::fprintf(stderr, "cannot write %s\n", path.c_str());
    return ok;
}

bool dumpTiled(const std::string &name, mrx_renderer *shard, uint32_t numImages, uint32_t resX,
               uint32_t resY, DumpWhat what, bool transpose)
{
    const bool depth = what != DumpWhat::Rgb && what != DumpWhat::Normal && what != DumpWhat::Labels;
    const size_t bytesPerImage = (size_t)4 * resX * resY;
    std::vector<uint8_t> host(bytesPerImage * numImages);
    if (mrx_copy_to_host(shard, depth ? MRX_BUF_DEPTH : what == DumpWhat::Normal ? MRX_BUF_NORMAL
                                : what == DumpWhat::Labels ? MRX_BUF_SEGMASK : MRX_BUF_RGB,
                         host.data(), host.size()) != MRX_OK)
        return libraryError();
    float dmin = 0.0f;
    if (what == DumpWhat::InvDepth)
        for (size_t i = 0; i < host.size() / 4; ++i) {
            float d;
            std::memcpy(&d, host.data() + 4 * i, 4);
            if (d > 0.0f && (dmin == 0.0f || d < dmin))
                dmin = d;
        }
    const uint32_t tilesY = (uint32_t)std::ceil(std::sqrt((double)numImages));
    const uint32_t tilesX = (uint32_t)std::ceil((double)numImages / tilesY);
    const uint32_t outW = tilesX * resX, outH = tilesY * resY;
    std::vector<uint8_t> img((size_t)outW * outH * 4, 0);
    for (uint32_t i = 0; i < numImages; ++i) {
        const uint32_t tx = i % tilesX, ty = i / tilesX;
        const uint8_t *src = host.data() + bytesPerImage * i;
        for (uint32_t y = 0; y < resY; ++y)
            for (uint32_t x = 0; x < resX; ++x) {
                const size_t si = transpose ? ((size_t)x * resY + y) : ((size_t)y * resX + x);
                uint8_t *dst = &img[(((size_t)ty * resY + y) * outW + tx * resX + x) * 4];
                if (depth) {
                    float d;
                    std::memcpy(&d, src + 4 * si, 4);
                    const uint8_t g = what == DumpWhat::InvDepth
                                          ? (uint8_t)(d > 0.0f ? 255.0f * std::fmin(dmin / d, 1.0f) : 0.0f)
                                          : (uint8_t)(255.0f * std::fmin(d / 255.0f, 1.0f));
                    dst[0] = dst[1] = dst[2] = g;
                    dst[3] = 255;
                } else if (what == DumpWhat::Labels) {
                    int32_t lab;
                    std::memcpy(&lab, src + 4 * si, 4);
                    const uint32_t px = lab == -1 ? 0u : (((uint32_t)lab & 0xFFFFFFu) | 0xFF000000u);
                    dst[0] = (uint8_t)px; dst[1] = (uint8_t)(px >> 8); dst[2] = (uint8_t)(px >> 16); dst[3] = (uint8_t)(px >> 24);
                } else {
                    std::memcpy(dst, src + 4 * si, 4);
                }
            }
    }
    std::string err;
    if (!mrx::encodePNG(name + ".png", img.data(), outW, outH, err)) {
        std::fprintf(stderr, "%s\n", err.c_str());
        return false;
    }
    return true;
}

// NAME.ply of --positions: binary little-endian PLY, one vertex per hit pixel (w != 0) of the first `numImages` views
// in storage order: float x y z, and uchar red green blue where rgb is rendered (its storage is the positions').
bool dumpPly(const std::string &name, mrx_renderer *shard, uint32_t numImages, uint32_t resX, uint32_t resY, bool withRgb)
{
    const size_t px = (size_t)numImages * resX * resY;
    std::vector<float> pos(px * 4);
    std::vector<uint8_t> rgb(withRgb ? px * 4 : 0);
    if (mrx_copy_to_host(shard, MRX_BUF_POSITION, pos.data(), pos.size() * sizeof(float)) != MRX_OK ||
        (withRgb && mrx_copy_to_host(shard, MRX_BUF_RGB, rgb.data(), rgb.size()) != MRX_OK))
        return libraryError();
    size_t hits = 0;
    for (size_t i = 0; i < px; ++i)
        hits += pos[4 * i + 3] != 0.0f ? 1 : 0;
    std::string out = "ply\nformat binary_little_endian 1.0\nelement vertex " + std::to_string(hits) +
                      "\nproperty float x\nproperty float y\nproperty float z\n";
    if (withRgb)
        out += "property uchar red\nproperty uchar green\nproperty uchar blue\n";
    out += "end_header\n";
    out.reserve(out.size() + hits * (withRgb ? 15 : 12));
    for (size_t i = 0; i < px; ++i) {
        if (pos[4 * i + 3] == 0.0f)
            continue;
        out.append(reinterpret_cast<const char *>(&pos[4 * i]), 12);   // (the hosts this runs on are little-endian)
        if (withRgb)
            out.append(reinterpret_cast<const char *>(&rgb[4 * i]), 3);
    }
    return writeFile(name + ".ply", out);
}

// NAME.boxes.txt of --boxes: one line `view label xmin ymin xmax ymax count` per non-empty row of the box tensor of
// the first `numImages` views, in the tensor's order
bool dumpBoxes(const std::string &name, mrx_renderer *shard, uint32_t numImages, uint32_t K)
{
    std::vector<int32_t> rows((size_t)numImages * K * 5);
    if (mrx_copy_to_host(shard, MRX_BUF_BOXES, rows.data(), rows.size() * sizeof(int32_t)) != MRX_OK)
        return libraryError();
    std::string out;
    char line[160];
    for (size_t i = 0; i < (size_t)numImages * K; ++i) {
        const int32_t *b = &rows[5 * i];
        if (b[4] > 0) {
            std::snprintf(line, sizeof line, "%zu %zu %d %d %d %d %d\n", i / K, i % K, b[0], b[1], b[2], b[3], b[4]);
            out += line;
        }
    }
    return writeFile(name + ".boxes.txt", out);
}

// NAME.rays.txt of --rays: one line `world ray t id` per ray of the shard's worlds (world numbers are the job's), t with
// nine significant digits
bool dumpRays(const std::string &name, mrx_renderer *shard, uint32_t firstWorld, uint32_t numWorlds, uint32_t R)
{
    std::vector<float> t((size_t)numWorlds * R);
    std::vector<int32_t> id((size_t)numWorlds * R);
    if (mrx_copy_to_host(shard, MRX_BUF_RAY_DISTANCE, t.data(), t.size() * sizeof(float)) != MRX_OK ||
        mrx_copy_to_host(shard, MRX_BUF_RAY_ID, id.data(), id.size() * sizeof(int32_t)) != MRX_OK)
        return libraryError();
    std::string out;
    char line[96];
    for (size_t i = 0; i < t.size(); ++i) {
        std::snprintf(line, sizeof line, "%zu %zu %.9g %d\n", firstWorld + i / R, i % R, (double)t[i], id[i]);
        out += line;
    }
    return writeFile(name + ".rays.txt", out);
}

// A four-dimensional tensor of the shard as a NumPy file (format 1.0), NAME + suffix, in the tensor's own shape and
// order.  NAME.obs.npy of --observations: the observation tensor, (views, S * C, H, W); bfloat16 has no NumPy type and
// goes out as <u2, the bit patterns.  NAME.flow.npy of --flow: the flow tensor, (views, H, W, 4) <f4.
bool dumpNpy(const std::string &name, mrx_renderer *shard, int which = MRX_BUF_OBSERVATION, const char *suffix = ".obs.npy")
{
    int64_t dims[4] = { 0, 0, 0, 0 };
    int nd = 0, dt = 0, dev = 0;
    if (!mrx_buffer(shard, which, dims, &nd, &dt, &dev) || nd != 4)
        return libraryError();
    const char *descr = dt == MRX_DTYPE_F32 ? "<f4" : dt == MRX_DTYPE_F16 ? "<f2" : dt == MRX_DTYPE_BF16 ? "<u2" : "|u1";
    const size_t elem = dt == MRX_DTYPE_F32 ? 4 : dt == MRX_DTYPE_U8 ? 1 : 2;
    std::vector<uint8_t> data((size_t)(dims[0] * dims[1] * dims[2] * dims[3]) * elem);
    if (mrx_copy_to_host(shard, which, data.data(), data.size()) != MRX_OK)
        return libraryError();
    char dict[160];
    std::snprintf(dict, sizeof dict, "{'descr': '%s', 'fortran_order': False, 'shape': (%lld, %lld, %lld, %lld), }", descr,
                  (long long)dims[0], (long long)dims[1], (long long)dims[2], (long long)dims[3]);
    std::string header = dict;
    while ((10 + header.size() + 1) % 64 != 0)      // magic, version and length are 10 bytes; the data starts 64-aligned
        header += ' ';
    header += '\n';
    std::string out("\x93NUMPY\x01\x00", 8);
    out += (char)(header.size() & 0xFF);
    out += (char)(header.size() >> 8);
    out += header;
    return writeFile(name + suffix, out, data.data(), data.size());
}

}  // namespace

int main(int argc, char **argv)
{
    const Args args = parse(argc, argv);
    const char *dd = std::getenv("MADRONA_MI355_DATA");
    const std::string dataDir = dd ? dd : MRX_DATA_DIR;
    // MRX_HEADLESS_REHEARSAL=1: every shard on device 0 -- walks the N-device
    // control flow on a one-GPU box (the numbers then mean nothing)
    const char *reh = std::getenv("MRX_HEADLESS_REHEARSAL");
    const bool rehearsal = reh && reh[0] == '1';
    if (!rehearsal && (int)args.gpus > mrx_device_count()) {
        std::fprintf(stderr, "--gpus %u but %d HIP device(s) visible\n", args.gpus, mrx_device_count());
        return EXIT_FAILURE;
    }

    // the whole job's scene; ONE Manager spans the devices (Config::deviceIDs): it splits the
    // worlds into contiguous ranges, one shard per device, and step() launches on all of them
    Scene s;
    if (args.demo) buildDemo(s, args.numWorlds, dataDir);
    else buildSynthetic(s, 0, args.numWorlds, dataDir);
    for (auto &p : s.paths) s.pathPtrs.push_back(p.c_str());
    for (auto &p : s.texPaths) s.texPtrs.push_back(p.c_str());
    std::vector<int> devices(args.gpus);
    for (uint32_t g = 0; g < args.gpus; ++g)
        devices[g] = rehearsal ? 0 : (int)g;

    Manager::Config cfg {};
    cfg.gpuID = devices[0];
    cfg.numWorlds = args.numWorlds;
    cfg.renderMode = args.mode == Mode::Raycaster ? Manager::RenderMode::Raytracer
                                                  : Manager::RenderMode::Rasterizer;
    cfg.batchRenderViewWidth = args.width;
    cfg.batchRenderViewHeight = args.height;
    cfg.headlessMode = true;
    auto &rc = cfg.rcfg;
    rc.geoCfg = { s.verts.data(), s.uvs.data(), s.indices.data(), s.vertOff.data(), s.idxOff.data(),
                  s.meshMats.data(), (uint32_t)s.verts.size(), (uint32_t)s.indices.size(),
                  (uint32_t)s.vertOff.size() };
    rc.assetPaths = s.pathPtrs.data();
    rc.numAssetPaths = (uint32_t)s.pathPtrs.size();
    rc.matAssignments = s.matAssign.data();
    rc.numMatAssignments = (uint32_t)s.matAssign.size();
    rc.additionalMats = s.mats.data();
    rc.numAdditionalMats = (uint32_t)s.mats.size();
    rc.additionalTextures = s.texPtrs.data();
    rc.numAdditionalTextures = (uint32_t)s.texPtrs.size();
    rc.importedInstances = s.instances.data();
    rc.numInstances = (uint32_t)s.instances.size();
    rc.cameras = s.cameras.data();
    rc.numCameras = (uint32_t)s.cameras.size();
    const std::vector<Manager::CameraProjection> projections(s.cameras.size(), { args.vfov, args.znear });
    if (args.vfov != 90.0f || args.znear != 0.0f)
        cfg.cameraProjections = projections.data();
    const std::vector<Manager::Light> lights(args.numWorlds, args.light);
    if (args.hasLight)
        cfg.worldLights = lights.data();
    // --instance-colors: row i of the instance table gets (r, g, b) = the low bytes of splitmix64(splitmix64(SEED) ^ i)
    std::vector<uint8_t> colors;
    if (args.hasColors) {
        const uint64_t base = splitmix64(args.colorSeed);
        for (uint64_t i = 0; i < s.instances.size(); ++i) {
            const uint64_t z = splitmix64(base ^ i);
            colors.insert(colors.end(), { (uint8_t)z, (uint8_t)(z >> 8), (uint8_t)(z >> 16), (uint8_t)255 });
        }
        cfg.instanceColors = colors.data();
    }
    // --instance-materials: row i gets material splitmix64(splitmix64(SEED) ^ i) % (the scene's API materials); rows
    // 1::4 -- and every row of a scene without materials -- keep -1, no override
    std::vector<int32_t> matIds;
    if (args.hasMaterials) {
        const uint64_t base = splitmix64(args.materialSeed), nm = s.mats.size();
        for (uint64_t i = 0; i < s.instances.size(); ++i)
            matIds.push_back(nm && i % 4 != 1 ? (int32_t)(splitmix64(base ^ i) % nm) : -1);
        cfg.instanceMaterials = matIds.data();
        cfg.instanceMaterialColumn = true;
    }
    // --instance-labels: row i gets 1000 + splitmix64(splitmix64(SEED) ^ i) % 1000; rows 1::4 keep the sentinel, the id
    // of their bound object
    std::vector<int32_t> labels;
    if (args.hasLabels) {
        const uint64_t base = splitmix64(args.labelSeed);
        for (uint64_t i = 0; i < s.instances.size(); ++i)
            labels.push_back(i % 4 != 1 ? (int32_t)(1000 + splitmix64(base ^ i) % 1000) : Manager::kLabelObject);
        cfg.instanceLabels = labels.data();
        cfg.instanceLabelColumn = true;
    }
    rc.worlds = s.worlds.data();
    if (args.gpus > 1) {
        cfg.deviceIDs = devices.data();
        cfg.numDevices = args.gpus;
    }
    cfg.renderOutputs = args.outputs;
    cfg.normals = args.normals;
    cfg.supersample = args.supersample;
    cfg.positions = args.positions;
    cfg.boxLabels = args.boxes;
    cfg.raysPerWorld = args.rays;
    cfg.flow = args.flow;
    if (args.obsLayout)
        cfg.observations = MRX_FLAG_OBSERVATIONS(args.obsLayout, args.obsDtype, args.obsStack);

    Manager mgr(cfg);              // aborts (FATAL) on failure, like the reference
    if (args.hasObsRange)
        mgr.setObservationDepthRange(args.obsLo, args.obsHi);
    // --rays: ray i of a world leaves its first camera's position at angle 2 pi i / R in the XY plane, t in (0, 1000]
    if (args.rays) {
        mrx_renderer *top = (mrx_renderer *)mgr.nativeHandle();
        for (uint32_t g = 0; g < mgr.numShards(); ++g) {
            const uint32_t lo = mgr.shardFirstWorld(g), hi = mgr.shardFirstWorld(g + 1);
            std::vector<float> fan((size_t)(hi - lo) * args.rays * 8u);
            for (uint32_t w = lo; w < hi; ++w) {
                const ImportedCamera &cam = s.cameras[s.worlds[w].camerasOffset];
                for (uint32_t i = 0; i < args.rays; ++i) {
                    const double a = 2.0 * M_PI * (double)i / (double)args.rays;
                    float *ray = &fan[((size_t)(w - lo) * args.rays + i) * 8u];
                    ray[0] = cam.position.x; ray[1] = cam.position.y; ray[2] = cam.position.z; ray[3] = 0.0f;
                    ray[4] = (float)std::cos(a); ray[5] = (float)std::sin(a); ray[6] = 0.0f; ray[7] = 1000.0f;
                }
            }
            if (mrx_set_rays(mrx_shard(top, (int)g), 0, hi - lo, fan.data()) != MRX_OK) {
                std::fprintf(stderr, "%s\n", mrx_last_error());
                return EXIT_FAILURE;
            }
        }
    }
    mgr.sync();

    const auto start = std::chrono::system_clock::now();
    mgr.mark(0);                   // an event on every device's stream, for the per-device lines
    for (uint32_t i = 0; i < args.numSteps; ++i)
        mgr.step();
    mgr.mark(1);
    mgr.sync();
    const auto end = std::chrono::system_clock::now();
    const double seconds = std::chrono::duration<double>(end - start).count();

    bool ok = true;
    mrx_renderer *top = (mrx_renderer *)mgr.nativeHandle();
    for (uint32_t g = 0; g < mgr.numShards(); ++g) {
        const uint32_t lo = mgr.shardFirstWorld(g), hi = mgr.shardFirstWorld(g + 1);
        mrx_renderer *sh = mrx_shard(top, (int)g);
        if (args.gpus > 1) {
            float ms = 0.0f;
            if (mrx_elapsed_ms(sh, &ms) != MRX_OK || !(ms > 0.0f))
                ms = (float)(seconds * 1000.0);
            std::printf("GPU %d: worlds [%u, %u) FPS %f\n", devices[g], lo, hi,
                        (double)args.numSteps * (double)(hi - lo) / (ms * 1e-3));
        }
        if (args.dump) {
            const bool rt = args.mode == Mode::Raycaster;
            const uint32_t resY = rt ? args.width : args.height;
            const std::string name = args.gpus == 1 ? args.outName : args.outName + ".gpu" + std::to_string(g);
            const DumpWhat what = args.dumpDepth ? DumpWhat::Depth
                                  : args.outputs == Manager::RenderOutputs::Depth ? DumpWhat::InvDepth : DumpWhat::Rgb;
            ok = dumpTiled(name, sh, hi - lo, args.width, resY, what, rt) && ok;
            if (args.normals)
                ok = dumpTiled(name + ".normals", sh, hi - lo, args.width, resY, DumpWhat::Normal, rt) && ok;
            if (args.hasLabels)
                ok = dumpTiled(name + ".labels", sh, hi - lo, args.width, resY, DumpWhat::Labels, rt) && ok;
            if (args.positions)
                ok = dumpPly(name + ".points", sh, hi - lo, args.width, resY,
                             args.outputs != Manager::RenderOutputs::Depth) && ok;
            if (args.boxes)
                ok = dumpBoxes(name, sh, hi - lo, args.boxes) && ok;
            if (args.rays)
                ok = dumpRays(name, sh, lo, hi - lo, args.rays) && ok;
            if (args.obsLayout)
                ok = dumpNpy(name, sh) && ok;
            if (args.flow)      // NAME.flow.npy: the flow tensor as it is, (views, H, W, 4) float32 in storage order
                ok = dumpNpy(name, sh, MRX_BUF_FLOW, ".flow.npy") && ok;
        }
    }
    if (!ok)
        return EXIT_FAILURE;
    // whole node: every world of the job over the time all devices took
    const double fps = (double)args.numSteps * (double)args.numWorlds / seconds;
    std::printf("FPS %f\n", fps);
    std::printf("Average total step time: %f ms\n",
                1000.0 * seconds / (double)(args.numSteps ? args.numSteps : 1));
    return 0;
}
