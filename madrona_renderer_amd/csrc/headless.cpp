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
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/madrona_mi355/manager.hpp"
#include "../../include/mrx.h"
#include "assets.hpp"

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

// a number of the whole argument, finite
float parseFloat(const char *flag, const char *s)
{
    char *end = nullptr;
    const float v = std::strtof(s, &end);
    if (!*s || *end || !std::isfinite(v)) {
        std::fprintf(stderr, "%s: not a number: %s\n", flag, s);
        std::exit(EXIT_FAILURE);
    }
    return v;
}

[[noreturn]] void usage(const char *argv0)
{
    std::fprintf(stderr,
                 "%s [NUM_WORLDS] [NUM_STEPS] [rt|rast] [BATCH_WIDTH] [BATCH_HEIGHT] "
                 "[--dump-last-frame file_name_without_extension] [--scene synthetic|demo] [--depth] [--gpus N] [--outputs rgbd|depth|rgb] [--vfov DEG] [--znear Z] [--light X,Y,Z[,AMBIENT,DIFFUSE]] [--instance-colors SEED] [--instance-materials SEED] [--normals] [--instance-labels SEED] [--supersample N] [--positions [world|view]] [--boxes K] [--rays R] [--flow] [--observations CHANNELS[,DTYPE[,STACK]]] [--obs-depth-range LO,HI]\n",
                 argv0);
    std::exit(EXIT_FAILURE);
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
        if (!std::strcmp(argv[i], "--dump-last-frame") && i + 1 < argc) {
            a.dump = true;
            a.outName = argv[++i];
        } else if (!std::strcmp(argv[i], "--scene") && i + 1 < argc) {
            a.demo = !std::strcmp(argv[++i], "demo");
        } else if (!std::strcmp(argv[i], "--depth")) {
            a.dumpDepth = true;
        } else if (!std::strcmp(argv[i], "--normals")) {
            a.normals = true;
        } else if (!std::strcmp(argv[i], "--gpus") && i + 1 < argc) {
            a.gpus = (uint32_t)std::atoi(argv[++i]);
        } else if (!std::strcmp(argv[i], "--vfov") && i + 1 < argc) {
            a.vfov = parseFloat("--vfov", argv[++i]);
            if (!(a.vfov > 0.0f && a.vfov < 180.0f)) {
                std::fprintf(stderr, "--vfov: %s is not in (0, 180) degrees\n", argv[i]);
                std::exit(EXIT_FAILURE);
            }
        } else if (!std::strcmp(argv[i], "--light") && i + 1 < argc) {
            // three or five numbers; the library's own check decides (mrx_light_constants needs no device)
            std::vector<std::string> fields(1);
            for (const char *ch = argv[++i]; *ch; ++ch) {
                if (*ch == ',')
                    fields.emplace_back();
                else
                    fields.back() += *ch;
            }
            const int n = (int)fields.size();
            float v[5] = { 0.0f, 0.0f, 0.0f, a.light.ambient, a.light.diffuse };
            for (int k = 0; k < n && k < 5; ++k)
                v[k] = parseFloat("--light", fields[(size_t)k].c_str());
            float c[5];
            const mrx_light l = { { v[0], v[1], v[2] }, v[3], v[4] };
            if (n != 3 && n != 5) {
                std::fprintf(stderr, "--light: wants X,Y,Z or X,Y,Z,AMBIENT,DIFFUSE, got %s\n", argv[i]);
                std::exit(EXIT_FAILURE);
            }
            if (mrx_light_constants(l, c) != MRX_OK) {
                std::fprintf(stderr, "--light: %s\n", mrx_last_error());
                std::exit(EXIT_FAILURE);
            }
            a.light = { { v[0], v[1], v[2] }, v[3], v[4] };
            a.hasLight = true;
        } else if (!std::strcmp(argv[i], "--instance-colors") && i + 1 < argc) {
            const char *s = argv[++i];
            char *end = nullptr;
            errno = 0;
            a.colorSeed = std::strtoull(s, &end, 0);
            if (!*s || *s == '-' || *s == '+' || *end || errno != 0) {
                std::fprintf(stderr, "--instance-colors: not an unsigned integer seed: %s\n", s);
                std::exit(EXIT_FAILURE);
            }
            a.hasColors = true;
        } else if (!std::strcmp(argv[i], "--instance-materials") && i + 1 < argc) {
            const char *s = argv[++i];
            char *end = nullptr;
            errno = 0;
            a.materialSeed = std::strtoull(s, &end, 0);
            if (!*s || *s == '-' || *s == '+' || *end || errno != 0) {
                std::fprintf(stderr, "--instance-materials: not an unsigned integer seed: %s\n", s);
                std::exit(EXIT_FAILURE);
            }
            a.hasMaterials = true;
        } else if (!std::strcmp(argv[i], "--instance-labels") && i + 1 < argc) {
            const char *s = argv[++i];
            char *end = nullptr;
            errno = 0;
            a.labelSeed = std::strtoull(s, &end, 0);
            if (!*s || *s == '-' || *s == '+' || *end || errno != 0) {
                std::fprintf(stderr, "--instance-labels: not an unsigned integer seed: %s\n", s);
                std::exit(EXIT_FAILURE);
            }
            a.hasLabels = true;
        } else if (!std::strcmp(argv[i], "--supersample") && i + 1 < argc) {
            const char *s = argv[++i];
            char *end = nullptr;
            errno = 0;
            const unsigned long long v = std::strtoull(s, &end, 10);
            if (!*s || *s == '-' || *s == '+' || *end || errno != 0 || v < 1 || v > 4) {
                std::fprintf(stderr, "--supersample: not a factor from 1 to 4: %s\n", s);
                std::exit(EXIT_FAILURE);
            }
            a.supersample = (uint32_t)v;
        } else if (!std::strcmp(argv[i], "--boxes") && i + 1 < argc) {
            const char *s = argv[++i];
            char *end = nullptr;
            errno = 0;
            const unsigned long long v = std::strtoull(s, &end, 10);
            if (!*s || *s == '-' || *s == '+' || *end || errno != 0 || v < 1 || v > 1024) {
                std::fprintf(stderr, "--boxes: not a number of labels from 1 to 1024: %s\n", s);
                std::exit(EXIT_FAILURE);
            }
            a.boxes = (uint32_t)v;
        } else if (!std::strcmp(argv[i], "--rays") && i + 1 < argc) {
            const char *s = argv[++i];
            char *end = nullptr;
            errno = 0;
            const unsigned long long v = std::strtoull(s, &end, 10);
            if (!*s || *s == '-' || *s == '+' || *end || errno != 0 || v < 1 || v > 65536) {
                std::fprintf(stderr, "--rays: not a number of rays per world from 1 to 65536: %s\n", s);
                std::exit(EXIT_FAILURE);
            }
            a.rays = (uint32_t)v;
        } else if (!std::strcmp(argv[i], "--flow")) {
            a.flow = true;
        } else if (!std::strcmp(argv[i], "--observations") && i + 1 < argc) {
            static const char *const layouts[] = { "", "rgb", "rgbd", "d", "y", "yd" };
            static const char *const dtypes[] = { "float32", "float16", "bfloat16", "uint8" };
            const char *v = argv[++i];
            const std::vector<std::string> f = splitCommas(v);
            uint32_t layout = 0, dtype = f.size() > 1 ? 4u : 0u, stack = 1;
            for (uint32_t k = 1; k <= 5; ++k)
                if (f[0] == layouts[k])
                    layout = k;
            for (uint32_t k = 0; f.size() > 1 && k < 4; ++k)
                if (f[1] == dtypes[k])
                    dtype = k;
            if (f.size() > 2) {
                const char *t = f[2].c_str();
                stack = t[0] >= '1' && t[0] <= '8' && !t[1] ? (uint32_t)(t[0] - '0') : 0u;
            }
            if (!layout || dtype == 4 || !stack || f.size() > 3) {
                std::fprintf(stderr, "--observations: wants CHANNELS[,DTYPE[,STACK]] -- rgb|rgbd|d|y|yd, "
                                     "float32|float16|bfloat16|uint8, 1 ... 8 -- got: %s\n", v);
                std::exit(EXIT_FAILURE);
            }
            a.obsLayout = layout; a.obsDtype = dtype; a.obsStack = stack;
        } else if (!std::strcmp(argv[i], "--obs-depth-range") && i + 1 < argc) {
            const char *v = argv[++i];
            const std::vector<std::string> f = splitCommas(v);
            if (f.size() != 2) {
                std::fprintf(stderr, "--obs-depth-range: wants LO,HI, got: %s\n", v);
                std::exit(EXIT_FAILURE);
            }
            a.obsLo = parseFloat("--obs-depth-range", f[0].c_str());
            a.obsHi = parseFloat("--obs-depth-range", f[1].c_str());
            if (!(a.obsLo >= 0.0f && a.obsLo < a.obsHi)) {
                std::fprintf(stderr, "--obs-depth-range: wants 0 <= LO < HI, got: %s\n", v);
                std::exit(EXIT_FAILURE);
            }
            a.hasObsRange = true;
        } else if (!std::strcmp(argv[i], "--positions")) {
            // the frame is optional: the next argument is taken for it unless it is another option
            a.positions = 1;
            if (i + 1 < argc && std::strncmp(argv[i + 1], "--", 2) != 0) {
                const char *f = argv[++i];
                if (!std::strcmp(f, "view"))
                    a.positions = 2;
                else if (std::strcmp(f, "world") != 0) {
                    std::fprintf(stderr, "--positions: the frame is world or view, not: %s\n", f);
                    std::exit(EXIT_FAILURE);
                }
            }
        } else if (!std::strcmp(argv[i], "--znear") && i + 1 < argc) {
            a.znear = parseFloat("--znear", argv[++i]);
            if (!(a.znear > 0.0f)) {
                std::fprintf(stderr, "--znear: %s is not > 0\n", argv[i]);
                std::exit(EXIT_FAILURE);
            }
        } else if (!std::strcmp(argv[i], "--outputs") && i + 1 < argc) {
            const char *o = argv[++i];
            if (!std::strcmp(o, "rgbd")) a.outputs = Manager::RenderOutputs::RGBD;
            else if (!std::strcmp(o, "depth")) a.outputs = Manager::RenderOutputs::Depth;
            else if (!std::strcmp(o, "rgb")) a.outputs = Manager::RenderOutputs::RGB;
            else usage(argv[0]);
        } else {
            usage(argv[0]);
        }
    }
    if (a.numWorlds == 0 || a.width == 0 || a.height == 0 || a.gpus == 0 || a.gpus > a.numWorlds)
        usage(argv[0]);
    if ((uint64_t)a.supersample * a.width > 16384 || (uint64_t)a.supersample * a.height > 16384) {
        std::fprintf(stderr, "--supersample: %u times %u x %u is more than 16384 pixels a side\n", a.supersample, a.width,
                     a.height);
        std::exit(EXIT_FAILURE);
    }
    if (a.mode == Mode::Raycaster && !(a.znear < 1000.0f)) {
        std::fprintf(stderr, "--znear: must be below the Raytracer far plane (1000)\n");
        std::exit(EXIT_FAILURE);
    }
    if (a.dumpDepth && a.outputs == Manager::RenderOutputs::RGB) {
        std::fprintf(stderr, "--depth: depth is not rendered with --outputs rgb\n");
        std::exit(EXIT_FAILURE);
    }
    if (a.positions && a.outputs == Manager::RenderOutputs::RGB) {
        std::fprintf(stderr, "--positions: positions are computed from depth, which is not rendered with --outputs rgb\n");
        std::exit(EXIT_FAILURE);
    }
    if (a.flow && a.outputs == Manager::RenderOutputs::RGB) {
        std::fprintf(stderr, "--flow: the flow is computed from depth, which is not rendered with --outputs rgb\n");
        std::exit(EXIT_FAILURE);
    }
    if (a.flow && (a.boxes || a.hasLabels)) {
        std::fprintf(stderr, "--flow: the ids tensor holds visibility ids, so there is no segmask for --boxes or --instance-labels\n");
        std::exit(EXIT_FAILURE);
    }
    if (a.boxes && a.mode == Mode::Rasterizer && !a.hasLabels) {
        std::fprintf(stderr, "--boxes: boxes are computed from the segmask, which rast has only with --instance-labels\n");
        std::exit(EXIT_FAILURE);
    }
    {
        const bool colour = a.obsLayout && a.obsLayout != MRX_OBS_D;
        const bool depth = a.obsLayout == MRX_OBS_RGBD || a.obsLayout == MRX_OBS_D || a.obsLayout == MRX_OBS_YD;
        if (colour && a.outputs == Manager::RenderOutputs::Depth) {
            std::fprintf(stderr, "--observations: these channels need rgb, which is not rendered with --outputs depth\n");
            std::exit(EXIT_FAILURE);
        }
        if (depth && a.outputs == Manager::RenderOutputs::RGB) {
            std::fprintf(stderr, "--observations: these channels need depth, which is not rendered with --outputs rgb\n");
            std::exit(EXIT_FAILURE);
        }
        if (a.hasObsRange && !depth) {
            std::fprintf(stderr, "--obs-depth-range: needs --observations with a depth channel (rgbd, d or yd)\n");
            std::exit(EXIT_FAILURE);
        }
    }
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
bool dumpTiled(const std::string &name, mrx_renderer *shard, uint32_t numImages, uint32_t resX,
               uint32_t resY, DumpWhat what, bool transpose)
{
    const bool depth = what != DumpWhat::Rgb && what != DumpWhat::Normal && what != DumpWhat::Labels;
    const size_t bytesPerImage = (size_t)4 * resX * resY;
    std::vector<uint8_t> host(bytesPerImage * numImages);
    if (mrx_copy_to_host(shard, depth ? MRX_BUF_DEPTH : what == DumpWhat::Normal ? MRX_BUF_NORMAL
                                : what == DumpWhat::Labels ? MRX_BUF_SEGMASK : MRX_BUF_RGB,
                         host.data(), host.size()) != MRX_OK) {
        std::fprintf(stderr, "%s\n", mrx_last_error());
        return false;
    }
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
        (withRgb && mrx_copy_to_host(shard, MRX_BUF_RGB, rgb.data(), rgb.size()) != MRX_OK)) {
        std::fprintf(stderr, "%s\n", mrx_last_error());
        return false;
    }
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
    FILE *f = std::fopen((name + ".ply").c_str(), "wb");
    const bool ok = f && std::fwrite(out.data(), 1, out.size(), f) == out.size();
    if (f && std::fclose(f) != 0)
        return false;
    if (!ok)
        std::fprintf(stderr, "cannot write %s.ply\n", name.c_str());
    return ok;
}

// NAME.boxes.txt of --boxes: one line `view label xmin ymin xmax ymax count` per non-empty row of the box tensor of
// the first `numImages` views, in the tensor's order
bool dumpBoxes(const std::string &name, mrx_renderer *shard, uint32_t numImages, uint32_t K)
{
    std::vector<int32_t> rows((size_t)numImages * K * 5);
    if (mrx_copy_to_host(shard, MRX_BUF_BOXES, rows.data(), rows.size() * sizeof(int32_t)) != MRX_OK) {
        std::fprintf(stderr, "%s\n", mrx_last_error());
        return false;
    }
    FILE *f = std::fopen((name + ".boxes.txt").c_str(), "w");
    bool ok = f != nullptr;
    for (size_t i = 0; ok && i < (size_t)numImages * K; ++i) {
        const int32_t *b = &rows[5 * i];
        if (b[4] > 0)
            ok = std::fprintf(f, "%zu %zu %d %d %d %d %d\n", i / K, i % K, b[0], b[1], b[2], b[3], b[4]) > 0;
    }
    if (f && std::fclose(f) != 0)
        ok = false;
    if (!ok)
        std::fprintf(stderr, "cannot write %s.boxes.txt\n", name.c_str());
    return ok;
}

// NAME.rays.txt of --rays: one line `world ray t id` per ray of the shard's worlds (world numbers are the job's), t with
// nine significant digits
bool dumpRays(const std::string &name, mrx_renderer *shard, uint32_t firstWorld, uint32_t numWorlds, uint32_t R)
{
    std::vector<float> t((size_t)numWorlds * R);
    std::vector<int32_t> id((size_t)numWorlds * R);
    if (mrx_copy_to_host(shard, MRX_BUF_RAY_DISTANCE, t.data(), t.size() * sizeof(float)) != MRX_OK ||
        mrx_copy_to_host(shard, MRX_BUF_RAY_ID, id.data(), id.size() * sizeof(int32_t)) != MRX_OK) {
        std::fprintf(stderr, "%s\n", mrx_last_error());
        return false;
    }
    FILE *f = std::fopen((name + ".rays.txt").c_str(), "w");
    bool ok = f != nullptr;
    for (size_t i = 0; ok && i < t.size(); ++i)
        ok = std::fprintf(f, "%zu %zu %.9g %d\n", firstWorld + i / R, i % R, (double)t[i], id[i]) > 0;
    if (f && std::fclose(f) != 0)
        ok = false;
    if (!ok)
        std::fprintf(stderr, "cannot write %s.rays.txt\n", name.c_str());
    return ok;
}

// A four-dimensional tensor of the shard as a NumPy file (format 1.0), NAME + suffix, in the tensor's own shape and
// order.  NAME.obs.npy of --observations: the observation tensor, (views, S * C, H, W); bfloat16 has no NumPy type and
// goes out as <u2, the bit patterns.  NAME.flow.npy of --flow: the flow tensor, (views, H, W, 4) <f4.
bool dumpNpy(const std::string &name, mrx_renderer *shard, int which = MRX_BUF_OBSERVATION, const char *suffix = ".obs.npy")
{
    int64_t dims[4] = { 0, 0, 0, 0 };
    int nd = 0, dt = 0, dev = 0;
    if (!mrx_buffer(shard, which, dims, &nd, &dt, &dev) || nd != 4) {
        std::fprintf(stderr, "%s\n", mrx_last_error());
        return false;
    }
    const char *descr = dt == MRX_DTYPE_F32 ? "<f4" : dt == MRX_DTYPE_F16 ? "<f2" : dt == MRX_DTYPE_BF16 ? "<u2" : "|u1";
    const size_t elem = dt == MRX_DTYPE_F32 ? 4 : dt == MRX_DTYPE_U8 ? 1 : 2;
    std::vector<uint8_t> data((size_t)(dims[0] * dims[1] * dims[2] * dims[3]) * elem);
    if (mrx_copy_to_host(shard, which, data.data(), data.size()) != MRX_OK) {
        std::fprintf(stderr, "%s\n", mrx_last_error());
        return false;
    }
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
    FILE *f = std::fopen((name + suffix).c_str(), "wb");
    const bool ok = f && std::fwrite(out.data(), 1, out.size(), f) == out.size() &&
                    std::fwrite(data.data(), 1, data.size(), f) == data.size();
    if (f && std::fclose(f) != 0)
        return false;
    if (!ok)
        std::fprintf(stderr, "cannot write %s%s\n", name.c_str(), suffix);
    return ok;
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
