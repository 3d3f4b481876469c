// What the stand-alone sanitizer drivers share (*_host_driver.cpp, host_asan_driver.cpp): the random numbers their
// inputs are drawn from, heap blocks of exactly the size asked for -- a read or write past an end is a report -- and,
// for the drivers of the stages that trace (define HOST_DRIVER_SCENE ahead of the include: it needs assets.hpp), the
// small scene both build and the command line both take.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "../../include/mrx.h"

namespace {

uint64_t rng(uint64_t &s)
{
    s += 0x9E3779B97F4A7C15ull;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
[[maybe_unused]] float uni(uint64_t &s, float lo, float hi)
{
    return lo + (hi - lo) * (float)((rng(s) >> 40) * (1.0 / 16777216.0));
}

// a random direction: n components, unit length
[[maybe_unused]] void unit(uint64_t &s, float *q, int n)
{
    float len = 0.0f;
    for (int c = 0; c < n; ++c) {
        q[c] = uni(s, -1.0f, 1.0f);
        len += q[c] * q[c];
    }
    len = std::sqrt(len > 0.0f ? len : 1.0f);
    for (int c = 0; c < n; ++c)
        q[c] /= len;
}

template <typename T>
std::unique_ptr<T[]> block(size_t n) { return std::unique_ptr<T[]>(new T[n]); }

#ifdef HOST_DRIVER_SCENE
struct Scene {
    std::vector<float> tris;                    // [T][9]
    std::vector<int32_t> first, count;
    std::vector<mrx_instance> inst;
    std::vector<uint32_t> worldStart;
    std::vector<int32_t> labels, frame;         // (a driver that asks for them)
};

// two worlds: every object once per world under a random pose, one row hidden, one with a zero scale component;
// `labelled`: a label per row and a frame per world, too
void populate(Scene &sc, uint64_t &s, float extent, bool labelled)
{
    const uint32_t nobj = (uint32_t)sc.first.size();
    sc.worldStart.push_back(0);
    for (int w = 0; w < 2; ++w) {
        for (uint32_t o = 0; o < nobj + 2; ++o) {
            mrx_instance in {};
            for (int c = 0; c < 3; ++c) {
                in.position[c] = uni(s, -extent, extent);
                in.scale[c] = uni(s, 0.5f, 2.0f) * (rng(s) % 5 == 0 ? -1.0f : 1.0f);
            }
            unit(s, in.rotation, 4);
            in.object_id = o < nobj ? (int32_t)o : o == nobj ? -1 : (int32_t)(nobj ? nobj - 1 : 0);
            if (o == nobj + 1)
                in.scale[1] = 0.0f;
            sc.inst.push_back(in);
            if (labelled)
                sc.labels.push_back(rng(s) % 3 == 0 ? (int32_t)(rng(s) % 100) : MRX_LABEL_OBJECT);
        }
        sc.worldStart.push_back((uint32_t)sc.inst.size());
        if (labelled)
            sc.frame.push_back(w == 0 ? -1 : 0);
    }
}

// The command line of a scene driver, `assets FILE.obj... N SEED | soup NUM_TRIS N SEED KIND`: the shipped meshes, or an
// adversarial soup (KIND: 0 cloud, 1 degenerate triangles, 2 NaN and infinite vertices, 3 coincident), as the objects
// of populate's two worlds; then run(scene, N, seed, extent).
int sceneMain(int argc, char **argv, const char *usage, bool labelled,
              int (*run)(const Scene &sc, uint32_t n, uint64_t &s, float extent))
{
    if (argc >= 5 && !std::strcmp(argv[1], "assets")) {
        Scene sc;
        uint64_t s = (uint64_t)std::atoll(argv[argc - 1]);
        const uint32_t n = (uint32_t)std::atoi(argv[argc - 2]);
        for (int i = 2; i < argc - 2; ++i) {
            mrx::TriSoup soup;
            std::string err;
            if (!mrx::loadOBJ(argv[i], soup, err)) {
                std::fprintf(stderr, "%s: %s\n", argv[i], err.c_str());
                return 2;
            }
            sc.first.push_back((int32_t)(sc.tris.size() / 9));
            sc.count.push_back((int32_t)soup.numTris());
            sc.tris.insert(sc.tris.end(), soup.pos.begin(), soup.pos.begin() + 9 * (size_t)soup.numTris());
        }
        populate(sc, s, 4.0f, labelled);
        return run(sc, n, s, 4.0f);
    }
    if (argc == 6 && !std::strcmp(argv[1], "soup")) {
        const uint32_t T = (uint32_t)std::atoi(argv[2]), n = (uint32_t)std::atoi(argv[3]);
        uint64_t s = (uint64_t)std::atoll(argv[4]);
        const int kind = std::atoi(argv[5]);
        Scene sc;
        // three objects: a large one (BLAS), a flat one, an empty one
        const uint32_t sizes[3] = { T, T < 20 ? T : 20, 0 };
        for (uint32_t o = 0; o < 3; ++o) {
            sc.first.push_back((int32_t)(sc.tris.size() / 9));
            sc.count.push_back((int32_t)sizes[o]);
            for (uint32_t t = 0; t < sizes[o]; ++t) {
                float v[9];
                const float cx = uni(s, -3.0f, 3.0f), cy = uni(s, -3.0f, 3.0f), cz = uni(s, -3.0f, 3.0f);
                for (int c = 0; c < 9; ++c)
                    v[c] = (c % 3 == 0 ? cx : c % 3 == 1 ? cy : cz) + uni(s, -0.4f, 0.4f);
                if (kind == 1 && t % 3 == 0)
                    std::memcpy(v + 6, v + 3, 12);                      // two vertices coincide
                if (kind == 1 && t % 3 == 1)
                    for (int c = 0; c < 3; ++c)
                        v[6 + c] = v[c] + 2.0f * (v[3 + c] - v[c]);     // collinear
                if (kind == 2 && t % 5 == 0)
                    v[rng(s) % 9] = rng(s) % 2 ? std::numeric_limits<float>::quiet_NaN()
                                               : std::numeric_limits<float>::infinity();
                if (kind == 3 && t > 0 && t % 2 == 1)
                    std::memcpy(v, &sc.tris[sc.tris.size() - 9], 36);   // the triangle before, again: exact t ties
                sc.tris.insert(sc.tris.end(), v, v + 9);
            }
        }
        populate(sc, s, 3.0f, labelled);
        return run(sc, n, s, 6.0f);
    }
    std::fprintf(stderr, "usage: %s\n", usage);
    return 2;
}
#endif

}  // namespace
