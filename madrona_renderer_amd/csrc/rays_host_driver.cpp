// Sanitizer driver for the ray-cast sensor's host entry (rays_host.cpp: rays_core.hpp on the CPU over the BLAS builder,
// DESIGN.md 4.22).  Built with -fsanitize=address,undefined by `python -m madrona_renderer_amd.build --rays-driver` (g++,
// host only) and run by tests/test_ray_cpu.py in the CPU suite -- never on the GPU box.
//
//   rays_host_driver assets FILE.obj... RAYS SEED    the shipped meshes as objects of two worlds, RAYS random rays each
//   rays_host_driver soup NUM_TRIS RAYS SEED KIND    an adversarial soup (KIND: 0 cloud, 1 degenerate triangles, 2 NaN
//                                                    and infinite vertices, 3 coincident), culled and brute
// The culled and the brute form must agree bit for bit; a disagreement or a sanitizer report fails the run.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/mrx.h"
#include "assets.hpp"

namespace {

uint64_t rng(uint64_t &s)
{
    s += 0x9E3779B97F4A7C15ull;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
float uni(uint64_t &s, float lo, float hi) { return lo + (hi - lo) * (float)((rng(s) >> 40) * (1.0 / 16777216.0)); }

struct Scene {
    std::vector<float> tris;                    // [T][9]
    std::vector<int32_t> first, count;
    std::vector<mrx_instance> inst;
    std::vector<int32_t> labels;
    std::vector<uint32_t> worldStart;
    std::vector<int32_t> frame;
};

// two worlds: every object once per world under a random pose, one row hidden, one with a zero scale component
void populate(Scene &sc, uint64_t &s, float extent)
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
            float n = 0.0f;
            for (int c = 0; c < 4; ++c) {
                in.rotation[c] = uni(s, -1.0f, 1.0f);
                n += in.rotation[c] * in.rotation[c];
            }
            n = std::sqrt(n > 0.0f ? n : 1.0f);
            for (int c = 0; c < 4; ++c)
                in.rotation[c] /= n;
            in.object_id = o < nobj ? (int32_t)o : o == nobj ? -1 : (int32_t)(nobj ? nobj - 1 : 0);
            if (o == nobj + 1)
                in.scale[1] = 0.0f;
            sc.inst.push_back(in);
            sc.labels.push_back(rng(s) % 3 == 0 ? (int32_t)(rng(s) % 100) : MRX_LABEL_OBJECT);
        }
        sc.worldStart.push_back((uint32_t)sc.inst.size());
        sc.frame.push_back(w == 0 ? -1 : 0);
    }
}

int run(const Scene &sc, uint32_t R, uint64_t &s, float extent)
{
    const uint32_t worlds = (uint32_t)sc.worldStart.size() - 1u;
    std::vector<float> rays((size_t)worlds * R * 8u);
    for (size_t i = 0; i < (size_t)worlds * R; ++i) {
        float *r = &rays[8 * i];
        for (int c = 0; c < 3; ++c) {
            r[c] = uni(s, -2.0f * extent, 2.0f * extent);
            r[4 + c] = rng(s) % 7 == 0 ? 0.0f : uni(s, -1.0f, 1.0f);
        }
        r[3] = 0.0f;
        r[7] = rng(s) % 4 == 0 ? std::numeric_limits<float>::infinity() : 8.0f * extent;
        if (rng(s) % 97 == 0)
            r[rng(s) % 8] = std::numeric_limits<float>::quiet_NaN();
    }
    const size_t n = (size_t)worlds * R;
    std::vector<float> t0(n), t1(n);
    std::vector<int32_t> id0(n), id1(n);
    const uint32_t numTris = (uint32_t)(sc.tris.size() / 9);
    for (int brute = 0; brute < 2; ++brute) {
        const int rc = mrx_trace_rays_host(sc.tris.data(), numTris, sc.first.data(), sc.count.data(),
                                           (uint32_t)sc.first.size(), sc.inst.data(), (uint32_t)sc.inst.size(),
                                           sc.labels.data(), sc.worldStart.data(), worlds, sc.frame.data(), rays.data(), R,
                                           brute, brute ? t1.data() : t0.data(), brute ? id1.data() : id0.data());
        if (rc != MRX_OK) {
            std::fprintf(stderr, "mrx_trace_rays_host: %d\n", rc);
            return 2;
        }
    }
    size_t hits = 0, bad = 0;
    for (size_t i = 0; i < n; ++i) {
        hits += id0[i] != -1 || t0[i] != rays[8 * i + 7];
        const bool same = std::memcmp(&t0[i], &t1[i], 4) == 0 || (std::isnan(t0[i]) && std::isnan(t1[i]));
        bad += !same || id0[i] != id1[i];
    }
    std::printf("rays %zu hits %zu mismatches %zu\n", n, hits, bad);
    return bad ? 1 : 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc >= 5 && !std::strcmp(argv[1], "assets")) {
        Scene sc;
        uint64_t s = (uint64_t)std::atoll(argv[argc - 1]);
        const uint32_t R = (uint32_t)std::atoi(argv[argc - 2]);
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
        populate(sc, s, 4.0f);
        return run(sc, R, s, 4.0f);
    }
    if (argc == 6 && !std::strcmp(argv[1], "soup")) {
        const uint32_t T = (uint32_t)std::atoi(argv[2]), R = (uint32_t)std::atoi(argv[3]);
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
        populate(sc, s, 3.0f);
        return run(sc, R, s, 6.0f);
    }
    std::fprintf(stderr, "usage: rays_host_driver assets FILE.obj... RAYS SEED | soup NUM_TRIS RAYS SEED KIND\n");
    return 2;
}
