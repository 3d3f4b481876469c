// Sanitizer driver for the shadow stage's host entry (shadow_host.cpp: shadow_core.hpp on the CPU over the host scene of
// rays_host.cpp and the BLAS builder).  Built with -fsanitize=address,undefined by `python -m
// madrona_renderer_amd.build --shadow-driver` (g++, host only) and run by tests/test_shadow_cpu.py in the CPU suite --
// never on the GPU box.
//
//   shadow_host_driver assets FILE.obj... SIDE SEED    the shipped meshes as objects of two worlds, two views of
//                                                      SIDE x (SIDE + 3) pixels each
//   shadow_host_driver soup NUM_TRIS SIDE SEED KIND    an adversarial soup (KIND: 0 cloud, 1 degenerate triangles, 2 NaN
//                                                      and infinite vertices, 3 coincident)
// Depths are random, with NaN, negative, zero and infinite ones among them; one view's light direction is zero.  The
// culled and the brute form, one pass and passes of one row, must agree on every byte of the mask and of the darkened
// rgb; a disagreement or a sanitizer report fails the run.
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

void unit(uint64_t &s, float *q, int n)
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

struct Scene {
    std::vector<float> tris;                    // [T][9]
    std::vector<int32_t> first, count;
    std::vector<mrx_instance> inst;
    std::vector<uint32_t> worldStart;
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
            unit(s, in.rotation, 4);
            in.object_id = o < nobj ? (int32_t)o : o == nobj ? -1 : (int32_t)(nobj ? nobj - 1 : 0);
            if (o == nobj + 1)
                in.scale[1] = 0.0f;
            sc.inst.push_back(in);
        }
        sc.worldStart.push_back((uint32_t)sc.inst.size());
    }
}

int run(const Scene &sc, uint32_t side, uint64_t &s, float extent)
{
    const uint32_t views = 4, nfast = side, nslow = side + 3;
    const size_t px = (size_t)views * nfast * nslow;
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    std::vector<float> depth(px), consts(4 * views), camPos(3 * views), camRot(4 * views), lights(5 * views);
    std::vector<uint32_t> viewWorld(views), rgb0(px), normal(px);
    for (uint32_t v = 0; v < views; ++v) {
        viewWorld[v] = v / 2;
        consts[4 * v] = 2.0f / (float)nfast; consts[4 * v + 1] = 1.0f / (float)nfast - 1.0f;
        consts[4 * v + 2] = -2.0f / (float)nslow; consts[4 * v + 3] = 1.0f - 1.0f / (float)nslow;
        for (int c = 0; c < 3; ++c)
            camPos[3 * v + c] = uni(s, -2.0f * extent, 2.0f * extent);
        unit(s, &camRot[4 * v], 4);
        unit(s, &lights[5 * v], 3);
        if (v == 3)
            lights[5 * v] = lights[5 * v + 1] = lights[5 * v + 2] = 0.0f;
        lights[5 * v + 3] = v == 1 ? 0.0f : 0.25f;
        lights[5 * v + 4] = 0.75f;
    }
    for (size_t i = 0; i < px; ++i) {
        const uint64_t k = rng(s) % 64;
        depth[i] = k == 0 ? nan : k == 1 ? -1.0f : k == 2 ? inf : k == 3 ? -inf : k < 8 ? 0.0f : uni(s, 0.01f, 3.0f * extent);
        rgb0[i] = (uint32_t)rng(s);
        normal[i] = (uint32_t)rng(s) | 0xFF000000u;
    }
    const uint32_t numTris = (uint32_t)(sc.tris.size() / 9), worlds = (uint32_t)sc.worldStart.size() - 1u;
    std::vector<uint8_t> mask[4];
    std::vector<uint32_t> rgb[4];
    for (int form = 0; form < 4; ++form) {
        mask[form].assign(px, 7);
        rgb[form] = rgb0;
        const int rc = mrx_shadow_host(sc.tris.data(), numTris, sc.first.data(), sc.count.data(), (uint32_t)sc.first.size(),
                                       sc.inst.data(), (uint32_t)sc.inst.size(), sc.worldStart.data(), worlds, depth.data(),
                                       views, nfast, nslow, form & 2 ? 1 : 0, 1, consts.data(), camPos.data(), camRot.data(),
                                       viewWorld.data(), lights.data(), MRX_SHADOW_DEFAULT_BIAS,
                                       form & 2 ? 4.0f * extent : MRX_SHADOW_NO_MAX_DISTANCE, form & 2 ? 1u : 0u, form & 1,
                                       rgb[form].data(), normal.data(), mask[form].data());
        if (rc != MRX_OK) {
            std::fprintf(stderr, "mrx_shadow_host: %d\n", rc);
            return 2;
        }
    }
    // forms 0 / 1 and forms 2 / 3 differ in the cull alone
    size_t occluded = 0, bad = 0;
    for (size_t i = 0; i < px; ++i) {
        occluded += mask[0][i] == 0;
        bad += mask[0][i] != mask[1][i] || mask[2][i] != mask[3][i] || rgb[0][i] != rgb[1][i] || rgb[2][i] != rgb[3][i];
        bad += (mask[0][i] != 0 && mask[0][i] != 255) || (mask[0][i] == 255 && rgb[0][i] != rgb0[i]);
        bad += !(depth[i] > 0.0f) && mask[0][i] != 255;
    }
    std::printf("pixels %zu occluded %zu mismatches %zu\n", px, occluded, bad);
    return bad ? 1 : 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc >= 5 && !std::strcmp(argv[1], "assets")) {
        Scene sc;
        uint64_t s = (uint64_t)std::atoll(argv[argc - 1]);
        const uint32_t side = (uint32_t)std::atoi(argv[argc - 2]);
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
        return run(sc, side, s, 4.0f);
    }
    if (argc == 6 && !std::strcmp(argv[1], "soup")) {
        const uint32_t T = (uint32_t)std::atoi(argv[2]), side = (uint32_t)std::atoi(argv[3]);
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
                    std::memcpy(v, &sc.tris[sc.tris.size() - 9], 36);   // the triangle before, again
                sc.tris.insert(sc.tris.end(), v, v + 9);
            }
        }
        populate(sc, s, 3.0f);
        return run(sc, side, s, 6.0f);
    }
    std::fprintf(stderr, "usage: shadow_host_driver assets FILE.obj... SIDE SEED | soup NUM_TRIS SIDE SEED KIND\n");
    return 2;
}
