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
#include "assets.hpp"
#define HOST_DRIVER_SCENE
#include "host_driver.hpp"

namespace {

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
    return sceneMain(argc, argv, "shadow_host_driver assets FILE.obj... SIDE SEED | soup NUM_TRIS SIDE SEED KIND", false, run);
}
