// Sanitizer driver for the ray-cast sensor's host entry (rays_host.cpp: rays_core.hpp on the CPU over the BLAS builder,
// DESIGN.md 4.22).  Built with -fsanitize=address,undefined by `python -m madrona_renderer_amd.build --rays-driver` (g++,
// host only) and run by tests/test_ray_cpu.py in the CPU suite -- never on the GPU box.
//
//   rays_host_driver assets FILE.obj... RAYS SEED    the shipped meshes as objects of two worlds, RAYS random rays each
//   rays_host_driver soup NUM_TRIS RAYS SEED KIND    an adversarial soup (KIND: 0 cloud, 1 degenerate triangles, 2 NaN
//                                                    and infinite vertices, 3 coincident), culled and brute
// The culled and the brute form must agree bit for bit; a disagreement or a sanitizer report fails the run.
#include "assets.hpp"
#define HOST_DRIVER_SCENE
#include "host_driver.hpp"

namespace {

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
    return sceneMain(argc, argv, "rays_host_driver assets FILE.obj... RAYS SEED | soup NUM_TRIS RAYS SEED KIND", true, run);
}
