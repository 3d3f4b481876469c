// Sanitizer driver for the optical-flow output's host entry (flow_host.cpp: flow_core.hpp on the CPU).
// Built with -fsanitize=address,undefined by `python -m madrona_renderer_amd.build --flow-driver` (g++, host only) and
// run by tests/test_flow_cpu.py in the CPU suite as a stand-alone program -- never on the GPU box.
//
//   flow_host_driver VIEWS NFAST NSLOW ROWS S SEED
//
// VIEWS views of NSLOW rows of NFAST pixels, one world per view of ROWS instance rows (every third one undrawn: it
// repeats its successor's base), factor S.  Every array is a heap block of exactly the size the entry may read or
// write, so that a read or write past an end is a report.  Each case runs in both storage orders, with uniform and
// with per-view constants, and with the default staging pass and passes of 1 and 3 rows, which must agree bit for bit;
// a disagreement or a sanitizer report fails the run.
#include "host_driver.hpp"

int main(int argc, char **argv)
{
    if (argc != 7) {
        std::fprintf(stderr, "usage: %s VIEWS NFAST NSLOW ROWS S SEED\n", argv[0]);
        return 2;
    }
    const uint32_t views = (uint32_t)std::atoi(argv[1]), nfast = (uint32_t)std::atoi(argv[2]);
    const uint32_t nslow = (uint32_t)std::atoi(argv[3]), rowsPerWorld = (uint32_t)std::atoi(argv[4]);
    const uint32_t sFactor = (uint32_t)std::atoi(argv[5]);
    uint64_t s = (uint64_t)std::atoll(argv[6]);
    const size_t px = (size_t)views * nfast * nslow, I = (size_t)views * rowsPerWorld;

    // the tables: one world per view; every third row is undrawn and repeats its successor's base
    auto kBase = block<uint32_t>(I);
    auto worldStart = block<uint32_t>(views + 1);
    auto viewWorld = block<uint32_t>(views);
    uint32_t worldTris = 0;
    for (uint32_t w = 0; w < views; ++w) {
        worldStart[w] = w * rowsPerWorld;
        viewWorld[w] = views - 1 - w;
        uint32_t k = 0;
        for (uint32_t r = 0; r < rowsPerWorld; ++r) {
            kBase[(size_t)w * rowsPerWorld + r] = k;
            if (r % 3 != 1)
                k += 1 + (uint32_t)(rng(s) % 12);
        }
        worldTris = k > worldTris ? k : worldTris;
    }
    worldStart[views] = views * rowsPerWorld;

    auto depth = block<float>(px);
    auto ids = block<int32_t>(px);
    for (size_t i = 0; i < px; ++i) {
        const uint64_t kind = rng(s) % 16;
        depth[i] = kind == 0 ? 0.0f : uni(s, 0.1f, 60.0f);
        ids[i] = kind == 1 ? -1 : (int32_t)(rng(s) % (worldTris + 2));      // some past the world's last triangle
    }
    std::unique_ptr<float[]> pose[2][5];
    for (int t = 0; t < 2; ++t) {
        pose[t][0] = block<float>(3 * I); pose[t][1] = block<float>(4 * I); pose[t][2] = block<float>(3 * I);
        pose[t][3] = block<float>(3 * (size_t)views); pose[t][4] = block<float>(4 * (size_t)views);
        for (size_t i = 0; i < 3 * I; ++i) {
            pose[t][0][i] = uni(s, -20.0f, 20.0f);
            pose[t][2][i] = rng(s) % 40 == 0 ? 0.0f : uni(s, 0.5f, 2.0f) * (rng(s) % 5 == 0 ? -1.0f : 1.0f);
        }
        for (size_t i = 0; i < 3 * (size_t)views; ++i)
            pose[t][3][i] = uni(s, -20.0f, 20.0f);
        for (size_t i = 0; i < I; ++i)
            unit(s, &pose[t][1][4 * i], 4);
        for (size_t v = 0; v < views; ++v)
            unit(s, &pose[t][4][4 * v], 4);
    }
    auto consts = block<float>(4 * (size_t)views), prevConsts = block<float>(4 * (size_t)views);
    for (size_t v = 0; v < views; ++v)
        for (int t = 0; t < 2; ++t) {
            float *c = (t ? prevConsts.get() : consts.get()) + 4 * v;
            c[0] = uni(s, 0.002f, 0.2f); c[1] = uni(s, -1.5f, -0.5f);
            c[2] = -uni(s, 0.002f, 0.2f); c[3] = uni(s, 0.5f, 1.5f);
        }
    const float *live[5], *prev[5];
    for (int c = 0; c < 5; ++c) {
        live[c] = pose[0][c].get();
        prev[c] = pose[1][c].get();
    }

    auto ref = block<float>(4 * px), out = block<float>(4 * px);
    uint64_t sum = 0;
    for (int transposed = 0; transposed < 2; ++transposed)
        for (int perView = 0; perView < 2; ++perView) {
            const uint32_t passes[3] = { 0, 1, 3 };
            for (int k = 0; k < 3; ++k) {
                float *dst = k == 0 ? ref.get() : out.get();
                std::memset(dst, 0xA5, 16 * px);
                const int rc = mrx_flow_host(depth.get(), ids.get(), views, nfast, nslow, transposed, sFactor,
                                             consts.get(), perView, prevConsts.get(), kBase.get(), worldStart.get(),
                                             viewWorld.get(), views, (uint32_t)I, live, prev, passes[k], dst);
                if (rc != MRX_OK) {
                    std::fprintf(stderr, "mrx_flow_host returned %d\n", rc);
                    return 1;
                }
                if (k && std::memcmp(ref.get(), out.get(), 16 * px) != 0) {
                    std::fprintf(stderr, "passes of %u rows differ from the default\n", passes[k]);
                    return 1;
                }
            }
            for (size_t i = 0; i < 4 * px; ++i) {
                uint32_t bits;
                std::memcpy(&bits, &ref[i], 4);
                sum = sum * 1099511628211ull + bits;
            }
        }
    std::printf("flow_host_driver ok: %zu pixels, %zu rows, checksum %016llx\n", px, I, (unsigned long long)sum);
    return 0;
}
