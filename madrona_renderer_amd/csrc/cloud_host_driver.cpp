// Sanitizer driver for the point-cloud output's host entry (cloud_host.cpp: cloud_core.hpp on the CPU).
// Built with -fsanitize=address,undefined by `python -m madrona_renderer_amd.build --cloud-driver` (g++, host only) and
// run by tests/test_cloud_cpu.py in the CPU suite as a stand-alone program -- never on the GPU box.
//
//   cloud_host_driver VIEWS NFAST NSLOW N S SEED
//
// VIEWS views of NSLOW rows of NFAST pixels, N slots, factor S.  Every array is a heap block of exactly the size the
// entry may read or write, so that a read or write past an end is a report.  Each case runs in both storage orders and
// both frames, with and without a far crop, over a sparse and a dense depth, with 1, 2, 3 and 7 parts per view, which
// must agree bit for bit; every output is checked against the definition -- count, order, slot rule --; a disagreement
// or a sanitizer report fails the run.
#include "host_driver.hpp"

int main(int argc, char **argv)
{
    if (argc != 7) {
        std::fprintf(stderr, "usage: %s VIEWS NFAST NSLOW N S SEED\n", argv[0]);
        return 2;
    }
    const uint32_t views = (uint32_t)std::atoi(argv[1]), nfast = (uint32_t)std::atoi(argv[2]);
    const uint32_t nslow = (uint32_t)std::atoi(argv[3]), N = (uint32_t)std::atoi(argv[4]);
    const uint32_t sFactor = (uint32_t)std::atoi(argv[5]);
    uint64_t s = (uint64_t)std::atoll(argv[6]);
    const size_t pxPerView = (size_t)nfast * nslow, px = pxPerView * views, slots = (size_t)views * N;

    auto camPos = block<float>(3 * (size_t)views), camRot = block<float>(4 * (size_t)views);
    auto consts = block<float>(4 * (size_t)views);
    for (size_t v = 0; v < views; ++v) {
        unit(s, &camRot[4 * v], 4);
        for (int c = 0; c < 3; ++c)
            camPos[3 * v + c] = uni(s, -20.0f, 20.0f);
        consts[4 * v] = uni(s, 0.002f, 0.2f); consts[4 * v + 1] = uni(s, -1.5f, -0.5f);
        consts[4 * v + 2] = -uni(s, 0.002f, 0.2f); consts[4 * v + 3] = uni(s, 0.5f, 1.5f);
    }

    auto depth = block<float>(px);
    auto refPoints = block<float>(4 * slots), outPoints = block<float>(4 * slots);
    auto refPixel = block<int32_t>(slots), outPixel = block<int32_t>(slots);
    auto refCount = block<int32_t>(views), outCount = block<int32_t>(views);
    uint64_t sum = 0;
    for (int dense = 0; dense < 2; ++dense) {
        for (size_t i = 0; i < px; ++i) {
            const uint64_t kind = rng(s) % 16;
            const bool hole = dense ? kind == 0 : kind < 13;
            depth[i] = hole ? 0.0f : kind == 15 ? std::nanf("") : uni(s, 0.1f, 60.0f);
        }
        for (int transposed = 0; transposed < 2; ++transposed)
            for (int frame = 1; frame <= 2; ++frame)
                for (int crop = 0; crop < 2; ++crop) {
                    const float maxDepth = crop ? 30.0f : 0.0f;
                    const uint32_t parts[4] = { 1, 2, 3, 7 };
                    for (int k = 0; k < 4; ++k) {
                        float *pts = k == 0 ? refPoints.get() : outPoints.get();
                        int32_t *pix = k == 0 ? refPixel.get() : outPixel.get();
                        int32_t *cnt = k == 0 ? refCount.get() : outCount.get();
                        std::memset(pts, 0xA5, 16 * slots);
                        std::memset(pix, 0xA5, 4 * slots);
                        std::memset(cnt, 0xA5, 4 * (size_t)views);
                        const int rc = mrx_cloud_host(depth.get(), views, nfast, nslow, transposed, sFactor, consts.get(),
                                                      frame == 1 ? camPos.get() : nullptr,
                                                      frame == 1 ? camRot.get() : nullptr, frame, maxDepth, N, parts[k],
                                                      pts, pix, cnt);
                        if (rc != MRX_OK) {
                            std::fprintf(stderr, "mrx_cloud_host returned %d\n", rc);
                            return 1;
                        }
                        if (k && (std::memcmp(refPoints.get(), outPoints.get(), 16 * slots) != 0 ||
                                  std::memcmp(refPixel.get(), outPixel.get(), 4 * slots) != 0 ||
                                  std::memcmp(refCount.get(), outCount.get(), 4 * (size_t)views) != 0)) {
                            std::fprintf(stderr, "%u parts differ from one\n", parts[k]);
                            return 1;
                        }
                    }
                    // the definition: slot k holds the valid pixel of rank floor(k * M / N) (M >= N) or k (k < M < N)
                    const uint32_t imgW = transposed ? nslow : nfast;
                    for (uint32_t v = 0; v < views; ++v) {
                        std::vector<uint32_t> valid;
                        for (size_t i = 0; i < pxPerView; ++i) {
                            const float d = depth[v * pxPerView + i];
                            if (d > 0.0f && (!crop || d <= maxDepth))
                                valid.push_back((uint32_t)i);
                        }
                        const uint64_t M = valid.size();
                        if ((uint64_t)refCount[v] != M) {
                            std::fprintf(stderr, "view %u: count %d, %llu valid pixels\n", v, refCount[v], (unsigned long long)M);
                            return 1;
                        }
                        for (uint32_t k = 0; k < N; ++k) {
                            const bool filled = M >= N || k < M;
                            int32_t want = -1;
                            if (filled) {
                                const uint32_t i = valid[(size_t)(M >= N ? (uint64_t)k * M / N : k)];
                                const uint32_t slow = i / nfast, fast = i % nfast;
                                want = (int32_t)(transposed ? fast * imgW + slow : slow * imgW + fast);
                            }
                            const float w = refPoints[4 * ((size_t)v * N + k) + 3];
                            if (refPixel[(size_t)v * N + k] != want || w != (filled ? 1.0f : 0.0f)) {
                                std::fprintf(stderr, "view %u slot %u: pixel %d, expected %d\n", v, k,
                                             refPixel[(size_t)v * N + k], want);
                                return 1;
                            }
                        }
                    }
                    for (size_t i = 0; i < 4 * slots; ++i) {
                        uint32_t bits;
                        std::memcpy(&bits, &refPoints[i], 4);
                        sum = sum * 1099511628211ull + bits;
                    }
                }
    }
    std::printf("cloud_host_driver ok: %zu pixels, %zu slots, checksum %016llx\n", px, slots, (unsigned long long)sum);
    return 0;
}
