// The point-cloud output on the CPU: cloud_core.hpp run over host arrays in the kernels' own
// structure -- every part of a view counted into a scratch column, then every part walked span by span, segment by
// segment and lane by lane with the masks, counts and bases the wave-level code forms.  Host code only -- no HIP call,
// no device -- so that tests can hold the kernels' source against tests/cloud_oracle.py without a GPU and a sanitizer
// build can run it (cloud_host_driver.cpp).
#include <cstring>
#include <vector>

#include "../../include/mrx.h"
#include "cloud.hpp"

namespace mrx {

namespace {

// the mask of segment `seg` of the view at `base` as the ballot forms it
uint64_t segMask(const float *base, const CloudParams &p, uint64_t pxPerView, uint32_t seg, uint32_t segHi)
{
    uint64_t mask = 0;
    for (uint32_t lane = 0; lane < kCloudSeg; ++lane) {
        const uint64_t i = (uint64_t)seg * kCloudSeg + lane;
        const float d = seg < segHi && i < pxPerView ? base[i] : 0.0f;
        if (cloudValid(d, p.maxDepth))
            mask |= 1ull << lane;
    }
    return mask;
}

uint32_t countRange(const float *base, const CloudParams &p, uint64_t pxPerView, uint32_t segLo, uint32_t segHi)
{
    uint32_t c = 0;
    for (uint32_t seg = segLo; seg < segHi; ++seg)
        c += (uint32_t)__builtin_popcountll(segMask(base, p, pxPerView, seg, segHi));
    return c;
}

template <bool WORLD, typename W>
void selectUnit(const CloudParams &p, uint32_t parts, uint32_t view, uint32_t part)
{
    const uint64_t pxPerView = (uint64_t)p.nfast * p.nslow;
    const uint32_t segs = (uint32_t)((pxPerView + kCloudSeg - 1u) / kCloudSeg);
    const float *base = p.depth + (size_t)view * pxPerView;
    const uint32_t segLo = cloudPartSeg(part, parts, segs), segHi = cloudPartSeg(part + 1u, parts, segs);
    const float uniform[4] = { p.sx, p.ox, p.sz, p.oz };
    const CloudView cv = cloudLoadView<WORLD>(p.camRot, p.camPos, p.viewProj, uniform, view);
    float *points = p.points + 4 * (size_t)view * p.N;
    int32_t *pixel = p.pixel + (size_t)view * p.N;
    const uint32_t imgW = p.transposed ? p.nslow : p.nfast;

    uint32_t M = 0, run = 0;
    const bool fromScan = parts == 1u && segs <= kCloudSpanSegs;
    if (parts > 1u) {
        for (uint32_t q = 0; q < parts; ++q) {
            const uint32_t c = p.scratch[(size_t)view * parts + q];
            M += c;
            if (q < part)
                run += c;
        }
    } else if (!fromScan) {
        M = countRange(base, p, pxPerView, 0u, segs);
    }
    for (uint32_t spanLo = segLo; spanLo < segHi; spanLo += kCloudSpanSegs) {
        uint64_t mask[kCloudSpanSegs];
        uint32_t excl[kCloudSpanSegs], spanTotal = 0;
        for (uint32_t i = 0; i < kCloudSpanSegs; ++i) {
            mask[i] = segMask(base, p, pxPerView, spanLo + i, segHi);
            excl[i] = spanTotal;
            spanTotal += (uint32_t)__builtin_popcountll(mask[i]);
        }
        if (fromScan)
            M = spanTotal;
        for (uint32_t i = 0; i < kCloudSpanSegs; ++i)
            for (uint32_t lane = 0; lane < kCloudSeg; ++lane) {
                if (!(mask[i] >> lane & 1u))
                    continue;
                // (mbcnt: the valid lanes below this one)
                const uint32_t rho = run + excl[i] + (uint32_t)__builtin_popcountll(mask[i] & ((1ull << lane) - 1u));
                const uint32_t slot = cloudSlot<W>(rho, M, p.N);
                if (!(slot < p.N))
                    continue;
                const uint32_t px = (spanLo + i) * kCloudSeg + lane;
                const uint32_t slow = px / p.nfast, fast = px - slow * p.nfast;
                const uint32_t x = p.transposed ? slow : fast, y = p.transposed ? fast : slow;
                cloudUnproject<WORLD>(cv, p.s, p.half, x, y, base[px], points + 4 * (size_t)slot);
                pixel[slot] = (int32_t)(y * imgW + x);
            }
        run += spanTotal;
    }
    for (uint64_t k = (uint64_t)M + (uint64_t)part * kCloudBlock; k < p.N; k += (uint64_t)parts * kCloudBlock)
        for (uint64_t t = k; t < k + kCloudBlock && t < p.N; ++t) {
            std::memset(points + 4 * t, 0, 16);
            pixel[t] = -1;
        }
    if (part == 0u)
        p.count[view] = (int32_t)M;
}

}  // namespace

void cloudHost(const CloudParams &p)
{
    const uint64_t pxPerView = (uint64_t)p.nfast * p.nslow;
    if (pxPerView * p.numViews == 0)
        return;
    const uint32_t segs = (uint32_t)((pxPerView + kCloudSeg - 1u) / kCloudSeg);
    const uint32_t parts = cloudParts(p.numViews, pxPerView, p.numCUs, p.forcedParts);
    if (parts > 1u)
        for (uint32_t view = 0; view < p.numViews; ++view)
            for (uint32_t part = 0; part < parts; ++part)
                p.scratch[(size_t)view * parts + part] =
                    countRange(p.depth + (size_t)view * pxPerView, p, pxPerView, cloudPartSeg(part, parts, segs),
                               cloudPartSeg(part + 1u, parts, segs));
    const bool world = p.frame == 1, wide = cloudWide(pxPerView, p.N);
    for (uint32_t view = 0; view < p.numViews; ++view)
        for (uint32_t part = 0; part < parts; ++part) {
            if (world)
                wide ? selectUnit<true, uint64_t>(p, parts, view, part) : selectUnit<true, uint32_t>(p, parts, view, part);
            else
                wide ? selectUnit<false, uint64_t>(p, parts, view, part) : selectUnit<false, uint32_t>(p, parts, view, part);
        }
}

}  // namespace mrx

extern "C" int mrx_cloud_host(const float *depth, uint32_t views, uint32_t nfast, uint32_t nslow, int transposed,
                              uint32_t s, const float *consts, const float *cam_pos, const float *cam_rot, int frame,
                              float max_depth, uint32_t n, uint32_t parts, float *out_points, int32_t *out_pixel,
                              int32_t *out_count)
{
    using namespace mrx;
    const uint64_t pxPerView = (uint64_t)nfast * nslow;
    // per-view constants as the device table holds them
    std::vector<ViewProj> table(views);
    if (consts)
        for (uint32_t v = 0; v < views; ++v) {
            std::memset(&table[v], 0, sizeof(ViewProj));
            std::memcpy(&table[v], consts + 4 * (size_t)v, 16);
        }
    CloudParams p {};
    p.depth = depth;
    p.points = out_points;
    p.pixel = out_pixel;
    p.count = out_count;
    p.camPos = cam_pos;
    p.camRot = cam_rot;
    p.viewProj = table.data();
    p.numViews = views;
    p.nfast = nfast;
    p.nslow = nslow;
    p.N = n;
    p.s = s;
    p.half = s / 2;
    p.frame = frame;
    p.transposed = transposed;
    p.maxDepth = max_depth;
    p.numCUs = 1;
    p.forcedParts = parts ? parts : 1u;
    std::vector<uint32_t> scratch((size_t)views * cloudParts(views, pxPerView, 1, p.forcedParts) + 1u);
    p.scratch = scratch.data();
    p.scratchCount = scratch.size();
    if (pxPerView * views == 0)
        return MRX_OK;
    if (!consts || checkCloud(p) != hipSuccess)
        return MRX_E_INVALID;
    cloudHost(p);
    return MRX_OK;
}
