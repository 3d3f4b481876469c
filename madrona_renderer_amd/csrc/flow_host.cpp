// The optical-flow output on the CPU: flow_core.hpp run pixel by pixel over host arrays, in the
// kernel's own structure -- a view's world staged in passes, a pixel computed in the pass that holds its row.  Host code
// only -- no HIP call, no device -- so that tests can hold the kernel's source against tests/flow_oracle.py without a
// GPU and a sanitizer build can run it (flow_host_driver.cpp).
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/mrx.h"
#include "flow.hpp"

namespace mrx {

void flowHost(const FlowParams &p)
{
    const uint32_t pxPerView = p.nfast * p.nslow;
    const uint32_t passRows = p.passRows ? std::min(p.passRows, kFlowPassRows) : kFlowPassRows;
    const float uniform[4] = { p.sx, p.ox, p.sz, p.oz };
    std::vector<FlowRow> rows(passRows);
    std::vector<uint8_t> pending(pxPerView);
    for (uint32_t view = 0; view < p.numViews; ++view) {
        const size_t first = (size_t)view * pxPerView;
        FlowView fv;
        flowLoadView(view, p.live, p.prev, p.viewProj, uniform, p.prevProj, fv);
        const uint32_t world = p.viewWorld[view];
        const uint32_t rowLo = p.worldInstStart[world], rowHi = p.worldInstStart[world + 1];
        for (uint32_t i = 0; i < pxPerView; ++i) {
            const float d = p.depth[first + i];
            pending[i] = !(d == 0.0f) && p.ids[first + i] >= 0;
            std::memset(p.flow + 4 * (first + i), 0, 16);
        }
        for (uint32_t base = rowLo; base < rowHi; base += passRows) {
            const uint32_t n = std::min(passRows, rowHi - base);
            for (uint32_t i = 0; i < n; ++i)
                flowStageRow(base + i, p.instKBase[base + i], p.live, p.prev, rows[i]);
            const uint32_t next = base + n < rowHi ? p.instKBase[base + n] : kFlowNoBase;
            for (uint32_t i = 0; i < pxPerView; ++i) {
                const uint32_t k = (uint32_t)p.ids[first + i];
                if (!pending[i] || !(k < next))
                    continue;
                const uint32_t slow = i / p.nfast, fast = i - slow * p.nfast;
                const uint32_t x = p.transposed ? slow : fast, y = p.transposed ? fast : slow;
                const uint32_t r = flowFindRow(rows.data(), n, k);
                if (r < n)
                    flowPixel(fv, rows[r], p.s, p.half, x, y, p.depth[first + i], p.flow + 4 * (first + i));
                pending[i] = 0;
            }
        }
    }
}

}  // namespace mrx

extern "C" int mrx_flow_host(const float *depth, const int32_t *ids, uint32_t views, uint32_t nfast, uint32_t nslow,
                             int transposed, uint32_t s, const float *consts, int consts_per_view,
                             const float *prev_consts, const uint32_t *inst_kbase, const uint32_t *world_inst_start,
                             const uint32_t *view_world, uint32_t num_worlds, uint32_t num_instances,
                             const float *const live[5], const float *const prev[5], uint32_t pass_rows, float *out_flow)
{
    using namespace mrx;
    const uint64_t px = (uint64_t)views * nfast * nslow;
    if (s < 1 || s > 4 || px > kFlowMaxPixels || !consts || !live || !prev)
        return MRX_E_INVALID;
    if (px && (!depth || !ids || !out_flow))
        return MRX_E_INVALID;
    if (num_worlds && !world_inst_start)
        return MRX_E_INVALID;
    if (views && (!prev_consts || !view_world || !world_inst_start || !live[3] || !live[4] || !prev[3] || !prev[4]))
        return MRX_E_INVALID;
    if (num_instances && (!inst_kbase || !live[0] || !live[1] || !live[2] || !prev[0] || !prev[1] || !prev[2]))
        return MRX_E_INVALID;
    for (uint32_t w = 0; w < num_worlds; ++w)
        if (world_inst_start[w] > world_inst_start[w + 1] || world_inst_start[w + 1] > num_instances)
            return MRX_E_INVALID;
    for (uint32_t v = 0; v < views; ++v)
        if (view_world[v] >= num_worlds)
            return MRX_E_INVALID;
    // per-view constants as the device table holds them
    std::vector<ViewProj> table;
    if (consts_per_view) {
        table.resize(views);
        for (uint32_t v = 0; v < views; ++v) {
            std::memset(&table[v], 0, sizeof(ViewProj));
            std::memcpy(&table[v], consts + 4 * (size_t)v, 16);
        }
    }
    FlowParams p {};
    p.depth = depth;
    p.ids = ids;
    p.flow = out_flow;
    p.instKBase = inst_kbase;
    p.worldInstStart = world_inst_start;
    p.viewWorld = view_world;
    p.live = FlowPose { live[0], live[1], live[2], live[3], live[4] };
    p.prev = FlowPose { prev[0], prev[1], prev[2], prev[3], prev[4] };
    p.viewProj = consts_per_view ? table.data() : nullptr;
    if (!consts_per_view) {
        p.sx = consts[0]; p.ox = consts[1]; p.sz = consts[2]; p.oz = consts[3];
    }
    p.prevProj = prev_consts;
    p.numViews = views;
    p.numInstances = num_instances;
    p.nfast = nfast;
    p.nslow = nslow;
    p.s = s;
    p.half = s / 2;
    p.transposed = transposed;
    p.numCUs = 1;
    p.passRows = pass_rows;
    if (px)
        flowHost(p);
    return MRX_OK;
}
