// Trace stage of a renderer with a ray-cast sensor.  One workgroup of 256 lanes per (world, block
// of 256 rays); a lane owns one ray.
//
// Phase A: the workgroup stages the rows of its world into LDS, kRayPassRows at a time -- R(q_i), 1 / scale, position,
// the bound object's triangle range, BLAS root and box, the row's first world-local triangle index and the id a hit
// stores (rays_core.hpp rayStageRow).  A row that is no candidate (hidden, unbound, a zero or non-finite scale) is
// staged with no triangles.
//
// Phase B: a loop over the staged rows that every lane of the workgroup takes together; the row's record is read from
// LDS and made wave-uniform with readfirstlane, so it lives in SGPRs.  Each lane takes its ray into the instance's
// frame and tests the object's box.  Flat objects (no BLAS, <= 32 triangles) are walked in a wave-uniform loop, entered
// only when some lane's box test passed (ballot): the triangle index is uniform, the 64-byte ObjTri lines come through
// scalar loads, and every lane tests the triangle.  Objects with a BLAS are traversed per lane (rayTraverse); the stack
// is in LDS, stack[entry][lane], sized at launch from the scene's deepest BLAS -- a per-lane array indexed at run time
// would live in scratch.  The brute form (MRX_RAYS_BRUTE=1) skips every cull and walks every triangle of every
// candidate row in the uniform loop.
//
// t and the id are stored as coalesced dwords: lane l of block b of world w writes element w * R + 256 * b + l.
#include <algorithm>

#include <hip/hip_runtime.h>

#include "rays.hpp"

namespace mrx {

namespace {

// a staged row, the same in every lane, moved to SGPRs
__device__ __forceinline__ RayRow uniformRow(const RayRow &in)
{
    RayRow r;
#pragma unroll
    for (int i = 0; i < 9; ++i)
        r.R[i] = uniformF(in.R[i]);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        r.is[i] = uniformF(in.is[i]);
        r.t[i] = uniformF(in.t[i]);
        r.bbMin[i] = uniformF(in.bbMin[i]);
        r.bbMax[i] = uniformF(in.bbMax[i]);
    }
    r.firstTri = uniformU(in.firstTri);
    r.numTris = uniformU(in.numTris);
    r.root = (int32_t)uniformU((uint32_t)in.root);
    r.kBase = uniformU(in.kBase);
    r.id = (int32_t)uniformU((uint32_t)in.id);
    return r;
}

struct RayArgs {
    RayTables s;
    const float *rays;
    const int32_t *frame;
    float *outT;
    int32_t *outId;
    uint32_t R, blocksPerWorld, passRows, stackCap;
};

template <bool BRUTE>
__global__ __launch_bounds__(kRayBlock) void rayKernel(const RayArgs a)
{
    __shared__ RayRow rows[kRayPassRows];
    extern __shared__ uint32_t stackMem[];

    const uint32_t world = blockIdx.x / a.blocksPerWorld, block = blockIdx.x - world * a.blocksPerWorld;
    const uint32_t rayIdx = block * kRayBlock + threadIdx.x;
    const bool live = rayIdx < a.R;
    const size_t slot = (size_t)world * a.R + rayIdx;
    const uint32_t rowLo = a.s.worldInstStart[world], rowHi = a.s.worldInstStart[world + 1];

    // a lane past the end holds the zero ray, which misses everything
    float in[8] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
    if (live) {
        const float4 lo = reinterpret_cast<const float4 *>(a.rays)[2 * slot];
        const float4 hi = reinterpret_cast<const float4 *>(a.rays)[2 * slot + 1];
        in[0] = lo.x; in[1] = lo.y; in[2] = lo.z; in[3] = lo.w;
        in[4] = hi.x; in[5] = hi.y; in[6] = hi.z; in[7] = hi.w;
    }
    const Ray ray = rayFromFrame(in, a.frame[world], rowLo, rowHi, a.s);
    // S16's degenerate rays (and the idle lanes' zero ray) take no box and no BLAS node; the brute form tests them like
    // any other ray
    const bool dead = !BRUTE && rayDegenerate(ray);
    RayBest best { 0.0f, kRayNoHit, -1 };
    LaneStack<kRayBlock> stack { stackMem + threadIdx.x, 0u, a.stackCap };

    for (uint32_t base = rowLo; base < rowHi; base += a.passRows) {
        const uint32_t n = min(a.passRows, rowHi - base);
        if (base != rowLo)
            __syncthreads();            // the pass before is still being read
        for (uint32_t i = threadIdx.x; i < n; i += kRayBlock)
            rayStageRow(base + i, a.s, rows[i]);
        __syncthreads();

        for (uint32_t i = 0; i < n; ++i) {
            const RayRow row = uniformRow(rows[i]);
            if (row.numTris == 0)
                continue;
            float o[3], d[3];
            rayToInstance(row, ray, o, d);
            bool walk = true;
            if (!BRUTE) {
                float id[3];
                rayInvDir(d, id);
                const float tHi = best.k == kRayNoHit ? ray.tmax : (best.t < ray.tmax ? best.t : ray.tmax);
                const bool keep = !dead && raySlabKeeps(row.bbMin, row.bbMax, o, id, ray.tmin, tHi);
                if (row.root >= 0) {
                    if (keep) {
                        stack.sp = 0;
                        rayTraverse(row, a.s, o, d, id, ray.tmin, ray.tmax, stack, best);
                    }
                    continue;
                }
                walk = __builtin_amdgcn_ballot_w64(keep) != 0;
            }
            if (walk) {
                // the pool is read-only for the whole launch and the address is wave-uniform: read through the constant
                // address space, the nine floats come as scalar loads whatever else the kernel stores in between
                const ConstFloat *tri = (const ConstFloat *)(a.s.tris + row.firstTri)->p;
                for (uint32_t k = 0; k < row.numTris; ++k, tri += sizeof(ObjTri) / sizeof(float)) {
                    float v[9];
#pragma unroll
                    for (int c = 0; c < 9; ++c)
                        v[c] = tri[c];
                    rayTriangle(v, o, d, ray.tmin, ray.tmax, row.kBase + k, row.id, best);
                }
            }
        }
    }
    if (live) {
        a.outT[slot] = best.k == kRayNoHit ? in[7] : best.t;
        a.outId[slot] = best.k == kRayNoHit ? -1 : best.id;
    }
}

template <bool BRUTE>
hipError_t launchKernel(const RayArgs &a, const RayPlan &plan, hipStream_t stream)
{
    hipLaunchKernelGGL(rayKernel<BRUTE>, dim3(plan.workgroups), dim3(kRayBlock), plan.ldsBytes, stream, a);
    return hipGetLastError();
}

}  // namespace

hipError_t planRays(const RayParams &p, RayPlan &plan)
{
    plan = RayPlan {};
    if (p.R < 1 || p.R > kRayMaxPerWorld || (uint64_t)p.numWorlds * p.R >= (1ull << 31) || p.numCUs == 0)
        return hipErrorInvalidValue;
    if (!p.rays || !p.frame || !p.outT || !p.outId || !p.s.tris || !p.s.instInfo || !p.s.instKBase || !p.s.boundObj ||
        !p.s.worldInstStart || !p.s.instPos || !p.s.instRot || !p.s.instScale || !p.s.instObj)
        return hipErrorInvalidValue;
    const uint32_t entries = 1u + 7u * p.bvhDepth;
    if (p.bvhDepth > kBvhStackCap || entries > kBvhStackCap)
        return hipErrorInvalidValue;
    if (p.bvhDepth && (!p.s.nodes || !p.s.leafTris))
        return hipErrorInvalidValue;
    plan.blocksPerWorld = (p.R + kRayBlock - 1u) / kRayBlock;
    plan.workgroups = p.numWorlds * plan.blocksPerWorld;            // <= (worlds * R + 255 * worlds) / 256 < 2^31
    plan.stackEntries = entries;
    plan.passRows = p.passRows ? std::min(p.passRows, kRayPassRows) : kRayPassRows;
    plan.ldsBytes = entries * kRayBlock * 4u;
    return hipSuccess;
}

hipError_t prepareRays()
{
    // static rows + the deepest stacks pass the 64 KiB a kernel gets unasked
    const int bytes = (int)(kBvhStackCap * kRayBlock * 4u);
    const hipError_t e = hipFuncSetAttribute((const void *)rayKernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    return e != hipSuccess ? e
                           : hipFuncSetAttribute((const void *)rayKernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

hipError_t launchRays(const RayParams &p, hipStream_t stream)
{
    RayPlan plan;
    {
        const hipError_t e = planRays(p, plan);
        if (e != hipSuccess)
            return e;
    }
    if (plan.workgroups == 0)
        return hipSuccess;
    RayArgs a;
    a.s = p.s;
    a.rays = p.rays;
    a.frame = p.frame;
    a.outT = p.outT;
    a.outId = p.outId;
    a.R = p.R;
    a.blocksPerWorld = plan.blocksPerWorld;
    a.passRows = plan.passRows;
    a.stackCap = plan.stackEntries;
    return p.brute ? launchKernel<true>(a, plan, stream) : launchKernel<false>(a, plan, stream);
}

}  // namespace mrx
