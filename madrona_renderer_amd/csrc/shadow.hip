// Shadow stage of a renderer with cast shadows.  One workgroup of 256 lanes per (view, block of
// 256 consecutive pixels in storage order); a lane owns one pixel.  The view, its world, its camera, its projection
// constants and its light are uniform: they are read through the workgroup's view index, that is with scalar loads.
//
// Every ray of a view has one direction, so a row's record carries that direction in the row's frame and its
// reciprocals (shadow_core.hpp shadowStageRow): the lane that stages the row computes them once, and a lane's work per
// row is the origin alone.
//
// Phase A: the workgroup stages the rows of the view's world into LDS, kShadowPassRows at a time.  Phase B: a loop over
// the staged rows; the record is made wave-uniform with readfirstlane.  A lane is UNDECIDED while it is a hit pixel
// whose ray is not degenerate and nothing has occluded it.  A row is skipped when no undecided lane of the wave passes
// its slab test (one ballot) and the row loop of a wave ends when it has no undecided lane left; the barriers of a
// world of several passes stay outside that loop, so every wave meets them.  Flat objects are walked in a uniform
// triangle loop that stops when the ballot of undecided lanes empties; the half of the triangle test that the
// direction and the triangle decide alone is computed once per triangle and wave, 32 triangles at a time, one per
// lane, and read back from the wave's LDS records as broadcasts (measured: 4.25).  Objects with a BLAS are traversed
// per lane, any hit (shadowTraverse); the stack is in dynamic LDS, stack[entry][lane], sized at launch from the scene's
// deepest BLAS.  The brute form (MRX_SHADOW_BRUTE=1) has no cull, no early exit and no shared half: every lane tests
// every triangle of every candidate row, the 36 bytes of a triangle read through the constant address space.
//
// The mask leaves as one byte per lane, 64 contiguous bytes per wave.  The applying form then reads one dword of the
// normal tensor and reads and writes one dword of rgb on its occluded lanes.
#include <algorithm>
#include <cmath>

#include <hip/hip_runtime.h>

#include "shadow.hpp"

namespace mrx {

namespace {

// a staged row, the same in every lane, moved to SGPRs (kBase and id are never staged)
__device__ __forceinline__ ShadowRow uniformRow(const ShadowRow &in)
{
    ShadowRow r;
#pragma unroll
    for (int i = 0; i < 9; ++i)
        r.r.R[i] = uniformF(in.r.R[i]);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        r.r.is[i] = uniformF(in.r.is[i]);
        r.r.t[i] = uniformF(in.r.t[i]);
        r.r.bbMin[i] = uniformF(in.r.bbMin[i]);
        r.r.bbMax[i] = uniformF(in.r.bbMax[i]);
        r.d[i] = uniformF(in.d[i]);
        r.id[i] = uniformF(in.id[i]);
    }
    r.r.firstTri = uniformU(in.r.firstTri);
    r.r.numTris = uniformU(in.r.numTris);
    r.r.root = (int32_t)uniformU((uint32_t)in.r.root);
    r.r.kBase = 0u;
    r.r.id = -1;
    return r;
}

struct ShadowArgs {
    RayTables s;
    const uint32_t *viewWorld;
    const float *depth;
    uint8_t *mask;
    uint32_t *rgb;
    const uint32_t *normal;
    const float *camPos, *camRot;
    const ViewProj *viewProj;
    const ViewLight *viewLight;
    float proj[4];                  // sx ox sz oz (viewProj == null)
    float light[5];                 // toLight, ambient, diffuse (viewLight == null)
    uint32_t nfast, pxPerView, blocksPerView;
    uint32_t ss, half, transposed;
    float bias, maxDistance;
    uint32_t passRows, stackCap;
};

template <bool APPLY, bool BRUTE>
__global__ __launch_bounds__(kShadowBlock) void shadowKernel(const ShadowArgs a)
{
    __shared__ ShadowRow rows[kShadowPassRows];
    __shared__ RayTriPrep prep[kShadowBlock / 64u][kShadowPrepTris];   // a wave's records of a flat object's triangles
    extern __shared__ uint32_t stackMem[];

    const uint32_t view = blockIdx.x / a.blocksPerView, block = blockIdx.x - view * a.blocksPerView;
    const uint32_t pix = block * kShadowBlock + threadIdx.x;
    const uint32_t wave = threadIdx.x / 64u, lane = threadIdx.x % 64u;
    const bool live = pix < a.pxPerView;
    const size_t item = (size_t)view * a.pxPerView + pix;
    const uint32_t world = a.viewWorld[view];
    const uint32_t rowLo = a.s.worldInstStart[world], rowHi = a.s.worldInstStart[world + 1];
    const CloudView cv = cloudLoadView<true>(a.camRot, a.camPos, a.viewProj, a.proj, view);
    const ShadowLight lt = shadowLoadLight(a.viewLight, a.light, view);

    // a lane past the view's end holds a background pixel
    const float z = live ? a.depth[item] : 0.0f;
    const uint32_t slow = pix / a.nfast, fast = pix - slow * a.nfast;
    const uint32_t x = a.transposed ? slow : fast, y = a.transposed ? fast : slow;
    const Ray ray = shadowRay(cv, a.ss, a.half, x, y, z, lt.toLight, a.bias, a.maxDistance);
    const bool hit = shadowHit(z);
    // S16's degenerate rays (a zero light direction, tmin >= tmax, a NaN in either) take no box and no BLAS node; the
    // brute form tests them like any other ray
    const bool dead = !BRUTE && rayDegenerate(ray);
    bool occluded = false;
    LaneStack<kShadowBlock> stack { stackMem + threadIdx.x, 0u, a.stackCap };

    for (uint32_t base = rowLo; base < rowHi; base += a.passRows) {
        const uint32_t n = min(a.passRows, rowHi - base);
        if (base != rowLo)
            __syncthreads();            // the pass before is still being read
        for (uint32_t i = threadIdx.x; i < n; i += kShadowBlock)
            shadowStageRow(base + i, a.s, lt.toLight, rows[i]);
        __syncthreads();

        for (uint32_t i = 0; i < n; ++i) {
            if (!BRUTE && __builtin_amdgcn_ballot_w64(hit && !dead && !occluded) == 0)
                break;                  // (the pass loop goes on: its barriers are every wave's)
            const ShadowRow row = uniformRow(rows[i]);
            if (row.r.numTris == 0)
                continue;
            float o[3];
            shadowOrigin(row.r, ray, o);
            if (!BRUTE) {
                const bool keep = hit && !dead && !occluded &&
                                  raySlabKeeps(row.r.bbMin, row.r.bbMax, o, row.id, ray.tmin, ray.tmax);
                if (__builtin_amdgcn_ballot_w64(keep) == 0)
                    continue;
                if (row.r.root >= 0) {
                    if (keep) {
                        stack.sp = 0;
                        occluded = shadowTraverse(row.r, a.s, o, row.d, row.id, ray.tmin, ray.tmax, stack);
                    }
                    continue;
                }
            }
            if (BRUTE) {
                // the pool is read-only for the whole launch and the address is wave-uniform: read through the constant
                // address space, the nine floats come as scalar loads whatever else the kernel stores in between
                const ConstFloat *tri = (const ConstFloat *)(a.s.tris + row.r.firstTri)->p;
                for (uint32_t k = 0; k < row.r.numTris; ++k, tri += sizeof(ObjTri) / sizeof(float)) {
                    float v[9], t;
#pragma unroll
                    for (int c = 0; c < 9; ++c)
                        v[c] = tri[c];
                    if (rayTriangleTest(v, o, row.d, ray.tmin, ray.tmax, t))
                        occluded = true;
                }
                continue;
            }
            // A flat object.  The direction is the row's, so half of the triangle test -- edges, d x e2, the
            // determinant and its reciprocal -- is the same for every pixel: lane l of the wave computes it for triangle
            // k0 + l and leaves it in the wave's own LDS records, then all lanes walk the records, each read a broadcast of
            // four 16-byte loads.  Only this wave writes and reads its records: no barrier, the fences order the wave's
            // own LDS traffic.
            for (uint32_t k0 = 0; k0 < row.r.numTris; k0 += kShadowPrepTris) {
                const uint32_t m = min(kShadowPrepTris, row.r.numTris - k0);
                if (lane < m) {
                    const float *tv = a.s.tris[row.r.firstTri + k0 + lane].p;
                    float v[9];
#pragma unroll
                    for (int c = 0; c < 9; ++c)
                        v[c] = tv[c];
                    RayTriPrep q;
                    rayTrianglePrep(v, row.d, q);
                    prep[wave][lane] = q;
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                for (uint32_t k = 0; k < m; ++k) {
                    if (__builtin_amdgcn_ballot_w64(hit && !dead && !occluded) == 0)
                        break;
                    const RayTriPrep q = prep[wave][k];
                    float t;
                    if (rayTrianglePrepped(q, o, row.d, ray.tmin, ray.tmax, t))
                        occluded = true;
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();        // (the next chunk, or the next row, overwrites the records)
            }
        }
    }
    if (live) {
        const bool dark = hit && occluded;
        a.mask[item] = dark ? (uint8_t)0 : (uint8_t)255;
        if (APPLY && dark) {
            float Rc[9], lv[3];
            quatRotation(a.camRot + 4 * (size_t)view, Rc);
            rotateT(Rc, lt.toLight, lv);
            a.rgb[item] = shadowApply(a.rgb[item], a.normal[item], lv, lt.ambient, lt.diffuse);
        }
    }
}

template <bool APPLY, bool BRUTE>
hipError_t launchKernel(const ShadowArgs &a, const ShadowPlan &plan, hipStream_t stream)
{
    hipLaunchKernelGGL((shadowKernel<APPLY, BRUTE>), dim3(plan.workgroups), dim3(kShadowBlock), plan.ldsBytes, stream, a);
    return hipGetLastError();
}

}  // namespace

hipError_t prepareShadow()
{
    // static rows + the deepest stacks pass the 64 KiB a kernel gets unasked
    const int bytes = (int)(kBvhStackCap * kShadowBlock * 4u);
    const void *kernels[4] = { (const void *)shadowKernel<false, false>, (const void *)shadowKernel<false, true>,
                               (const void *)shadowKernel<true, false>, (const void *)shadowKernel<true, true> };
    for (const void *k : kernels) {
        const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

hipError_t launchShadow(const ShadowParams &p, hipStream_t stream)
{
    ShadowPlan plan;
    {
        const hipError_t e = planShadow(p, plan);
        if (e != hipSuccess)
            return e;
    }
    if (plan.workgroups == 0)
        return hipSuccess;
    ShadowArgs a;
    a.s = p.s;
    a.viewWorld = p.viewWorld;
    a.depth = p.depth;
    a.mask = p.mask;
    a.rgb = p.rgb;
    a.normal = p.normal;
    a.camPos = p.camPos;
    a.camRot = p.camRot;
    a.viewProj = p.viewProj;
    a.viewLight = p.viewLight;
    a.proj[0] = p.sx; a.proj[1] = p.ox; a.proj[2] = p.sz; a.proj[3] = p.oz;
    a.light[0] = p.toLight[0]; a.light[1] = p.toLight[1]; a.light[2] = p.toLight[2];
    a.light[3] = p.ambient; a.light[4] = p.diffuse;
    a.nfast = p.nfast;
    a.pxPerView = p.nfast * p.nslow;
    a.blocksPerView = plan.blocksPerView;
    a.ss = p.ss;
    a.half = p.half;
    a.transposed = p.transposed ? 1u : 0u;
    a.bias = p.bias;
    a.maxDistance = p.maxDistance;
    a.passRows = plan.passRows;
    a.stackCap = plan.stackEntries;
    if (p.apply)
        return p.brute ? launchKernel<true, true>(a, plan, stream) : launchKernel<true, false>(a, plan, stream);
    return p.brute ? launchKernel<false, true>(a, plan, stream) : launchKernel<false, false>(a, plan, stream);
}

}  // namespace mrx
