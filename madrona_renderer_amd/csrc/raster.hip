// Tiled software rasterizer / primary-ray caster for gfx950 (MI355X).
//
// Three kernels share the spec arithmetic below:
//   rasterGroupKernel    the production path for worlds of <= 256 triangles:
//                        one workgroup per group of views / tiles, setup per
//                        view, register/LDS binning, packed-FMA raster,
//                        16-byte write-through stores
//   rasterChunkedKernel  worlds of more than 256 triangles: one workgroup per
//                        tile, triangles through LDS in passes of 256
//   rasterBruteKernel    the round's first kernel (every triangle at every
//                        pixel), kept as an on-device cross-check (variant 1)
// Phases: S setup (lane = triangle: pose -> view-space vertices -> edge /
// 1-over-depth / attribute planes, flat colour), binning (lane = triangle,
// regions of the tile), R raster (lane = pixels, per-pixel z and winner in
// VGPRs, triangle planes broadcast from LDS), O output (shade, 1/depth, store).
//
// The file is compiled with -ffp-contract=off; fused multiply-adds appear only
// where the spec writes fma().  The CPU oracle (oracle/raster_oracle.c) is a
// separate restatement of the same spec and is never linked here.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>

#include "raster.hpp"
#include "raster_dev.hpp"

namespace mrx {
namespace {

constexpr int kWavesPerBlock = 4;
// launch bounds of the brute and the chunked kernels, uniform and form alike (the second bound is waves per SIMD)
constexpr int kBruteThreads = kWave * kWavesPerBlock;
constexpr int kChunkedThreads = kWave * kWavesPerBlock, kChunkedWavesPerSimd = 3;
constexpr int kHot = 16;         // dwords: edges, depth plane, rgba, tex, seg, k
constexpr int kBandRows = 16;    // a band is 64 x 16 pixels = 16 blocks of 8x8
constexpr int kBlocksPerBand = 16;

// Per-wave LDS: the shading record of each triangle of the chunk.  The brute
// variant also parks the planes here (hot[0..11]); the strip variant keeps
// them in registers and uses the compact layout.
struct WaveLds {
    float hot[kChunk][kHot];     // [0..11] planes (brute only), [12..15] shade
    float cold[kChunk][kCold];
};

// ---------------------------------------------------------------------------
// Shared pieces of the per-wave tile loop
// ---------------------------------------------------------------------------
struct TileCtx {
    uint32_t view, tileX0, tileY0;
    uint32_t triBegin, numTris;
    int lx, ly;
};

// PV: the per-view form -- `lt` receives the light of the view's world from its record, read
// beside the camera rotation it is combined with; else the uniform light of the kernel arguments.
template <bool PV>
__device__ __forceinline__ bool tileSetup(const RasterParams &p, uint32_t item, int lane,
                                          TileCtx &t, ViewConst &vc, ViewLight &lt)
{
    const uint32_t tilesPerView = p.tilesFast * p.tilesSlow;
    if (item >= p.numViews * tilesPerView)
        return false;
    t.view = item / tilesPerView;
    const uint32_t tile = item % tilesPerView;
    t.tileX0 = (tile % p.tilesFast) * 64u;
    t.tileY0 = (tile / p.tilesFast) * 64u;
    const float4 q = *reinterpret_cast<const float4 *>(p.camRot + 4 * t.view);
    // (a wave renders tiles of one view: the index is wave-uniform, the record a scalar load)
    if (PV)
        lt = viewLightOf(p, true, __builtin_amdgcn_readfirstlane(t.view));
    quatToMat(q.x, q.y, q.z, q.w, vc.Rc);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        vc.c[r] = p.camPos[3 * t.view + r];
        if (PV)
            vc.lv[r] = dot3(vc.Rc[0][r], vc.Rc[1][r], vc.Rc[2][r], lt.toLight[0], lt.toLight[1], lt.toLight[2]);
        else
            vc.lv[r] = dot3(vc.Rc[0][r], vc.Rc[1][r], vc.Rc[2][r],
                            p.toLight[0], p.toLight[1], p.toLight[2]);
    }
    // wave-uniform: park the view constants in SGPRs
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int cc = 0; cc < 3; ++cc)
            vc.Rc[r][cc] = __uint_as_float(
                __builtin_amdgcn_readfirstlane(__float_as_uint(vc.Rc[r][cc])));
        vc.c[r] = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(vc.c[r])));
        vc.lv[r] = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(vc.lv[r])));
    }
    t.triBegin = t.view * p.viewTriStride;
    t.numTris = p.viewTriCount[t.view];
    t.lx = lane & 7;
    t.ly = lane >> 3;
    return true;
}

// What the group kernel's set-up reads per triangle (instanceTransform / setupTriangleCore are templates over
// the parameter type): pointers from the preloaded header or from RasterParams, scalars from RasterParams
// (the projection constants: from the view's record in the per-view form).
struct GroupSetupArgs {
    const ObjTri *tris;
    const TriMat *triMats;
    const float *instPos, *instRot, *instScale;
    float sx, ox, sz, oz, s6bPad, ambient, diffuse;
    int32_t transposed;
};

// setupTriangle under the projection constants `pr` of the view and the light `lt` of its world (per-view form), and
// under the colour and material overrides of the instance row where the renderer has the columns (DESIGN.md 4.13,
// 4.14; wave-uniform tests).  LAB (the instantiations that store ids): under the label column too (S11, 4.16).
template <bool LAB = false, typename NRMOUT = NoNormalOut>
__device__ __forceinline__ bool setupTriangleProj(const RasterParams &p, const ViewProj &pr, const ViewLight &lt,
                                                  const ViewConst &vc, WorldTri wt, int32_t kWorld, TriPlanes &out,
                                                  float *shade, float *cold, const NRMOUT nrm = NRMOUT())
{
    const GroupSetupArgs sa = { p.tris, p.triMats, p.instPos, p.instRot, p.instScale,
                                pr.sx, pr.ox, pr.sz, pr.oz, pr.s6bPad, lt.ambient, lt.diffuse, p.transposed };
    InstXform x;
    instanceTransform(sa, vc, wt.inst, x);
    const uint32_t icol = p.instColor ? p.instColor[wt.inst] : 0u;
    // (read where the set-up turns to colour: raster_dev.hpp)
    const auto matOf = [&]() -> MatOverride {
        return MatOverride { p.instMat ? p.instMat[wt.inst] : -1, p.numMaterials, p.matTable };
    };
    const bool valid = setupTriangleCore<true, true, true, true>(sa, vc.lv, x, wt.tri, p.instObj[wt.inst], kWorld, out, shade,
                                                                 cold, icol, matOf, nrm);
    if (LAB)
        applyLabel(shade, p.instLabel, wt.inst);
    return valid;
}

// A TriPlanes of zeros: what an idle slot publishes.
__device__ __forceinline__ void zeroPlanes(TriPlanes &c)
{
    c.A0 = c.B0 = c.C0 = c.A1 = c.B1 = c.C1 = 0.0f;
    c.A2 = c.B2 = c.C2 = c.Dx = c.Dy = c.Dc = 0.0f;
    c.bbX0 = c.bbX1 = c.bbY0 = c.bbY1 = 0.0f;
}
// The planes of a triangle as phase R reads them from LDS (loadPlanes): A0 A1 A2 Dx | B0 B1 B2 Dy | C0 C1 C2 Dc, and a
// fourth float4 that is the kernel's own -- the bounding box in the group kernel, the region mask in the chunked one.
__device__ __forceinline__ void publishPlanes(float (&rec)[16], const TriPlanes &c, float4 fourth)
{
    float4 *dst = reinterpret_cast<float4 *>(rec);
    dst[0] = make_float4(c.A0, c.A1, c.A2, c.Dx);
    dst[1] = make_float4(c.B0, c.B1, c.B2, c.Dy);
    dst[2] = make_float4(c.C0, c.C1, c.C2, c.Dc);
    dst[3] = fourth;
}

// S for one chunk of up to 64 world-triangles; returns the valid-lane mask.
// PV: the per-view form, the view's projection constants in `pr` and its world's light in `lt`.
// NRM: the normals form: the packed normal of the lane's triangle goes to nrmTab[lane].
// LAB: passed on to setupTriangleProj.
template <bool PV, bool NRM = false, bool LAB = false>
__device__ __forceinline__ uint64_t setupChunk(const RasterParams &p, const ViewConst &vc,
                                               const TileCtx &t, uint32_t chunk, int lane,
                                               WaveLds &L, const ViewProj &pr, const ViewLight &lt,
                                               uint32_t *nrmTab = nullptr)
{
    bool valid = false;
    const uint32_t k = chunk + lane;
    if (k < t.numTris) {
        const WorldTri wt = p.viewTris[t.triBegin + k];
        TriPlanes c;
        float *h = L.hot[lane];
        if (NRM)
            valid = PV ? setupTriangleProj<LAB>(p, pr, lt, vc, wt, (int32_t)k, c, h + 12, L.cold[lane], NormalOut { nrmTab + lane })
                       : setupTriangle(p, vc, wt, (int32_t)k, c, h + 12, L.cold[lane], NormalOut { nrmTab + lane });
        else
            valid = PV ? setupTriangleProj<LAB>(p, pr, lt, vc, wt, (int32_t)k, c, h + 12, L.cold[lane])
                       : setupTriangle(p, vc, wt, (int32_t)k, c, h + 12, L.cold[lane]);
        h[0] = c.A0; h[1] = c.B0; h[2] = c.C0;
        h[3] = c.A1; h[4] = c.B1; h[5] = c.C1;
        h[6] = c.A2; h[7] = c.B2; h[8] = c.C2;
        h[9] = c.Dx; h[10] = c.Dy; h[11] = c.Dc;
    }
    const uint64_t mask = __ballot(valid);
    waveLdsSync();
    return mask;
}

// Winner lookup + shading of one pixel (lane) of block b.
__device__ __forceinline__ const float *shadeRec(const WaveLds &L, int32_t w) { return &L.hot[w][12]; }

template <bool IDS, typename LDS>
__device__ __forceinline__ void resolvePixel(const RasterParams &p, const LDS &L,
                                             int32_t w, float bestInv, float px, float py,
                                             uint32_t &rgba, int32_t &id)
{
    const float *h = shadeRec(L, w);
    rgba = __float_as_uint(h[0]);
    const int32_t tex = __float_as_int(h[1]);
    if (tex >= 0) {
        const float tt = 1.0f / bestInv;
        rgba = shadeTextured(p, L.cold[w], tex, px, py, tt);
    }
    if (IDS)
        id = __float_as_int(p.idsAreSegmask ? h[2] : h[3]);
}

// ---------------------------------------------------------------------------
// Variant 1 ("brute"): every valid triangle is tested at every pixel.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void rasterBandBrute(const WaveLds &L, uint64_t validMask,
                                                const float (&pxf)[8], float py0, float py1,
                                                float invNear,
                                                float (&best)[kBlocksPerBand],
                                                int32_t (&bid)[kBlocksPerBand])
{
    for (uint64_t m = validMask; m != 0; m &= m - 1) {
        const int k = __builtin_ctzll(m);
        const float *h = L.hot[k];
        const float A0 = h[0], B0 = h[1], C0 = h[2];
        const float A1 = h[3], B1 = h[4], C1 = h[5];
        const float A2 = h[6], B2 = h[7], C2 = h[8];
        const float Dx = h[9], Dy = h[10], Dc = h[11];
        float r0[2], r1[2], r2[2], rd[2];
        r0[0] = __builtin_fmaf(B0, py0, C0); r0[1] = __builtin_fmaf(B0, py1, C0);
        r1[0] = __builtin_fmaf(B1, py0, C1); r1[1] = __builtin_fmaf(B1, py1, C1);
        r2[0] = __builtin_fmaf(B2, py0, C2); r2[1] = __builtin_fmaf(B2, py1, C2);
        rd[0] = __builtin_fmaf(Dy, py0, Dc); rd[1] = __builtin_fmaf(Dy, py1, Dc);
#pragma unroll
        for (int b = 0; b < kBlocksPerBand; ++b) {
            const int r = b >> 3, bx = b & 7;
            const float e0 = __builtin_fmaf(A0, pxf[bx], r0[r]);
            const float e1 = __builtin_fmaf(A1, pxf[bx], r1[r]);
            const float e2 = __builtin_fmaf(A2, pxf[bx], r2[r]);
            const float it = __builtin_fmaf(Dx, pxf[bx], rd[r]);
            const bool in = (fminf(fminf(e0, e1), e2) >= 0.0f) &&
                            (it > best[b]) && (it <= invNear);
            best[b] = in ? it : best[b];
            bid[b] = in ? k : bid[b];
        }
    }
}

// OUT: output selection (raster.hpp OutSel: kOutRGBD, kOutDepth or kOutRGB; kOutByPointer in the per-view form)
// PV: per-view projection -- a wave renders one tile, so the view's record is wave-uniform
// NRM: the normals form: the chunk's packed normals in an LDS array of their own, one more
// resolved dword per pixel, one more store
template <bool IDS, bool MULTI, int OUT, bool PV, bool NRM = false>
__device__ __forceinline__ void bruteKernelBody(const RasterParams p)
{
    __shared__ WaveLds lds[kWavesPerBlock];
    __shared__ uint32_t nrmLds[NRM ? kWavesPerBlock : 1][NRM ? kChunk : 1];
    touchKernelArguments();
    const int wave = threadIdx.x / kWave;
    const int lane = threadIdx.x % kWave;
    TileCtx t;
    ViewConst vc;
    ViewLight lt = {};
    if (!tileSetup<PV>(p, blockIdx.x * kWavesPerBlock + wave, lane, t, vc, lt))
        return;
    WaveLds &L = lds[wave];
    uint32_t *const nrmTab = NRM ? nrmLds[wave] : nullptr;
    const ViewProj pr = viewProjOf(p, PV, t.view);

    float pxf[8];
#pragma unroll
    for (int bx = 0; bx < 8; ++bx)
        pxf[bx] = (float)(t.tileX0 + bx * 8 + t.lx);
    const float invNear = PV ? pr.invNear : p.invNear;

    uint64_t mask0 = 0;
    if (!MULTI)
        mask0 = setupChunk<PV, NRM, IDS>(p, vc, t, 0, lane, L, pr, lt, nrmTab);

    for (int band = 0; band < 4; ++band) {
        float best[kBlocksPerBand];
        int32_t bid[kBlocksPerBand];
        uint32_t outRgba[kBlocksPerBand];
        int32_t outId[kBlocksPerBand];
        uint32_t outNrm[kBlocksPerBand];
#pragma unroll
        for (int b = 0; b < kBlocksPerBand; ++b) {
            best[b] = p.invFar;
            bid[b] = -1;
            outRgba[b] = 0xFF000000u;
            outId[b] = -1;
            if (NRM)
                outNrm[b] = kNormalBackground;
        }
        const float py0 = (float)(t.tileY0 + band * kBandRows + t.ly);
        const float py1 = (float)(t.tileY0 + band * kBandRows + 8 + t.ly);

        if (!MULTI) {
            rasterBandBrute(L, mask0, pxf, py0, py1, invNear, best, bid);
#pragma unroll
            for (int b = 0; b < kBlocksPerBand; ++b)
                if (bid[b] >= 0) {
                    resolvePixel<IDS>(p, L, bid[b], best[b], pxf[b & 7],
                                      (b >> 3) ? py1 : py0, outRgba[b], outId[b]);
                    if (NRM)
                        outNrm[b] = nrmTab[bid[b]];
                }
        } else {
            for (uint32_t chunk = 0; chunk < t.numTris; chunk += kChunk) {
                const uint64_t mask = setupChunk<PV, NRM, IDS>(p, vc, t, chunk, lane, L, pr, lt, nrmTab);
                rasterBandBrute(L, mask, pxf, py0, py1, invNear, best, bid);
                // resolve this chunk's winners before its records are replaced
#pragma unroll
                for (int b = 0; b < kBlocksPerBand; ++b) {
                    if (bid[b] >= 0) {
                        resolvePixel<IDS>(p, L, bid[b], best[b], pxf[b & 7],
                                          (b >> 3) ? py1 : py0, outRgba[b], outId[b]);
                        if (NRM)
                            outNrm[b] = nrmTab[bid[b]];
                    }
                    bid[b] = -1;
                }
                waveLdsSync();
            }
        }

        // ---- O: output the band
#pragma unroll
        for (int b = 0; b < kBlocksPerBand; ++b) {
            const int r = b >> 3, bx = b & 7;
            const uint32_t fx = t.tileX0 + bx * 8 + t.lx;
            const uint32_t fy = t.tileY0 + band * kBandRows + r * 8 + t.ly;
            if (fx < p.nfast && fy < p.nslow) {
                const bool hit = best[b] > p.invFar;
                const float dep = hit ? 1.0f / best[b] : 0.0f;
                const size_t o = ((size_t)t.view * p.nslow + fy) * p.nfast + fx;
                if (storesRgb<OUT>(p.rgb))
                    p.rgb[o] = outRgba[b];
                if (storesDepth<OUT>(p.depth))
                    p.depth[o] = dep;
                if (IDS)
                    p.ids[o] = outId[b];
                if (NRM)
                    p.normal[o] = outNrm[b];
            }
        }
    }
}

template <bool IDS, bool MULTI, int OUT = kOutRGBD>
__global__ __launch_bounds__(kBruteThreads)
void rasterBruteKernel(const RasterParams p)
{
    bruteKernelBody<IDS, MULTI, OUT, false>(p);
}

// The form kernel (raster.hpp KernelForm; the bound does not depend on the form), output selection by pointer:
// PV the per-view form (p.viewProj), N and NPV the normals forms (p.normal) over the uniform constants
// and over the per-view tables (and the colour / material columns behind their null checks).
template <KernelForm F, bool IDS, bool MULTI>
__global__ __launch_bounds__(kBruteThreads)
void rasterBruteFormKernel(const RasterParams p)
{
    static_assert(F == KernelForm::PV || F == KernelForm::N || F == KernelForm::NPV, "the forms of this family");
    bruteKernelBody<IDS, MULTI, kOutByPointer, formFlags(F).pv, formFlags(F).nrm>(p);
}

// Bits 0..15: the tile's 32x8 regions (bit 2*strip + half) the lane's triangle
// can touch.  Bit 16: the 1/depth plane stays <= invNear over the whole tile,
// so the per-pixel near test can be dropped for this triangle.
constexpr uint32_t kNearFree = 1u << 16;

// ---------------------------------------------------------------------------
// Wave-level binning.  The lane that set a triangle up classifies the tile's
// sixteen 32x8-pixel regions against it: a region is dropped when one edge
// plane is negative, or the 1/depth plane is outside (invFar, invNear], at the
// region pixel where that plane is largest / smallest, or when it misses the
// triangle's conservative bounding box.  The planes are evaluated as
// fl(A*x + fl(B*y + C)), monotone in x and in y, so the extreme over a region
// is the value at one of its corner pixels and dropping a region cannot change
// any pixel: binning only skips work.
// ---------------------------------------------------------------------------
// Region bits of strips [S0, S1) for the lane's triangle; `nearOk` reports
// whether the 1/depth plane stays <= invNear over those strips.
template <int S0, int S1>
__device__ __forceinline__ uint32_t classifyStrips(const TriPlanes &c, uint32_t tileX0,
                                                   uint32_t tileY0, float invNear, float invFar,
                                                   bool &nearOk)
{
    const float X0 = (float)tileX0, Y0 = (float)tileY0;
    // x / y of the region pixel where each plane is largest (depth: also smallest)
    const float xa0 = c.A0 < 0.0f ? X0 : X0 + 31.0f;
    const float xa1 = c.A1 < 0.0f ? X0 : X0 + 31.0f;
    const float xa2 = c.A2 < 0.0f ? X0 : X0 + 31.0f;
    const float xdh = c.Dx < 0.0f ? X0 : X0 + 31.0f;
    const float xdl = c.Dx < 0.0f ? X0 + 31.0f : X0;
    const float yb0 = c.B0 < 0.0f ? Y0 : Y0 + 7.0f;
    const float yb1 = c.B1 < 0.0f ? Y0 : Y0 + 7.0f;
    const float yb2 = c.B2 < 0.0f ? Y0 : Y0 + 7.0f;
    const float ydh = c.Dy < 0.0f ? Y0 : Y0 + 7.0f;
    const float ydl = c.Dy < 0.0f ? Y0 + 7.0f : Y0;
    uint32_t mask = 0;
    float dmax = -__builtin_inff();
#pragma unroll
    for (int s = S0; s < S1; ++s) {
        const float dy = (float)(8 * s);
        const float r0 = __builtin_fmaf(c.B0, yb0 + dy, c.C0);
        const float r1 = __builtin_fmaf(c.B1, yb1 + dy, c.C1);
        const float r2 = __builtin_fmaf(c.B2, yb2 + dy, c.C2);
        const float rh = __builtin_fmaf(c.Dy, ydh + dy, c.Dc);
        const float rl = __builtin_fmaf(c.Dy, ydl + dy, c.Dc);
        const bool yin = (Y0 + dy + 7.0f >= c.bbY0) && (Y0 + dy <= c.bbY1);
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const float dx = (float)(32 * hf);
            const float e0 = __builtin_fmaf(c.A0, xa0 + dx, r0);
            const float e1 = __builtin_fmaf(c.A1, xa1 + dx, r1);
            const float e2 = __builtin_fmaf(c.A2, xa2 + dx, r2);
            const float dh = __builtin_fmaf(c.Dx, xdh + dx, rh);
            const float dl = __builtin_fmaf(c.Dx, xdl + dx, rl);
            const bool xin = (X0 + dx + 31.0f >= c.bbX0) && (X0 + dx <= c.bbX1);
            const bool possible = (fminf(fminf(e0, e1), e2) >= 0.0f) &&
                                  (dh > invFar) && (dl <= invNear) && xin && yin;
            mask |= possible ? (1u << (2 * s + hf)) : 0u;
            dmax = fmaxf(dmax, dh);
        }
    }
    nearOk = dmax <= invNear;
    return mask;
}

__device__ __forceinline__ uint32_t classifyRegions(const TriPlanes &c, const TileCtx &t,
                                                    float invNear, float invFar)
{
    bool nearOk;
    uint32_t mask = classifyStrips<0, 8>(c, t.tileX0, t.tileY0, invNear, invFar, nearOk);
    if (nearOk)
        mask |= kNearFree;
    return mask;
}


// One pixel of the lane against one triangle.  The three lane predicates are
// combined on the scalar unit (s_and_b64), which runs beside the vector ALU
// that bounds this kernel.
template <bool NEAR>
__device__ __forceinline__ void pixelTest(const PlanePairs &q, f32x2 r01, f32x2 r2d, float px,
                                          float invNear, int32_t kv, float &best, int32_t &bid)
{
    const f32x2 pp = { px, px };
    const f32x2 e01 = fma2(q.A01, pp, r01);       // e0, e1
    const f32x2 e2d = fma2(q.A2D, pp, r2d);       // e2, 1/depth
    bool in = (fminf(fminf(e01.x, e01.y), e2d.x) >= 0.0f) & (e2d.y > best);
    if (NEAR)
        in = in & (e2d.y <= invNear);
    best = in ? e2d.y : best;
    bid = in ? kv : bid;
}

// Rasterise one 32x8 region against the triangles in `act` (bit k = triangle
// k of the chunk survives classification for this region), in triangle order.
// Triangle planes are broadcast from LDS (all lanes read the same 48 bytes).
template <bool NEAR, int IDSHIFT>
__device__ __forceinline__ void rasterRegion(const float (*planes)[16], uint64_t act, int recBase,
                                             const float (&px)[kRegionBlocks], float py,
                                             float invNear,
                                             float (&best)[kRegionBlocks],
                                             int32_t (&bid)[kRegionBlocks])
{
    const f32x2 yy = { py, py };
    for (; act != 0; act &= act - 1) {
        const int k = recBase + __builtin_ctzll(act);   // record index in the LDS tables
        const PlanePairs q = loadPlanes(planes, k);
        const f32x2 r01 = fma2(q.B01, yy, q.C01);
        const f32x2 r2d = fma2(q.B2D, yy, q.C2D);
        // the winner is tracked as k << IDSHIFT (group kernel: the byte offset
        // of its shading record)
#pragma unroll
        for (int b = 0; b < kRegionBlocks; ++b)
            pixelTest<NEAR>(q, r01, r2d, px[b], invNear, k << IDSHIFT, best[b], bid[b]);
    }
}

// Store a region whose pixels are already shaded (chunked kernel).  A lane owns
// four consecutive pixels of one row (pixel b of the lane is x = fx0 + b), so
// the common case is one 16-byte store per output tensor per lane.
// NRM: the normals form -- `nrm` holds the pixels' packed normals, one more store of the same shape
template <bool IDS, bool NRM = false>
__device__ __forceinline__ void outputRegion(const RasterParams &p, const TileCtx &t,
                                             uint32_t fx0, uint32_t fy, float invFar,
                                             const float (&best)[kRegionBlocks],
                                             const uint32_t (&rgba)[kRegionBlocks],
                                             const int32_t (&id)[kRegionBlocks],
                                             const uint32_t *nrm = nullptr)
{
    float dep[kRegionBlocks];
#pragma unroll
    for (int b = 0; b < kRegionBlocks; ++b)
        dep[b] = best[b] > invFar ? __builtin_amdgcn_rcpf(best[b]) : 0.0f;
    if (fy >= p.nslow || (p.debugSkip & 1u))
        return;
    const size_t o = ((size_t)t.view * p.nslow + fy) * p.nfast + fx0;
    // (output selection: a runtime guard on each tensor's stores)
    const bool doRgb = storesRgb<kOutByPointer>(p.rgb), doDepth = storesDepth<kOutByPointer>(p.depth);
    if ((p.nfast & 3u) == 0 && fx0 + 3 < p.nfast) {
        if (doRgb)
            streamStore16(p.writeThrough, p.rgb + o, rgba[0], rgba[1], rgba[2], rgba[3]);
        if (doDepth)
            streamStore16(p.writeThrough, p.depth + o, __float_as_uint(dep[0]), __float_as_uint(dep[1]),
                          __float_as_uint(dep[2]), __float_as_uint(dep[3]));
        if (IDS)
            streamStore16(p.writeThrough, p.ids + o, (uint32_t)id[0], (uint32_t)id[1], (uint32_t)id[2], (uint32_t)id[3]);
        if (NRM)
            streamStore16(p.writeThrough, p.normal + o, nrm[0], nrm[1], nrm[2], nrm[3]);
    } else {
#pragma unroll
        for (int b = 0; b < kRegionBlocks; ++b) {
            if (fx0 + b < p.nfast) {
                if (doRgb)
                    streamStore4(p.writeThrough, p.rgb + o + b, rgba[b]);
                if (doDepth)
                    streamStore4(p.writeThrough, p.depth + o + b, __float_as_uint(dep[b]));
                if (IDS)
                    streamStore4(p.writeThrough, p.ids + o + b, (uint32_t)id[b]);
                if (NRM)
                    streamStore4(p.writeThrough, p.normal + o + b, nrm[b]);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Worlds with more than 64 triangles: one workgroup = one 64x64 tile, the
// triangles go through LDS in passes of 256.  In a pass every wave sets up and
// classifies 64 triangles (lane = triangle) and publishes planes + region
// mask; after the barrier every wave rasterises its own two 64x8 strips
// against the 256 records and shades the pass's winners before the next pass
// replaces the records.  Large meshes proper are BVH territory.
// ---------------------------------------------------------------------------
constexpr int kPass = kChunk * kWavesPerBlock;    // triangles per pass

struct PassRecs {
    float shade[kPass][4];       // rgba, texture, objectID, world-local index
    float cold[kPass][kCold];    // u/v planes, lit colour
};
struct TileLds {
    float planes[kPass][16];     // A0 A1 A2 Dx | B0 B1 B2 Dy | C0 C1 C2 Dc | mask
    PassRecs rec;                // shading records
};
__device__ __forceinline__ const float *shadeRec(const PassRecs &L, int32_t w) { return L.shade[w]; }

// PV: per-view projection -- a workgroup renders one tile of one view: its record is uniform
// NRM: the normals form: the pass's packed normals in an LDS array of their own
template <bool IDS, bool PV, bool NRM = false>
__device__ __forceinline__ void chunkedKernelBody(const RasterParams p)
{
    __shared__ TileLds lds;
    __shared__ uint32_t nrmLds[NRM ? kPass : 1];
    touchKernelArguments();
    const int wave = threadIdx.x / kWave;
    const int lane = threadIdx.x % kWave;
    TileCtx t;
    ViewConst vc;
    ViewLight lt = {};
    if (!tileSetup<PV>(p, blockIdx.x, lane, t, vc, lt))
        return;                                   // whole workgroup leaves together
    // per-view projection: a wave-uniform runtime guard -- a workgroup renders one tile of one view
    const ViewProj pr = viewProjOf(p, PV, t.view);
    const float invNear = PV ? pr.invNear : p.invNear, invFar = p.invFar;

    // per-wave pixel state: strips 2*wave and 2*wave+1, two regions each
    float best[4][kRegionBlocks];
    int32_t bid[4][kRegionBlocks];
    uint32_t outRgba[4][kRegionBlocks];
    int32_t outId[4][kRegionBlocks];
    uint32_t outNrm[4][kRegionBlocks];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int b = 0; b < kRegionBlocks; ++b) {
            best[g][b] = invFar;
            bid[g][b] = -1;
            outRgba[g][b] = 0xFF000000u;
            outId[g][b] = -1;
            if (NRM)
                outNrm[g][b] = kNormalBackground;
        }

    for (uint32_t pass = 0; pass < t.numTris; pass += kPass) {
        if (pass != 0)
            __syncthreads();                      // previous pass fully consumed
        {
            const int rec = wave * kWave + lane;
            const uint32_t k = pass + (uint32_t)rec;
            TriPlanes c;
            zeroPlanes(c);
            uint32_t mask = 0;
            // whole waves past the end of the list skip the setup code
            if (pass + (uint32_t)(wave * kWave) < t.numTris) {
                bool valid = false;
                if (k < t.numTris && !(p.debugSkip & 8u)) {
                    const WorldTri wt = p.viewTris[t.triBegin + k];
                    if (NRM && PV)
                        valid = setupTriangleProj<IDS>(p, pr, lt, vc, wt, (int32_t)k, c, lds.rec.shade[rec], lds.rec.cold[rec],
                                                       NormalOut { nrmLds + rec });
                    else if (NRM)
                        valid = setupTriangle(p, vc, wt, (int32_t)k, c, lds.rec.shade[rec], lds.rec.cold[rec],
                                              NormalOut { nrmLds + rec });
                    else if (PV)
                        valid = setupTriangleProj<IDS>(p, pr, lt, vc, wt, (int32_t)k, c, lds.rec.shade[rec], lds.rec.cold[rec]);
                    else
                        valid = setupTriangle(p, vc, wt, (int32_t)k, c, lds.rec.shade[rec], lds.rec.cold[rec]);
                }
                if (valid && !(p.debugSkip & 4u))
                    mask = classifyRegions(c, t, invNear, invFar);
            }
            publishPlanes(lds.planes[rec], c, make_float4(__uint_as_float(mask), 0.f, 0.f, 0.f));   // the fourth: the mask
        }
        __syncthreads();

        const uint32_t left = t.numTris - pass;
        const int subs = left >= (uint32_t)kPass ? kWavesPerBlock : (int)((left + kWave - 1) / kWave);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int strip = 2 * wave + (g >> 1), hf = g & 1;
            const uint32_t fy = t.tileY0 + strip * 8 + t.ly;
            const float py = (float)fy;
            const uint32_t fx0 = t.tileX0 + hf * 32 + 4 * t.lx;
            float px[kRegionBlocks];
#pragma unroll
            for (int b = 0; b < kRegionBlocks; ++b)
                px[b] = (float)(fx0 + b);
            // lane k looks at the region mask of records k, 64 + k, ...; draw
            // order is record order, so the sub-chunks are visited in order
            for (int sub = 0; sub < subs; ++sub) {
                const uint32_t mask = __float_as_uint(lds.planes[sub * kWave + lane][12]);
                const uint64_t act = __ballot((mask >> (2 * strip + hf)) & 1u);
                if (!(p.debugSkip & 2u))
                    rasterRegion<true, 0>(lds.planes, act, sub * kWave, px, py, invNear, best[g], bid[g]);
            }
            // shade this pass's winners before its records are replaced
#pragma unroll
            for (int b = 0; b < kRegionBlocks; ++b) {
                if (bid[g][b] >= 0) {
                    resolvePixel<IDS>(p, lds.rec, bid[g][b], best[g][b], px[b], py,
                                      outRgba[g][b], outId[g][b]);
                    if (NRM)
                        outNrm[g][b] = nrmLds[bid[g][b]];
                }
                bid[g][b] = -1;
            }
        }
    }

#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int strip = 2 * wave + (g >> 1), hf = g & 1;
        const uint32_t fy = t.tileY0 + strip * 8 + t.ly;
        const uint32_t fx0 = t.tileX0 + hf * 32 + 4 * t.lx;
        if (NRM)
            outputRegion<IDS, true>(p, t, fx0, fy, invFar, best[g], outRgba[g], outId[g], outNrm[g]);
        else
            outputRegion<IDS>(p, t, fx0, fy, invFar, best[g], outRgba[g], outId[g]);
    }
}

template <bool IDS>
__global__ __launch_bounds__(kChunkedThreads, kChunkedWavesPerSimd)
void rasterChunkedKernel(const RasterParams p)
{
    chunkedKernelBody<IDS, false>(p);
}

// the form kernel: PV, N and NPV, as the brute kernel's
template <KernelForm F, bool IDS>
__global__ __launch_bounds__(kChunkedThreads, kChunkedWavesPerSimd)
void rasterChunkedFormKernel(const RasterParams p)
{
    static_assert(F == KernelForm::PV || F == KernelForm::N || F == KernelForm::NPV, "the forms of this family");
    chunkedKernelBody<IDS, formFlags(F).pv, formFlags(F).nrm>(p);
}

// ---------------------------------------------------------------------------
// Worlds of at most 256 triangles (every BASELINE scene): one workgroup renders
// a group of views (all their tiles) or a chunk of the tiles of one view.
//   S1  one lane per (view of the group, triangle slot): the setup waves
//       publish planes, bounding boxes and shading records in LDS (dense
//       lanes: four 14-triangle views fill 56 of wave 0's 64 lanes); the last
//       wave notes where the group's tiles lie and the order of the work items;
//   S2  one lane per (tile, triangle slot): wave w classifies four of the
//       tile's sixteen regions (strips 2(w&3), 2(w&3)+1), OR-ing bits into LDS;
//   R+O all waves pull (tile, strip) items off an LDS counter, rasterise the
//       strip's two regions and store them.
// ---------------------------------------------------------------------------
// (the group's limits -- kGroupTilesMax, kGroupSlotsMax, groupTilesMax -- and groupWaves: raster.hpp, beside the launch plan)

template <int SLOTS, bool PV = false>
struct GroupLds {
    static constexpr int kRecs = SLOTS <= kChunk ? kChunk + 16 : SLOTS;
    static constexpr int kBackground = kRecs;   // record index of "nothing hit"
    float planes[kRecs][16];            // A0 A1 A2 Dx | B0 B1 B2 Dy | C0 C1 C2 Dc | bbox
    uint32_t live[kRecs];               // record holds a triangle that can be visible
    float shade[kRecs + 1][4];          // rgba, texture, objectID, world-local index
    float cold[kRecs][kCold];           // u/v planes, lit colour
    // per (tile, slot of the tile's view): region bits 0..15, near-free bits 16..19
    uint32_t masks[groupTilesMax(SLOTS) * (SLOTS <= kChunk ? kChunk : SLOTS)];
    uint32_t tileInfo[kGroupTilesMax][4];   // view, x0, y0, flags | first record << 8
    float tileNear[PV ? kGroupTilesMax : 1];   // PV: 1/znear of each tile's view
    uint32_t nextItem;                  // (tile, strip) work counter of phase R
    uint8_t itemOrder[kGroupTilesMax * 8];  // work item -> tile * 8 + strip
    // FAST untextured kernels (16 slots, one-tile views): S2 writes each work item in the form phase R consumes --
    // x: surviving slots of the strip's left half (bits 0..15) and right half (16..31),
    // y: tile | strip << 4 | kItem* flags -- at its place in the work order (itemPos: tile * 8 + strip -> item)
    uint2 items[SLOTS == 16 ? kGroupTilesMax * 8 : 1];
    uint8_t itemPos[SLOTS == 16 ? kGroupTilesMax * 8 : 1];
};
constexpr uint32_t kTileValid = 4u;
constexpr uint32_t kItemValid = 1u << 8;      // the tile's view is part of the batch
constexpr uint32_t kItemNearFree = 1u << 9;   // every surviving slot stays behind the near plane over the strip
constexpr uint32_t kItemAnyTex = 1u << 10;    // a surviving slot of the strip is textured


// Shade + store one region of a tile (group kernel).  `bid` is the byte offset
// of the winner's shading record (the background has its own record, so the
// lookup is unconditional); base pointers are wave-uniform.
// OUT: output selection (raster.hpp OutSel); doRgb / doDepth = storesRgb / storesDepth of the kernel.
// NRM: the normals form: the winner's packed normal is one more dword found through the same
// offset, in the array `nrmTab` parallel to the records (the background's entry included), and one more store.
template <bool IDS, bool FULL, bool TEX, int OUT, bool NRM = false, typename LDS>
__device__ __forceinline__ void storeRegion(const RasterParams &p, const LDS &L, bool doRgb, bool doDepth,
                                            uint32_t *rgbTile, float *depthTile, int32_t *idsTile,
                                            uint32_t pixOff, uint32_t fx0, uint32_t fy,
                                            bool anyTex, const float (&px)[kRegionBlocks], float py,
                                            const float (&best)[kRegionBlocks],
                                            const int32_t (&bid)[kRegionBlocks],
                                            const uint32_t *nrmTab = nullptr, uint32_t *nrmTile = nullptr)
{
    uint32_t nrm[kRegionBlocks];
    if (NRM) {
#pragma unroll
        for (int b = 0; b < kRegionBlocks; ++b)
            nrm[b] = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(nrmTab) + (bid[b] >> 2));
    }
    uint32_t rgba[kRegionBlocks];
    int32_t id[kRegionBlocks];
    float dep[kRegionBlocks];
    const char *shadeBase = reinterpret_cast<const char *>(&L.shade[0][0]);
#pragma unroll
    for (int b = 0; b < kRegionBlocks; ++b) {
        const float *h = reinterpret_cast<const float *>(shadeBase + bid[b]);
        if (OUT != kOutDepth)
            rgba[b] = __float_as_uint(h[0]);
        if (IDS)
            id[b] = __float_as_int(p.idsAreSegmask ? h[2] : h[3]);
        // depth = 1/best: v_rcp_f32 (<= 1 ulp); textured colour below uses the
        // correctly rounded quotient because texel choice depends on it
        if (OUT != kOutRGB)
            dep[b] = bid[b] != LDS::kBackground * 16 ? __builtin_amdgcn_rcpf(best[b]) : 0.0f;
    }
    // TEX is a kernel-level switch: texel loads inside the work loop make the
    // compiler drain vmcnt at every loop header, which would also wait for the
    // previous strip's stores -- and so is the output selection of the kernels that
    // carry the shipped configurations: a depth-only instantiation has no texel load
    if (TEX && OUT != kOutDepth && anyTex && (OUT != kOutByPointer || doRgb)) {
#pragma unroll
        for (int b = 0; b < kRegionBlocks; ++b) {
            const int32_t rec = bid[b] >> 4;
            const int32_t tex = __float_as_int(L.shade[rec][1]);
            if (tex >= 0)
                rgba[b] = shadeTextured(p, L.cold[rec], tex, px[b], py, 1.0f / best[b]);
        }
    }
    if (p.debugSkip & 1u)
        return;
    if (FULL) {
        if (doRgb)
            streamStore16(p.writeThrough, rgbTile + pixOff, rgba[0], rgba[1], rgba[2], rgba[3]);
        if (doDepth)
            streamStore16(p.writeThrough, depthTile + pixOff, __float_as_uint(dep[0]), __float_as_uint(dep[1]),
                          __float_as_uint(dep[2]), __float_as_uint(dep[3]));
        if (IDS)
            streamStore16(p.writeThrough, idsTile + pixOff, (uint32_t)id[0], (uint32_t)id[1], (uint32_t)id[2], (uint32_t)id[3]);
        if (NRM)
            streamStore16(p.writeThrough, nrmTile + pixOff, nrm[0], nrm[1], nrm[2], nrm[3]);
    } else if (fy < p.nslow) {
#pragma unroll
        for (int b = 0; b < kRegionBlocks; ++b) {
            if (fx0 + b < p.nfast) {
                if (doRgb)
                    streamStore4(p.writeThrough, rgbTile + pixOff + b, rgba[b]);
                if (doDepth)
                    streamStore4(p.writeThrough, depthTile + pixOff + b, __float_as_uint(dep[b]));
                if (IDS)
                    streamStore4(p.writeThrough, idsTile + pixOff + b, (uint32_t)id[b]);
                if (NRM)
                    streamStore4(p.writeThrough, nrmTile + pixOff + b, nrm[b]);
            }
        }
    }
}

// A region no triangle can touch: background everywhere, no per-pixel work.
template <bool IDS, bool FULL, bool NRM = false>
__device__ __forceinline__ void storeBackground(const RasterParams &p, bool doRgb, bool doDepth, uint32_t *rgbTile,
                                                float *depthTile, int32_t *idsTile,
                                                uint32_t pixOff, uint32_t fx0, uint32_t fy, uint32_t *nrmTile = nullptr)
{
    if (p.debugSkip & 1u)
        return;
    const uint32_t bg = 0xFF000000u;
    if (FULL) {
        if (doRgb)
            streamStore16(p.writeThrough, rgbTile + pixOff, bg, bg, bg, bg);
        if (doDepth)
            streamStore16(p.writeThrough, depthTile + pixOff, 0u, 0u, 0u, 0u);
        if (IDS)
            streamStore16(p.writeThrough, idsTile + pixOff, ~0u, ~0u, ~0u, ~0u);
        if (NRM)
            streamStore16(p.writeThrough, nrmTile + pixOff, kNormalBackground, kNormalBackground, kNormalBackground,
                          kNormalBackground);
    } else if (fy < p.nslow) {
#pragma unroll
        for (int b = 0; b < kRegionBlocks; ++b) {
            if (fx0 + b < p.nfast) {
                if (doRgb)
                    streamStore4(p.writeThrough, rgbTile + pixOff + b, bg);
                if (doDepth)
                    streamStore4(p.writeThrough, depthTile + pixOff + b, 0u);
                if (IDS)
                    streamStore4(p.writeThrough, idsTile + pixOff + b, ~0u);
                if (NRM)
                    streamStore4(p.writeThrough, nrmTile + pixOff + b, kNormalBackground);
            }
        }
    }
}

// S2 of the group kernel for one (tile j, triangle slot k) pair: the region bits of the wave's two strips
// (bit 2 * strip + half), whether the triangle stays behind the near plane over them and whether it is
// textured; nothing for a dead slot or a view past the end of the batch.
template <typename LDS>
__device__ __forceinline__ uint32_t classifyPair(const LDS &L, int j, int k, int wave, float invNear, float invFar,
                                                 bool &nearOk, bool &tex)
{
    nearOk = false;
    tex = false;
    const uint32_t info = L.tileInfo[j][3];
    const int rec = (int)(info >> 8) + k;
    if (!(info & kTileValid) || !L.live[rec])
        return 0u;
    const float4 *src = reinterpret_cast<const float4 *>(L.planes[rec]);
    const float4 a = src[0], b = src[1], cc = src[2], bb = src[3];
    TriPlanes c;
    c.A0 = a.x; c.A1 = a.y; c.A2 = a.z; c.Dx = a.w;
    c.B0 = b.x; c.B1 = b.y; c.B2 = b.z; c.Dy = b.w;
    c.C0 = cc.x; c.C1 = cc.y; c.C2 = cc.z; c.Dc = cc.w;
    c.bbX0 = bb.x; c.bbX1 = bb.y; c.bbY0 = bb.z; c.bbY1 = bb.w;
    const uint32_t tx0 = L.tileInfo[j][1], ty0 = L.tileInfo[j][2];
    uint32_t m;
    switch (wave & 3) {
    case 0: m = classifyStrips<0, 2>(c, tx0, ty0, invNear, invFar, nearOk); break;
    case 1: m = classifyStrips<2, 4>(c, tx0, ty0, invNear, invFar, nearOk); break;
    case 2: m = classifyStrips<4, 6>(c, tx0, ty0, invNear, invFar, nearOk); break;
    default: m = classifyStrips<6, 8>(c, tx0, ty0, invNear, invFar, nearOk); break;
    }
    tex = __float_as_int(L.shade[rec][1]) >= 0;
    return m;
}

// XMODE (16-slot instantiations only): bit 0 = the workgroups of every pair trade places
// (XCD phase, below), bit 1 = workgroup 0 reports the XCD it runs on.  Separate
// instantiations, chosen per launch by the host, because any extra state in this kernel's
// work loop costs more than the split gains (59 of 64 VGPRs, SGPRs spilled): XMODE 0 is
// the kernel as it always was.
// FAST (16-slot instantiations; chosen by the host for uniform worlds of one-tile views without diagnostics): the
// set-up waves' path to their first pose loads reads nothing but the twelve leading header arguments (GroupHeader,
// raster.hpp), which the command processor preloads into SGPRs (-mllvm -amdgpu-kernarg-preload-count=12): the loads
// go out without a round trip to the argument block; `p` is read for what comes after.
// OUT (raster.hpp OutSel): the output selection of the instantiation.
// PV: per-view projection: the set-up lanes read their view's record, S2 and phase R the 1/znear of
// each tile's view, which the last wave leaves in LDS beside the tile's place.
// LT (with PV): the worlds' lights differ too: the set-up lanes read their view's light record beside
// the camera; without it the per-view form takes the uniform light of the kernel arguments.
// COL: per-instance colour override: the set-up lanes read their row's packed colour beside its ObjectID.
// MAT (with COL): per-instance material override: they read the row's material id too; the colour
// column is then the slot of the pose block -- zero-filled in a renderer that has the material column alone.
// NRM: the normals form (instantiated with COL and MAT, output selection by pointer and XMODE 0):
// the set-up lanes pack their triangle's normal into an LDS array parallel to the shading records, phase R + O stores
// one more tensor.  The colour and material columns are read behind null tests, and the XCD trade and report are
// run-time tests of p.xcdPhase / p.xccReport here, so that two forms (uniform constants, per-view tables) cover
// every renderer with the output.
// LAB: the label form (instantiated with IDS, PV, LT, COL and MAT, output selection by pointer and
// XMODE 0, with and without NRM): the set-up lanes read their row's label beside its ObjectID and write S11's value into
// the record's label slot.  Everything optional is taken as the normals form takes it: the colour and material columns
// behind null tests, the XCD trade and report at run time, so one form per family and normals setting covers every
// renderer with the column (which always launches with the per-view tables filled).
// What an instantiation of the body is: the settings above by name.  GroupKindOf makes a type of one (C++17 has no
// class-type template arguments) from the parameters the entries have themselves; the form's flags come from formFlags.
struct GroupKind {
    bool ids;
    int slots;
    bool tex;
    int xmode;
    bool fast;
    int out;
    FormFlags form;
};
template <KernelForm F, bool IDS, int SLOTS, bool TEX, int XMODE, bool FAST, int OUT>
struct GroupKindOf {
    static constexpr GroupKind value()
    {
        GroupKind k {};
        k.ids = IDS;
        k.slots = SLOTS;
        k.tex = TEX;
        k.xmode = XMODE;
        k.fast = FAST;
        k.out = OUT;
        k.form = formFlags(F);
        return k;
    }
};

template <typename KIND>
__device__ __forceinline__ void groupKernelBody(const char *hPose, const char *hGeom, uint32_t hViews, uint32_t hInstances,
                                                uint32_t hPool, uint32_t hShape, uint32_t hGroups, uint32_t hPrefix,
                                                uint32_t hFirst01, uint32_t hFirst23, const RasterParams p)
{
    constexpr GroupKind K = KIND::value();
    constexpr bool IDS = K.ids, TEX = K.tex, FAST = K.fast;
    constexpr int SLOTS = K.slots, XMODE = K.xmode, OUT = K.out;
    constexpr bool PV = K.form.pv, LT = K.form.lt, COL = K.form.col, MAT = K.form.mat, NRM = K.form.nrm, LAB = K.form.lab;
    __shared__ GroupLds<SLOTS, PV> lds;
    constexpr int kBackground = GroupLds<SLOTS, PV>::kBackground;
    __shared__ uint32_t nrmLds[NRM ? GroupLds<SLOTS, PV>::kRecs + 1 : 1];   // [record], the background's last
    // readfirstlane: the compiler cannot see that threadIdx.x / 64 is
    // wave-uniform and would predicate every `wave` branch instead of jumping
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const int lane = threadIdx.x % kWave;
    // (FAST: the set-up waves -- 0 and 1 -- have what they need in SGPRs and must not wait for the argument block;
    // the other waves touch it for the whole CU, whose scalar cache they share)
    if (!FAST || wave >= 2)
        touchKernelArguments<(FAST ? 48 : 0) + sizeof(RasterParams)>();
    // ==== arguments ====  what the prologue reads: from the preloaded header (FAST) or from `p`
    const uint32_t aNumViews = FAST ? hViews : p.numViews;
    const uint32_t aGrpViews = FAST ? hdrGrpViews(hShape) : p.grpViews;
    const uint32_t aXcdSkew = FAST ? hdrXcdSkew(hShape) : p.xcdSkew;
    const uint32_t aXcdRotate = FAST ? hdrXcdRotate(hShape) : p.xcdRotate;
    const uint32_t aGrpPerView = FAST ? 1u : p.grpPerView;
    const uint32_t aGrid = FAST ? hGroups : gridDim.x;
    const uint32_t aUniInstances = FAST ? hdrUniInstances(hShape) : p.uniInstances;
    const uint32_t aUniCams = FAST ? hdrUniCams(hShape) : p.uniCamsPerWorld;
    const uint32_t dskip = FAST ? 0u : p.debugSkip;           // (the host never picks FAST with diagnostics on)
    const PoseLayout lay = poseLayout(hViews, hInstances);
    const float *aCamRot = FAST ? reinterpret_cast<const float *>(hPose + lay.camRot) : p.camRot;
    const float *aCamPos = FAST ? reinterpret_cast<const float *>(hPose + lay.camPos) : p.camPos;
    const int32_t *aInstObj = FAST ? reinterpret_cast<const int32_t *>(hPose + lay.instObj) : p.instObj;
    // (NRM, LAB: whichever columns the renderer has -- null without)
    constexpr bool BYPTR = NRM || LAB;
    const uint32_t *aInstColor = BYPTR ? p.instColor
                                 : FAST ? reinterpret_cast<const uint32_t *>(hPose + lay.total)
                                 : MAT ? reinterpret_cast<const uint32_t *>(p.poseBlock + poseColorOffset(p.numViews, p.numInstances))
                                       : p.instColor;
    const int32_t *aInstMat = BYPTR ? p.instMat
                              : FAST ? reinterpret_cast<const int32_t *>(hPose + lay.total + mrxAlign256(hInstances * 4u))
                                     : p.instMat;
    const uint32_t tilesPerView = FAST ? 1u : p.tilesFast * p.tilesSlow;
    // FAST, untextured (16 slots, one-tile views): S2 hands phase R ready-made work items (GroupLds::items).
    // The plain entry and the textured kernels keep the per-tile masks: measured slower with the items
    //  -- the plain entry carries both loops, the textured one lost its register budget.
    constexpr bool readyItems = FAST && !TEX;
    // ==== ownership ====  which views / tiles this workgroup owns (groupPlan, raster.hpp):
    //  A  grpPerView == 1: grpViews whole views (all their tiles);
    //  B  otherwise: grpChunkTiles tiles of one view.
    uint32_t firstView, groupViews, firstTile, groupTiles;
    // Workgroup b runs on XCD b % 8.  With xcdRotate the group it renders moves
    // two places on within its round of eight, round after round, so that an
    // XCD does not keep writing the same eighth of every 512 KiB of the output
    // (parity is kept: the XCD-aware split below pairs even with odd groups).
    // Which XCD a launch's workgroup 0 lands on depends on the hardware queue and what
    // ran on it before (measured: XCC 0, 6 or 7 for different streams of one process,
    // stable from launch to launch; profiles/r02_xcd_phase.txt).  On an odd start the
    // XCD-aware split below would move its strips the wrong way (24.9 instead of 22.5
    // us), so the two workgroups of every pair trade places then (XMODE bit 0): the host
    // picks the instantiation by the parity workgroup 0 reported in an earlier launch
    // of this renderer -- every workgroup of a launch runs the same code, so the trade
    // is consistent whatever the hardware does; a stale value costs speed, never pixels.
    const uint32_t blk = ((BYPTR ? (p.xcdPhase & 1u) != 0u : (XMODE & 1) != 0) && SLOTS == 16 && aXcdSkew && (blockIdx.x ^ 1u) < aGrid)
                             ? blockIdx.x ^ 1u : blockIdx.x;
    // workgroup 0 reports where it runs: a host-mapped word, written by the last wave,
    // which issues no loads during set-up -- the slow write sits ahead of nothing
    if (((XMODE & 2) || (BYPTR && SLOTS == 16)) && blockIdx.x == 0 && threadIdx.x == (groupWaves(TEX) - 1) * kWave && p.xccReport)
        *p.xccReport = __builtin_amdgcn_s_getreg((3 << 11) | 20);   // HW_REG_XCC_ID[3:0]
    uint32_t bid = blk;
    if (aXcdRotate && (bid | 7u) < aGrid)
        bid = (bid & ~7u) | ((bid + 2u * (bid >> 3)) & 7u);
    if (aGrpPerView == 1) {
        firstView = bid * aGrpViews;
        groupViews = aGrpViews;
        firstTile = 0;
        groupTiles = groupViews * tilesPerView;
    } else {
        firstView = bid / aGrpPerView;
        groupViews = 1;
        firstTile = (bid - firstView * aGrpPerView) * p.grpChunkTiles;
        groupTiles = min(p.grpChunkTiles, tilesPerView - firstTile);
    }
    // XCD-aware split (see groupPlan; one-tile views, four per group):
    // consecutive workgroups run on consecutive XCDs and the odd XCD of each pair
    // drains its stores more slowly.  Workgroups 2m and 2m+1 (after the trade above:
    // even = on an even XCD) share the view between their two runs of four: the odd
    // one leaves its first p.xcdSkew strips to the even one (both set the view up).
    uint32_t firstStrip = 0, numStrips = groupTiles * 8;
    if (SLOTS == 16 && aXcdSkew) {
        if (blk & 1u) {
            firstStrip = aXcdSkew;
            numStrips -= aXcdSkew;
        } else {
            groupViews += 1;
            groupTiles += 1;
            numStrips += aXcdSkew;
        }
    }
    const int groupRecs = (int)groupViews * SLOTS;
    const int numPairs = (int)groupTiles * SLOTS;
    const float invNear = p.invNear, invFar = p.invFar;
    if (dskip & 16u)
        return;                                   // timing aid: bare launch
    unsigned long long *stamps = (!FAST && p.debugStamps && wave < 4)
        ? p.debugStamps + ((size_t)blockIdx.x * 4 + wave) * 8 : nullptr;
#define MRX_STAMP(i)                                                           \
    do {                                                                       \
        if (stamps && lane == 0)                                               \
            stamps[i] = __builtin_amdgcn_s_memrealtime();                      \
    } while (0)
    MRX_STAMP(0);
    if (!readyItems)
        for (int i = threadIdx.x; i < numPairs; i += groupWaves(TEX) * kWave)
            lds.masks[i] = 0u;

    // ==== S1: tile notes and item order (the last wave) ====
    //      S1 is one lane per (view vi of the group, triangle slot k): setup.
    //      Wave 0 covers the first 64 records, wave 1 a fifth 16-slot view or
    //      the next 64 slots of a large view, ...  Meanwhile the last wave
    //      notes where each tile of the group lies.
    if (wave == groupWaves(TEX) - 1 && lane < (int)groupTiles) {
        uint32_t vi = (uint32_t)lane, tile = firstTile;
        if (tilesPerView != 1) {
            vi = groupViews == 1 ? 0u : (uint32_t)lane / tilesPerView;
            tile = firstTile + (uint32_t)lane - vi * tilesPerView;
        }
        const uint32_t ty = tilesPerView != 1 ? tile / p.tilesFast : 0u;
        lds.tileInfo[lane][0] = firstView + vi;
        lds.tileInfo[lane][1] = (tile - ty * p.tilesFast) * 64u;
        lds.tileInfo[lane][2] = ty * 64u;
        lds.tileInfo[lane][3] = (firstView + vi < aNumViews ? kTileValid : 0u) | ((vi * SLOTS) << 8);
        if (PV)
            lds.tileNear[lane] = firstView + vi < aNumViews ? viewProjOf(p, true, firstView + vi).invNear : 0.0f;
    }
    // ... and the order of the work items.  One-tile views: strip by strip
    // across the views, top strips first -- strips above the horizon cost
    // nothing, so every wave has stores in flight right after the barrier.
    // Larger views: tile by tile (switching tiles per item costs more there).
    if (wave == groupWaves(TEX) - 1) {
        uint32_t base = 0;
        for (uint32_t c0 = 0; c0 < groupTiles * 8u; c0 += kWave) {
            const uint32_t c = c0 + (uint32_t)lane;
            uint32_t strip = c / groupTiles, tile = c - strip * groupTiles;
            if (tilesPerView != 1) {
                tile = c >> 3;
                strip = c & 7u;
            }
            const uint32_t g = tile * 8u + strip;
            const bool ok = strip < 8u && g >= firstStrip && g < firstStrip + numStrips;
            const uint64_t m = __ballot(ok);
            const uint32_t pos = base + __builtin_popcountll(m & ((1ull << lane) - 1ull));
            if (readyItems) {
                if (strip < 8u)                   // every (tile, strip) of the group: its item, or none
                    lds.itemPos[g] = ok ? (uint8_t)pos : (uint8_t)0xFF;
            } else if (ok) {
                lds.itemOrder[pos] = (uint8_t)g;
            }
            base += (uint32_t)__builtin_popcountll(m);
        }
    }
    // ==== S1: set-up per record ====
    if (wave * kWave < groupRecs) {
        const int rec = wave * kWave + lane;
        const int vi = rec / SLOTS, k = rec % SLOTS;
        const bool recOk = rec < groupRecs;
        const bool viewOk = recOk && firstView + vi < aNumViews;
        const uint32_t view = viewOk ? firstView + vi : 0u;
        // everything addressed by the view index is requested up front; the
        // pose / geometry rows one level down follow as soon as wt arrives --
        // or at once, when the draw list is arithmetic (uniform worlds)
        WorldTri wt;
        uint32_t numTris;
        if (aUniInstances) {
            const uint32_t kk = (uint32_t)k;
            // (FAST: the table rides in the header, eight / sixteen bits per entry)
            const uint32_t pre1 = FAST ? hdrPrefix(hPrefix, 1) : p.uniPrefix[1], pre2 = FAST ? hdrPrefix(hPrefix, 2) : p.uniPrefix[2];
            const uint32_t pre3 = FAST ? hdrPrefix(hPrefix, 3) : p.uniPrefix[3], pre4 = FAST ? hdrPrefix(hPrefix, 4) : p.uniPrefix[4];
            const uint32_t ft0 = FAST ? hdrFirst(hFirst01, 0) : p.uniFirstTri[0], ft1 = FAST ? hdrFirst(hFirst01, 1) : p.uniFirstTri[1];
            const uint32_t ft2 = FAST ? hdrFirst(hFirst23, 2) : p.uniFirstTri[2], ft3 = FAST ? hdrFirst(hFirst23, 3) : p.uniFirstTri[3];
            const uint32_t li = (kk >= pre1 ? 1u : 0u) + (kk >= pre2 ? 1u : 0u) + (kk >= pre3 ? 1u : 0u);
            const uint32_t pre = li == 0 ? 0u : li == 1 ? pre1 : li == 2 ? pre2 : pre3;
            const uint32_t first = li == 0 ? ft0 : li == 1 ? ft1 : li == 2 ? ft2 : ft3;
            // integer divisions cost ~25 VALU each: a real (scalar) branch
            // around this one for the common one-camera-per-world case
            uint32_t world = view;
            if (aUniCams != 1)
                world = view / aUniCams;
            wt.inst = world * aUniInstances + li;
            wt.tri = first + (kk - pre);
            numTris = viewOk ? pre4 : 0u;
            if (kk >= pre4) {                     // idle slot: keep the loads in range
                wt.inst = 0;
                wt.tri = 0;
            }
        } else {
            // slots past the view's row are idle: keep their load inside the row
            wt = p.viewTris[view * p.viewTriStride + ((uint32_t)k < p.viewTriStride ? (uint32_t)k : 0u)];
            numTris = viewOk ? p.viewTriCount[view] : 0u;
        }
        ViewConst vc;
        // (LT: the light of the lane's view, a vector load beside the camera's -- the lanes span views)
        const ViewLight lt = viewLightOf(p, PV && LT, view);
        {
            const float4 q = *reinterpret_cast<const float4 *>(aCamRot + 4 * view);
            quatToMat(q.x, q.y, q.z, q.w, vc.Rc);
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                vc.c[r] = aCamPos[3 * view + r];
                vc.lv[r] = dot3(vc.Rc[0][r], vc.Rc[1][r], vc.Rc[2][r],
                                lt.toLight[0], lt.toLight[1], lt.toLight[2]);
            }
        }
        TriPlanes c;
        zeroPlanes(c);
        bool valid = false;
        MRX_STAMP(1);
        if (recOk) {
            lds.shade[rec][1] = __int_as_float(-1);
            if ((uint32_t)k < numTris && !(dskip & 8u)) {
                // the pose / geometry rows through pointers that come from the header (FAST) or from `p`
                const ViewProj pr = viewProjOf(p, PV, view);
                const GroupSetupArgs sa = {
                    FAST ? reinterpret_cast<const ObjTri *>(hGeom) : p.tris,
                    FAST ? reinterpret_cast<const TriMat *>(hGeom + geomMatsOffset(hPool)) : p.triMats,
                    FAST ? reinterpret_cast<const float *>(hPose + lay.instPos) : p.instPos,
                    FAST ? reinterpret_cast<const float *>(hPose + lay.instRot) : p.instRot,
                    FAST ? reinterpret_cast<const float *>(hPose + lay.instScale) : p.instScale,
                    pr.sx, pr.ox, pr.sz, pr.oz, pr.s6bPad, lt.ambient, lt.diffuse, p.transposed };
                InstXform x;
                instanceTransform(sa, vc, wt.inst, x);
                // one dispatch: the by-pointer forms (NRM, LAB) take every column behind a null test and set everything up,
                // the others what their parameters name; NRM: the packed normal goes to the array beside the records
                const MatOverride mo = { BYPTR ? (aInstMat ? aInstMat[wt.inst] : -1) : MAT ? aInstMat[wt.inst] : -1,
                                         p.numMaterials, p.matTable };
                const auto nrmOut = [&] {
                    if constexpr (NRM)
                        return NormalOut { nrmLds + rec };
                    else
                        return NoNormalOut {};
                }();
                valid = setupTriangleCore<true, BYPTR || OUT != kOutDepth, BYPTR || COL, BYPTR || MAT>(
                    sa, vc.lv, x, wt.tri, aInstObj[wt.inst], k, c, lds.shade[rec], lds.cold[rec],
                    BYPTR ? (aInstColor ? aInstColor[wt.inst] : 0u) : COL ? aInstColor[wt.inst] : 0u, mo, nrmOut);
                if (LAB)
                    applyLabel(lds.shade[rec], p.instLabel, wt.inst);
            }
            MRX_STAMP(2);
            publishPlanes(lds.planes[rec], c, make_float4(c.bbX0, c.bbX1, c.bbY0, c.bbY1));       // the fourth: the box
            lds.live[rec] = (valid && !(dskip & 4u)) ? 1u : 0u;
        }
        if (rec == 0) {
            lds.nextItem = 0;
            lds.shade[kBackground][0] = __uint_as_float(0xFF000000u);
            lds.shade[kBackground][1] = __int_as_float(-1);
            lds.shade[kBackground][2] = __int_as_float(-1);
            lds.shade[kBackground][3] = __int_as_float(-1);
            if (NRM)
                nrmLds[kBackground] = kNormalBackground;
        }
    }
    __syncthreads();
    MRX_STAMP(3);

    // ==== S2: ready items | masks ====
    //      classification of every (tile, triangle slot) pair against the
    //      tile's sixteen 32x8 regions.  Wave w takes strips 2(w&3), 2(w&3)+1
    //      (four regions) of the pairs (w>>2)*64 + lane, + 64 * (waves / 4), ...;
    //      results are OR-ed in LDS: bits 0..15 regions, bits 16..19
    //      "near-free over this wave's strips".
    //      readyItems: a pass of a wave covers four whole tiles (lane = 16 * tile + slot), so the
    //      wave assembles its strips' work items (GroupLds::items) by ballot instead.
    constexpr int kPairStride = (groupWaves(TEX) / 4) * kWave;
    for (int pair = (wave >> 2) * kWave + lane; pair - lane < numPairs; pair += kPairStride) {
        if (readyItems) {
            uint32_t m = 0;
            bool nearOk = false, tex = false;
            if (pair < numPairs)
                m = classifyPair(lds, pair / SLOTS, pair % SLOTS, wave, PV ? lds.tileNear[pair / SLOTS] : invNear, invFar,
                                 nearOk, tex);
            m >>= 4 * (wave & 3);                 // bit 2i + hf: strip 2 (wave & 3) + i, half hf
            const uint64_t l0 = __ballot(m & 1u), r0 = __ballot(m & 2u), l1 = __ballot(m & 4u), r1 = __ballot(m & 8u);
            const uint64_t near0 = __ballot((m & 3u) && !nearOk), near1 = __ballot((m & 12u) && !nearOk);
            const uint64_t tex0 = __ballot((m & 3u) && tex), tex1 = __ballot((m & 12u) && tex);
            if (lane % 16 == 0 && pair < numPairs) {
                // lane 16 t: tile j = pair / 16, its slots are bits 16 t .. 16 t + 15 of the ballots
                const uint32_t j = (uint32_t)pair / 16u;
                const uint32_t valid = firstView + j < aNumViews ? kItemValid : 0u;
                const auto put = [&](uint32_t strip, uint64_t l, uint64_t r, uint64_t nearHit, uint64_t texHit) {
                    const uint32_t pos = lds.itemPos[j * 8u + strip];
                    if (pos == 0xFFu)
                        return;                   // left to the other workgroup of the pair (XCD-aware split)
                    const uint32_t desc = j | strip << 4 | valid |
                                          (((nearHit >> lane) & 0xFFFFu) == 0 ? kItemNearFree : 0u) |
                                          (((texHit >> lane) & 0xFFFFu) != 0 ? kItemAnyTex : 0u);
                    lds.items[pos] = make_uint2((uint32_t)((l >> lane) & 0xFFFFu) | (uint32_t)((r >> lane) & 0xFFFFu) << 16,
                                                desc);
                };
                put(2u * (wave & 3), l0, r0, near0, tex0);
                put(2u * (wave & 3) + 1u, l1, r1, near1, tex1);
            }
            continue;
        }
        if (pair >= numPairs)
            continue;
        bool nearOk, tex;
        uint32_t m = classifyPair(lds, pair / SLOTS, pair % SLOTS, wave, PV ? lds.tileNear[pair / SLOTS] : invNear,
                                  invFar, nearOk, tex);
        if (nearOk)
            m |= 1u << (16 + (wave & 3));
        if (m)
            atomicOr(&lds.masks[pair], m);
    }
    __syncthreads();
    MRX_STAMP(4);

    // ==== R + O: item fetch (ready items | tile masks), then the strip's two regions ====
    //      the four waves pull (tile, strip) work items off an LDS
    //      counter -- strips differ a lot in cost (sky vs. ground vs. objects),
    //      a static split leaves waves idle
    // lane -> four consecutive pixels of one row of a 32x8 region (a 64x4
    // region with fully linear 1 KiB stores was measured slower: no x culling)
    const int lx = lane & 7, ly = lane >> 3;
    const uint32_t laneOff = (uint32_t)ly * p.nfast + 4u * lx;
    int cachedTile = -1, recBase = 0;
    constexpr int SUBS = (SLOTS + kWave - 1) / kWave;     // 64-slot sub-chunks of a view
    constexpr int LANES = SLOTS < kWave ? SLOTS : kWave;
    uint32_t view = 0, tileX0 = 0, tileY0 = 0, mask[SUBS] = {};
    float pxTile[2][kRegionBlocks] = {};
    bool anyTex = false, nearFree = false, full = false;
    uint32_t *rgbTile = nullptr;
    float *depthTile = nullptr;
    int32_t *idsTile = nullptr;
    uint32_t *nrmTile = nullptr;
    const bool doRgb = storesRgb<OUT>(p.rgb), doDepth = storesDepth<OUT>(p.depth);
    uint32_t itemMasks = 0;     // readyItems: the item's surviving slots, left half bits 0..15, right half 16..31
    float tileNear = invNear;   // 1/znear of the item's view (PV: from LDS, tile by tile)
    if (readyItems) {
        // the tile of a one-tile view sits at the view's origin: what depends on the tile origin is set once
        full = (p.nfast & 3u) == 0 && 64u <= p.nfast && 64u <= p.nslow;
#pragma unroll
        for (int hf = 0; hf < 2; ++hf)
#pragma unroll
            for (int b = 0; b < kRegionBlocks; ++b)
                pxTile[hf][b] = (float)(hf * 32 + 4 * lx + b);
    }
    for (;;) {
        uint32_t item = 0;
        if (lane == 0)
            item = atomicAdd(&lds.nextItem, 1u);
        item = __builtin_amdgcn_readfirstlane(item);
        if (item >= numStrips)
            break;
        int j, strip;
        if (readyItems) {
            // one ticket, one 8-byte read: the item is ready to go
            const uint2 d = lds.items[item];
            itemMasks = __builtin_amdgcn_readfirstlane(d.x);
            const uint32_t desc = __builtin_amdgcn_readfirstlane(d.y);
            if (!(desc & kItemValid))
                continue;                           // a view past the end of the batch
            j = (int)(desc & 15u);
            strip = (int)((desc >> 4) & 7u);
            nearFree = (desc & kItemNearFree) != 0;
            anyTex = (desc & kItemAnyTex) != 0;
            recBase = j * SLOTS;
            if (PV)
                tileNear = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(lds.tileNear[j])));
            const size_t tileBase = (size_t)(firstView + (uint32_t)j) * p.nslow * p.nfast;
            rgbTile = p.rgb + tileBase;
            depthTile = p.depth + tileBase;
            idsTile = IDS ? p.ids + tileBase : nullptr;
            nrmTile = NRM ? p.normal + tileBase : nullptr;
        } else {
            item = __builtin_amdgcn_readfirstlane((uint32_t)lds.itemOrder[item]);
            j = (int)(item >> 3);
            strip = (int)(item & 7u);
            if (j != cachedTile) {
                const uint32_t info = __builtin_amdgcn_readfirstlane(lds.tileInfo[j][3]);
                if (!(info & kTileValid))
                    continue;                           // a view past the end of the batch
                cachedTile = j;
                recBase = (int)(info >> 8);
                view = __builtin_amdgcn_readfirstlane(lds.tileInfo[j][0]);
                tileX0 = __builtin_amdgcn_readfirstlane(lds.tileInfo[j][1]);
                tileY0 = __builtin_amdgcn_readfirstlane(lds.tileInfo[j][2]);
                if (PV)
                    tileNear = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(lds.tileNear[j])));
                const size_t tileBase = ((size_t)view * p.nslow + tileY0) * p.nfast + tileX0;
                rgbTile = p.rgb + tileBase;
                depthTile = p.depth + tileBase;
                idsTile = IDS ? p.ids + tileBase : nullptr;
                nrmTile = NRM ? p.normal + tileBase : nullptr;
                full = (p.nfast & 3u) == 0 && tileX0 + 64u <= p.nfast && tileY0 + 64u <= p.nslow;
                // lane k looks at the region masks of triangle slots k, 64 + k, ... of tile j
                anyTex = false;
                nearFree = true;
#pragma unroll
                for (int sub = 0; sub < SUBS; ++sub) {
                    const int slot = sub * kWave + lane;
                    mask[sub] = lane < LANES ? lds.masks[j * SLOTS + slot] : 0u;
                    const int32_t tex = lane < LANES ? __float_as_int(lds.shade[recBase + slot][1]) : -1;
                    anyTex = anyTex || __ballot((mask[sub] & 0xFFFFu) != 0 && tex >= 0) != 0;
                    // every surviving triangle stays behind the near plane over the
                    // whole tile: the per-pixel near test is dropped for the tile
                    nearFree = nearFree &&
                               __ballot((mask[sub] & 0xFFFFu) != 0 && ((mask[sub] >> 16) & 0xFu) != 0xFu) == 0;
                }
#pragma unroll
                for (int hf = 0; hf < 2; ++hf)
#pragma unroll
                    for (int b = 0; b < kRegionBlocks; ++b)
                        pxTile[hf][b] = (float)(tileX0 + hf * 32 + 4 * lx + b);
            }
        }
        // ==== R + O: the regions of the item ====
        const uint32_t fy = tileY0 + strip * 8 + ly;
        const float py = (float)fy;
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const uint32_t fx0 = tileX0 + hf * 32 + 4 * lx;
            const uint32_t pixOff = (uint32_t)(strip * 8) * p.nfast + hf * 32 + laneOff;
            // bit k of act[sub]: triangle slot 64 sub + k of the tile's view survives here
            uint64_t act[SUBS];
            bool any = false;
#pragma unroll
            for (int sub = 0; sub < SUBS; ++sub) {
                act[sub] = readyItems ? (uint64_t)((itemMasks >> (16 * hf)) & 0xFFFFu)
                                     : __ballot((mask[sub] >> (2 * strip + hf)) & 1u);
                any = any || act[sub] != 0;
            }
            if (!any) {
                if (full)
                    storeBackground<IDS, true, NRM>(p, doRgb, doDepth, rgbTile, depthTile, idsTile, pixOff, fx0, fy, nrmTile);
                else
                    storeBackground<IDS, false, NRM>(p, doRgb, doDepth, rgbTile, depthTile, idsTile, pixOff, fx0, fy, nrmTile);
                continue;
            }
            const float (&px)[kRegionBlocks] = pxTile[hf];
            float best[kRegionBlocks];
            int32_t bid[kRegionBlocks];
#pragma unroll
            for (int b = 0; b < kRegionBlocks; ++b) {
                best[b] = invFar;
                bid[b] = kBackground * 16;
            }
            if (!(dskip & 2u)) {
#pragma unroll
                for (int sub = 0; sub < SUBS; ++sub) {
                    if (SUBS > 1 && act[sub] == 0)
                        continue;
                    if (nearFree)
                        rasterRegion<false, 4>(lds.planes, act[sub], recBase + sub * kWave, px, py, tileNear, best, bid);
                    else
                        rasterRegion<true, 4>(lds.planes, act[sub], recBase + sub * kWave, px, py, tileNear, best, bid);
                }
            }
            if (full)
                storeRegion<IDS, true, TEX, OUT, NRM>(p, lds, doRgb, doDepth, rgbTile, depthTile, idsTile, pixOff, fx0, fy,
                                                      anyTex, px, py, best, bid, nrmLds, nrmTile);
            else
                storeRegion<IDS, false, TEX, OUT, NRM>(p, lds, doRgb, doDepth, rgbTile, depthTile, idsTile, pixOff, fx0, fy,
                                                       anyTex, px, py, best, bid, nrmLds, nrmTile);
        }
    }
    MRX_STAMP(5);
    MRX_STAMP(6);
    if (stamps && lane == 0)       // where this wave ran: HW_ID (reg 4) and XCC_ID (reg 20)
        stamps[7] = ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32) |
                    (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4);
#undef MRX_STAMP
}

// Launch bounds of the group kernels, uniform and form, plain and FAST (FAST: slots = 16).  Block size:
constexpr int groupThreads(bool tex) { return kWave * groupWaves(tex); }
// The second bound, waves per SIMD.
constexpr int groupWavesPerSimd(KernelForm f, int slots, bool tex)
{
    // textured (four waves per workgroup): four; 256-slot groups are LDS-limited to 3 per CU
    if (tex)
        return slots > 128 ? 3 : 4;
    // The forms over the light table (PVL, PVLC, PVLM, NPV, L, LN): six waves per SIMD -- three
    // workgroups of eight waves -- where the others have eight.  The set-up lanes span views, so the five words of the
    // light are per lane, on top of the five of the projection: with them the set-up wants 68 - 69 registers, and held
    // to the 64 of eight waves it spills five to fifteen of them to scratch wherever the loads are placed.
    if (formFlags(f).lt)
        return 6;
    // The uniform normals form has six FROM 128 slots ON (>=, where the others below have >):
    // held to the 64 registers of eight waves, its 128-slot instantiation with ids spilled 22 of them to scratch.
    if (f == KernelForm::N)
        return slots >= 128 ? 6 : 8;
    // the uniform kernels, PV, C, M: eight, six with 256 slots
    return slots > 128 ? 6 : 8;
}

// The two entry points of the body: the plain one (arguments = RasterParams, as every other kernel here) and the
// FAST one with the preloaded header in front.
// OUT: output selection (raster.hpp OutSel): kOutRGBD or kOutDepth fixed per instantiation; rgb only takes
// kOutByPointer -- a runtime guard on the depth stores -- because a fixed rgb-only instantiation of the 128-slot
// kernel spilled 20 VGPRs to scratch
template <bool IDS, int SLOTS, bool TEX, int XMODE = 0, int OUT = kOutRGBD>
__global__ __launch_bounds__(groupThreads(TEX), groupWavesPerSimd(KernelForm::Uniform, SLOTS, TEX))
void rasterGroupKernel(const RasterParams p)
{
    groupKernelBody<GroupKindOf<KernelForm::Uniform, IDS, SLOTS, TEX, XMODE, false, OUT>>(nullptr, nullptr, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, p);
}

// OUT: output selection (raster.hpp OutSel: kOutRGBD, kOutDepth or kOutRGB), fixed per instantiation
template <bool IDS, bool TEX, int XMODE, int OUT>
__global__ __launch_bounds__(groupThreads(TEX), groupWavesPerSimd(KernelForm::Uniform, 16, TEX))
void rasterGroupKernelFast(const char *hPose, const char *hGeom, uint32_t hViews, uint32_t hInstances, uint32_t hPool,
                           uint32_t hShape, uint32_t hGroups, uint32_t hPrefix, uint32_t hFirst01, uint32_t hFirst23,
                           const RasterParams p)
{
    groupKernelBody<GroupKindOf<KernelForm::Uniform, IDS, 16, TEX, XMODE, true, OUT>>(hPose, hGeom, hViews, hInstances, hPool, hShape,
                                                                                   hGroups, hPrefix, hFirst01, hFirst23, p);
}

// The form kernels of both entry points (raster.hpp KernelForm, formFlags): XMODE 0 (the XCD phase
// trade and report are left to the uniform kernels, or are run-time tests in the normals and label forms) and output
// selection by pointer, so that one instantiation per id / texture / slot setting covers every batch of a form.
// Instantiations of their own, so that a renderer without the tables, columns or outputs launches what it always did:
//   PV, PVL     the per-view forms (p.viewProj, 4.11): PVL with the light table (p.lightTable, 4.12), so that batches
//               whose projections alone differ keep PV
//   C, PVLC     the colour forms (p.instColor, 4.13): C over the uniform projection and light of the kernel arguments,
//               PVLC over both tables (batches whose projections alone differ take it too); a depth-only renderer has
//               no colour form -- it never reads the column
//   M, PVLM     the material forms (p.instMat, 4.14), as the colour forms are.  They read both columns -- a renderer
//               with the material column has the colour column's slot, zero-filled where it has no colour column -- so
//               two forms cover every renderer with this column
//   N, NPV      the normals forms (p.normal, 4.15): N over the uniform projection and light, NPV over both tables; the
//               colour and material columns behind null tests
//   L, LN       the label forms (p.instLabel, S11, 4.16), without and with normals; IDS only.  They store ids (the
//               segmask), read both tables -- a renderer with the label column always fills them -- and every other
//               column behind a null test
template <KernelForm F, bool IDS, int SLOTS, bool TEX>
__global__ __launch_bounds__(groupThreads(TEX), groupWavesPerSimd(F, SLOTS, TEX))
void rasterGroupFormKernel(const RasterParams p)
{
    static_assert(F != KernelForm::Uniform && F != KernelForm::PVM && (IDS || !formFlags(F).lab), "the forms of this family");
    groupKernelBody<GroupKindOf<F, IDS, SLOTS, TEX, 0, false, kOutByPointer>>(nullptr, nullptr, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, p);
}

// (the argument list is the FAST entry's: ten header words, then RasterParams -- the body relies on their preload)
template <KernelForm F, bool IDS, bool TEX>
__global__ __launch_bounds__(groupThreads(TEX), groupWavesPerSimd(F, 16, TEX))
void rasterGroupFormKernelFast(const char *hPose, const char *hGeom, uint32_t hViews, uint32_t hInstances, uint32_t hPool,
                               uint32_t hShape, uint32_t hGroups, uint32_t hPrefix, uint32_t hFirst01, uint32_t hFirst23,
                               const RasterParams p)
{
    static_assert(F != KernelForm::Uniform && F != KernelForm::PVM && (IDS || !formFlags(F).lab), "the forms of this family");
    groupKernelBody<GroupKindOf<F, IDS, 16, TEX, 0, true, kOutByPointer>>(hPose, hGeom, hViews, hInstances, hPool, hShape, hGroups, hPrefix,
                                                                      hFirst01, hFirst23, p);
}

// ---- which form a launch takes (host; first match wins) ---------------------------------------------------------------
// The brute and the chunked kernel:
KernelForm tileForm(const RasterParams &p)
{
    if (p.normal && p.viewProj) return KernelForm::NPV;   // normals over the per-view tables
    if (p.normal)               return KernelForm::N;     // normals over the uniform constants
    if (p.viewProj)             return KernelForm::PV;    // per-view tables (columns behind null checks)
    return KernelForm::Uniform;
}
// The group kernel, both entries:
KernelForm groupForm(const RasterParams &p)
{
    const bool pv = p.viewProj != nullptr;
    // the label column of a segmask renderer (which always fills the tables): the label forms, with or without normals
    if (p.instLabel && p.ids && pv)       return p.normal ? KernelForm::LN : KernelForm::L;
    // the normals output: over the tables where they vary, else over the uniform constants
    if (p.normal && pv && p.tablesVary)   return KernelForm::NPV;
    if (p.normal)                         return KernelForm::N;
    // the material column (and the colour column's slot), likewise
    if (p.instMat && pv && p.tablesVary)  return KernelForm::PVLM;
    if (p.instMat)                        return KernelForm::M;
    // the colour column alone, likewise
    if (p.instColor && pv && p.tablesVary) return KernelForm::PVLC;
    if (p.instColor)                      return KernelForm::C;
    // no column, no extra output: the tables, with the light where the worlds' lights differ
    if (pv && p.lightTable)               return KernelForm::PVL;
    if (pv)                               return KernelForm::PV;
    // the uniform kernels, by XMODE and OUT
    return KernelForm::Uniform;
}

// ---- the three launchers behind launchRaster -------------------------------------------------------------------------
// v1 reference: one wave per tile, every triangle at every pixel
void launchBrute(const RasterParams &p, uint32_t items, bool multi, hipStream_t stream, LaunchForm *took)
{
    const dim3 block(kWave * kWavesPerBlock);
    const bool ids = p.ids != nullptr;
    const dim3 grid((items + kWavesPerBlock - 1) / kWavesPerBlock);
    const KernelForm form = tileForm(p);
    if (took) *took = LaunchForm { (int32_t)form, 0 };
    const OutSel out = outSelOf(p.rgb, p.depth);
    const auto byIdsMulti = [&](auto f) {
        withBool(ids, [&](auto IDS) { withBool(multi, [&](auto MULTI) { f(IDS, MULTI); }); });
    };
    if (form != KernelForm::Uniform)
        withValue<KernelForm, KernelForm::NPV, KernelForm::N, KernelForm::PV>(form, [&](auto F) {
            byIdsMulti([&](auto IDS, auto MULTI) {
                rasterBruteFormKernel<decltype(F)::value, decltype(IDS)::value, decltype(MULTI)::value><<<grid, block, 0, stream>>>(p);
            });
        });
    else
        withValue<int, kOutDepth, kOutRGB, kOutRGBD>(out, [&](auto O) {
            byIdsMulti([&](auto IDS, auto MULTI) {
                rasterBruteKernel<decltype(IDS)::value, decltype(MULTI)::value, decltype(O)::value><<<grid, block, 0, stream>>>(p);
            });
        });
}

// more triangles per world than the group kernel holds: one workgroup per tile
void launchChunked(const RasterParams &p, uint32_t items, hipStream_t stream, LaunchForm *took)
{
    const dim3 block(kWave * kWavesPerBlock);
    const bool ids = p.ids != nullptr;
    const KernelForm form = tileForm(p);
    if (took) *took = LaunchForm { (int32_t)form, 0 };
    withBool(ids, [&](auto IDS) {
        constexpr bool kIds = decltype(IDS)::value;
        if (form != KernelForm::Uniform)
            withValue<KernelForm, KernelForm::PV, KernelForm::N, KernelForm::NPV>(form, [&](auto F) {
                rasterChunkedFormKernel<decltype(F)::value, kIds><<<dim3(items), block, 0, stream>>>(p);
            });
        else
            rasterChunkedKernel<kIds><<<dim3(items), block, 0, stream>>>(p);
    });
}

// the group kernel in the shape `plan` gives it (raster.hpp groupPlan)
void launchGroup(const RasterParams &p, const GroupPlan &plan, hipStream_t stream, LaunchForm *took)
{
    RasterParams q = p;
    q.grpViews = plan.grpViews;
    q.grpChunkTiles = plan.grpChunkTiles;
    q.grpPerView = plan.grpPerView;
    q.xcdSkew = plan.xcdSkew;
    q.xcdRotate = plan.xcdRotate;
    const dim3 grid(plan.workgroups);
    const dim3 gblock(plan.threads);
    const GroupHeader &h = plan.header;
    const int slots = plan.slots, xmode = plan.xmode;
    const bool fast = plan.fast, ids = p.ids != nullptr;
    // Instantiation choice: the form (groupForm), then slots x ids x textured; the uniform kernels by XMODE and OUT
    // too.  FAST and XMODE 1..3 exist with 16 slots only, the label forms with ids only.
    const KernelForm form = groupForm(p);
    if (took) *took = LaunchForm { (int32_t)form, slots };
    const bool tex = p.anyTextured != 0;
    // output selection: one instantiation per setting (kOutRGBD = the kernels as they always were)
    const OutSel out = outSelOf(p.rgb, p.depth);
    const auto byTexIds = [&](auto f) {
        withBool(tex, [&](auto TEX) { withBool(ids, [&](auto IDS) { f(IDS, TEX); }); });
    };
    const auto launchFast = [&](auto kernel) {        // the FAST entry: the header in front
        kernel<<<grid, gblock, 0, stream>>>(h.pose, h.geom, h.views, h.instances, h.poolTris, h.shape, h.groups, h.prefix,
                                            h.first01, h.first23, q);
    };
    const auto launchPlain = [&](auto kernel) { kernel<<<grid, gblock, 0, stream>>>(q); };
    withValue<int, 16, 32, 64, 128, 256>(slots, [&](auto S) {
        constexpr int kSlots = decltype(S)::value;
        if (form != KernelForm::Uniform) {
            withValue<KernelForm, KernelForm::PV, KernelForm::PVL, KernelForm::C, KernelForm::PVLC, KernelForm::M,
                      KernelForm::PVLM, KernelForm::N, KernelForm::NPV, KernelForm::L, KernelForm::LN>(form, [&](auto F) {
                constexpr KernelForm kForm = decltype(F)::value;
                byTexIds([&](auto IDS, auto TEX) {
                    constexpr bool kIds = decltype(IDS)::value, kTex = decltype(TEX)::value;
                    if constexpr (kIds || !formFlags(kForm).lab) {   // (groupForm: labels with ids only)
                        if constexpr (kSlots == 16) {
                            if (fast)
                                return launchFast(rasterGroupFormKernelFast<kForm, kIds, kTex>);
                        }
                        launchPlain(rasterGroupFormKernel<kForm, kIds, kSlots, kTex>);
                    }
                });
            });
            return;
        }
        withValue<int, 0, 1, 2, 3>(xmode, [&](auto X) {
            constexpr int kX = decltype(X)::value;
            if constexpr (kX == 0 || kSlots == 16)
                withValue<int, kOutDepth, kOutRGB, kOutRGBD>(out, [&](auto O) {
                    // rgb only: the FAST entry has its fixed instantiation, the plain one selects by pointer
                    constexpr int kO = decltype(O)::value, kOP = kO == kOutRGB ? kOutByPointer : kO;
                    if constexpr (kSlots == 16) {
                        if (fast)
                            return byTexIds([&](auto IDS, auto TEX) {
                                launchFast(rasterGroupKernelFast<decltype(IDS)::value, decltype(TEX)::value, kX, kO>);
                            });
                    }
                    byTexIds([&](auto IDS, auto TEX) {
                        launchPlain(rasterGroupKernel<decltype(IDS)::value, kSlots, decltype(TEX)::value, kX, kOP>);
                    });
                });
        });
    });
}

}  // namespace

hipError_t launchRaster(const RasterParams &p, uint32_t maxWorldTris,
                        int32_t variant, hipStream_t stream, int32_t *entry, LaunchForm *took)
{
    const uint32_t items = p.numViews * p.tilesFast * p.tilesSlow;
    if (items == 0)
        return hipSuccess;
    if (variant == kVariantBrute) {
        if (entry) *entry = kEntryBrute;
        launchBrute(p, items, maxWorldTris > (uint32_t)kChunk, stream, took);     // (above a chunk: the chunk loop)
    } else if (maxWorldTris > (uint32_t)kGroupSlotsMax) {
        if (entry) *entry = kEntryChunked;
        launchChunked(p, items, stream, took);
    } else {
        bool fastAllowed = true;
        if (const char *dbg = std::getenv("MRX_GROUP_FAST"))      // 0: never (A/B and tests)
            fastAllowed = std::atoi(dbg) != 0;
        const GroupPlan plan = groupPlan(p, maxWorldTris, fastAllowed);
        if (entry) *entry = plan.fast ? kEntryGroupFast : kEntryGroup;
        launchGroup(p, plan, stream, took);
    }
    return hipGetLastError();
}

}  // namespace mrx
