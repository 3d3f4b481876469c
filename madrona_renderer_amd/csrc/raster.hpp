// Device-side parameter block of the tiled raster / ray-cast kernels and the
// host launcher.  Layouts are described in DESIGN.md section 4.
#pragma once

#include <algorithm>
#include <cstdint>
#include <type_traits>
#include <hip/hip_runtime_api.h>

namespace mrx {

struct BvhNode;
struct ObjInfo;

// Per-view projection (DESIGN.md S5 per view, 4.11): the constants of one view as the host works them out
// (mrx_projection_constants), one 32-byte record per view in the device table RasterParams::viewProj.
struct alignas(32) ViewProj {
    float sx, ox, sz, oz;
    float invNear, s6bPad;
    float pad[2];
};
static_assert(sizeof(ViewProj) == 32, "ViewProj is one 32-byte record");

// Per-world light, expanded by the host to one record per view (DESIGN.md S4 / S7 per world, 4.12): the unit vector
// towards the light and the two S7 constants as mrx_light_constants resolves them, in the device table
// RasterParams::viewLight.  Per view and not per world: a kernel indexes it with the view it already has, beside
// the camera rotation the direction is combined with, without a viewWorld[] load in front.
struct alignas(32) ViewLight {
    float toLight[3];
    float ambient, diffuse;
    float pad[3];
};
static_assert(sizeof(ViewLight) == 32, "ViewLight is one 32-byte record");

// Object-space triangle: 16 dwords, one 64-byte line.
struct alignas(16) ObjTri {
    float p[9];      // 3 vertices x xyz
    float uv[6];     // 3 vertices x uv
    int32_t mat;     // material index, -1 = default material
};
static_assert(sizeof(ObjTri) == 64, "ObjTri must be one 64-byte line");

// Material of one object triangle, resolved on the host (mesh material or the
// default colour; texture index validated): one 32-byte record next to ObjTri.
struct alignas(16) TriMat {
    // rgb of the resolved material; the alpha slot (nothing shades with it) holds the
    // int32 id of the object the triangle belongs to -- the segmask label, so that label
    // and geometry agree whatever non-negative value the live ObjectID column holds
    float color[4];
    int32_t tex;       // texture index, -1 = untextured
    // S6b back-face culling data of the triangle's shell (edge-connected
    // component of its object): orient = +1 / -1 when the shell is a closed,
    // consistently wound mesh (sign of its volume), 0 otherwise; bb = the
    // shell's object-space bounding box, padded
    float orient;
    float bbMin[3];
    float bbMax[3];
    int32_t texDesc[4];   // TexDesc of `tex` (offset, width, height, 0), zero when untextured
};
static_assert(sizeof(TriMat) == 64, "TriMat layout");

struct TexDesc {
    uint32_t offset;  // texel offset into the RGBA8 pool
    uint32_t width, height;
    uint32_t pad;
};

// One material of the renderer's table as the override reads it (RasterParams::matTable): rgb and the validated
// texture index (-1 = untextured; its TexDesc is RasterParams::textures[tex]).
struct alignas(16) MatRec {
    float r, g, b;
    int32_t tex;
};
static_assert(sizeof(MatRec) == 16, "MatRec is one 16-byte record");

// One world-triangle slot: which instance row draws which object triangle.
struct WorldTri {
    uint32_t inst;   // row of the world-major instance tables
    uint32_t tri;    // index into the ObjTri pool
};

struct RasterParams {
    // shared read-only scene
    const ObjTri *tris;
    const TriMat *triMats;           // parallel to tris
    const TexDesc *textures;
    const uint32_t *texels;          // RGBA8
    int32_t anyTextured;             // some drawn triangle has a texture
    // per-view draw lists: view v draws viewTris[v * viewTriStride + k],
    // k < viewTriCount[v] -- one load level between the view index and the
    // triangle's pose / geometry rows
    const WorldTri *viewTris;
    const uint32_t *viewTriCount;    // [views]
    uint32_t viewTriStride;
    // Uniform worlds (every world: the same <= 4 objects in the same order, the
    // same camera count): the draw list is arithmetic on kernel arguments --
    // slot k of a view belongs to local instance i with uniPrefix[i] <= k <
    // uniPrefix[i+1], object triangle uniFirstTri[i] + k - uniPrefix[i] -- so
    // no table load sits between the view index and the pose / geometry rows.
    uint32_t uniInstances;           // instances per world, 0 = not uniform
    uint32_t uniCamsPerWorld;
    uint32_t uniPrefix[5];
    uint32_t uniFirstTri[4];
    // the blocks the pose tensors / geometry tables are slices of (GroupHeader; filled in by mrx_create)
    const char *poseBlock;
    const char *geomBlock;
    uint32_t numInstances, poolTris;
    // pose state (the exported, mutable tensors)
    const float *instPos;            // [I][3]
    const float *instRot;            // [I][4] w,x,y,z
    const float *instScale;          // [I][3]
    const int32_t *instObj;          // [I]
    const float *camPos;             // [V][3]
    const float *camRot;             // [V][4]
    // outputs, storage order [view][slow][fast]
    uint32_t *rgb;
    float *depth;
    int32_t *ids;                    // visibility ids or segmask, may be null
    uint32_t numViews;
    uint32_t nfast, nslow;           // pixels per row, rows per view
    uint32_t tilesFast, tilesSlow;   // 64x64 tiles per view
    // pixel -> ray constants
    float sx, ox, sz, oz;
    float invNear, invFar;
    // S6b: the eye counts as outside a shell only when it is further than this
    // from the shell's box -- no front face can then be cut by the near plane
    float s6bPad;
    float toLight[3];
    float ambient, diffuse;
    int32_t transposed;              // Raytracer-mode [x][y] storage
    int32_t idsAreSegmask;           // ids buffer holds objectID instead of tri index
    // Timing-only ablation switches (MRX_DEBUG_SKIP env, never set in
    // production): 1 skip stores, 2 skip raster, 4 skip classification,
    // 8 skip triangle setup.  Outputs are wrong when any bit is set.
    uint32_t debugSkip;
    // Output store policy: 1 = write-through (sc1), 0 = plain write-back.
    uint32_t writeThrough;
    // Shape of the group kernel's workgroups (filled in by launchRaster):
    // grpPerView == 1: a workgroup owns grpViews whole views; otherwise it owns
    // grpChunkTiles tiles of one view and a view takes grpPerView workgroups.
    // grpViewsWanted / grpTilesWanted: MRX_GROUP_VIEWS / MRX_GROUP_TILES
    // tuning overrides (0 = automatic).
    uint32_t grpViews, grpChunkTiles, grpPerView;
    int32_t grpViewsWanted, grpTilesWanted;
    // XCD-aware split of the group kernel (filled in by launchRaster);
    // xcdSkew = strips moved per workgroup pair; xcdSkewWanted is the
    // MRX_XCD_SKEW override: -1 automatic, 0 off, 1..7 strips.
    uint32_t xcdSkew;
    int32_t xcdSkewWanted;
    // XCD phase feedback of the split: workgroup 0 of every launch writes its XCC id to
    // a host-mapped word; its parity, read back by the host before a later launch, makes
    // the workgroups of each pair trade places (raster.hip)
    uint32_t *xccReport;
    uint32_t xcdPhase;
    // rotate the group <-> XCD relation by two every round of eight workgroups
    // (MRX_XCD_ROTATE override: -1 automatic, 0 off, 1 on)
    uint32_t xcdRotate;
    int32_t xcdRotateWanted;
    int32_t debugSlots;              // MRX_DEBUG_SLOTS: force 32 / 64 triangle slots per tile
    // Diagnostic only (MRX_DEBUG_STAMPS=1): per-wave s_memrealtime stamps,
    // [workgroup][wave][8], written to memory nothing else reads.
    unsigned long long *debugStamps;
    // ---- BVH path (bvh.hip): per-object BLAS built at load (bvh.hpp), the
    //      world -> instance-row and view -> world tables the per-step TLAS is
    //      built from, and each instance's first world-local triangle index
    const BvhNode *bvhNodes;
    const uint32_t *bvhLeafTris;
    const ObjInfo *instInfo;         // [I]: the ObjInfo of each instance's (creation-time) object
    uint32_t numObjects;
    uint32_t bvhUniInst, bvhUniCams; // every world: this many instances / cameras (0: look the tables up)
    const uint32_t *worldInstStart;  // [worlds + 1]
    const uint32_t *viewWorld;       // [views]
    const uint32_t *instKBase;       // [I]
    uint32_t bvhPassInst;            // instances whose TLAS records fit LDS at once (a multiple of 8)
    int32_t bvhTile;                 // tile of a workgroup: 0 = 64x64, 1 = 64 wide x 32, 2 = 32x32 (MRX_BVH_TILE)
    int32_t bvhSmallArea;            // boxes of up to this many pixels are walked by their triangle's lane
    int32_t bvhClassify;             // 64x64 tiles: the instantiation that classifies listed triangles per strip
    // tiles of a view one workgroup renders in turn over one TLAS build (1 when a world needs several
    // TLAS passes; filled in by the host, MRX_BVH_GROUP_TILES overrides)
    uint32_t bvhGroupTiles;
    // one-tile views a workgroup renders in turn, their TLASes built side by side in one phase I (a power of
    // two; 1 unless every world fits one TLAS pass; filled in by the host, MRX_BVH_GROUP_VIEWS overrides);
    // bit 16 (two views): a launch of as many workgroups as the chip holds, pairs on the first of them and single
    // views on the others; bits 17..19: wave-priority mode of the younger workgroups (bvh.hip; 0 off); bits 20..31:
    // the index of the first workgroup that is a CU's second (= the number of CUs)
    uint32_t bvhGroupViews;
    // every world holds at most 64 triangles in at most 64 instance rows: the kernel that sets a view's
    // triangles up once and shares the per-tile work among all waves (bvh.hip, bvhFlatKernel; MRX_BVH_FLAT=0: never)
    uint32_t bvhFlat;
    // textured BVH instantiations: 48-byte shading records per round of a tile (64 ... 1023; chosen by the host so that
    // the workgroup's LDS stays within half a CU's: mrx_api.cpp chooseBvhGroups)
    uint32_t bvhTexCap;
    // compute units of the device the renderer runs on (hipDeviceAttributeMultiprocessorCount at creation):
    // every "does the batch fill the chip" decision of the launchers follows from it (groupFill below)
    uint32_t numCUs;
    // Per-view projection form: [numViews] records whose sx ox sz oz invNear s6bPad replace the uniform ones
    // above, view by view; null = the uniform form (every view uses the kernel-argument constants).  The
    // launchers pick the kernels' per-view instantiations from it.
    const ViewProj *viewProj;
    // Per-world light, one record per view: set together with viewProj -- the per-view
    // instantiations read both tables, and the host fills the one that does not vary with the uniform values.
    // Null with viewProj: the uniform form (toLight / ambient / diffuse above).
    const ViewLight *viewLight;
    // 1: the worlds' lights differ (the group kernels then launch the per-view instantiations that read viewLight;
    // where only projections differ they keep the ones that take the uniform light above); 0 otherwise
    uint32_t lightTable;
    // 1: the projections or the lights above differ between views; 0 with viewProj set: the tables repeat the uniform
    // values and are there for the instance colours alone (the group kernels then launch their uniform colour form)
    uint32_t tablesVary;
    // Per-instance colour override: [I] packed bytes (r, g, b, a), r lowest; a != 0 replaces
    // material.rgb of the row's triangles by (r, g, b) / 255.  The slice of the pose block behind instObj
    // (poseColorOffset); null = no column, or a depth-only renderer, which never reads it.  Set together with
    // viewProj: the per-view instantiations of the chunked, brute and BVH kernels read it behind a null check, the
    // group kernels have colour instantiations of their own.
    const uint32_t *instColor;
    // Per-instance material override: [I] material ids; an id below numMaterials (one unsigned
    // compare: negative ids fail it) replaces the rgb and the texture index of the row's triangles by those of
    // matTable[id].  The slice of the pose block behind the colour column's slot (poseMaterialOffset); null = no
    // column, or a depth-only renderer.  Set together with viewProj, as instColor is: the per-view instantiations of
    // the chunked, brute and BVH kernels read it behind a null check, the group kernels have instantiations of their own.
    const int32_t *instMat;
    // [numMaterials + 1] records of the renderer's material table (the last one a spare nothing may select)
    const MatRec *matTable;
    uint32_t numMaterials;
    // Surface-normal output: [view][slow][fast] packed view-space normals, storage as rgb's;
    // null = not rendered (no MRX_FLAG_NORMALS): the launchers then pick the kernels they always did, none of
    // which reads this member.
    uint32_t *normal;
    // Per-instance label: [I] int32; kLabelObject = the id of the object the row is bound to
    // (S9's segmask value), any other value is what the segmask holds on the pixels the row's triangles win.  The slice
    // of the pose block behind the material column's slot (poseLabelOffset); null = no column, or a renderer whose ids
    // tensor holds visibility ids.  Set together with viewProj and with ids (idsAreSegmask): the per-view segmask
    // instantiations of the chunked, brute and BVH kernels read it behind a null check, the group kernels have label
    // forms of their own.  The last member of the block.
    const int32_t *instLabel;
};

// the label that stands for "the bound object's id" (include/mrx.h MRX_LABEL_OBJECT)
constexpr int32_t kLabelObject = INT32_MIN;

// ---- the argument header of the group kernel's fast prologue (raster.hip, FAST) -------------------------------------
// The command processor can write the first dwords of a kernel's argument block into SGPRs at wave launch
// (-mllvm -amdgpu-kernarg-preload-count): a kernel whose first loads need only those starts them without the
// s_load round trip to the argument block (a fresh copy, hence a cache miss, on every launch: 0.24 us in
// scripts/micro/kernarg_preload.hip).  Fourteen dwords at most, so everything the set-up waves of a
// uniform-world, one-tile-per-view launch need ahead of their pose loads is packed into twelve: the pose
// tensors live in ONE block and the geometry tables in another, at offsets that follow from the counts.
#if defined(__HIP__) || defined(__HIPCC__)
#define MRX_HD __host__ __device__
#else
#define MRX_HD
#endif
struct PoseLayout {
    uint32_t camRot, camPos, instRot, instPos, instScale, instObj, total;   // byte offsets, 256-byte aligned
};
MRX_HD inline uint32_t mrxAlign256(uint32_t x) { return (x + 255u) & ~255u; }
MRX_HD inline PoseLayout poseLayout(uint32_t views, uint32_t instances)
{
    PoseLayout l;
    l.camRot = 0;
    l.camPos = l.camRot + mrxAlign256(views * 16u);
    l.instRot = l.camPos + mrxAlign256(views * 12u);
    l.instPos = l.instRot + mrxAlign256(instances * 16u);
    l.instScale = l.instPos + mrxAlign256(instances * 12u);
    l.instObj = l.instScale + mrxAlign256(instances * 12u);
    l.total = l.instObj + mrxAlign256(instances * 4u);
    return l;
}
// the colour column of a renderer that has one (RasterParams::instColor): [instances] dwords behind the layout above,
// whose offsets therefore do not move
MRX_HD inline uint32_t poseColorOffset(uint32_t views, uint32_t instances) { return poseLayout(views, instances).total; }
// the material column of a renderer that has one (RasterParams::instMat): [instances] dwords behind the colour column's
// slot, which a renderer with this column always has (zero-filled where it has no colour column)
MRX_HD inline uint32_t poseMaterialOffset(uint32_t views, uint32_t instances)
{
    return poseColorOffset(views, instances) + mrxAlign256(instances * 4u);
}
// the label column of a renderer that has one (RasterParams::instLabel): [instances] dwords behind the slots of the
// colour and the material column, whether or not the renderer has those
MRX_HD inline uint32_t poseLabelOffset(uint32_t views, uint32_t instances)
{
    return poseMaterialOffset(views, instances) + mrxAlign256(instances * 4u);
}
// geometry block: ObjTri[pool] at 0, TriMat[pool] at geomMatsOffset(pool)
MRX_HD inline uint32_t geomMatsOffset(uint32_t poolTris) { return mrxAlign256(poolTris * 64u); }

struct GroupHeader {
    const char *pose;        // base of the pose block (poseLayout(views, instances))
    const char *geom;        // base of the geometry block
    uint32_t views, instances, poolTris;
    // grpViews | xcdSkew << 8 | xcdRotate << 12 | uniInstances << 13 | uniCamsPerWorld << 16 | valid << 31
    uint32_t shape;
    uint32_t groups;         // workgroups of the launch
    uint32_t prefix;         // uniPrefix[1..4], eight bits each
    uint32_t first01, first23;   // uniFirstTri[0..3], sixteen bits each
};
// The layout of the four packed words, defined once: the host packs with these functions (groupPlan below), the
// kernel's prologue unpacks with them (raster.hip), and what a field cannot hold keeps a launch off the FAST entry
// (hdrFits).  A field is (first bit, width) within its word.
struct HdrField {
    uint32_t shift, bits;
};
constexpr HdrField kHdrGrpViews = { 0, 8 }, kHdrXcdSkew = { 8, 4 }, kHdrXcdRotate = { 12, 1 }, kHdrUniInstances = { 13, 3 },
                   kHdrUniCams = { 16, 8 }, kHdrValid = { 31, 1 };
constexpr uint32_t kHdrPrefixBits = 8;    // prefix: uniPrefix[i] at 8 (i - 1), i = 1..4
constexpr uint32_t kHdrFirstBits = 16;    // first01 / first23: uniFirstTri[i] at 16 (i & 1)
MRX_HD inline bool hdrFits(uint32_t value, uint32_t bits) { return value < (1u << bits); }
MRX_HD inline uint32_t hdrPackShape(uint32_t grpViews, uint32_t xcdSkew, uint32_t xcdRotate, uint32_t uniInstances,
                                    uint32_t uniCams)
{
    return (grpViews << kHdrGrpViews.shift) | (xcdSkew << kHdrXcdSkew.shift) | (xcdRotate << kHdrXcdRotate.shift) |
           (uniInstances << kHdrUniInstances.shift) | (uniCams << kHdrUniCams.shift) | (1u << kHdrValid.shift);
}
MRX_HD inline uint32_t hdrPackPrefix(const uint32_t (&uniPrefix)[5])
{
    return uniPrefix[1] | (uniPrefix[2] << kHdrPrefixBits) | (uniPrefix[3] << 2 * kHdrPrefixBits) |
           (uniPrefix[4] << 3 * kHdrPrefixBits);
}
MRX_HD inline uint32_t hdrPackFirst(uint32_t even, uint32_t odd) { return even | (odd << kHdrFirstBits); }
// the fields of the shape word, each with its shift and mask as constants where the expression is written
constexpr uint32_t hdrMask(HdrField f) { return (1u << f.bits) - 1u; }
static_assert(kHdrGrpViews.shift == 0, "the first field");
MRX_HD inline uint32_t hdrGrpViews(uint32_t shape) { constexpr uint32_t m = hdrMask(kHdrGrpViews); return shape & m; }
MRX_HD inline uint32_t hdrXcdSkew(uint32_t shape) { constexpr uint32_t s = kHdrXcdSkew.shift, m = hdrMask(kHdrXcdSkew); return (shape >> s) & m; }
MRX_HD inline uint32_t hdrXcdRotate(uint32_t shape) { constexpr uint32_t s = kHdrXcdRotate.shift, m = hdrMask(kHdrXcdRotate); return (shape >> s) & m; }
MRX_HD inline uint32_t hdrUniInstances(uint32_t shape) { constexpr uint32_t s = kHdrUniInstances.shift, m = hdrMask(kHdrUniInstances); return (shape >> s) & m; }
MRX_HD inline uint32_t hdrUniCams(uint32_t shape) { constexpr uint32_t s = kHdrUniCams.shift, m = hdrMask(kHdrUniCams); return (shape >> s) & m; }
// uniPrefix[i], i = 1..4, of the prefix word; uniFirstTri[i] of the word that holds it (first01 for 0 and 1, first23)
MRX_HD inline uint32_t hdrPrefix(uint32_t word, uint32_t i) { return (word >> kHdrPrefixBits * (i - 1u)) & ((1u << kHdrPrefixBits) - 1u); }
MRX_HD inline uint32_t hdrFirst(uint32_t word, uint32_t i) { return (word >> kHdrFirstBits * (i & 1u)) & ((1u << kHdrFirstBits) - 1u); }

// Default dispatch: worlds of this many triangles and more take the BVH path
// (measured crossover, profiles/r02_bvh_crossover.txt; MRX_BVH_MIN_TRIS overrides; small batches of 64x64 views
// cross earlier -- from 65 triangles up to 640 views, from 91 up to 1024 untextured ones: mrx_api.cpp).
constexpr uint32_t kBvhMinTris = 129;

// Output selection (mrx_config.flags MRX_FLAG_NO_RGB / MRX_FLAG_NO_DEPTH).  The host passes a null pointer for an
// output that is not selected.  The kernels that carry the shipped configurations (rasterGroupKernelFast, bvhFlatKernel)
// take the setting as a template parameter and compile the unselected output's work out; the others take
// kOutByPointer and skip the stores of a null output at run time.
enum OutSel : int {
    kOutRGBD = 0,       // rgb and depth
    kOutDepth = 1,      // depth only: no colour set-up, no texel loads, no rgb stores
    kOutRGB = 2,        // rgb only: no depth reciprocal, no depth stores
    kOutByPointer = 3   // whatever pointers are not null (wave-uniform runtime guard)
};
inline OutSel outSelOf(const void *rgb, const void *depth)
{
    return !rgb ? kOutDepth : !depth ? kOutRGB : kOutRGBD;
}

// Kernel forms.  Beside its uniform kernel every kernel family has ONE form kernel, a template over
// this enum: which tables and columns of RasterParams the instantiation reads, which extra outputs it stores.  The
// launchers pick the form with one host function per family (groupForm in raster.hip, bvhForm in bvh.hip).  Not every
// family has every form: the brute, chunked and flat kernels have PV, N and NPV, the BVH tile kernel those and PVM.
enum class KernelForm : int {
    Uniform = 0,   // the uniform kernels themselves (projection and light from the kernel arguments, no column)
    PV, PVL, C, PVLC, M, PVLM, N, NPV, L, LN,
    PVM,           // BVH tile kernel only: per-view tables and the material column
};
struct FormFlags {
    bool pv;    // per-view projection table (viewProj)
    bool lt;    // per-view light table (viewLight, 4.12)
    bool col;   // colour column (instColor, 4.13)
    bool mat;   // material column (instMat, 4.14)
    bool nrm;   // normals output (normal, 4.15)
    bool lab;   // label column (instLabel, 4.16)
};
constexpr FormFlags formFlags(KernelForm f)
{
    switch (f) {                                     //  pv     lt     col    mat    nrm    lab
    case KernelForm::PV:   return FormFlags { true,  false, false, false, false, false };
    case KernelForm::PVL:  return FormFlags { true,  true,  false, false, false, false };
    case KernelForm::C:    return FormFlags { false, false, true,  false, false, false };
    case KernelForm::PVLC: return FormFlags { true,  true,  true,  false, false, false };
    case KernelForm::M:    return FormFlags { false, false, true,  true,  false, false };
    case KernelForm::PVLM: return FormFlags { true,  true,  true,  true,  false, false };
    case KernelForm::N:    return FormFlags { false, false, true,  true,  true,  false };
    case KernelForm::NPV:  return FormFlags { true,  true,  true,  true,  true,  false };
    case KernelForm::L:    return FormFlags { true,  true,  true,  true,  false, true };
    case KernelForm::LN:   return FormFlags { true,  true,  true,  true,  true,  true };
    case KernelForm::PVM:  return FormFlags { true,  false, false, true,  false, false };
    default:               return FormFlags { false, false, false, false, false, false };
    }
}

// ---- run-time value -> template argument (the launchers' instantiation choice) --------------------------------------
// withBool(b, f) calls f(std::true_type) or f(std::false_type); withValue<T, V0, V1, ...>(v, f) calls
// f(std::integral_constant<T, Vi>) for the first Vi equal to v, and for the LAST value of the list when none is (the
// list's "otherwise").  f is a generic lambda that reads the constant as decltype(arg)::value; `if constexpr` on such
// constants inside it keeps combinations nothing launches from being instantiated.  Both return what f returns.
template <typename F>
inline auto withBool(bool b, F &&f)
{
    return b ? f(std::true_type {}) : f(std::false_type {});
}
template <typename T, T V0, T... Vs, typename F>
inline auto withValue(T v, F &&f)
{
    if constexpr (sizeof...(Vs) == 0)
        return f(std::integral_constant<T, V0> {});
    else
        return v == V0 ? f(std::integral_constant<T, V0> {}) : withValue<T, Vs...>(v, f);
}

// Kernel variants (mrx_config.kernel_variant).
enum KernelVariant : int32_t {
    kVariantDefault = 0,     // group kernel up to kBvhMinTris-1 triangles per world, BVH above
    kVariantBrute = 1,       // v1: every triangle tested at every pixel
    kVariantBvh = 2,         // BVH path whatever the scene size
    kVariantRaster = 3,      // never the BVH path (group kernel, chunked kernel above 256)
    kNumVariants
};

// ---- launch-shape constants as functions of the device (they were MI355X literals) ----------------
// Workgroups of the group kernel a launch needs before the chip counts as full: a CU holds 2048 threads = four
// workgroups of 512 (the untextured kernel; the textured one has 256 threads and longer tiles -- same target).
inline uint32_t groupFill(uint32_t numCUs) { return 4u * (numCUs ? numCUs : 256u); }

// ---- the group kernel's launch plan (raster.hip rasterGroupKernel) --------------------------------
// (kWave and kChunk are the device sources' names for the wave size and the set-up pass; they stand here, in namespace mrx,
// because the plan below is the launcher's text -- no other source of the library defines either name)
constexpr int kWave = 64;
constexpr int kChunk = 64;       // triangles set up per pass (one per lane)
// A group is up to 16 tiles drawn from one or more views whose triangles fit
// the records together (setup is per view, shared by the view's tiles).  Up to
// 64 slots per view the group holds kChunk records (with the XCD-aware split
// a workgroup on a fast XCD carries one 16-slot view more); views of 128 / 256
// slots are one view per group.
constexpr int kGroupTilesMax = 16;
constexpr int kGroupSlotsMax = 256;
constexpr int groupTilesMax(int slots) { return slots <= 128 ? kGroupTilesMax : 8; }
// Waves per workgroup of the group kernel: eight for untextured scenes (more
// waves in flight absorb the stalls of a saturated store path), four for the
// textured variant (its texel loads cost registers and vmcnt drains).
constexpr int groupWaves(bool tex) { return tex ? 4 : 8; }

// What launchRaster launches for a batch of worlds of at most kGroupSlotsMax triangles: the shape of the workgroups,
// the XCD split, the entry and the header that goes with the launch.  All of it decides speed only -- every shape
// renders the same pixels -- so it is host arithmetic a test can read (mrx_group_plan) where no parity test would
// notice a slip.
struct GroupPlan {
    int slots;                   // triangle slots per view: 16 ... 256
    uint32_t grpViews, grpChunkTiles, grpPerView;   // RasterParams' members of these names
    uint32_t workgroups, threads;
    uint32_t xcdSkew, xcdRotate; // RasterParams' members of these names
    int xmode;                   // the XMODE instantiation (raster.hip): bit 0 trade places, bit 1 report
    bool fast;                   // the FAST entry
    GroupHeader header;          // shape, prefix, first01 and first23 are filled in for the FAST entry only
};
// `fastAllowed`: MRX_GROUP_FAST as launchRaster reads it (false: never the FAST entry).  No HIP call, no environment.
inline GroupPlan groupPlan(const RasterParams &p, uint32_t maxWorldTris, bool fastAllowed)
{
    GroupPlan plan {};
    // triangle slots per view: the smallest of 16 ... 256 that holds a world
    int slots = 16;
    while ((uint32_t)slots < maxWorldTris)
        slots *= 2;
    if (p.debugSlots >= slots && p.debugSlots <= kGroupSlotsMax && (p.debugSlots & (p.debugSlots - 1)) == 0)
        slots = p.debugSlots;                 // tuning / test aid (MRX_DEBUG_SLOTS)
    // Workgroup shape.  Setup is per view and the view's tiles share it, so
    // a workgroup takes as many whole views as fit 64 records and 16 tiles
    // (8 for views of 256 slots); a view of more tiles is cut into chunks.
    // Small batches shrink the workgroups again until there are ~4 per CU.
    const uint32_t tpv = p.tilesFast * p.tilesSlow;
    const uint32_t maxTiles = (uint32_t)groupTilesMax(slots);
    const uint32_t kFill = groupFill(p.numCUs);    // 4 resident workgroups per CU: 1024 on 256 CUs
    uint32_t vg = 1, ct = tpv, gpv = 1;
    if (tpv == 1) {
        // one-tile views: as many as fit 64 records, all workgroups resident
        // (textured: two -- its workgroups have four waves and longer tiles)
        vg = std::max<uint32_t>(1u, (uint32_t)(kChunk / slots));
        if (p.anyTextured)
            vg = std::min<uint32_t>(vg, 2u);
        // ... until ~4 workgroups per CU remain; two views per workgroup are kept
        // down to 2 per CU (1024 worlds: 9.9 -> 9.3 us)
        while (vg > 1 && (p.numViews + vg - 1) / vg < (vg == 2 ? kFill / 2 : kFill))
            vg /= 2;
    } else if (p.anyTextured) {
        // textured, several tiles per view: a quarter of a view per workgroup, at most four
        // tiles (4 waves per workgroup and per-pixel texturing make a tile long enough for
        // its own setup; measured on 128^2 and 256^2: profiles/r01_group_shapes.txt)
        ct = std::max<uint32_t>(1u, std::min<uint32_t>(4u, tpv / 4u));
    } else {
        // untextured, several tiles per view: one view per workgroup, at most eight tiles
        ct = std::min<uint32_t>(tpv, std::min<uint32_t>(maxTiles, 8u));
    }
    if (tpv != 1)
        while (ct > 1 && (uint64_t)p.numViews * ((tpv + ct - 1) / ct) < kFill)
            ct = (ct + 1) / 2;
    if (p.grpViewsWanted > 0 && tpv * (uint32_t)p.grpViewsWanted <= maxTiles &&
        p.grpViewsWanted * slots <= kChunk) {
        vg = (uint32_t)p.grpViewsWanted;
        ct = tpv;
    }
    if (p.grpTilesWanted > 0 && (uint32_t)p.grpTilesWanted <= maxTiles) {
        vg = 1;
        ct = std::min<uint32_t>((uint32_t)p.grpTilesWanted, tpv);
    }
    gpv = (tpv + ct - 1) / ct;
    plan.slots = slots;
    plan.grpViews = vg;
    plan.grpChunkTiles = ct;
    plan.grpPerView = gpv;
    const uint32_t numGroups = gpv == 1 ? (p.numViews + vg - 1) / vg : p.numViews * gpv;
    // XCD-aware split.  Workgroups go round-robin to the eight XCDs and the
    // odd XCD of every pair drains its stores ~15 % more slowly (measured,
    // profiles/r01_xcd.txt): once the batch fills the chip, xcdSkew strips
    // (eighths of a tile) per workgroup pair move from the odd to the even
    // XCD (see the kernel prologue).
    const bool skewable = slots == 16 && tpv == 1 && (vg == 4 || vg == 2);
    plan.xcdSkew = (skewable && numGroups >= kFill) ? (vg == 4 ? 3u : 1u) : 0u;
    if (p.xcdSkewWanted >= 0)
        plan.xcdSkew = skewable ? (uint32_t)(p.xcdSkewWanted < 8 ? p.xcdSkewWanted : 7) : 0u;
    plan.xcdRotate = (tpv == 1 && numGroups >= kFill) ? 1u : 0u;
    if (p.xcdRotateWanted >= 0)
        plan.xcdRotate = p.xcdRotateWanted ? 1u : 0u;
    plan.workgroups = numGroups;
    plan.threads = (uint32_t)(kWave * groupWaves(p.anyTextured != 0));
    // The argument header (GroupHeader) goes along with every launch; the FAST instantiations --
    // 16 slots, one-tile views, uniform worlds whose table fits the header, no diagnostics -- read nothing else
    // ahead of their pose loads.
    GroupHeader &h = plan.header;
    h.pose = p.poseBlock;
    h.geom = p.geomBlock;
    h.views = p.numViews;
    h.instances = p.numInstances;
    h.poolTris = p.poolTris;
    h.groups = numGroups;
    bool fast = slots == 16 && tpv == 1 && gpv == 1 && p.uniInstances != 0 && hdrFits(p.uniCamsPerWorld, kHdrUniCams.bits) &&
                hdrFits(vg, kHdrGrpViews.bits) && p.poseBlock && p.geomBlock && p.debugSkip == 0 && p.debugStamps == nullptr &&
                hdrFits(p.uniPrefix[4], kHdrPrefixBits);
    for (int i = 0; i < 4 && fast; ++i)
        fast = hdrFits(p.uniFirstTri[i], kHdrFirstBits);
    fast = fast && fastAllowed;
    plan.fast = fast;
    if (fast) {
        h.shape = hdrPackShape(vg, plan.xcdSkew, plan.xcdRotate, p.uniInstances, p.uniCamsPerWorld);
        h.prefix = hdrPackPrefix(p.uniPrefix);
        h.first01 = hdrPackFirst(p.uniFirstTri[0], p.uniFirstTri[1]);
        h.first23 = hdrPackFirst(p.uniFirstTri[2], p.uniFirstTri[3]);
    }
    // XCD phase: trade places within the pairs on an odd start, ask for a report now and then
    plan.xmode = slots != 16 ? 0 : ((plan.xcdSkew && (p.xcdPhase & 1u)) ? 1 : 0) | (p.xccReport ? 2 : 0);
    return plan;
}
// Triangles per world from which the default dispatch takes the BVH path (mrx_api.cpp bindGeometry).  `base` is the
// general threshold (kBvhMinTris or MRX_BVH_MIN_TRIS).  Small batches of one-tile views cross earlier, because up to two
// workgroups per CU the BVH kernel's launch costs what its slowest workgroup costs while the raster kernels' 128-slot
// shape pays for its slots -- measured on 256 CUs (profiles/r03_bvh_threshold.txt): from 65 triangles up to 640 views =
// 2.5 per CU (512 views of 74 triangles 10.7 against 12.3 us, textured 13.0 against 15.5), from 91 up to 1024 = 4 per CU
// for untextured worlds (1024 views of 98 triangles 18.0 against 18.6); larger batches cross at `base`.
inline uint32_t bvhDispatchMinTris(uint32_t base, uint32_t numViews, bool anyTextured, uint32_t nfast, uint32_t nslow,
                                   uint32_t numCUs)
{
    const uint32_t cus = numCUs ? numCUs : 256u;
    if (nfast > 64u || nslow > 64u)
        return base;
    if (2ull * numViews <= 5ull * cus)
        return base < 65u ? base : 65u;
    if (numViews <= 4u * cus && !anyTextured)
        return base < 91u ? base : 91u;
    return base;
}

// Raytracer-mode batches of small worlds that the default dispatch gives to the BVH path's flat kernel (bvh.hip,
// bvhFlatKernel: worlds of <= 64 triangles in <= 64 rows) instead of the raster group kernel: views of at least 16
// tiles, at least 192 tiles per compute unit in the batch -- BASELINE configs[4], 4096 views of 256x256 = 65536 tiles on 256
// CUs, is the measured case (474 - 483 us against 488 - 494 on the same boxes, profiles/r04_c5_shape_by_views.txt,
// r04_bench_k20_kernel_stats.csv); at 2048 views and fewer, and in Rasterizer mode (no segmask: two output tensors), the
// raster kernel is ahead by 1 - 3 % and keeps the batch.
inline bool bvhDispatchFlat(bool raytracer, uint32_t numViews, uint32_t nfast, uint32_t nslow, uint32_t maxWorldTris,
                            uint32_t maxWorldInstances, uint32_t numCUs)
{
    const uint32_t cus = numCUs ? numCUs : 256u;
    const uint64_t tpv = (uint64_t)((nfast + 63u) / 64u) * ((nslow + 63u) / 64u);
    return raytracer && maxWorldTris >= 1u && maxWorldTris <= 64u && maxWorldInstances <= 64u && tpv >= 16u &&
           (uint64_t)numViews * tpv >= 192ull * cus;
}

// Which kernel a launch ran (mrx_raster_entry; the values are include/mrx.h's MRX_ENTRY_*): launchRaster writes
// the raster entry it picked to *entry, host side; no kernel sees it.
enum RasterEntry : int32_t {
    kEntryNone = 0, kEntryGroupFast = 1, kEntryGroup = 2, kEntryChunked = 3, kEntryBrute = 4, kEntryBvh = 5,
};
// Which instantiation it ran (mrx_kernel_form; include/mrx.h's MRX_FORM_* are the KernelForm values): the form the
// launcher picked and, for the group kernel, the triangle slots per view it launched with (0 in every other family).
// Written next to *entry, host side; no kernel sees either.
struct LaunchForm {
    int32_t form = 0;     // KernelForm
    int32_t slots = 0;
};
hipError_t launchRaster(const RasterParams &p, uint32_t maxWorldTris,
                        int32_t variant, hipStream_t stream, int32_t *entry = nullptr, LaunchForm *took = nullptr);

// BVH path: per-step TLAS in LDS, wave-packet traversal of TLAS + BLAS,
// exact S6 leaf test (bvh.hip).  p.bvhPassInst is filled in by the caller.
hipError_t launchBvh(const RasterParams &p, hipStream_t stream, LaunchForm *took = nullptr);
constexpr uint32_t kBvhMaxWorldTris = 0x1FFFFEu;   // the depth buffer's key holds 21 bits of triangle index
// dynamic LDS bytes one workgroup of the BVH kernel needs for `passInst` instance records
size_t bvhLdsBytes(uint32_t passInst, bool textured, bool classify, uint32_t groupViews, uint32_t texCap);

// What launchBvh launches for `p`, worked out the way it does (mrx_bvh_launch; include/mrx.h mrx_bvh_launch_t has
// the meaning of each field).  Host only.
struct BvhLaunchShape {
    int32_t flat;
    uint32_t tileW, tileH, classify, textured, recordCap, recordUsable, texCap, bigCap, passInst;
    uint32_t groupViews, mixed, priority, groupTiles, workgroups;
    int32_t smallArea;
};
BvhLaunchShape bvhLaunchShape(const RasterParams &p);

}  // namespace mrx
