/*
 * mrx.h -- C-ABI of the MI355X batch renderer (libmrx_hip.so).
 *
 * This is the drop-in boundary for the reference's per-frame hot path
 *   Manager::step()                      /root/reference/src/mgr.cpp:529-546
 * and the state around it that the path needs (construction, tensor export).
 * The reference's own boundary is the C++ class madRender::Manager
 * (/root/reference/src/mgr.hpp:29-120); its Python module binds that class
 * (/root/reference/src/bindings.cpp:123-233).  Everything below Manager --
 * the un-vendored Madrona executor, RenderingSystem, BatchRenderer and BVH
 * tracer -- is replaced by the HIP kernels behind these entry points.
 *
 * Plain C types only: pointers, sizes, PODs.  No torch, no C++ types.
 * Every function returns 0 on success or a negative MRX_E_* code;
 * mrx_last_error() gives the message of the calling thread's last failure.
 * The library is HIP-only: mrx_create() fails with MRX_E_NO_DEVICE when no
 * gfx950 device is usable -- there is no CPU fallback.
 */
#ifndef MRX_H
#define MRX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MRX_ABI_VERSION 4

enum {
    MRX_OK = 0,
    MRX_E_INVALID = -1,     /* bad argument / inconsistent config          */
    MRX_E_NO_DEVICE = -2,   /* no usable HIP device                        */
    MRX_E_HIP = -3,         /* a HIP runtime call failed                   */
    MRX_E_ASSET = -4,       /* an asset file could not be read or parsed   */
    MRX_E_UNSUPPORTED = -5  /* e.g. segmask in Rasterizer mode             */
};

/* Manager::RenderMode, /root/reference/src/mgr.hpp:31-34 */
enum { MRX_MODE_RASTERIZER = 0, MRX_MODE_RAYTRACER = 1 };

/* madRender::ImportedInstance, /root/reference/src/sim.hpp:31-36 (44 bytes,
 * rotation is w,x,y,z). */
typedef struct {
    float position[3];
    float rotation[4];
    float scale[3];
    int32_t object_id;
} mrx_instance;

/* madRender::ImportedCamera, /root/reference/src/sim.hpp:47-50 (28 bytes). */
typedef struct {
    float position[3];
    float rotation[4];
} mrx_camera;

/* madRender::Sim::WorldInit, /root/reference/src/sim.hpp:76-82 (16 bytes). */
typedef struct {
    uint32_t num_instances;
    uint32_t instances_offset;
    uint32_t num_cameras;
    uint32_t cameras_offset;
} mrx_world_init;

/* The projection of a camera (the vfov / znear arguments of RenderingSystem::attachEntityToView,
 * /root/reference/src/sim.cpp:168-171): vertical field of view in degrees, 0 < vfov_deg < 180, and the near
 * plane, znear > 0 (Raytracer mode: also < 1000, its far plane); znear = 0 means the mode's default (0.001 in
 * Rasterizer mode, 0.1 in Raytracer mode).  The defaults, {90, 0}, give the constants every view had before. */
typedef struct {
    float vfov_deg;
    float znear;
} mrx_projection;

/* The directional light of a world (the one light of the reference, its src/mgr.cpp:357, per world):
 * `direction` is the direction the light travels (any length but zero), `ambient` and `diffuse` the two constants
 * of DESIGN.md S7, lit = fma(diffuse, max(n.l, 0), ambient), both >= 0.  All five values finite.  The default,
 * {(1, -1, -0.05), 0.25, 0.75}, gives the colours every world had before. */
typedef struct {
    float direction[3];
    float ambient;
    float diffuse;
} mrx_light;

/* madrona::imp::SourceMaterial as the reference fills it,
 * /root/reference/src/bindings.cpp:44-49 (28 bytes). */
typedef struct {
    float color[4];
    int32_t texture_idx;    /* -1: untextured */
    float roughness;
    float metalness;
} mrx_material;

/* Manager::GeometryConfig, /root/reference/src/mgr.hpp:36-47. */
typedef struct {
    const float *vertices;              /* [num_vertices][3] */
    const float *uvs;                   /* [num_vertices][2] */
    const uint32_t *indices;            /* [num_indices]     */
    const uint32_t *mesh_vertex_offsets;/* [num_meshes]      */
    const uint32_t *mesh_index_offsets; /* [num_meshes]      */
    const int32_t *mesh_materials;      /* [num_meshes]      */
    uint32_t num_vertices;
    uint32_t num_indices;
    uint32_t num_meshes;
} mrx_geometry;

enum {
    /* also write a per-pixel int32 visibility buffer (world-local triangle
     * index, -1 = background); parity tests use it for bit-exact checks */
    MRX_FLAG_VISIBILITY_IDS = 1u << 0,
    /* several devices (device_ids): mrx_step only posts the render to the per-device host threads and returns;
     * every other entry point joins them first (the same as MRX_SHARD_ASYNC=1 in the environment) */
    MRX_FLAG_SHARD_ASYNC = 1u << 1,
    /* output selection (the engine's RenderMode RGBD / Depth, plus colour only): a render stores only
     * the outputs selected, and the tensor of an output that is not is never allocated -- mrx_buffer /
     * mrx_buffer_shard / mrx_copy_to_host on it fail with MRX_E_UNSUPPORTED.  The segmask (Raytracer
     * mode) and the visibility ids are written under every setting.  Both bits together: MRX_E_INVALID. */
    MRX_FLAG_NO_RGB = 1u << 2,      /* depth only */
    MRX_FLAG_NO_DEPTH = 1u << 3,    /* rgb only   */
    /* per-instance colour override: allocates the MRX_BUF_INSTANCE_COLOR column, zero-filled, and selects the launch
     * forms that read it.  Without it nothing is allocated, mrx_buffer / mrx_buffer_shard /
     * mrx_copy_to_host on the column fail with MRX_E_UNSUPPORTED and every launch is the one it always was. */
    MRX_FLAG_INSTANCE_COLORS = 1u << 4,
    /* per-instance material override: allocates the MRX_BUF_INSTANCE_MATERIAL column, filled with -1, and selects the
     * launch forms that read it.  Without it nothing is allocated, mrx_buffer / mrx_buffer_shard /
     * mrx_copy_to_host on the column fail with MRX_E_UNSUPPORTED and every launch is the one it always was.  With it
     * (and rgb rendered) the textured kernels are chosen when some material of the table is textured, whether or not
     * a drawn triangle is: a caller who wants the untextured kernels passes a table without textured materials. */
    MRX_FLAG_INSTANCE_MATERIALS = 1u << 5,
    /* surface-normal output: allocates the MRX_BUF_NORMAL tensor and selects the launch forms that store it (DESIGN.md
     * S10, 4.15).  It changes no other output and never which kernel family renders; it combines with MRX_FLAG_NO_RGB
     * (normals + depth) and with MRX_FLAG_NO_DEPTH (normals + rgb).  Without it nothing is allocated, mrx_buffer /
     * mrx_buffer_shard / mrx_copy_to_host on the tensor fail with MRX_E_UNSUPPORTED and every launch is the one it
     * always was. */
    MRX_FLAG_NORMALS = 1u << 6,
    /* per-instance labels: allocates the MRX_BUF_INSTANCE_LABEL column, filled with MRX_LABEL_OBJECT, and the ids
     * tensor in Rasterizer mode too, and selects the launch forms that read the column:
     * MRX_BUF_SEGMASK then holds, in both modes, the label of the instance row that wins each pixel.  Labels change
     * that tensor only.  Without the flag nothing is allocated, mrx_buffer / mrx_buffer_shard / mrx_copy_to_host on the
     * column fail with MRX_E_UNSUPPORTED, Rasterizer-mode MRX_BUF_SEGMASK fails as it always did and every launch is
     * the one it always was.  Together with MRX_FLAG_VISIBILITY_IDS the one ids tensor holds visibility ids:
     * the column exists and is mutable, MRX_BUF_SEGMASK is refused. */
    MRX_FLAG_INSTANCE_LABELS = 1u << 7,
    /* (bits 8 and 9: the supersampling factor, MRX_FLAG_SUPERSAMPLE_MASK below) */
    /* position output: allocates the MRX_BUF_POSITION tensor -- the 3-D point every pixel sees, xyzw, w = 0 where
     * nothing was hit -- and enqueues an unprojection stage behind every render (and resolve) on the same stream
     * (DESIGN.md S13, 4.19).  The points are in world space, or, with MRX_FLAG_POSITIONS_VIEW, in view space (+X right,
     * +Y forward, +Z up); that flag implies this one and means nothing else.  The stage reads the depth tensor the
     * caller sees, so MRX_FLAG_NO_DEPTH beside it is MRX_E_INVALID; it combines with everything else and changes no
     * other output.  Without it nothing is allocated, mrx_buffer / mrx_buffer_shard / mrx_copy_to_host on the tensor
     * fail with MRX_E_UNSUPPORTED and every launch is the one it always was. */
    MRX_FLAG_POSITIONS = 1u << 10,
    MRX_FLAG_POSITIONS_VIEW = 1u << 11
    /* (bits 12 ... 22: the number of box labels, MRX_FLAG_BOX_LABELS_MASK below) */
    /* (bits 23 ... 30: the packed observation output, MRX_FLAG_OBS_MASK below) */
};
/* supersampled antialiasing: a two-bit field of the flags holds the factor,
 * s = 1 + ((flags >> MRX_FLAG_SUPERSAMPLE_SHIFT) & 3), so s = 1 ... 4 and MRX_FLAG_SUPERSAMPLE(s) sets it.  With s > 1
 * the render runs exactly as a renderer of s * view_width x s * view_height views would (Raytracer mode: s * res
 * square) -- the sample tensors, mrx_sample_buffer -- and a resolve stage behind it on the same stream writes the
 * view_width x view_height tensors every other entry point sees: rgb box-filtered per byte, (sum + s*s/2) / (s*s);
 * depth, normals and the ids tensor unfiltered, each native pixel (x, y) taking sample (s*x + s/2, s*y + s/2).
 * s * view_width or s * view_height above 16384: MRX_E_INVALID.  With the field zero nothing is allocated and every
 * launch is the one it always was. */
#define MRX_FLAG_SUPERSAMPLE_SHIFT 8
#define MRX_FLAG_SUPERSAMPLE_MASK (3u << MRX_FLAG_SUPERSAMPLE_SHIFT)
#define MRX_FLAG_SUPERSAMPLE(s) ((((uint32_t)(s) - 1u) & 3u) << MRX_FLAG_SUPERSAMPLE_SHIFT)
/* box labels: an 11-bit field of the flags, bits 12 ... 22, holds K, the number of labels whose
 * 2-D bounding box and pixel count the renderer computes; MRX_FLAG_BOX_LABELS(k) sets it.  With K in 1 ... 1024 the
 * MRX_BUF_BOXES tensor is allocated and a box stage runs behind every render, resolve and unprojection on the same
 * stream: it reads the ids tensor the caller sees, which must be a segmask -- Raytracer mode, or Rasterizer mode with
 * MRX_FLAG_INSTANCE_LABELS, and in neither beside MRX_FLAG_VISIBILITY_IDS: MRX_E_INVALID otherwise, as is K > 1024.
 * It combines with everything else and changes no other output.  With the field zero nothing is allocated and every
 * launch is the one it always was. */
#define MRX_FLAG_BOX_LABELS_SHIFT 12
#define MRX_FLAG_BOX_LABELS_MASK (0x7FFu << MRX_FLAG_BOX_LABELS_SHIFT)
#define MRX_FLAG_BOX_LABELS(k) (((uint32_t)(k) & 0x7FFu) << MRX_FLAG_BOX_LABELS_SHIFT)
/* packed observation output: an 8-bit field of the flags, bits 23 ... 30 -- the layout in bits
 * 23 ... 25 (MRX_OBS_RGB ... MRX_OBS_YD, 0: no output), the element type in bits 26 and 27 (MRX_OBS_F32 ... MRX_OBS_U8)
 * and S - 1 in bits 28 ... 30, S = 1 ... 8 the number of stacked frames; MRX_FLAG_OBSERVATIONS(layout, dtype, stack)
 * sets it.  With a layout the MRX_BUF_OBSERVATION tensor [views, S * C, H, W] is allocated -- and, with S > 1, the
 * MRX_BUF_OBSERVATION_RESET column -- and an observation stage runs last behind every render on the same stream: it
 * reads the rgb and depth tensors the caller sees and writes the tensor a policy takes, channel first.  MRX_E_INVALID:
 * a layout with colour beside MRX_FLAG_NO_RGB, a layout with depth beside MRX_FLAG_NO_DEPTH, layout values 6 and 7,
 * element type or stack bits with layout 0.  It combines with everything else and changes no other output.  With the
 * field zero nothing is allocated and every launch is the one it always was. */
#define MRX_FLAG_OBS_SHIFT 23
#define MRX_FLAG_OBS_MASK (0xFFu << MRX_FLAG_OBS_SHIFT)
#define MRX_FLAG_OBS_LAYOUT_MASK (7u << MRX_FLAG_OBS_SHIFT)
#define MRX_FLAG_OBS_DTYPE_SHIFT 26
#define MRX_FLAG_OBS_DTYPE_MASK (3u << MRX_FLAG_OBS_DTYPE_SHIFT)
#define MRX_FLAG_OBS_STACK_SHIFT 28
#define MRX_FLAG_OBS_STACK_MASK (7u << MRX_FLAG_OBS_STACK_SHIFT)
#define MRX_FLAG_OBSERVATIONS(layout, dtype, stack)                                                                      \
    ((((uint32_t)(layout) & 7u) << MRX_FLAG_OBS_SHIFT) | (((uint32_t)(dtype) & 3u) << MRX_FLAG_OBS_DTYPE_SHIFT) |        \
     ((((uint32_t)(stack) - 1u) & 7u) << MRX_FLAG_OBS_STACK_SHIFT))
/* layouts: the channels of one frame -- rgb (C = 3), rgb and depth (4), depth (1), luma (1), luma and depth (2); luma
 * is y = (77 r + 150 g + 29 b + 128) >> 8 */
enum { MRX_OBS_NONE = 0, MRX_OBS_RGB = 1, MRX_OBS_RGBD = 2, MRX_OBS_D = 3, MRX_OBS_Y = 4, MRX_OBS_YD = 5 };
/* element types: float32, float16, bfloat16 (round to nearest even), uint8 */
enum { MRX_OBS_F32 = 0, MRX_OBS_F16 = 1, MRX_OBS_BF16 = 2, MRX_OBS_U8 = 3 };

/* the label that stands for "the id of the object the row is bound to" (INT32_MIN): what the column starts at */
#define MRX_LABEL_OBJECT ((int32_t)(-2147483647 - 1))

/* Manager::Config + Config::RenderConfig, /root/reference/src/mgr.hpp:49-88.
 * All pointers are borrowed for the duration of mrx_create() only. */
typedef struct {
    uint32_t struct_size;       /* = sizeof(mrx_config), ABI check */
    int32_t gpu_id;
    uint32_t num_worlds;
    int32_t render_mode;
    uint32_t view_width;
    uint32_t view_height;
    mrx_geometry geo;
    const char *const *asset_paths;
    uint32_t num_asset_paths;
    const int32_t *mat_assignments;     /* per asset path, -1 = none */
    uint32_t num_mat_assignments;
    const mrx_material *materials;
    uint32_t num_materials;
    const char *const *texture_paths;
    uint32_t num_textures;
    const mrx_instance *instances;
    uint32_t num_instances;
    const mrx_camera *cameras;
    uint32_t num_cameras;
    const mrx_world_init *worlds;       /* [num_worlds] */
    /* build-only knobs (no counterpart in the reference) */
    void *stream;               /* hipStream_t to launch on; NULL = null stream */
    uint32_t flags;             /* MRX_FLAG_* */
    int32_t kernel_variant;     /* 0 = default (raster kernels up to 128 triangles per
                                 * world, BVH path from 129 -- from 65 for batches of up to 640
                                 * 64x64 views, from 91 for up to 1024 untextured ones; and for
                                 * Raytracer-mode batches of many large views of small worlds:
                                 * mrx_dispatch_flat);
                                 * 1 = brute-force cross-check;
                                 * 2 = BVH path always; 3 = raster kernels always */
    /* -- ABI 3 (a caller that sets struct_size = MRX_CONFIG_V2_SIZE passes none of these) --
     * Single-process multi-device: with num_devices > 1 the renderer spans device_ids[0 ..
     * num_devices): the worlds are split into contiguous ranges (sizes differ by at most one,
     * as scenes.shard_range), one shard per listed device -- its own tensors, launched on that
     * device's null stream -- and mrx_step launches on all of them.  gpu_id is then ignored;
     * an id may repeat (several shards on one device).  The reference has a single gpuID
     * (/root/reference/src/mgr.hpp:50) and every caller constructs ONE Manager
     * (scripts/test.py:112-130, src/bindings.cpp:183-205): this is that constructor, wider. */
    const int32_t *device_ids;
    uint32_t num_devices;       /* 0 or 1: one device, gpu_id */
    /* Rows per world at least (0 = exactly num_instances of each world): the reference sizes
     * its renderer by maxInstancesPerWorld (/root/reference/src/mgr.cpp:378-388) and creates
     * renderables at run time (src/sim.inl:5-8).  Spare rows start hidden and unbound
     * (ObjectID -1, identity pose); see mrx_refresh_objects. */
    uint32_t max_instances_per_world;
    /* -- per-camera projection (a caller that sets struct_size = MRX_CONFIG_V4_SIZE or MRX_CONFIG_V2_SIZE passes
     * none): [num_cameras] entries parallel to `cameras`, NULL = every camera {90, 0}.  A view takes the projection
     * of the camera row it is assembled from (mrx_world_init.cameras_offset), as it takes its pose. */
    const mrx_projection *camera_projections;
    /* -- per-world light (a caller that sets struct_size to one of the sizes below passes none): [num_worlds]
     * entries parallel to `worlds`, NULL = every world the default light.  Every view of a world takes its world's. */
    const mrx_light *world_lights;
    /* -- per-instance colour override (a caller that sets struct_size to one of the sizes below passes none):
     * [num_instances][4] bytes (r, g, b, a) parallel to `instances`, the initial values of MRX_BUF_INSTANCE_COLOR --
     * expanded per world as the poses are, so worlds that alias rows get the same colours.  NULL = all zero;
     * non-NULL implies MRX_FLAG_INSTANCE_COLORS. */
    const uint8_t *instance_colors;
    /* reserved, must be zero.  (It also keeps sizeof(mrx_config) away from MRX_CONFIG_V4_LIGHT_SIZE + 8: a caller built
     * against the struct as it was before instance_colors that overstates its size by one pointer is still refused,
     * not read past its end.) */
    uint64_t reserved0;
} mrx_config;
#define MRX_CONFIG_V2_SIZE ((uint32_t)offsetof(mrx_config, device_ids))
#define MRX_CONFIG_V4_SIZE ((uint32_t)offsetof(mrx_config, camera_projections))
#define MRX_CONFIG_V4_PROJ_SIZE ((uint32_t)offsetof(mrx_config, world_lights))
#define MRX_CONFIG_V4_LIGHT_SIZE ((uint32_t)offsetof(mrx_config, instance_colors))

typedef struct mrx_renderer mrx_renderer;

/* Buffers of mrx_buffer(): the tensors Manager exports,
 * /root/reference/src/mgr.cpp:547-665 and ExportID /root/reference/src/sim.hpp:19-29. */
enum {
    MRX_BUF_RGB = 0,            /* u8  [views,H,W,4]  (Raytracer: [views,res,res,4]) */
    MRX_BUF_DEPTH = 1,          /* f32 [views,H,W,1]  (Raytracer: [views,res,res])   */
    MRX_BUF_SEGMASK = 2,        /* i32 [views,res,res], Raytracer only -- with MRX_FLAG_INSTANCE_LABELS in Rasterizer
                                 * mode too, [views,H,W]: per pixel the label of the winning row, -1 = background */
    MRX_BUF_INSTANCE_POSITION = 3, /* f32 [instances,3]                              */
    MRX_BUF_INSTANCE_ROTATION = 4, /* f32 [instances,4]  w,x,y,z                     */
    MRX_BUF_CAMERA_POSITION = 5,   /* f32 [cameras,3]                                */
    MRX_BUF_CAMERA_ROTATION = 6,   /* f32 [cameras,4]                                */
    MRX_BUF_VISIBILITY = 7,     /* i32 [views,H,W], needs MRX_FLAG_VISIBILITY_IDS    */
    MRX_BUF_INSTANCE_SCALE = 8, /* f32 [instances,3]                                 */
    /* i32 [instances], mutable: the ObjectID column of the renderables
     * (/root/reference/src/sim.cpp:152-156).  A negative value hides the instance
     * from the next step on (cleanupRenderableEntity, src/sim.inl:10-16), writing
     * the id back shows it again (makeEntityRenderable, src/sim.inl:5-8).  Only
     * the sign is interpreted: the geometry an instance draws is bound when the
     * renderer is created, triangle slots / visibility ids stay where they are, and
     * the segmask shows the id of the bound object (label and geometry always agree:
     * writing a different non-negative id changes neither) -- until
     * mrx_refresh_objects() re-binds the rows to the ids the column holds. */
    MRX_BUF_INSTANCE_OBJECT = 9,
    /* u8 [instances,4], mutable, needs MRX_FLAG_INSTANCE_COLORS: the colour override (r, g, b, a) of every row
     * (upstream's per-renderable colour override column).  a == 0: the row's triangles shade with their material
     * colour; a != 0: with (r, g, b) / 255 in its place (textured triangles are modulated by it).
     * The value of a beyond zero / non-zero is not interpreted, output alpha stays 255.  It changes colour only --
     * never which kernel runs, visibility, depth or the segmask -- and belongs to the row: it stays through hiding
     * (a negative ObjectID) and through mrx_refresh_objects(); spare rows start at 0.  Written on the device, like a
     * pose, on the renderer's stream; a depth-only renderer never reads it. */
    MRX_BUF_INSTANCE_COLOR = 10,
    /* the ids of ABI 4 as first shipped end here; MRX_NUM_BUFFERS_EXT counts the ones added since as well */
    MRX_NUM_BUFFERS = 11,
    /* i32 [instances], mutable, needs MRX_FLAG_INSTANCE_MATERIALS: the material override of every row (upstream's
     * per-renderable material override column).  m < 0 or m >= mrx_info_t.num_materials: none, the row's triangles
     * shade as their own materials say; otherwise every triangle of the row shades with material m of the renderer's
     * table (the API materials, then the ones of MTL files: what mesh_materials / mat_assignments index) -- its rgb
     * in S7, its texture, or none, in S8.  A colour override (MRX_BUF_INSTANCE_COLOR, a != 0) then
     * replaces that material's rgb.  It changes colour only -- never which kernel runs, visibility, depth or the
     * segmask -- and belongs to the row: it stays through hiding and through mrx_refresh_objects(); spare rows start
     * at -1.  Written on the device, like a pose, on the renderer's stream; a depth-only renderer never reads it. */
    MRX_BUF_INSTANCE_MATERIAL = 11,
    MRX_NUM_BUFFERS_EXT = 12,
    /* u8 [views,H,W,4] (Raytracer: [views,res,res,4], transposed like rgb), needs MRX_FLAG_NORMALS: the flat geometric
     * normal of the triangle that wins the pixel, in VIEW space (+X right, +Y forward, +Z up), unit length, turned
     * towards the eye, one byte per axis: b = (uint) fma(clamp(c, -1, 1), 127, 128.5), so 1 ... 255 with 128 = 0, and
     * a caller decodes (b - 128) / 127.  Alpha is 255 on a hit; background pixels hold (128, 128, 128, 0) -- the zero
     * vector, alpha 0 marks the miss.  Independent of winding, mirroring scales, light, material, colour override and
     * texture.  One tensor per shard, like rgb. */
    MRX_BUF_NORMAL = 12,
    MRX_NUM_BUFFERS_EXT2 = 13,
    /* i32 [instances], mutable, needs MRX_FLAG_INSTANCE_LABELS: the label of every row.  On the pixels
     * a row's triangles win, the segmask holds the row's label -- any int32, stored as it is, -1 and other negatives
     * included -- except MRX_LABEL_OBJECT (INT32_MIN), which stands for the id of the object the row is bound to: the
     * segmask value of a renderer without the column.  Background pixels hold -1.  It changes the ids tensor only --
     * never which kernel family renders, visibility, depth, rgb or normals -- and belongs to the row: it stays through
     * hiding and through mrx_refresh_objects() (a row at MRX_LABEL_OBJECT follows whatever object it is bound to);
     * spare rows start at MRX_LABEL_OBJECT.  Written on the device, like a pose, on the renderer's stream; read under
     * every output selection, a depth-only renderer included. */
    MRX_BUF_INSTANCE_LABEL = 13,
    MRX_NUM_BUFFERS_EXT3 = 14,
    /* f32 [views,H,W,4] (Raytracer: [views,res,res,4], transposed like rgb), needs MRX_FLAG_POSITIONS: per pixel the
     * point (x, y, z, 1) its depth stands for -- in world space, or in view space with MRX_FLAG_POSITIONS_VIEW -- and
     * (0, 0, 0, 0) where depth is 0 (background).  Computed from the depth tensor, the camera pose tensors and the
     * projection constants as they are when the stage runs: view space P = (d * rx, d, d * rz) with S5's
     * ray of the pixel centre (on a supersampled renderer: of the sample depth was taken from), world space
     * R(q) * P + c with the view's camRot / camPos rows -- the inverse of the camera transform for a unit quaternion
     * only: the quaternion is used as given, as everywhere.  An allocation of its own, one per shard. */
    MRX_BUF_POSITION = 14,
    MRX_NUM_BUFFERS_EXT4 = 15,
    /* i32 [views,K,5], needs the MRX_FLAG_BOX_LABELS field: row (v, l) is (xmin, ymin, xmax, ymax, count) of the pixels
     * of view v whose value in the ids tensor the caller sees (MRX_BUF_SEGMASK; the resolved one on a supersampled
     * renderer) equals l -- the smallest and largest image column and image row (row 0 up), all four inclusive, and the
     * number of pixels; (W, H, -1, -1, 0) where there is none (Raytracer mode: W = H = res).  Image coordinates in both
     * modes: the stage undoes the Raytracer transposition.  Ids outside 0 ... K-1 -- the background -1, negative
     * labels, labels >= K -- belong to no row.  An allocation of its own, one per shard; it has no
     * sample tensor. */
    MRX_BUF_BOXES = 15,
    MRX_NUM_BUFFERS_EXT5 = 16,
    /* f32 / f16 / bf16 / u8 [views, S*C, H, W], needs the MRX_FLAG_OBSERVATIONS field: channel f * C + c is channel c of
     * frame f, frame 0 the oldest and S - 1 the one just rendered; (H, W) are image rows and columns in both modes
     * (Raytracer: H = W = res, the stage undoes the transposition).  A colour byte b is (float)b * (1.0f / 255.0f)
     * (u8: b itself); depth is the depth tensor's value, or with a range (mrx_set_observation_depth_range)
     * d == 0 ? 1 : clamp((d - lo) * inv, 0, 1); u8 stores (uint32)(clamp(o, 0, 1) * 255.0f + 0.5f).
     * With S > 1 the tensor is state: every run of the stage pushes a frame.  An allocation of its own, one per shard;
     * it has no sample tensor. */
    MRX_BUF_OBSERVATION = 16,
    /* u8 [views], needs S > 1: a view whose byte is not zero when the stage runs has every frame of its stack set to
     * the current one.  Written on the device, like a pose, on the renderer's stream; starts at 1, and the renderer
     * clears it behind every run of the stage, so a flag is consumed by exactly the next run. */
    MRX_BUF_OBSERVATION_RESET = 17,
    MRX_NUM_BUFFERS_EXT6 = 18,
    /* The ray-cast sensor (mrx_rays_create); all four need it, are indexed by world and are per
     * shard, like the other outputs.
     * f32 [worlds,R,8], mutable, written like a pose: ray r of world w is (ox, oy, oz, tmin, dx, dy, dz, tmax), two
     * aligned 16-byte halves.  Zero-filled at creation: the zero ray misses. */
    MRX_BUF_RAYS = 18,
    /* i32 [worlds], mutable, written like a pose: the world-local instance row the world's rays are mounted on -- they
     * are then given in that row's frame, o = R(q) ol + p, d = R(q) dl with the row's live pose; its scale and ObjectID
     * are not read.  Any value outside 0 ... rows of the world - 1 means the world frame.  Starts at -1. */
    MRX_BUF_RAY_FRAME = 19,
    /* f32 [worlds,R]: the parameter t of the nearest hit, hit = o + t d (a distance when d has unit length); the ray's
     * own tmax, bit for bit, where nothing is hit. */
    MRX_BUF_RAY_DISTANCE = 20,
    /* i32 [worlds,R]: the segmask value of the instance row that was hit -- its label, or the id
     * of the object it is bound to -- and -1 on a miss. */
    MRX_BUF_RAY_ID = 21,
    MRX_NUM_BUFFERS_EXT7 = 22,
    /* f32 [views,H,W,4] (Raytracer: [views,res,res,4], transposed like rgb), needs mrx_flow_create (DESIGN.md S17,
     * 4.23): per native pixel (dx, dy, dz, 1) -- the surface point the pixel (x, y) sees was at image position
     * (x - dx, y - dy) when the snapshot was taken, that is at the previous step; dx runs along image columns and dy
     * along image rows in both modes; dz is the change of depth -- and (0, 0, 0, 0) on background, where the ids tensor
     * holds -1 and where the point lay behind the previous camera.  Camera motion, the rigid motion and the scale of
     * the instance the pixel's visibility id belongs to and a change of projection all count.  An allocation of its
     * own, one per shard; it has no sample tensor. */
    MRX_BUF_FLOW = 22,
    MRX_NUM_BUFFERS_EXT8 = 23,
    /* The point-cloud output (mrx_cloud_create); all three need it and are per shard, like the
     * other outputs; none has a sample tensor.
     * f32 [views,N,4]: slot k of view v is the point (x, y, z, 1) of one valid pixel of the view -- bit for bit what
     * MRX_BUF_POSITION holds at that pixel in the chosen frame -- or (0, 0, 0, 0) where the slot is empty.  A pixel is
     * valid where its depth d, in the depth tensor the caller sees, has d > 0 and, with a max_depth, d <= max_depth (a
     * NaN is not).  With M valid pixels, ranked in storage order (Raytracer mode: [x][y], column-major in image terms),
     * slot k takes the pixel of rank floor(k * M / N) where M >= N, rank k where k < M < N, and is empty where k >= M:
     * an even thinning that keeps storage order, the same from run to run. */
    MRX_BUF_CLOUD = 23,
    /* i32 [views,N]: y * W + x of the slot's pixel in image coordinates in both modes (Raytracer: W = res, the stage
     * undoes the transposition) -- what a caller gathers rgb, labels or normals with -- and -1 in an empty slot. */
    MRX_BUF_CLOUD_PIXEL = 24,
    /* i32 [views]: M, the valid pixels of the view -- not min(M, N). */
    MRX_BUF_CLOUD_COUNT = 25,
    MRX_NUM_BUFFERS_EXT9 = 26,
    /* The shadow mask (mrx_shadow_create); per shard, like the other outputs; it has no sample
     * tensor.  u8 [views,H,W] (Raytracer: [views,res,res], transposed), stored exactly like depth: 0 where the pixel's
     * point, in the depth tensor the caller sees, is cut off from the light of its world by a triangle of that world,
     * 255 on every other pixel, background included. */
    MRX_BUF_SHADOW = 26,
    MRX_NUM_BUFFERS_EXT10 = 27
};

enum { MRX_DTYPE_U8 = 0, MRX_DTYPE_I32 = 1, MRX_DTYPE_F32 = 2, MRX_DTYPE_F16 = 3, MRX_DTYPE_BF16 = 4 };

typedef struct {
    uint32_t num_worlds, num_views, num_instances;
    uint32_t num_objects, num_triangles, num_materials, num_textures;
    uint32_t max_world_triangles;   /* most triangles any one world draws  */
    uint32_t storage_fast, storage_slow; /* pixels per row / rows per view */
    int32_t device_id;
    int32_t kernel_variant;
    uint64_t bytes_per_step;        /* algorithmic HBM bytes of one render */
    int32_t render_path;            /* 0 = tiled raster kernels, 1 = BVH ray-trace path */
    uint32_t bvh_nodes;             /* 8-wide BLAS nodes of all objects     */
    uint32_t bvh_depth;             /* deepest BLAS                         */
    uint32_t max_world_instances;   /* most instances any one world holds   */
    /* -- ABI 3 (mrx_info writes none of these: see mrx_info_sized) -- */
    uint32_t num_shards;            /* devices the renderer spans (1 unless device_ids) */
} mrx_info_t;
#define MRX_INFO_V2_SIZE ((size_t)offsetof(mrx_info_t, num_shards))

/* -- lifetime: replaces Manager::Manager / ~Manager (mgr.cpp:505-527).
 *    Like the reference constructor, mrx_create renders the first frame. */
int mrx_create(const mrx_config *cfg, mrx_renderer **out);
void mrx_destroy(mrx_renderer *r);

/* -- per-frame: mrx_step == Manager::step (mgr.cpp:529-546); mrx_render is
 *    its render half (the north star's Manager::render()).  Both enqueue on
 *    the renderer's stream and return without waiting. */
int mrx_step(mrx_renderer *r);
int mrx_render(mrx_renderer *r);
int mrx_sync(mrx_renderer *r);

/* -- tensor export: replaces Manager::*Tensor()/ *CudaPtr() (mgr.cpp:547-665).
 *    Returns the device pointer (owned by the renderer, valid until
 *    mrx_destroy) or NULL on error. */
void *mrx_buffer(mrx_renderer *r, int which, int64_t dims[4], int *ndim,
                 int *dtype, int *device);

/* -- supersampling (MRX_FLAG_SUPERSAMPLE_MASK).  mrx_supersample returns the factor s, 1 ... 4 (MRX_E_INVALID for a
 *    null renderer).  On a renderer with s > 1 mrx_buffer / mrx_buffer_shard / mrx_copy_to_host give the resolved
 *    tensors, mrx_info the native storage_fast / storage_slow (bytes_per_step: the sample render's bytes plus what the
 *    resolve reads and writes), mrx_set_view_projection / mrx_view_projection speak in the caller's terms, and
 *    mrx_step / mrx_render / mrx_time_renders / the first frame of mrx_create enqueue the render and then the resolve.
 *    mrx_sample_buffer is mrx_buffer for the s * W x s * H tensor the render writes: same signature, ownership and
 *    lifetime; `which` is an output id (rgb, depth, segmask, visibility, normal).  NULL with MRX_E_UNSUPPORTED at
 *    s = 1, on an output that is not rendered, and on a renderer of several shards (address one shard).
 *    mrx_resolve enqueues the resolve stage alone on the renderer's stream (every shard's on its own), as mrx_render
 *    enqueues the render: what a caller that wrote the sample tensors itself, or timed the stage, calls.
 *    MRX_E_UNSUPPORTED at s = 1. */
int mrx_supersample(mrx_renderer *r);
void *mrx_sample_buffer(mrx_renderer *r, int which, int64_t dims[4], int *ndim,
                        int *dtype, int *device);
int mrx_resolve(mrx_renderer *r);

/* -- position output (MRX_FLAG_POSITIONS).  mrx_positions returns 0 (no position output), 1 (world space) or 2 (view
 *    space); MRX_E_INVALID for a null renderer.  With the output, mrx_step / mrx_render / mrx_time_renders / the first
 *    frame of mrx_create enqueue the render, the resolve where there is one, and then the unprojection stage.
 *    mrx_unproject enqueues that stage alone on the renderer's stream (every shard's on its own), as mrx_resolve does
 *    the resolve: what a caller that wrote depth, a camera pose or a projection itself, or timed the stage, calls.
 *    MRX_E_UNSUPPORTED without the output. */
int mrx_positions(mrx_renderer *r);
int mrx_unproject(mrx_renderer *r);

/* -- box labels (MRX_FLAG_BOX_LABELS).  mrx_box_labels returns K, or 0 without the output; MRX_E_INVALID for a null
 *    renderer.  With the output, mrx_step / mrx_render / mrx_time_renders / the first frame of mrx_create enqueue the
 *    render, the resolve and the unprojection where there are any, and then the box stage.  mrx_boxes enqueues that
 *    stage alone on the renderer's stream (every shard's on its own), as mrx_unproject does: what a caller that wrote
 *    the ids tensor itself, or timed the stage, calls.  MRX_E_UNSUPPORTED without the output.
 *    mrx_box_plan is host arithmetic, for tests: the answer of the stage's launch checks for a tensor of `views` views
 *    of nslow rows of nfast pixels and K labels on num_cus compute units (null_pointers != 0: with a null tensor) --
 *    MRX_E_INVALID where the launch would be refused, 0 where it would enqueue nothing, otherwise the number of
 *    workgroups per view (forced_parts: MRX_BOX_PARTS, 0 = the automatic rule).  It touches no device. */
int mrx_box_labels(mrx_renderer *r);
int mrx_boxes(mrx_renderer *r);
int mrx_box_plan(uint32_t views, uint32_t nfast, uint32_t nslow, uint32_t k, uint32_t num_cus, uint32_t forced_parts,
                 int null_pointers);

/* -- packed observation output (MRX_FLAG_OBSERVATIONS).  mrx_observations returns the field as it lies in the flags
 *    (flags & MRX_FLAG_OBS_MASK: a positive int, read with the mask macros), or 0 without the output; MRX_E_INVALID for a null renderer.  With the
 *    output, mrx_step / mrx_render / mrx_time_renders / the first frame of mrx_create enqueue the render, the resolve,
 *    the unprojection and the boxes where there are any, and then the observation stage.  mrx_observe enqueues that
 *    stage alone on the renderer's stream (every shard's on its own), as mrx_unproject does; on a stacked renderer it
 *    pushes one more frame.  mrx_set_observation_depth_range stores the range depth is normalised to, 0 <= lo < hi,
 *    both finite (lo = hi = 0: no range, depth is stored raw; anything else MRX_E_INVALID) -- the stage then uses
 *    inv = 1.0f / (hi - lo) -- marks every view reset and enqueues the stage: frames packed under another range are
 *    meaningless.  A renderer starts without a range.  MRX_E_INVALID for a layout without depth beside a range.
 *    mrx_observation_depth_range reads it back (0, 0 without).  MRX_E_UNSUPPORTED without the output. */
int mrx_observations(mrx_renderer *r);
int mrx_observe(mrx_renderer *r);
int mrx_set_observation_depth_range(mrx_renderer *r, float lo, float hi);
int mrx_observation_depth_range(mrx_renderer *r, float *lo, float *hi);

/* -- ray-cast sensor.  The flag word is full and mrx_config keeps its size, so the sensor is
 *    attached after creation: mrx_rays_create(r, R) allocates the four MRX_BUF_RAY* tensors for R rays per world, 1 ...
 *    65536 with worlds * R < 2^31, and from then on mrx_step / mrx_render / mrx_time_renders enqueue the trace stage
 *    last on the render's stream, behind the render, the resolve, the unprojection, the boxes and the observation.  It
 *    is called once: a second call, or R out of range, returns MRX_E_INVALID; on a renderer of several shards it fans
 *    out (a shard cannot be given a sensor on its own).  MRX_RAYS_BRUTE=1 in the environment at that call selects the
 *    form of the kernel that skips every cull, MRX_RAY_PASS_ROWS=n stages n rows of a world at a time (tests).
 *    mrx_rays returns R, or 0 without the sensor; MRX_E_INVALID for a null renderer.  mrx_trace enqueues the stage
 *    alone on the renderer's stream (every shard's on its own), as mrx_boxes does: what a caller that only wrote rays
 *    or poses calls.  MRX_E_UNSUPPORTED without the sensor.  The stage reads the ray tensors, the live pose, scale,
 *    ObjectID and label columns and the geometry tables; it writes MRX_BUF_RAY_DISTANCE and MRX_BUF_RAY_ID only.
 *    mrx_set_rays copies `count` worlds of rays, [count][R][8] host floats, into MRX_BUF_RAYS from world first_world on,
 *    on the renderer's stream, and waits for the copy: what a host program without the HIP runtime at hand calls
 *    (a caller with device tensors writes the buffer itself).  One shard at a time, like mrx_copy_to_host.
 *    mrx_ray_plan is host arithmetic, for tests: the answer of the stage's launch checks for `worlds` worlds of R rays
 *    over a scene whose deepest BLAS has bvh_depth levels, on num_cus compute units (null_pointers != 0: with null
 *    tensors; pass_rows: MRX_RAY_PASS_ROWS, 0 = the default) -- MRX_E_INVALID where the launch would be refused,
 *    otherwise the number of workgroups (0: nothing is enqueued), and out[0 ... 3], when not null, = workgroups per
 *    world, stack entries per lane, rows per staging pass, dynamic LDS bytes.  It touches no device.
 *    mrx_trace_rays_host runs the stage's source on the CPU, for tests; it touches no device and sets no error text.
 *    tri_pos [num_tris][9] are the triangles of num_objects objects (obj_first / obj_count index them); `instances`
 *    are the rows of all worlds, world-major (world_inst_start [num_worlds + 1]) -- a row draws object object_id, a
 *    negative id hides it --; labels_or_null [num_instances] is the label column, frame_or_null [num_worlds] the mount
 *    rows (null: world frame), rays [num_worlds][rays_per_world][8]; brute != 0 skips every cull.  It builds the BLAS
 *    as mrx_create does and writes out_t / out_id [num_worlds][rays_per_world]. */
int mrx_rays_create(mrx_renderer *r, uint32_t rays_per_world);
int mrx_rays(mrx_renderer *r);
int mrx_trace(mrx_renderer *r);
int mrx_set_rays(mrx_renderer *r, uint32_t first_world, uint32_t count, const float *rays);
int mrx_ray_plan(uint32_t worlds, uint32_t rays_per_world, uint32_t bvh_depth, uint32_t num_cus, uint32_t pass_rows,
                 int null_pointers, uint32_t out[4]);
int mrx_trace_rays_host(const float *tri_pos, uint32_t num_tris, const int32_t *obj_first, const int32_t *obj_count,
                        uint32_t num_objects, const mrx_instance *instances, uint32_t num_instances,
                        const int32_t *labels_or_null, const uint32_t *world_inst_start, uint32_t num_worlds,
                        const int32_t *frame_or_null, const float *rays, uint32_t rays_per_world, int brute,
                        float *out_t, int32_t *out_id);

/* -- optical-flow output.  Attached after creation, as the sensor is: mrx_flow_create(r) allocates
 *    MRX_BUF_FLOW and a device snapshot of the instance position, rotation and scale columns, the camera position and
 *    rotation columns and every view's projection constants, takes the snapshot and computes a first, still-scene flow.
 *    From then on mrx_step / mrx_render / mrx_time_renders enqueue two more kernels last on the render's stream, behind
 *    the trace stage: the flow, which reads the depth and ids tensors the caller sees, the live columns and constants
 *    and the snapshot, and then the snapshot of the live state for the next step.  MRX_E_INVALID unless the renderer
 *    has MRX_FLAG_VISIBILITY_IDS and renders depth, at 2^32 native pixels or more, on a second call and on a shard; on
 *    a renderer of several shards it fans out, all or nothing.  mrx_flow_enabled returns 1 or 0; MRX_E_INVALID for a null
 *    renderer.  mrx_flow enqueues the flow kernel alone (every shard's on its own stream): it does not advance the
 *    snapshot, so calling it twice gives the same tensor.  mrx_flow_snapshot enqueues the snapshot alone: what a caller
 *    that teleported bodies on an episode reset calls after writing the poses, so that the reset shows no motion.
 *    Both MRX_E_UNSUPPORTED without the output.  MRX_FLOW_PASS_ROWS=n in the environment at mrx_flow_create stages n
 *    rows of a world at a time (tests).
 *    mrx_flow_host runs the stage's source on the CPU, for tests; it touches no device and sets no error text.  depth
 *    and ids are [views][nslow][nfast] in storage order (transposed != 0: [x][y]), s the supersampling factor; consts
 *    is sx ox sz oz -- [views][4] with consts_per_view != 0, else one set for all views --, prev_consts always
 *    [views][4]; inst_kbase [num_instances], world_inst_start [num_worlds + 1], view_world [views]; live and prev are
 *    each five arrays: instance position [I][3], rotation [I][4], scale [I][3], camera position [views][3], rotation
 *    [views][4]; pass_rows as MRX_FLOW_PASS_ROWS (0: the default).  It writes out_flow [views][nslow][nfast][4]. */
int mrx_flow_create(mrx_renderer *r);
int mrx_flow_enabled(mrx_renderer *r);
int mrx_flow(mrx_renderer *r);
int mrx_flow_snapshot(mrx_renderer *r);
int mrx_flow_host(const float *depth, const int32_t *ids, uint32_t views, uint32_t nfast, uint32_t nslow,
                  int transposed, uint32_t s, const float *consts, int consts_per_view, const float *prev_consts,
                  const uint32_t *inst_kbase, const uint32_t *world_inst_start, const uint32_t *view_world,
                  uint32_t num_worlds, uint32_t num_instances, const float *const live[5], const float *const prev[5],
                  uint32_t pass_rows, float *out_flow);

/* -- point-cloud output.  Attached after creation, as the sensor and the flow are:
 *    mrx_cloud_create(r, N, frame, max_depth) allocates MRX_BUF_CLOUD, MRX_BUF_CLOUD_PIXEL and MRX_BUF_CLOUD_COUNT for N
 *    points per view, 1 ... 65536 with views * N < 2^31, runs the stage once and waits.  frame is 1 for world space and
 *    2 for view space, mrx_positions' values; max_depth is 0 for none, otherwise finite and > 0: pixels farther away
 *    are dropped.  From then on mrx_step / mrx_render / mrx_time_renders enqueue the compaction stage last on the
 *    render's stream, behind every other stage; bytes_per_step grows by 4 per native pixel and N * 20 + 4 per view.
 *    MRX_E_INVALID for a null renderer, a shard, a second call, N out of range, views * N at 2^31 or more, another
 *    frame, another max_depth, a renderer without depth (MRX_FLAG_NO_DEPTH), more than 2^32 - 1 native pixels or more
 *    than 2^31 - 1 in one view; on a renderer of several shards it fans out, all or nothing.  MRX_CLOUD_PARTS=n in the
 *    environment at that call splits every view over n workgroups (tests; the result does not depend on it).
 *    mrx_cloud returns N, or 0 without the output; MRX_E_INVALID for a null renderer.  mrx_compact enqueues the stage
 *    alone on the renderer's stream (every shard's on its own), as mrx_unproject does: what a caller that wrote depth, a
 *    camera pose or a projection itself, or timed the stage, calls.  MRX_E_UNSUPPORTED without the output.
 *    mrx_cloud_plan is host arithmetic, for tests: the answer of the stage's launch checks for `views` views of nslow
 *    rows of nfast pixels and n points on num_cus compute units (null_pointers != 0: with null tensors; forced_parts:
 *    MRX_CLOUD_PARTS, 0 = the automatic rule) -- MRX_E_INVALID where the launch would be refused, otherwise the number
 *    of workgroups (0: nothing is enqueued), and out[0 ... 2], when not null, = workgroups per view, LDS bytes of a
 *    workgroup, 1 where the slot rule runs in 64 bits (nfast * nslow * n reaches 2^32).  It touches no device.
 *    mrx_cloud_host runs the stage's source on the CPU, part by part and segment by segment as the kernels walk them,
 *    for tests; it touches no device and sets no error text.  depth is [views][nslow][nfast] in storage order
 *    (transposed != 0: [x][y]), s the supersampling factor, consts sx ox sz oz [views][4], cam_pos [views][3], cam_rot
 *    [views][4] (both may be null in view space), parts as MRX_CLOUD_PARTS (0: one).  It writes out_points
 *    [views][n][4] (16-byte aligned), out_pixel [views][n] and out_count [views]. */
int mrx_cloud_create(mrx_renderer *r, uint32_t points_per_view, int frame, float max_depth);
int mrx_cloud(mrx_renderer *r);
int mrx_compact(mrx_renderer *r);
int mrx_cloud_plan(uint32_t views, uint32_t nfast, uint32_t nslow, uint32_t n, uint32_t num_cus, uint32_t forced_parts,
                   int null_pointers, uint32_t out[3]);
int mrx_cloud_host(const float *depth, uint32_t views, uint32_t nfast, uint32_t nslow, int transposed, uint32_t s,
                   const float *consts, const float *cam_pos, const float *cam_rot, int frame, float max_depth,
                   uint32_t n, uint32_t parts, float *out_points, int32_t *out_pixel, int32_t *out_count);

/* -- cast shadows.  Attached after creation, as the sensor, the flow and the cloud are:
 *    mrx_shadow_create(r, apply, bias, max_distance) allocates MRX_BUF_SHADOW, runs the stage once in its mask-only form
 *    and waits.  Per native pixel with depth z > 0 one ray leaves the pixel's world point (MRX_BUF_POSITION's, world
 *    space) towards the light of the view's world, from t = bias * z (bias finite and >= 0; MRX_SHADOW_DEFAULT_BIAS) to
 *    t = max_distance (MRX_SHADOW_NO_MAX_DISTANCE = FLT_MAX for none, otherwise finite and > 0); the mask holds 0 where
 *    some triangle of a visible row of the world is in its way, 255 elsewhere.  From then on mrx_step / mrx_render /
 *    mrx_time_renders enqueue the shadow stage behind the unprojection and ahead of the boxes and the observation; with
 *    apply != 0 that launch also scales the rgb of an occluded pixel down to its ambient term, lit = diffuse * max(n . l,
 *    0) + ambient from the normal tensor's bytes, f = ambient / lit where lit > ambient, so a packed observation holds the
 *    shadowed colours.  bytes_per_step grows by 5 per native pixel.  MRX_E_INVALID, each with its own text, for a null
 *    renderer, a shard, a second call, a bias or max_distance out of range, a renderer without depth, apply on a
 *    renderer without rgb or without MRX_FLAG_NORMALS, more than 2^32 - 1 native pixels; on a renderer of several
 *    shards it fans out, all or nothing.  MRX_SHADOW_BRUTE=1 in the environment at that call selects the form of the
 *    kernel that skips every cull, MRX_SHADOW_PASS_ROWS=n stages n rows of a world at a time (tests).
 *    mrx_shadows returns 0 (off), 1 (mask) or 2 (mask and rgb); MRX_E_INVALID for a null renderer.  mrx_shadow enqueues
 *    the stage alone on the renderer's stream (every shard's on its own) in its MASK-ONLY form whatever apply is: calling
 *    it any number of times leaves rgb as the last step left it.  MRX_E_UNSUPPORTED without the stage.
 *    mrx_shadow_plan is host arithmetic, for tests: the answer of the stage's launch checks for `views` views of nslow
 *    rows of nfast pixels at supersampling factor s over a scene whose deepest BLAS has bvh_depth levels, on num_cus
 *    compute units (pass_rows: MRX_SHADOW_PASS_ROWS, 0 = the default; bad_pointers: 0 none, 1 null tensors, 2 a depth
 *    tensor off a 4-byte boundary, 3 an rgb tensor off one) -- MRX_E_INVALID where the launch would be refused,
 *    otherwise the number of workgroups (0: nothing is enqueued), and out[0 ... 3], when not null, = workgroups per view,
 *    stack entries per lane, rows per staging pass, dynamic LDS bytes.  It touches no device.
 *    mrx_shadow_host runs the stage's source on the CPU, for tests; it touches no device and sets no error text.
 *    Geometry as mrx_trace_rays_host takes it; depth [views][nslow][nfast] in storage order (transposed != 0: [x][y]), s
 *    the supersampling factor, consts sx ox sz oz [views][4], cam_pos [views][3], cam_rot [views][4] as mrx_cloud_host
 *    takes them; view_world [views]; lights [views][5] = toLight xyz, ambient, diffuse as mrx_light_constants resolves
 *    them; pass_rows as MRX_SHADOW_PASS_ROWS; brute != 0 skips every cull.  rgb_or_null and normal_or_null
 *    [views][nslow][nfast] packed pixels, both or neither: with them the applying form runs and rgb is changed in
 *    place.  It builds the BLAS as mrx_create does and writes out_mask [views][nslow][nfast]. */
#define MRX_SHADOW_DEFAULT_BIAS (1.0f / 1024.0f)
#define MRX_SHADOW_NO_MAX_DISTANCE 3.402823466e+38f
int mrx_shadow_create(mrx_renderer *r, int apply, float bias, float max_distance);
int mrx_shadows(mrx_renderer *r);
int mrx_shadow(mrx_renderer *r);
int mrx_shadow_plan(uint32_t views, uint32_t nfast, uint32_t nslow, uint32_t s, uint32_t bvh_depth, uint32_t num_cus,
                    uint32_t pass_rows, int apply, float bias, float max_distance, int bad_pointers, uint32_t out[4]);
int mrx_shadow_host(const float *tri_pos, uint32_t num_tris, const int32_t *obj_first, const int32_t *obj_count,
                    uint32_t num_objects, const mrx_instance *instances, uint32_t num_instances,
                    const uint32_t *world_inst_start, uint32_t num_worlds, const float *depth, uint32_t views,
                    uint32_t nfast, uint32_t nslow, int transposed, uint32_t s, const float *consts,
                    const float *cam_pos, const float *cam_rot, const uint32_t *view_world, const float *lights,
                    float bias, float max_distance, uint32_t pass_rows, int brute, uint32_t *rgb_or_null,
                    const uint32_t *normal_or_null, uint8_t *out_mask);

/* -- debug readback: waits for the stream, then copies the first `bytes`
 *    bytes of a buffer to host memory (what /root/reference/src/dump.cpp:53-70
 *    does with cudaMemcpy). */
int mrx_copy_to_host(mrx_renderer *r, int which, void *dst, uint64_t bytes);

/* -- re-binding (makeEntityRenderable at run time, /root/reference/src/sim.inl:5-8): reads
 *    the ObjectID column back and binds every row whose id is non-negative and differs from
 *    the object it draws to that object -- a spare row (max_instances_per_world) gets its
 *    geometry this way, an existing row swaps it.  Rows holding a negative id stay bound to
 *    what they drew (hidden).  World-local triangle indices (visibility ids) are renumbered in
 *    row order; the kernel and its launch shape are chosen again for the new triangle counts.
 *    Waits for the stream; pose tensors and outputs keep their addresses. */
int mrx_refresh_objects(mrx_renderer *r);

/* -- shards (device_ids): mrx_num_shards = devices the renderer spans; mrx_shard returns shard i
 *    as a renderer of its own -- valid with every function here until the parent is destroyed
 *    (never destroy a shard) -- whose tensors hold its world range; mrx_buffer_shard is
 *    mrx_buffer(mrx_shard(r, i), ...).  On a renderer of several shards mrx_step / mrx_render /
 *    mrx_sync / mrx_refresh_objects / mrx_time_renders act on all of them, mrx_info adds up,
 *    and mrx_buffer / mrx_copy_to_host / mrx_set_stream want a shard (MRX_E_UNSUPPORTED). */
/*    Host side: mrx_step has the launches enqueued by one thread per device and returns when all are queued
 *    (MRX_SHARD_THREADS=0: by the calling thread, one after the other).  MRX_SHARD_ASYNC=1 in the environment of
 *    mrx_create: mrx_step only posts the render to those threads and returns; every other entry point here, called
 *    on the renderer or on one of its shards, waits for them to have enqueued everything posted. */
int mrx_num_shards(mrx_renderer *r);
mrx_renderer *mrx_shard(mrx_renderer *r, int shard);
void *mrx_buffer_shard(mrx_renderer *r, int shard, int which, int64_t dims[4], int *ndim,
                       int *dtype, int *device);
/*    first world of shard i in the renderer's world order (shard i owns worlds
 *    [mrx_shard_first_world(i), mrx_shard_first_world(i + 1)); i = num_shards gives num_worlds) */
int64_t mrx_shard_first_world(mrx_renderer *r, int shard);
/*    the split itself (host only, no renderer needed): first world of shard `shard` of
 *    `num_shards` over `num_worlds` worlds; shard = num_shards gives num_worlds */
int64_t mrx_shard_split(uint32_t num_worlds, uint32_t shard, uint32_t num_shards);

/* -- mrx_info writes the first MRX_INFO_V2_SIZE bytes of mrx_info_t -- the struct as ABI 2 declared
 *    it, whatever the caller was compiled against; mrx_info_sized(r, &info, sizeof info) writes
 *    min(size, sizeof(mrx_info_t)) bytes, so a caller gets exactly the fields it knows (ABI 4).
 *    The struct only ever grows at its end. */
/* -- which kernel the last render launched, as the host picked it: MRX_ENTRY_NONE before the first render
 *    (mrx_create renders once), then one of the raster entries -- the group kernel's FAST instantiations, the
 *    group kernel, the chunked kernel, the brute-force kernel -- or the BVH path.  A renderer that spans several
 *    devices reports its first shard's; MRX_E_INVALID for a null renderer. */
enum {
    MRX_ENTRY_NONE = 0, MRX_ENTRY_GROUP_FAST = 1, MRX_ENTRY_GROUP = 2, MRX_ENTRY_CHUNKED = 3,
    MRX_ENTRY_BRUTE = 4, MRX_ENTRY_BVH = 5
};
int mrx_raster_entry(mrx_renderer *r);
/* -- which instantiation of that kernel: the form the launcher picked from the renderer's per-view tables, columns and
 *    extra outputs (MRX_FORM_UNIFORM: the uniform kernels, and before the first render) and, for the
 *    group kernel, the triangle slots per view it launched with (16 ... 256; 0 for every other kernel).  Read-only,
 *    host side: no kernel sees either value.  A renderer that spans several devices reports its first shard's;
 *    MRX_E_INVALID for a null renderer or output. */
enum {
    MRX_FORM_UNIFORM = 0, MRX_FORM_PV = 1, MRX_FORM_PVL = 2, MRX_FORM_C = 3, MRX_FORM_PVLC = 4, MRX_FORM_M = 5,
    MRX_FORM_PVLM = 6, MRX_FORM_N = 7, MRX_FORM_NPV = 8, MRX_FORM_L = 9, MRX_FORM_LN = 10, MRX_FORM_PVM = 11
};
typedef struct {
    int32_t form;              /* MRX_FORM_* */
    int32_t slots;             /* group kernel: triangle slots per view; else 0 */
} mrx_kernel_form_t;
int mrx_kernel_form(mrx_renderer *r, mrx_kernel_form_t *out);
/* -- the BVH path's launch shape as the host chose it for the bound geometry (mrx_create, mrx_refresh_objects):
 *    what the next BVH render launches.  kernel is MRX_BVH_KERNEL_NONE when the raster kernels render; the other
 *    fields are filled in all the same.  The flat kernel has no record table or large-triangle list (their caps
 *    read 0).  A renderer that spans several devices reports its first shard's; MRX_E_INVALID for a null
 *    renderer or output. */
enum { MRX_BVH_KERNEL_NONE = 0, MRX_BVH_KERNEL_TILE = 1, MRX_BVH_KERNEL_FLAT = 2 };
typedef struct {
    int32_t kernel;            /* MRX_BVH_KERNEL_* */
    uint32_t tile_w, tile_h;   /* pixels of a workgroup's tile, over the storage axes (fast, slow) */
    uint32_t classify;         /* the instantiation that classifies listed large triangles per strip */
    uint32_t textured;         /* the textured instantiation (48-byte records) */
    uint32_t record_cap;       /* records a round's table holds: textured tex_cap, else 512 / 768 / 1024 */
    uint32_t record_usable;    /* of them usable before the round ends (slot 1023 marks stashed pixels) */
    uint32_t tex_cap;          /* records of a textured round (bvhTexCap, 64 ... 1008) */
    uint32_t big_cap;          /* large-triangle list entries per round (64, 96 with classify) */
    uint32_t pass_inst;        /* TLAS instances per pass */
    uint32_t group_views;      /* views per workgroup: 1, 2, 4 or 8 */
    uint32_t mixed;            /* pairs and single views in one launch (group_views = 2) */
    uint32_t priority;         /* wave-priority mode of the younger workgroups (0 off) */
    uint32_t group_tiles;      /* tiles of a view per workgroup, one after the other */
    int32_t small_area;        /* triangles whose box in the tile covers more pixels go on the large list */
    uint32_t workgroups;       /* of the launch */
} mrx_bvh_launch_t;
int mrx_bvh_launch(mrx_renderer *r, mrx_bvh_launch_t *out);
int mrx_info(mrx_renderer *r, mrx_info_t *out);
int mrx_info_sized(mrx_renderer *r, void *out, size_t size);
void *mrx_stream(mrx_renderer *r);
/* -- stream: later launches are enqueued on `stream` (a hipStream_t; NULL = the
 *    device's null stream).  Work already enqueued on the old stream is waited
 *    for first, so the switch never reorders two renders.  A caller that
 *    writes the pose tensors from its own stream (e.g. a non-default torch
 *    stream) passes that stream here and needs no host synchronisation between
 *    the write and mrx_step(): both are ordered on the one stream. */
int mrx_set_stream(mrx_renderer *r, void *stream);

/* -- measurement: enqueue `steps` back-to-back mrx_render launches between
 *    two HIP events on the renderer's stream; *ms_total = elapsed device ms.
 *    Synchronises the stream before returning. */
int mrx_time_renders(mrx_renderer *r, int steps, float *ms_total);
/*    Host side of the same loop: `steps` mrx_step calls back to back with no synchronisation in
 *    between; *us_per_step = host wall time until the last call returned, per call (what the
 *    calling thread pays to have one step enqueued on every device).  Synchronises afterwards. */
int mrx_time_steps_host(mrx_renderer *r, int steps, double *us_per_step);
/*    mrx_mark(r, 0 | 1) records HIP event 0 / 1 on the renderer's stream;
 *    mrx_elapsed_ms waits for event 1 and returns event1 - event0.  They let a
 *    caller bracket its own timed region of mrx_step calls with device time. */
/*    Diagnostic: with MRX_DEBUG_STAMPS=1 in the environment at mrx_create, the
 *    kernels record per-wave timestamps; mrx_debug_stamps copies them out
 *    ([workgroups][4 waves][8] u64, 100 MHz ticks). Returns the count copied. */
int64_t mrx_debug_stamps(mrx_renderer *r, uint64_t *dst, int64_t capacity);
int mrx_mark(mrx_renderer *r, int which);
int mrx_elapsed_ms(mrx_renderer *r, float *ms);
/*    Output placement (outputs of 256 MiB and more: mrx_create times at most two
 *    candidate allocations and keeps the faster): writes the us per
 *    render of the candidates timed, in order (up to `capacity`), and of the one kept;
 *    returns how many were timed -- 0 when the layout needed no search. */
int mrx_placement(mrx_renderer *r, float *cand_us, int capacity, float *kept_us);

/* -- loader cross-check (host copies of what was uploaded) */
int mrx_copy_triangles(mrx_renderer *r, float *tri_pos /*[T][9]*/,
                       float *tri_uv /*[T][6]*/, int32_t *tri_mat /*[T]*/,
                       int32_t *obj_first /*[O]*/, int32_t *obj_count /*[O]*/);

/* -- host-only asset readers (no device needed); free results with mrx_free */
int mrx_load_obj(const char *path, float **tri_pos, float **tri_uv,
                 uint32_t *num_tris);
/*    The `o` / `g` blocks (with faces) of an OBJ file: writes up to `capacity`
 *    first-triangle indices and returns the block count, or a negative MRX_E_*.
 *    mrx_create makes ONE object of an asset file, as the reference does
 *    (importFromDisk(..., one_object_per_asset = true), /root/reference/src/mgr.cpp:301-303;
 *    objects[i] <-> asset path i, :340-345) -- the blocks are its meshes; with
 *    MRX_OBJ_SPLIT_BLOCKS=1 in the environment every block becomes an object of its own. */
int mrx_obj_objects(const char *path, uint32_t *first_tri, uint32_t capacity);
int mrx_decode_png(const char *path, uint8_t **rgba, uint32_t *width,
                   uint32_t *height);
/*    Texture files as mrx_create reads them: .ktx2 (BC7 or RGBA8 base level,
 *    decoded to RGBA8 on the host -- the reference's "ktx2" handler,
 *    /root/reference/src/mgr.cpp:199-212,297-298) or PNG. */
int mrx_decode_texture(const char *path, uint8_t **rgba, uint32_t *width,
                       uint32_t *height);
/*    BC7 blocks (16 bytes each) -> RGBA8, 16 pixels per block, row-major in the block. */
int mrx_decode_bc7(const uint8_t *blocks, uint32_t num_blocks, uint8_t *rgba /*[num_blocks][16][4]*/);
/*    What the OBJ reader makes of a file's material statements, as JSON text:
 *    {"num_tris":N,"tri_mtl":[...],"names":[...],"libs":[...],
 *     "materials":[{"name":..,"kd":[r,g,b],"map_kd":..},...]} (materials = every
 *    newmtl of the file's mtllibs).  Returns the length, or a negative MRX_E_*. */
int64_t mrx_describe_obj_materials(const char *path, char *json, uint64_t capacity);
/*    Builds the bottom-level BVH of one triangle soup exactly as mrx_create does
 *    for an object (the counterpart of AssetProcessor::makeBVHData,
 *    /root/reference/src/mgr.cpp:472-473) and checks its invariants: every
 *    triangle sits in exactly one leaf, every child box contains all that hangs
 *    below it, leaves hold at most 16 triangles, the traversal stack bound
 *    holds.  Returns MRX_OK or MRX_E_INVALID; counts are 0 for soups small
 *    enough to need no hierarchy. */
int mrx_blas_check(const float *tri_pos /*[T][9]*/, uint32_t num_tris, uint32_t *num_nodes,
                   uint32_t *depth, uint32_t *num_leaves);
void mrx_free(void *p);
/*    The dispatch rules that depend on the size of the device, as pure functions (host only): the triangles
 *    per world from which the default dispatch takes the BVH path for a batch of `num_views` views of
 *    width x height pixels on a device of `num_cus` compute units (`base` = the general threshold, 0 = the
 *    built-in 129), and the workgroups of the raster group kernel from which a launch counts as filling the
 *    chip.  mrx_create reads the CU count from the device (hipDeviceAttributeMultiprocessorCount). */
uint32_t mrx_dispatch_min_tris(uint32_t base, uint32_t num_views, int textured, uint32_t width, uint32_t height,
                               uint32_t num_cus);
uint32_t mrx_group_fill(uint32_t num_cus);
/*    ... and whether the default dispatch gives a Raytracer-mode batch of small worlds (<= 64 triangles in <= 64
 *    rows) to the BVH path (its flat kernel) rather than to the raster kernels: views of >= 16 tiles, >= 192 tiles per
 *    compute unit in the batch (BASELINE configs[4]); 1 / 0. */
int mrx_dispatch_flat(int raytracer, uint32_t num_views, uint32_t width, uint32_t height, uint32_t max_world_triangles,
                      uint32_t max_world_instances, uint32_t num_cus);
/*    The launch plan of the raster group kernel (host arithmetic, for tests; it touches no device): what the launcher
 *    works out for a batch of `views` views of nslow rows of nfast pixels (64x64 tiles) over worlds of at most
 *    max_world_triangles triangles on num_cus compute units (0 = 256).  uni_instances != 0 describes uniform worlds
 *    (that many instances, at most 4, uni_cams_per_world cameras, the triangle prefix sums and first pool triangles
 *    of the instances); has_blocks: the pose and geometry blocks exist; diagnostics: MRX_DEBUG_SKIP / MRX_DEBUG_STAMPS
 *    is on (any non-zero value; 2 = the stamps alone, bit 1 of any other value adds them to a MRX_DEBUG_SKIP switch);
 *    group_views / group_tiles / debug_slots: MRX_GROUP_VIEWS / MRX_GROUP_TILES / MRX_DEBUG_SLOTS (0 = automatic);
 *    xcd_skew / xcd_rotate: MRX_XCD_SKEW / MRX_XCD_ROTATE (-1 = automatic); fast_allowed: MRX_GROUP_FAST; xcd_phase:
 *    the XCD workgroup 0 last reported; has_report: a report word exists.  Returns the entry (MRX_ENTRY_GROUP_FAST or
 *    MRX_ENTRY_GROUP), 0 for a batch of no pixels (nothing is launched, *out is zeroed), MRX_E_INVALID for a null
 *    pointer, worlds of more than 256 triangles (the group kernel does not render them), more than 4 uniform
 *    instances, a negative group_views / group_tiles / debug_slots, or an xcd_skew / xcd_rotate below -1.  shape,
 *    prefix, first01 and first23 are the packed words of the FAST entry's argument header (0 for MRX_ENTRY_GROUP). */
typedef struct {
    uint32_t views, nfast, nslow, max_world_triangles;
    int32_t textured;
    uint32_t num_cus;
    uint32_t uni_instances, uni_cams_per_world, uni_prefix[5], uni_first_tri[4];
    int32_t has_blocks, diagnostics;
    int32_t group_views, group_tiles, xcd_skew, xcd_rotate, debug_slots;
    int32_t fast_allowed;
    uint32_t xcd_phase;
    int32_t has_report;
} mrx_group_plan_in;
typedef struct {
    int32_t slots;             /* triangle slots per view: 16 ... 256 */
    uint32_t group_views;      /* whole views per workgroup (groups_per_view = 1) */
    uint32_t chunk_tiles;      /* tiles of one view per workgroup (groups_per_view > 1) */
    uint32_t groups_per_view;
    uint32_t workgroups, threads;
    uint32_t xcd_skew, xcd_rotate;
    int32_t xmode;             /* bit 0: the workgroups of a pair trade places, bit 1: workgroup 0 reports its XCD */
    int32_t fast;
    uint32_t shape, prefix, first01, first23;
} mrx_group_plan_t;
int mrx_group_plan(const mrx_group_plan_in *in, mrx_group_plan_t *out);

/* -- per-view projection.  View indices are the whole job's (a renderer of several shards splits the range).
 *    mrx_set_view_projection sets views [first_view, first_view + count) and is stream-ordered: renders enqueued
 *    before it use the old values, the next render the new ones (each shard's table is updated by a copy on its
 *    stream).  Every value is checked before anything changes: MRX_E_INVALID leaves the renderer as it was.
 *    mrx_view_projection reads the current values back, defaults resolved (znear never 0). */
int mrx_set_view_projection(mrx_renderer *r, uint32_t first_view, uint32_t count, const mrx_projection *proj);
int mrx_view_projection(mrx_renderer *r, uint32_t first_view, uint32_t count, mrx_projection *out);
/*    The constants of one projection (host only, no renderer needed) -- DESIGN.md S5: out = sx, ox, sz, oz,
 *    1/znear, S6b pad, for views of width x height pixels (Raytracer mode: width x width) in `render_mode`.
 *    Both launch forms (uniform and per-view) take their constants from here. */
int mrx_projection_constants(uint32_t width, uint32_t height, int render_mode, mrx_projection proj, float out[6]);

/* -- per-world light.  World indices are the whole job's (a renderer of several shards splits the range at
 *    mrx_shard_first_world).  mrx_set_world_light sets worlds [first_world, first_world + count) and is stream-ordered
 *    as mrx_set_view_projection is: renders enqueued before it keep the old light, the next render has the new one.
 *    Every value is checked before anything changes: MRX_E_INVALID leaves the renderer as it was.  The light changes
 *    colour only -- never which kernel runs, visibility, depth or the segmask.  mrx_world_light reads back what was
 *    set (the caller's values, not normalised). */
int mrx_set_world_light(mrx_renderer *r, uint32_t first_world, uint32_t count, const mrx_light *lights);
int mrx_world_light(mrx_renderer *r, uint32_t first_world, uint32_t count, mrx_light *out);
/*    The constants of one light (host only, no renderer needed) -- DESIGN.md S4 / S7: out = the unit vector towards
 *    the light (x, y, z: -direction / |direction|, worked out in double and rounded once), ambient, diffuse.
 *    Both launch forms (uniform and per-view) take their constants from here. */
int mrx_light_constants(mrx_light light, float out[5]);

/* -- per-instance material override (MRX_FLAG_INSTANCE_MATERIALS).  Rows are the rows of MRX_BUF_INSTANCE_MATERIAL
 *    over the whole job: world-major, spare rows included (a renderer of several shards splits the range at its world
 *    boundaries).  mrx_set_instance_materials writes rows [first_row, first_row + count) and is stream-ordered as
 *    mrx_set_view_projection is: renders enqueued before it keep the old ids, the next render has the new ones.  Any
 *    int32 is accepted -- values outside the material table mean "no override", as on the device.  MRX_E_INVALID: a
 *    null pointer or rows outside the renderer; MRX_E_UNSUPPORTED: no column.  mrx_instance_materials reads the
 *    column back (it waits for the stream). */
int mrx_set_instance_materials(mrx_renderer *r, uint32_t first_row, uint32_t count, const int32_t *materials);
int mrx_instance_materials(mrx_renderer *r, uint32_t first_row, uint32_t count, int32_t *out);

/* -- per-instance labels (MRX_FLAG_INSTANCE_LABELS).  Rows are the rows of MRX_BUF_INSTANCE_LABEL over the whole job,
 *    as above.  mrx_set_instance_labels writes rows [first_row, first_row + count) and is stream-ordered as
 *    mrx_set_instance_materials is: renders enqueued before it keep the old labels, the next render has the new ones.
 *    Any int32 is accepted; MRX_LABEL_OBJECT gives a row the id of its bound object back.  MRX_E_INVALID: a null
 *    pointer or rows outside the renderer; MRX_E_UNSUPPORTED: no column.  mrx_instance_labels reads the column back
 *    (it waits for the stream). */
int mrx_set_instance_labels(mrx_renderer *r, uint32_t first_row, uint32_t count, const int32_t *labels);
int mrx_instance_labels(mrx_renderer *r, uint32_t first_row, uint32_t count, int32_t *out);

int mrx_device_count(void);
int mrx_abi_version(void);
const char *mrx_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MRX_H */
