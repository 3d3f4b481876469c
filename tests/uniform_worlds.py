"""Deterministic uniform worlds for the FAST raster group kernel (raster.hip, rasterGroupKernelFast).

The host gives a batch to that kernel only when its worlds are uniform and its views fit one tile
(scene.cpp bindGeometry, raster.hip launchRaster): every world binds the same 1..4 drawn objects in the
same order and has the same number of cameras (below 256), a world draws at most 16 triangles, a view is at
most 64x64 and every used object's first triangle is below 65536.  The scenes here keep to all of that and
put the hard cases inside it: cube.obj next to raw meshes holding exact duplicate triangles (ties), a
collinear triangle, a triangle with a repeated vertex, a sliver, a triangle tens of units across, a
sub-pixel one and a material that does not exist; per-world poses with random and non-unit quaternions,
per-axis scales of random sign and nearly flat instances; cameras 10^U(-2.5, 1.5) units from an instance
(closed meshes straddle the near plane, the eye is often inside a cube), some looking anywhere, and in
Raytracer scenes some geometry across the far plane.  `CASES` names the scenes the tests share;
`edge_counts` counts, from the oracle's output and camera-space vertices, how often a batch reaches the
cases the FAST kernel's per-strip near-free bit and tie rule decide."""
import os

import numpy as np

from madrona_renderer_amd import scenes

CUBE = os.path.join(scenes.DATA_DIR, "cube.obj")
CUBE_TRIS = 12
RASTER_NEAR, RT_NEAR = 0.001, 0.1
MISSING_MATERIAL = 99
MISSING_TEXTURE = 7


def _raw_meshes():
    """name -> (verts [N,3], uvs [N,2], indices [3T], material).  Vertex positions are exact in float32."""
    tie = (np.array([[-0.6, 0.0, -0.5], [0.7, 0.1, -0.4], [0.0, -0.2, 0.75],      # T
                     [-0.5, 0.3, -0.3], [0.0, 0.3, 0.0], [0.5, 0.3, 0.3],          # collinear
                     [-0.7, -0.1, 0.6], [0.7, -0.1, 0.6], [0.7, -0.1, 0.6078125]], np.float32),  # sliver
           np.array([[0.0, 0.0], [1.0, 0.0], [0.5, 1.0], [0.0, 0.0], [0.5, 0.5], [1.0, 1.0],
                     [0.0, 0.0], [1.0, 0.0], [1.0, 1.0]], np.float32),
           # T, its exact duplicate (a tie: the lower index wins), the collinear one, the sliver
           np.array([0, 1, 2, 0, 1, 2, 3, 4, 5, 6, 7, 8], np.uint32), 1)
    junk = (np.array([[0.0, 0.0, 0.0], [0.4, 0.1, 0.3],                           # repeated vertex
                      [-15.0, 12.0, -3.0], [18.0, 10.0, -2.0], [1.0, -14.0, 4.0],  # tens of units across
                      [0.2, 0.2, 0.2], [0.2009765625, 0.2, 0.2], [0.2, 0.2009765625, 0.2001953125]], np.float32),
            np.zeros((8, 2), np.float32),
            np.array([0, 0, 1, 2, 3, 4, 5, 6, 7], np.uint32), MISSING_MATERIAL)
    # uv well outside [0, 1): repeat addressing; textured in the textured variant
    quad = (np.array([[-0.8, 0.0, -0.8], [0.8, 0.0, -0.8], [-0.8, 0.0, 0.8], [0.8, 0.0, 0.8]], np.float32),
            np.array([[-1.25, -0.5], [2.75, -0.5], [-1.25, 3.5], [2.75, 3.5]], np.float32),
            np.array([0, 1, 2, 2, 1, 3], np.uint32), 2)
    # its material names a texture that does not exist: drawn untextured
    one = (np.array([[-0.9, -0.4, -0.3], [0.8, 0.5, -0.2], [0.1, 0.0, 0.9]], np.float32),
           np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]], np.float32),
           np.array([0, 1, 2], np.uint32), 3)
    return {"tie": tie, "junk": junk, "quad": quad, "one": one}


RAW_NAMES = ("tie", "junk", "quad", "one")
RAW_TRIS = {"cube": CUBE_TRIS, "tie": 4, "junk": 3, "quad": 2, "one": 1}

# the objects of every world, in order (world triangles in brackets)
LAYOUTS = (
    ("cube", "tie"),                   # 16
    ("cube",),                         # 12
    ("tie", "cube"),                   # 16: the cube at slot 4
    ("quad", "cube", "one", "one"),    # 16, four objects, one of them twice
    ("junk", "tie", "quad", "one"),    # 10, no cube
    ("junk", "cube", "one"),           # 16, three objects
    ("one",),                          # 1
    ("tie", "junk", "quad"),           # 9
)


def _f32(x):
    return tuple(float(np.float32(v)) for v in x)


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _quat(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def _look(eye, target):
    fwd = np.asarray(target, np.float64) - np.asarray(eye, np.float64)
    n = np.linalg.norm(fwd)
    if n == 0 or abs(fwd[2]) > 0.999 * n:         # look_at has no roll for a vertical view direction
        target = np.asarray(target, np.float64) + 1e-2 * max(n, 1e-3) * np.array([1.0, 0.5, 0.0])
    return scenes.look_at(eye, target)


def uniform_scene(seed, num_worlds, width=64, height=64, mode="Rasterizer", layout=None, cams=None,
                  textured=False, first_raw_tri=None):
    """A batch of `num_worlds` uniform worlds: each binds the objects of `layout` (names of LAYOUTS' entries;
    default LAYOUTS[seed % 8]) in that order and sees `cams` cameras (default 1 + seed % 3).
    `first_raw_tri`: an unused raw mesh in front of the others puts the first raw object at that triangle
    index (header limits).  Raytracer views are square, `width` pixels on a side."""
    layout = tuple(LAYOUTS[seed % len(LAYOUTS)] if layout is None else layout)
    cams = 1 + seed % 3 if cams is None else int(cams)
    rt = mode == "Raytracer"
    if rt:
        height = width
    raw = _raw_meshes()
    meshes = []
    if first_raw_tri is not None:
        pad = int(first_raw_tri) - CUBE_TRIS
        assert pad >= 1
        meshes.append((np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.zeros((3, 2), np.float32),
                       np.tile(np.array([0, 1, 2], np.uint32), pad), 0))
    obj_id = {"cube": 0}
    for name in RAW_NAMES:
        obj_id[name] = 1 + len(meshes)
        meshes.append(raw[name])
    verts, uvs, idx, voff, ioff, mats = [], [], [], [], [], []
    nv = ni = 0
    for v, t, i, m in meshes:
        voff.append(nv)
        ioff.append(ni)
        verts.append(v)
        uvs.append(t)
        idx.append(i)
        mats.append(m)
        nv += len(v)
        ni += len(i)
    materials = [((0.7, 0.6, 0.5, 1.0), 0 if textured else -1, 0.8, 0.2),
                 ((0.2, 0.8, 0.4, 1.0), -1, 0.5, 0.5),
                 ((1.0, 0.9, 0.8, 1.0), 0 if textured else -1, 0.5, 0.5),
                 ((0.9, 0.3, 0.3, 1.0), MISSING_TEXTURE, 0.5, 0.5)]
    instances, cameras, worlds = [], [], []
    for w in range(num_worlds):
        rng = np.random.default_rng([seed, w])
        i0 = len(instances)
        for name in layout:
            pos = rng.normal(size=3) * 2.0
            q = _quat(rng)
            if rng.random() < 0.2:
                q = q * rng.uniform(0.6, 1.5)           # not a rotation
            s = rng.uniform(0.4, 2.5, size=3) * np.where(rng.random(3) < 0.35, -1.0, 1.0)
            if rng.random() < 0.15:
                s[rng.integers(0, 3)] = float(rng.choice([-1.0, 1.0])) * 10.0 ** rng.uniform(-4, -2)   # nearly flat
            instances.append((_f32(pos), _f32(q), _f32(s), obj_id[name]))
        far_world = rt and rng.random() < 0.25
        if far_world:
            # instance 0 grows to ~60 units and camera 0 sees it from ~1000: it straddles the far plane
            p, q, s, o = instances[i0]
            instances[i0] = (p, q, _f32(np.asarray(s) * 40.0), o)
        c0 = len(cameras)
        for c in range(cams):
            k = i0 + int(rng.integers(0, len(layout)))
            target = np.asarray(instances[k][0], np.float64)
            if far_world and c == 0:
                target = np.asarray(instances[i0][0], np.float64)
                eye = target + rng.uniform(975.0, 1030.0) * _unit(rng)
                cameras.append((_f32(eye), _look(eye, target)))
            elif rng.random() < 0.8:
                d = 10.0 ** rng.uniform(-2.5, 1.5)
                eye = target + d * _unit(rng)
                aim = target + rng.normal(size=3) * 0.3 * min(d, 1.0)
                cameras.append((_f32(eye), _look(eye, aim)))
            else:
                eye = target + rng.normal(size=3) * 2.0
                cameras.append((_f32(eye), _f32(_quat(rng))))
        worlds.append((len(layout), i0, cams, c0))
    return scenes.SceneDesc(
        num_worlds=num_worlds, render_mode=mode, width=width, height=height,
        asset_paths=[(CUBE, 0)],
        mesh_vertices=np.concatenate(verts).astype(np.float32), mesh_uvs=np.concatenate(uvs).astype(np.float32),
        mesh_indices=np.concatenate(idx).astype(np.uint32), mesh_vertex_offsets=np.asarray(voff, np.uint32),
        mesh_indices_offsets=np.asarray(ioff, np.uint32), mesh_materials=np.asarray(mats, np.int32),
        materials=materials, texture_paths=[os.path.join(scenes.DATA_DIR, "cube.png")],
        instances=instances, cameras=cameras, worlds=worlds)


RASTER_SIZES = ((64, 64), (64, 32), (32, 64), (50, 30), (63, 64), (64, 57), (33, 9), (4, 64), (64, 1), (1, 1))
RT_SIZES = (64, 33, 17, 1)
BATCHES = (1, 3, 7, 130, 1024)


def _cases():
    out = {}
    seed = 11
    # every raster view size, batches of every size, every layout, one to three cameras
    for n, ((w, h), nw) in enumerate(zip(RASTER_SIZES, (1024, 130, 7, 130, 3, 7, 130, 7, 3, 1))):
        out[f"raster-{w}x{h}-w{nw}"] = dict(seed=seed + n, num_worlds=nw, width=w, height=h)
    for res, nw, s in zip(RT_SIZES, (130, 7, 3, 1), (31, 32, 37, 34)):
        out[f"rt-{res}-w{nw}"] = dict(seed=s, num_worlds=nw, width=res, mode="Raytracer")
    out["rt-64-w1024"] = dict(seed=seed + 30, num_worlds=1024, width=64, mode="Raytracer", cams=1)
    out["tex-raster-64x64-w130"] = dict(seed=seed + 37, num_worlds=130, textured=True)
    out["tex-raster-50x30-w7"] = dict(seed=seed + 40, num_worlds=7, width=50, height=30, textured=True)
    out["tex-rt-64-w7"] = dict(seed=seed + 41, num_worlds=7, width=64, mode="Raytracer", textured=True)
    return out


CASES = _cases()


def case(name):
    return uniform_scene(**CASES[name])


# --------------------------------------------------------------------------------------------------
def _quat_mat(q):
    w, x, y, z = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def world_triangles(fs, w):
    """[(instance row, triangle)] of world w in visibility-id order (the oracle's world-local numbering)."""
    out = []
    for i in range(fs.world_inst_start[w], fs.world_inst_start[w + 1]):
        o = int(fs.inst_obj0[i])
        if 0 <= o < len(fs.obj_first_tri):
            f = int(fs.obj_first_tri[o])
            out += [(i, t) for t in range(f, f + int(fs.obj_num_tris[o]))]
    return out


def edge_counts(fs, ref, cube_object=0):
    """How often a batch reaches the cases the FAST kernel decides per strip or per pixel (float64, from the
    oracle's visibility ids and camera-space vertices; storage layout, so Raytracer strips are 8 storage rows):
      near_pixels  covered pixels whose winning triangle crosses the near plane
      mixed_tiles  views holding a strip with such a pixel and a covered strip without one
      inside_views views whose eye is inside a cube instance
      tie_pixels   covered pixels won by a triangle that has an exact duplicate of higher index
      mirror_pixels covered pixels won by a mirrored instance (negative determinant)"""
    near = RT_NEAR if fs.raytracer else RASTER_NEAR
    tri_id = ref["tri_id"]
    counts = dict(near_pixels=0, mixed_tiles=0, inside_views=0, tie_pixels=0, mirror_pixels=0)
    cache = {}
    for v in range(fs.num_views):
        w = int(fs.view_world[v])
        if w not in cache:
            tris = world_triangles(fs, w)
            world_pts, dup, mirror = [], [], []
            for k, (i, t) in enumerate(tris):
                M = _quat_mat(fs.inst_rot[i]) * fs.inst_scale[i].astype(np.float64)[None, :]
                world_pts.append(fs.tri_pos[t].astype(np.float64) @ M.T + fs.inst_pos[i].astype(np.float64))
                dup.append(any(i2 == i and np.array_equal(fs.tri_pos[t2], fs.tri_pos[t])
                               for i2, t2 in tris[k + 1:]))
                mirror.append(np.linalg.det(M) < 0)
            cubes = [(_quat_mat(fs.inst_rot[i]) * fs.inst_scale[i].astype(np.float64)[None, :],
                      fs.inst_pos[i].astype(np.float64))
                     for i in range(fs.world_inst_start[w], fs.world_inst_start[w + 1])
                     if int(fs.inst_obj0[i]) == cube_object]
            cache[w] = (np.asarray(world_pts).reshape(-1, 3, 3), np.asarray(dup, bool), np.asarray(mirror, bool),
                        cubes)
        pts, dup, mirror, cubes = cache[w]
        ids = tri_id[v]
        cov = ids >= 0
        if not cov.any():
            continue
        Rc = _quat_mat(fs.cam_rot[v])
        eye = fs.cam_pos[v].astype(np.float64)
        y = (pts - eye) @ Rc[:, 1]                        # camera-space forward coordinate of every vertex
        cross = (y.min(axis=1) < near) & (y.max(axis=1) > near)
        win = np.where(cov, ids, 0)
        near_px = cov & cross[win]
        counts["near_pixels"] += int(near_px.sum())
        counts["tie_pixels"] += int((cov & dup[win]).sum())
        counts["mirror_pixels"] += int((cov & mirror[win]).sum())
        rows = ids.shape[0]
        strip_near = [near_px[s:s + 8].any() for s in range(0, rows, 8)]
        strip_free = [cov[s:s + 8].any() and not near_px[s:s + 8].any() for s in range(0, rows, 8)]
        counts["mixed_tiles"] += int(any(strip_near) and any(strip_free))
        for M, t in cubes:
            try:
                local = np.linalg.solve(M, eye - t)
            except np.linalg.LinAlgError:
                continue
            if (np.abs(local) < 0.5).all():
                counts["inside_views"] += 1
                break
    return counts
