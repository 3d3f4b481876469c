"""Shared by tests/test_view_shapes_cpu.py and tests/test_view_shapes_gpu.py (not collected): the view sizes from 1 to
16384 pixels a side that mrx_create accepts, through every kernel family.

  SHAPES      one explicit table, rows (name, width, height, mode, vfov): views below the units the kernels are built
              from (a lane's four pixels, an 8-row strip, a 32 x 8 region, a 64 x 64 tile), strips that reach x or y
              16383 at 10^5 pixels, and large views of up to 1024 tiles.  Raytracer views are square: the width counts.
              vfov None is the default (90 degrees); a strip's vfov is matched to its shape, so that the view is busy
  scenes      `uniform` (tests.uniform_worlds.uniform_scene: the FAST entry's batches, UNIFORM_WORLDS worlds), `synth`
              and `wall` (scenes.synthetic_scene: 14 and 16 triangles), `cubes20` and `cubes40` (scenes.cube_field: 242
              triangles, the most the group kernel takes at 256 slots, and 482)
  projections None (the defaults), "per-view" (two vfovs a case, the shape's -- 60 degrees where it has none -- and 1.1
              times it: the per-view table is on)
              or "shared" (the shape's vfov on every camera: the uniform argument form)
  reference   `reference(case)`: tests/projection_oracle.render of every view, once per (shape, scene, projections)
  witnesses   `tile_witness` and `batch_witness`: what tests/test_view_shapes_cpu.py asserts of every reference
  CASES       one explicit table; every case names the entry (raster_entry), the BVH kernel (bvh_launch) and the form
              (kernel_form) it must reach

Cameras.  Shapes without a vfov keep the scenes' own rings of cameras.  A strip's views are seen by `horizon_camera`
whatever the scene: the 14 triangles of synthetic_scene cannot put an edge into one tile in twenty of a strip of 256
tiles from their own ring, and a strip 0.1 degrees high that looks down at cube_field sees one line of the ground.  The
eye looks level over the ground quad from low on a ring, the image's long side along the horizon, pitched and rolled so
that the quad's far edge crosses the strip from one corner to the last line of pixels at the other end: the boundary
between sky and ground sits elsewhere in every tile column (tall strips: row), and the cubes stand across it.  A strip
one pixel thin holds one line of pixels, which the horizon cannot cross, and 14 triangles give it a handful of edges:
those two shapes take `cubes20` through the group kernel (kernel variant 3: 256 slots).  The seed of a (shape, scene)
and the azimuth of a strip's first camera are the first that meet the witnesses (SEEDS, AZIMUTHS;
tests/test_view_shapes_cpu.py's docstring has the measured shares and what was tried before)."""
import dataclasses
import functools
import math
from collections import namedtuple

import numpy as np

from madrona_renderer_amd import scenes
from tests import projection_oracle as po
from tests import uniform_worlds as uw

# ---- shapes -----------------------------------------------------------------------------------------------------------
Shape = namedtuple("Shape", "name width height mode vfov")
RAST, RT = "Rasterizer", "Raytracer"
BELOW_A_UNIT = tuple(Shape("%dx%d" % (w, h), w, h, RAST, None) for w, h in (
    (1, 1), (2, 1), (1, 2), (3, 2), (4, 1), (1, 9), (7, 5), (31, 8), (33, 7), (5, 65), (65, 3), (63, 63), (65, 65))) + \
    tuple(Shape("rt%d" % w, w, w, RT, None) for w in (1, 2, 5, 65))
STRIPS = (Shape("16384x1", 16384, 1, RAST, 0.0125), Shape("1x16384", 1, 16384, RAST, 120.0),
          Shape("16384x8", 16384, 8, RAST, 0.1), Shape("8x16384", 8, 16384, RAST, 120.0),
          Shape("16383x3", 16383, 3, RAST, 0.04), Shape("2x8191", 2, 8191, RAST, 120.0),
          Shape("4097x5", 4097, 5, RAST, 0.25), Shape("16384x64", 16384, 64, RAST, 0.8),
          # (256 tile columns and a second tile row: the tile index goes past the columns of a row)
          Shape("16384x65", 16384, 65, RAST, 0.8))
LARGE = (Shape("640x480", 640, 480, RAST, None), Shape("1024x768", 1024, 768, RAST, None),
         Shape("2048x2048", 2048, 2048, RAST, None), Shape("rt640", 640, 640, RT, None),
         Shape("rt1024", 1024, 1024, RT, None))
SHAPES = BELOW_A_UNIT + STRIPS + LARGE
SHAPE = {s.name: s for s in SHAPES}
assert len(SHAPE) == len(SHAPES)


def storage(shape):
    """(nslow, nfast) of a view's tensors: (height, width), or (width, width) in Raytracer mode"""
    return (shape.width, shape.width) if shape.mode == RT else (shape.height, shape.width)


def tiles(shape):
    """(tile rows, tile columns) of 64 x 64 pixels in storage order"""
    nslow, nfast = storage(shape)
    return (nslow + 63) // 64, (nfast + 63) // 64


def one_tile(shape):
    return tiles(shape) == (1, 1)


def num_views(shape, scene):
    """a batch of uniform worlds for the one-tile shapes; else 2 to 8 views, about 400,000 pixels a case"""
    nslow, nfast = storage(shape)
    return UNIFORM_WORLDS if scene == "uniform" else max(2, min(8, 400000 // (nslow * nfast)))


# ---- scenes -----------------------------------------------------------------------------------------------------------
UNIFORM_WORLDS = 130
# (shape name, scene) -> the seed of uniform_scene and cube_field, first_world + 1 of synthetic_scene.  A pair that is not
# listed takes 1 (uniform worlds: 10).
SEEDS = {("5x65", "synth"): 59, ("5x65", "wall"): 44}
# (shape name, scene) -> the azimuth in degrees of a strip's first camera on its ring.  A pair that is not listed takes 20.
# ("2x8191", "synth") is not the witnesses' choice: azimuth 20 meets them, and was moved on because of the first-principles
# test (tests/test_view_shapes_cpu.py) -- there one pixel of view 0 lies 0.9 m inside the far edge of the 20 km ground quad
# at depth 8862, and the oracle's float32 edge functions and the float64 ray caster name different triangles at a margin
# of 4.4e-5, above that test's 1e-6.  The input was changed, not the bound.
AZIMUTHS = {("16384x1", "cubes20"): 24.0, ("1x16384", "cubes20"): 30.0, ("2x8191", "synth"): 21.0}
RING_RADIUS, RING_HEIGHT, RING_STEP = 12.0, 0.6, 47.0


def horizon_camera(shape, az):
    """(eye, rotation) of a strip's camera: the eye RING_HEIGHT up on a ring of RING_RADIUS around the world's axis, at
    azimuth `az` (degrees), heading for the axis; the image's long side lies along the horizon, and pitch and roll are
    those that put the horizon through two points of the image: the outer corner of the long side's first pixel, on the
    side of the ground, and, at the long side's last pixel, the boundary between the outermost line of pixels on the
    side of the sky and the next.  So the sky's share falls from all to one line along the strip, the boundary crosses
    every line of pixels but that one, and the last tile column (wide strips) or row (tall ones) holds sky and ground.
    Wide strips have the sky above; tall ones, rolled a quarter turn, on the right, and end at the bottom."""
    W, H = shape.width, shape.height
    px = 2.0 * math.tan(math.radians(shape.vfov / 2)) / H              # one pixel, as the tangent of its angle
    if W > H:
        first, last, sky = (-W / 2, -H / 2), (W / 2, H / 2 - 1), (0.0, 4.0 * H)
    else:
        first, last, sky = (-W / 2, H / 2), (W / 2 - 1, -H / 2), (4.0 * W, 0.0)
    ray = lambda p: np.array([p[0] * px, 1.0, p[1] * px])
    zc = np.cross(ray(first), ray(last))                                # the world's up in camera space, but for its sign
    zc /= np.linalg.norm(zc)
    if zc @ ray(sky) < 0:
        zc = -zc
    a = math.radians(az)
    c = math.sqrt(1.0 - zc[1] ** 2)
    fwd = np.array([-c * math.cos(a), -c * math.sin(a), zc[1]])
    east = np.cross(fwd, [0.0, 0.0, 1.0])
    east /= np.linalg.norm(east)
    north = np.cross(east, fwd)
    right = (zc[2] * east + zc[0] * north) / north[2]                   # right . up(world) = zc[0], up . up(world) = zc[2]
    up = np.cross(right, fwd)
    assert abs(right @ right - 1.0) < 1e-12 and abs(up[2] - zc[2]) < 1e-12 and abs(right[2] - zc[0]) < 1e-12
    eye = tuple(float(np.float32(x)) for x in (RING_RADIUS * math.cos(a), RING_RADIUS * math.sin(a), RING_HEIGHT))
    return eye, scenes._quat_from_basis(right, fwd, up)


def strip_cameras(shape, scene, n):
    az = AZIMUTHS.get((shape.name, scene), 20.0)
    return [horizon_camera(shape, az + RING_STEP * v) for v in range(n)]


@functools.lru_cache(maxsize=4)
def base_scene(shape, scene, textured):
    n = num_views(shape, scene)
    seed = SEEDS.get((shape.name, scene), 10 if scene == "uniform" else 1)
    if scene == "uniform":
        return uw.uniform_scene(seed, n, shape.width, shape.height, shape.mode, textured=textured)
    if scene in ("synth", "wall"):
        d = scenes.synthetic_scene(n, width=shape.width, height=shape.height, with_wall=scene == "wall",
                                   textured=textured, render_mode=shape.mode, first_world=seed - 1)
    else:
        d = scenes.cube_field(n, {"cubes20": 20, "cubes40": 40}[scene], width=shape.width, height=shape.height,
                              mode=shape.mode, textured=textured, seed=seed)
    if shape.vfov is not None:
        d.cameras = strip_cameras(shape, scene, n)
    return d


SHARED_VFOV = 60.0          # of a shape without a vfov of its own (per-view: 60 and 66 degrees)


def projections(shape, n, proj):
    if proj is None:
        return None
    if proj == "shared":
        return [(shape.vfov or SHARED_VFOV, None)] * n
    assert proj == "per-view", (shape, proj)
    return [((shape.vfov or SHARED_VFOV) * (1.0, 1.1)[c % 2], None) for c in range(n)]


@functools.lru_cache(maxsize=4)
def scene_desc(shape, scene, textured, proj):
    base = base_scene(shape, scene, textured)
    d = dataclasses.replace(base)
    p = projections(shape, len(base.cameras), proj)
    d.camera_projections = None if p is None else list(p)
    return d


@functools.lru_cache(maxsize=2)
def cached_reference(shape, scene, textured, proj):
    """the oracle's images of every view under the desc's own projections: rgb, depth, tri_id, segmask.  The two last
    references stay cached (up to 100 MB each); CASES keeps the cases of one reference together."""
    desc = scene_desc(shape, scene, textured, proj)
    ref = po.render(desc, None, 0, desc.num_views, want_ids=True)
    out = {k: ref[k] for k in ("rgb", "depth", "tri_id", "segmask")}
    for v in out.values():
        v.setflags(write=False)
    return out


# ---- witnesses (CPU, the oracle alone) --------------------------------------------------------------------------------
def _distinct(block):
    return len(np.unique(block))


def tile_witness(tri_id):
    """of tri_id [views, slow, fast]: (share of the 64 x 64 tiles of all views that hold at least two distinct ids --
    the background's -1 is one --, views whose last tile column holds two, views whose last tile row does, hit share)"""
    views, nslow, nfast = tri_id.shape
    rows, cols = (nslow + 63) // 64, (nfast + 63) // 64
    edges = last_col = last_row = 0
    for v in range(views):
        col = row = False
        for ty in range(rows):
            for tx in range(cols):
                two = _distinct(tri_id[v, ty * 64:ty * 64 + 64, tx * 64:tx * 64 + 64]) >= 2
                edges += two
                col |= two and tx == cols - 1
                row |= two and ty == rows - 1
        last_col += col
        last_row += row
    return edges / float(views * rows * cols), last_col, last_row, float((tri_id >= 0).mean())


def batch_witness(tri_id):
    """of the one-tile views of a batch: (hit pixels, background pixels, distinct triangles that win a pixel)"""
    hit = tri_id >= 0
    return int(hit.sum()), int((~hit).sum()), len(np.unique(tri_id[hit]))


# ---- the case table ---------------------------------------------------------------------------------------------------
# family: group-fast, group, brute, chunked, bvh-tile, bvh-flat.  variant: MADRONA_MI355_KERNEL, None = the default
# dispatch.  env: the launch knobs (monkeypatch.setenv).  form: what kernel_form names -- Uniform under the defaults and
# under a shared vfov (the argument form), PV under two vfovs.  launch: what bvh_launch must hold besides the kernel.
Case = namedtuple("Case", "name family shape scene textured proj variant env form launch")
ENTRY = {"group-fast": ("group-fast", "none"), "group": ("group", "none"), "brute": ("brute", "none"),
         "chunked": ("chunked", "none"), "bvh-tile": ("bvh", "tile"), "bvh-flat": ("bvh", "flat")}
SIX = ("7x5", "65x65", "16384x8", "8x16384", "16383x3", "640x480")
THIN = ("16384x1", "1x16384")
BVH_TILE = {0: (64, 64), 1: (64, 32), 2: (32, 32)}


def _proj(shape, shared=False, per_view=False):
    return "shared" if shared else None if shape.vfov is None and not per_view else "per-view"


def _cases():
    out = []

    def add(family, shape, scene, textured=False, variant=None, env=None, shared=False, launch=None, tag="",
            per_view=False):
        proj = _proj(shape, shared, per_view)
        name = "-".join(x for x in (family, shape.name, scene, "tex" if textured else "", "shared" if shared else "",
                                    "pv" if per_view else "", tag) if x)
        out.append(Case(name, family, shape, scene, textured, proj, variant, dict(env or {}),
                        "PV" if proj == "per-view" else "Uniform", dict(launch or {})))

    # group kernel: the FAST entry and the plain entry on the one-tile shapes (uniform worlds, textured every other one);
    # the plain entry on every multi-tile shape, untextured and textured
    for i, shape in enumerate(SHAPES):
        if one_tile(shape):
            add("group-fast", shape, "uniform", textured=i % 2 == 1)
            add("group", shape, "uniform", textured=i % 2 == 1, env={"MRX_GROUP_FAST": "0"}, tag="plain")
        else:
            for textured in (False, True):
                if shape.name in THIN:
                    add("group", shape, "cubes20", textured, variant=3)
                else:
                    add("group", shape, "wall" if textured else "synth", textured)
    add("group", SHAPE["16384x8"], "synth", env={"MRX_GROUP_TILES": "1"}, tag="tiles1")
    add("group", SHAPE["16384x64"], "wall", True, env={"MRX_GROUP_TILES": "16"}, tag="tiles16")
    add("group", SHAPE["16384x8"], "synth", shared=True)
    add("group-fast", SHAPE["31x8"], "uniform", shared=True)
    # the FAST entry's per-view table below a lane's four pixels, below a strip's eight rows, past a 32-pixel region and in
    # Raytracer order: two vfovs on the two cameras of every uniform world
    for name, textured in (("3x2", False), ("7x5", True), ("33x7", False), ("rt5", False)):
        add("group-fast", SHAPE[name], "uniform", textured, per_view=True)
    # brute and chunked
    for name in SIX:
        add("brute", SHAPE[name], "wall", variant=1)
        add("chunked", SHAPE[name], "cubes40", variant=3)
    add("brute", SHAPE["16384x65"], "wall", variant=1)
    add("chunked", SHAPE["16384x65"], "cubes40", variant=3)
    add("brute", SHAPE["16383x3"], "wall", variant=1, shared=True)
    add("chunked", SHAPE["16383x3"], "cubes40", variant=3, shared=True)
    # BVH tile kernel, default dispatch: every tile shape; at 16384 x 8 runs of one tile, the default (one tile too for so few
    # views: scene.cpp) and sixteen
    for name in SIX:
        for t in (0, 1, 2):
            add("bvh-tile", SHAPE[name], "cubes40", textured=t == 1, env={"MRX_BVH_TILE": str(t)},
                launch={"tile": BVH_TILE[t]}, tag="t%d" % t)
    add("bvh-tile", SHAPE["16384x8"], "cubes40", env={"MRX_BVH_GROUP_TILES": "1"}, launch={"group_tiles": 1}, tag="run1")
    add("bvh-tile", SHAPE["16384x8"], "cubes40", tag="run")
    add("bvh-tile", SHAPE["16384x8"], "cubes40", env={"MRX_BVH_GROUP_TILES": "16"}, launch={"group_tiles": 16}, tag="run16")
    add("bvh-tile", SHAPE["16384x8"], "cubes40", shared=True)
    # (the tile index past the 256 -- at 32 x 32, 512 -- tile columns of a row, as the brute and the chunked kernel above)
    for t in (0, 1, 2):
        add("bvh-tile", SHAPE["16384x65"], "cubes40", env={"MRX_BVH_TILE": str(t)}, launch={"tile": BVH_TILE[t]},
            tag="t%d" % t)
    # BVH flat kernel (variant 2 on worlds of at most 64 triangles)
    for name in ("rt5", "rt65", "rt1024", "16384x8", "65x65"):
        add("bvh-flat", SHAPE[name], "wall", textured=name in ("rt65", "16384x8"), variant=2)
    add("bvh-flat", SHAPE["16384x8"], "wall", variant=2, shared=True)
    add("bvh-flat", SHAPE["16384x65"], "wall", variant=2)
    names = [c.name for c in out]
    assert len(names) == len(set(names)), sorted(n for n in names if names.count(n) > 1)
    # the cases of one reference together, references in the order of their first case (cached_reference holds two)
    first = {}
    for c in out:
        first.setdefault((c.shape, c.scene, c.textured, c.proj), len(first))
    return sorted(out, key=lambda c: first[(c.shape, c.scene, c.textured, c.proj)])


CASES = _cases()


def desc_of(case):
    return scene_desc(case.shape, case.scene, case.textured, case.proj)


def reference(case):
    return cached_reference(case.shape, case.scene, case.textured, case.proj)


def reference_keys():
    """the distinct (shape, scene, textured, proj) of the case table, with the families that render each"""
    seen = {}
    for c in CASES:
        seen.setdefault((c.shape, c.scene, c.textured, c.proj), []).append(c.family)
    return seen
