"""Witnesses for the BVH tile kernel's round-overflow paths, computed from the CPU oracle alone.

bvhTileKernel (madrona_renderer_amd/csrc/bvh.hip) renders a tile in rounds.  A round hands out records from a
per-tile table; when the table is full the round ends, resolveStrip<FINAL=false> writes the round's winners to
the output tensors and marks their depth-buffer words kStashed, and the table starts over.  The tile's last round,
resolveStrip<FINAL=true>, loads the stashed pixels back.  Large triangles go on a per-tile list of bigCap entries;
a full list ends the round too (the batch is taken again; the table is not reset).

Nothing here knows the kernel's traversal order, so the witnesses are lower bounds that hold for any order:
  - every final winner of a pixel held a record in the round whose resolve output it, and a resolve outputs at most
    `usable` distinct records, so a tile needs at least ceil(distinct winners / usable) table rounds;
  - with MRX_BVH_SMALL_AREA=0 every live triangle is large (bvh.hip: `small = live && area <= smallArea`, and a live
    triangle's box has area >= 1), every winner was rasterised by a large pass, and a large pass takes at most bigCap
    entries, so a tile needs at least ceil(distinct winners / bigCap) large passes.

The scenes the GPU tests render (tests/test_bvh_rounds_gpu.py) are built here too, so that the CPU tests can check
that each still reaches the witness it claims (tests/test_bvh_rounds_cpu.py)."""
import math
import os
from dataclasses import dataclass

import numpy as np

from madrona_renderer_amd import scenes
from tests import meshes

# ---- restated from bvh.hip (kSlotBits, kStashed, tabCap, tabUsable, bigCap, MRX_TEX_BIGCAP); the GPU tests check
#      these against what mrx_bvh_launch reports
SLOT_BITS = 10
STASHED = (1 << SLOT_BITS) - 1          # slot 1023: "resolved in an earlier round of the tile"
TEX_BIGCAP = 64
TILE_SHAPES = {0: (64, 64), 1: (64, 32), 2: (32, 32)}       # MRX_BVH_TILE -> (TW over nfast, TH over nslow)


def tab_cap(tw, th, cls):
    """Records of an untextured round (bvh.hip tabCap)."""
    return (1024 if cls else 768) if tw * th >= 4096 else 512


def tab_usable(cap):
    """Records a round may hand out before it ends: slot STASHED is the marker (bvh.hip tabUsable; the textured
    instantiations take min(bvhTexCap, kStashed))."""
    return min(cap, STASHED)


def big_cap(tw, th, cls, textured=False):
    """Entries of the large-triangle list per round (bvh.hip bigCap)."""
    return 96 if tw * th >= 4096 and cls else (TEX_BIGCAP if textured else 64)


def shape(bvh_tile=0, classify=False, textured=False, tex_cap=None):
    """(tw, th, usable records, bigCap) of a tile-kernel launch; CLS applies to 64x64 tiles only."""
    tw, th = TILE_SHAPES[bvh_tile]
    cls = bool(classify) and bvh_tile == 0
    cap = tex_cap if textured else tab_cap(tw, th, cls)
    return tw, th, tab_usable(cap), big_cap(tw, th, cls, textured)


@dataclass
class TileWitness:
    view: int
    x0: int                 # first pixel over the storage fast axis
    y0: int                 # ... over the slow axis
    partial: bool           # the kernel's per-pixel stash / reload branches (resolveStrip `full` is false)
    winners: int            # distinct final winners (world-local triangle ids) among the tile's pixels
    rounds: int             # lower bound on the tile's record-table rounds
    passes: int             # lower bound on its large passes under MRX_BVH_SMALL_AREA=0


def witness(tri_id, tw, th, usable, bigcap):
    """Per (view, tile) witnesses from the oracle's visibility ids, storage layout [view, nslow, nfast] (Raytracer
    views are stored transposed: their tiles run over image y first).  Tiles are laid out as bvhTileKernel lays
    them out: TW pixels over nfast, TH over nslow, edge tiles cut short."""
    tri_id = np.asarray(tri_id)
    nv, nslow, nfast = tri_id.shape
    out = []
    for v in range(nv):
        for y0 in range(0, nslow, th):
            for x0 in range(0, nfast, tw):
                ids = tri_id[v, y0:y0 + th, x0:x0 + tw]
                w = len(np.unique(ids[ids >= 0]))
                full = nfast % 4 == 0 and x0 + tw <= nfast and y0 + th <= nslow
                out.append(TileWitness(v, x0, y0, not full, w, max(1, math.ceil(w / usable)),
                                       max(1, math.ceil(w / bigcap))))
    return out


def max_rounds(wit, view=None):
    return max(t.rounds for t in wit if view is None or t.view == view)


# ---------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------
DOWN = (0.7071068, -0.7071068, 0.0, 0.0)          # camera looking straight down (-z)
TEX_PATH = os.path.join(scenes.DATA_DIR, "cube.png")


def _mats(textured):
    return [((0.4, 0.7, 0.3, 1.0), 0 if textured else -1, 0.5, 0.5),
            ((0.9, 0.5, 0.3, 1.0), 0 if textured else -1, 0.5, 0.5)]


def dense_scene(mode="Rasterizer", width=64, height=64, textured=False, cameras=("far", "near")):
    """One world: a sphere of 2304 triangles (object 0) and terrain(70) (9800 triangles, object 1: the segmask label
    of most pixels is 1, not the 0 a tensor that was never written holds).  Cameras:
    "far"    12 units above the terrain looking straight down: ~3900 distinct winners in a 64x64 view, so every
             table overflows;
    "near"   at height 1.6, just above the terrain, looking down: few triangles, one round;
    "inside" inside the sphere looking along it: every winner is large on screen (the large list);
    "ground" just above the terrain looking along it (the large list)."""
    ter, sph = meshes.terrain(70), meshes.sphere(48, 24)
    geo = meshes.pack_meshes([(sph[0], sph[1], sph[2], 1), (ter[0], ter[1], ter[2], 0)])
    inst = [((0.0, 0.0, -1.0), meshes.IDENT, (1.0, 1.0, 1.0), 1),
            ((4.0, -3.0, 2.5), (0.9238795, 0.0, 0.3826834, 0.0), (2.0, 2.0, 2.0), 0)]
    cams_all = {
        "far": ((0.0, 0.0, 12.0), DOWN),
        "near": ((-6.0, 5.0, 1.6), DOWN),
        "inside": ((4.3, -3.2, 2.6), scenes.look_at((4.3, -3.2, 2.6), (5.5, -1.0, 2.8))),
        "ground": ((-9.0, -9.0, 1.2), scenes.look_at((-9.0, -9.0, 1.2), (6.0, 4.0, 0.0))),
    }
    cams = [cams_all[c] for c in cameras]
    return scenes.SceneDesc(
        num_worlds=1, render_mode=mode, width=width, height=height, materials=_mats(textured),
        texture_paths=[TEX_PATH] if textured else [], instances=inst, cameras=cams,
        worlds=[(len(inst), 0, len(cams), 0)], **geo)


def tie_scene(mode="Rasterizer", width=64, height=64):
    """Two instances of the same textured terrain(40) at the same pose: every covered pixel is an exact tie in
    1/depth between triangle k and k + 3200, which the lower index must win whichever round each landed in."""
    ter = meshes.terrain(40)
    geo = meshes.pack_meshes([(ter[0], ter[1], ter[2], 0)])
    pose = ((0.0, 0.0, -1.0), meshes.IDENT, (1.0, 1.0, 1.0))
    inst = [pose + (0,), pose + (0,)]
    cams = [((0.0, 0.0, 12.0), DOWN), ((2.0, -1.0, 6.0), DOWN)]
    return scenes.SceneDesc(
        num_worlds=1, render_mode=mode, width=width, height=height, materials=_mats(True),
        texture_paths=[TEX_PATH], instances=inst, cameras=cams, worlds=[(2, 0, 2, 0)], **geo)


def instanced_scene(mode="Rasterizer", width=64, height=64, copies=24):
    """Many instances of one small dense mesh -- a sphere of 512 triangles -- in a grid under a camera looking down,
    textured: the TLAS takes several passes at MRX_BVH_PASS_INST=8, and the record table outlives a pass."""
    sph = meshes.sphere(32, 8)
    geo = meshes.pack_meshes([(sph[0], sph[1], sph[2], 0)])
    inst = []
    side = int(math.ceil(math.sqrt(copies)))
    for i in range(copies):
        x, y = (i % side - (side - 1) / 2) * 2.1, (i // side - (side - 1) / 2) * 2.1
        inst.append(((float(np.float32(x)), float(np.float32(y)), 0.0), meshes.IDENT, (1.0, 1.0, 1.0), 0))
    cams = [((0.0, 0.0, 9.0), DOWN)]
    return scenes.SceneDesc(
        num_worlds=1, render_mode=mode, width=width, height=height, materials=_mats(True),
        texture_paths=[TEX_PATH], instances=inst, cameras=cams, worlds=[(len(inst), 0, 1, 0)], **geo)


def one_tile_views(num_views, mode="Rasterizer", textured=False):
    """`num_views` 64x64 views of terrain(40) (3200 triangles) from above, each world its own pose, so that one-tile
    views overflow the table in groups of views (MRX_BVH_GROUP_VIEWS) and in the mixed pairs-and-singles launch."""
    ter = meshes.terrain(40)
    geo = meshes.pack_meshes([(ter[0], ter[1], ter[2], 0)])
    inst, cams, worlds = [], [], []
    for w in range(num_views):
        rng = np.random.default_rng(1000 + w)
        th = float(rng.uniform(0, 2 * math.pi))
        inst.append(((0.0, 0.0, -1.0), (float(np.float32(math.cos(th / 2))), 0.0, 0.0,
                                        float(np.float32(math.sin(th / 2)))), (1.0, 1.0, 1.0), 0))
        h = float(np.float32(rng.uniform(9.0, 13.0)))
        cams.append(((float(np.float32(rng.uniform(-2, 2))), float(np.float32(rng.uniform(-2, 2))), h), DOWN))
        worlds.append((1, w, 1, w))
    return scenes.SceneDesc(
        num_worlds=num_views, render_mode=mode, width=64, height=64, materials=_mats(textured),
        texture_paths=[TEX_PATH] if textured else [], instances=inst, cameras=cams, worlds=worlds, **geo)


def small_world_scene(width, num_worlds=3):
    """Raytracer views of worlds of at most 64 triangles (cube + plane + a 32-triangle sphere: 58): the flat
    kernel's territory, with ragged views of several tiles."""
    sph = meshes.sphere(8, 2)
    geo = meshes.pack_meshes([(sph[0], sph[1], sph[2], 1)])
    inst, cams, worlds = [], [], []
    for w in range(num_worlds):
        rng = np.random.default_rng(77 + w)
        i0 = len(inst)
        # objects: the disk assets first (cube 0, plane 1), then the sphere (2)
        inst.append(((0.0, 0.0, 0.0), meshes.IDENT, (8.0, 8.0, 1.0), 1))
        inst.append(((float(np.float32(rng.uniform(-1, 1))), 1.5, 0.6), meshes.IDENT, (0.6, 0.6, 0.6), 0))
        inst.append(((-1.2, 0.5, 1.0), meshes.random_quat(rng), (0.9, 0.9, 0.9), 2))
        eye = (float(np.float32(rng.uniform(-1, 1))), -4.0, float(np.float32(rng.uniform(3.5, 5.0))))
        cams.append((eye, scenes.look_at(eye, (0.0, 0.5, 0.5))))
        worlds.append((3, i0, 1, w))
    return scenes.SceneDesc(
        num_worlds=num_worlds, render_mode="Raytracer", width=width, height=width,
        asset_paths=[(meshes.CUBE, 2), (meshes.PLANE, 0)], materials=_mats(False) + [((0.8, 0.8, 0.8, 1.0), 0, 0.5, 0.5)],
        texture_paths=[TEX_PATH], instances=inst, cameras=cams, worlds=worlds, **geo)
