"""CPU checks behind tests/test_bvh_rounds_gpu.py: every scene there reaches the round-overflow path it claims
(tests/bvh_rounds.py: lower bounds from the oracle alone), so a later edit to a scene cannot quietly make it benign;
and on those scenes the oracle agrees with the float64 caster of test_independent_raycast.py on decisive pixels."""
import numpy as np
import pytest

from tests import bvh_rounds as br
from tests.test_independent_raycast import raycast_colour, raycast_view
from tests.util import render_oracle


def _wit(desc, **shape):
    return br.witness(render_oracle(desc)["tri_id"], *br.shape(**shape))


def test_witness_counts_distinct_winners_per_storage_tile():
    # a hand-made id buffer: 2 views of 70 (slow) x 36 (fast) pixels, tiles 32 x 32
    ids = np.full((2, 70, 36), -1, np.int32)
    ids[0, :32, :32] = np.arange(32 * 32).reshape(32, 32) % 600      # 600 distinct winners in tile (0, 0)
    ids[0, 64:, 32:] = 7                                             # one winner in the corner tile
    ids[1, 40:50, 0:3] = np.arange(30).reshape(10, 3)
    w = br.witness(ids, 32, 32, 512, 64)
    assert [(t.view, t.x0, t.y0) for t in w[:6]] == [(0, 0, 0), (0, 32, 0), (0, 0, 32), (0, 32, 32), (0, 0, 64),
                                                     (0, 32, 64)]
    t = {(t.view, t.x0, t.y0): t for t in w}
    assert (t[0, 0, 0].winners, t[0, 0, 0].rounds, t[0, 0, 0].passes) == (600, 2, 10)
    assert not t[0, 0, 0].partial and t[0, 32, 0].partial          # 36 - 32 = 4 pixels wide
    assert t[0, 0, 64].partial                                      # 70 - 64 = 6 rows
    assert (t[0, 32, 64].winners, t[0, 32, 64].rounds) == (1, 1)
    assert (t[1, 0, 32].winners, t[1, 0, 32].rounds, t[1, 0, 32].passes) == (30, 1, 1)
    assert t[1, 32, 32].winners == 0 and t[1, 32, 32].rounds == 1
    # a width that is not a multiple of 4 takes the per-pixel branches in every tile
    assert all(t.partial for t in br.witness(ids[:, :, :33], 32, 32, 512, 64))


def test_restated_constants():
    # bvh.hip: kStashed = (1 << kSlotBits) - 1; tabCap / tabUsable / bigCap (the GPU tests compare these with
    # what the host reports for each launch)
    assert br.STASHED == 1023
    assert br.shape(0) == (64, 64, 768, 64)
    assert br.shape(0, classify=True) == (64, 64, 1023, 96)          # 1024 records, slot 1023 is the marker
    assert br.shape(1, classify=True) == (64, 32, 512, 64)           # CLS is a 64x64 instantiation only
    assert br.shape(2) == (32, 32, 512, 64)
    assert br.shape(0, textured=True, tex_cap=64) == (64, 64, 64, 64)
    assert br.shape(0, classify=True, textured=True, tex_cap=1008) == (64, 64, 1008, 96)


@pytest.mark.parametrize("bvh_tile,classify,rounds", [(0, False, 6), (0, True, 4), (1, False, 4), (2, False, 2)])
def test_dense_scene_overflows_every_tile_shape(bvh_tile, classify, rounds):
    # case a: the far camera overflows whatever the tile shape, the near one fits a single round
    w = _wit(br.dense_scene(), bvh_tile=bvh_tile, classify=classify)
    assert br.max_rounds(w, view=0) >= rounds
    assert all(t.rounds >= 2 for t in w if t.view == 0)
    assert br.max_rounds(w, view=1) == 1


def test_dense_scene_raytracer_overflows():
    w = _wit(br.dense_scene("Raytracer", 64, 64), bvh_tile=0, classify=True)
    assert br.max_rounds(w, view=0) >= 3 and br.max_rounds(w, view=1) == 1
    w = _wit(br.dense_scene("Raytracer", 64, 64), bvh_tile=2)
    assert br.max_rounds(w, view=0) >= 2


@pytest.mark.parametrize("tex_cap,rounds", [(64, 40), (96, 30), (1008, 4)])
def test_textured_dense_scene_overflows_at_every_cap(tex_cap, rounds):
    # case b: the default cap is at most 1008 records (scene.cpp chooseBvhGroups)
    w = _wit(br.dense_scene(textured=True), textured=True, tex_cap=tex_cap)
    assert br.max_rounds(w, view=0) >= rounds


@pytest.mark.parametrize("mode,size,shape", [
    ("Rasterizer", (72, 40), dict(bvh_tile=0, classify=True)),
    ("Rasterizer", (33, 65), dict(bvh_tile=0, classify=True)),
    ("Rasterizer", (33, 65), dict(bvh_tile=2)),
    ("Rasterizer", (200, 136), dict(textured=True, tex_cap=64)),
    ("Raytracer", (65, 65), dict(bvh_tile=0, classify=True)),
])
def test_ragged_views_overflow_a_partial_tile(mode, size, shape):
    # case c: the per-pixel stash and reload branches (a tile cut short, or a width that is not a multiple of 4)
    w = _wit(br.dense_scene(mode, *size, textured=shape.get("textured", False), cameras=("far",)), **shape)
    assert any(t.partial and t.rounds >= 2 for t in w)
    assert any(not t.partial for t in w) or size[0] % 4 != 0 or size[1] < 64


def test_ties_overflow_where_they_are_visible():
    # case g: two copies of one terrain at one pose; every covered pixel is a tie the lower copy wins
    d = br.tie_scene()
    ref = render_oracle(d)
    n = len(d.mesh_indices) // 3
    hit = ref["tri_id"] >= 0
    assert hit.mean() > 0.9 and (ref["tri_id"][hit] < n).all()
    w = br.witness(ref["tri_id"], *br.shape(textured=True, tex_cap=64))
    assert all(t.rounds >= 10 for t in w)


def test_large_list_overflows_with_small_area_zero():
    # case h: every triangle large; the eye inside the sphere and just above the terrain
    w = _wit(br.dense_scene(cameras=("inside", "ground", "far")), bvh_tile=0, classify=True)
    assert min(t.passes for t in w) >= 4 and br.max_rounds(w, view=2) >= 4


def test_instanced_scene_overflows_across_passes():
    # case i: 24 instances, three TLAS passes at MRX_BVH_PASS_INST=8, cap 64
    d = br.instanced_scene()
    assert len(d.instances) == 24
    w = _wit(d, textured=True, tex_cap=64)
    assert br.max_rounds(w) >= 10


def test_one_tile_views_overflow():
    # case j: every one-tile view needs two rounds or more at the CLS table's 1023 records
    w = _wit(br.one_tile_views(8), bvh_tile=0, classify=True)
    assert len(w) == 8 and all(t.rounds >= 2 for t in w) and br.max_rounds(w) >= 3


def test_small_worlds_are_the_flat_kernels():
    # case l: at most 64 triangles in at most 64 rows per world (scene.cpp chooseBvhGroups), views of several tiles
    d = br.small_world_scene(200)
    from oracle import oracle
    fs = oracle.FlatScene(d)
    assert len(fs.tri_pos) <= 64 and all(n <= 64 for n, _, _, _ in d.worlds)
    ref = fs.render()
    assert ref["tri_id"].shape == (3, 200, 200)
    assert ((ref["tri_id"] >= 0).mean(axis=(1, 2)) > 0.3).all()


@pytest.mark.parametrize("scene,views,decisive,colour", [
    ("dense", (0, 1), 0.5, True),
    ("dense-rt", (0,), 0.5, True),
    # (colour: the sphere's pole triangles collapse their uv edge, which the caster's texel choice does not model)
    ("instanced", (0,), 0.5, False),
])
def test_oracle_agrees_with_the_float64_caster_on_the_new_scenes(oracle_mod, scene, views, decisive, colour):
    d = {"dense": lambda: br.dense_scene(cameras=("far", "inside")),
         "dense-rt": lambda: br.dense_scene("Raytracer", 48, 48, cameras=("far",)),
         "instanced": lambda: br.instanced_scene()}[scene]()
    fs = oracle_mod.FlatScene(d)
    ref = fs.render()
    for v in views:
        tri, depth, margin = raycast_view(fs, v)
        sure = margin > 1e-4          # (edge pixels of adjacent mesh triangles within float32 of a tie are not)
        hits = int((ref["tri_id"][v] >= 0).sum())
        assert sure.sum() >= decisive * hits > 0, f"view {v}: {int(sure.sum())} of {hits} decisive"
        bad = int((ref["tri_id"][v][sure] != tri[sure]).sum())
        assert bad == 0, f"view {v}: {bad} decisive pixels name another triangle"
        np.testing.assert_allclose(ref["depth"][v][sure], depth[sure], rtol=1e-4)
        if not colour:
            continue
        rgb, sure_tex = raycast_colour(fs, v)
        near_half = np.abs(rgb - np.floor(rgb) - 0.5) < 0.02
        diff = np.abs(ref["rgb"][v][..., :3].astype(np.float64) - np.floor(rgb + 0.5))
        assert not ((sure & sure_tex)[..., None] & (diff > np.where(near_half, 1.0, 0.0))).any()


def test_bvh_launch_refuses_a_null_renderer(native):
    # mrx_bvh_launch (include/mrx.h), as mrx_raster_entry: argument checks before anything touches HIP
    import ctypes
    lib = native.load_capi()
    lib.mrx_last_error.restype = ctypes.c_char_p
    lib.mrx_bvh_launch.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    buf = (ctypes.c_uint8 * 128)()
    assert lib.mrx_bvh_launch(None, ctypes.byref(buf)) == -1 and b"null renderer" in lib.mrx_last_error()
    assert lib.mrx_bvh_launch(None, None) == -1
    assert hasattr(native.load_module().MadronaRenderer, "bvh_launch")
