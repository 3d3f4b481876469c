"""The BVH tile kernel's round-overflow paths on the GPU (madrona_renderer_amd/csrc/bvh.hip, bvhTileKernel).

Every scene comes from tests/bvh_rounds.py, and tests/test_bvh_rounds_cpu.py checks that it overflows what it is
meant to: the record table (resolveStrip<FINAL=false> stashes a round's winners in the output tensors and marks
them kStashed; the tile's last round loads them back), in full and partial tiles, textured and not, and the
large-triangle list.  Each test asserts the launch shape the host reports (Manager.bvh_launch, mrx_bvh_launch),
oracle parity (bit-exact ids, segmask and colour; depth within 1 ulp), and byte identity between settings that
must agree."""
import functools

import numpy as np
import pytest

from madrona_renderer_amd import scenes
from tests import bvh_rounds as br
from tests.util import assert_parity, fetch, render_oracle

pytestmark = pytest.mark.gpu

BVH = 2          # mrx_config.kernel_variant: the BVH path whatever the scene size


def _make(monkeypatch, desc, env=None, visibility=True, outputs=None, variant=None):
    """A renderer created under the MRX_* settings in `env` (read at creation), which are gone again after."""
    with monkeypatch.context() as m:
        m.setenv("MADRONA_MI355_VISIBILITY", "1" if visibility else "0")
        if variant is not None:
            m.setenv("MADRONA_MI355_KERNEL", str(variant))
        for k, v in (env or {}).items():
            m.setenv(k, str(v))
        return scenes.make_renderer(desc, render_outputs=outputs)


def _fetch(r, desc, visibility=True, outputs=None):
    if outputs is None:
        return fetch(r, visibility=visibility, raytracer=desc.render_mode == "Raytracer")
    r.sync()
    if outputs == "RGB":
        return {"rgb": r.rgb_tensor().to_torch().cpu().numpy()}
    d = r.depth_tensor().to_torch().cpu().numpy()
    return {"depth": d.reshape(d.shape[:3])}


@functools.lru_cache(maxsize=None)
def _oracle(key):
    return render_oracle(_SCENES[key]())


_SCENES = {
    "dense-r": lambda: br.dense_scene(),
    "dense-t": lambda: br.dense_scene("Raytracer"),
    "dense-tex": lambda: br.dense_scene(textured=True),
    "dense-far-tex": lambda: br.dense_scene(textured=True, cameras=("far",)),
    "rag-72x40": lambda: br.dense_scene("Rasterizer", 72, 40, cameras=("far",)),
    "rag-33x65": lambda: br.dense_scene("Rasterizer", 33, 65, cameras=("far",)),
    "rag-200x136-tex": lambda: br.dense_scene("Rasterizer", 200, 136, textured=True, cameras=("far",)),
    "rag-rt65": lambda: br.dense_scene("Raytracer", 65, 65, cameras=("far",)),
    "ids-r": lambda: br.dense_scene(textured=True, cameras=("far",)),
    "ids-t": lambda: br.dense_scene("Raytracer", textured=True, cameras=("far",)),
    "large": lambda: br.dense_scene(cameras=("inside", "ground", "far")),
    "tie": lambda: br.tie_scene(),
    "instanced": lambda: br.instanced_scene(),
    "one-tile": lambda: br.one_tile_views(8),
    "small-200": lambda: br.small_world_scene(200),
    "small-72": lambda: br.small_world_scene(72),
}


def _shape(r, kernel="tile", **expect):
    """The reported launch: the kernel, the caps restated in tests/bvh_rounds.py, and whatever else `expect` names."""
    la = r.bvh_launch()
    assert la["kernel"] == kernel, la
    if kernel == "tile":
        tw, th = la["tile"]
        bvh_tile = {(64, 64): 0, (64, 32): 1, (32, 32): 2}[(tw, th)]
        cap = la["tex_cap"] if la["textured"] else br.tab_cap(tw, th, la["classify"])
        assert la["record_cap"] == cap, la
        assert br.shape(bvh_tile, la["classify"], la["textured"], la["tex_cap"]) == (tw, th, la["record_usable"],
                                                                                    la["big_cap"]), la
    for k, v in expect.items():
        assert la[k] == v, (k, la)
    return la


def _overflows(ref, la, rounds=2):
    """The oracle's witness for the reported shape: some tile needs `rounds` table rounds or more."""
    tw, th = la["tile"]
    w = br.witness(ref["tri_id"], tw, th, la["record_usable"], la["big_cap"])
    assert br.max_rounds(w) >= rounds, [(t.view, t.x0, t.y0, t.winners) for t in w]
    return w


def _same(a, b, keys=None):
    for k in keys or a:
        assert np.array_equal(a[k], b[k]), f"{k} differs"


def _parity(got, ref):
    assert_parity(got, {k: ref[k] for k in ("rgb", "depth", "tri_id", "segmask")})


# ---------------------------------------------------------------------------
# a. dense untextured mesh, every tile shape, with and without per-strip classification
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["dense-r", "dense-t"])
def test_dense_mesh_every_tile_shape(native, monkeypatch, key):
    desc, ref = _SCENES[key](), _oracle(key)
    first = None
    for cls in (0, 1):
        for tile in (0, 1, 2):
            r = _make(monkeypatch, desc, {"MRX_BVH_CLASSIFY": cls, "MRX_BVH_TILE": tile})
            la = _shape(r, tile=br.TILE_SHAPES[tile], classify=bool(cls and tile == 0), textured=False)
            if cls and tile == 0:
                assert (la["record_cap"], la["record_usable"], la["big_cap"]) == (1024, 1023, 96)
            w = _overflows(ref, la, rounds=4 if tile == 0 else 2)
            assert max(t.rounds for t in w if t.view == 1) == 1          # the near camera: one round
            got = fetch(r, raytracer=desc.render_mode == "Raytracer")
            _parity(got, ref)
            first = first or got
            _same(got, first)
            del r


# ---------------------------------------------------------------------------
# b. textured: the same bytes at every record cap
# ---------------------------------------------------------------------------
def test_textured_dense_mesh_every_record_cap(native, monkeypatch):
    desc, ref = _SCENES["dense-tex"](), _oracle("dense-tex")
    outs = []
    for cap in (64, 96, None):
        r = _make(monkeypatch, desc, {"MRX_BVH_TEX_CAP": cap} if cap else {})
        la = _shape(r, textured=True)
        if cap:
            assert la["tex_cap"] == cap and la["record_usable"] == cap
        else:
            assert 64 <= la["tex_cap"] <= 1008 and la["tex_cap"] % 32 == 0
        _overflows(ref, la, rounds=40 if cap == 64 else 4)
        outs.append(fetch(r))
        _parity(outs[-1], ref)
        del r
    _same(outs[0], outs[1])
    _same(outs[0], outs[2])


# ---------------------------------------------------------------------------
# c. ragged views: overflowing tiles cut short (the per-pixel stash and reload branches)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("key,env,visibility", [
    ("rag-72x40", {}, True),
    ("rag-33x65", {}, True),
    ("rag-33x65", {"MRX_BVH_TILE": 2}, False),
    ("rag-200x136-tex", {"MRX_BVH_TEX_CAP": 64}, True),
    ("rag-rt65", {}, False),                             # segmask labels stashed pixel by pixel
    ("rag-rt65", {"MRX_BVH_TILE": 1}, True),
])
def test_ragged_views_overflow_partial_tiles(native, monkeypatch, key, env, visibility):
    desc, ref = _SCENES[key](), _oracle(key)
    r = _make(monkeypatch, desc, env, visibility=visibility)
    la = _shape(r)
    w = _overflows(ref, la)
    assert any(t.partial and t.rounds >= 2 for t in w)
    _parity(_fetch(r, desc, visibility), ref)


# ---------------------------------------------------------------------------
# d. visibility ids, segmask (IDS == 2 stashes labels), no ids
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("key,visibility", [("ids-t", True), ("ids-t", False), ("ids-r", False), ("ids-r", True)])
def test_ids_segmask_and_none_across_rounds(native, monkeypatch, key, visibility):
    desc, ref = _SCENES[key](), _oracle(key)
    assert (ref["segmask"] == 1).mean() > 0.5 and (ref["segmask"] == 0).any()
    r = _make(monkeypatch, desc, {"MRX_BVH_TEX_CAP": 64}, visibility=visibility)
    _overflows(ref, _shape(r, textured=True, tex_cap=64), rounds=40)
    got = _fetch(r, desc, visibility)
    assert ("tri_id" in got) == visibility and ("segmask" in got) == (not visibility and key == "ids-t")
    _parity(got, ref)


# ---------------------------------------------------------------------------
# e. output selection: Depth and RGB byte-identical to RGBD where tiles overflow
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{}, {"MRX_BVH_TEX_CAP": 64}])
def test_selected_outputs_match_rgbd_across_rounds(native, monkeypatch, env):
    desc, ref = _SCENES["dense-tex"](), _oracle("dense-tex")
    full = _fetch(_make(monkeypatch, desc, env), desc)
    _parity(full, ref)
    for outputs in ("Depth", "RGB"):
        r = _make(monkeypatch, desc, env, outputs=outputs)
        _overflows(ref, _shape(r, textured=True))
        got = _fetch(r, desc, outputs=outputs)
        _same(got, full)
        del r


# ---------------------------------------------------------------------------
# f. streaming stores, then reloads by the same lane
# ---------------------------------------------------------------------------
def test_write_through_either_way(native, monkeypatch):
    desc, ref = _SCENES["dense-far-tex"](), _oracle("dense-far-tex")
    outs = []
    for wt in (0, 1):
        r = _make(monkeypatch, desc, {"MRX_WRITE_THROUGH": wt, "MRX_BVH_TEX_CAP": 64})
        _overflows(ref, _shape(r, textured=True, tex_cap=64), rounds=40)
        outs.append(fetch(r))
        _parity(outs[-1], ref)
        del r
    _same(outs[0], outs[1])


# ---------------------------------------------------------------------------
# g. ties across rounds: the lower visibility index wins whichever round each copy landed in
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [64, 96])
def test_ties_across_rounds_go_to_the_lower_index(native, monkeypatch, cap):
    desc, ref = _SCENES["tie"](), _oracle("tie")
    n = len(desc.mesh_indices) // 3
    r = _make(monkeypatch, desc, {"MRX_BVH_TEX_CAP": cap}, variant=BVH)
    _overflows(ref, _shape(r, textured=True, tex_cap=cap), rounds=10)
    got = fetch(r)
    hit = got["tri_id"] >= 0
    assert hit.mean() > 0.9 and (got["tri_id"][hit] < n).all()
    _parity(got, ref)


# ---------------------------------------------------------------------------
# h. the large-triangle list: every triangle large (0) or none (4096)
# ---------------------------------------------------------------------------
def test_large_list_overflows(native, monkeypatch):
    desc, ref = _SCENES["large"](), _oracle("large")
    outs = []
    for area in (None, 0, 4096):
        for cls in (0, 1):
            env = {"MRX_BVH_CLASSIFY": cls}
            if area is not None:
                env["MRX_BVH_SMALL_AREA"] = area
            r = _make(monkeypatch, desc, env)
            la = _shape(r, small_area=256 if area is None else area, classify=bool(cls))
            if area == 0:
                w = br.witness(ref["tri_id"], *la["tile"], la["record_usable"], la["big_cap"])
                assert min(t.passes for t in w) >= 4
            outs.append(fetch(r))
            _parity(outs[-1], ref)
            _same(outs[-1], outs[0])
            del r


# ---------------------------------------------------------------------------
# i. TLAS passes: the record table lives across passes
# ---------------------------------------------------------------------------
def test_table_outlives_tlas_passes(native, monkeypatch):
    desc, ref = _SCENES["instanced"](), _oracle("instanced")
    outs = []
    for env in ({"MRX_BVH_PASS_INST": 8, "MRX_BVH_TEX_CAP": 64}, {"MRX_BVH_TEX_CAP": 64}, {}):
        r = _make(monkeypatch, desc, env, variant=BVH)
        la = _shape(r, textured=True, pass_inst=env.get("MRX_BVH_PASS_INST", 24))
        _overflows(ref, la, rounds=10 if "MRX_BVH_TEX_CAP" in env else 1)
        outs.append(fetch(r))
        _parity(outs[-1], ref)
        _same(outs[-1], outs[0])
        del r


# ---------------------------------------------------------------------------
# j. one-tile views in groups of views, and the mixed pairs-and-singles launch
# ---------------------------------------------------------------------------
def test_groups_of_one_tile_views_overflow(native, monkeypatch):
    desc, ref = _SCENES["one-tile"](), _oracle("one-tile")
    base = None
    for gv in (1, 2, 4, 8):
        r = _make(monkeypatch, desc, {"MRX_BVH_GROUP_VIEWS": gv})
        la = _shape(r, group_views=gv, classify=True, group_tiles=1)
        assert la["workgroups"] == 8 // gv or (gv == 2 and la["mixed"])
        w = _overflows(ref, la)
        assert all(t.rounds >= 2 for t in w)
        got = fetch(r)
        _parity(got, ref)
        base = base or got
        _same(got, base)
        del r
    # 8 views on a device of 3 CUs: resident = 6 < 8 <= 12 -- pairs on the first two workgroups, single views on
    # the four others, unless MRX_BVH_NO_MIXED
    for no_mixed in (False, True):
        env = {"MRX_FAKE_CUS": 3}
        if no_mixed:
            env["MRX_BVH_NO_MIXED"] = 1
        r = _make(monkeypatch, desc, env)
        _shape(r, group_views=2, mixed=not no_mixed, workgroups=4 if no_mixed else 6)
        got = fetch(r)
        _parity(got, ref)
        _same(got, base)
        del r


# ---------------------------------------------------------------------------
# k. determinism: the same pose gives the same bytes, whatever order the atomics reserved records in
# ---------------------------------------------------------------------------
def test_overflowing_renders_are_deterministic(native, monkeypatch):
    desc, ref = _SCENES["dense-tex"](), _oracle("dense-tex")
    r = _make(monkeypatch, desc, {"MRX_BVH_TEX_CAP": 64})
    _overflows(ref, _shape(r, textured=True, tex_cap=64), rounds=40)
    pos = r.instance_position_tensor().to_torch()
    z0 = float(pos[1, 2])
    seen = []
    for _ in range(2):
        pos[1, 2] = z0
        r.step()
        a = fetch(r)
        pos[1, 2] = z0 + 0.75                  # the sphere moves: other winners, other rounds
        r.step()
        b = fetch(r)
        seen.append((a, b))
    _parity(seen[0][0], ref)
    assert not np.array_equal(seen[0][0]["tri_id"], seen[0][1]["tri_id"])
    _same(seen[0][0], seen[1][0])
    _same(seen[0][1], seen[1][1])


# ---------------------------------------------------------------------------
# l. the flat kernel: every run of tiles per workgroup gives the same bytes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("key,tiles", [("small-200", 16), ("small-72", 4)])
def test_flat_kernel_every_group_tiles(native, monkeypatch, key, tiles):
    desc, ref = _SCENES[key](), _oracle(key)
    base = None
    for gt in (1, 2, 3, 5, 16):
        r = _make(monkeypatch, desc, {"MRX_BVH_GROUP_TILES": gt}, visibility=False, variant=BVH)
        la = _shape(r, kernel="flat", group_tiles=min(gt, tiles), tile=(64, 64))
        assert la["workgroups"] == 3 * -(-tiles // la["group_tiles"])
        got = fetch(r, visibility=False, raytracer=True)
        _parity(got, ref)
        base = base or got
        _same(got, base)
        del r


# ---------------------------------------------------------------------------
# m. MRX_BVH_MIN_TRIS moves the dispatch across the threshold
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("key,tris", [("one-tile", 3200), ("small-72", 46)])
def test_min_tris_moves_the_dispatch(native, monkeypatch, key, tris):
    desc, ref = _SCENES[key](), _oracle(key)
    for min_tris, path in ((tris, "bvh"), (tris + 1, "raster")):
        r = _make(monkeypatch, desc, {"MRX_BVH_MIN_TRIS": min_tris})
        assert r.render_path() == path
        assert (r.bvh_launch()["kernel"] == "none") == (path == "raster")
        assert (r.raster_entry() == "bvh") == (path == "bvh")
        _parity(_fetch(r, desc), ref)
        del r
