"""CPU checks of the uniform-world generator (tests/uniform_worlds.py) that the FAST raster group kernel's
GPU tests use: it is deterministic, every scene it names meets the host's uniformity predicate (restated
here from scene.cpp bindGeometry and raster.hip launchRaster), the batches reach the cases the kernel's
per-strip near-free bit and tie rule decide, and the oracle agrees with the independent float64 caster
and shading model on them."""
import numpy as np
import pytest

from tests import uniform_worlds as uw
from tests.test_independent_raycast import raycast_colour, raycast_view
from tests.util import digest


def fast_eligible(desc, fs):
    """The host's conditions for the FAST entry, from the scene alone (scene.cpp bindGeometry: uniInstances,
    uniCamsPerWorld, uniPrefix, uniFirstTri; raster.hip launchRaster: 16 slots, one tile per view)."""
    w0 = desc.worlds[0]
    n0, c0 = w0[0], w0[2]
    if not (1 <= n0 <= 4 and 1 <= c0 < 256):
        return False
    bound0 = [desc.instances[w0[1] + i][3] for i in range(n0)]
    for ni, io, nc, _ in desc.worlds:
        if ni != n0 or nc != c0 or [desc.instances[io + i][3] for i in range(ni)] != bound0:
            return False
    if not all(0 <= o < len(fs.obj_first_tri) for o in bound0):
        return False
    if sum(int(fs.obj_num_tris[o]) for o in bound0) > 16:
        return False
    if any(int(fs.obj_first_tri[o]) >= 65536 for o in bound0):
        return False
    return fs.width <= 64 and fs.height <= 64


def test_generator_is_deterministic():
    for name in ("raster-64x32-w130", "rt-33-w7", "tex-raster-50x30-w7"):
        a, b = uw.case(name), uw.case(name)
        assert a.instances == b.instances and a.cameras == b.cameras and a.worlds == b.worlds
        assert digest(a.mesh_vertices) == digest(b.mesh_vertices)
        assert digest(a.mesh_indices) == digest(b.mesh_indices)
    # worlds differ from each other, and seeds from seeds
    d = uw.case("raster-64x32-w130")
    assert len({tuple(i[0]) for i in d.instances}) == len(d.instances)
    assert uw.uniform_scene(1, 3).instances != uw.uniform_scene(2, 3).instances


@pytest.mark.parametrize("name", sorted(uw.CASES))
def test_every_scene_is_uniform_and_fits_one_tile(oracle_mod, name):
    desc = uw.case(name)
    fs = oracle_mod.FlatScene(desc)
    assert fast_eligible(desc, fs)
    assert desc.num_worlds in uw.BATCHES


def test_cases_cover_the_issue_matrix():
    sizes = {(c.get("width", 64), c.get("height", 64)) for c in uw.CASES.values() if c.get("mode") != "Raytracer"}
    assert set(uw.RASTER_SIZES) <= sizes
    assert set(uw.RT_SIZES) <= {c["width"] for c in uw.CASES.values() if c.get("mode") == "Raytracer"}
    assert set(uw.BATCHES) <= {c["num_worlds"] for c in uw.CASES.values()}
    layouts = {uw.LAYOUTS[c["seed"] % len(uw.LAYOUTS)] for c in uw.CASES.values() if "layout" not in c}
    assert layouts == set(uw.LAYOUTS)
    assert {sum(uw.RAW_TRIS[o] for o in lay) for lay in uw.LAYOUTS} >= {1, 16}
    cams = {c.get("cams", 1 + c["seed"] % 3) for c in uw.CASES.values()}
    assert cams == {1, 2, 3}
    # the textured cases draw textured triangles (cube and quad take the texture, the others do not)
    for name, c in uw.CASES.items():
        lay = uw.LAYOUTS[c["seed"] % len(uw.LAYOUTS)]
        assert c.get("textured", False) == name.startswith("tex-")
        if name.startswith("tex-"):
            assert {"cube", "quad"} & set(lay), name


def test_header_limit_scenes_sit_on_either_side(oracle_mod):
    for first, fast in ((65535, True), (65536, False)):
        d = uw.uniform_scene(5, 3, layout=("cube", "tie"), first_raw_tri=first)
        fs = oracle_mod.FlatScene(d)
        assert int(fs.obj_first_tri[d.instances[1][3]]) == first
        assert fast_eligible(d, fs) == fast
    for cams, fast in ((255, True), (256, False)):
        d = uw.uniform_scene(6, 1, width=8, height=8, layout=("tie",), cams=cams)
        assert fast_eligible(d, oracle_mod.FlatScene(d)) == fast
    d = uw.uniform_scene(7, 3, layout=("tie", "one", "one", "one", "one"))
    assert not fast_eligible(d, oracle_mod.FlatScene(d))


def test_batches_reach_the_edges(oracle_mod):
    total = dict.fromkeys(("near_pixels", "mixed_tiles", "inside_views", "tie_pixels", "mirror_pixels"), 0)
    for name in sorted(uw.CASES):
        desc = uw.case(name)
        fs = oracle_mod.FlatScene(desc)
        ref = fs.render()
        c = uw.edge_counts(fs, ref)
        print(f"{name:24s} views {fs.num_views:5d} covered {float((ref['tri_id'] >= 0).mean()):.3f} {c}")
        assert (ref["tri_id"] >= 0).any(), f"{name}: nothing covered"
        for k in total:
            total[k] += c[k]
    print("total", total)
    for k, n in total.items():
        assert n > 0, f"no batch reaches {k}"
    # the near-free bit's case in the headline-sized batches themselves
    for name in ("raster-64x64-w1024", "rt-64-w1024"):
        fs = oracle_mod.FlatScene(uw.case(name))
        assert uw.edge_counts(fs, fs.render())["mixed_tiles"] >= 10, name


# the float64 caster names another triangle than the oracle only where its margin is 0 (ties, exact
# edges): measured on 40 views of each of six cases.  1e-6 keeps the bound of the other caster tests.
DECISIVE = 1e-6


@pytest.mark.parametrize("name", ["raster-64x64-w1024", "rt-64-w130", "raster-32x64-w7", "tex-raster-64x64-w130",
                                  "tex-rt-64-w7"])
def test_oracle_agrees_with_the_float64_caster(oracle_mod, name):
    fs = oracle_mod.FlatScene(uw.case(name))
    ref = fs.render()
    checked = hits = 0
    for v in range(0, min(fs.num_views, 60), 3):
        tri, depth, margin = raycast_view(fs, v)
        sure = margin > DECISIVE
        assert np.array_equal(ref["tri_id"][v][sure], tri[sure]), \
            f"view {v}: {(ref['tri_id'][v][sure] != tri[sure]).sum()} decisive pixels name another triangle"
        # eyes 0.003 units from a surface and nearly flat instances (an axis scaled by 1e-4): the float32
        # set-up carries up to 1.3e-4 (measured on these views) against float64
        np.testing.assert_allclose(ref["depth"][v][sure], depth[sure], rtol=3e-4)
        rgb, sure_tex = raycast_colour(fs, v)
        ok = sure & sure_tex & (tri >= 0)
        diff = np.abs(ref["rgb"][v][..., :3].astype(np.float64) - np.floor(rgb + 0.5))
        near_half = np.abs(rgb - np.floor(rgb) - 0.5) < 0.02
        assert not (ok[..., None] & (diff > np.where(near_half, 1.0, 0.0))).any(), f"view {v}: colour"
        checked += int(sure.sum())
        hits += int((ref["tri_id"][v] >= 0).sum())
    # (ties, duplicate triangles, pixels at the far plane and on nearly flat instances are never decisive)
    assert checked > 0.5 * hits > 0, f"only {checked} of {hits} covered pixels were decisive"


def test_ulp_distance_of_assert_parity():
    from tests.util import depth_ulps
    a = np.array([1.0, 2.0, 0.0, 0.5], np.float32)
    b = a.copy()
    assert depth_ulps(a, b) == 0
    b[0] = np.nextafter(np.float32(1.0), np.float32(2.0))
    assert depth_ulps(a, b) == 1
    b[1] = np.float32(2.0) * np.float32(1 + 1e-6)
    assert depth_ulps(a, b) >= 8
    with pytest.raises(AssertionError, match="background"):
        depth_ulps(a, np.array([1.0, 2.0, 1e-30, 0.5], np.float32))
    with pytest.raises(AssertionError, match="sign"):
        depth_ulps(a, np.array([1.0, -2.0, 0.0, 0.5], np.float32))
