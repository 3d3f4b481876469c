"""Per-world light on the MI355X (-m gpu): mixed lights -- along every axis, grazing, ambient only, diffuse only,
over-bright -- against the oracle rendered group by group under the same lights (tests/light_oracle.py), through
every kernel family and with mixed projections beside them; the uniform form; defaults given explicitly;
set_world_light between steps, its stream order and its refusals; a renderer of two shards; the headless binary.
Colour, visibility and segmask bit for bit, depth to 1 ulp (tests.util.assert_parity, unchanged)."""
import dataclasses
import subprocess

import numpy as np
import pytest

from madrona_renderer_amd import scenes
from tests import light_oracle as lo
from tests import meshes
from tests import projection_oracle as po
from tests.test_projection_gpu import CASES, _fetch_sel, _make
from tests.util import assert_parity, depth_ulps, fetch

pytestmark = pytest.mark.gpu


def _with(desc, lights=None, projections=None):
    d = dataclasses.replace(desc)
    d.world_lights = None if lights is None else list(lights)
    if projections is not None:
        d.camera_projections = list(projections)
    return d


def _check(r, desc, lights, raytracer=False, visibility=True, views=None, projections=None):
    got = fetch(r, visibility=visibility, raytracer=raytracer)
    lo_, hi = views if views else (0, desc.num_views)
    ref = lo.render(desc, lights, projections, lo_, hi, want_ids=visibility or raytracer)
    got = {k: v[lo_:hi] for k, v in got.items()}
    ref = {k: ref[k][lo_:hi] for k in got}
    assert_parity(got, ref)
    return ref


def _assert_light_decided_pixels(base, ref, rt, n=50):
    """`ref` (under the lights) against the default-light oracle: colour differs, nothing else does."""
    n = min(n, base.num_views)
    plain = po.render(base, None, 0, n, want_ids=True)
    assert (plain["rgb"][:n] != ref["rgb"][:n]).any()
    key = "segmask" if rt else "tri_id"
    assert np.array_equal(plain[key][:n], ref[key][:n])
    assert np.array_equal(plain["depth"][:n].view(np.uint32), np.asarray(ref["depth"][:n], np.float32).view(np.uint32))


def _read_back(r, lights):
    d, a, f = r.world_light()
    assert d.tolist() == [[np.float32(x) for x in l[0]] for l in lights]
    assert a.tolist() == [np.float32(l[1]) for l in lights] and f.tolist() == [np.float32(l[2]) for l in lights]


@pytest.mark.parametrize("case", list(CASES))
def test_mixed_lights_match_the_oracle(native, case):
    build, variant, entry, bvh, rt = CASES[case]
    base = build()
    lights = lo.mixed(base.num_worlds)
    r = _make(_with(base, lights), visibility=not rt, variant=variant)
    assert r.raster_entry() == entry
    assert r.bvh_launch()["kernel"] == bvh
    if case == "bvh-tile-pairs":
        assert r.bvh_launch()["group_views"] == 2
    _read_back(r, lights)
    ref = _check(r, base, lights, raytracer=rt, visibility=not rt)
    ref_ids = lo.render(base, lights, None, 0, min(50, base.num_views), want_ids=True)
    _assert_light_decided_pixels(base, ref_ids, rt)


def test_mixed_lights_through_the_plain_entry_at_16_slots(native, monkeypatch):
    # the light-table form behind the plain entry of a 16-slot world (the FAST entry switched off): two one-tile views
    monkeypatch.setenv("MRX_GROUP_FAST", "0")
    base = scenes.synthetic_scene(2)
    lights = lo.mixed(base.num_worlds)
    r = _make(_with(base, lights))
    assert r.raster_entry() == "group"
    _check(r, base, lights)


@pytest.mark.parametrize("outputs", ["RGBD", "Depth"])
def test_raytracer_flat_kernel_with_mixed_lights(native, outputs):
    # BASELINE configs[4]'s shape (4096 views of 256x256, Raytracer mode): the BVH path's flat kernel; a slice of the
    # views against the oracle
    base = scenes.synthetic_scene(4096, width=256, height=256, render_mode="Raytracer")
    lights = lo.mixed(base.num_worlds)
    sel = None if outputs == "RGBD" else outputs
    r = _make(_with(base, lights), visibility=False, outputs=sel)
    assert r.raster_entry() == "bvh" and r.bvh_launch()["kernel"] == "flat"
    r.sync()
    n = 44
    seg = r.segmask_tensor().to_torch()[:n].cpu().numpy()
    d = r.depth_tensor().to_torch()[:n].cpu().numpy()
    d = d.reshape(d.shape[0], d.shape[1], d.shape[2])
    ref = lo.render(base, lights, None, 0, n, want_ids=True)
    if outputs == "RGBD":
        rgb = r.rgb_tensor().to_torch()[:n].cpu().numpy()
        assert_parity({"segmask": seg, "rgb": rgb, "depth": d}, {k: ref[k][:n] for k in ("segmask", "rgb", "depth")})
        _assert_light_decided_pixels(base, ref, True, n=22)
    else:
        assert int((seg != ref["segmask"][:n]).sum()) == 0
        plain = _make(base, visibility=False, outputs=sel)
        plain.sync()
        d0 = plain.depth_tensor().to_torch()[:n].cpu().numpy().reshape(d.shape)
        assert np.array_equal(d.view(np.uint32), d0.view(np.uint32))   # the light never reaches the depth
        np.testing.assert_allclose(d, ref["depth"][:n], rtol=1e-4, atol=0)
        assert depth_ulps(d, ref["depth"][:n]) <= 1


@pytest.mark.parametrize("outputs", ["RGBD", "Depth", "RGB"])
def test_mixed_lights_under_output_selection(native, outputs):
    base = scenes.synthetic_scene(1024)
    lights = lo.mixed(base.num_worlds)
    sel = None if outputs == "RGBD" else outputs
    r = _make(_with(base, lights), visibility=False, outputs=sel)
    assert r.raster_entry() == "group-fast"
    ref = lo.render(base, lights, want_ids=False)
    if sel is None:
        _check(r, base, lights, visibility=False)
        return
    got = _fetch_sel(r, outputs)
    if outputs == "Depth":
        assert "rgb" not in got
        np.testing.assert_allclose(got["depth"], ref["depth"], rtol=1e-4, atol=0)
        assert depth_ulps(got["depth"], ref["depth"]) <= 1
    else:
        assert "depth" not in got
        assert int((got["rgb"] != ref["rgb"]).any(axis=-1).sum()) == 0


@pytest.mark.parametrize("case", ["group-fast", "bvh-tile", "flat"])
def test_mixed_lights_and_mixed_projections_together(native, case):
    if case == "flat":
        base = scenes.synthetic_scene(4096, width=256, height=256, render_mode="Raytracer")
        entry, bvh, rt, views = "bvh", "flat", True, (0, 40)
    else:
        build, _, entry, bvh, rt = CASES[case]
        base, views = build(), None
        if case == "group-fast":
            views = (0, 600)
    lights = lo.mixed(base.num_worlds, shift=2)
    projs = po.mixed(len(base.cameras))
    r = _make(_with(base, lights, projs), visibility=not rt)
    assert r.raster_entry() == entry and r.bvh_launch()["kernel"] == bvh
    _check(r, base, lights, raytracer=rt, visibility=not rt, views=views, projections=projs)


def test_uniform_non_default_light_takes_the_argument_form(native):
    base = scenes.synthetic_scene(512, textured=True)
    light = ((0.0, 0.0, -1.0), 0.1, 0.9)
    r = _make(_with(base, [light] * base.num_worlds))
    assert r.raster_entry() == "group-fast"
    _check(r, base, [light] * base.num_worlds)
    uni = fetch(r)
    # the table form given that one light for every world: the same bytes.  (World 0's direction has another
    # length: the lights differ as given, so the table is launched with, and resolve to the same constants.)
    lights = [light] * base.num_worlds
    lights[0] = ((0.0, 0.0, -2.0), 0.1, 0.9)
    t = _make(_with(base, lights))
    tab = fetch(t)
    for k in uni:
        assert np.array_equal(uni[k].view(np.uint8), tab[k].view(np.uint8)), k


def test_explicit_defaults_render_the_same_bytes(native):
    for build in (lambda: scenes.synthetic_scene(256, textured=True),
                  lambda: meshes.cube_field(num_worlds=16, cubes=40),
                  lambda: scenes.synthetic_scene(64, width=128, height=128, render_mode="Raytracer")):
        base = build()
        rt = base.render_mode == "Raytracer"
        a = fetch(_make(base, visibility=not rt), visibility=not rt, raytracer=rt)
        b = fetch(_make(_with(base, [lo.DEFAULT] * base.num_worlds), visibility=not rt), visibility=not rt, raytracer=rt)
        for k in a:
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def test_set_world_light_between_steps(native):
    base = scenes.synthetic_scene(256, with_wall=True)
    n = base.num_worlds
    r = _make(base)
    first = fetch(r)
    # mixed, through arrays
    lights = lo.mixed(n)
    r.set_world_light(np.array([l[0] for l in lights], np.float32), [l[1] for l in lights], [l[2] for l in lights])
    r.step()
    _read_back(r, lights)
    _check(r, base, lights)
    before = fetch(r)
    # a sub-range: one triple for worlds 100 .. 109, their ambient / diffuse kept; the others' pixels untouched
    r.set_world_light(np.tile(np.array([0.0, 0.0, -1.0], np.float32), (10, 1)), first_world=100)
    want = list(lights)
    want[100:110] = [((0.0, 0.0, -1.0), l[1], l[2]) for l in lights[100:110]]
    r.step()
    _read_back(r, want)
    _check(r, base, want)
    after = fetch(r)
    keep = np.r_[0:100, 110:n]
    assert np.array_equal(before["rgb"][keep], after["rgb"][keep])
    assert (before["rgb"][100:110] != after["rgb"][100:110]).any()
    # one triple and scalars: every world from first_world on (uniform again)
    r.set_world_light((2.0, 0.0, -2.0), 0.3, 0.6)
    r.step()
    _check(r, base, [((2.0, 0.0, -2.0), 0.3, 0.6)] * n)
    # back to the defaults: the first frame's bytes
    r.set_world_light(lo.DEFAULT[0], lo.DEFAULT[1], lo.DEFAULT[2])
    r.step()
    last = fetch(r)
    for k in first:
        assert np.array_equal(first[k].view(np.uint8), last[k].view(np.uint8)), k


def test_set_world_light_is_stream_ordered(native):
    import torch
    base = scenes.synthetic_scene(512)
    n = base.num_worlds
    old, new = lo.mixed(n), lo.mixed(n, shift=5)
    r = _make(_with(base, old))
    s = torch.cuda.Stream()
    r.set_stream(s.cuda_stream)
    with torch.cuda.stream(s):
        r.step()                                          # A
        r.set_world_light(np.array([l[0] for l in new], np.float32), [l[1] for l in new], [l[2] for l in new])
        a_rgb = r.rgb_tensor().to_torch().clone()
        a_ids = r.visibility_tensor().to_torch().clone()
        r.step()                                          # B
        b_rgb = r.rgb_tensor().to_torch().clone()
        b_ids = r.visibility_tensor().to_torch().clone()
    s.synchronize()
    ref_a = lo.render(base, old, want_ids=True)
    ref_b = lo.render(base, new, want_ids=True)
    assert (ref_a["rgb"] != ref_b["rgb"]).any()
    assert np.array_equal(a_ids.cpu().numpy(), ref_a["tri_id"]) and np.array_equal(a_rgb.cpu().numpy(), ref_a["rgb"])
    assert np.array_equal(b_ids.cpu().numpy(), ref_b["tri_id"]) and np.array_equal(b_rgb.cpu().numpy(), ref_b["rgb"])


def test_a_refused_set_changes_nothing(native):
    base = scenes.synthetic_scene(128)
    n = base.num_worlds
    lights = lo.mixed(n)
    r = _make(_with(base, lights))
    before = fetch(r)
    nan, inf = float("nan"), float("inf")
    for bad in (((0.0, 0.0, 0.0), 0.2, 0.8), ((nan, 0.0, 1.0), 0.2, 0.8), ((1.0, 0.0, 0.0), -0.1, 0.8),
                ((1.0, 0.0, 0.0), 0.2, inf)):
        rng = [((0.0, 1.0, 0.0), 0.5, 0.5)] * 9
        rng[4] = bad                                      # one bad light in the middle of a range
        with pytest.raises(ValueError):
            r.set_world_light(np.array([l[0] for l in rng], np.float32), [l[1] for l in rng], [l[2] for l in rng],
                              first_world=20)
    for bad in (dict(direction=[(1.0, 0.0, 0.0)] * (n + 1)), dict(direction=(1.0, 0.0, 0.0), first_world=n + 1),
                dict(direction=(1.0, 0.0)), dict(direction=[(1.0, 0.0, 0.0)] * 3, ambient=[0.1] * 4)):
        with pytest.raises(ValueError):
            r.set_world_light(**bad)
    _read_back(r, lights)
    r.step()
    after = fetch(r)
    for k in before:
        assert np.array_equal(before[k].view(np.uint8), after[k].view(np.uint8)), k


def test_two_shards_split_the_whole_job_world_range(native):
    base = scenes.synthetic_scene(301)
    n = base.num_worlds
    lights = lo.mixed(n)
    r = _make(_with(base, lights), device_ids=[0, 0])
    assert r.num_shards == 2
    _read_back(r, lights)
    new = list(lights)
    new[140:170] = [((0.0, 0.0, -1.0), 0.05, 0.95)] * 30   # across the shard boundary (151)
    r.set_world_light(np.tile(np.array([0.0, 0.0, -1.0], np.float32), (30, 1)), 0.05, 0.95, first_world=140)
    r.refresh_objects()                                    # keeps the lights
    r.step()
    r.sync()
    _read_back(r, new)
    ref = lo.render(base, new, want_ids=True)
    for sh in range(2):
        a, b = r.shard_first_world(sh), r.shard_first_world(sh + 1)
        ids = r.visibility_tensor(shard=sh).to_torch().cpu().numpy()
        rgb = r.rgb_tensor(shard=sh).to_torch().cpu().numpy()
        assert np.array_equal(ids, ref["tri_id"][a:b]) and np.array_equal(rgb, ref["rgb"][a:b])


def test_over_bright_light_on_a_textured_scene_is_clamped(native):
    base = scenes.synthetic_scene(256, textured=True)
    light = ((-1.0, -1.0, -1.0), 0.9, 0.9)
    lights = [light if w % 2 else ((0.0, 0.0, -1.0), 0.9, 0.9) for w in range(base.num_worlds)]
    r = _make(_with(base, lights))
    ref = _check(r, base, lights)
    assert (ref["rgb"][..., :3] == 255).any()              # the clamp decided pixels


def test_headless_light(native, tmp_path):
    from madrona_renderer_amd import build
    from tests.test_headless_gpu import _tiles
    exe = build.headless_path()
    args = ["16", "2", "rast", "64", "64"]
    ok = subprocess.run(["timeout", "-k", "5", "120", exe] + args +
                        ["--light", "0,0,-1,0.1,0.9", "--dump-last-frame", "frame"], cwd=tmp_path,
                        capture_output=True, text=True)
    assert ok.returncode == 0, ok.stderr
    ref = lo.render(scenes.synthetic_scene(16), [((0.0, 0.0, -1.0), 0.1, 0.9)] * 16)["rgb"]
    plain = po.render(scenes.synthetic_scene(16))["rgb"]
    assert (ref != plain).any()
    for w, tile in enumerate(_tiles(tmp_path / "frame.png", 16, 64, 64)):
        assert np.array_equal(tile, ref[w]), f"world {w}"
    for bad in (["--light", "0,0,0"], ["--light", "1,0"], ["--light", "1,0,0,-0.1,0.5"], ["--light", "a,b,c"],
                ["--light", "1,0,0,0.5"], ["--light", "1,0,0,0.1,0.2,0.3"], ["--light", "nan,0,0"]):
        p = subprocess.run(["timeout", "-k", "5", "120", exe] + args + bad, cwd=tmp_path, capture_output=True, text=True)
        assert p.returncode not in (0, 124, 137) and "--light" in p.stderr, (bad, p.stderr)
