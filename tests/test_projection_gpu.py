"""Per-view projection on the MI355X (-m gpu): mixed fovs and near planes -- some cutting through the cube, so that
the near plane and the S6b pad decide pixels -- against the oracle rendered group by group under the same
projections (tests/projection_oracle.py), through every kernel family; the uniform form; defaults given explicitly;
set_camera_projection between steps and its stream order; a renderer of two shards; the headless binary."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

from madrona_renderer_amd import scenes
from tests import meshes
from tests import projection_oracle as po
from tests.util import assert_parity, fetch

pytestmark = pytest.mark.gpu


def _make(desc, visibility=True, variant=None, outputs=None, **kw):
    old = {k: os.environ.get(k) for k in ("MADRONA_MI355_VISIBILITY", "MADRONA_MI355_KERNEL")}
    os.environ["MADRONA_MI355_VISIBILITY"] = "1" if visibility else "0"
    if variant is not None:
        os.environ["MADRONA_MI355_KERNEL"] = str(variant)
    try:
        return scenes.make_renderer(desc, render_outputs=outputs, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _with(desc, projections):
    d = dataclasses.replace(desc)
    d.camera_projections = list(projections)
    return d


def _check(r, desc, raytracer=False, visibility=True, views=None, outputs=None, projections=None):
    got = fetch(r, visibility=visibility, raytracer=raytracer) if outputs is None else _fetch_sel(r, outputs)
    lo, hi = views if views else (0, desc.num_views)
    ref = po.render(desc, projections, lo, hi, want_ids=visibility or raytracer)
    got = {k: v[lo:hi] for k, v in got.items()}
    ref = {k: ref[k][lo:hi] for k in got}
    if outputs == "Depth":
        np.testing.assert_allclose(got["depth"], ref["depth"], rtol=1e-4, atol=0)
        return ref
    if outputs == "RGB":
        assert int((got["rgb"] != ref["rgb"]).any(axis=-1).sum()) == 0
        return ref
    assert_parity(got, ref)
    return ref


def _fetch_sel(r, outputs):
    r.sync()
    out = {}
    if outputs != "Depth":
        out["rgb"] = r.rgb_tensor().to_torch().cpu().numpy()
    if outputs != "RGB":
        d = r.depth_tensor().to_torch().cpu().numpy()
        out["depth"] = d.reshape(d.shape[0], d.shape[1], d.shape[2])
    return out


# (builder, kernel variant, the entry the render must reach, the BVH kernel, raytracer)
CASES = {
    "group-fast": (lambda: scenes.synthetic_scene(4096), None, "group-fast", "none", False),
    "group": (lambda: scenes.synthetic_scene(96, width=128, height=128, with_wall=True), None, "group", "none", False),
    "textured": (lambda: scenes.synthetic_scene(512, textured=True), None, "group-fast", "none", False),
    "chunked": (lambda: meshes.cube_field(num_worlds=24, cubes=40), 3, "chunked", "none", False),
    "brute": (lambda: scenes.synthetic_scene(48, with_wall=True), 1, "brute", "none", False),
    "bvh-tile": (lambda: meshes.cube_field(num_worlds=48, cubes=40), None, "bvh", "tile", False),
    "bvh-tile-pairs": (lambda: meshes.cube_field(num_worlds=700, cubes=40), None, "bvh", "tile", False),
    "bvh-tile-rt": (lambda: meshes.cube_field(num_worlds=9, cubes=40, mode="Raytracer", textured=True), None, "bvh",
                    "tile", True),
}


@pytest.mark.parametrize("case", list(CASES))
def test_mixed_projections_match_the_oracle(native, case):
    build, variant, entry, bvh, rt = CASES[case]
    base = build()
    desc = _with(base, po.mixed(len(base.cameras)))
    r = _make(desc, visibility=not rt, variant=variant)
    assert r.raster_entry() == entry
    assert r.bvh_launch()["kernel"] == bvh
    if case == "bvh-tile-pairs":
        assert r.bvh_launch()["group_views"] == 2
    f, z = r.camera_projection()
    want = po.view_projections(desc)
    assert f.tolist() == [np.float32(a) for a, _ in want]
    dflt = 0.1 if rt else 0.001
    assert z.tolist() == [np.float32(dflt if b is None else b) for _, b in want]
    ref = _check(r, desc, raytracer=rt, visibility=not rt)
    # the projections decide pixels: the same views under the defaults differ
    plain = po.render(base, None, 0, min(50, base.num_views), want_ids=True)
    key = "tri_id" if not rt else "segmask"
    assert (plain[key][:50] != ref[key][:50]).any()


@pytest.mark.parametrize("outputs", ["RGBD", "Depth", "RGB"])
def test_mixed_projections_under_output_selection(native, outputs):
    base = scenes.synthetic_scene(1024)
    desc = _with(base, po.mixed(len(base.cameras)))
    r = _make(desc, visibility=False, outputs=outputs)
    assert r.raster_entry() == "group-fast"
    _check(r, desc, visibility=False, outputs=None if outputs == "RGBD" else outputs)


def test_mixed_projections_through_the_plain_entry_at_16_slots(native, monkeypatch):
    # the per-view form behind the plain entry of a 16-slot world, which a batch reaches only with the FAST entry
    # switched off: two one-tile views
    monkeypatch.setenv("MRX_GROUP_FAST", "0")
    base = scenes.synthetic_scene(2)
    desc = _with(base, po.mixed(len(base.cameras)))
    r = _make(desc)
    assert r.raster_entry() == "group"
    _check(r, desc)


@pytest.mark.parametrize("outputs", ["RGBD", "Depth"])
def test_raytracer_flat_kernel_with_mixed_projections(native, outputs):
    # BASELINE configs[4]'s shape (4096 views of 256x256, Raytracer mode): the BVH path's flat kernel; a slice of the
    # views against the oracle
    base = scenes.synthetic_scene(4096, width=256, height=256, render_mode="Raytracer")
    desc = _with(base, po.mixed(len(base.cameras), znears=(None, 0.5, 2.0, 999.0, 3.0)))
    r = _make(desc, visibility=False, outputs=None if outputs == "RGBD" else outputs)
    assert r.raster_entry() == "bvh" and r.bvh_launch()["kernel"] == "flat"
    r.sync()
    got = {"segmask": r.segmask_tensor().to_torch()[:60].cpu().numpy()}
    d = r.depth_tensor().to_torch()[:60].cpu().numpy()
    got["depth"] = d.reshape(d.shape[0], d.shape[1], d.shape[2])
    ref = po.render(desc, None, 0, 60, want_ids=True)
    assert int((got["segmask"] != ref["segmask"][:60]).sum()) == 0
    np.testing.assert_allclose(got["depth"], ref["depth"][:60], rtol=1e-4, atol=0)
    if outputs == "RGBD":
        rgb = r.rgb_tensor().to_torch()[:60].cpu().numpy()
        assert int((rgb != ref["rgb"][:60]).any(axis=-1).sum()) == 0


def test_uniform_non_default_projection_takes_the_argument_form(native):
    base = scenes.synthetic_scene(512)
    desc = _with(base, [(60.0, None)] * len(base.cameras))
    r = _make(desc)
    assert r.raster_entry() == "group-fast"
    _check(r, desc)
    import ctypes
    lib = native.load_capi()
    # the uniform form: no per-view table -- the kernel-argument constants are 60 degrees'
    f, z = r.camera_projection()
    assert (f == 60.0).all() and (z == np.float32(0.001)).all()


def test_explicit_defaults_render_the_same_bytes(native):
    for build in (lambda: scenes.synthetic_scene(256, textured=True),
                  lambda: meshes.cube_field(num_worlds=16, cubes=40),
                  lambda: scenes.synthetic_scene(64, width=128, height=128, render_mode="Raytracer")):
        base = build()
        rt = base.render_mode == "Raytracer"
        a = fetch(_make(base, visibility=not rt), visibility=not rt, raytracer=rt)
        b = fetch(_make(_with(base, [(90.0, None)] * len(base.cameras)), visibility=not rt), visibility=not rt,
                  raytracer=rt)
        c = fetch(_make(_with(base, [(90.0, 0.1 if rt else 0.001)] * len(base.cameras)), visibility=not rt),
                  visibility=not rt, raytracer=rt)
        for k in a:
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
            assert np.array_equal(a[k].view(np.uint8), c[k].view(np.uint8)), k


def test_set_camera_projection_between_steps(native):
    base = scenes.synthetic_scene(256, with_wall=True)
    n = len(base.cameras)
    mixed_a = po.mixed(n)
    mixed_b = po.mixed(n, fovs=(150.0, 45.0, 100.0), znears=(1.5, None, 2.5))
    r = _make(_with(base, mixed_a))
    _check(r, base, projections=mixed_a)
    # uniform
    r.set_camera_projection(70.0, 1.0)
    r.step()
    _check(r, base, projections=[(70.0, 1.0)] * n)
    f, z = r.camera_projection()
    assert (f == 70.0).all() and (z == 1.0).all()
    # mixed again, through sequences, and a part of the views
    r.set_camera_projection([p[0] for p in mixed_b], [p[1] if p[1] is not None else 0.001 for p in mixed_b])
    r.set_camera_projection(np.full(10, 33.0, np.float32), first_view=100)
    want = [(p[0], p[1] if p[1] is not None else 0.001) for p in mixed_b]
    want[100:110] = [(33.0, 0.001)] * 10                # (znear None: the mode's default again)
    r.step()
    _check(r, base, projections=want)
    # bad values change nothing
    for bad in (dict(vfov=0.0), dict(vfov=180.0), dict(vfov=float("nan")), dict(vfov=60.0, znear=-1.0),
                dict(vfov=60.0, znear=0.0), dict(vfov=[60.0] * (n + 1)), dict(vfov=60.0, first_view=n + 1)):
        with pytest.raises(ValueError):
            r.set_camera_projection(**bad)
    f2, z2 = r.camera_projection()
    assert f2.tolist() == [np.float32(a) for a, _ in want] and z2.tolist() == [np.float32(b) for _, b in want]


def test_set_camera_projection_is_stream_ordered(native):
    import torch
    base = scenes.synthetic_scene(512)
    n = len(base.cameras)
    old, new = po.mixed(n), po.mixed(n, fovs=(45.0, 135.0), znears=(None, 2.0, 3.5))
    r = _make(_with(base, old))
    s = torch.cuda.Stream()
    r.set_stream(s.cuda_stream)
    with torch.cuda.stream(s):
        r.step()                                          # A
        r.set_camera_projection([p[0] for p in new], [p[1] or 0.001 for p in new])
        a_rgb = r.rgb_tensor().to_torch().clone()
        a_ids = r.visibility_tensor().to_torch().clone()
        r.step()                                          # B
        b_rgb = r.rgb_tensor().to_torch().clone()
        b_ids = r.visibility_tensor().to_torch().clone()
    s.synchronize()
    ref_a = po.render(base, old, want_ids=True)
    ref_b = po.render(base, [(f, z or 0.001) for f, z in new], want_ids=True)
    assert np.array_equal(a_ids.cpu().numpy(), ref_a["tri_id"]) and np.array_equal(a_rgb.cpu().numpy(), ref_a["rgb"])
    assert np.array_equal(b_ids.cpu().numpy(), ref_b["tri_id"]) and np.array_equal(b_rgb.cpu().numpy(), ref_b["rgb"])


def test_two_shards_split_the_whole_job_view_range(native):
    base = scenes.synthetic_scene(301)
    n = len(base.cameras)
    projs = po.mixed(n)
    desc = _with(base, projs)
    r = _make(desc, device_ids=[0, 0])
    assert r.num_shards == 2
    f, z = r.camera_projection()
    assert f.tolist() == [np.float32(a) for a, _ in projs]
    new = list(projs)
    new[140:170] = [(20.0, 2.0)] * 30                     # across the shard boundary (151)
    r.set_camera_projection(np.full(30, 20.0, np.float32), 2.0, first_view=140)
    r.step()
    r.sync()
    ref = po.render(base, [(a, b) for a, b in new], want_ids=True)
    for sh in range(2):
        lo, hi = r.shard_first_world(sh), r.shard_first_world(sh + 1)
        ids = r.visibility_tensor(shard=sh).to_torch().cpu().numpy()
        rgb = r.rgb_tensor(shard=sh).to_torch().cpu().numpy()
        assert np.array_equal(ids, ref["tri_id"][lo:hi]) and np.array_equal(rgb, ref["rgb"][lo:hi])


def test_headless_vfov(native, tmp_path):
    from madrona_renderer_amd import build
    exe = build.headless_path()
    args = ["16", "2", "rast", "64", "64"]
    ok = subprocess.run(["timeout", "-k", "5", "120", exe] + args + ["--vfov", "60", "--znear", "0.5"], cwd=tmp_path,
                        capture_output=True, text=True)
    assert ok.returncode == 0, ok.stderr
    for bad in (["--vfov", "0"], ["--vfov", "180"], ["--znear", "-1"], ["--vfov", "abc"], ["--znear", "0"]):
        p = subprocess.run(["timeout", "-k", "5", "120", exe] + args + bad, cwd=tmp_path, capture_output=True, text=True)
        assert p.returncode not in (0, 124, 137) and ("--vfov" in p.stderr or "--znear" in p.stderr), (bad, p.stderr)
    p = subprocess.run(["timeout", "-k", "5", "120", exe, "16", "2", "rt", "64", "64", "--znear", "1000"], cwd=tmp_path,
                       capture_output=True, text=True)
    assert p.returncode not in (0, 124, 137)
