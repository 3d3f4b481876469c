"""Supersampling on the MI355X (-m gpu).

The resolve kernel alone: the sample tensors filled with seeded random bytes and bit patterns, resolve(), compared bit
for bit with tests/supersample_oracle.resolve for s = 2, 3, 4 at native sizes with row tails, unaligned pitches, the
aligned path and several workgroups, in both modes.  The whole renderer against the oracle's render of the sample image
resolved (rgb, ids, normals, labels bit-exact, depth within 1 ulp: tests/util.assert_parity) through the raster
kernels, the BVH tile kernel and the flat kernel, in both modes, under every output selection, with projections
changed and a pose written between steps.  The sample tensors against a plain renderer of the sample size, two shards
against one, factor 1 against no argument, and the yardstick: one resolve takes no longer than device-to-device copies
of the tensors it reads."""
import dataclasses
import statistics

import numpy as np
import pytest

from madrona_renderer_amd import scenes
from tests import label_oracle as lb
from tests import meshes
from tests import normal_oracle as no
from tests import projection_oracle as po
from tests import supersample_oracle as so
from tests.test_projection_gpu import _make
from tests.util import assert_parity, fetch

pytestmark = pytest.mark.gpu

SIZES = [(5, 3), (7, 5), (6, 6), (12, 8), (40, 24)]


def _ss(desc, s, **kw):
    return dataclasses.replace(desc, supersample=s, **kw)


def _scene(mode, w, h, worlds=4):
    if mode == "Raytracer":
        h = w                                               # (Raytracer mode: the width only, square views)
    return scenes.synthetic_scene(worlds, width=w, height=h, with_wall=True, textured=True, render_mode=mode)


def _np(t):
    return t.to_torch().cpu().numpy()


@pytest.mark.parametrize("mode", ["Rasterizer", "Raytracer"])
@pytest.mark.parametrize("s", [2, 3, 4])
def test_the_resolve_kernel_is_exact_on_random_samples(native, s, mode):
    import torch
    rng = np.random.default_rng(1000 * s + (mode == "Raytracer"))
    for w, h in SIZES:
        desc = _ss(_scene(mode, w, h, worlds=3), s, normals=True, instance_labels=True)
        r = _make(desc, visibility=False)
        assert r.supersample == s
        nfast, nslow = (w, w) if mode == "Raytracer" else (w, h)
        names = {"rgb": np.uint8, "normal": np.uint8, "depth": np.uint32, "segmask": np.uint32}
        filled = {}
        for name, dt in names.items():
            t = r.sample_tensor(name).to_torch()
            lead = (3, s * nslow, s * nfast)
            assert tuple(t.shape)[:3] == lead, (name, tuple(t.shape))
            if dt == np.uint8:
                a = rng.integers(0, 256, lead + (4,), dtype=np.uint8)
                t.copy_(torch.from_numpy(a).to(t.device))
            else:
                a = rng.integers(0, 2 ** 32, lead, dtype=np.uint64).astype(np.uint32)
                t.view(torch.int32).reshape(lead).copy_(torch.from_numpy(a.view(np.int32)).to(t.device))
            filled[name] = a
        r.resolve()
        r.sync()
        want = so.resolve(filled, s)
        got = {"rgb": _np(r.rgb_tensor()), "normal": _np(r.normal_tensor()),
               "depth": _np(r.depth_tensor()).reshape(3, nslow, nfast).view(np.uint32),
               "segmask": _np(r.segmask_tensor()).view(np.uint32)}
        for name in names:
            assert got[name].shape == want[name].shape, (w, h, name, got[name].shape)
            bad = int((got[name] != want[name]).sum())
            assert bad == 0, f"{w}x{h} s={s} {name}: {bad} values differ"
        # the samples are as written: the resolve reads, it does not write them
        assert np.array_equal(_np(r.sample_tensor("rgb")), filled["rgb"])


def _reference(desc, s, projections=None, normals=False, labels=False, mutate=None):
    """The oracle's render of the sample image of `desc`, resolved: rgb, depth, tri_id, segmask (+ normal)."""
    from oracle import oracle
    d = so.sample_desc(desc, s)
    fs = oracle.FlatScene(d)
    if mutate:
        mutate(fs)
    ref = po.render(d, projections, 0, d.num_views, want_ids=True) if projections is not None else fs.render()
    ref = {k: v for k, v in ref.items() if isinstance(v, np.ndarray)}
    if normals:
        ref["normal"] = no.normals(fs, ref["tri_id"])
    if labels:
        ref["segmask"] = lb.segmask(fs, lb.expand(d), ref["tri_id"])
    return so.resolve(ref, s)


PARITY = {
    # name: (builder, variant, raster entry, bvh kernel, raytracer, s)
    "raster-40x24": (lambda: _scene("Rasterizer", 40, 24), None, None, "none", False, 2),
    "raster-64x64": (lambda: _scene("Rasterizer", 64, 64), None, None, "none", False, 2),
    "raster-rt-40": (lambda: _scene("Raytracer", 40, 40), None, None, "none", True, 2),
    "raster-40x24-s3": (lambda: _scene("Rasterizer", 40, 24), None, None, "none", False, 3),
    "raster-rt-24-s4": (lambda: _scene("Raytracer", 24, 24), None, None, "none", True, 4),
    "bvh-tile-40x24": (lambda: meshes.cube_field(num_worlds=3, cubes=40, width=40, height=24), None, "bvh", "tile", False, 2),
    "bvh-tile-rt-64": (lambda: meshes.cube_field(num_worlds=3, cubes=40, width=64, height=64, mode="Raytracer",
                                                 textured=True), None, "bvh", "tile", True, 2),
    "flat-rt-40": (lambda: _scene("Raytracer", 40, 40), 2, "bvh", "flat", True, 2),
    "flat-64x64": (lambda: _scene("Rasterizer", 64, 64), 2, "bvh", "flat", False, 2),
}


@pytest.mark.parametrize("case", list(PARITY))
def test_the_resolved_images_match_the_oracle_resolved(native, oracle_mod, case):
    build, variant, entry, bvh, rt, s = PARITY[case]
    base = build()
    r = _make(_ss(base, s), visibility=not rt, variant=variant)
    if entry is not None:
        assert r.raster_entry() == entry
    assert r.bvh_launch()["kernel"] == bvh
    ref = _reference(base, s)
    got = fetch(r, visibility=not rt, raytracer=rt)
    assert got["rgb"].shape == (base.num_views,) + ((base.width, base.width) if rt else (base.height, base.width)) + (4,)
    assert_parity(got, {k: ref[k] for k in got})
    assert (got["rgb"][..., 3] == 255).all()
    # not vacuous: the filter decides pixels -- the native render of the same views differs
    native_ref = oracle_mod.FlatScene(base).render()
    assert (native_ref["rgb"] != ref["rgb"]).any(axis=-1).mean() > 0.01
    # the sample tensors are the outputs of a plain renderer of the sample size, bit for bit
    import torch
    plain = _make(so.sample_desc(base, s), visibility=not rt, variant=variant)
    plain.sync()
    assert plain.raster_entry() == r.raster_entry() and plain.bvh_launch() == r.bvh_launch()
    assert torch.equal(r.sample_tensor("rgb").to_torch(), plain.rgb_tensor().to_torch())
    assert torch.equal(r.sample_tensor("depth").to_torch().view(torch.int32),
                       plain.depth_tensor().to_torch().view(torch.int32))
    if rt:
        assert torch.equal(r.sample_tensor("segmask").to_torch(), plain.segmask_tensor().to_torch())
    else:
        assert torch.equal(r.sample_tensor("visibility").to_torch(), plain.visibility_tensor().to_torch())


@pytest.mark.parametrize("mode", ["Rasterizer", "Raytracer"])
@pytest.mark.parametrize("outputs", ["RGBD", "Depth", "RGB"])
def test_output_selections_resolve_what_they_render(native, oracle_mod, outputs, mode):
    rt = mode == "Raytracer"
    base = _scene(mode, 40, 24, worlds=3)
    r = _make(_ss(base, 2), visibility=False, outputs=outputs)
    ref = _reference(base, 2)
    r.sync()
    if outputs != "Depth":
        assert int((_np(r.rgb_tensor()) != ref["rgb"]).any(axis=-1).sum()) == 0
    else:
        for call in (r.rgb_tensor, lambda: r.sample_tensor("rgb")):
            with pytest.raises(RuntimeError):
                call()
    if outputs != "RGB":
        d = _np(r.depth_tensor())
        got = {"rgb": ref["rgb"], "depth": d.reshape(d.shape[:3])}
        assert_parity(got, {"rgb": ref["rgb"], "depth": ref["depth"]})
    else:
        for call in (r.depth_tensor, lambda: r.sample_tensor("depth")):
            with pytest.raises(RuntimeError):
                call()
    if rt:
        assert np.array_equal(_np(r.segmask_tensor()), ref["segmask"])
    else:
        with pytest.raises(RuntimeError):
            r.sample_tensor("segmask")


@pytest.mark.parametrize("mode", ["Rasterizer", "Raytracer"])
def test_normals_and_labels_take_the_same_sample_as_depth(native, oracle_mod, mode):
    rt = mode == "Raytracer"
    base = _scene(mode, 40, 24, worlds=5)
    base.normals = True
    base.instance_labels = lb.mixed(len(base.instances))
    r = _make(_ss(base, 2), visibility=False)
    ref = _reference(base, 2, normals=True, labels=True)
    r.sync()
    got = {"rgb": _np(r.rgb_tensor()), "depth": _np(r.depth_tensor()).reshape(ref["depth"].shape),
           "segmask": _np(r.segmask_tensor())}
    assert_parity(got, {k: ref[k] for k in got})
    normal = _np(r.normal_tensor())
    assert int((normal != ref["normal"]).any(axis=-1).sum()) == 0
    # one sample for all three: background depth <=> label -1 <=> normal alpha 0
    miss = got["depth"] == 0
    assert miss.any() and (~miss).any()
    assert np.array_equal(miss, normal[..., 3] == 0) and (got["segmask"][miss] == -1).all()
    assert len(np.unique(got["segmask"])) >= 3


def test_projections_changed_between_two_steps(native, oracle_mod):
    base = _scene("Rasterizer", 40, 24, worlds=5)
    r = _make(_ss(base, 2), visibility=True)
    assert_parity(fetch(r), {k: v for k, v in _reference(base, 2).items() if k != "segmask"})
    projections = [(f, 0.001 if z is None else z) for f, z in po.mixed(base.num_views)]
    r.set_camera_projection([f for f, _ in projections], [z for _, z in projections])
    r.step()
    f, z = r.camera_projection()                            # the caller's terms
    assert f.tolist() == [np.float32(a) for a, _ in projections]
    ref = _reference(base, 2, projections=projections)
    got = fetch(r)
    assert_parity(got, {k: ref[k] for k in got})
    assert (ref["tri_id"] != _reference(base, 2)["tri_id"]).any()


def test_a_pose_written_between_two_steps_that_are_not_synchronised(native, oracle_mod):
    import torch
    base = _scene("Rasterizer", 40, 24, worlds=4)
    r = _make(_ss(base, 2), visibility=True)
    pos = r.instance_position_tensor().to_torch()
    moved = pos.clone()
    moved[1::3, 2] += 1.5                                   # every world's cube, up
    r.step()
    pos.copy_(moved)
    r.step()
    want = moved.cpu().numpy()

    def mutate(fs):
        fs.inst_pos[:] = want

    ref = _reference(base, 2, mutate=mutate)
    got = fetch(r)
    assert_parity(got, {k: ref[k] for k in got})
    assert (ref["tri_id"] != _reference(base, 2)["tri_id"]).any()
    del torch


def test_two_shards_on_one_device_resolve_their_own_slabs(native, oracle_mod):
    import torch
    base = _scene("Rasterizer", 40, 24, worlds=5)
    one = _make(_ss(base, 2), visibility=True)
    two = _make(_ss(base, 2), visibility=True, device_ids=[0, 0])
    assert two.num_shards == 2 and two.supersample == 2
    two.step()
    one.step()
    one.sync()
    two.sync()
    for getter in ("rgb_tensor", "depth_tensor", "visibility_tensor"):
        whole = getattr(one, getter)().to_torch()
        parts = torch.cat([getattr(two, getter)(shard=i).to_torch() for i in range(2)])
        assert whole.shape == parts.shape and torch.equal(whole.view(torch.uint8), parts.view(torch.uint8)), getter
    samples = torch.cat([two.sample_tensor("rgb", shard=i).to_torch() for i in range(2)])
    assert torch.equal(samples, one.sample_tensor("rgb").to_torch())
    with pytest.raises(ValueError):
        two.sample_tensor("rgb")                            # several shards: say which
    ref = _reference(base, 2)
    got = fetch(one)
    assert_parity(got, {k: ref[k] for k in got})
    # resolve() alone reaches every shard: scribble over shard 1's native rgb, resolve, and it is back
    t = two.rgb_tensor(shard=1).to_torch()
    keep = t.clone()
    t.zero_()
    two.resolve()
    two.sync()
    assert torch.equal(t, keep)


def test_factor_1_is_the_renderer_without_the_argument(native):
    import torch
    base = _scene("Raytracer", 40, 40, worlds=3)
    a = _make(base, visibility=False)
    b = _make(_ss(base, 1), visibility=False)
    assert a.supersample == b.supersample == 1
    a.sync()
    b.sync()
    assert a.raster_entry() == b.raster_entry() and a.bytes_per_step() == b.bytes_per_step()
    for getter in ("rgb_tensor", "depth_tensor", "segmask_tensor"):
        x, y = getattr(a, getter)().to_torch(), getattr(b, getter)().to_torch()
        assert x.shape == y.shape and torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    for r in (a, b):
        with pytest.raises(RuntimeError, match="without supersampling"):
            r.sample_tensor("rgb")
        with pytest.raises(RuntimeError, match="without supersampling"):
            r.resolve()
    # ... and a supersampled renderer's bytes: the sample render's plus what the resolve reads and writes
    c = _make(_ss(base, 2), visibility=False)
    plain = _make(so.sample_desc(base, 2), visibility=False)
    px = base.num_views * 40 * 40
    assert c.bytes_per_step() == plain.bytes_per_step() + px * ((16 + 4) + 2 * 8)


def test_yardstick_one_resolve_takes_no_longer_than_copying_what_it_reads(native):
    """1024 views of native 64x64 at s = 2, RGBD: the resolve reads the rgb samples once (16 MiB), the lines of every
    second depth row, and writes two 4 MiB tensors; device-to-device copies of the rgb and depth sample tensors move
    twice their 32 MiB.  Same process, same stream, events around batches of 10, the median of 9 batches each.  A
    resolve slower than the copies is not streaming."""
    import torch
    r = _make(_ss(scenes.synthetic_scene(1024), 2), visibility=False)
    rgb, depth = r.sample_tensor("rgb").to_torch(), r.sample_tensor("depth").to_torch()
    assert tuple(rgb.shape) == (1024, 128, 128, 4) and tuple(depth.shape) == (1024, 128, 128, 1)
    rgb2, depth2 = torch.empty_like(rgb), torch.empty_like(depth)
    r.sync()

    def copies():
        rgb2.copy_(rgb)
        depth2.copy_(depth)

    def timed(fn, batch=10):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(batch):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / batch

    for fn in (r.resolve, copies):
        timed(fn, 20)                                       # warm-up
    res, cop = [], []
    for _ in range(9):                                      # alternating, so that a clock change hits both
        res.append(timed(r.resolve))
        cop.append(timed(copies))
    res_us, cop_us = statistics.median(res), statistics.median(cop)
    print(f"resolve {res_us:.2f} us, copies {cop_us:.2f} us (1024 x 64x64, s = 2, RGBD)")
    assert res_us <= cop_us, (res_us, cop_us)
