"""The point-cloud output on the MI355X (-m gpu).

The compaction stage against tests/cloud_oracle.cloud applied to the renderer's own depth, camera columns and
camera_projection() on every bit of all three outputs: through the raster kernels and the BVH tile kernel, both modes,
s = 1, 2, 3, both frames, a forced split, a far crop that empties views.  The oracle-free check against
position_tensor(), hand-built masks written into depth_tensor(), every other output against a twin without the stage, a
pose write, two shards, the refusals, the zero-copy tensors and the yardstick."""
import dataclasses
import os
import statistics

import numpy as np
import pytest

from madrona_renderer_amd import scenes
from tests import cloud_oracle as co
from tests import meshes
from tests import position_oracle as pos
from tests.test_cloud_cpu import depth_of, hand_built_masks
from tests.test_projection_gpu import _make
from tests.test_supersample_gpu import _scene

pytestmark = pytest.mark.gpu

# the yardstick's bound: compact() took 20.48 us against 17.66 us for unproject() on one MI355X, ratio 1.16
# (profiles/cloud_latest.txt); times 1.5, rounded up
YARDSTICK_RATIO = 2.0

F = np.float32


def _np(t):
    return t.to_torch().cpu().numpy()


def _t(x):
    return x.cpu().numpy()


def _depth(r, **kw):
    d = _np(r.depth_tensor(**kw))
    return d.reshape(d.shape[:3])


def _expected(r, desc, s, frame, rt, n, max_depth=None):
    """tests/cloud_oracle.cloud of what the renderer holds NOW: its depth, its camera tensors, its projections"""
    f, z = r.camera_projection()
    consts = pos.constants(desc.width, desc.height, rt, list(zip(f.tolist(), z.tolist())), s)
    return co.cloud(_depth(r), _np(r.camera_position_tensor()), _np(r.camera_rotation_tensor()), consts, s, frame, rt, n,
                    max_depth)


def _got(c, **kw):
    return _t(c.points_tensor(**kw)), _t(c.pixel_tensor(**kw)), _t(c.count_tensor(**kw))


def _assert_same(got, want, what):
    for g, w, name in zip(got, want, ("points", "pixel", "count")):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        bad = int((g.view(np.uint32) != w.view(np.uint32)).sum())
        assert bad == 0, f"{what}: {bad} of {g.size} values of {name} differ in their bits"


def _attach(r, n, frame="world", max_depth=None, parts=None):
    """cloud.attach under MRX_CLOUD_PARTS (read at that call), which is gone again after"""
    from madrona_renderer_amd import cloud
    old = os.environ.get("MRX_CLOUD_PARTS")
    if parts is not None:
        os.environ["MRX_CLOUD_PARTS"] = str(parts)
    try:
        return cloud.attach(r, n, frame=frame, max_depth=max_depth)
    finally:
        if old is None:
            os.environ.pop("MRX_CLOUD_PARTS", None)
        else:
            os.environ["MRX_CLOUD_PARTS"] = old


CASES = {
    # name: (builder, raytracer, s, frame, N, max_depth, forced parts)
    "raster-64x64-256": (lambda: scenes.synthetic_scene(4, with_wall=True, textured=True), False, 1, "world", 256, None, None),
    "raster-64x64-5000": (lambda: scenes.synthetic_scene(4, with_wall=True, textured=True), False, 1, "world", 5000, None, None),
    "raster-5x3-s3-1": (lambda: _scene("Rasterizer", 5, 3, worlds=3), False, 3, "world", 1, None, None),
    "raster-5x3-s3-7": (lambda: _scene("Rasterizer", 5, 3, worlds=3), False, 3, "view", 7, None, None),
    "raster-5x3-s3-16": (lambda: _scene("Rasterizer", 5, 3, worlds=3), False, 3, "world", 16, None, None),
    "rt-40-s2-view": (lambda: _scene("Raytracer", 40, 40, worlds=3), True, 2, "view", 300, None, None),
    "bvh-40x24-parts3": (lambda: meshes.cube_field(num_worlds=3, cubes=40, width=40, height=24), False, 1, "world", 200,
                         None, 3),
}


@pytest.mark.parametrize("case", list(CASES))
def test_the_stage_is_the_oracle_s_on_the_renderer_s_own_depth(native, case):
    build, rt, s, frame, n, max_depth, parts = CASES[case]
    base = dataclasses.replace(build(), supersample=s)
    r = _make(base, visibility=False)
    if case.startswith("bvh"):
        assert r.bvh_launch()["kernel"] != "none"
    before = r.bytes_per_step()
    c = _attach(r, n, frame, max_depth, parts)
    assert (c.points, c.frame, c.max_depth) == (n, frame, max_depth)
    views = base.num_views
    nslow, nfast = (base.width, base.width) if rt else (base.height, base.width)
    assert tuple(c.points_tensor().shape) == (views, n, 4) and tuple(c.pixel_tensor().shape) == (views, n)
    assert tuple(c.count_tensor().shape) == (views,)
    assert r.bytes_per_step() == before + views * nslow * nfast * 4 + views * (n * 20 + 4)
    r.sync()
    _assert_same(_got(c), _expected(r, base, s, frame, rt, n, max_depth), case + " at attach")    # it ran once
    r.step()
    r.sync()
    got = _got(c)
    _assert_same(got, _expected(r, base, s, frame, rt, n, max_depth), case + " after a step")
    depth = _depth(r)
    assert (depth > 0).any() and (got[2] > 0).any()


def test_a_far_crop_that_leaves_some_views_nothing(native):
    import torch
    base = scenes.synthetic_scene(4, with_wall=True, textured=True)
    far = 30.0
    r = _make(base, visibility=False)
    c = _attach(r, 300, "world", far)
    r.sync()
    t = r.depth_tensor().to_torch()
    t[:2] = torch.where(t[:2] > 0, t[:2] + 2.0 * far, t[:2])       # views 0 and 1: nothing within the crop
    t[2:] = torch.where(t[2:] > 0, t[2:].clamp(max=far - 1.0), t[2:])       # views 2 and 3: everything
    c.compact()
    r.sync()
    got = _got(c)
    _assert_same(got, _expected(r, base, 1, "world", False, 300, far), "far crop")
    assert (got[2][:2] == 0).all() and (got[2][2:] > 0).all()
    assert (got[1][:2] == -1).all() and (got[0][:2].view(np.uint32) == 0).all()


def test_the_points_are_the_position_tensor_s_at_their_pixels(native):
    """oracle-free: on a renderer created with positions="world", points[v, k] == position_tensor() at pixel[v, k]"""
    for builder, rt, s in ((lambda: scenes.synthetic_scene(4, with_wall=True, textured=True), False, 1),
                           (lambda: _scene("Raytracer", 40, 40, worlds=3), True, 2)):
        base = dataclasses.replace(builder(), supersample=s, positions="world")
        r = _make(base, visibility=False)
        c = _attach(r, 777)
        r.step()
        r.sync()
        points, pixel, count = _got(c)
        position = _np(r.position_tensor())                 # [views, slow, fast, 4]
        views, nslow, nfast = position.shape[:3]
        width = nslow if rt else nfast
        filled = pixel >= 0
        assert filled.any() and np.array_equal(filled.sum(axis=1), np.minimum(count, 777))
        for v in range(views):
            p = pixel[v][filled[v]].astype(np.int64)
            y, x = p // width, p % width
            at = position[v, x, y] if rt else position[v, y, x]
            assert np.array_equal(points[v][filled[v]].view(np.uint32), at.view(np.uint32)), v
            assert (at[:, 3] == 1).all()


@pytest.mark.parametrize("w,h,rt,n,parts", [(64, 64, False, 256, None), (40, 24, False, 100, 3), (40, 40, True, 1024, None),
                                            (150, 64, False, 4096, None), (150, 64, False, 4096, 7)])
def test_hand_built_masks_written_into_the_depth_tensor(native, w, h, rt, n, parts):
    """the only way to pin M = N - 1, N, N + 1 and the lane-0 / lane-63 segments on the device; 150 x 64 is three spans"""
    import torch
    nslow, nfast = (w, w) if rt else (h, w)
    masks = hand_built_masks(nslow, nfast, n, parts or 1)
    base = _scene("Raytracer" if rt else "Rasterizer", w, h, worlds=len(masks))
    names = [list(masks)[v % len(masks)] for v in range(base.num_views)]
    r = _make(base, visibility=False)
    c = _attach(r, n, "world", None, parts)
    r.sync()
    rng = np.random.default_rng(w + h + n)
    depth = np.stack([depth_of(masks[k], rng) for k in names])
    t = r.depth_tensor().to_torch()
    t.copy_(torch.from_numpy(depth).reshape(tuple(t.shape)).to(t.device))
    c.compact()
    r.sync()
    got = _got(c)
    _assert_same(got, _expected(r, base, 1, "world", rt, n), (w, h, rt, n, parts, names))
    for i, k in enumerate(names):
        assert int(got[2][i]) == int(masks[k].sum()), k


def test_every_other_output_is_the_twin_s(native):
    import torch
    base = dataclasses.replace(scenes.synthetic_scene(4, with_wall=True, textured=True), supersample=2, normals=True,
                               positions="view")
    r, twin = _make(base, visibility=True), _make(base, visibility=True)
    _attach(r, 512, "view", 25.0)
    for x in (r, twin):
        x.step()
        x.sync()
    for getter in ("rgb_tensor", "depth_tensor", "visibility_tensor", "normal_tensor", "position_tensor"):
        a, b = getattr(r, getter)().to_torch(), getattr(twin, getter)().to_torch()
        assert a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), getter


def test_a_pose_write_and_a_step_move_the_points(native):
    import torch
    base = scenes.synthetic_scene(4, with_wall=True, textured=True)
    r = _make(base, visibility=False)
    c = _attach(r, 256)
    r.sync()
    first = _got(c)
    cp = r.camera_position_tensor().to_torch()
    cp.add_(torch.tensor([0.5, -0.25, 0.125], device=cp.device))
    r.step()
    r.sync()
    moved = _got(c)
    _assert_same(moved, _expected(r, base, 1, "world", False, 256), "after the pose write")
    assert (moved[0] != first[0]).any()


def test_two_shards_on_one_device(native):
    import torch
    base = dataclasses.replace(_scene("Rasterizer", 40, 24, worlds=5), supersample=2)
    one = _make(base, visibility=False)
    two = _make(base, visibility=False, device_ids=[0, 0])
    assert two.num_shards == 2
    ca, cb = _attach(one, 128, "world", 40.0), _attach(two, 128, "world", 40.0)
    for x in (one, two):
        for i in range(x.num_shards):
            cp = x.camera_position_tensor(shard=i).to_torch()
            cp.add_(torch.tensor([0.5, -0.25, 0.125], device=cp.device))
        x.step()
        x.sync()
    for getter in ("points_tensor", "pixel_tensor", "count_tensor"):
        whole = getattr(ca, getter)()
        parts = torch.cat([getattr(cb, getter)(shard=i) for i in range(2)])
        assert whole.shape == parts.shape and torch.equal(whole.view(torch.int32), parts.view(torch.int32)), getter
        with pytest.raises(ValueError, match="say which shard"):
            getattr(cb, getter)()
    assert (ca.count_tensor() > 0).any()
    # compact() reaches every shard: scribble over shard 1's points, compact(), the same tensors again
    cb.points_tensor(shard=1).fill_(7.0)
    cb.compact()
    two.sync()
    parts = torch.cat([cb.points_tensor(shard=i) for i in range(2)])
    assert torch.equal(ca.points_tensor().view(torch.int32), parts.view(torch.int32))


def test_refusals(native):
    from madrona_renderer_amd import cloud
    base = _scene("Rasterizer", 40, 24, worlds=3)
    r = _make(base, visibility=False)
    cloud.attach(r, 64)
    with pytest.raises(RuntimeError, match="already has the point-cloud output"):
        cloud.attach(r, 64)
    rgb_only = _make(base, visibility=False, outputs="RGB")
    with pytest.raises(RuntimeError, match="needs depth"):
        cloud.attach(rgb_only, 64)
    # the refused renderer works on, and a renderer without the stage says so
    rgb_only.step()
    rgb_only.sync()
    lib = cloud._capi()
    plain = _make(base, visibility=False)
    assert lib.mrx_cloud(plain.native_handle()) == 0 and lib.mrx_cloud(r.native_handle()) == 64
    assert lib.mrx_compact(plain.native_handle()) == -5                     # MRX_E_UNSUPPORTED
    assert b"mrx_cloud_create was not called" in lib.mrx_last_error()


def test_the_tensors_are_the_renderer_s_memory(native):
    """zero-copy: data_ptr() is the C-ABI pointer, and a write through the tensor is seen by compact()"""
    import ctypes
    from madrona_renderer_amd import cloud
    base = scenes.synthetic_scene(4, with_wall=True, textured=True)
    r = _make(base, visibility=False)
    c = cloud.attach(r, 256)
    r.sync()
    lib = cloud._capi()
    for which, getter in ((23, c.points_tensor), (24, c.pixel_tensor), (25, c.count_tensor)):
        dims = (ctypes.c_int64 * 4)()
        nd, dt, dev = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        ptr = lib.mrx_buffer(r.native_handle(), which, dims, ctypes.byref(nd), ctypes.byref(dt), ctypes.byref(dev))
        t = getter()
        assert ptr and t.data_ptr() == ptr and t.is_cuda and t.device.index == dev.value
        assert tuple(t.shape) == tuple(dims[:nd.value])
    want = _got(c)
    # writes through the tensors: compact() overwrites every slot and every count with the same values again
    c.points_tensor().fill_(3.0)
    c.pixel_tensor().fill_(12345)
    c.count_tensor().fill_(-9)
    r.sync()
    assert (_t(c.points_tensor()) == 3.0).all() and (_t(c.count_tensor()) == -9).all()      # the same memory on re-export
    c.compact()
    r.sync()
    _assert_same(_got(c), want, "after scribbling over the outputs")
    # the tensor outlives the names that made it
    t = c.points_tensor()
    del c, r
    import gc
    gc.collect()
    assert np.array_equal(_t(t).view(np.uint32), want[0].view(np.uint32))


def test_yardstick_the_compaction_against_the_unprojection(native):
    """1024 views of 64 x 64, N = 1024: one compact() (4 bytes read per pixel, 20 written per slot) against one
    unproject() (20 bytes per pixel) on the same renderer, same stream, mark / elapsed_ms around each, the median of 20
    taken in turns after a warm-up.  Measured 20.48 us against 17.66 us, ratio 1.16 (profiles/cloud_latest.txt,
    DESIGN.md 4.24); the bound is that ratio times 1.5, rounded up: 2."""
    r = _make(dataclasses.replace(scenes.synthetic_scene(1024), positions="world"), visibility=False)
    c = _attach(r, 1024)
    assert tuple(c.points_tensor().shape) == (1024, 1024, 4)
    r.sync()

    def timed(fn):
        r.mark(0)
        fn()
        r.mark(1)
        return r.elapsed_ms() * 1000.0

    for fn in (c.compact, r.unproject):
        for _ in range(5):
            timed(fn)                                       # warm-up
    cloud_us, unproject_us = [], []
    for _ in range(20):                                     # alternating, so that a clock change hits both
        cloud_us.append(timed(c.compact))
        unproject_us.append(timed(r.unproject))
    f, u = statistics.median(cloud_us), statistics.median(unproject_us)
    print(f"compact {f:.2f} us, unproject {u:.2f} us, ratio {f / u:.2f} (1024 x 64x64, N = 1024)")
    assert f <= YARDSTICK_RATIO * u, (f, u)
