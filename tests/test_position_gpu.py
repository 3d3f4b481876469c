"""The position output on the MI355X (-m gpu).

The unprojection kernel alone: the depth tensor filled with seeded values (a quarter exact zeros), random unit
quaternions and positions in the camera tensors, distinct per-view projections, unproject(), compared bit for bit with
tests/position_oracle.unproject for both frames, both modes and s = 1, 2, 3 at sizes with views smaller than a wave,
view boundaries inside a wave and several workgroups; once more on a one-CU grid, where the grid-stride loop runs.  The
whole renderer through the raster kernels, the BVH tile kernel and the flat kernel: positions bit-exact against the
reference applied to the renderer's own depth, every other output bit for bit that of a renderer without the option.
Pose and projection are read when the stage runs, two shards equal one, the option off is the renderer without the
argument, the yardstick (one unproject takes no longer than a device-to-device copy of its output), and the headless
tool's point cloud."""
import dataclasses
import os
import statistics
import subprocess

import numpy as np
import pytest

from madrona_renderer_amd import scenes
from tests import position_oracle as pos
from tests import projection_oracle as po
from tests.test_projection_gpu import _make
from tests.test_supersample_gpu import PARITY, SIZES, _scene

pytestmark = pytest.mark.gpu

FOVS = (35.0, 90.0, 128.0, 61.5, 147.0)


def _np(t):
    return t.to_torch().cpu().numpy()


def _depth(r):
    d = _np(r.depth_tensor())
    return d.reshape(d.shape[:3])


def _reference(r, desc, s, frame, rt):
    """tests/position_oracle.unproject of what the renderer holds NOW: its depth, its camera tensors, its projections"""
    f, z = r.camera_projection()
    consts = pos.constants(desc.width, desc.height, rt, list(zip(f.tolist(), z.tolist())), s)
    return pos.unproject(_depth(r), _np(r.camera_position_tensor()), _np(r.camera_rotation_tensor()), consts, s, frame, rt)


def _assert_bits(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape)
    bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    assert bad == 0, f"{what}: {bad} of {got.size} values differ in their bits"


def _fill(r, rng, views):
    """seeded depth (a quarter zeros), unit quaternions, positions and distinct projections; returns the depth written"""
    import torch
    t = r.depth_tensor().to_torch()
    d = rng.uniform(0.05, 500.0, tuple(t.shape)).astype(np.float32)
    d[rng.random(d.shape) < 0.25] = 0.0
    t.copy_(torch.from_numpy(d).to(t.device))
    q = rng.normal(size=(views, 4))
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    c = rng.uniform(-40.0, 40.0, (views, 3)).astype(np.float32)
    rot, cp = r.camera_rotation_tensor().to_torch(), r.camera_position_tensor().to_torch()
    assert tuple(rot.shape) == (views, 4) and tuple(cp.shape) == (views, 3)
    rot.copy_(torch.from_numpy(q).to(rot.device))
    cp.copy_(torch.from_numpy(c).to(cp.device))
    r.set_camera_projection([FOVS[v % len(FOVS)] + 0.25 * v for v in range(views)])
    return d


def _kernel_alone(desc, s, frame, rng):
    rt = desc.render_mode == "Raytracer"
    views = desc.num_views
    r = _make(dataclasses.replace(desc, supersample=s, positions=frame), visibility=False)
    assert r.positions == frame and r.supersample == s
    nslow, nfast = (desc.width, desc.width) if rt else (desc.height, desc.width)
    assert tuple(r.position_tensor().shape) == (views, nslow, nfast, 4)
    r.sync()
    written = _fill(r, rng, views)
    r.unproject()
    r.sync()
    got = _np(r.position_tensor())
    _assert_bits(got, _reference(r, desc, s, frame, rt), f"{desc.width}x{desc.height} s={s} {frame}")
    assert np.array_equal(_np(r.depth_tensor()).view(np.uint32), written.view(np.uint32))    # depth is read, not written
    hit = written.reshape(got.shape[:3]) != 0
    assert hit.any() and (~hit).any() and np.array_equal(got[..., 3], hit.astype(np.float32))
    return got


@pytest.mark.parametrize("mode", ["Rasterizer", "Raytracer"])
@pytest.mark.parametrize("frame", ["world", "view"])
@pytest.mark.parametrize("s", [1, 2, 3])
def test_the_unproject_kernel_is_exact_on_random_depth(native, s, frame, mode):
    rng = np.random.default_rng(100 * s + 10 * (frame == "view") + (mode == "Raytracer"))
    for w, h in SIZES:
        _kernel_alone(_scene(mode, w, h, worlds=3), s, frame, rng)


@pytest.mark.parametrize("frame", ["world", "view"])
def test_the_grid_stride_loop_on_a_one_cu_grid(native, monkeypatch, frame):
    """MRX_FAKE_CUS=1: eight workgroups, a stride of 2048 items.  4 views of 64 x 64 -- eight trips, half a view each --
    and 5 views of 40 x 24, where the stride is two views, three rows and eight pixels and every digit carries."""
    monkeypatch.setenv("MRX_FAKE_CUS", "1")
    rng = np.random.default_rng(7 + (frame == "view"))
    _kernel_alone(_scene("Rasterizer", 64, 64, worlds=4), 1, frame, rng)
    _kernel_alone(_scene("Rasterizer", 40, 24, worlds=5), 1, frame, rng)
    _kernel_alone(_scene("Raytracer", 40, 40, worlds=5), 2, frame, rng)


@pytest.mark.parametrize("case", list(PARITY))
def test_the_whole_renderer_unprojects_its_own_depth(native, case):
    import torch
    build, variant, entry, bvh, rt, s = PARITY[case]
    frame = "view" if list(PARITY).index(case) % 2 else "world"
    base = dataclasses.replace(build(), supersample=s, normals=True)
    r = _make(dataclasses.replace(base, positions=frame), visibility=not rt, variant=variant)
    plain = _make(base, visibility=not rt, variant=variant)
    if entry is not None:
        assert r.raster_entry() == entry
    assert r.bvh_launch()["kernel"] == bvh and plain.bvh_launch() == r.bvh_launch()
    assert plain.raster_entry() == r.raster_entry()
    r.sync()
    plain.sync()
    got = _np(r.position_tensor())
    depth = _depth(r)
    _assert_bits(got, _reference(r, base, s, frame, rt), case)
    assert (depth != 0).any() and (depth == 0).any()
    assert np.array_equal(got[..., 3].view(np.uint32), np.where(depth != 0, np.float32(1), np.float32(0)).view(np.uint32))
    # every other output is bit for bit that of the renderer without the option
    for getter in ("rgb_tensor", "depth_tensor", "normal_tensor", "segmask_tensor" if rt else "visibility_tensor"):
        a, b = getattr(r, getter)().to_torch(), getattr(plain, getter)().to_torch()
        assert a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), getter
    # ... and so are the bytes of a step, but for the stage's 4 + 16 per native pixel
    assert r.bytes_per_step() == plain.bytes_per_step() + depth.size * 20


@pytest.mark.parametrize("mode", ["Rasterizer", "Raytracer"])
def test_a_depth_only_renderer_has_positions(native, mode):
    rt = mode == "Raytracer"
    base = _scene(mode, 40, 24, worlds=3)
    r = _make(dataclasses.replace(base, positions=True), visibility=False, outputs="Depth")
    assert r.positions == "world"
    r.sync()
    with pytest.raises(RuntimeError):
        r.rgb_tensor()
    _assert_bits(_np(r.position_tensor()), _reference(r, base, 1, "world", rt), mode)
    assert (_depth(r) != 0).any()
    with pytest.raises((RuntimeError, ValueError)):
        _make(dataclasses.replace(base, positions=True), visibility=False, outputs="RGB")


def test_pose_and_projection_are_read_when_the_stage_runs(native):
    import torch
    base = _scene("Rasterizer", 40, 24, worlds=5)
    r = _make(dataclasses.replace(base, positions="world"), visibility=False)
    r.sync()
    first = _np(r.position_tensor())
    _assert_bits(first, _reference(r, base, 1, "world", False), "first frame")
    # a camera moved and new projections, then step(): the points are those of the new camera and the new depth
    cp = r.camera_position_tensor().to_torch()
    cp.add_(torch.tensor([0.5, -0.25, 1.0], device=cp.device))
    projections = [(f, 0.001 if z is None else z) for f, z in po.mixed(base.num_views)]
    r.set_camera_projection([f for f, _ in projections], [z for _, z in projections])
    r.step()
    r.sync()
    second = _np(r.position_tensor())
    _assert_bits(second, _reference(r, base, 1, "world", False), "after step()")
    assert (second != first).any()
    # unproject() alone after a pose write: the same depth, the points moved with the camera
    depth = _depth(r).copy()
    rot = r.camera_rotation_tensor().to_torch()
    rot.copy_(rot.roll(1, 0))
    cp.add_(torch.tensor([3.0, 2.0, -1.0], device=cp.device))
    r.unproject()
    r.sync()
    third = _np(r.position_tensor())
    assert np.array_equal(_depth(r).view(np.uint32), depth.view(np.uint32))
    _assert_bits(third, _reference(r, base, 1, "world", False), "after unproject()")
    hit = depth != 0
    assert (third[hit] != second[hit]).any(axis=-1).all()


def test_two_shards_on_one_device_equal_one(native):
    import torch
    base = dataclasses.replace(_scene("Rasterizer", 40, 24, worlds=5), supersample=2, positions="world")
    one = _make(base, visibility=True)
    two = _make(base, visibility=True, device_ids=[0, 0])
    assert two.num_shards == 2 and two.positions == "world"
    two.step()
    one.step()
    one.sync()
    two.sync()
    for getter in ("position_tensor", "depth_tensor", "rgb_tensor"):
        whole = getattr(one, getter)().to_torch()
        parts = torch.cat([getattr(two, getter)(shard=i).to_torch() for i in range(2)])
        assert whole.shape == parts.shape and torch.equal(whole.view(torch.uint8), parts.view(torch.uint8)), getter
    with pytest.raises(ValueError):
        two.position_tensor()                               # several shards: say which
    # unproject() alone reaches every shard: scribble over shard 1's points, unproject, and they are back
    t = two.position_tensor(shard=1).to_torch()
    keep = t.clone()
    t.fill_(7.0)
    two.unproject()
    two.sync()
    assert torch.equal(t.view(torch.int32), keep.view(torch.int32))


def test_the_option_off_is_the_renderer_without_the_argument(native):
    import torch
    base = _scene("Raytracer", 40, 40, worlds=3)
    a = _make(base, visibility=False)
    b = _make(dataclasses.replace(base, positions=False), visibility=False)
    a.sync()
    b.sync()
    assert a.positions is None and b.positions is None
    assert a.raster_entry() == b.raster_entry() and a.bytes_per_step() == b.bytes_per_step()
    for getter in ("rgb_tensor", "depth_tensor", "segmask_tensor"):
        x, y = getattr(a, getter)().to_torch(), getattr(b, getter)().to_torch()
        assert x.shape == y.shape and torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    for r in (a, b):
        with pytest.raises(RuntimeError, match="MRX_FLAG_POSITIONS"):
            r.position_tensor()
        with pytest.raises(RuntimeError, match="MRX_FLAG_POSITIONS"):
            r.unproject()
    for good, name in ((True, "world"), ("world", "world"), ("view", "view")):
        c = _make(dataclasses.replace(base, positions=good), visibility=False)
        assert c.positions == name and c.bytes_per_step() == a.bytes_per_step() + 3 * 40 * 40 * 20


def test_yardstick_one_unproject_takes_no_longer_than_copying_its_output(native):
    """1024 views of 64 x 64, world frame: the stage reads 4 and writes 16 bytes per pixel, 80 MiB; a device-to-device
    copy of the position tensor reads 16 and writes 16, 128 MiB.  Same process, same stream, mark / elapsed_ms around
    batches of 10, the median of 9 batches each.  A stage slower than the copy is not streaming."""
    import torch
    r = _make(dataclasses.replace(scenes.synthetic_scene(1024), positions="world"), visibility=False)
    p = r.position_tensor().to_torch()
    assert tuple(p.shape) == (1024, 64, 64, 4) and p.dtype == torch.float32
    p2 = torch.empty_like(p)
    r.sync()

    def timed(fn, batch=10):
        r.mark(0)
        for _ in range(batch):
            fn()
        r.mark(1)
        return r.elapsed_ms() * 1000.0 / batch

    def copy():
        p2.copy_(p)

    for fn in (r.unproject, copy):
        timed(fn, 20)                                       # warm-up
    stage, cop = [], []
    for _ in range(9):                                      # alternating, so that a clock change hits both
        stage.append(timed(r.unproject))
        cop.append(timed(copy))
    stage_us, copy_us = statistics.median(stage), statistics.median(cop)
    print(f"unproject {stage_us:.2f} us, copy of the position tensor {copy_us:.2f} us (1024 x 64x64, world frame)")
    assert stage_us <= copy_us, (stage_us, copy_us)


def _read_ply(path):
    data = open(path, "rb").read()
    head, _, body = data.partition(b"end_header\n")
    lines = head.decode().splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    count = int([l for l in lines if l.startswith("element vertex ")][0].split()[2])
    props = [l.split()[1:] for l in lines if l.startswith("property ")]
    return count, props, body


@pytest.mark.parametrize("outputs", ["rgbd", "depth"])
def test_headless_writes_the_hit_pixels_as_a_point_cloud(native, tmp_path, outputs):
    from madrona_renderer_amd import build
    cmd = ["timeout", "-k", "10", "120", build.headless_path(), "4", "1", "rast", "64", "64", "--positions",
           "--dump-last-frame", "cloud", "--outputs", outputs]
    p = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    count, props, body = _read_ply(tmp_path / "cloud.points.ply")
    r = _make(dataclasses.replace(scenes.synthetic_scene(4), positions=True), visibility=False)
    r.sync()
    hit = _depth(r) != 0
    assert count == int(hit.sum()) and 0 < count < hit.size
    xyz = [["float", "x"], ["float", "y"], ["float", "z"]]
    colour = [["uchar", "red"], ["uchar", "green"], ["uchar", "blue"]]
    assert props == (xyz + colour if outputs == "rgbd" else xyz)
    rec = np.dtype([("p", "<f4", 3)] + ([("c", "u1", 3)] if outputs == "rgbd" else []))
    assert len(body) == count * rec.itemsize
    v = np.frombuffer(body, rec)
    assert np.array_equal(v["p"].view(np.uint32), _np(r.position_tensor())[hit][:, :3].view(np.uint32))   # storage order
    if outputs == "rgbd":
        assert np.array_equal(v["c"], _np(r.rgb_tensor())[hit][:, :3])
    assert os.path.exists(tmp_path / "cloud.png")
