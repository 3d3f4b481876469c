"""Box labels on the MI355X (-m gpu).

The box kernel alone: the ids tensor overwritten with seeded values (background, labels in range, and ids that belong
to no row), boxes(), compared bit for bit with tests/box_oracle.boxes in both modes for K = 1, 5, 64, 1024 at sizes
with one-lane and two-lane tail segments, several segments per row and several workgroups per view, and on the
resolved tensor of a supersampled renderer.  The merge path -- several workgroups per view, forced by MRX_BOX_PARTS
and chosen by the automatic rule on a small grid -- against the oracle and against the one-workgroup form.  The whole
renderer: boxes of its own segmask, every other output bit for bit that of a renderer without the option.  A
depth-only renderer, a label write between steps, two shards against one, the stage run twice, the option off, the
headless tool's text file, and the yardstick: one boxes() takes no longer than two device-to-device copies of the
tensor it reads."""
import dataclasses
import statistics
import subprocess

import numpy as np
import pytest

from madrona_renderer_amd import scenes
from tests import box_oracle as bx
from tests import label_oracle as lb
from tests.test_projection_gpu import _make
from tests.test_supersample_gpu import PARITY, _scene

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (5, 3), (7, 5), (40, 24), (64, 64), (65, 2), (100, 7), (130, 3)]


def _np(t):
    return t.to_torch().cpu().numpy()


def _desc(mode, w, h, worlds=3, **kw):
    """a scene with a segmask in either mode: Raytracer has one, Rasterizer with the label column"""
    d = _scene(mode, w, h, worlds=worlds)
    if mode == "Rasterizer":
        d = dataclasses.replace(d, instance_labels=True)
    return dataclasses.replace(d, **kw)


def _kernel_alone(desc, k, ids=None, rng=None):
    """a renderer with boxes=k, its ids tensor overwritten, boxes() alone: (the box tensor, the ids written)"""
    import torch
    rt = desc.render_mode == "Raytracer"
    views = desc.num_views
    r = _make(dataclasses.replace(desc, boxes=k), visibility=False)
    assert r.box_labels == k
    nslow, nfast = (desc.width, desc.width) if rt else (desc.height, desc.width)
    assert tuple(r.box_tensor().shape) == (views, k, 5)
    r.sync()
    t = r.segmask_tensor().to_torch()
    assert tuple(t.shape) == (views, nslow, nfast) and t.dtype == torch.int32
    if ids is None:
        ids = bx.labels(rng, (views, nslow, nfast), k)
    t.copy_(torch.from_numpy(ids).to(t.device))
    r.boxes()
    r.sync()
    got = _np(r.box_tensor())
    assert got.dtype == np.int32
    want = bx.boxes(ids, k, rt)
    assert np.array_equal(got, want), (desc.width, desc.height, k, rt, int((got != want).sum()))
    assert np.array_equal(_np(r.segmask_tensor()), ids)     # the ids are read, not written
    return got, ids


@pytest.mark.parametrize("mode", ["Rasterizer", "Raytracer"])
@pytest.mark.parametrize("k", [1, 5, 64, 1024])
def test_the_box_kernel_is_exact_on_seeded_ids(native, k, mode):
    rng = np.random.default_rng(10 * k + (mode == "Raytracer"))
    for w, h in SIZES:
        _kernel_alone(_desc(mode, w, h), k, rng=rng)


@pytest.mark.parametrize("mode", ["Rasterizer", "Raytracer"])
@pytest.mark.parametrize("s", [2, 3])
def test_the_stage_reads_the_resolved_tensor_of_a_supersampled_renderer(native, s, mode):
    rng = np.random.default_rng(50 + s)
    for k in (1, 5, 64, 1024):
        _kernel_alone(_desc(mode, 12, 8, supersample=s), k, rng=rng)


def _merge_against_one_part(monkeypatch, desc, k, rng, env):
    """the same ids through the renderer under `env` and under MRX_BOX_PARTS=1: both the oracle's tensor"""
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    got, ids = _kernel_alone(desc, k, rng=rng)
    monkeypatch.setenv("MRX_BOX_PARTS", "1")
    one, _ = _kernel_alone(desc, k, ids=ids)
    monkeypatch.delenv("MRX_BOX_PARTS")
    assert np.array_equal(got, one)
    assert (got[..., 4] > 0).any()


@pytest.mark.parametrize("mode", ["Rasterizer", "Raytracer"])
def test_the_merge_path_forced_to_three_parts(native, monkeypatch, mode):
    rng = np.random.default_rng(3 + (mode == "Raytracer"))
    for w, h in ((7, 5), (40, 24), (64, 64)):
        for k in (5, 1024):
            _merge_against_one_part(monkeypatch, _desc(mode, w, h), k, rng, {"MRX_BOX_PARTS": "3"})


def test_the_automatic_rule_on_a_small_grid_and_the_stride_over_views(native, monkeypatch):
    """MRX_FAKE_CUS=1: eight resident workgroups; 2 views of 64 x 64 and 40 views of 7 x 5, whose workgroups stride
    over the views (2 * CUs = 2 views make one workgroup per view already).  MRX_FAKE_CUS=4 asks for 8 workgroups: 2 views
    of 64 x 64 are split into 4 parts each by the automatic rule."""
    rng = np.random.default_rng(11)
    _merge_against_one_part(monkeypatch, _desc("Rasterizer", 64, 64, worlds=2), 8, rng, {"MRX_FAKE_CUS": "1"})
    _merge_against_one_part(monkeypatch, _desc("Rasterizer", 7, 5, worlds=40), 8, rng, {"MRX_FAKE_CUS": "1"})
    _merge_against_one_part(monkeypatch, _desc("Raytracer", 7, 7, worlds=40), 64, rng, {"MRX_FAKE_CUS": "1"})
    _merge_against_one_part(monkeypatch, _desc("Rasterizer", 64, 64, worlds=2), 8, rng, {"MRX_FAKE_CUS": "4"})
    _merge_against_one_part(monkeypatch, _desc("Raytracer", 64, 64, worlds=2), 8, rng, {"MRX_FAKE_CUS": "4"})


def _some_labels(n):
    """most rows at the sentinel (their object's id), a few labelled 3 and 6"""
    rows = np.full(n, lb.SENTINEL, np.int32)
    rows[::3] = 3
    rows[1::7] = 6
    return rows


@pytest.mark.parametrize("case", list(PARITY))
def test_the_whole_renderer_boxes_its_own_segmask(native, case):
    import torch
    build, variant, entry, bvh, rt, s = PARITY[case]
    k = 8
    base = dataclasses.replace(build(), supersample=s, normals=True)
    if not rt:
        base = dataclasses.replace(base, instance_labels=_some_labels(len(base.instances)))
    r = _make(dataclasses.replace(base, boxes=k), visibility=False, variant=variant)
    plain = _make(base, visibility=False, variant=variant)
    if entry is not None:
        assert r.raster_entry() == entry
    assert r.bvh_launch()["kernel"] == bvh and plain.bvh_launch() == r.bvh_launch()
    assert plain.raster_entry() == r.raster_entry()
    r.sync()
    plain.sync()
    ids = _np(r.segmask_tensor())
    got = _np(r.box_tensor())
    assert got.shape == (base.num_views, k, 5) and np.array_equal(got, bx.boxes(ids, k, rt)), case
    assert (got[..., 4] > 0).any() and (got[..., 4] == 0).any()
    assert (ids == -1).any() and (ids >= 0).any()
    # every other output is bit for bit that of the renderer without the option
    for getter in ("rgb_tensor", "depth_tensor", "normal_tensor", "segmask_tensor"):
        a, b = getattr(r, getter)().to_torch(), getattr(plain, getter)().to_torch()
        assert a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), getter
    # ... and so are the bytes of a step, but for the stage's 4 per native pixel and its tensor
    assert r.bytes_per_step() == plain.bytes_per_step() + 4 * ids.size + base.num_views * k * 20


@pytest.mark.parametrize("mode", ["Rasterizer", "Raytracer"])
def test_a_depth_only_renderer_has_boxes(native, mode):
    rt = mode == "Raytracer"
    r = _make(_desc(mode, 40, 24, boxes=16), visibility=False, outputs="Depth")
    assert r.box_labels == 16
    r.sync()
    with pytest.raises(RuntimeError):
        r.rgb_tensor()
    got = _np(r.box_tensor())
    assert np.array_equal(got, bx.boxes(_np(r.segmask_tensor()), 16, rt)) and (got[..., 4] > 0).any()


def test_a_label_write_and_a_step_move_a_rows_count(native):
    r = _make(_desc("Rasterizer", 40, 24, boxes=8), visibility=False)
    r.sync()
    t = r.instance_label_tensor().to_torch()
    t.fill_(2)
    r.step()
    r.sync()
    first = _np(r.box_tensor())
    covered = (_np(r.segmask_tensor()) != -1).reshape(first.shape[0], -1).sum(axis=1)
    assert covered.min() > 0 and np.array_equal(first[:, 2, 4], covered) and (first[:, 5, 4] == 0).all()
    t.fill_(5)
    r.step()
    r.sync()
    second = _np(r.box_tensor())
    assert np.array_equal(second[:, 5], first[:, 2]) and np.array_equal(second[:, 2], first[:, 5])
    assert np.array_equal(second, bx.boxes(_np(r.segmask_tensor()), 8, False))


def test_two_shards_on_one_device_equal_one(native):
    import torch
    base = _desc("Rasterizer", 40, 24, worlds=5, supersample=2, boxes=8)
    one = _make(base, visibility=False)
    two = _make(base, visibility=False, device_ids=[0, 0])
    assert two.num_shards == 2 and two.box_labels == 8
    two.step()
    one.step()
    one.sync()
    two.sync()
    for getter in ("box_tensor", "segmask_tensor", "rgb_tensor"):
        whole = getattr(one, getter)().to_torch()
        parts = torch.cat([getattr(two, getter)(shard=i).to_torch() for i in range(2)])
        assert whole.shape == parts.shape and torch.equal(whole.view(torch.uint8), parts.view(torch.uint8)), getter
    assert bool((one.box_tensor().to_torch()[..., 4] > 0).any())
    with pytest.raises(ValueError):
        two.box_tensor()                                    # several shards: say which
    # boxes() alone reaches every shard: scribble over shard 1's rows, boxes(), and they are back
    t = two.box_tensor(shard=1).to_torch()
    keep = t.clone()
    t.fill_(7)
    two.boxes()
    two.sync()
    assert torch.equal(t, keep)


@pytest.mark.parametrize("parts", ["1", "3"])
def test_two_consecutive_boxes_calls_give_identical_tensors(native, monkeypatch, parts):
    monkeypatch.setenv("MRX_BOX_PARTS", parts)
    r = _make(_desc("Raytracer", 40, 40, boxes=64), visibility=False)
    r.sync()
    first = _np(r.box_tensor()).copy()
    r.boxes()
    r.boxes()
    r.sync()
    again = _np(r.box_tensor())
    assert np.array_equal(first, again) and (first[..., 4] > 0).any()
    assert np.array_equal(first, bx.boxes(_np(r.segmask_tensor()), 64, True))


def test_the_option_off_is_the_renderer_without_the_argument(native):
    import torch
    base = _scene("Raytracer", 40, 40, worlds=3)
    a = _make(base, visibility=False)
    b = _make(dataclasses.replace(base, boxes=0), visibility=False)
    a.sync()
    b.sync()
    assert a.box_labels == 0 and b.box_labels == 0
    assert a.raster_entry() == b.raster_entry() and a.bytes_per_step() == b.bytes_per_step()
    for getter in ("rgb_tensor", "depth_tensor", "segmask_tensor"):
        x, y = getattr(a, getter)().to_torch(), getattr(b, getter)().to_torch()
        assert x.shape == y.shape and torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    for r in (a, b):
        with pytest.raises(RuntimeError, match="MRX_FLAG_BOX_LABELS"):
            r.box_tensor()
        with pytest.raises(RuntimeError, match="MRX_FLAG_BOX_LABELS"):
            r.boxes()
    c = _make(dataclasses.replace(base, boxes=8), visibility=False)
    assert c.box_labels == 8 and c.bytes_per_step() == a.bytes_per_step() + 3 * 40 * 40 * 4 + 3 * 8 * 20
    # Rasterizer mode without labels has no segmask, visibility ids are none: refused
    with pytest.raises((RuntimeError, ValueError)):
        _make(dataclasses.replace(_scene("Rasterizer", 40, 24), boxes=8), visibility=False)
    with pytest.raises((RuntimeError, ValueError)):
        _make(dataclasses.replace(base, boxes=8), visibility=True)


def test_yardstick_one_boxes_takes_no_longer_than_two_copies_of_the_ids(native):
    """1024 views of 64 x 64, Rasterizer mode with labels, K = 8: the stage reads 16 MiB and writes 160 KiB; a
    device-to-device copy of the ids tensor reads and writes 16 MiB.  Same process, same stream, mark / elapsed_ms around
    every call, alternating; the median of 20 each; stage <= 2 x copy."""
    import torch
    desc = dataclasses.replace(scenes.synthetic_scene(1024), instance_labels=True, boxes=8)
    r = _make(desc, visibility=False)
    ids = r.segmask_tensor().to_torch()
    assert tuple(ids.shape) == (1024, 64, 64) and ids.dtype == torch.int32
    ids2 = torch.empty_like(ids)
    r.sync()
    assert np.array_equal(_np(r.box_tensor()), bx.boxes(ids.cpu().numpy(), 8, False))

    def timed(fn):
        r.mark(0)
        fn()
        r.mark(1)
        return r.elapsed_ms() * 1000.0

    def copy():
        ids2.copy_(ids)

    for fn in (r.boxes, copy):
        for _ in range(20):                                 # warm-up
            timed(fn)
    stage, cop = [], []
    for _ in range(20):                                     # alternating, so that a clock change hits both
        stage.append(timed(r.boxes))
        cop.append(timed(copy))
    stage_us, copy_us = statistics.median(stage), statistics.median(cop)
    print(f"boxes {stage_us:.2f} us, copy of the ids tensor {copy_us:.2f} us, ratio {stage_us / copy_us:.3f} "
          f"(1024 x 64x64, K = 8)")
    assert stage_us <= 2.0 * copy_us, (stage_us, copy_us)


@pytest.mark.parametrize("mode", ["rast", "rt"])
def test_headless_writes_the_boxes_of_the_dumped_labels(native, tmp_path, mode):
    from madrona_renderer_amd import build
    from tests.test_headless_gpu import _tiles
    cmd = ["timeout", "-k", "10", "120", build.headless_path(), "16", "1", mode, "64", "64", "--instance-labels", "7",
           "--boxes", "1024", "--dump-last-frame", "frame"]
    p = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    # NAME.labels.png holds the low 24 bits of every label, alpha 0 on background, upright in both modes
    png = np.stack(_tiles(tmp_path / "frame.labels.png", 16, 64, 64)).astype(np.int32)
    ids = np.where(png[..., 3] == 0, -1, png[..., 0] | (png[..., 1] << 8) | (png[..., 2] << 16)).astype(np.int32)
    want = bx.boxes(ids, 1024, False)
    lines = ["%d %d %d %d %d %d %d" % ((v, l) + tuple(want[v, l])) for v in range(16) for l in range(1024)
             if want[v, l, 4] > 0]
    assert lines                                            # (the sentinel rows' object ids, and labels 1000 ... 1023)
    assert (tmp_path / "frame.boxes.txt").read_text().splitlines() == lines
