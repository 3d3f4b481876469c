"""The ray-cast sensor on the MI355X (-m gpu).

The trace stage alone: rays written from torch, trace(), compared bit for bit with tests/ray_oracle.trace -- the scenes,
generators and ray counts of tests/test_ray_cpu.py plus R = 1000, in both render modes, culled and with
MRX_RAYS_BRUTE=1, the two also equal to each other, the ray tensors unchanged.  A world with more rows than a staging
pass holds (MRX_RAY_PASS_ROWS).  The whole renderer: step() after a pose write, after hiding a row, after a label write
and after refresh_objects; pinhole rays against the renderer's own segmask and depth.  No side effects: every other
output and the kernel form are those of a renderer without rays=, which allocates nothing.  Two shards against one, the
stage run twice, the headless tool's text file, and the yardstick against the depth-only render of the same views."""
import dataclasses
import functools
import statistics
import subprocess

import numpy as np
import pytest

from madrona_renderer_amd import scenes
from tests import ray_oracle as ro
from tests.test_projection_gpu import _make
from tests.test_ray_cpu import R_VALUES, SCENES, state

pytestmark = pytest.mark.gpu

F = np.float32


def _np(t):
    return t.to_torch().cpu().numpy()


def _put(tensor, array):
    import torch
    t = tensor.to_torch()
    a = torch.from_numpy(np.array(array))               # (a copy: the shared cases are read-only)
    assert tuple(t.shape) == tuple(a.shape) and t.dtype == a.dtype, (t.shape, a.shape, t.dtype, a.dtype)
    t.copy_(a.to(t.device))


@functools.lru_cache(maxsize=None)
def _case(name, R):
    """(desc, fs, labels, frames, rays, want_t, want_id) of a scene and a ray count: computed once, never changed"""
    from oracle import oracle
    desc, cube = SCENES[name]()
    fs, labels, frames, _ = state(name, oracle)
    rays = ro.mixed(fs, R, seed=R, cube=cube)
    want_t, want_id = ro.trace(fs, rays, frames, labels)
    for a in (labels, frames, rays, want_t, want_id):
        a.setflags(write=False)
    return desc, fs, labels, frames, rays, want_t, want_id


def _renderer(desc, fs, labels, R, mode, **kw):
    """a renderer of `desc` with the sensor, in the state of `fs`: its hidden rows hidden, the labels written"""
    d = dataclasses.replace(desc, render_mode=mode, rays=R, instance_labels=None if labels is None else True)
    r = _make(d, visibility=False, **kw)
    assert r.rays == R
    if r.num_shards == 1:
        _put(r.instance_object_tensor(), fs.inst_obj)
        if labels is not None:
            _put(r.instance_label_tensor(), labels)
    return r


def _assert_same(got_t, got_id, want_t, want_id, what):
    bad = ~((got_t.view(np.uint32) == want_t.view(np.uint32)) | (np.isnan(got_t) & np.isnan(want_t))) | (got_id != want_id)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5], got_t[bad][:5], want_t[bad][:5], got_id[bad][:5],
                           want_id[bad][:5])


# ---- the stage alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", R_VALUES + (1000,))
@pytest.mark.parametrize("name", sorted(SCENES))
def test_the_trace_stage_is_exact(native, monkeypatch, name, R):
    desc, fs, labels, frames, rays, want_t, want_id = _case(name, R)
    W = desc.num_worlds
    # every kind of degenerate ray reaches the kernel: zero rays, NaNs, tmin >= tmax, zero directions, tmax = inf
    assert R < 63 or all(n > 0 for n in ro.degenerate_kinds(rays)), (R, ro.degenerate_kinds(rays))
    results = {}
    for mode in ("Rasterizer", "Raytracer"):
        for brute in ("0", "1"):
            monkeypatch.setenv("MRX_RAYS_BRUTE", brute)
            r = _renderer(desc, fs, labels, R, mode)
            assert tuple(r.ray_tensor().shape) == (W, R, 8) and tuple(r.ray_frame_tensor().shape) == (W,)
            assert tuple(r.ray_distance_tensor().shape) == (W, R) and tuple(r.ray_id_tensor().shape) == (W, R)
            r.sync()
            # as created: zero rays in the world frame, every one a miss with its tmax, 0
            assert not _np(r.ray_tensor()).any() and (_np(r.ray_frame_tensor()) == -1).all()
            assert not _np(r.ray_distance_tensor()).any() and (_np(r.ray_id_tensor()) == -1).all()
            _put(r.ray_tensor(), rays)
            _put(r.ray_frame_tensor(), frames)
            r.trace()
            r.sync()
            got_t, got_id = _np(r.ray_distance_tensor()), _np(r.ray_id_tensor())
            _assert_same(got_t, got_id, want_t, want_id, (name, R, mode, brute))
            # the inputs are inputs
            assert np.array_equal(_np(r.ray_tensor()).view(np.uint32), rays.view(np.uint32))
            assert np.array_equal(_np(r.ray_frame_tensor()), frames)
            results[mode, brute] = (got_t.view(np.uint32).copy(), got_id.copy())
            del r
    first = results["Rasterizer", "0"]
    for key, (t, i) in results.items():
        assert np.array_equal(t, first[0]) and np.array_equal(i, first[1]), key


@pytest.mark.parametrize("rows", ["1", "5", "13", "64"])
def test_a_world_with_more_rows_than_one_staging_pass_holds(native, monkeypatch, rows):
    # cube_field(3, 12): 13 rows a world -- 13, 3, 1 and 1 passes
    desc, fs, labels, frames, rays, want_t, want_id = _case("cubes", 257)
    monkeypatch.setenv("MRX_RAY_PASS_ROWS", rows)
    r = _renderer(desc, fs, labels, 257, "Rasterizer")
    _put(r.ray_tensor(), rays)
    _put(r.ray_frame_tensor(), frames)
    r.trace()
    r.sync()
    _assert_same(_np(r.ray_distance_tensor()), _np(r.ray_id_tensor()), want_t, want_id, rows)
    assert (want_id != -1).sum() > 100


def test_the_stage_run_twice_gives_identical_tensors(native):
    desc, fs, labels, frames, rays, want_t, want_id = _case("meshes", 257)
    r = _renderer(desc, fs, labels, 257, "Raytracer")
    _put(r.ray_tensor(), rays)
    _put(r.ray_frame_tensor(), frames)
    r.trace()
    r.sync()
    first = (_np(r.ray_distance_tensor()).copy(), _np(r.ray_id_tensor()).copy())
    r.trace()
    r.trace()
    r.sync()
    _assert_same(_np(r.ray_distance_tensor()), _np(r.ray_id_tensor()), first[0], first[1], "twice")
    _assert_same(first[0], first[1], want_t, want_id, "oracle")


# ---- the whole renderer ---------------------------------------------------------------------------------------------------
def test_step_follows_pose_hiding_label_and_refresh(native):
    from oracle import oracle
    R = 257
    desc = scenes.synthetic_scene(3, 32, 32, with_wall=True)
    fs = oracle.FlatScene(desc)
    rays = ro.mixed(fs, R, seed=5)
    r = _make(dataclasses.replace(desc, rays=R, instance_labels=True), visibility=False)
    _put(r.ray_tensor(), rays)
    labels = np.full(len(fs.inst_obj), ro.LABEL_OBJECT, np.int32)

    def check(what):
        r.step()
        r.sync()
        want_t, want_id = ro.trace(fs, rays, None, labels)
        _assert_same(_np(r.ray_distance_tensor()), _np(r.ray_id_tensor()), want_t, want_id, what)
        return want_id

    before = check("as created")
    assert (before == 0).any() and (before == 1).any() and (before == 2).any()
    # a pose write: every cube moves and turns, every wall grows
    fs.inst_pos[1::3] += F(0.75)
    fs.inst_rot[1::3] = fs.inst_rot[2::3]
    fs.inst_scale[2::3] *= F(1.5)
    _put(r.instance_position_tensor(), fs.inst_pos)
    _put(r.instance_rotation_tensor(), fs.inst_rot)
    _put(r.instance_scale_tensor(), fs.inst_scale)
    moved = check("pose")
    assert not np.array_equal(moved, before)
    # hiding world 0's cube
    fs.inst_obj[1] = -1
    _put(r.instance_object_tensor(), fs.inst_obj)
    hidden = check("hidden")
    assert not (hidden[0] == 0).any() and (hidden[1] == 0).any()
    # a label write
    labels[2::3] = 77
    labels[4] = -5
    _put(r.instance_label_tensor(), labels)
    labelled = check("labels")
    assert (labelled == 77).any() and not (labelled == 2).any()
    # world 1's cube becomes a wall, world 0's comes back
    fs.inst_obj[1] = 0
    fs.inst_obj[4] = 2
    labels[4] = ro.LABEL_OBJECT
    _put(r.instance_object_tensor(), fs.inst_obj)
    _put(r.instance_label_tensor(), labels)
    r.refresh_objects()
    fs.refresh_objects()
    rebound = check("refresh_objects")
    assert (rebound[1] == 2).any() and not (rebound[1] == 0).any() and (rebound[0] == 0).any()


@pytest.mark.parametrize("name,make", [
    ("synthetic", lambda: scenes.synthetic_scene(4, 32, 32)),
    ("wall", lambda: scenes.synthetic_scene(4, 40, 24, with_wall=True)),
    ("cubes", lambda: scenes.cube_field(3, 12, 32, 32)),
])
def test_pinhole_rays_reproduce_the_renderers_own_segmask_and_depth(native, name, make):
    from oracle import oracle
    desc = make()
    fs = oracle.FlatScene(desc)
    V, H, Wd = desc.num_views, desc.height, desc.width
    rays = np.stack([ro.pinhole(fs, v, tmin=oracle.RASTER_ZNEAR) for v in range(V)])
    r = _make(dataclasses.replace(desc, rays=H * Wd, instance_labels=True), visibility=False)
    _put(r.ray_tensor(), rays)
    r.step()
    r.sync()
    seg = _np(r.segmask_tensor())
    depth = _np(r.depth_tensor()).reshape(V, H, Wd).astype(np.float64)
    t, ident = _np(r.ray_distance_tensor()).reshape(V, H, Wd), _np(r.ray_id_tensor()).reshape(V, H, Wd)
    pad = np.pad(seg, ((0, 0), (1, 1), (1, 1)), mode="edge")
    decisive = ((pad[:, :-2, 1:-1] == seg) & (pad[:, 2:, 1:-1] == seg) & (pad[:, 1:-1, :-2] == seg) &
                (pad[:, 1:-1, 2:] == seg))
    covered = seg != -1
    excluded = float((~decisive & covered).sum()) / float(covered.sum())     # the share of the covered pixels left out
    assert excluded <= 0.20, excluded
    assert np.array_equal(ident[decisive], seg[decisive])
    on = decisive & covered
    rel = np.abs(t[on].astype(np.float64) - depth[on]) / depth[on]
    ground = seg[on] == 1
    print("%s: excluded %.2f %%, max relative depth error %.3g off the ground, %.3g on it" %
          (name, 100 * excluded, rel[~ground].max(), rel[ground].max() if ground.any() else 0.0))
    assert rel[~ground].max() <= 2e-6
    assert not ground.any() or rel[ground].max() <= 3e-4


# ---- no side effects ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["Rasterizer", "Raytracer"])
def test_every_other_output_is_that_of_a_renderer_without_the_sensor(native, mode):
    import torch
    # (the label column gives Rasterizer mode the segmask the box stage reads; boxes and observations are the two stages
    # directly in front of the trace stage)
    base = dataclasses.replace(scenes.synthetic_scene(5, 40, 24, with_wall=True, textured=True), render_mode=mode,
                               normals=True, positions=True, instance_labels=True, boxes=8,
                               observations=dict(channels="rgbd", dtype="float16", stack=2))
    a = _make(base, visibility=False)
    b = _make(dataclasses.replace(base, rays=100), visibility=False)
    for r in (a, b):
        r.step()
        r.sync()
    assert a.rays == 0 and b.rays == 100
    assert a.raster_entry() == b.raster_entry() and a.kernel_form() == b.kernel_form()
    assert b.bytes_per_step() == a.bytes_per_step() + 5 * 100 * 40
    getters = ["rgb_tensor", "depth_tensor", "normal_tensor", "position_tensor", "segmask_tensor", "box_tensor",
               "observation_tensor"]
    assert bool((a.box_tensor().to_torch()[..., 4] > 0).any()) and bool(a.observation_tensor().to_torch().any())
    for getter in getters:
        x, y = getattr(a, getter)().to_torch(), getattr(b, getter)().to_torch()
        assert x.shape == y.shape and torch.equal(x.view(torch.uint8), y.view(torch.uint8)), getter
    # rays=None allocates nothing: the getters and trace() raise
    for getter in ("ray_tensor", "ray_frame_tensor", "ray_distance_tensor", "ray_id_tensor", "trace"):
        with pytest.raises(RuntimeError, match="mrx_rays_create"):
            getattr(a, getter)()


def test_two_shards_on_one_device_equal_one(native):
    import torch
    desc, fs, labels, frames, rays, want_t, want_id = _case("wall", 257)
    one = _renderer(desc, fs, None, 257, "Rasterizer")
    two = _renderer(desc, fs, None, 257, "Rasterizer", device_ids=[0, 0])
    assert two.num_shards == 2 and two.rays == 257
    lo = [two.shard_first_world(i) for i in range(3)]
    _put(one.ray_tensor(), rays)
    _put(one.ray_frame_tensor(), frames)
    _put(one.instance_object_tensor(), fs.inst_obj)
    for i in range(2):
        _put(two.ray_tensor(shard=i), rays[lo[i]:lo[i + 1]])
        _put(two.ray_frame_tensor(shard=i), frames[lo[i]:lo[i + 1]])
        rows = slice(int(fs.world_inst_start[lo[i]]), int(fs.world_inst_start[lo[i + 1]]))
        _put(two.instance_object_tensor(shard=i), fs.inst_obj[rows])
    one.step()
    two.step()
    one.sync()
    two.sync()
    want_t, want_id = ro.trace(fs, rays, frames, None)
    _assert_same(_np(one.ray_distance_tensor()), _np(one.ray_id_tensor()), want_t, want_id, "one")
    for getter in ("ray_distance_tensor", "ray_id_tensor"):
        whole = getattr(one, getter)().to_torch()
        parts = torch.cat([getattr(two, getter)(shard=i).to_torch() for i in range(2)])
        assert whole.shape == parts.shape and torch.equal(whole.view(torch.uint8), parts.view(torch.uint8)), getter
    with pytest.raises(ValueError):
        two.ray_distance_tensor()                           # several shards: say which
    # trace() alone reaches every shard: scribble over shard 1's distances, trace(), and they are back
    t = two.ray_distance_tensor(shard=1).to_torch()
    keep = t.clone()
    t.fill_(7)
    two.trace()
    two.sync()
    assert torch.equal(t.view(torch.int32), keep.view(torch.int32))


def test_headless_writes_the_rays_of_the_last_frame(native, tmp_path):
    from madrona_renderer_amd import build
    cmd = ["timeout", "-k", "10", "120", build.headless_path(), "8", "1", "rast", "64", "64", "--rays", "90",
           "--dump-last-frame", "frame"]
    p = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    lines = (tmp_path / "frame.rays.txt").read_text().splitlines()
    assert len(lines) == 8 * 90
    rows = [l.split() for l in lines]
    assert [(int(a), int(b)) for a, b, _, _ in rows] == [(w, i) for w in range(8) for i in range(90)]
    ids = np.array([int(x[3]) for x in rows])
    t = np.array([float(x[2]) for x in rows])
    # a horizontal fan from a camera above the ground: no ray meets the ground quad (object 1); a miss holds its tmax
    assert set(ids.tolist()) <= {-1, 0} and (ids == -1).any()
    assert (t[ids == -1] == 1000.0).all() and (t[ids == 0] > 0.0).all() and (t[ids == 0] < 1000.0).all()


# ---- yardstick ------------------------------------------------------------------------------------------------------------
# Measured on an MI355X (profiles/rays_latest.txt): the trace of 1024 x 4096 pinhole rays 110.1 us (0.0262 ns per ray), the
# depth-only render of the same 1024 views of 64 x 64 11.3 us, ratio 9.74.  The bound is that ratio times 1.5, rounded up
# to an integer; the margin covers clock and placement variation, as the other perf guards' do.
RATIO_BOUND = 15


def test_yardstick_a_trace_of_4096_pinhole_rays_against_the_depth_only_render(native):
    """1024 worlds of synthetic_scene, 64 x 64 views: the trace of the 4096 pinhole rays of every world's view against
    the depth-only render of the same 1024 views, same process, same stream, mark / elapsed_ms around every call,
    alternating; the median of 20 each."""
    from oracle import oracle
    desc = scenes.synthetic_scene(1024)
    fs = oracle.FlatScene(desc)
    rays = np.stack([ro.pinhole(fs, v, tmin=oracle.RASTER_ZNEAR) for v in range(1024)])
    r = _make(dataclasses.replace(desc, rays=4096), visibility=False, outputs="Depth")
    plain = _make(desc, visibility=False, outputs="Depth")          # the render as it is without the sensor
    _put(r.ray_tensor(), rays)
    r.sync()
    plain.sync()

    def timed(who, fn):
        who.mark(0)
        fn()
        who.mark(1)
        return who.elapsed_ms() * 1000.0

    for who, fn in ((r, r.trace), (plain, plain.render)):
        for _ in range(10):                                 # warm-up
            timed(who, fn)
    trace, render = [], []
    for _ in range(20):                                     # alternating, so that a clock change hits both
        trace.append(timed(r, r.trace))
        render.append(timed(plain, plain.render))
    trace_us, render_us = statistics.median(trace), statistics.median(render)
    depth = _np(r.depth_tensor()).reshape(1024, 4096)
    ident = _np(r.ray_id_tensor())
    assert ((depth != 0) == (ident != -1)).mean() > 0.99
    print(f"trace {trace_us:.2f} us ({trace_us * 1000 / (1024 * 4096):.4f} ns per ray), depth-only render "
          f"{render_us:.2f} us, ratio {trace_us / render_us:.2f} (1024 x 4096 rays, 1024 x 64x64)")
    assert trace_us <= RATIO_BOUND * render_us, (trace_us, render_us)
