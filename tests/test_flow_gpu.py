"""The optical-flow output on the MI355X (-m gpu).

The flow kernel against tests/flow_oracle.flow applied to the renderer's own depth, visibility ids, pose columns and the
previous state -- read back from the tensors before the step that moves them -- on every bit: through the raster group
kernel, the BVH tile kernel and the flat kernel, both modes, s = 1, 2, 3, a one-CU grid, a world of more rows than one
staging pass and a world with spare rows.  The order of flow and snapshot on the stream, flow() and flow_snapshot()
alone, every other output against a renderer without the option, two shards, the option off, boxes= and flow= refused together, the
headless dump and the yardstick."""
import dataclasses
import os
import statistics
import subprocess

import numpy as np
import pytest

from madrona_renderer_amd import scenes
from tests import flow_oracle as fo
from tests import meshes
from tests.test_projection_gpu import _make
from tests.test_supersample_gpu import _scene

pytestmark = pytest.mark.gpu

# the yardstick's bound: flow() + flow_snapshot() took 52.98 us against 16.92 us for unproject() on one MI355X, ratio 3.13
# (profiles/flow_latest.txt); times 1.5, rounded up
YARDSTICK_RATIO = 5.0

F = np.float32


def _np(t):
    return t.to_torch().cpu().numpy()


def _tables(fs):
    """instKBase as the renderer builds it: the first world-local triangle index of every row, an undrawn row repeating
    its successor's"""
    kbase = np.zeros(len(fs.inst_obj0), np.uint32)
    for w in range(len(fs.world_inst_start) - 1):
        k = 0
        for row in range(int(fs.world_inst_start[w]), int(fs.world_inst_start[w + 1])):
            kbase[row] = k
            o = int(fs.inst_obj0[row])
            if 0 <= o < len(fs.obj_num_tris):
                k += int(fs.obj_num_tris[o])
    return kbase, np.asarray(fs.world_inst_start, np.uint32), np.asarray(fs.view_world, np.uint32)


def _state(r, shard=None):
    """the five live columns, and the constants of every view, as they are now"""
    kw = {} if shard is None else {"shard": shard}
    return tuple(_np(getattr(r, g)(**kw)).copy() for g in ("instance_position_tensor", "instance_rotation_tensor",
                                                           "instance_scale_tensor", "camera_position_tensor",
                                                           "camera_rotation_tensor"))


def _consts(r, desc, s, rt):
    f, z = r.camera_projection()
    return fo.constants(desc.width, desc.height, rt, list(zip(f.tolist(), z.tolist())), s)


def _expected(r, desc, tables, s, rt, prev, prev_consts):
    d = _np(r.depth_tensor())
    return fo.flow(d.reshape(d.shape[:3]), _np(r.visibility_tensor()), _consts(r, desc, s, rt), prev_consts, *tables,
                   _state(r), prev, s, rt)


def _assert_bits(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype == F, (what, got.shape, want.shape)
    bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    assert bad == 0, f"{what}: {bad} of {got.size} values differ in their bits"


def _move(r, rng, desc):
    """instance positions, rotations and scales through the tensors, cameras moved and turned, new per-view projections"""
    import torch

    def write(t, a):
        t.copy_(torch.from_numpy(np.ascontiguousarray(a, F)).to(t.device))

    def turn(q, sigma):
        x = q.astype(np.float64) + rng.normal(scale=sigma, size=q.shape)
        return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(F)

    pos, rot, scl, cp, cr = (getattr(r, g)().to_torch() for g in (
        "instance_position_tensor", "instance_rotation_tensor", "instance_scale_tensor", "camera_position_tensor",
        "camera_rotation_tensor"))
    write(pos, pos.cpu().numpy() + rng.uniform(-0.3, 0.3, tuple(pos.shape)))
    write(rot, turn(rot.cpu().numpy(), 0.05))
    write(scl, scl.cpu().numpy() * rng.uniform(0.9, 1.1, tuple(scl.shape)))
    write(cp, cp.cpu().numpy() + rng.uniform(-0.2, 0.2, tuple(cp.shape)))
    write(cr, turn(cr.cpu().numpy(), 0.02))
    r.set_camera_projection([70.0 + 7.0 * (v % 5) for v in range(desc.num_views)])


CASES = {
    # name: (builder, kernel variant, bvh kernel, raytracer, s, positions= of both renderers)
    "raster-64x64": (lambda: scenes.synthetic_scene(4, with_wall=True, textured=True), None, "none", False, 1, "world"),
    "raster-5x3-s3": (lambda: _scene("Rasterizer", 5, 3, worlds=3), None, "none", False, 3, "view"),
    "raster-rt-40-s2": (lambda: _scene("Raytracer", 40, 40, worlds=3), None, "none", True, 2, "world"),
    "bvh-tile-40x24-s2": (lambda: meshes.cube_field(num_worlds=3, cubes=40, width=40, height=24), None, "tile", False, 2,
                          "view"),
    "bvh-tile-71-rows": (lambda: meshes.cube_field(num_worlds=3, cubes=70, width=40, height=24), None, "tile", False, 1,
                         None),
    "flat-rt-40-s3": (lambda: _scene("Raytracer", 40, 40, worlds=3), 2, "flat", True, 3, "world"),
    "flat-64x64": (lambda: _scene("Rasterizer", 64, 64, worlds=4), 2, "flat", False, 1, None),
}


def _run_case(case, oracle_mod):
    import torch
    build, variant, bvh, rt, s, positions = CASES[case]
    base = dataclasses.replace(build(), supersample=s, normals=True, positions=positions)
    rng = np.random.default_rng(len(case) + 100 * s)
    r = _make(dataclasses.replace(base, flow=True), visibility=False, variant=variant)      # flow= sets the flag itself
    plain = _make(base, visibility=True, variant=variant)
    assert r.flows is True and plain.flows is False and r.bvh_launch()["kernel"] == bvh
    assert r.positions == positions and plain.positions == positions
    tables = _tables(oracle_mod.FlatScene(base))
    nslow, nfast = (base.width, base.width) if rt else (base.height, base.width)
    assert tuple(r.flow_tensor().shape) == (base.num_views, nslow, nfast, 4)
    assert r.bytes_per_step() == plain.bytes_per_step() + base.num_views * nslow * nfast * 24
    r.sync()
    # the first frame: the snapshot was taken at creation, a still scene
    _assert_bits(_np(r.flow_tensor()), _expected(r, base, tables, s, rt, _state(r), _consts(r, base, s, rt)), case + " first")
    # motion between two steps, the same on both renderers
    prev, prev_consts = _state(r), _consts(r, base, s, rt)
    for x in (r, plain):
        _move(x, np.random.default_rng(len(case)), base)
        x.step()
        x.sync()
    moved = _np(r.flow_tensor())
    _assert_bits(moved, _expected(r, base, tables, s, rt, prev, prev_consts), case + " moved")
    valid = moved[..., 3] == 1
    assert valid.any() and (~valid).any() and (moved[valid][:, :3] != 0).any()
    # every other output is bit for bit that of a renderer with the visibility flag and without flow=
    # (the unprojection runs just ahead of the flow on the same stream and reads the same depth)
    for getter in ("rgb_tensor", "depth_tensor", "visibility_tensor", "normal_tensor") + \
            (("position_tensor",) if positions else ()):
        a, b = getattr(r, getter)().to_torch(), getattr(plain, getter)().to_torch()
        assert a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), getter
    # a third step with nothing written: the snapshot followed the second, a still scene
    r.step()
    r.sync()
    still = _np(r.flow_tensor())
    _assert_bits(still, _expected(r, base, tables, s, rt, _state(r), _consts(r, base, s, rt)), case + " still")
    assert (still != moved).any()
    return r, base, tables, rng


@pytest.mark.parametrize("case", list(CASES))
def test_the_flow_of_the_whole_renderer_is_the_oracle_s(native, oracle_mod, case):
    _run_case(case, oracle_mod)


def test_the_grid_stride_loop_on_a_one_cu_grid(native, oracle_mod, monkeypatch):
    """MRX_FAKE_CUS=1: eight workgroups for 4 x 16 items of 64 x 64 views, eight trips each; passes of 2 rows restage"""
    monkeypatch.setenv("MRX_FAKE_CUS", "1")
    monkeypatch.setenv("MRX_FLOW_PASS_ROWS", "2")
    _run_case("raster-64x64", oracle_mod)
    _run_case("bvh-tile-40x24-s2", oracle_mod)


def test_flow_alone_is_idempotent_and_the_snapshot_alone_stills_the_scene(native, oracle_mod):
    import torch
    r, base, tables, rng = _run_case("raster-64x64", oracle_mod)
    s, rt = 1, False
    prev, prev_consts = _state(r), _consts(r, base, s, rt)         # what the last step's snapshot holds
    pos = r.instance_position_tensor().to_torch()
    pos.add_(torch.tensor([0.25, -0.5, 0.125], device=pos.device))
    r.flow()
    r.sync()
    once = _np(r.flow_tensor()).copy()
    _assert_bits(once, _expected(r, base, tables, s, rt, prev, prev_consts), "flow() after a pose write")
    r.flow()                                                        # it did not advance the snapshot
    r.sync()
    _assert_bits(_np(r.flow_tensor()), once, "flow() twice")
    assert (once[once[..., 3] == 1][:, :3] != 0).any()
    r.flow_snapshot()                                               # an episode reset: the teleport shows no motion
    r.flow()
    r.sync()
    still = _np(r.flow_tensor())
    _assert_bits(still, _expected(r, base, tables, s, rt, _state(r), prev_consts), "flow_snapshot() then flow()")
    assert (still != once).any()


def test_a_world_with_spare_rows_between_drawn_ones(native, oracle_mod):
    """two spare rows per world, a cube spawned into the second: the first stays undrawn and repeats the cube's base"""
    import torch
    base = scenes.synthetic_scene(4, width=40, height=24, with_wall=True)
    base.max_instances_per_world = 6
    r = _make(dataclasses.replace(base, flow=True), visibility=False)
    fs = oracle_mod.FlatScene(base)
    obj, pos = r.instance_object_tensor().to_torch(), r.instance_position_tensor().to_torch()
    rows = [int(fs.world_inst_start[w + 1]) - 1 for w in range(4)]
    assert all(fs.inst_obj[row] < 0 and fs.inst_obj[row - 1] < 0 for row in rows)
    eyes = _np(r.camera_position_tensor())
    for w, row in enumerate(rows):
        fs.inst_obj[row] = 0
        fs.inst_pos[row] = 0.5 * eyes[w] + np.array([0.0, 0.0, 0.5], F)       # half way to the eye: in sight
    obj.copy_(torch.from_numpy(fs.inst_obj).to(obj.device))
    pos.copy_(torch.from_numpy(fs.inst_pos).to(pos.device))
    r.refresh_objects()
    fs.refresh_objects()
    tables = _tables(fs)
    assert all(tables[0][row] == tables[0][row - 1] for row in rows)
    r.flow_snapshot()
    r.step()
    r.sync()
    prev, prev_consts = _state(r), _consts(r, base, 1, False)
    vis = _np(r.visibility_tensor())
    assert all((vis[w] >= tables[0][rows[w]]).any() for w in range(4))        # the spawned cube is seen
    pos[rows[0]:rows[0] + 1].add_(0.2)
    pos[rows[1] - 2:rows[1] - 1].add_(-0.2)
    r.step()
    r.sync()
    got = _np(r.flow_tensor())
    _assert_bits(got, _expected(r, base, tables, 1, False, prev, prev_consts), "spare rows")
    assert (got[0][..., :3] != 0).any()


def test_two_shards_on_one_device(native, oracle_mod):
    import torch
    base = dataclasses.replace(_scene("Rasterizer", 40, 24, worlds=5), supersample=2, flow=True)
    one = _make(base, visibility=False)
    two = _make(base, visibility=False, device_ids=[0, 0])
    assert two.num_shards == 2 and two.flows is True
    for x in (one, two):
        for i in range(x.num_shards):
            cp = x.camera_position_tensor(shard=i).to_torch()
            cp.add_(torch.tensor([0.5, -0.25, 0.125], device=cp.device))
        x.step()
        x.sync()
    whole = one.flow_tensor().to_torch()
    parts = torch.cat([two.flow_tensor(shard=i).to_torch() for i in range(2)])
    assert whole.shape == parts.shape and torch.equal(whole.view(torch.int32), parts.view(torch.int32))
    assert (whole[..., :3] != 0).any()
    with pytest.raises(ValueError):
        two.flow_tensor()                                   # several shards: say which
    # flow() and flow_snapshot() reach every shard: scribble over shard 1's flow, move the cameras again, flow() --
    # the snapshot is the last step's on every shard -- then flow_snapshot() and flow(): the still scene on every shard
    def both():
        a = one.flow_tensor().to_torch().view(torch.int32)
        b = torch.cat([two.flow_tensor(shard=i).to_torch() for i in range(2)]).view(torch.int32)
        assert torch.equal(a, b)
        return a.clone()

    two.flow_tensor(shard=1).to_torch().fill_(7.0)
    for x in (one, two):
        for i in range(x.num_shards):
            cp = x.camera_position_tensor(shard=i).to_torch()
            cp.add_(torch.tensor([-0.25, 0.5, 0.25], device=cp.device))
        x.flow()
        x.sync()
    moved = both()
    for x in (one, two):
        x.flow_snapshot()
        x.flow()
        x.sync()
    still = both()
    assert not torch.equal(moved, whole.view(torch.int32)) and not torch.equal(still, moved)
    assert torch.equal(still[..., 3], moved[..., 3])


def test_the_option_off(native):
    base = _scene("Rasterizer", 40, 24, worlds=3)
    a = _make(base, visibility=True)
    assert a.flows is False
    for call in (a.flow_tensor, a.flow, a.flow_snapshot):
        with pytest.raises(RuntimeError, match="mrx_flow_create"):
            call()
    with pytest.raises((RuntimeError, ValueError)):
        _make(dataclasses.replace(base, flow=True), visibility=False, outputs="RGB")
    b = _make(dataclasses.replace(base, flow=True), visibility=False, outputs="Depth")
    assert b.flows is True
    with pytest.raises(RuntimeError):
        b.segmask_tensor()                                  # the known limit: the ids tensor holds visibility ids


def test_boxes_and_flow_together_are_refused_and_the_next_renderer_works(native):
    """boxes= reads label or segmask ids, flow= turns the ids tensor into visibility ids: the pair is an error, raised
    before anything is created, and leaves nothing behind that a renderer created right afterwards would trip over"""
    scene = _scene("Rasterizer", 40, 24, worlds=3)
    labelled = dataclasses.replace(scene, instance_labels=True, boxes=8)
    with pytest.raises(ValueError, match="flow and boxes exclude each other"):
        _make(dataclasses.replace(labelled, flow=True), visibility=False)
    for desc in (labelled, dataclasses.replace(scene, flow=True)):
        r = _make(desc, visibility=False)
        r.step()
        r.sync()
        assert (_np(r.depth_tensor()) != 0).any()
        if desc.boxes:
            assert r.flows is False and (_np(r.box_tensor())[..., 4] > 0).any()
        else:
            assert r.flows is True and (_np(r.flow_tensor())[..., 3] == 1).any()


def test_headless_dump_equals_the_tensor(native, tmp_path):
    from madrona_renderer_amd import build
    cmd = ["timeout", "-k", "10", "120", build.headless_path(), "4", "2", "rast", "64", "64", "--flow",
           "--dump-last-frame", "frame"]
    p = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    dumped = np.load(tmp_path / "frame.flow.npy")
    r = _make(dataclasses.replace(scenes.synthetic_scene(4), flow=True), visibility=False)
    r.step()
    r.step()
    r.sync()
    got = _np(r.flow_tensor())
    assert dumped.dtype == F and dumped.shape == got.shape == (4, 64, 64, 4)
    assert np.array_equal(dumped.view(np.uint32), got.view(np.uint32)) and (got[..., 3] == 1).any()
    assert os.path.exists(tmp_path / "frame.png")


def test_yardstick_flow_and_snapshot_against_the_unprojection(native):
    """1024 views of 64 x 64: one flow() plus one flow_snapshot() (24 bytes per pixel, and the rows of the view's world
    staged per 256 pixels) against one unproject() (20 bytes per pixel) on the same renderer, same stream, mark /
    elapsed_ms around each, the median of 20.  Both working sets (96 and 80 MiB) fit the Infinity Cache: neither figure
    is an HBM rate.  Measured 52.98 us against 16.92 us, ratio 3.13 (profiles/flow_latest.txt); the bound
    is that ratio times 1.5, rounded up: 5."""
    r = _make(dataclasses.replace(scenes.synthetic_scene(1024), flow=True, positions="world"), visibility=False)
    assert tuple(r.flow_tensor().shape) == (1024, 64, 64, 4)
    r.sync()

    def timed(fn):
        r.mark(0)
        fn()
        r.mark(1)
        return r.elapsed_ms() * 1000.0

    def both():
        r.flow()
        r.flow_snapshot()

    for fn in (both, r.unproject):
        for _ in range(5):
            timed(fn)                                       # warm-up
    flow_us, unproject_us = [], []
    for _ in range(20):                                     # alternating, so that a clock change hits both
        flow_us.append(timed(both))
        unproject_us.append(timed(r.unproject))
    f, u = statistics.median(flow_us), statistics.median(unproject_us)
    print(f"flow + snapshot {f:.2f} us, unproject {u:.2f} us, ratio {f / u:.2f} (1024 x 64x64)")
    assert f <= YARDSTICK_RATIO * u, (f, u)


