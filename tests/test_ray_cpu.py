"""The ray-cast sensor on the host (no GPU): the host entry mrx_trace_rays_host -- the kernel's own
source, rays_core.hpp, run on the CPU -- against the NumPy restatement tests/ray_oracle.py bit for bit, culled and
brute; that restatement against the raster oracle through pinhole rays; known answers; the kernel's resources as the
compiler reports them; the launch checks through mrx_ray_plan; the Python constructor's ValueError; and the sanitizer
build of the host entry, run as a stand-alone program."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from madrona_renderer_amd import scenes
from tests import meshes
from tests import ray_oracle as ro
from tests.conftest import ROOT, has_gpu

F = np.float32
MRX_E_INVALID, MRX_E_UNSUPPORTED = -1, -5
R_VALUES = (1, 63, 64, 65, 257)


class Instance(ctypes.Structure):
    _fields_ = [("position", ctypes.c_float * 3), ("rotation", ctypes.c_float * 4), ("scale", ctypes.c_float * 3),
                ("object_id", ctypes.c_int32)]


def scaled_scene(num_worlds=3, width=32, height=32, mode="Rasterizer"):
    """Ground, an axis-aligned unrotated cube of half-size 1 (row 1: what ray_oracle.cube_grid runs over), a mirrored
    cube, a non-uniformly scaled one and a row with a zero scale component, per world."""
    inst, cams, worlds = [], [], []
    for w in range(num_worlds):
        rng = np.random.default_rng(4242 + w)
        i0 = len(inst)
        inst.append(((0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 1))
        inst.append(((2.0 + w, 1.0, 1.0), (1.0, 0.0, 0.0, 0.0), (2.0, 2.0, 2.0), 0))
        inst.append(((-3.0, 2.0 - w, 1.5), meshes.random_quat(rng), (-1.5, 1.0, 0.75), 0))
        inst.append(((0.5, -4.0, 2.0), meshes.random_quat(rng), (0.5, 3.0, 1.0), 0))
        inst.append(((-1.0, -1.0, 1.0), meshes.random_quat(rng), (1.0, 0.0, 1.0), 0))
        eye = (9.0 + w, -7.0, 6.0)
        cams.append((eye, scenes.look_at(eye, (0.0, 0.0, 1.0))))
        worlds.append((5, i0, 1, w))
    dd = scenes.DATA_DIR
    return scenes.SceneDesc(num_worlds=num_worlds, render_mode=mode, width=width, height=height,
                            asset_paths=[(os.path.join(dd, "cube.obj"), 0), (os.path.join(dd, "plane.obj"), 0)],
                            materials=[((0.6, 0.6, 0.6, 1.0), -1, 0.8, 0.2)], instances=inst, cameras=cams, worlds=worlds)


SCENES = {
    "wall": lambda: (scenes.synthetic_scene(3, 32, 32, with_wall=True), None),
    "cubes": lambda: (scenes.cube_field(3, 12, 32, 32), None),
    "meshes": lambda: (meshes.mesh_worlds(3, 32, 32), None),
    "scaled": lambda: (scaled_scene(), (1, 1.0)),
}


def state(name, oracle_mod):
    """(fs, labels, frames, cube) of a scene: a hidden row, labels on some rows, a mount row per world"""
    desc, cube = SCENES[name]()
    fs = oracle_mod.FlatScene(desc)
    rng = np.random.default_rng(len(name))
    n = len(fs.inst_obj)
    labels = np.where(rng.random(n) < 0.5, rng.integers(-3, 50, n), ro.LABEL_OBJECT).astype(np.int32)
    frames = np.zeros(len(fs.world_inst_start) - 1, np.int32)
    for w in range(len(frames)):
        lo, hi = int(fs.world_inst_start[w]), int(fs.world_inst_start[w + 1])
        frames[w] = (w + 1) % (hi - lo) if w != 1 else -1            # world 1 stays in the world frame
        if w == 2:
            fs.inst_obj[hi - 2] = -1                                    # a hidden row
    return fs, labels, frames, cube


@pytest.fixture(scope="module")
def capi(native):
    lib = native.load_capi()
    lib.mrx_trace_rays_host.restype = ctypes.c_int
    lib.mrx_trace_rays_host.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                        ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p,
                                        ctypes.c_void_p]
    lib.mrx_ray_plan.restype = ctypes.c_int
    lib.mrx_ray_plan.argtypes = [ctypes.c_uint32] * 5 + [ctypes.c_int, ctypes.c_void_p]
    for f in (lib.mrx_rays_create, lib.mrx_rays, lib.mrx_trace):
        f.restype = ctypes.c_int
    lib.mrx_rays_create.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
    lib.mrx_rays.argtypes = [ctypes.c_void_p]
    lib.mrx_trace.argtypes = [ctypes.c_void_p]
    return lib


def host_trace(lib, fs, rays, frames, labels, brute):
    rays = np.ascontiguousarray(rays, F)
    W, R = rays.shape[:2]
    n = len(fs.inst_obj)
    inst = (Instance * max(n, 1))()
    for i in range(n):
        inst[i].position[:] = [float(x) for x in fs.inst_pos[i]]
        inst[i].rotation[:] = [float(x) for x in fs.inst_rot[i]]
        inst[i].scale[:] = [float(x) for x in fs.inst_scale[i]]
        inst[i].object_id = int(fs.inst_obj0[i]) if fs.inst_obj[i] >= 0 else -1
    tri = np.ascontiguousarray(fs.tri_pos, F)
    first = np.ascontiguousarray(fs.obj_first_tri, np.int32)
    count = np.ascontiguousarray(fs.obj_num_tris, np.int32)
    start = np.ascontiguousarray(fs.world_inst_start, np.uint32)
    lab = None if labels is None else np.ascontiguousarray(labels, np.int32)
    frm = None if frames is None else np.ascontiguousarray(frames, np.int32)
    t = np.full((W, R), -7.0, F)
    ident = np.full((W, R), -7, np.int32)
    rc = lib.mrx_trace_rays_host(tri.ctypes.data, len(tri), first.ctypes.data, count.ctypes.data, len(first), inst, n,
                                 None if lab is None else lab.ctypes.data, start.ctypes.data, W,
                                 None if frm is None else frm.ctypes.data, rays.ctypes.data, R, int(brute),
                                 t.ctypes.data, ident.ctypes.data)
    assert rc == 0, rc
    return t, ident


# ---- exactness of the host entry --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENES))
def test_the_host_entry_equals_the_numpy_restatement_bit_for_bit(name, capi, oracle_mod):
    fs, labels, frames, cube = state(name, oracle_mod)
    hits = misses = 0
    for R in R_VALUES:
        rays = ro.mixed(fs, R, seed=R, cube=cube)
        # every kind of degenerate ray is there: zero rays, NaNs, tmin >= tmax, zero directions, tmax = inf
        assert R < 63 or all(n > 0 for n in ro.degenerate_kinds(rays)), (R, ro.degenerate_kinds(rays))
        for lab, frm in ((labels, frames), (None, None)):
            want_t, want_id = ro.trace(fs, rays, frm, lab)
            for brute in (0, 1):
                got_t, got_id = host_trace(capi, fs, rays, frm, lab, brute)
                bad = ~((got_t.view(np.uint32) == want_t.view(np.uint32)) | (np.isnan(got_t) & np.isnan(want_t)))
                bad |= got_id != want_id
                assert not bad.any(), (name, R, brute, np.argwhere(bad)[:5], got_t[bad][:5], want_t[bad][:5],
                                       got_id[bad][:5], want_id[bad][:5])
            hits += int((want_id != -1).sum())
            misses += int((want_id == -1).sum())
    assert hits > 100 and misses > 100, (hits, misses)


def test_exact_ties_on_the_cube_grid_go_to_the_lowest_triangle(capi, oracle_mod):
    fs, _, _, cube = state("scaled", oracle_mod)
    row = int(fs.world_inst_start[0]) + cube[0]
    grid = ro.cube_grid(fs.inst_pos[row].astype(np.float64), cube[1], 5)
    rays = np.stack([grid] * 3)
    want_t, want_id = ro.trace(fs, rays)
    # world 0: every ray of the grid meets the top face, z = 2, from z = 9; edges and diagonals included
    assert np.array_equal(want_t[0], np.full(25, 7.0, F)) and np.array_equal(want_id[0], np.zeros(25, np.int32))
    for brute in (0, 1):
        got_t, got_id = host_trace(capi, fs, rays, None, None, brute)
        assert ro.same(got_t, want_t) and np.array_equal(got_id, want_id)


# ---- anchor to the raster oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,make,ground", [
    ("synthetic", lambda: scenes.synthetic_scene(4, 32, 32), 1),
    ("wall", lambda: scenes.synthetic_scene(4, 40, 24, with_wall=True), 1),
    ("cubes", lambda: scenes.cube_field(3, 12, 32, 32), 1),
])
def test_pinhole_rays_reproduce_the_raster_oracle(name, make, ground, oracle_mod):
    fs = oracle_mod.FlatScene(make())
    ref = fs.render()
    seg, depth = ref["segmask"], ref["depth"]
    V, H, Wd = seg.shape
    # the raster oracle's near plane (0.001) as tmin: depth is the view-space distance along +Y, which is t
    rays = np.stack([ro.pinhole(fs, v, tmin=oracle_mod.RASTER_ZNEAR) for v in range(V)])
    t, ident = ro.trace(fs, rays)
    t, ident = t.reshape(V, H, Wd), ident.reshape(V, H, Wd)
    pad = np.pad(seg, ((0, 0), (1, 1), (1, 1)), mode="edge")
    decisive = ((pad[:, :-2, 1:-1] == seg) & (pad[:, 2:, 1:-1] == seg) & (pad[:, 1:-1, :-2] == seg) &
                (pad[:, 1:-1, 2:] == seg))
    covered = seg != -1
    excluded = float((~decisive & covered).sum()) / float(covered.sum())     # the share of the covered pixels left out
    print("%s: excluded %.2f %% of covered pixels" % (name, 100.0 * excluded))
    assert excluded <= 0.20
    assert np.array_equal(ident[decisive], seg[decisive])              # hit / miss agrees with it: -1 is the miss
    on = decisive & covered
    rel = np.abs(t[on].astype(np.float64) - depth[on]) / depth[on]
    is_ground = seg[on] == ground
    print("%s: max relative depth error %.3g off the ground, %.3g on it" %
          (name, rel[~is_ground].max(), rel[is_ground].max() if is_ground.any() else 0.0))
    assert rel[~is_ground].max() <= 2e-6
    assert not is_ground.any() or rel[is_ground].max() <= 3e-4


# ---- known answers --------------------------------------------------------------------------------------------------------
def anchor_quad():
    """S3's anchor: a 10 x 10 quad at y = 10 facing the origin, and a hidden row turned 90 degrees about Z"""
    verts = np.array([[-5, 10, -5], [5, 10, -5], [5, 10, 5], [-5, 10, 5]], F)
    h = float(F(math.sqrt(0.5)))
    return scenes.SceneDesc(
        num_worlds=1, width=64, height=64, mesh_vertices=verts, mesh_uvs=np.zeros((4, 2), F),
        mesh_indices=np.array([0, 1, 2, 0, 2, 3], np.uint32), mesh_vertex_offsets=np.array([0], np.uint32),
        mesh_indices_offsets=np.array([0], np.uint32), mesh_materials=np.array([-1], np.int32),
        instances=[((0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 0),
                   ((0.0, 0.0, 0.0), (h, 0.0, 0.0, h), (1.0, 1.0, 1.0), -1)],
        cameras=[((0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0))], worlds=[(2, 0, 1, 0)])


def test_known_answers_on_the_anchor_quad(capi, oracle_mod):
    fs = oracle_mod.FlatScene(anchor_quad())
    inf = np.inf
    outside = 5.00001           # (o - v0 = 10.00001 is formed in binary32: one ulp of 5 would be rounded away there)
    rays = np.array([[[0, 0, 0, 0, 0, 1, 0, inf],               # straight at it: t = 10 exactly
                      [outside, 0, outside, 0, 0, 1, 0, inf],   # just outside a corner
                      [0, 0, 0, 0, 0, 1, 0, 9.5],               # tmax short of it
                      [0, 0, 0, 0, 0, 1, 0, 10.0],              # t <= tmax is closed
                      [0, 0, 0, 10.0, 0, 1, 0, inf],            # t > tmin is open
                      [0, 0, 0, 0, 0, 2, 0, inf],               # t is the parameter, not the distance
                      [0, 0, 0, 0, 0, 0, 0, 0]]], F)            # the zero ray
    want = ([10.0, inf, 9.5, 10.0, inf, 5.0, 0.0], [0, -1, -1, 0, -1, 0, -1])
    # mounted on the turned row, (1, 0, 0) is the ray that hits; the row is hidden and still carries the rays
    local = np.array([[[0, 0, 0, 0, 1, 0, 0, inf], [0, 0, 0, 0, 0, 1, 0, inf]]], F)
    mount = np.array([1], np.int32)
    for trace in (lambda r, fr: ro.trace(fs, r, fr), lambda r, fr: host_trace(capi, fs, r, fr, None, 0),
                  lambda r, fr: host_trace(capi, fs, r, fr, None, 1)):
        t, ident = trace(rays, None)
        assert t[0].tolist() == want[0] and ident[0].tolist() == want[1]
        t, ident = trace(local, mount)
        assert ident[0].tolist() == [0, -1] and abs(float(t[0, 0]) - 10.0) <= 1e-5 and t[0, 1] == inf


def test_a_nan_tmax_comes_back_a_nan_and_an_infinite_one_as_it_is(capi, oracle_mod):
    fs = oracle_mod.FlatScene(anchor_quad())
    rays = np.array([[[0, 0, 0, 0, 0, 1, 0, np.nan], [0, 0, 0, 0, 0, -1, 0, np.inf], [0, 0, 0, 0, 0, -1, 0, -0.0]]], F)
    for brute in (0, 1):
        t, ident = host_trace(capi, fs, rays, None, None, brute)
        assert np.isnan(t[0, 0]) and t[0, 1] == np.inf and ident[0].tolist() == [-1, -1, -1]
        assert t[0, 2] == 0 and np.signbit(t[0, 2])


# ---- kernel resources -----------------------------------------------------------------------------------------------------
def test_the_trace_kernels_use_no_scratch_and_spill_nothing():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources
    kernels = kernel_resources.resources(os.path.join(ROOT, "madrona_renderer_amd", "csrc", "rays.hip"))
    assert len(kernels) == 2, [k["name"] for k in kernels]              # the culled and the brute form
    for k in kernels:
        assert int(k["ScratchSize [bytes/lane]"]) == 0, k
        assert int(k["VGPRs Spill"]) == 0, k
        assert int(k["VGPRs"]) <= 64, k                                 # 8 waves per SIMD
    # the committed table lists the render kernels only, as before
    table = open(os.path.join(ROOT, "profiles", "kernel_resources_latest.txt")).read()
    assert "rays.hip" not in table


# ---- host logic -----------------------------------------------------------------------------------------------------------
def test_the_launch_checks_and_the_plan(capi):
    out = (ctypes.c_uint32 * 4)()
    plan = lambda *a: capi.mrx_ray_plan(*a, out)
    assert plan(1024, 4096, 0, 256, 0, 0) == 1024 * 16 and list(out) == [16, 1, 64, 1024]
    assert plan(3, 257, 3, 256, 0, 0) == 6 and list(out) == [2, 22, 64, 22 * 1024]
    assert plan(3, 1, 9, 256, 5, 0) == 3 and list(out) == [1, 64, 5, 64 * 1024]
    assert plan(3, 65536, 0, 256, 1000, 0) == 3 * 256 and out[2] == 64      # the table holds 64 rows at most
    assert plan(0, 16, 0, 256, 0, 0) == 0                                   # no world: nothing is enqueued
    for bad in ((4, 0, 0, 256, 0, 0), (4, 65537, 0, 256, 0, 0), (32768, 65536, 0, 256, 0, 0), (4, 16, 0, 0, 0, 0),
                (4, 16, 10, 256, 0, 0), (4, 16, 0, 256, 0, 1)):
        assert plan(*bad) == MRX_E_INVALID, bad
    assert plan(32767, 65536, 0, 256, 0, 0) == 32767 * 256                  # worlds * R just below 2^31
    assert capi.mrx_ray_plan(4, 16, 0, 256, 0, 0, None) == 4


def test_the_entry_points_refuse_a_null_renderer(capi):
    assert capi.mrx_rays_create(None, 16) == MRX_E_INVALID
    assert capi.mrx_rays(None) == MRX_E_INVALID
    assert capi.mrx_trace(None) == MRX_E_INVALID


def test_the_host_entry_checks_its_arguments(capi, oracle_mod):
    fs = oracle_mod.FlatScene(anchor_quad())
    one = np.zeros((1, 1, 8), F)
    f = capi.mrx_trace_rays_host
    tri = np.ascontiguousarray(fs.tri_pos, F)
    first, count = np.array([0], np.int32), np.array([2], np.int32)
    start = np.array([0, 0], np.uint32)
    t, ident = np.zeros(1, F), np.zeros(1, np.int32)
    ok = lambda **kw: f(tri.ctypes.data, kw.get("ntri", 2), first.ctypes.data, kw.get("count", count).ctypes.data, 1, None,
                        0, None, kw.get("start", start).ctypes.data, 1, None, one.ctypes.data, kw.get("R", 1), 0,
                        t.ctypes.data, ident.ctypes.data)
    assert ok() == 0 and ident[0] == -1
    assert ok(R=0) == MRX_E_INVALID and ok(R=65537) == MRX_E_INVALID
    assert ok(count=np.array([3], np.int32)) == MRX_E_INVALID              # an object past the pool's end
    assert ok(start=np.array([0, 1], np.uint32)) == MRX_E_INVALID          # rows past the table's end


def test_the_python_constructor_refuses_anything_but_a_count(native):
    m = native.load_module()
    assert m.MRX_BUF_RAYS == 18 and m.MRX_BUF_RAY_FRAME == 19 and m.MRX_BUF_RAY_DISTANCE == 20
    assert m.MRX_BUF_RAY_ID == 21 and m.MRX_NUM_BUFFERS_EXT7 == 22 and m.MRX_NUM_BUFFERS_EXT6 == 18
    assert scenes.synthetic_scene(2).rays is None
    for bad in (0, -1, 65537, "8", 2.5, True, False, [8]):
        desc = scenes.synthetic_scene(2)
        desc.rays = bad
        with pytest.raises(ValueError, match="rays"):
            scenes.make_renderer(desc)
    if not has_gpu():
        for good in (1, 64, 65536, None):
            desc = scenes.synthetic_scene(2)
            desc.rays = good
            with pytest.raises(RuntimeError, match="no HIP device"):
                scenes.make_renderer(desc)


# ---- the sanitizer build of the host entry, a stand-alone program ---------------------------------------------------------
@pytest.fixture(scope="module")
def driver():
    from madrona_renderer_amd import build
    return build.build_rays_driver()


def _run(exe, *args):
    p = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (args, p.stdout[-2000:], p.stderr[-4000:])
    assert "mismatches 0" in p.stdout and "ERROR" not in p.stderr and "runtime error" not in p.stderr, (p.stdout, p.stderr)
    return p.stdout


def test_sanitized_host_entry_on_the_shipped_assets(driver):
    dd = scenes.DATA_DIR
    out = _run(driver, "assets", os.path.join(dd, "cube.obj"), os.path.join(dd, "plane.obj"),
               os.path.join(dd, "wall_render.obj"), 10000, 1)
    assert "rays 20000" in out


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_sanitized_host_entry_on_adversarial_soups(driver, kind):
    # 3000 triangles (a BLAS of several levels), 20 (flat) and none; degenerate, NaN / infinite and coincident ones
    out = _run(driver, "soup", 3000, 10000, 11 + kind, kind)
    assert "rays 20000" in out
