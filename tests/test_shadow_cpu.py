"""Cast shadows on the host (no GPU): the host entry mrx_shadow_host -- the kernel's own source,
shadow_core.hpp, run on the CPU -- against the NumPy restatement tests/shadow_oracle.py on every byte of the mask and of
the darkened rgb, culled and brute, in one staging pass and in passes of one row; the launch checks through
mrx_shadow_plan; the ValueErrors of shadows.attach; the kernels' resources as the compiler reports them; and the
sanitizer build of the host entry, run as a stand-alone program.

Depth comes from pinhole rays through tests/ray_oracle.py (t of a pinhole ray is the view depth), normals from the
geometry, so nothing here needs a render."""
import copy
import ctypes
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

from madrona_renderer_amd import scenes
from tests import meshes
from tests import position_oracle as pos
from tests import ray_oracle as ro
from tests import shadow_oracle as so
from tests.conftest import ROOT

F = np.float32
MRX_E_INVALID, MRX_E_UNSUPPORTED = -1, -5
W, H = 24, 20                       # 480 pixels: the second block of 256 is partial
VFOV = 20.0
LIGHT = ((0.4, -0.3, -1.0), 0.25, 0.75)         # slanted off the vertical
CUBE_AT = (0.0, 0.0, 1.5)                       # the unit cube floats: z from 1 to 2


class Instance(ctypes.Structure):
    _fields_ = [("position", ctypes.c_float * 3), ("rotation", ctypes.c_float * 4), ("scale", ctypes.c_float * 3),
                ("object_id", ctypes.c_int32)]


def test_the_constants_the_tests_use_are_the_header_s():
    header = open(os.path.join(ROOT, "include", "mrx.h")).read()
    for text in ("MRX_BUF_SHADOW = 26,", "MRX_NUM_BUFFERS_EXT10 = 27", "MRX_NUM_BUFFERS_EXT9 = 26,",
                 "#define MRX_SHADOW_DEFAULT_BIAS (1.0f / 1024.0f)", "#define MRX_SHADOW_NO_MAX_DISTANCE 3.402823466e+38f",
                 "#define MRX_ABI_VERSION"):
        assert text in header, text
    from madrona_renderer_amd import shadows
    assert shadows.MRX_BUF_SHADOW == 26 and shadows.DEFAULT_BIAS == float(so.DEFAULT_BIAS) == 2.0 ** -10
    assert shadows._FLT_MAX == float(so.FLT_MAX)
    import madrona_renderer_amd
    assert "shadows" in madrona_renderer_amd.__all__ and "cloud" in madrona_renderer_amd.__all__


# ---- scenes -------------------------------------------------------------------------------------------------------------
EYES = ((4.0, -5.0, 5.5), (-5.5, -3.0, 4.5))
TARGET = (0.3, -0.25, 0.6)


def cube_scene(worlds=1, cams=1, mode="Rasterizer", rows3=False, width=W, height=H, vary=False):
    """Per world a plane, the unit cube floating above it and `cams` cameras of VFOV degrees that see cube, shadow and
    lit floor.  rows3: the world's three rows are the plane, the cube at its place (the caller hides it) and a mirrored
    cube.  vary: the cube sits a little elsewhere in every world."""
    dd = scenes.DATA_DIR
    inst, cam, world = [], [], []
    for w in range(worlds):
        i0, c0 = len(inst), len(cam)
        at = (CUBE_AT[0] + 0.125 * (w % 4), CUBE_AT[1] - 0.0625 * (w % 3), CUBE_AT[2] + 0.03125 * w) if vary else CUBE_AT
        inst.append(((0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 1))
        inst.append((at, (1.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 0))
        if rows3:
            inst.append(((0.9, 0.4, 1.3), meshes.random_quat(np.random.default_rng(7 + w)), (-1.0, 1.5, 0.75), 0))
        for c in range(cams):
            cam.append((EYES[c], scenes.look_at(EYES[c], TARGET)))
        world.append((len(inst) - i0, i0, cams, c0))
    return scenes.SceneDesc(num_worlds=worlds, render_mode=mode, width=width, height=width if mode == "Raytracer" else height,
                            asset_paths=[(os.path.join(dd, "cube.obj"), 0), (os.path.join(dd, "plane.obj"), 0)],
                            materials=[((0.6, 0.6, 0.6, 1.0), -1, 0.8, 0.2)], instances=inst, cameras=cam, worlds=world,
                            camera_projections=[(VFOV, None)] * len(cam), world_lights=[LIGHT] * worlds)


def sphere_scene(worlds=1, width=W, height=H):
    """Per world a floor quad and a floating sphere of 144 triangles: an object with a BLAS"""
    sph = meshes.sphere(12, 6, 0.7)
    quad = meshes.grid_mesh(1, 1, lambda u, v: (40.0 * u - 20.0, 40.0 * v - 20.0, 0.0))
    geo = meshes.pack_meshes([(sph[0], sph[1], sph[2], 0), (quad[0], quad[1], quad[2], 0)])
    inst, cam, world = [], [], []
    for w in range(worlds):
        inst.append(((0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 1))
        inst.append((CUBE_AT, meshes.random_quat(np.random.default_rng(3 + w)), (1.0, 1.2, 0.9), 0))
        cam.append((EYES[w % 2], scenes.look_at(EYES[w % 2], TARGET)))
        world.append((2, 2 * w, 1, w))
    return scenes.SceneDesc(num_worlds=worlds, width=width, height=height, asset_paths=[],
                            materials=[((0.6, 0.6, 0.6, 1.0), -1, 0.8, 0.2)], instances=inst, cameras=cam, worlds=world,
                            camera_projections=[(VFOV, None)] * worlds, world_lights=[LIGHT] * worlds, **geo)


@dataclasses.dataclass
class Case:
    """What one call of the stage reads"""
    fs: object
    depth: np.ndarray               # [views, slow, fast]
    consts: np.ndarray              # [views, 4]
    lights: np.ndarray              # [views, 5]
    s: int = 1
    rt: bool = False
    bias: float = float(so.DEFAULT_BIAS)
    max_distance: object = None

    @property
    def cam_pos(self):
        return self.fs.cam_pos

    @property
    def cam_rot(self):
        return self.fs.cam_rot

    @property
    def view_world(self):
        return np.ascontiguousarray(self.fs.view_world, np.uint32)


def pinhole_depth(fs, consts, s, rt, nslow, nfast):
    """float32 [views, slow, fast]: the view depth along pinhole rays through S13's pixel centres (t of the ray
    (rx, 1, rz) turned by the camera), 0 where the ray meets nothing"""
    px, py = pos.pixel_centres(nslow, nfast, s, rt)
    out = np.zeros((fs.num_views, nslow, nfast), F)
    for v in range(fs.num_views):
        sx, ox, sz, oz = (F(c) for c in consts[v])
        rx, rz = (px * sx + ox).ravel(), (py * sz + oz).ravel()
        one = np.ones_like(rx)
        Rc = ro.rotation(fs.cam_rot[v])
        rays = np.zeros((1, rx.size, 8), F)
        rays[0, :, 0:3] = fs.cam_pos[v]
        rays[0, :, 3] = F(0.001)
        for r in range(3):
            rays[0, :, 4 + r] = (Rc[r][0] * rx + Rc[r][1] * one) + Rc[r][2] * rz
        rays[0, :, 7] = np.inf
        t, ident = ro.trace(so._world_of(fs, int(fs.view_world[v])), rays)
        out[v] = np.where(ident[0] != -1, t[0], F(0)).reshape(nslow, nfast)
    return out


def make_case(desc, oracle_mod, lights=None, projections=None, s=1, hide=None, **kw):
    fs = oracle_mod.FlatScene(desc)
    for row in hide or ():
        fs.inst_obj[row] = -1
    rt = fs.raytracer
    nslow, nfast = (fs.width, fs.width) if rt else (fs.height, fs.width)
    proj = projections or [(VFOV, None)] * fs.num_views
    consts = pos.constants(fs.width, fs.height, rt, proj, s)
    per_world = lights or [LIGHT] * desc.num_worlds
    rec = so.light_records(per_world)[np.asarray(fs.view_world)]
    return Case(fs, pinhole_depth(fs, consts, s, rt, nslow, nfast), consts, rec, s=s, rt=rt, **kw)


# ---- the host entry -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def capi(native):
    lib = native.load_capi()
    lib.mrx_shadow_host.restype = ctypes.c_int
    lib.mrx_shadow_host.argtypes = ([ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                     ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32] +
                                    [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int,
                                     ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.c_float, ctypes.c_float, ctypes.c_uint32, ctypes.c_int,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p])
    lib.mrx_shadow_plan.restype = ctypes.c_int
    lib.mrx_shadow_plan.argtypes = [ctypes.c_uint32] * 7 + [ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_int,
                                                           ctypes.c_void_p]
    for f in (lib.mrx_shadows, lib.mrx_shadow):
        f.restype = ctypes.c_int
        f.argtypes = [ctypes.c_void_p]
    lib.mrx_shadow_create.restype = ctypes.c_int
    lib.mrx_shadow_create.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_float]
    return lib


def host_shadow(lib, case, pass_rows=0, brute=0, rgb=None, normal=None, expect=0):
    fs = case.fs
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
    depth = np.ascontiguousarray(case.depth, F)
    views, nslow, nfast = depth.shape
    consts, lights = np.ascontiguousarray(case.consts, F), np.ascontiguousarray(case.lights, F)
    cam_pos, cam_rot = np.ascontiguousarray(case.cam_pos, F), np.ascontiguousarray(case.cam_rot, F)
    view_world = case.view_world
    mask = np.full((views, nslow, nfast), 7, np.uint8)
    out_rgb = None if rgb is None else np.ascontiguousarray(rgb).copy()
    nrm = None if normal is None else np.ascontiguousarray(normal)
    tmax = float(so.FLT_MAX) if case.max_distance is None else case.max_distance
    rc = lib.mrx_shadow_host(tri.ctypes.data, len(tri), first.ctypes.data, count.ctypes.data, len(first), inst, n,
                             start.ctypes.data, len(start) - 1, depth.ctypes.data, views, nfast, nslow, int(case.rt),
                             case.s, consts.ctypes.data, cam_pos.ctypes.data, cam_rot.ctypes.data, view_world.ctypes.data,
                             lights.ctypes.data, case.bias, tmax, pass_rows, brute,
                             None if out_rgb is None else out_rgb.ctypes.data, None if nrm is None else nrm.ctypes.data,
                             mask.ctypes.data)
    assert rc == expect, rc
    return mask, out_rgb


def oracle_mask(case):
    return so.mask(case.fs, case.depth, case.cam_pos, case.cam_rot, case.consts, case.s, case.rt, case.view_world,
                   case.lights, case.bias, case.max_distance)


FORMS = [(0, 0), (0, 1), (1, 0), (1, 1)]            # (brute, pass_rows)


def assert_every_form(lib, case, want, rgb=None, normal=None, want_rgb=None, what=""):
    for brute, pass_rows in FORMS:
        got, got_rgb = host_shadow(lib, case, pass_rows, brute, rgb, normal)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, (what, brute, pass_rows, len(bad), bad[:5], got[got != want][:5])
        if want_rgb is not None:
            bad = np.argwhere(got_rgb != want_rgb)
            assert len(bad) == 0, (what, brute, pass_rows, len(bad), bad[:5])


def shares(case, mask):
    hit = case.depth > 0
    return float(((mask == 0) & hit).sum()) / float(hit.sum()), float(((mask == 255) & hit).sum()) / float(hit.sum())


def geometry_normals(case):
    """uint8 [views, slow, fast, 4]: S10's bytes of a scene of a plane and axis-aligned unit cubes, from the pixel's
    world point: the floor's normal is +Z, a cube's the axis its point is farthest out on; turned to face the eye,
    taken into view space (S2's axes), b = (uint)(c * 127 + 128.5); background (128, 128, 128, 0)"""
    fs = case.fs
    p = pos.unproject(case.depth, case.cam_pos, case.cam_rot, case.consts, case.s, "world", case.rt).astype(np.float64)
    out = np.zeros(case.depth.shape + (4,), np.uint8)
    out[..., :3] = 128
    R = pos.rotation(case.cam_rot).astype(np.float64)
    for v in range(fs.num_views):
        pts = p[v, ..., :3]
        n = np.zeros_like(pts)
        n[..., 2] = 1.0
        local = pts - np.asarray(CUBE_AT)
        on_cube = (np.abs(local).max(axis=-1) < 0.5 + 1e-3) & (pts[..., 2] > 0.5)
        axis = np.abs(local).argmax(axis=-1)
        cube_n = np.zeros_like(pts)
        np.put_along_axis(cube_n, axis[..., None], np.sign(np.take_along_axis(local, axis[..., None], -1)), -1)
        n = np.where(on_cube[..., None], cube_n, n)
        to_eye = np.asarray(case.cam_pos[v], np.float64) - pts
        n = np.where((n * to_eye).sum(-1, keepdims=True) < 0, -n, n)
        nv = n @ R[v]                                           # Rc^T n
        hit = case.depth[v] > 0
        b = np.clip(nv, -1, 1) * 127.0 + 128.5
        out[v, ..., :3] = np.where(hit[..., None], b.astype(np.uint32), 128).astype(np.uint8)
        out[v, ..., 3] = np.where(hit, 255, 0)
    return out


# ---- the base scene, and the condition that keeps the tests from passing on nothing --------------------------------------
@pytest.fixture(scope="module")
def base(oracle_mod):
    case = make_case(cube_scene(), oracle_mod)
    return case, oracle_mask(case)


def test_the_base_scene_has_shadow_and_light_by_the_oracle_alone(base):
    case, want = base
    assert case.depth.shape == (1, H, W) and case.depth.size == 480
    dark, lit = shares(case, want)
    print("occluded %.1f %% of the hit pixels, lit %.1f %%" % (100 * dark, 100 * lit))
    assert dark >= 0.05 and lit >= 0.05
    # the floor under the light-side of the cube is in shadow although nothing of its own is in the way: a cast shadow
    floor = (case.depth > 0) & (pos.unproject(case.depth, case.cam_pos, case.cam_rot, case.consts, 1, "world", False)[..., 2]
                                < 0.01)
    assert ((want == 0) & floor).sum() >= 8 and ((want == 255) & floor).sum() >= 8


def test_the_host_entry_is_the_oracle_s_on_every_byte(capi, base):
    case, want = base
    assert_every_form(capi, case, want, what="base")


def test_apply_darkens_what_the_diffuse_term_had_lit_and_nothing_else(capi, base):
    case, want = base
    normal = geometry_normals(case)
    rgb = np.zeros(case.depth.shape + (4,), np.uint8)
    rgb[..., 3] = 255
    rgb[case.depth > 0] = (200, 150, 101, 255)
    want_rgb, kept = so.apply(rgb, normal, want, case.cam_rot, case.lights)
    changed = (want_rgb != rgb).any(axis=-1)
    print("apply changes %d pixels, keeps %d occluded ones (lit <= ambient)" % (changed.sum(), kept.sum()))
    assert changed.sum() >= 1 and kept.sum() >= 1               # by the oracle alone
    assert not changed[want == 255].any() and (want_rgb[..., 3] == rgb[..., 3]).all()
    # the floor in shadow: n . l = toLight.z, lit = 0.75 * toLight.z + 0.25, to within the normal's quantisation
    f = 0.25 / (0.75 * float(case.lights[0, 2]) + 0.25)
    floor_shadow = changed & (normal[..., 2] > 200)
    assert floor_shadow.any() and np.abs(want_rgb[floor_shadow][:, 0].astype(float) - 200 * f).max() <= 1.5
    as_u32 = lambda a: np.ascontiguousarray(a).view(np.uint32).reshape(a.shape[:3])
    assert_every_form(capi, case, want, as_u32(rgb), as_u32(normal), as_u32(want_rgb), what="apply")


# ---- variants -------------------------------------------------------------------------------------------------------------
def _hidden_and_mirrored(oracle_mod):
    return make_case(cube_scene(rows3=True), oracle_mod, hide=[1])


def _two_worlds(oracle_mod):
    return make_case(cube_scene(worlds=2), oracle_mod, lights=[LIGHT, ((-0.5, 0.2, -1.0), 0.0, 1.0)])


VARIANTS = {
    "three-rows-hidden-mirrored": _hidden_and_mirrored,
    "blas-object": lambda om: make_case(sphere_scene(), om),
    "two-cameras": lambda om: make_case(cube_scene(cams=2), om),
    "transposed": lambda om: make_case(cube_scene(mode="Raytracer"), om),
    "per-view-projections": lambda om: make_case(cube_scene(cams=2), om, projections=[(20.0, None), (100.0, 0.05)]),
    "two-worlds-two-lights": _two_worlds,
    "s2": lambda om: make_case(cube_scene(), om, s=2),
    "bias-0": lambda om: make_case(cube_scene(), om, bias=0.0),
    "short-max-distance": lambda om: make_case(cube_scene(), om, max_distance=0.4),
}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_variants_in_every_form(capi, oracle_mod, name):
    case = VARIANTS[name](oracle_mod)
    want = oracle_mask(case)
    dark, lit = shares(case, want)
    print("%s: occluded %.1f %%, lit %.1f %%" % (name, 100 * dark, 100 * lit))
    assert lit > 0
    if name == "short-max-distance":
        # 0.4 is short of the cube's distance to the floor along the light (> 1): the floor holds no shadow
        p = pos.unproject(case.depth, case.cam_pos, case.cam_rot, case.consts, 1, "world", False)
        assert not ((want == 0) & (case.depth > 0) & (p[..., 2] < 0.01)).any()
    else:
        assert dark > 0.02
    if name == "blas-object":
        assert int(case.fs.obj_num_tris[0]) > 32
    if name == "per-view-projections":
        assert (case.depth[1] == 0).any() and (want[1][case.depth[1] == 0] == 255).all()    # the wide view sees the sky
    if name == "three-rows-hidden-mirrored":
        # the hidden cube casts nothing -- the same depth over the scene with the row shown, but far away, gives the
        # same mask -- and shown where it is, it would
        for place, same in (((5000.0, 5000.0, 5000.0), True), (CUBE_AT, False)):
            shown = dataclasses.replace(case, fs=copy.deepcopy(case.fs))
            shown.fs.inst_obj[1] = shown.fs.inst_obj0[1]
            shown.fs.inst_pos[1] = place
            assert np.array_equal(oracle_mask(shown), want) == same, place
        assert (case.fs.inst_scale[2] < 0).any()
    if name == "two-worlds-two-lights":
        assert not np.array_equal(want[0], want[1]) and case.lights[1, 3] == 0
    rng = np.random.default_rng(len(name))
    # the geometry's normals where the scene is the plane and the unrotated cube, any bytes elsewhere
    normal = geometry_normals(case) if name not in ("blas-object", "three-rows-hidden-mirrored") else \
        rng.integers(0, 256, case.depth.shape + (4,), dtype=np.uint8)
    rgb = rng.integers(0, 256, case.depth.shape + (4,), dtype=np.uint8)
    want_rgb, _ = so.apply(rgb, normal, want, case.cam_rot, case.lights)
    as_u32 = lambda a: np.ascontiguousarray(a).view(np.uint32).reshape(a.shape[:3])
    assert_every_form(capi, case, want, as_u32(rgb), as_u32(normal), as_u32(want_rgb), what=name)


def test_degenerate_rays_leave_255(capi, oracle_mod):
    """a zero light direction and NaN, negative, infinite and zero depths: nothing is accepted, whatever the form"""
    case = make_case(cube_scene(worlds=2), oracle_mod)
    case.lights[1, :3] = 0.0
    d = case.depth[0]
    hit = np.argwhere(d > 0)
    for k, value in enumerate((np.nan, -1.0, np.inf, -np.inf, 0.0, -0.0)):
        for y, x in hit[k::6][:8]:
            d[y, x] = value
    want = oracle_mask(case)
    assert (want[1] == 255).all() and (want[0] == 0).any()
    assert (want[0][~(d > 0)] == 255).all()
    assert_every_form(capi, case, want, what="degenerate")
    # random bytes as normals and colours: the applying form keeps every pixel of the view without a light direction
    rng = np.random.default_rng(5)
    rgb = rng.integers(0, 2 ** 32, case.depth.shape, dtype=np.uint32)
    normal = rng.integers(0, 2 ** 32, case.depth.shape, dtype=np.uint32)
    to_u8 = lambda a: a.view(np.uint8).reshape(a.shape + (4,))
    want_rgb, _ = so.apply(to_u8(rgb), to_u8(normal), want, case.cam_rot, case.lights)
    want_rgb = np.ascontiguousarray(want_rgb).view(np.uint32).reshape(rgb.shape)
    assert np.array_equal(want_rgb[1], rgb[1]) and (want_rgb[0] != rgb[0]).any()
    assert_every_form(capi, case, want, rgb, normal, want_rgb, what="degenerate, apply")


def test_the_host_entry_checks_its_arguments(capi, base):
    case, _ = base
    host_shadow(capi, dataclasses.replace(case, bias=-1.0), expect=MRX_E_INVALID)
    host_shadow(capi, dataclasses.replace(case, bias=float("nan")), expect=MRX_E_INVALID)
    host_shadow(capi, dataclasses.replace(case, max_distance=0.0), expect=MRX_E_INVALID)
    host_shadow(capi, dataclasses.replace(case, max_distance=float("inf")), expect=MRX_E_INVALID)
    host_shadow(capi, dataclasses.replace(case, s=5), expect=MRX_E_INVALID)
    rgb = np.zeros(case.depth.shape, np.uint32)
    host_shadow(capi, case, rgb=rgb, normal=None, expect=MRX_E_INVALID)          # rgb and normals: both or neither


# ---- plan, refusals, resources -----------------------------------------------------------------------------------------------
def test_the_launch_checks_and_the_plan(capi):
    out = (ctypes.c_uint32 * 4)()
    bias, far = 2.0 ** -10, float(so.FLT_MAX)

    def plan(views, nfast, nslow, s=1, depth=0, cus=256, pass_rows=0, apply=0, bias=bias, far=far, bad=0):
        return capi.mrx_shadow_plan(views, nfast, nslow, s, depth, cus, pass_rows, apply, bias, far, bad, out)

    assert plan(1024, 64, 64) == 1024 * 16 and list(out) == [16, 1, 64, 1024]
    assert plan(1, 24, 20) == 2 and list(out) == [2, 1, 64, 1024]             # 480 pixels: a full block and a partial one
    assert plan(3, 24, 20, depth=3, pass_rows=5, apply=1) == 6 and list(out) == [2, 22, 5, 22 * 1024]
    assert plan(3, 1, 1, depth=9, pass_rows=1000) == 3 and list(out) == [1, 64, 64, 64 * 1024]
    assert plan(0, 64, 64) == 0 and plan(4, 0, 64) == 0                         # no pixel: nothing is enqueued
    assert plan(4, 64, 64, far=1.5) == 64 and plan(4, 64, 64, bias=0.0) == 64
    assert plan(4, 64, 64, s=4) == 64
    for bad in (dict(s=0), dict(s=5), dict(depth=10), dict(cus=0), dict(bad=1), dict(bad=2), dict(bad=3, apply=1),
                dict(bias=-2.0 ** -10), dict(bias=float("inf")), dict(bias=float("nan")), dict(far=0.0), dict(far=-1.0),
                dict(far=float("inf")), dict(far=float("nan"))):
        assert plan(4, 64, 64, **bad) == MRX_E_INVALID, bad
    assert plan(4, 64, 64, bad=3, apply=0) == 64                                # rgb is not looked at without apply
    assert plan(65536, 256, 256) == MRX_E_INVALID                               # 2^32 native pixels
    assert plan(65535, 256, 256) == 65535 * 256                                 # 2^32 - 65536
    assert capi.mrx_shadow_plan(4, 64, 64, 1, 0, 256, 0, 0, bias, far, 0, None) == 64


def test_the_entry_points_refuse_a_null_renderer(capi):
    assert capi.mrx_shadow_create(None, 1, 2.0 ** -10, float(so.FLT_MAX)) == MRX_E_INVALID
    assert capi.mrx_shadows(None) == MRX_E_INVALID
    assert capi.mrx_shadow(None) == MRX_E_INVALID


class _StandIn:
    def native_handle(self):
        raise AssertionError("reached the renderer")


@pytest.mark.parametrize("kw,names", [
    (dict(apply=1), ["apply"]), (dict(apply=None), ["apply"]), (dict(apply="yes"), ["apply"]),
    (dict(bias=-0.001), ["bias"]), (dict(bias=float("nan")), ["bias"]), (dict(bias=float("inf")), ["bias"]),
    (dict(bias="0"), ["bias"]), (dict(bias=True), ["bias"]), (dict(bias=1e300), ["bias", "single precision"]),
    (dict(max_distance=0), ["max_distance"]), (dict(max_distance=-1.0), ["max_distance"]),
    (dict(max_distance=float("inf")), ["max_distance"]), (dict(max_distance=float("nan")), ["max_distance"]),
    (dict(max_distance="far"), ["max_distance"]), (dict(max_distance=True), ["max_distance"]),
    (dict(max_distance=1e-60), ["max_distance", "single precision"]),
    (dict(max_distance=1e60), ["max_distance", "single precision"]),
])
def test_attach_checks_its_arguments_before_any_native_call(native, kw, names):
    from madrona_renderer_amd import shadows
    with pytest.raises(ValueError) as e:
        shadows.attach(_StandIn(), **kw)
    for name in names:
        assert name in str(e.value), (kw, str(e.value))


def test_good_arguments_reach_the_renderer(native):
    from madrona_renderer_amd import shadows
    assert shadows._check_arguments(True, 2 ** -10, None) == (1, 2.0 ** -10, float(so.FLT_MAX))
    assert shadows._check_arguments(False, 0, 3) == (0, 0.0, 3.0)
    for kw in (dict(), dict(apply=False), dict(bias=0), dict(bias=0.5, max_distance=2), dict(max_distance=0.25)):
        with pytest.raises(AssertionError, match="reached the renderer"):
            shadows.attach(_StandIn(), **kw)


def test_cloud_keeps_its_names_over_the_shared_dlpack_module(native):
    """the DLPack helpers moved to a module both outputs import; the unsigned 8-bit type is new there"""
    torch = pytest.importorskip("torch")
    from madrona_renderer_amd import _dlpack, cloud, shadows
    assert cloud._Exported is _dlpack.Exported and cloud._LIVE is _dlpack._LIVE and shadows._dlpack is _dlpack
    assert _dlpack.DTYPES[0] == (_dlpack.kDLUInt, 8)
    backing = np.arange(24, dtype=np.uint8).reshape(2, 3, 4)
    t = torch.from_dlpack(_dlpack.Exported(backing.ctypes.data, backing.shape, _dlpack.kDLUInt, 8, _dlpack.kDLCPU, 0,
                                           backing))
    assert t.dtype == torch.uint8 and tuple(t.shape) == (2, 3, 4) and t.data_ptr() == backing.ctypes.data
    backing[1, 2, 3] = 200
    assert t[1, 2, 3].item() == 200
    del t


def test_the_binding_s_surface_is_untouched(native):
    m = native.load_module()
    assert not hasattr(m, "MRX_BUF_SHADOW") and not hasattr(m, "MRX_NUM_BUFFERS_EXT10")
    assert not hasattr(m.MadronaRenderer, "shadow_tensor")


def test_the_shadow_kernels_use_no_scratch_and_spill_no_vgpr():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources
    kernels = kernel_resources.resources(os.path.join(ROOT, "madrona_renderer_amd", "csrc", "shadow.hip"))
    assert len(kernels) == 4, [k["name"] for k in kernels]              # APPLY x BRUTE
    names = sorted(k["name"].split("(")[0] for k in kernels)
    assert names == ["shadowKernel<false, false>", "shadowKernel<false, true>", "shadowKernel<true, false>",
                     "shadowKernel<true, true>"], names
    for k in kernels:
        assert int(k["ScratchSize [bytes/lane]"]) == 0, k
        assert int(k["VGPRs Spill"]) == 0, k
        assert int(k["VGPRs"]) <= 64, k                                 # 8 waves per SIMD by registers
        # 64 staged rows of 128 bytes and, but for the brute form, 32 triangle records of 64 bytes per wave; the stacks
        # are dynamic
        brute = k["name"].split("(")[0].endswith(", true>")
        assert int(k["LDS Size [bytes/block]"]) == 64 * 128 + (0 if brute else 4 * 32 * 64), k
    committed = open(os.path.join(ROOT, "profiles", "kernel_resources_shadow.txt")).read()
    for k in kernels:
        assert k["name"].split("(")[0] in committed
    # the committed table of the render kernels lists them only, as before
    assert "shadow.hip" not in open(os.path.join(ROOT, "profiles", "kernel_resources_latest.txt")).read()


# ---- the sanitizer build of the host entry, a stand-alone program ---------------------------------------------------------
def test_sanitized_host_entry_on_assets_and_adversarial_soups():
    from madrona_renderer_amd import build
    exe = build.build_shadow_driver()
    dd = scenes.DATA_DIR
    runs = [("assets", os.path.join(dd, "cube.obj"), os.path.join(dd, "plane.obj"), os.path.join(dd, "wall_render.obj"), 48, 1)]
    runs += [("soup", 3000, 40, 11 + kind, kind) for kind in range(4)]      # cloud, degenerate, NaN / infinite, coincident
    for args in runs:
        p = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, (args, p.stdout[-2000:], p.stderr[-4000:])
        assert "mismatches 0" in p.stdout and "ERROR" not in p.stderr and "runtime error" not in p.stderr, (p.stdout, p.stderr)
        assert ("pixels 9792" if args[0] == "assets" else "pixels 6880") in p.stdout
