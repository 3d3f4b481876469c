"""Per-world light on the host (no GPU): mrx_light_constants gives the oracle's light vector bit for bit (the
default: today's three words), every entry point refuses what is out of range -- mrx_create before it looks for a
device -- every mrx_config size that was accepted stays accepted, and the helper the GPU tests compare against
(tests/light_oracle.py) is anchored to known answers and to a float64 shading model under the world's light."""
import ctypes
import math

import numpy as np
import pytest

from madrona_renderer_amd import scenes
from tests import light_oracle as lo
from tests.golden.make_golden import cases
from tests.test_independent_raycast import quat_to_mat, raycast_view
from tests.test_output_select_cpu import small_config
from tests.test_projection_cpu import Cfg as CfgProj

MRX_E_INVALID, MRX_E_NO_DEVICE = -1, -2
NAN, INF = float("nan"), float("inf")


class Light(ctypes.Structure):
    _fields_ = [("direction", ctypes.c_float * 3), ("ambient", ctypes.c_float), ("diffuse", ctypes.c_float)]


def _light(d, a, f):
    return Light((ctypes.c_float * 3)(*d), a, f)


def _capi(native):
    lib = native.load_capi()
    lib.mrx_light_constants.argtypes = [Light, ctypes.POINTER(ctypes.c_float)]
    lib.mrx_light_constants.restype = ctypes.c_int
    lib.mrx_set_world_light.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(Light)]
    lib.mrx_world_light.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(Light)]
    return lib


def _constants(lib, d, a=0.25, f=0.75):
    out = (ctypes.c_float * 5)()
    rc = lib.mrx_light_constants(_light(d, a, f), out)
    return rc, np.array(out[:], np.float32)


def _oracle_constants(oracle, d, a, f):
    saved = (oracle.LIGHT_DIR, oracle.AMBIENT, oracle.DIFFUSE)
    try:
        oracle.LIGHT_DIR = tuple(float(x) for x in d)
        oracle.AMBIENT, oracle.DIFFUSE = float(np.float32(a)), float(np.float32(f))
        return np.concatenate([oracle.to_light_vector(), np.array([oracle.AMBIENT, oracle.DIFFUSE], np.float32)])
    finally:
        oracle.LIGHT_DIR, oracle.AMBIENT, oracle.DIFFUSE = saved


def test_defaults_are_todays_constants(native, oracle_mod):
    lib = _capi(native)
    rc, got = _constants(lib, (1.0, -1.0, -0.05))
    assert rc == 0
    # what every world was lit with before: the oracle's module constants, untouched
    assert (oracle_mod.LIGHT_DIR, oracle_mod.AMBIENT, oracle_mod.DIFFUSE) == ((1.0, -1.0, -0.05), 0.25, 0.75)
    want = np.concatenate([oracle_mod.to_light_vector(), np.array([0.25, 0.75], np.float32)])
    assert got.view(np.int32).tolist() == want.view(np.int32).tolist()
    d = np.array([1.0, -1.0, -0.05])
    assert got[:3].view(np.int32).tolist() == (-d / math.sqrt(float(d @ d))).astype(np.float32).view(np.int32).tolist()


def test_constants_equal_the_oracles_bit_for_bit(native, oracle_mod):
    lib = _capi(native)
    rng = np.random.default_rng(20261016)
    n = 10000
    dirs = rng.standard_normal((n, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    dirs = (dirs * 10.0 ** rng.uniform(-3, 3, n)[:, None]).astype(np.float32)      # lengths 1e-3 ... 1e3
    amb = rng.uniform(0, 1.5, n).astype(np.float32)
    dif = rng.uniform(0, 1.5, n).astype(np.float32)
    bad = 0
    for d, a, f in zip(dirs, amb, dif):
        rc, got = _constants(lib, d, a, f)
        assert rc == 0, (d, a, f)
        want = _oracle_constants(oracle_mod, d, a, f)
        bad += got.view(np.int32).tolist() != want.view(np.int32).tolist()
    assert bad == 0, f"{bad} of {n} lights differ from the oracle's"
    # unit length is reached to float rounding whatever the length given
    for d in ((1e-3, 0, 0), (0, 1e3, 0), (3.0, 4.0, 0.0)):
        rc, got = _constants(lib, d)
        assert rc == 0 and abs(float(np.linalg.norm(got[:3].astype(np.float64))) - 1.0) < 1e-6


@pytest.mark.parametrize("light", [
    ((0.0, 0.0, 0.0), 0.25, 0.75), ((0.0, -0.0, 0.0), 0.25, 0.75),
    ((NAN, 0.0, 1.0), 0.25, 0.75), ((0.0, INF, 1.0), 0.25, 0.75), ((0.0, 1.0, -INF), 0.25, 0.75),
    ((1.0, 0.0, 0.0), NAN, 0.75), ((1.0, 0.0, 0.0), INF, 0.75), ((1.0, 0.0, 0.0), -INF, 0.75),
    ((1.0, 0.0, 0.0), 0.25, NAN), ((1.0, 0.0, 0.0), 0.25, INF), ((1.0, 0.0, 0.0), 0.25, -INF),
    ((1.0, 0.0, 0.0), -0.01, 0.75), ((1.0, 0.0, 0.0), 0.25, -1.0)])
def test_bad_lights_are_refused(native, light):
    lib = _capi(native)
    assert _constants(lib, *light)[0] == MRX_E_INVALID


def test_zero_ambient_and_zero_diffuse_are_accepted(native):
    lib = _capi(native)
    assert _constants(lib, (0.0, 0.0, -1.0), 0.0, 0.0)[0] == 0
    rc, got = _constants(lib, (0.0, 0.0, -2.0), 0.0, 3.0)
    assert rc == 0 and got.tolist() == [0.0, 0.0, 1.0, 0.0, 3.0]


def test_null_renderer_and_null_pointers(native):
    lib = _capi(native)
    one = (Light * 1)(_light((1.0, 0.0, 0.0), 0.25, 0.75))
    assert lib.mrx_set_world_light(None, 0, 1, one) == MRX_E_INVALID
    assert lib.mrx_world_light(None, 0, 1, one) == MRX_E_INVALID
    assert lib.mrx_light_constants(_light((1.0, 0.0, 0.0), 0.25, 0.75), None) == MRX_E_INVALID


class Cfg(ctypes.Structure):      # the whole mrx_config: the struct as it was with camera_projections, world_lights
    _fields_ = [("prev", CfgProj), ("world_lights", ctypes.POINTER(Light))]


V2_SIZE = CfgProj.device_ids.offset
V4_SIZE = CfgProj.camera_projections.offset
PREV_SIZE = ctypes.sizeof(CfgProj)


def _create(lib, desc, size, lights=None):
    v2, keep = small_config(desc, 0)
    cfg = Cfg()
    cfg.prev.v2 = v2
    cfg.prev.v2.struct_size = size
    if lights is not None:
        arr = (Light * len(lights))(*[_light(*l) for l in lights])
        cfg.world_lights = arr
        keep = keep + (arr,)
    h = ctypes.c_void_p()
    rc = lib.mrx_create(ctypes.byref(cfg), ctypes.byref(h))
    assert not h.value
    return rc


@pytest.mark.parametrize("mode", ["Rasterizer", "Raytracer"])
def test_every_config_size_stays_accepted_and_lights_are_checked_first(native, mode):
    """The accepted sizes are an exact set: V2, V4, V4 + 8 (the struct as it was with camera_projections) and the
    current one; on a machine without a GPU mrx_create then fails on the device probe, after every argument check.
    A bad light is refused before the probe -- but only a caller whose struct holds the field passes one."""
    lib = native.load_capi()
    desc = scenes.synthetic_scene(3, render_mode=mode, textured=True)
    assert PREV_SIZE == V4_SIZE + 8 and ctypes.sizeof(Cfg) == V4_SIZE + 16 and ctypes.sizeof(Light) == 20
    ok = MRX_E_NO_DEVICE
    accepted = (V2_SIZE, V4_SIZE, PREV_SIZE, ctypes.sizeof(Cfg))
    for size in accepted:
        assert _create(lib, desc, size) == ok, size
    for size in range(V2_SIZE - 4, ctypes.sizeof(Cfg) + 12, 4):
        if size not in accepted:
            assert _create(lib, desc, size) == MRX_E_INVALID, size
    good = [((0.0, 0.0, -1.0), 0.1, 0.9), lo.DEFAULT, ((2.0, 3.0, -4.0), 0.0, 1.0)]
    assert _create(lib, desc, ctypes.sizeof(Cfg), good) == ok
    for bad in (((0.0, 0.0, 0.0), 0.25, 0.75), ((NAN, 0.0, 0.0), 0.25, 0.75), ((1.0, 0.0, INF), 0.25, 0.75),
                ((1.0, 0.0, 0.0), -0.5, 0.75), ((1.0, 0.0, 0.0), 0.25, -0.5), ((1.0, 0.0, 0.0), NAN, 0.75),
                ((1.0, 0.0, 0.0), 0.25, INF)):
        lights = good[:2] + [bad]
        assert _create(lib, desc, ctypes.sizeof(Cfg), lights) == MRX_E_INVALID, bad
        # (the callers of the older sizes pass no lights: the field is not read)
        for size in accepted[:3]:
            assert _create(lib, desc, size, lights) == ok, (size, bad)


def test_scene_desc_world_lights_of_the_wrong_length_raise(native):
    desc = scenes.synthetic_scene(4)
    desc.world_lights = lo.mixed(3)
    with pytest.raises(ValueError):
        scenes.make_renderer(desc)
    desc.world_lights = lo.mixed(5)
    with pytest.raises(ValueError):
        scenes.make_renderer(desc)


# ---- anchors of the helper: known answers, not self-comparison ---------------------------------------------------

def _to_u8(c):
    c = np.clip(np.asarray(c, np.float32), np.float32(0), np.float32(1))
    # fmaf(c, 255, 0.5): exact in double, rounded once to float, truncated
    return (c.astype(np.float64) * 255.0 + 0.5).astype(np.float32).astype(np.uint8)


def _material_rgb(fs, desc, v):
    """The bare material colour of the triangle each pixel of view v sees, as bytes (untextured scenes)."""
    w = int(fs.view_world[v])
    cols = []
    for i in range(fs.world_inst_start[w], fs.world_inst_start[w + 1]):
        obj = int(fs.inst_obj[i])
        f0, n = int(fs.obj_first_tri[obj]), int(fs.obj_num_tris[obj])
        for ti in range(f0, f0 + n):
            cols.append(fs.mat_color[int(fs.tri_mat[ti])][:3])
    return np.asarray(cols, np.float32)


def test_ambient_only_gives_the_bare_material_colour(oracle_mod):
    desc = scenes.synthetic_scene(4)
    fs = oracle_mod.FlatScene(desc)
    for d in ((1.0, -1.0, -0.05), (0.0, 0.0, 1.0), (-3.0, 0.5, 0.25)):
        out = lo.render(desc, [(d, 1.0, 0.0)] * 4)
        for v in range(4):
            tri = out["tri_id"][v]
            cols = _to_u8(_material_rgb(fs, desc, v))
            hit = tri >= 0
            assert hit.any()
            assert np.array_equal(out["rgb"][v][hit][:, :3], cols[tri[hit]])
            assert (out["rgb"][v][hit][:, 3] == 255).all()


def test_light_from_above_gives_the_ground_its_full_brightness(oracle_mod):
    desc = scenes.synthetic_scene(4)
    fs = oracle_mod.FlatScene(desc)
    # (instance 0 of every world is the plane: the world's first triangles are the upward z = 0 ground quad)
    nplane = int(fs.obj_num_tris[1])
    for a, f in ((0.1, 0.9), (0.25, 0.5), (0.9, 0.9)):
        out = lo.render(desc, [((0.0, 0.0, -1.0), a, f)] * 4)
        lit = np.float32(np.float32(f) * np.float32(1.0) + np.float32(a))
        for v in range(4):
            tri = out["tri_id"][v]
            ground = (tri >= 0) & (tri < nplane)
            assert ground.sum() > 500
            want = _to_u8(lit * _material_rgb(fs, desc, v)[0])
            assert (out["rgb"][v][ground][:, :3] == want[None, :]).all()


def test_the_light_changes_colour_only(oracle_mod):
    desc = scenes.synthetic_scene(12, with_wall=True)
    plain = oracle_mod.FlatScene(desc).render()
    out = lo.render(desc, lo.mixed(12))
    assert np.array_equal(out["tri_id"], plain["tri_id"])
    assert np.array_equal(out["depth"].view(np.uint32), plain["depth"].view(np.uint32))
    # the default's worlds keep today's pixels; the others do not
    for w, light in enumerate(lo.mixed(12)):
        same = np.array_equal(out["rgb"][w], plain["rgb"][w])
        assert same == (light == lo.DEFAULT), w
    # ... and the globals are restored
    assert (oracle_mod.LIGHT_DIR, oracle_mod.AMBIENT, oracle_mod.DIFFUSE) == ((1.0, -1.0, -0.05), 0.25, 0.75)


def test_helper_merges_lights_and_projections(oracle_mod):
    from tests import projection_oracle as po
    desc = scenes.synthetic_scene(6)
    projs = po.mixed(6)
    lights = lo.mixed(6, shift=3)
    out = lo.render(desc, lights, projs)
    geo = po.render(desc, projs)
    assert np.array_equal(out["tri_id"], geo["tri_id"]) and np.array_equal(out["depth"], geo["depth"])
    assert (out["rgb"] != geo["rgb"]).any()
    # one world at a time, directly under the oracle's globals
    for w in (1, 4):
        saved = (oracle_mod.LIGHT_DIR, oracle_mod.AMBIENT, oracle_mod.DIFFUSE)
        try:
            d, a, f = lights[w]
            oracle_mod.LIGHT_DIR = tuple(float(np.float32(x)) for x in d)
            oracle_mod.AMBIENT, oracle_mod.DIFFUSE = float(np.float32(a)), float(np.float32(f))
            one = po.render(desc, projs, w, w + 1)
        finally:
            oracle_mod.LIGHT_DIR, oracle_mod.AMBIENT, oracle_mod.DIFFUSE = saved
        assert np.array_equal(one["rgb"][w], out["rgb"][w])


# ---- a float64 shading model under the world's light -------------------------------------------------------------

def raycast_colour_lit(fs, v, light):
    """tests/test_independent_raycast.py::raycast_colour with the world's light in place of the fixed one: (rgb
    [H,W,3] float64 prediction in 0..255 before rounding, sure_tex [H,W]) of the nearest hit per pixel in float64 --
    world-space normal turned towards the eye, one directional light travelling along `direction`, ambient +
    diffuse * max(n.l, 0), material colour, nearest texel of the barycentric uv with v up, clamped to [0, 1]."""
    direction, ambient, diffuse = light
    W, H = fs.width, fs.height
    w = int(fs.view_world[v])
    Rc = quat_to_mat(fs.cam_rot[v])
    c = fs.cam_pos[v].astype(np.float64)
    th = math.tan(math.radians(45.0))
    px = (np.arange(W) + 0.5) / W * 2 - 1
    py = 1 - (np.arange(H) + 0.5) / H * 2
    X, Z = np.meshgrid(px * th * (W / H), py * th)
    dirs = np.stack([X, np.ones_like(X), Z], axis=-1) @ Rc.T
    to_light = -np.asarray([float(np.float32(x)) for x in direction])
    to_light /= np.linalg.norm(to_light)
    ambient, diffuse = float(np.float32(ambient)), float(np.float32(diffuse))
    rt = fs.raytracer
    near, far = (0.1, 1000.0) if rt else (0.001, np.inf)
    best = np.full((H, W), np.inf)
    rgb = np.zeros((H, W, 3))
    sure_tex = np.ones((H, W), bool)
    for i in range(fs.world_inst_start[w], fs.world_inst_start[w + 1]):
        obj = int(fs.inst_obj[i])
        if obj < 0 or obj >= len(fs.obj_first_tri):
            continue
        M = quat_to_mat(fs.inst_rot[i]) * fs.inst_scale[i].astype(np.float64)[None, :]
        t = fs.inst_pos[i].astype(np.float64)
        f0, n = int(fs.obj_first_tri[obj]), int(fs.obj_num_tris[obj])
        for ti in range(f0, f0 + n):
            P = fs.tri_pos[ti].astype(np.float64) @ M.T + t
            e1, e2 = P[1] - P[0], P[2] - P[0]
            pvec = np.cross(dirs, e2)
            det = pvec @ e1
            with np.errstate(divide="ignore", invalid="ignore"):
                inv = 1.0 / det
                tvec = c - P[0]
                u = (pvec @ tvec) * inv
                qvec = np.cross(tvec, e1)
                vv = (dirs @ qvec) * inv
                tt = (qvec @ e2) * inv
            ok = (np.abs(det) > 0) & (np.minimum(np.minimum(u, vv), 1 - u - vv) >= 0) & (tt >= near) & (tt <= far)
            closer = ok & (tt < best)
            nrm = np.cross(e1, e2)
            ln = np.linalg.norm(nrm)
            if not closer.any() or ln == 0:
                continue
            if nrm @ (c - P[0]) < 0:
                nrm = -nrm
            lit = ambient + diffuse * max(float(nrm @ to_light) / ln, 0.0)
            mi = int(fs.tri_mat[ti])
            col, tex = np.ones(3), -1
            if 0 <= mi < len(fs.mat_color):
                col, tex = fs.mat_color[mi][:3].astype(np.float64), int(fs.mat_tex[mi])
            if not (0 <= tex < fs.num_textures):
                val = np.broadcast_to(255.0 * np.clip(lit * col, 0, 1), (H, W, 3))
                st = np.ones((H, W), bool)
            else:
                uv = fs.tri_uv[ti].astype(np.float64)
                U = (1 - u - vv) * uv[0, 0] + u * uv[1, 0] + vv * uv[2, 0]
                V = (1 - u - vv) * uv[0, 1] + u * uv[1, 1] + vv * uv[2, 1]
                tw_, th_ = int(fs.tex_w[tex]), int(fs.tex_h[tex])
                with np.errstate(invalid="ignore"):
                    fu = (U - np.floor(U)) * tw_
                    fv = (1.0 - (V - np.floor(V))) * th_
                    st = (np.abs(fu - np.round(fu)) > 2e-3) & (np.abs(fv - np.round(fv)) > 2e-3)
                    tx = np.clip(np.nan_to_num(fu).astype(np.int64), 0, tw_ - 1)
                    ty = np.clip(np.nan_to_num(fv).astype(np.int64), 0, th_ - 1)
                texel = fs.tex_data[int(fs.tex_offset[tex]) + ty * tw_ + tx][..., :3].astype(np.float64)
                val = 255.0 * np.clip(texel / 255.0 * lit * col, 0, 1)
            rgb = np.where(closer[..., None], val, rgb)
            sure_tex = np.where(closer, st, sure_tex)
            best = np.where(closer, tt, best)
    if rt:
        return np.transpose(rgb, (1, 0, 2)), sure_tex.T
    return rgb, sure_tex


LIGHTS = (((0.0, 0.0, -1.0), 0.1, 0.9), ((-2.0, 1.0, -0.5), 0.4, 0.5), ((0.3, 0.8, -0.2), 0.9, 0.9))


@pytest.mark.parametrize("light", range(len(LIGHTS)))
@pytest.mark.parametrize("name", ["synthetic_wall_textured_64", "demo_raytracer_64"])
def test_colours_agree_with_a_float64_shading_model_under_the_worlds_light(oracle_mod, name, light):
    """S4 / S7 / S8 from first principles under a non-default light: where visibility and texel choice are decisive
    the helper's bytes are the float64 colour's (a colour within 0.02 of a rounding boundary may land on either
    side), and more than 90 % of the covered pixels are decisive, as in tests/test_independent_raycast.py."""
    desc = cases()[name]
    fs = oracle_mod.FlatScene(desc)
    ref = lo.render(desc, [LIGHTS[light]] * desc.num_worlds)
    checked = hits = 0
    for v in range(min(fs.num_views, 2)):
        tri, depth, margin = raycast_view(fs, v)
        rgb, sure_tex = raycast_colour_lit(fs, v, LIGHTS[light])
        # decisive: the nearest hit is unambiguous in float64 (that file's margin, 1e-6: the oracle names the same
        # triangle there, whatever the light) and so is the texel
        sure = (margin > 1e-6) & sure_tex & (tri >= 0)
        got = ref["rgb"][v][..., :3].astype(np.float64)
        diff = np.abs(got - np.floor(rgb + 0.5))
        near_half = np.abs(rgb - np.floor(rgb) - 0.5) < 0.02
        bad = sure[..., None] & (diff > np.where(near_half, 1.0, 0.0))
        assert not bad.any(), f"view {v}: {int(bad.any(axis=-1).sum())} decisive pixels differ, max {diff[sure].max()}"
        checked += int(sure.sum())
        hits += int((ref["tri_id"][v] >= 0).sum())
    print(f"{name} light {light}: {checked} decisive of {hits} covered")
    assert checked > 0.9 * hits > 0, f"only {checked} of {hits} covered pixels were decisive"
