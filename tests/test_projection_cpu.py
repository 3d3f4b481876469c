"""Per-view projection on the host (no GPU): mrx_projection_constants gives the oracle's S5 constants bit for bit
over a sweep of fovs, near planes, sizes and both modes (the defaults: today's), and every entry point refuses
what is out of range -- mrx_create before it looks for a device."""
import ctypes
import math

import numpy as np
import pytest

from madrona_renderer_amd import scenes
from tests.test_output_select_cpu import Cfg as CfgV2, small_config

MRX_E_INVALID, MRX_E_NO_DEVICE = -1, -2


class Proj(ctypes.Structure):
    _fields_ = [("vfov_deg", ctypes.c_float), ("znear", ctypes.c_float)]


def _capi(native):
    lib = native.load_capi()
    lib.mrx_projection_constants.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, Proj,
                                             ctypes.POINTER(ctypes.c_float)]
    lib.mrx_projection_constants.restype = ctypes.c_int
    lib.mrx_set_view_projection.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(Proj)]
    lib.mrx_view_projection.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(Proj)]
    return lib


def _constants(lib, w, h, mode, fov, znear):
    out = (ctypes.c_float * 6)()
    rc = lib.mrx_projection_constants(w, h, mode, Proj(fov, znear), out)
    return rc, np.array(out[:], np.float32)


def _oracle_constants(oracle, w, h, rt, fov, znear):
    """oracle.projection_constants and FlatScene._struct's near plane / S6b pad under the given globals."""
    saved = (oracle.VFOV_DEG, oracle.RASTER_ZNEAR, oracle.RT_ZNEAR)
    try:
        oracle.VFOV_DEG = float(np.float32(fov))
        if znear:
            oracle.RASTER_ZNEAR = oracle.RT_ZNEAR = float(np.float32(znear))
        hh = w if rt else h
        sx, ox, sz, oz = oracle.projection_constants(w, hh, rt)
        zn = np.float32(oracle.RT_ZNEAR if rt else oracle.RASTER_ZNEAR)
        th = float(np.float32(math.tan(oracle.VFOV_DEG * math.pi / 360.0)))
        asp = float(w) / float(hh)
        pad = np.float32(float(zn) * math.sqrt(1.0 + th * th * (1.0 + asp * asp)) * 1.001)
        return np.array([sx, ox, sz, oz, np.float32(1.0) / zn, pad], np.float32)
    finally:
        oracle.VFOV_DEG, oracle.RASTER_ZNEAR, oracle.RT_ZNEAR = saved


@pytest.mark.parametrize("mode", [0, 1], ids=["raster", "raytracer"])
@pytest.mark.parametrize("size", [(64, 64), (128, 72), (96, 160)])
def test_constants_equal_the_oracles_bit_for_bit(native, oracle_mod, mode, size):
    lib = _capi(native)
    w, h = size
    for fov in (5.0, 30.0, 60.0, 89.5, 90.0, 120.0, 170.0):
        for znear in (0.0, 0.001, 0.01, 0.1, 0.5, 2.0, 7.25, 999.0):
            rc, got = _constants(lib, w, h, mode, fov, znear)
            assert rc == 0, (fov, znear)
            want = _oracle_constants(oracle_mod, w, h, mode == 1, fov, znear)
            assert got.view(np.int32).tolist() == want.view(np.int32).tolist(), (fov, znear, got, want)


@pytest.mark.parametrize("mode", [0, 1])
def test_defaults_are_todays_constants(native, oracle_mod, mode):
    lib = _capi(native)
    rc, got = _constants(lib, 64, 64, mode, 90.0, 0.0)
    assert rc == 0
    # what every view rendered with before: th = tan(45 deg) in float, znear 0.001 / 0.1
    th = float(np.float32(math.tan(90.0 * math.pi / 360.0)))
    zn = np.float32(0.1 if mode else 0.001)
    assert got[4] == np.float32(1.0) / zn
    assert got[0] == np.float32(2.0 * th / 64)
    assert (got == _oracle_constants(oracle_mod, 64, 64, mode == 1, 90.0, 0.0)).all()
    rc2, explicit = _constants(lib, 64, 64, mode, 90.0, float(zn))
    assert rc2 == 0 and explicit.view(np.int32).tolist() == got.view(np.int32).tolist()


@pytest.mark.parametrize("fov", [0.0, 180.0, -30.0, 200.0, float("nan"), float("inf"), -float("inf")])
def test_bad_fov_is_refused(native, fov):
    lib = _capi(native)
    for mode in (0, 1):
        assert _constants(lib, 64, 64, mode, fov, 0.0)[0] == MRX_E_INVALID


@pytest.mark.parametrize("znear", [-0.001, -1.0, float("nan"), float("inf"), -float("inf")])
def test_bad_znear_is_refused(native, znear):
    lib = _capi(native)
    for mode in (0, 1):
        assert _constants(lib, 64, 64, mode, 60.0, znear)[0] == MRX_E_INVALID


def test_raytracer_znear_must_stay_below_its_far_plane(native):
    lib = _capi(native)
    assert _constants(lib, 64, 64, 1, 60.0, 999.0)[0] == 0
    assert _constants(lib, 64, 64, 1, 60.0, 1000.0)[0] == MRX_E_INVALID
    assert _constants(lib, 64, 64, 1, 60.0, 5000.0)[0] == MRX_E_INVALID
    assert _constants(lib, 64, 64, 0, 60.0, 5000.0)[0] == 0          # Rasterizer mode has no far plane
    assert _constants(lib, 64, 64, 2, 60.0, 0.0)[0] == MRX_E_INVALID  # no such mode


def test_null_renderer_and_null_output(native):
    lib = _capi(native)
    p = (Proj * 1)(Proj(60.0, 0.0))
    assert lib.mrx_set_view_projection(None, 0, 1, p) == MRX_E_INVALID
    assert lib.mrx_view_projection(None, 0, 1, p) == MRX_E_INVALID
    assert lib.mrx_projection_constants(64, 64, 0, Proj(60.0, 0.0), None) == MRX_E_INVALID


class Cfg(ctypes.Structure):      # the whole mrx_config: the V2 struct, the ABI 3 fields, camera_projections
    _fields_ = [("v2", CfgV2), ("device_ids", ctypes.c_void_p), ("num_devices", ctypes.c_uint32),
                ("max_instances_per_world", ctypes.c_uint32), ("camera_projections", ctypes.POINTER(Proj))]


V2_SIZE = Cfg.device_ids.offset
V4_SIZE = Cfg.camera_projections.offset


def _create(lib, desc, size, projections=None):
    v2, keep = small_config(desc, 0)
    cfg = Cfg()
    cfg.v2 = v2
    cfg.v2.struct_size = size
    if projections is not None:
        arr = (Proj * len(projections))(*[Proj(f, z) for f, z in projections])
        cfg.camera_projections = arr
        keep = keep + (arr,)
    h = ctypes.c_void_p()
    rc = lib.mrx_create(ctypes.byref(cfg), ctypes.byref(h))
    assert not h.value
    return rc


@pytest.mark.parametrize("mode", ["Rasterizer", "Raytracer"])
def test_config_sizes_v2_v4_and_current_are_accepted_and_projections_checked_first(native, mode):
    """Every size that worked before is accepted (on a machine without a GPU mrx_create then fails on the device
    probe, after every argument check); a bad camera projection is refused before the probe -- but only a caller
    whose struct holds the field passes one."""
    lib = native.load_capi()
    desc = scenes.synthetic_scene(3, render_mode=mode, textured=True)
    assert ctypes.sizeof(Cfg) == V4_SIZE + 8 and V2_SIZE == ctypes.sizeof(CfgV2)
    ok = MRX_E_NO_DEVICE
    for size in (V2_SIZE, V4_SIZE, ctypes.sizeof(Cfg)):
        assert _create(lib, desc, size) == ok, size
    assert _create(lib, desc, V4_SIZE + 4) == MRX_E_INVALID
    good = [(60.0, 0.0), (120.0, 0.5), (90.0, 0.0)]
    assert _create(lib, desc, ctypes.sizeof(Cfg), good) == ok
    for bad in ([(0.0, 0.0)], [(180.0, 0.0)], [(float("nan"), 0.0)], [(60.0, -1.0)], [(60.0, float("inf"))]):
        projs = good[:2] + bad
        assert _create(lib, desc, ctypes.sizeof(Cfg), projs) == MRX_E_INVALID, bad
        # (the V4 and V2 callers pass no projections: the field is not read)
        assert _create(lib, desc, V4_SIZE, projs) == ok
        assert _create(lib, desc, V2_SIZE, projs) == ok
    far = good[:2] + [(60.0, 1000.0)]
    assert _create(lib, desc, ctypes.sizeof(Cfg), far) == (MRX_E_INVALID if mode == "Raytracer" else ok)


def test_python_camera_checks_its_projection(native):
    m = native.load_module()
    c = m.ImportedCamera(position=[0, 0, 0], rotation=[1, 0, 0, 0])
    assert c.vfov == 90.0 and c.znear is None
    c = m.ImportedCamera([0, 0, 0], [1, 0, 0, 0], vfov=60.0, znear=0.5)
    assert c.vfov == 60.0 and c.znear == 0.5
    for bad in (dict(vfov=0.0), dict(vfov=180.0), dict(vfov=float("nan")), dict(vfov=float("inf")),
                dict(znear=0.0), dict(znear=-1.0), dict(znear=float("nan"))):
        with pytest.raises(ValueError):
            m.ImportedCamera([0, 0, 0], [1, 0, 0, 0], **bad)
