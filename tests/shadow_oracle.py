"""The shadow stage's reference: NumPy float32, every operation a separately rounded binary32 operation
in exactly S19's order, on top of tests/position_oracle.py (the pixel's world point, S13) and tests/ray_oracle.py (the
triangle test over a world's candidate rows, S16) -- brute force, no box, no BLAS, no cull -- so that the shadow kernel
and the host entry can be compared on every byte.  Works on the arrays of oracle.FlatScene(desc); depth, cameras,
constants and lights are arguments."""
import ctypes
import types

import numpy as np

from tests import position_oracle as pos
from tests import ray_oracle as ro

F = np.float32
FLT_MAX = F(3.402823466e+38)
DEFAULT_BIAS = F(2.0 ** -10)


class Light(ctypes.Structure):
    _fields_ = [("direction", ctypes.c_float * 3), ("ambient", ctypes.c_float), ("diffuse", ctypes.c_float)]


def light_records(lights):
    """float32 [n, 5] = (toLight xyz, ambient, diffuse) of each (direction, ambient, diffuse) in `lights`, resolved by
    the library's own host function (mrx_light_constants, no device needed)"""
    import madrona_renderer_amd
    lib = madrona_renderer_amd.load_capi()
    lib.mrx_light_constants.argtypes = [Light, ctypes.POINTER(ctypes.c_float)]
    lib.mrx_light_constants.restype = ctypes.c_int
    out = np.zeros((len(lights), 5), F)
    buf = (ctypes.c_float * 5)()
    for i, (d, a, f) in enumerate(lights):
        rc = lib.mrx_light_constants(Light((ctypes.c_float * 3)(*[float(x) for x in d]), float(a), float(f)), buf)
        assert rc == 0, (d, a, f)
        out[i] = buf[:]
    return out


def _world_of(fs, w):
    """`fs` narrowed to world w: what ro.trace walks as its world 0"""
    return types.SimpleNamespace(world_inst_start=np.asarray([fs.world_inst_start[w], fs.world_inst_start[w + 1]]),
                                 inst_obj0=fs.inst_obj0, inst_obj=fs.inst_obj, inst_scale=fs.inst_scale,
                                 inst_rot=fs.inst_rot, inst_pos=fs.inst_pos, obj_first_tri=fs.obj_first_tri,
                                 obj_num_tris=fs.obj_num_tris, tri_pos=fs.tri_pos)


def mask(fs, depth, cam_pos, cam_rot, consts, s, raytracer, view_world, lights, bias=DEFAULT_BIAS, max_distance=None):
    """depth float32 [views, slow, fast] (a trailing 1 is dropped) in storage order, cameras and consts as
    position_oracle.unproject takes them, view_world [views], lights float32 [views, 5] (light_records of each view's
    world) -> uint8 [views, slow, fast]: 0 where the pixel is occluded, 255 elsewhere"""
    d = np.asarray(depth, F)
    if d.ndim == 4:
        d = d[..., 0]
    views, nslow, nfast = d.shape
    lights = np.asarray(lights, F)
    tmax = FLT_MAX if max_distance is None else F(max_distance)
    with np.errstate(all="ignore"):
        p = pos.unproject(d, cam_pos, cam_rot, consts, s, "world", raytracer)
        out = np.full((views, nslow, nfast), 255, np.uint8)
        for v in range(views):
            z = d[v].ravel()
            hit = z > 0                                         # false for a NaN
            rays = np.zeros((1, z.size, 8), F)
            rays[0, :, 0:3] = p[v, :, :, :3].reshape(-1, 3)
            rays[0, :, 3] = F(bias) * z
            rays[0, :, 4:7] = lights[v, :3]
            rays[0, :, 7] = tmax
            _, ident = ro.trace(_world_of(fs, int(view_world[v])), rays)
            out[v] = np.where(hit & (ident[0] != -1), 0, 255).astype(np.uint8).reshape(nslow, nfast)
    return out


def apply(rgb, normal, shadow_mask, cam_rot, lights):
    """rgb, normal uint8 [views, slow, fast, 4], shadow_mask uint8 [views, slow, fast], cam_rot [views, 4], lights
    [views, 5] -> (rgb with every occluded pixel darkened by S19's rule, the bool map of occluded pixels whose bytes
    the rule keeps because lit <= ambient)"""
    rgb = np.asarray(rgb, np.uint8)
    n = np.asarray(normal, np.uint8)
    lights = np.asarray(lights, F)
    R = pos.rotation(cam_rot)                                   # [views, 3, 3]
    L = [lights[:, k] for k in range(3)]
    lv = [(R[:, 0, c] * L[0] + R[:, 1, c] * L[1]) + R[:, 2, c] * L[2] for c in range(3)]
    c = [(n[..., i].astype(F) - F(128.0)) / F(127.0) for i in range(3)]
    b = lambda x: x[:, None, None]
    ndl = (c[0] * b(lv[0]) + c[1] * b(lv[1])) + c[2] * b(lv[2])
    ambient, diffuse = b(lights[:, 3]), b(lights[:, 4])
    lit = diffuse * np.maximum(ndl, F(0)) + ambient
    assert lit.dtype == F and ndl.dtype == F
    occluded = np.asarray(shadow_mask) == 0
    darken = occluded & (lit > ambient)
    with np.errstate(all="ignore"):
        f = ambient / lit
        out = rgb.copy()
        for i in range(3):
            scaled = (rgb[..., i].astype(F) * f + F(0.5))
            out[..., i] = np.where(darken, np.where(darken, scaled, F(0)).astype(np.uint32), rgb[..., i]).astype(np.uint8)
    return out, occluded & ~darken
