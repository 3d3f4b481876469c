"""The position output's reference: NumPy float32, every operation a separately rounded binary32
operation in exactly S13's order, so that the unprojection kernel can be compared bit for bit.  Host only: the
projection constants come from the library's own host function (mrx_projection_constants, no device needed) for the
SAMPLE size s*W x s*H -- the constants the render used."""
import ctypes

import numpy as np

F = np.float32


class Proj(ctypes.Structure):
    _fields_ = [("vfov_deg", ctypes.c_float), ("znear", ctypes.c_float)]


def constants(width, height, raytracer, projections, s=1):
    """float32 [views, 4]: sx, ox, sz, oz of each (vfov, znear or None) in `projections` for views of width x height
    native pixels rendered at factor s (Raytracer mode: width x width)."""
    import madrona_renderer_amd
    lib = madrona_renderer_amd.load_capi()
    lib.mrx_projection_constants.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, Proj,
                                             ctypes.POINTER(ctypes.c_float)]
    lib.mrx_projection_constants.restype = ctypes.c_int
    out = np.zeros((len(projections), 4), F)
    buf = (ctypes.c_float * 6)()
    for v, (fov, znear) in enumerate(projections):
        rc = lib.mrx_projection_constants(s * width, s * (width if raytracer else height), 1 if raytracer else 0,
                                          Proj(float(fov), 0.0 if znear is None else float(znear)), buf)
        assert rc == 0, (fov, znear)
        out[v] = buf[:4]
    return out


def rotation(q):
    """S1: R(q) of float32 quaternions [views, 4] (w, x, y, z), used as given, in binary32 -> [views, 3, 3]"""
    q = np.asarray(q, F)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    x2, y2, z2 = x + x, y + y, z + z
    xx, yy, zz = x * x2, y * y2, z * z2
    xy, xz, yz = x * y2, x * z2, y * z2
    wx, wy, wz = w * x2, w * y2, w * z2
    one = F(1.0)
    R = np.empty((len(q), 3, 3), F)
    R[:, 0, 0] = one - (yy + zz); R[:, 0, 1] = xy - wz;          R[:, 0, 2] = xz + wy
    R[:, 1, 0] = xy + wz;          R[:, 1, 1] = one - (xx + zz); R[:, 1, 2] = yz - wx
    R[:, 2, 0] = xz - wy;          R[:, 2, 1] = yz + wx;          R[:, 2, 2] = one - (xx + yy)
    return R


def pixel_centres(nslow, nfast, s, raytracer):
    """(px, py) float32 [slow, fast] of S13: the index of sample (s*x + s//2, s*y + s//2), whose centre S5's ox / oz make
    of it (they carry the half pixel, as in the render kernels); storage [y][x], Raytracer mode [x][y]."""
    slow, fast = np.meshgrid(np.arange(nslow, dtype=np.uint32), np.arange(nfast, dtype=np.uint32), indexing="ij")
    x, y = (slow, fast) if raytracer else (fast, slow)
    half = np.uint32(s // 2)
    px = (np.uint32(s) * x + half).astype(F)
    py = (np.uint32(s) * y + half).astype(F)
    return px, py


def unproject(depth, cam_pos, cam_rot, consts, s, frame, raytracer):
    """depth float32 [views, slow, fast] (a trailing 1 is dropped) in storage order, cam_pos [views, 3], cam_rot
    [views, 4], consts [views, 4] (constants() above), frame "world" or "view" -> float32 [views, slow, fast, 4]."""
    assert frame in ("world", "view")
    d = np.asarray(depth, F)
    if d.ndim == 4:
        d = d[..., 0]
    views, nslow, nfast = d.shape
    consts = np.asarray(consts, F)
    px, py = pixel_centres(nslow, nfast, s, raytracer)
    sx, ox, sz, oz = (consts[:, k][:, None, None] for k in range(4))
    rx = px[None] * sx + ox
    rz = py[None] * sz + oz
    pv = [d * rx, d, d * rz]
    if frame == "world":
        R = rotation(cam_rot)
        c = np.asarray(cam_pos, F)
        p = [((R[:, r, 0][:, None, None] * pv[0] + R[:, r, 1][:, None, None] * pv[1]) + R[:, r, 2][:, None, None] * pv[2])
             + c[:, r][:, None, None] for r in range(3)]
    else:
        p = pv
    hit = ~(d == 0)
    out = np.zeros((views, nslow, nfast, 4), F)
    for k in range(3):
        assert p[k].dtype == F
        out[..., k] = np.where(hit, p[k], F(0))
    out[..., 3] = np.where(hit, F(1), F(0))
    return out
