"""The point-cloud output's reference: NumPy.  The selection is integer arithmetic on the storage-order
ranks of the valid pixels (Python ints where a product may pass 32 bits); the points are tests/position_oracle.unproject
at the selected pixels, so a filled slot holds by construction what the position oracle gives that pixel."""
import numpy as np

from tests import position_oracle as po

F = np.float32


def valid_mask(depth, max_depth):
    """bool, depth's shape: d > 0 and (no max_depth or d <= max_depth); False for a NaN"""
    d = np.asarray(depth, F)
    with np.errstate(invalid="ignore"):
        ok = d > F(0)
        if max_depth:
            ok &= d <= F(max_depth)
    return ok


def select(valid, n):
    """valid: bool [px] in storage order -> (int64 [n] storage index of every slot's pixel, -1 where empty; M)"""
    idx = np.flatnonzero(valid)
    m = len(idx)
    out = np.full(n, -1, np.int64)
    if m >= n:
        ranks = (np.arange(n, dtype=object) * m) // n           # exact: Python ints
        out[:] = idx[ranks.astype(np.int64)]
    else:
        out[:m] = idx
    return out, m


def cloud(depth, cam_pos, cam_rot, consts, s, frame, raytracer, n, max_depth=None):
    """depth float32 [views, slow, fast] (a trailing 1 is dropped) in storage order -> (points float32 [views, n, 4],
    pixel int32 [views, n], count int32 [views])"""
    d = np.asarray(depth, F)
    if d.ndim == 4:
        d = d[..., 0]
    views, nslow, nfast = d.shape
    pos = po.unproject(d, cam_pos, cam_rot, consts, s, frame, raytracer).reshape(views, nslow * nfast, 4)
    ok = valid_mask(d, max_depth).reshape(views, -1)
    points = np.zeros((views, n, 4), F)
    pixel = np.full((views, n), -1, np.int32)
    count = np.zeros(views, np.int32)
    width = nslow if raytracer else nfast                       # the image's width
    for v in range(views):
        sel, m = select(ok[v], n)
        count[v] = m
        filled = sel >= 0
        i = sel[filled]
        slow, fast = i // nfast, i % nfast
        x, y = (slow, fast) if raytracer else (fast, slow)
        points[v, filled] = pos[v, i]
        pixel[v, filled] = (y * width + x).astype(np.int32)
    return points, pixel, count
