"""The optical-flow output's reference: NumPy float32, every operation a separately rounded binary32
operation in exactly S17's order, so that the flow kernel and the host entry can be compared bit for bit.  Host only.
The row search is S17's rule taken literally: the last row of the view's world whose base is not above the id."""
import numpy as np

from tests.position_oracle import constants, pixel_centres, rotation  # noqa: F401  (constants: re-exported for the tests)

F = np.float32


def find_rows(ids, kbase, lo, hi):
    """ids int32 [...] -> (row int64 [...], found bool [...]): the last row r of [lo, hi) with kbase[r] <= id; found is
    false for a negative id and where no row qualifies (row is then lo, or 0 for an empty world: never used)."""
    k = np.asarray(ids, np.int64)
    bases = np.asarray(kbase[lo:hi], np.int64)
    if hi == lo:
        return np.zeros(k.shape, np.int64), np.zeros(k.shape, bool)
    ok = (bases[(None,) * k.ndim] <= k[..., None]) & (k[..., None] >= 0)
    last = ok.shape[-1] - 1 - np.argmax(ok[..., ::-1], axis=-1)
    found = ok.any(axis=-1)
    return np.where(found, lo + last, lo), found


def _apply(R, v, t):
    """R [..., 3, 3], v and t lists of three [...] arrays: ((R[i][0] v0 + R[i][1] v1) + R[i][2] v2) + t_i"""
    return [((R[..., i, 0] * v[0] + R[..., i, 1] * v[1]) + R[..., i, 2] * v[2]) + t[i] for i in range(3)]


def _apply_t(R, v):
    """the transpose product: (R[0][j] v0 + R[1][j] v1) + R[2][j] v2"""
    return [(R[..., 0, j] * v[0] + R[..., 1, j] * v[1]) + R[..., 2, j] * v[2] for j in range(3)]


def flow(depth, ids, consts, prev_consts, kbase, world_inst_start, view_world, live, prev, s, raytracer):
    """depth float32 / ids int32 [views, slow, fast] in storage order (a trailing 1 of depth is dropped); consts and
    prev_consts float32 [views, 4] (sx ox sz oz); live and prev are (inst_pos [I, 3], inst_rot [I, 4], inst_scale
    [I, 3], cam_pos [views, 3], cam_rot [views, 4]) -> float32 [views, slow, fast, 4]."""
    d_all = np.asarray(depth, F)
    if d_all.ndim == 4:
        d_all = d_all[..., 0]
    ids = np.asarray(ids, np.int32)
    views, nslow, nfast = d_all.shape
    consts, prev_consts = np.asarray(consts, F), np.asarray(prev_consts, F)
    lp, lq, ls, lc, lcq = (np.asarray(a, F) for a in live)
    pp, pq, ps, pc, pcq = (np.asarray(a, F) for a in prev)
    px, py = pixel_centres(nslow, nfast, s, raytracer)
    Rc, Rcp = rotation(lcq), rotation(pcq)
    out = np.zeros((views, nslow, nfast, 4), F)
    one, zero, fs = F(1.0), F(0.0), F(s)
    with np.errstate(all="ignore"):
        for v in range(views):
            d, k = d_all[v], ids[v]
            w = int(view_world[v])
            rows, found = find_rows(k, kbase, int(world_inst_start[w]), int(world_inst_start[w + 1]))
            hit = ~(d == 0) & (k >= 0) & found
            if not found.any():
                continue
            sx, ox, sz, oz = consts[v]
            sxp, oxp, szp, ozp = prev_consts[v]
            # 2: the current point, as S13
            rx = px * sx + ox
            rz = py * sz + oz
            pv = [d * rx, d, d * rz]
            P = _apply(Rc[v], pv, [lc[v, i] for i in range(3)])
            # 4: into the instance's frame, out again with the previous pose
            R, Rp = rotation(lq[rows.ravel()]).reshape(rows.shape + (3, 3)), \
                rotation(pq[rows.ravel()]).reshape(rows.shape + (3, 3))
            u = [P[i] - lp[rows, i] for i in range(3)]
            l = _apply_t(R, u)
            m = [l[i] * (one / ls[rows, i]) for i in range(3)]
            n = [m[i] * ps[rows, i] for i in range(3)]
            Pp = _apply(Rp, n, [pp[rows, i] for i in range(3)])
            # 5: into the previous view
            up = [Pp[i] - pc[v, i] for i in range(3)]
            pvp = _apply_t(Rcp[v], up)
            Y = pvp[1]
            # 6, 7
            valid = hit & (Y > 0)
            pxp = (pvp[0] / Y - oxp) / sxp
            pyp = (pvp[2] / Y - ozp) / szp
            res = [(px - pxp) / fs, (py - pyp) / fs, d - Y, np.full(d.shape, one, F)]
            for c in range(4):
                assert res[c].dtype == F
                out[v, ..., c] = np.where(valid, res[c], zero)
    return out
