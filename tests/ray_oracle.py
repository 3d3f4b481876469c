"""The ray-cast sensor's reference: NumPy float32, every operation a separately rounded binary32
operation in exactly S16's order, brute force over a world's candidate triangles -- no box, no BLAS, no cull -- so that
the trace kernel and the host entry can be compared bit for bit.  Works on the arrays of oracle.FlatScene(desc); labels
and frames are arguments.  Also the seeded ray generators the tests share."""
import math

import numpy as np

F = np.float32
LABEL_OBJECT = -2 ** 31


def rotation(q):
    """S1: R(q) of a float32 quaternion (w, x, y, z), used as given, in binary32 -> [3][3] of float32 scalars"""
    w, x, y, z = (F(c) for c in q)
    x2, y2, z2 = x + x, y + y, z + z
    xx, yy, zz = x * x2, y * y2, z * z2
    xy, xz, yz = x * y2, x * z2, y * z2
    wx, wy, wz = w * x2, w * y2, w * z2
    one = F(1.0)
    return [[one - (yy + zz), xy - wz, xz + wy],
            [xy + wz, one - (xx + zz), yz - wx],
            [xz - wy, yz + wx, one - (xx + yy)]]


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def world_rays(fs, w, rays_w, frame):
    """The rays of world w, [R, 8], out of the frame of mount row `frame` -> (o [3][R], d [3][R])"""
    lo, hi = int(fs.world_inst_start[w]), int(fs.world_inst_start[w + 1])
    ol = [rays_w[:, c] for c in range(3)]
    dl = [rays_w[:, 4 + c] for c in range(3)]
    if 0 <= frame < hi - lo:
        row = lo + frame
        Rf = rotation(fs.inst_rot[row])
        p = fs.inst_pos[row]
        o = [((Rf[r][0] * ol[0] + Rf[r][1] * ol[1]) + Rf[r][2] * ol[2]) + p[r] for r in range(3)]
        d = [(Rf[r][0] * dl[0] + Rf[r][1] * dl[1]) + Rf[r][2] * dl[2] for r in range(3)]
        return o, d
    return ol, dl


def trace(fs, rays, frames=None, labels=None):
    """rays float32 [worlds, R, 8]; frames int32 [worlds] or None (world frame); labels int32 [instances] or None
    -> (t float32 [worlds, R], id int32 [worlds, R])"""
    rays = np.asarray(rays, F)
    W, R = rays.shape[0], rays.shape[1]
    out_t = np.empty((W, R), F)
    out_id = np.full((W, R), -1, np.int32)
    nobj = len(fs.obj_first_tri)
    with np.errstate(all="ignore"):
        for w in range(W):
            lo, hi = int(fs.world_inst_start[w]), int(fs.world_inst_start[w + 1])
            o, d = world_rays(fs, w, rays[w], -1 if frames is None else int(frames[w]))
            tmin, tmax = rays[w, :, 3], rays[w, :, 7]
            best_t = np.zeros(R, F)
            best_id = np.full(R, -1, np.int32)
            has = np.zeros(R, bool)
            for row in range(lo, hi):
                bound = int(fs.inst_obj0[row])
                drawn = 0 <= bound < nobj
                count = int(fs.obj_num_tris[bound]) if drawn else 0
                s = fs.inst_scale[row]
                if not (fs.inst_obj[row] >= 0 and count > 0 and np.all(s != 0) and np.all(np.isfinite(s))):
                    continue
                first = int(fs.obj_first_tri[bound])
                lab = LABEL_OBJECT if labels is None else int(labels[row])
                ident = bound if lab == LABEL_OBJECT else lab
                Ri = rotation(fs.inst_rot[row])
                ti = fs.inst_pos[row]
                inv_s = [F(1.0) / F(s[c]) for c in range(3)]
                wv = [o[c] - ti[c] for c in range(3)]
                oi = [((Ri[0][c] * wv[0] + Ri[1][c] * wv[1]) + Ri[2][c] * wv[2]) * inv_s[c] for c in range(3)]
                di = [((Ri[0][c] * d[0] + Ri[1][c] * d[1]) + Ri[2][c] * d[2]) * inv_s[c] for c in range(3)]
                oi = [np.asarray(x, F)[None, :] for x in oi]
                di = [np.asarray(x, F)[None, :] for x in di]
                V = fs.tri_pos[first:first + count]                     # [T, 3, 3]
                v0 = [V[:, 0, c][:, None] for c in range(3)]
                e1 = [V[:, 1, c][:, None] - v0[c] for c in range(3)]
                e2 = [V[:, 2, c][:, None] - v0[c] for c in range(3)]
                p = _cross(di, e2)
                det = _dot(e1, p)
                inv = F(1.0) / det
                sv = [oi[c] - v0[c] for c in range(3)]
                u = _dot(sv, p) * inv
                q = _cross(sv, e1)
                v = _dot(di, q) * inv
                t = _dot(e2, q) * inv
                assert t.dtype == F and u.dtype == F and v.dtype == F
                acc = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > tmin[None, :]) & (t <= tmax[None, :])
                any_acc = acc.any(axis=0)
                tm = np.where(acc, t, F(np.inf)).min(axis=0)
                # rows come in row order, triangles in object order: k only grows, so an equal t never replaces
                better = any_acc & (~has | (tm < best_t))
                best_t = np.where(better, tm, best_t)
                best_id = np.where(better, np.int32(ident), best_id)
                has |= any_acc
            out_t[w] = np.where(has, best_t, tmax)
            # (np.where keeps a NaN tmax a NaN; its payload is compared as a value by the tests, not as bits)
            out_id[w] = np.where(has, best_id, -1)
    return out_t, out_id


# ---- generators: every one returns float32 [n, 8] = (ox, oy, oz, tmin, dx, dy, dz, tmax) --------------------------------
def _pack(o, d, tmin=0.0, tmax=np.inf):
    o, d = np.asarray(o, F).reshape(-1, 3), np.asarray(d, F).reshape(-1, 3)
    r = np.zeros((len(o), 8), F)
    r[:, 0:3] = o
    r[:, 3] = tmin
    r[:, 4:7] = d
    r[:, 7] = tmax
    return r


def _unit(v):
    v = np.asarray(v, np.float64)
    n = np.linalg.norm(v, axis=-1, keepdims=True)
    return v / np.where(n == 0, 1.0, n)


def world_bounds(fs, w):
    """(centre [3], extent) of world w: its instance positions, the ground quad's size left out"""
    lo, hi = int(fs.world_inst_start[w]), int(fs.world_inst_start[w + 1])
    p = fs.inst_pos[lo:hi].astype(np.float64)
    if len(p) == 0:
        return np.zeros(3), 1.0
    c = p.mean(axis=0)
    return c, float(np.abs(p - c).max()) + 3.0


def pinhole(fs, view, tmin=0.0, tmax=np.inf):
    """(a) rays through the pixel centres of view `view`, [H * W, 8] in image order (row 0 up): d = R(q_cam) * (px*sx+ox,
    1, py*sz+oz), every step in float32, so t is the view depth"""
    from oracle import oracle
    width, height = fs.width, fs.height
    sx, ox, sz, oz = oracle.projection_constants(width, height, fs.raytracer)
    y, x = np.meshgrid(np.arange(height, dtype=np.uint32), np.arange(width, dtype=np.uint32), indexing="ij")
    px, py = x.astype(F).ravel(), y.astype(F).ravel()
    rx, rz = px * F(sx) + F(ox), py * F(sz) + F(oz)
    one = np.ones_like(rx)
    Rc = rotation(fs.cam_rot[view])
    d = np.stack([(Rc[r][0] * rx + Rc[r][1] * one) + Rc[r][2] * rz for r in range(3)], axis=1)
    o = np.broadcast_to(fs.cam_pos[view], d.shape)
    return _pack(o, d, tmin, tmax)


def aimed(fs, w, n, rng):
    """(b) random origins around the scene, aimed at random points inside its bounds; unit directions"""
    c, e = world_bounds(fs, w)
    o = c + rng.uniform(-2.5, 2.5, (n, 3)) * e
    target = c + rng.uniform(-1, 1, (n, 3)) * e * [1, 1, 0.3]
    return _pack(o, _unit(target - o), 0.0, 1e4)


def axis_parallel(fs, w, n, rng):
    """(c) axis-parallel rays: one or two direction components exactly 0"""
    c, e = world_bounds(fs, w)
    o = c + rng.uniform(-1.5, 1.5, (n, 3)) * e
    o[:, 2] = np.abs(o[:, 2]) + 0.5
    d = np.zeros((n, 3))
    axis = rng.integers(0, 3, n)
    sign = np.where(c[axis] > o[np.arange(n), axis], 1.0, -1.0)
    d[np.arange(n), axis] = sign
    two = rng.random(n) < 0.5                       # half of them: a second non-zero component
    other = (axis + 1 + rng.integers(0, 2, n)) % 3
    d[np.arange(n)[two], other[two]] = rng.uniform(-1, 1, int(two.sum()))
    return _pack(o, d, 0.0, np.inf)


def inside_boxes(fs, w, n, rng):
    """(d) origins inside instance boxes (at the instance's position, jittered by a fraction of its scale)"""
    lo, hi = int(fs.world_inst_start[w]), int(fs.world_inst_start[w + 1])
    if hi == lo:
        return aimed(fs, w, n, rng)
    rows = rng.integers(lo, hi, n)
    s = np.nan_to_num(np.abs(fs.inst_scale[rows].astype(np.float64)), posinf=1.0)
    o = fs.inst_pos[rows].astype(np.float64) + rng.uniform(-0.3, 0.3, (n, 3)) * np.minimum(s, 4.0)
    return _pack(o, _unit(rng.normal(size=(n, 3))), 0.0, np.inf)


def cube_grid(centre, half, n, height=8.0):
    """(e) a downward grid of n x n rays (n odd) over the top face of an axis-aligned, unrotated cube of half-size `half`
    (a power of two) at `centre`: the outer lines coincide with its edges, the diagonals with the shared edges of the
    face's triangles -- exact t ties, decided by the lowest k"""
    assert n % 2 == 1
    k = (np.arange(n) - n // 2) * (2.0 * half / (n - 1))
    gx, gy = np.meshgrid(k, k, indexing="ij")
    o = np.stack([centre[0] + gx.ravel(), centre[1] + gy.ravel(), np.full(n * n, centre[2] + height)], axis=1)
    return _pack(o, np.broadcast_to([0.0, 0.0, -1.0], o.shape), 0.0, 64.0)


DEGENERATE_KINDS = 6


def degenerate(fs, w, n, rng, first=0):
    """(f) rays aimed at the scene and then spoilt, kind (first + i) mod 6 for ray i: 0 the zero ray, 1 a NaN in one of
    the eight components (the component advances with i), 2 tmin == tmax, 3 tmin > tmax, 4 a zero direction from a
    non-zero origin, 5 a good ray with tmax = inf"""
    r = aimed(fs, w, n, rng)
    for i in range(n):
        kind = (first + i) % DEGENERATE_KINDS
        if kind == 0:
            r[i] = 0
        elif kind == 1:
            r[i, ((first + i) // DEGENERATE_KINDS) % 8] = np.nan
        elif kind == 2:
            r[i, 3], r[i, 7] = 5.0, 5.0
        elif kind == 3:
            r[i, 3], r[i, 7] = 1e3, 1.0
        elif kind == 4:
            r[i, 4:7] = 0
        else:
            r[i, 7] = np.inf
    return r


def degenerate_kinds(rays):
    """how many rays of [..., 8] are of each kind of (f) -- by what they hold, wherever they came from: (zero rays, rays
    with a NaN, non-zero rays with tmin >= tmax, zero directions from a non-zero origin, tmax = inf)"""
    r = np.asarray(rays, F).reshape(-1, 8)
    zero = ~r.any(axis=1)
    nan = np.isnan(r).any(axis=1)
    with np.errstate(invalid="ignore"):
        closed = ~zero & ~nan & (r[:, 3] >= r[:, 7])
    nodir = ~zero & ~nan & ~r[:, 4:7].any(axis=1)
    return int(zero.sum()), int(nan.sum()), int(closed.sum()), int(nodir.sum()), int(np.isinf(r[:, 7]).sum())


def far_away(fs, w, n, rng):
    """(g) origins 10^3 scene extents away, aimed at the scene"""
    c, e = world_bounds(fs, w)
    o = c + _unit(rng.normal(size=(n, 3)) + [0, 0, 1.5]) * e * 1e3
    target = c + rng.uniform(-1, 1, (n, 3)) * e * [1, 1, 0.2]
    return _pack(o, _unit(target - o), 0.0, np.inf)


GENERATORS = (aimed, axis_parallel, inside_boxes, degenerate, far_away)


def mixed(fs, R, seed, cube=None, views=True):
    """float32 [worlds, R, 8]: ray i of world w takes turn g = (i + seed + w) mod 7: 0 is (a), a pixel of the world's
    first view; 1 is (e) over `cube` = (world-local row, half-size) of the axis-aligned cube; 2 ... 6 are (b), (c), (d),
    (f), (g).  Turn 0 in a world without a view (or with views=False) and turn 1 without a cube go to GENERATORS[(g - 2)
    mod 5]: (f) and (g).  (f) is drawn from a pool whose kinds rotate -- kind (w + j) mod 6 for the j-th (f) ray of world
    w -- so a set of a few dozen rays holds every kind; a small R meets only some turns in each world, and the turn it
    starts with moves with the seed and the world."""
    W = len(fs.world_inst_start) - 1
    out = np.zeros((W, R, 8), F)
    taken = {}
    for w in range(W):
        rng = np.random.default_rng(seed * 7919 + w)
        pools = {}
        view = int(np.flatnonzero(fs.view_world == w)[0]) if views and np.any(fs.view_world == w) else None
        for i in range(R):
            g = (i + seed + w) % 7
            if g == 0 and view is not None:
                if g not in pools:
                    pools[g] = pinhole(fs, view)[rng.permutation(fs.width * fs.height)]
                out[w, i] = pools[g][i % len(pools[g])]
            elif g == 1 and cube is not None:
                if g not in pools:
                    row = int(fs.world_inst_start[w]) + cube[0]
                    pools[g] = cube_grid(fs.inst_pos[row].astype(np.float64), cube[1], 5)
                out[w, i] = pools[g][(i // 7) % len(pools[g])]
            else:
                gen = GENERATORS[(g - 2) % len(GENERATORS)]
                if gen is degenerate:
                    if "f" not in pools:
                        pools["f"] = degenerate(fs, w, 8 * DEGENERATE_KINDS, rng, first=w)
                        taken[w] = 0
                    out[w, i] = pools["f"][taken[w] % len(pools["f"])]
                    taken[w] += 1
                else:
                    out[w, i] = gen(fs, w, 1, rng)[0]
    return out


def same(a, b):
    """bit-for-bit equality of two float32 arrays, except that any NaN equals any NaN"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))
