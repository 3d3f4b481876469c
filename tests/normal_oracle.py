"""The expected surface-normal image.  Nothing under oracle/ can emit normals, so this is a
float32 NumPy restatement of S1-S3, S6 (n, d) and S10 per (view, world-local triangle) -- the literal operation
order of oracle/raster_oracle.c's setup_view -- scattered through the C oracle's own tri_id image:

    expected[v][pixel] = table_v[tri_id[v][pixel]],   (128, 128, 128, 0) where tri_id < 0.

Triangles are numbered as setup_view numbers them: rows of the view's world in order, a hidden row skips its slots,
an unbound row has none, geometry and slots follow inst_obj0.  It composes with the projection, light, colour and
material oracles by taking tri_id from their renders: none of them changes a normal.

The arithmetic needs an exact fused multiply-add; `fma32` builds one from float64 (round to odd, then to float32).
`lit_table` restates S7 for white materials with the same n, d, len and sign rule, which is how the restatement is
pinned to the C oracle (tests/test_normal_cpu.py)."""
import numpy as np

F32 = np.float32
BACKGROUND = np.array([128, 128, 128, 0], np.uint8)


def fma32(a, b, c):
    """fmaf(a, b, c) for float32 arrays, bit for bit: the product is exact in float64 (48 bits), the float64 sum is
    rounded to odd with TwoSum's error term (53 >= 2 * 24 + 2 bits: no double rounding), then rounded to float32."""
    a = np.asarray(a, F32).astype(np.float64)
    b = np.asarray(b, F32).astype(np.float64)
    c = np.asarray(c, F32).astype(np.float64)
    a, b, c = np.broadcast_arrays(a, b, c)
    with np.errstate(over="ignore", invalid="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
        step = (err != 0) & even & np.isfinite(s)
        s = np.where(step, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(F32)


def dot3(ax, ay, az, bx, by, bz):
    """S2: one rounded product and two fused steps."""
    return fma32(az, bz, fma32(ay, by, np.asarray(ax, F32) * np.asarray(bx, F32)))


def quat_to_mat(q):
    """S1 for [..., 4] float32 quaternions (w, x, y, z) -> [..., 3, 3]."""
    q = np.asarray(q, F32)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    one = F32(1.0)
    x2, y2, z2 = x + x, y + y, z + z
    xx, yy, zz = x * x2, y * y2, z * z2
    xy, xz, yz = x * y2, x * z2, y * z2
    wx, wy, wz = w * x2, w * y2, w * z2
    R = np.empty(q.shape[:-1] + (3, 3), F32)
    R[..., 0, 0] = one - (yy + zz); R[..., 0, 1] = xy - wz;         R[..., 0, 2] = xz + wy
    R[..., 1, 0] = xy + wz;         R[..., 1, 1] = one - (xx + zz); R[..., 1, 2] = yz - wx
    R[..., 2, 0] = xz - wy;         R[..., 2, 1] = yz + wx;         R[..., 2, 2] = one - (xx + yy)
    return R


def _cross(a, b):
    o = np.empty_like(a)
    o[:, 0] = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
    o[:, 1] = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
    o[:, 2] = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    return o


def view_geometry(fs, v):
    """n [K, 3], d [K], len [K] (float32, as S6 / S7 compute them), the view-space vertices P [K, 3, 3] and the camera
    rotation Rc of view v of FlatScene `fs`, for the K world-local triangle slots of the view's world."""
    w = int(fs.view_world[v])
    Rc = quat_to_mat(fs.cam_rot[v])
    c = np.asarray(fs.cam_pos[v], F32)
    nobj = len(fs.obj_first_tri)
    rows, tris = [], []
    for i in range(int(fs.world_inst_start[w]), int(fs.world_inst_start[w + 1])):
        obj = int(fs.inst_obj0[i])
        if obj < 0 or obj >= nobj:
            continue                                  # unbound: no slots
        first, cnt = int(fs.obj_first_tri[obj]), int(fs.obj_num_tris[obj])
        rows.append(np.full(cnt, i, np.int64))        # (a hidden row keeps its slots: nothing of it is drawn)
        tris.append(np.arange(first, first + cnt, dtype=np.int64))
    if not rows:
        z = np.zeros((0, 3), F32)
        return z, np.zeros(0, F32), np.zeros(0, F32), np.zeros((0, 3, 3), F32), Rc
    rows, tris = np.concatenate(rows), np.concatenate(tris)
    Ri = quat_to_mat(fs.inst_rot[rows])               # [K, 3, 3]
    sc = np.asarray(fs.inst_scale[rows], F32)
    t = np.asarray(fs.inst_pos[rows], F32)
    M = Ri * sc[:, None, :]                           # M[r][c] = Ri[r][c] * sc[c]
    K = len(rows)
    MV = np.empty((K, 3, 3), F32)
    for r in range(3):
        for cc in range(3):
            MV[:, r, cc] = dot3(Rc[0, r], Rc[1, r], Rc[2, r], M[:, 0, cc], M[:, 1, cc], M[:, 2, cc])
    dt = t - c[None, :]
    tv = np.empty((K, 3), F32)
    for r in range(3):
        tv[:, r] = dot3(Rc[0, r], Rc[1, r], Rc[2, r], dt[:, 0], dt[:, 1], dt[:, 2])
    op = np.asarray(fs.tri_pos, F32).reshape(-1, 9)[tris]
    P = np.empty((K, 3, 3), F32)
    for j in range(3):
        for r in range(3):
            P[:, j, r] = fma32(MV[:, r, 2], op[:, 3 * j + 2],
                               fma32(MV[:, r, 1], op[:, 3 * j + 1], fma32(MV[:, r, 0], op[:, 3 * j], tv[:, r])))
    e1 = P[:, 1] - P[:, 0]
    e2 = P[:, 2] - P[:, 0]
    nn = _cross(e1, e2)
    d = dot3(nn[:, 0], nn[:, 1], nn[:, 2], P[:, 0, 0], P[:, 0, 1], P[:, 0, 2])
    ln = np.sqrt(dot3(nn[:, 0], nn[:, 1], nn[:, 2], nn[:, 0], nn[:, 1], nn[:, 2]))
    return nn, d, ln, P, Rc


def pack(nn, d, ln):
    """S10: [K, 4] uint8 from n, d, len."""
    out = np.empty((len(d), 4), np.uint8)
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(3):
            c = np.where(ln > 0, nn[:, i] / ln, F32(0.0)).astype(F32)
            c = np.where(d > 0, -c, c).astype(F32)
            c = np.minimum(np.maximum(c, F32(-1.0)), F32(1.0))
            out[:, i] = fma32(c, F32(127.0), F32(128.5)).astype(np.uint32).astype(np.uint8)
    out[:, 3] = 255
    return out


def view_table(fs, v):
    """[K, 4] uint8: the S10 pixel value of every world-local triangle slot of view v."""
    nn, d, ln, _, _ = view_geometry(fs, v)
    return pack(nn, d, ln)


def lit_table(fs, v, to_light, ambient, diffuse):
    """[K] uint8: S7's byte of a white material, to_u8(fma(diffuse, max(+-dot3(n, lv) / len, 0), ambient)), from the
    same n, d, len and sign rule as S10; `to_light` is the float32 unit vector towards the light (world space)."""
    nn, d, ln, _, Rc = view_geometry(fs, v)
    tl = np.asarray(to_light, F32)
    lv = [dot3(Rc[0, r], Rc[1, r], Rc[2, r], tl[0], tl[1], tl[2]) for r in range(3)]
    with np.errstate(divide="ignore", invalid="ignore"):
        ndl = (dot3(nn[:, 0], nn[:, 1], nn[:, 2], lv[0], lv[1], lv[2]) / ln).astype(F32)
    ndl = np.where(d > 0, -ndl, ndl).astype(F32)
    lit = fma32(F32(diffuse), np.maximum(ndl, F32(0.0)), F32(ambient))
    lit = lit * F32(1.0)
    cl = np.minimum(np.maximum(lit, F32(0.0)), F32(1.0))
    return fma32(cl, F32(255.0), F32(0.5)).astype(np.uint32).astype(np.uint8)


def scatter(table, tri_id):
    """One view: table[tri_id], the background where tri_id < 0."""
    out = np.empty(tri_id.shape + (4,), np.uint8)
    out[...] = BACKGROUND
    hit = tri_id >= 0
    out[hit] = table[tri_id[hit]]
    return out


def flat_scene(desc):
    from oracle import oracle
    return oracle.FlatScene(desc)


def normals(fs, tri_id, view_begin=0, view_end=None):
    """[view_end - view_begin, slow, fast, 4] uint8: the expected normals of views [view_begin, view_end) of FlatScene
    `fs` (poses, hidden rows and bindings as it holds them now), through tri_id[view_begin:view_end] of a render of
    the same state -- `tri_id` is indexed by view of the whole job."""
    if view_end is None:
        view_end = fs.num_views
    return np.stack([scatter(view_table(fs, v), tri_id[v]) for v in range(view_begin, view_end)])


def decode(img):
    """(b - 128) / 127 of the three axis bytes, float64."""
    return (np.asarray(img)[..., :3].astype(np.float64) - 128.0) / 127.0
