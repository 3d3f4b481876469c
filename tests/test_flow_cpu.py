"""The optical-flow output on the host (no GPU): the host entry mrx_flow_host -- the kernel's own
source, flow_core.hpp, run on the CPU -- against the NumPy restatement tests/flow_oracle.py bit for bit; that restatement
against a float64 evaluation within a bound derived by counting roundings; known answers; validity; the ABI's new names
beside the unchanged old ones; the kernels' resources as the compiler reports them; and the sanitizer build of the host
entry, run as a stand-alone program."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from madrona_renderer_amd import scenes
from tests import flow_oracle as fo
from tests.conftest import ROOT, has_gpu
from tests.test_color_cpu import Cfg

F = np.float32
MRX_E_INVALID, MRX_E_UNSUPPORTED = -1, -5
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def capi(native):
    lib = native.load_capi()
    lib.mrx_flow_host.restype = ctypes.c_int
    lib.mrx_flow_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                  ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32,
                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
    for f in (lib.mrx_flow_create, lib.mrx_flow_enabled, lib.mrx_flow, lib.mrx_flow_snapshot):
        f.restype = ctypes.c_int
        f.argtypes = [ctypes.c_void_p]
    return lib


def unit_quats(rng, n):
    q = rng.normal(size=(n, 4))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F)


def tables(rng, views, rows):
    """one world of `rows` rows per view, the views in another order than the worlds; every third row is undrawn: it
    repeats its successor's base (the last row of a world: the world's triangle count)"""
    kbase = np.zeros(views * rows, np.uint32)
    total = np.zeros(views, np.int64)
    for w in range(views):
        k = 0
        for r in range(rows):
            kbase[w * rows + r] = k
            if r % 3 != 1:
                k += int(rng.integers(1, 13))
        total[w] = k
    start = (np.arange(views + 1) * rows).astype(np.uint32)
    view_world = rng.permutation(views).astype(np.uint32)
    return kbase, start, view_world, total


def random_case(rng, views, w, h, rows, s, rt, per_view, wild=True):
    """Inputs of S17.  wild: poses, scales and constants anywhere (zeros and mirrors among the scales): the bit-for-bit
    tests.  Otherwise a scene that moved a little between two steps, every point staying in front of the camera: the
    float64 test."""
    nslow, nfast = (w, w) if rt else (h, w)
    kbase, start, view_world, total = tables(rng, views, rows)
    n_inst = views * rows
    ids = np.zeros((views, nslow, nfast), np.int32)
    for v in range(views):
        wd = int(view_world[v])
        b = kbase[wd * rows:(wd + 1) * rows].astype(np.int64)
        # the first and the last id of rows, ids next to undrawn rows (a repeated base is both), -1, and random ones
        special = np.concatenate([b, np.maximum(b - 1, 0), [total[wd] - 1, -1]])
        flat = rng.integers(0, max(int(total[wd]), 1), nslow * nfast)
        take = min(len(special), flat.size)
        flat[rng.permutation(flat.size)[:take]] = special[:take]
        flat[rng.random(flat.size) < 0.05] = -1
        ids[v] = flat.reshape(nslow, nfast)
    depth = rng.uniform(1.0 if wild else 3.0, 50.0, (views, nslow, nfast)).astype(F)
    depth[rng.random(depth.shape) < 0.1] = 0
    fovs = [(float(rng.uniform(40.0, 120.0)), None) for _ in range(views)]
    fovs_prev = [(float(rng.uniform(40.0, 120.0)), None) for _ in range(views)] if wild else \
        [(f * float(rng.uniform(0.95, 1.05)), None) for f, _ in fovs]
    if not per_view:
        fovs = [fovs[0]] * views
    consts = fo.constants(w, h, rt, fovs, s)
    prev_consts = fo.constants(w, h, rt, fovs_prev, s)
    if wild:
        scale = lambda: (rng.uniform(0.5, 2.0, (n_inst, 3)) * np.where(rng.random((n_inst, 3)) < 0.2, -1, 1) *
                         np.where(rng.random((n_inst, 3)) < 0.03, 0, 1)).astype(F)
        live = (rng.uniform(-20, 20, (n_inst, 3)).astype(F), unit_quats(rng, n_inst), scale(),
                rng.uniform(-20, 20, (views, 3)).astype(F), unit_quats(rng, views))
        prev = (rng.uniform(-20, 20, (n_inst, 3)).astype(F), unit_quats(rng, n_inst), scale(),
                rng.uniform(-20, 20, (views, 3)).astype(F), unit_quats(rng, views))
    else:
        nudge = lambda q: (lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(F))(
            q.astype(np.float64) + rng.normal(scale=0.002, size=q.shape))
        live = (rng.uniform(-20, 20, (n_inst, 3)).astype(F), unit_quats(rng, n_inst),
                rng.uniform(0.5, 2.0, (n_inst, 3)).astype(F), rng.uniform(-20, 20, (views, 3)).astype(F),
                unit_quats(rng, views))
        prev = ((live[0] + rng.uniform(-0.1, 0.1, (n_inst, 3))).astype(F), nudge(live[1]),
                (live[2] * rng.uniform(0.995, 1.005, (n_inst, 3))).astype(F),
                (live[3] + rng.uniform(-0.1, 0.1, (views, 3))).astype(F), nudge(live[4]))
    return dict(depth=depth, ids=ids, consts=consts, prev_consts=prev_consts, kbase=kbase, start=start,
                view_world=view_world, live=live, prev=prev, s=s, rt=rt, per_view=per_view)


def oracle(c):
    return fo.flow(c["depth"], c["ids"], c["consts"], c["prev_consts"], c["kbase"], c["start"], c["view_world"],
                   c["live"], c["prev"], c["s"], c["rt"])


def host(capi, c, pass_rows=0, want_rc=0):
    views, nslow, nfast = c["depth"].shape
    keep = [np.ascontiguousarray(a, F) for a in c["live"] + c["prev"]]
    live = (ctypes.c_void_p * 5)(*[a.ctypes.data for a in keep[:5]])
    prev = (ctypes.c_void_p * 5)(*[a.ctypes.data for a in keep[5:]])
    depth, ids = np.ascontiguousarray(c["depth"], F), np.ascontiguousarray(c["ids"], np.int32)
    consts = np.ascontiguousarray(c["consts"] if c["per_view"] else c["consts"][0], F)
    prev_consts = np.ascontiguousarray(c["prev_consts"], F)
    kbase, start, vw = (np.ascontiguousarray(c[k], np.uint32) for k in ("kbase", "start", "view_world"))
    out = np.full((views, nslow, nfast, 4), np.nan, F)
    rc = capi.mrx_flow_host(depth.ctypes.data, ids.ctypes.data, views, nfast, nslow, 1 if c["rt"] else 0, c["s"],
                            consts.ctypes.data, 1 if c["per_view"] else 0, prev_consts.ctypes.data, kbase.ctypes.data,
                            start.ctypes.data, vw.ctypes.data, len(start) - 1, len(kbase), live, prev, pass_rows,
                            out.ctypes.data)
    assert rc == want_rc
    return out


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, F).view(np.uint32), np.ascontiguousarray(b, F).view(np.uint32))


SHAPES = [(3, 5, 3), (3, 7, 5), (2, 40, 24)]


@pytest.mark.parametrize("rows", [1, 3, 70])
@pytest.mark.parametrize("views,w,h", SHAPES)
def test_the_host_entry_equals_the_oracle_on_every_bit(capi, views, w, h, rows):
    """both storage orders, s = 1, 2, 3, uniform and per-view constants; 70 rows are more than one staging pass of 64,
    and the forced pass of 3 rows restages every shape with more than three"""
    rng = np.random.default_rng(1000 * views + 10 * w + rows)
    valid = 0
    for rt in (False, True):
        for s in (1, 2, 3):
            for per_view in (False, True):
                c = random_case(rng, views, w, h, rows, s, rt, per_view)
                want = oracle(c)
                assert want.dtype == F and want.shape == c["depth"].shape + (4,)
                for pass_rows in (0, 3):
                    got = host(capi, c, pass_rows)
                    assert same_bits(got, want), (rt, s, per_view, pass_rows,
                                                  np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4])
                valid += int((want[..., 3] == 1).sum())
                assert (want[..., 3][(c["depth"] == 0) | (c["ids"] < 0)] == 0).all()
    assert valid > 0


def _f64(c):
    """S17 in float64 from the same float32 inputs, and the bounds of dx, dy, dz (test below)"""
    d = np.asarray(c["depth"], np.float64)
    views, nslow, nfast = d.shape
    px, py = (a.astype(np.float64) for a in fo.pixel_centres(nslow, nfast, c["s"], c["rt"]))

    def rot(q):
        q = np.asarray(q, np.float64)
        w, x, y, z = (q[..., i] for i in range(4))
        R = np.empty(q.shape[:-1] + (3, 3))
        A = np.empty(q.shape[:-1] + (3, 3))
        for (i, j), (a, b, sign) in {(0, 1): (x * y, w * z, -1), (0, 2): (x * z, w * y, 1), (1, 0): (x * y, w * z, 1),
                                     (1, 2): (y * z, w * x, -1), (2, 0): (x * z, w * y, -1), (2, 1): (y * z, w * x, 1)}.items():
            R[..., i, j] = 2 * (a + sign * b)
            A[..., i, j] = 2 * (np.abs(a) + np.abs(b))
        for i, (a, b) in enumerate(((y * y, z * z), (x * x, z * z), (x * x, y * y))):
            R[..., i, i] = 1 - 2 * (a + b)
            A[..., i, i] = 1 + 2 * (a + b)
        return R, A

    lp, lq, ls, lc, lcq = (np.asarray(a, np.float64) for a in c["live"])
    pp, pq, ps, pc, pcq = (np.asarray(a, np.float64) for a in c["prev"])
    out = np.zeros((views, nslow, nfast, 3))
    bound = np.zeros((views, nslow, nfast, 3))
    hit = np.zeros((views, nslow, nfast), bool)
    small = 0.0
    for v in range(views):
        wd = int(c["view_world"][v])
        rows, found = fo.find_rows(c["ids"][v], c["kbase"], int(c["start"][wd]), int(c["start"][wd + 1]))
        hit[v] = ~(d[v] == 0) & (c["ids"][v] >= 0) & found
        sx, ox, sz, oz = (float(t) for t in c["consts"][v])
        sxp, oxp, szp, ozp = (float(t) for t in c["prev_consts"][v])
        Rc, Ac = rot(lcq[v])
        Rcp, Acp = rot(pcq[v])
        Rr, Ar = rot(lq[rows])
        Rrp, Arp = rot(pq[rows])
        pv = np.stack([d[v] * (px * sx + ox), d[v], d[v] * (py * sz + oz)], -1)
        Mpv = np.stack([d[v] * (np.abs(px * sx) + abs(ox)), d[v], d[v] * (np.abs(py * sz) + abs(oz))], -1)
        P = pv @ Rc.T + lc[v]
        M = Mpv @ Ac.T + np.abs(lc[v])
        u, M = P - lp[rows], M + np.abs(lp[rows])
        l, M = np.einsum("...ij,...i->...j", Rr, u), np.einsum("...ij,...i->...j", Ar, M)
        n, M = l / ls[rows] * ps[rows], M / np.abs(ls[rows]) * np.abs(ps[rows])
        Pp = np.einsum("...ij,...j->...i", Rrp, n) + pp[rows]
        M = np.einsum("...ij,...j->...i", Arp, M) + np.abs(pp[rows])
        up, M = Pp - pc[v], M + np.abs(pc[v])
        pvp, M = up @ Rcp, M @ Acp
        Y, MY = pvp[..., 1], M[..., 1]
        small = max(small, float((34 * EPS * MY / Y)[hit[v]].max(initial=0.0)))
        for k, (j, o, sc, p) in enumerate(((0, oxp, sxp, px), (2, ozp, szp, py))):
            q = pvp[..., j] / Y
            Mt = (M[..., j] + np.abs(q) * MY) / Y + abs(o)
            out[v, ..., k] = (p - (q - o) / sc) / c["s"]
            bound[v, ..., k] = 40 * EPS * (Mt / abs(sc) + p) / c["s"]
        out[v, ..., 2] = d[v] - Y
        bound[v, ..., 2] = 36 * EPS * (MY + d[v])
        hit[v] &= Y > 0
        assert (Y[hit[v]] >= 0.1).all()                # far past every znear the modes default to (0.001, 0.1)
    return out, bound, hit, small


def test_the_float32_reference_agrees_with_float64_within_the_derived_bound(native):
    """The bound, to first order in eps = 2^-24.  A value computed with n roundings on its longest path, the counts of
    both operands of a product or a quotient adding up, differs from its exact value by at most n * eps * M, where M is
    the value's magnitude: the same expression over absolute values (of an entry of R(q): A = 1 + 2 (|aa| + |bb|) on the
    diagonal, 2 (|ab| + |wc|) beside it, which bounds the entry's every partial result).  The counts:
      entry of R(q) 3 (the doubling is exact); pv 3; P = (R pv) + c: 3 + 3 + 1, two sums, + c = 10; u = P - p 11;
      l = R^T u: 3 + 11 + 1, two sums = 17; 1 / s is 1, m = l * (1 / s) 19, n = m * s' 20;
      P' = (R' n) + p': 3 + 20 + 1, two sums, + p' = 27; u' = P' - c' 28; pv' = R_c'^T u': 3 + 28 + 1, two sums = 34.
    So |err pv'_j| <= 34 eps M_j, and dz = d - Y' is within 35 eps (M_Y + d): the test allows 36.
    The quotient q = pv'_0 / Y' is amplified by 1 / Y': |err q| <= (34 eps M_0 + |q| 34 eps M_Y) / Y' + eps |q|
    <= 35 eps M_q with M_q = (M_0 + |q| M_Y) / Y' >= 2 |q|.  q - ox' adds one rounding of at most |q| + |ox'|:
    36 eps M_t, M_t = M_q + |ox'|.  The division by sx' amplifies by 1 / |sx'| and adds one: 37 eps M_t / |sx'|.  px is
    exact; px - px' 38 eps (M_t / |sx'| + px); the division by s 39 eps (M_t / |sx'| + px) / s.  The test allows 40: room
    for the second-order terms (40 / 39 = 1 + 2^-5.3): the largest is the quotient's, 1 / (Y' (1 + t)) with |t| <= 34 eps
    M_Y / Y', which stays below 2^-6 of the first-order term as long as 34 eps M_Y / Y' <= 2^-7 -- asserted of the
    inputs, which are drawn so that every Y' >= 0.1 >= znear."""
    rng = np.random.default_rng(17)
    worst = 0.0
    for views, w, h in SHAPES + [(2, 33, 17)]:
        for rt in (False, True):
            for s in (1, 2, 3):
                c = random_case(rng, views, w, h, 5, s, rt, True, wild=False)
                got = oracle(c)
                want, bound, hit, small = _f64(c)
                assert small <= 2.0 ** -7, small
                assert hit.sum() > 0.7 * hit.size and ((got[..., 3] == 1) == hit).all()
                share = np.abs(got[..., :3].astype(np.float64) - want)[hit] / bound[hit]
                worst = max(worst, float(share.max()))
                assert share.max() <= 1.0, (views, w, h, rt, s, float(share.max()))
    print("largest error of the float32 reference: %.3f of the bound" % worst)


def quad_case(D=8.0, w=16, h=12, s=1, fov=90.0, fov_prev=None, cam=(0, 0, 0), cam_prev=(0, 0, 0), inst=(0, 0, 0),
              inst_prev=(0, 0, 0)):
    """one view that sees a fronto-parallel quad at depth D on every pixel (one row, id 0), identity rotations"""
    ident = np.array([[1, 0, 0, 0]], F)
    one = np.ones((1, 3), F)
    v3 = lambda t: np.array([t], F)
    return dict(depth=np.full((1, h, w), D, F), ids=np.zeros((1, h, w), np.int32),
                consts=fo.constants(w, h, False, [(fov, None)], s),
                prev_consts=fo.constants(w, h, False, [(fov if fov_prev is None else fov_prev, None)], s),
                kbase=np.zeros(1, np.uint32), start=np.array([0, 1], np.uint32), view_world=np.zeros(1, np.uint32),
                live=(v3(inst), ident.copy(), one.copy(), v3(cam), ident.copy()),
                prev=(v3(inst_prev), ident.copy(), one.copy(), v3(cam_prev), ident.copy()),
                s=s, rt=False, per_view=True)


def _both(capi, c):
    got = oracle(c)
    assert same_bits(host(capi, c), got)
    _, bound, hit, _ = _f64(c)
    assert hit.all() and (got[..., 3] == 1).all()
    return got.astype(np.float64), bound


@pytest.mark.parametrize("s", [1, 2])
def test_known_answers_of_a_fronto_parallel_quad(capi, s):
    D, delta = 8.0, 0.25
    sx = float(fo.constants(16, 12, False, [(90.0, None)], s)[0, 0])
    # the camera moved sideways (+x) by delta: the image moved the other way, by delta / (D sx) samples
    got, bound = _both(capi, quad_case(D, s=s, cam=(delta, 0, 0)))
    assert (np.abs(got[..., 0] - (-delta / (D * sx) / s)) <= bound[..., 0]).all() and -delta / (D * sx) < 0
    assert (np.abs(got[..., 1]) <= bound[..., 1]).all() and (np.abs(got[..., 2]) <= bound[..., 2]).all()
    # the instance moved instead: the opposite sign
    got, bound = _both(capi, quad_case(D, s=s, inst=(delta, 0, 0)))
    assert (np.abs(got[..., 0] - (delta / (D * sx) / s)) <= bound[..., 0]).all()
    assert (np.abs(got[..., 1]) <= bound[..., 1]).all() and (np.abs(got[..., 2]) <= bound[..., 2]).all()
    # the camera moved forward by delta: the surface is delta nearer than it was
    got, bound = _both(capi, quad_case(D, s=s, cam=(0, delta, 0)))
    assert (np.abs(got[..., 2] - (-delta)) <= bound[..., 2]).all()
    # a still scene
    got, bound = _both(capi, quad_case(D, s=s, cam=(1, 2, 3), cam_prev=(1, 2, 3), inst=(4, 5, 6), inst_prev=(4, 5, 6)))
    assert (np.abs(got[..., :3]) <= bound).all()


def test_a_change_of_vfov_alone_scales_the_offset_from_the_principal_point(capi):
    c = quad_case(fov=90.0, fov_prev=60.0)
    got, bound = _both(capi, c)
    (sx, ox, sz, oz), (sxp, oxp, szp, ozp) = (tuple(float(t) for t in k[0]) for k in (c["consts"], c["prev_consts"]))
    px, py = (a.astype(np.float64) for a in fo.pixel_centres(12, 16, 1, False))
    # previous position - previous principal point = (position - principal point) * sx / sx'
    prev_x, prev_y = px - got[0, ..., 0], py - got[0, ..., 1]
    assert (np.abs((prev_x + oxp / sxp) - (px + ox / sx) * sx / sxp) <= bound[0, ..., 0]).all()
    assert (np.abs((prev_y + ozp / szp) - (py + oz / sz) * sz / szp) <= bound[0, ..., 1]).all()
    assert sx / sxp > 1.5 and (np.abs(got[..., 2]) <= bound[..., 2]).all()


def test_pixels_that_are_not_valid_hold_four_selected_zeros(capi):
    inf, nan = float("inf"), float("nan")
    zero_bits = lambda a: (np.ascontiguousarray(a, F).view(np.uint32) == 0).all()
    # background (depth 0) and id -1
    c = quad_case()
    c["depth"][0, 0, :] = 0
    c["ids"][0, 1, :] = -1
    for got in (oracle(c), host(capi, c)):
        assert zero_bits(got[0, :2]) and (got[0, 2:, :, 3] == 1).all()
    # the point lay behind the previous camera (Y' < 0), or in its plane (Y' == 0)
    for cam_prev in ((0, 9.0, 0), (0, 8.0, 0)):
        c = quad_case(D=8.0, cam_prev=cam_prev)
        for got in (oracle(c), host(capi, c)):
            assert zero_bits(got)
    # a NaN pose, and an infinite intermediate (p' = inf: 0 * inf in the product with R_c'): zeros, not NaNs
    for bad in (nan, inf, -inf):
        c = quad_case(inst_prev=(bad, 0, 0))
        for got in (oracle(c), host(capi, c)):
            assert zero_bits(got)
    # values that are not finite while valid holds are stored as they come: a previous sx' of zero divides by it
    # (a zero scale makes every component of P' infinite or NaN, and Y' with them)
    c = quad_case()
    c["prev_consts"][0, 0] = 0
    a, b = oracle(c), host(capi, c)
    assert same_bits(a, b) and (a[..., 3] == 1).all() and not np.isfinite(a[..., 0]).any() and np.isfinite(a[..., 1:3]).all()
    c = quad_case()
    c["live"][2][0, 0] = 0
    assert same_bits(oracle(c), host(capi, c))


def test_the_entry_points_refuse_a_null_renderer_and_the_abi_keeps_its_size(capi, native):
    assert capi.mrx_flow_create(None) == MRX_E_INVALID
    assert capi.mrx_flow_enabled(None) == MRX_E_INVALID
    assert capi.mrx_flow(None) == MRX_E_INVALID
    assert capi.mrx_flow_snapshot(None) == MRX_E_INVALID
    m = native.load_module()
    assert m.MRX_BUF_FLOW == 22 and m.MRX_NUM_BUFFERS_EXT8 == 23 and m.MRX_NUM_BUFFERS_EXT7 == 22
    capi.mrx_abi_version.restype = ctypes.c_int
    assert capi.mrx_abi_version() == 4
    assert m.MRX_CONFIG_SIZE == ctypes.sizeof(Cfg)         # mrx_config did not grow


def test_the_host_entry_checks_its_arguments(capi):
    c = quad_case(w=4, h=3)
    assert host(capi, c).shape == (1, 3, 4, 4)
    host(capi, dict(c, s=5), want_rc=MRX_E_INVALID)
    # no view, a world and no world table: refused, not read
    none = np.zeros(1, F)
    five = (ctypes.c_void_p * 5)(*[none.ctypes.data] * 5)
    assert capi.mrx_flow_host(None, None, 0, 4, 3, 0, 1, none.ctypes.data, 0, None, None, None, None, 1, 0, five, five, 0,
                              None) == MRX_E_INVALID
    assert capi.mrx_flow_host(None, None, 0, 4, 3, 0, 1, none.ctypes.data, 0, None, None, None, None, 0, 0, five, five, 0,
                              None) == 0
    host(capi, dict(c, view_world=np.array([1], np.uint32)), want_rc=MRX_E_INVALID)   # a world past the table's end
    host(capi, dict(c, start=np.array([0, 2], np.uint32)), want_rc=MRX_E_INVALID)     # rows past the columns' end


def test_the_python_constructor_takes_the_option(native):
    m = native.load_module()
    assert scenes.synthetic_scene(2).flow is False
    desc = scenes.synthetic_scene(2)
    desc.flow = True
    with pytest.raises(ValueError, match="flow"):
        scenes.make_renderer(desc, render_outputs="RGB")
    desc = scenes.synthetic_scene(2)
    desc.render_mode = "Raytracer"
    desc.flow, desc.boxes = True, 4
    with pytest.raises(ValueError, match="flow"):
        scenes.make_renderer(desc)
    if not has_gpu():
        desc = scenes.synthetic_scene(2)
        desc.flow = True
        with pytest.raises(RuntimeError, match="no HIP device"):
            scenes.make_renderer(desc)
    assert hasattr(m.MadronaRenderer, "flow_tensor") and hasattr(m.MadronaRenderer, "flow_snapshot")


def test_the_flow_kernels_use_no_scratch_and_spill_nothing():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources
    kernels = kernel_resources.resources(os.path.join(ROOT, "madrona_renderer_amd", "csrc", "flow.hip"))
    names = [k["name"] for k in kernels]
    assert len(kernels) == 3, names                          # the flow in both storage orders, the snapshot
    for name in ("flowKernel<true>", "flowKernel<false>", "flowSnapshotKernel"):
        assert sum(name in n for n in names) == 1, names
    for k in kernels:
        assert int(k["ScratchSize [bytes/lane]"]) == 0, k
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, k
    have = [l.rstrip("\n") for l in open(os.path.join(ROOT, "profiles", "kernel_resources_flow.txt"))
            if not l.startswith("#")]
    assert have == [kernel_resources.line(k) for k in kernels], \
        "stale: regenerate profiles/kernel_resources_flow.txt (its header says how)"


def test_the_hip_compile_line_has_no_fast_math_flag():
    """S17's divisions must be IEEE divisions on the device: hipcc's default, as long as no flag takes it away"""
    src = open(os.path.join(ROOT, "madrona_renderer_amd", "build.py")).read()
    assert '"-fno-fast-math"' in src and '"-ffp-contract=off"' in src
    for flag in ("-ffast-math", "-Ofast", "-fno-hip-fp32-correctly-rounded-divide-sqrt", "-funsafe-math-optimizations",
                 "-freciprocal-math", "-fapprox-func"):
        assert '"%s"' % flag not in src, flag


# ---- the sanitizer build of the host entry, a stand-alone program ---------------------------------------------------------
@pytest.fixture(scope="module")
def driver():
    from madrona_renderer_amd import build
    return build.build_flow_driver()


@pytest.mark.parametrize("args", [(3, 5, 3, 1, 1), (3, 7, 5, 3, 2), (2, 40, 24, 70, 3), (3, 3, 5, 70, 1), (1, 1, 1, 1, 1),
                                  (2, 69, 67, 70, 2), (2, 5, 3, 0, 1)])
def test_sanitized_host_entry(driver, args):
    p = subprocess.run([driver] + [str(a) for a in args] + ["7"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (args, p.stdout[-2000:], p.stderr[-4000:])
    assert "flow_host_driver ok" in p.stdout and "ERROR" not in p.stderr and "runtime error" not in p.stderr, (p.stdout, p.stderr)
