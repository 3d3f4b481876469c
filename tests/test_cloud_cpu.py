"""The point-cloud output on the host (no GPU): the host entry mrx_cloud_host -- the kernels' own
source, cloud_core.hpp, walked part by part, span by span and segment by segment as the kernels walk it -- against
tests/cloud_oracle.py on every bit of all three outputs; the oracle's selection against a plain loop over the
definition; hand-built masks; the plan; the refusals of the entry points and of cloud.attach; the kernels' resources;
and the sanitizer build of the host entry, run as a stand-alone program."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import cloud_oracle as co
from tests import position_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
MRX_OK, MRX_E_INVALID = 0, -1


@pytest.fixture(scope="module")
def capi(native):
    lib = ctypes.CDLL(native.load_capi()._name)        # a handle of this module's own: its prototypes stay here
    lib.mrx_cloud_host.restype = ctypes.c_int
    lib.mrx_cloud_host.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int,
                                   ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                   ctypes.c_float, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                                   ctypes.c_void_p]
    lib.mrx_cloud_plan.restype = ctypes.c_int
    lib.mrx_cloud_plan.argtypes = [ctypes.c_uint32] * 6 + [ctypes.c_int, ctypes.c_void_p]
    for name in ("mrx_cloud", "mrx_compact"):
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = [ctypes.c_void_p]
    lib.mrx_cloud_create.restype = ctypes.c_int
    lib.mrx_cloud_create.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_float]
    return lib


def test_the_constants_the_tests_use_are_the_header_s():
    header = open(os.path.join(ROOT, "include", "mrx.h")).read()
    for text in ("MRX_BUF_CLOUD = 23,", "MRX_BUF_CLOUD_PIXEL = 24,", "MRX_BUF_CLOUD_COUNT = 25,",
                 "MRX_NUM_BUFFERS_EXT9 = 26", "MRX_NUM_BUFFERS_EXT8 = 23,"):
        assert text in header, text
    assert MRX_E_INVALID == -1 and "MRX_E_INVALID = -1" in header.replace("  ", " ")
    from madrona_renderer_amd import cloud
    assert (cloud.MRX_BUF_CLOUD, cloud.MRX_BUF_CLOUD_PIXEL, cloud.MRX_BUF_CLOUD_COUNT) == (23, 24, 25)
    import madrona_renderer_amd
    assert "cloud" in madrona_renderer_amd.__all__


# ---- the oracle's selection against the definition

def _select_by_definition(valid, n):
    """S18 read aloud: a plain loop, Python ints"""
    ranked = [i for i, ok in enumerate(valid) if ok]
    m = len(ranked)
    out = []
    for k in range(n):
        if m >= n:
            out.append(ranked[(k * m) // n])
        elif k < m:
            out.append(ranked[k])
        else:
            out.append(-1)
    return out, m


def test_the_oracle_s_selection_is_the_definition():
    rng = np.random.default_rng(5)
    for px in (1, 7, 64, 65, 300):
        for density in (0.0, 0.1, 0.5, 1.0):
            valid = rng.random(px) < density
            for n in (1, 2, 7, px - 1, px, px + 1, 70):
                if n < 1:
                    continue
                got, m = co.select(valid, n)
                want, wm = _select_by_definition(valid.tolist(), n)
                assert m == wm and got.tolist() == want, (px, density, n)


def test_the_scatter_form_of_the_slot_rule_is_the_forward_rule():
    """with M >= N the pixel of rank r is selected iff k0 = ceil(r N / M) < N and floor(k0 M / N) == r, its slot k0:
    brute force, as cloud_core.hpp's cloudSlot computes it"""
    for n in range(1, 71):
        for m in list(range(n, n + 40)) + [n + 299, n + 300]:
            forward = {(k * m) // n: k for k in range(n)}
            assert len(forward) == n                                        # at most one slot per rank
            for r in range(m):
                k0 = -(-(r * n) // m)
                slot = k0 if k0 < n and (k0 * m) // n == r else None
                assert slot == forward.get(r), (n, m, r)


# ---- the host entry against the oracle

def _cameras(rng, views):
    q = rng.normal(size=(views, 4))
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F)
    return rng.uniform(-20, 20, (views, 3)).astype(F), q


def _consts(w, h, rt, views, s):
    return po.constants(w, h, rt, [(60.0 + 9.0 * (v % 4), None if v % 2 else 0.05 * (v + 1)) for v in range(views)], s)


def host(capi, depth, cam_pos, cam_rot, consts, s, frame, rt, n, max_depth=None, parts=1, want_rc=MRX_OK):
    depth = np.ascontiguousarray(depth, F)
    views, nslow, nfast = depth.shape
    points = np.full((views, n, 4), np.nan, F)
    pixel = np.full((views, n), -77, np.int32)
    count = np.full(views, -77, np.int32)
    cp = np.ascontiguousarray(cam_pos, F) if cam_pos is not None else None
    cr = np.ascontiguousarray(cam_rot, F) if cam_rot is not None else None
    consts = np.ascontiguousarray(consts, F)
    rc = capi.mrx_cloud_host(depth.ctypes.data, views, nfast, nslow, 1 if rt else 0, s, consts.ctypes.data,
                             cp.ctypes.data if cp is not None else None, cr.ctypes.data if cr is not None else None,
                             {"world": 1, "view": 2}.get(frame, frame), 0.0 if max_depth is None else max_depth, n, parts,
                             points.ctypes.data, pixel.ctypes.data, count.ctypes.data)
    assert rc == want_rc, (rc, want_rc)
    return points, pixel, count


def _assert_same(got, want, what):
    for g, w, name in zip(got, want, ("points", "pixel", "count")):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        bad = int((g.view(np.uint32) != w.view(np.uint32)).sum())
        assert bad == 0, f"{what}: {bad} of {g.size} values of {name} differ in their bits"


def _properties(got, valid, n):
    """filled slots strictly increasing in storage order, count == M, every slot filled when M >= N"""
    points, pixel, count = got
    views = len(count)
    assert np.array_equal(count, valid.reshape(views, -1).sum(axis=1))
    for v in range(views):
        m = int(count[v])
        filled = pixel[v] >= 0
        assert int(filled.sum()) == min(m, n) and filled[:min(m, n)].all()
        assert (points[v, filled, 3] == 1).all() and (points[v, ~filled].view(np.uint32) == 0).all()
        assert (pixel[v, ~filled] == -1).all()


SHAPES = [(5, 3, False), (64, 1, False), (40, 24, False), (64, 64, False), (40, 40, True)]


@pytest.mark.parametrize("w,h,rt", SHAPES)
def test_the_host_entry_equals_the_oracle_on_every_bit(capi, w, h, rt):
    """random depth with zeros, NaNs and values beyond max_depth; s = 1, 2, 3, both frames, N around the pixel count,
    1, 2, 3 and 7 parts per view"""
    views = 3
    nslow, nfast = (w, w) if rt else (h, w)
    px = nslow * nfast
    rng = np.random.default_rng(100 * w + h)
    cam_pos, cam_rot = _cameras(rng, views)
    for s in (1, 2, 3):
        consts = _consts(w, h, rt, views, s)
        depth = rng.uniform(0.1, 60.0, (views, nslow, nfast)).astype(F)
        kind = rng.integers(0, 16, depth.shape)
        depth[kind < (3 + 4 * s)] = 0.0                     # more holes at larger s: M on both sides of N = 1024
        depth[kind == 15] = np.nan
        depth[0, 0, 0] = -1.0
        for frame in ("world", "view"):
            for max_depth in (None, 30.0):
                valid = co.valid_mask(depth, max_depth)
                order_key = None
                for n in sorted({1, 7, max(px - 1, 1), px, px + 1, 1024}):
                    want = co.cloud(depth, cam_pos, cam_rot, consts, s, frame, rt, n, max_depth)
                    for parts in (1, 2, 3, 7):
                        got = host(capi, depth, cam_pos, cam_rot, consts, s, frame, rt, n, max_depth, parts)
                        _assert_same(got, want, (w, h, rt, s, frame, max_depth, n, parts))
                    _properties(want, valid, n)
                    # storage order: the pixel indices, turned back into storage indices, increase strictly
                    width = nslow if rt else nfast
                    for v in range(views):
                        p = want[1][v][want[1][v] >= 0].astype(np.int64)
                        y, x = p // width, p % width
                        storage = x * nfast + y if rt else y * nfast + x
                        assert (np.diff(storage) > 0).all(), order_key


def hand_built_masks(nslow, nfast, n, parts=1):
    """name -> bool [nslow, nfast] in storage order: M = 0, 1, N - 1, N, N + 1, all; only lane 0 of every segment; only
    lane 63; one valid pixel in the last segment of the last part"""
    px = nslow * nfast
    segs = (px + 63) // 64
    out = {}

    def first(m):
        a = np.zeros(px, bool)
        a[np.linspace(0, px - 1, m).astype(np.int64) if m > 1 else ([px // 3] if m else [])] = True
        assert int(a.sum()) == m
        return a

    for name, m in (("M=0", 0), ("M=1", 1), ("M=N-1", n - 1), ("M=N", n), ("M=N+1", n + 1), ("all", px)):
        if 0 <= m <= px:
            out[name] = first(m)
    lane0 = np.zeros(px, bool)
    lane0[0::64] = True
    lane63 = np.zeros(px, bool)
    lane63[63::64] = True
    last = np.zeros(px, bool)
    last_part_lo = (parts - 1) * segs // parts
    last[min((segs - 1) * 64 + 1, px - 1)] = True
    assert segs - 1 >= last_part_lo
    out.update({"lane0": lane0, "lane63": lane63, "last-segment": last})
    return {k: v.reshape(nslow, nfast) for k, v in out.items()}


def depth_of(mask, rng):
    d = np.where(mask, rng.uniform(0.5, 40.0, mask.shape), 0.0).astype(F)
    assert np.array_equal(d > 0, mask)
    return d


@pytest.mark.parametrize("w,h,rt,n", [(64, 64, False, 256), (40, 24, False, 100), (40, 40, True, 1024), (5, 3, False, 7),
                                      (150, 64, False, 4096)])
def test_hand_built_masks_against_the_oracle(capi, w, h, rt, n):
    nslow, nfast = (w, w) if rt else (h, w)
    rng = np.random.default_rng(w + h + n)
    for parts in (1, 3, 7):
        masks = hand_built_masks(nslow, nfast, n, parts)
        names = list(masks)
        depth = np.stack([depth_of(masks[k], rng) for k in names])
        cam_pos, cam_rot = _cameras(rng, len(names))
        consts = _consts(w, h, rt, len(names), 1)
        want = co.cloud(depth, cam_pos, cam_rot, consts, 1, "world", rt, n)
        got = host(capi, depth, cam_pos, cam_rot, consts, 1, "world", rt, n, None, parts)
        _assert_same(got, want, (w, h, rt, n, parts, names))
        _properties(got, np.stack([masks[k] for k in names]), n)
        for i, k in enumerate(names):
            assert int(got[2][i]) == int(masks[k].sum()), k


def test_the_host_entry_checks_its_arguments(capi):
    rng = np.random.default_rng(1)
    depth = rng.uniform(1, 2, (2, 3, 5)).astype(F)
    cam_pos, cam_rot = _cameras(rng, 2)
    consts = _consts(5, 3, False, 2, 1)
    assert host(capi, depth, cam_pos, cam_rot, consts, 1, "world", False, 4)[0].shape == (2, 4, 4)
    for bad in (dict(n=0), dict(n=65537), dict(s=0), dict(s=5), dict(frame=0), dict(frame=3), dict(max_depth=-1.0),
                dict(max_depth=float("inf")), dict(max_depth=float("nan")), dict(cam_pos=None)):
        kw = dict(cam_pos=cam_pos, cam_rot=cam_rot, consts=consts, s=1, frame="world", rt=False, n=4)
        kw.update(bad)
        if kw["n"] < 1 or kw["n"] > 65536:
            # (the output blocks are sized by n: the entry must refuse before it writes)
            pts = np.zeros((2, 1, 4), F)
            rc = capi.mrx_cloud_host(depth.ctypes.data, 2, 5, 3, 0, 1, consts.ctypes.data, cam_pos.ctypes.data,
                                     cam_rot.ctypes.data, 1, 0.0, kw["n"], 1, pts.ctypes.data, pts.ctypes.data,
                                     pts.ctypes.data)
            assert rc == MRX_E_INVALID, bad
        else:
            host(capi, depth, want_rc=MRX_E_INVALID, **kw)
    # view space reads no camera; zero views write nothing
    host(capi, depth, None, None, consts, 1, "view", False, 4)
    assert capi.mrx_cloud_host(None, 0, 5, 3, 0, 1, None, None, None, 1, 0.0, 4, 1, None, None, None) == MRX_OK


# ---- the plan

def plan(capi, views, nfast, nslow, n, cus=256, forced=0, null=0):
    out = (ctypes.c_uint32 * 3)(9, 9, 9)
    rc = capi.mrx_cloud_plan(views, nfast, nslow, n, cus, forced, null, out)
    return rc, list(out)


def test_the_plan(capi):
    # refusals: N, null tensors, no CU, too many pixels, a view too large for an int32 pixel index, views * N
    for args in ((4, 64, 64, 0), (4, 64, 64, 65537)):
        assert plan(capi, *args)[0] == MRX_E_INVALID, args
    assert plan(capi, 4, 64, 64, 256, null=1)[0] == MRX_E_INVALID
    assert plan(capi, 4, 64, 64, 256, cus=0)[0] == MRX_E_INVALID
    assert plan(capi, 2, 65536, 65535, 16)[0] == MRX_E_INVALID            # 2^33 - 2^17 pixels
    assert plan(capi, 1, 65536, 32768, 16)[0] == MRX_E_INVALID            # 2^31 pixels in one view
    assert plan(capi, 32768, 8, 8, 65536)[0] == MRX_E_INVALID             # views * N = 2^31
    assert plan(capi, 32767, 8, 8, 65536)[0] > 0
    # zero views, zero pixels: nothing is enqueued
    assert plan(capi, 0, 64, 64, 256)[0] == 0 and plan(capi, 4, 0, 64, 256)[0] == 0
    # the headline: one workgroup per view, no more workgroups than are resident, 32-bit slots
    rc, out = plan(capi, 1024, 64, 64, 1024)
    assert rc == 1024 and out[0] == 1 and out[2] == 0 and 0 < out[1] <= 1024
    rc, out = plan(capi, 16384, 64, 64, 16)
    assert rc == 4 * 256 and out[0] == 1
    # few large views split: the smallest count that gives 2 * CUs workgroups, at most one part per whole span
    rc, out = plan(capi, 4, 1024, 1024, 1024)
    assert out[0] == 128 and rc == 512
    rc, out = plan(capi, 4, 128, 64, 1024)
    assert out[0] == 2 and rc == 8                                       # two spans: two parts
    assert plan(capi, 4, 64, 64, 256)[1][0] == 1                         # one span: never split by the rule
    assert plan(capi, 512, 1024, 1024, 1024)[1][0] == 1                  # views >= 2 * CUs
    # the forced split: at most one part per segment, at most 256
    assert plan(capi, 3, 40, 24, 16, forced=3)[1][0] == 3 and plan(capi, 3, 40, 24, 16, forced=3)[0] == 9
    assert plan(capi, 3, 40, 24, 16, forced=99)[1][0] == 15              # 960 pixels: 15 segments
    assert plan(capi, 1, 1024, 1024, 16, forced=1000)[1][0] == 256
    # the 64-bit path switches on where pxPerView * N first reaches 2^32
    assert plan(capi, 1, 65536, 1, 65535)[1][2] == 0 and plan(capi, 1, 65536, 1, 65536)[1][2] == 1
    assert plan(capi, 1, 4096, 1024, 1023)[1][2] == 0 and plan(capi, 1, 4096, 1024, 1024)[1][2] == 1
    assert plan(capi, 1, 4097, 1024, 1024)[1][2] == 1 and plan(capi, 1, 4095, 1024, 1024)[1][2] == 0


def test_the_wide_slot_rule_agrees_with_the_narrow_one_where_both_apply(capi):
    """a view of 2^16 + 64 pixels and N = 65536 takes the 64-bit path; the oracle is exact either way"""
    nfast, nslow, n = 1028, 64, 65536
    assert plan(capi, 1, nfast, nslow, n)[1][2] == 1 and plan(capi, 1, nfast, nslow, n - 1024)[1][2] == 0
    rng = np.random.default_rng(9)
    depth = rng.uniform(0.5, 9.0, (1, nslow, nfast)).astype(F)
    depth[0, ::7, ::3] = 0.0
    consts = _consts(nfast, nslow, False, 1, 1)
    for nn in (n, n - 1024):
        want = co.cloud(depth, None, None, consts, 1, "view", False, nn)
        for parts in (1, 5):
            _assert_same(host(capi, depth, None, None, consts, 1, "view", False, nn, None, parts), want, (nn, parts))


# ---- the entry points and the Python front end

def test_the_entry_points_refuse_a_null_renderer(capi):
    assert capi.mrx_cloud(None) == MRX_E_INVALID
    assert capi.mrx_compact(None) == MRX_E_INVALID
    assert capi.mrx_cloud_create(None, 16, 1, 0.0) == MRX_E_INVALID


class _StandIn:
    """what attach() is given instead of a renderer: any native call would need its handle"""

    def native_handle(self):
        raise AssertionError("attach() reached the renderer before it had checked its arguments")


@pytest.mark.parametrize("kw,names", [
    (dict(points=0), ("1", "65536")), (dict(points=65537), ("1", "65536")), (dict(points=True), ("1", "65536")),
    (dict(points=16.0), ("1", "65536")), (dict(points="16"), ("1", "65536")), (dict(points=None), ("1", "65536")),
    (dict(points=16, frame="World"), ("world", "view")), (dict(points=16, frame=1), ("world", "view")),
    (dict(points=16, frame=None), ("world", "view")),
    (dict(points=16, max_depth=0), ("None", "finite positive")), (dict(points=16, max_depth=-2.0), ("None", "finite positive")),
    (dict(points=16, max_depth=float("inf")), ("None", "finite positive")),
    (dict(points=16, max_depth=float("nan")), ("None", "finite positive")),
    (dict(points=16, max_depth="3"), ("None", "finite positive")), (dict(points=16, max_depth=True), ("None", "finite positive")),
    (dict(points=16, max_depth=1e300), ("None", "finite positive")),
])
def test_attach_checks_its_arguments_before_any_native_call(native, kw, names):
    from madrona_renderer_amd import cloud
    with pytest.raises(ValueError) as e:
        cloud.attach(_StandIn(), **kw)
    for name in names:
        assert name in str(e.value), (kw, str(e.value))


def test_good_arguments_reach_the_renderer(native):
    from madrona_renderer_amd import cloud
    for kw in (dict(points=1), dict(points=65536, frame="view"), dict(points=16, max_depth=2), dict(points=16, max_depth=0.5)):
        with pytest.raises(AssertionError, match="reached the renderer"):
            cloud.attach(_StandIn(), **kw)


def test_the_dlpack_capsule_is_a_view_of_the_memory_it_names(native):
    """the capsule cloud.py builds with ctypes, on host memory (device type kDLCPU): torch's tensor has the pointer, sees
    a write made behind its back, and keeps the owner alive until it is dropped"""
    torch = pytest.importorskip("torch")
    import gc
    import weakref
    from madrona_renderer_amd import cloud

    class Owner:
        pass

    for dtype, code in ((np.float32, cloud._kDLFloat), (np.int32, cloud._kDLInt)):
        backing = np.arange(24, dtype=dtype).reshape(2, 3, 4)
        owner = Owner()
        owner.backing = backing
        alive = weakref.ref(owner)
        t = torch.from_dlpack(cloud._Exported(backing.ctypes.data, backing.shape, code, 32, cloud._kDLCPU, 0, owner))
        assert t.data_ptr() == backing.ctypes.data and tuple(t.shape) == (2, 3, 4)
        assert t.dtype == (torch.float32 if dtype == np.float32 else torch.int32) and t.is_contiguous()
        backing[1, 2, 3] = 99
        assert t[1, 2, 3].item() == 99
        t[0, 0, 0] = 7
        assert backing[0, 0, 0] == 7
        del owner
        gc.collect()
        assert alive() is not None and len(cloud._LIVE) >= 1
        del t
        gc.collect()
        assert alive() is None
    assert len(cloud._LIVE) == 0


def test_the_binding_s_surface_is_untouched(native):
    m = native.load_module()
    assert m.MRX_NUM_BUFFERS_EXT8 == 23 and not hasattr(m, "MRX_NUM_BUFFERS_EXT9") and not hasattr(m, "MRX_BUF_CLOUD")
    assert not hasattr(m.MadronaRenderer, "cloud_tensor")


# ---- the kernels' resources

def test_the_cloud_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources
    kernels = kernel_resources.resources(os.path.join(ROOT, "madrona_renderer_amd", "csrc", "cloud.hip"))
    names = [k["name"] for k in kernels]
    assert len(kernels) == 5, names             # the count kernel; the select kernel in both frames and both widths
    assert sum("cloudCountKernel" in n for n in names) == 1 and sum("cloudSelectKernel" in n for n in names) == 4, names
    for k in kernels:
        assert int(k["ScratchSize [bytes/lane]"]) == 0, k
        assert int(k["VGPRs Spill"]) == 0, k
    have = [l.rstrip("\n") for l in open(os.path.join(ROOT, "profiles", "kernel_resources_cloud.txt"))
            if not l.startswith("#")]
    assert have == [kernel_resources.line(k) for k in kernels], \
        "stale: regenerate profiles/kernel_resources_cloud.txt (its header says how)"


# ---- the sanitizer build of the host entry, run as a stand-alone program

@pytest.fixture(scope="module")
def driver():
    from madrona_renderer_amd import build
    return build.build_cloud_driver()


@pytest.mark.parametrize("args", [(3, 5, 3, 7, 1), (2, 64, 1, 64, 2), (2, 40, 24, 961, 3), (3, 64, 64, 1024, 1),
                                  (1, 1, 1, 1, 1), (2, 130, 70, 4096, 1), (1, 1028, 64, 65536, 1)])
def test_sanitized_host_entry(driver, args):
    p = subprocess.run([driver] + [str(a) for a in args] + ["7"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (args, p.stdout[-2000:], p.stderr[-4000:])
    assert "cloud_host_driver ok" in p.stdout and "ERROR" not in p.stderr and "runtime error" not in p.stderr, \
        (p.stdout, p.stderr)
