"""The position output on the host (no GPU): the float32 reference the GPU tests compare against
(tests/position_oracle.py) against a float64 evaluation of the same float32 inputs within a derived bound, the known
answer of S3's anchor quad, background pixels, the Raytracer transposition, the sample a supersampled pixel stands
for, the C ABI's new names beside the unchanged old ones, mrx_create's argument checks ahead of the device probe, the
Python constructor's ValueError, SceneDesc carrying the option, the headless option's refusals, and the unprojection
kernels' resources as the compiler reports them."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from madrona_renderer_amd import scenes
from tests import position_oracle as pos
from tests.conftest import ROOT, has_gpu
from tests.test_color_cpu import Cfg, _create

MRX_E_INVALID, MRX_E_NO_DEVICE, MRX_E_UNSUPPORTED = -1, -2, -5
POSITIONS, POSITIONS_VIEW, NO_RGB, NO_DEPTH = 1 << 10, 1 << 11, 1 << 2, 1 << 3


def _unit_quats(rng, n):
    q = rng.normal(size=(n, 4))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def _float64(depth, cam_pos, cam_rot, consts, s, raytracer):
    """S13's world frame in float64 from the same float32 inputs, and the magnitude M of every component:
    M = sum_k |R[r][k]| * |Pv_k|+ + |c[r]|, |Pv_x|+ = d * (|px * sx| + |ox|), likewise z, |Pv_y|+ = d."""
    d = np.asarray(depth, np.float64)
    views, nslow, nfast = d.shape
    px, py = (a.astype(np.float64) for a in pos.pixel_centres(nslow, nfast, s, raytracer))
    c64 = np.asarray(consts, np.float64)
    sx, ox, sz, oz = (c64[:, k][:, None, None] for k in range(4))
    pv = np.stack([d * (px[None] * sx + ox), d, d * (py[None] * sz + oz)], axis=-1)
    mag = np.stack([d * (np.abs(px[None] * sx) + np.abs(ox)), d, d * (np.abs(py[None] * sz) + np.abs(oz))], axis=-1)
    q = np.asarray(cam_rot, np.float64)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((views, 3, 3))
    R[:, 0] = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], axis=-1)
    R[:, 1] = np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], axis=-1)
    R[:, 2] = np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=-1)
    c = np.asarray(cam_pos, np.float64)
    world = np.einsum("vrk,vijk->vijr", R, pv) + c[:, None, None, :]
    M = np.einsum("vrk,vijk->vijr", np.abs(R), mag) + np.abs(c)[:, None, None, :]
    return pv, mag, world, M


def test_the_float32_reference_agrees_with_float64_within_the_derived_bound(native):
    """Seven roundings lie on the longest path to a world component: x2, the product and the sum of an entry of R, the
    product R * Pv (whose Pv carries the rounding of px * sx, of + ox and of d * r: relative errors that add to the
    entry's), two sums and + c.  Each is at most 2^-24 of a partial result no larger than M, so 8 * 2^-24 * M bounds the
    difference with room for the second-order terms.  View frame: three roundings, the same bound on |Pv|+."""
    rng = np.random.default_rng(13)
    worst = 0.0
    for _ in range(200):
        w, h, s = int(rng.integers(1, 70)), int(rng.integers(1, 70)), int(rng.integers(1, 5))
        rt = bool(rng.integers(0, 2))
        nslow, nfast = (w, w) if rt else (h, w)
        depth = rng.uniform(0.05, 500.0, (1, nslow, nfast)).astype(np.float32)
        q, c = _unit_quats(rng, 1), rng.uniform(-50, 50, (1, 3)).astype(np.float32)
        consts = pos.constants(w, h, rt, [(float(rng.uniform(20.0, 150.0)), None)], s)
        got_w = pos.unproject(depth, c, q, consts, s, "world", rt)
        got_v = pos.unproject(depth, c, q, consts, s, "view", rt)
        pv, mag, world, M = _float64(depth, c, q, consts, s, rt)
        assert got_w.dtype == np.float32 and (got_w[..., 3] == 1).all() and (got_v[..., 3] == 1).all()
        eps = 8.0 * 2.0 ** -24
        rw = np.abs(got_w[..., :3].astype(np.float64) - world) / (eps * M)
        rv = np.abs(got_v[..., :3].astype(np.float64) - pv) / (eps * mag)
        worst = max(worst, float(rw.max()), float(rv.max()))
        assert rw.max() <= 1.0 and rv.max() <= 1.0, (w, h, s, rt, float(rw.max()), float(rv.max()))
    print("largest error of the float32 reference: %.2f of the 8 ulps of M allowed" % (8.0 * worst))


def _anchor_depth():
    # S3's anchor (tests/test_oracle_anchors.py): a 10 x 10 quad 10 in front of a 64 x 64 camera of vfov 90 fills
    # exactly the pixels [16, 48)^2 at depth 10
    d = np.zeros((1, 64, 64), np.float32)
    d[0, 16:48, 16:48] = 10.0
    return d


def test_known_answer_the_anchor_quad_in_the_view_frame(native):
    d = _anchor_depth()
    consts = pos.constants(64, 64, False, [(90.0, None)])
    ident, zero = np.array([[1, 0, 0, 0]], np.float32), np.zeros((1, 3), np.float32)
    p = pos.unproject(d, zero, ident, consts, 1, "view", False)
    assert p.shape == (1, 64, 64, 4)
    inside = p[0, 16:48, 16:48]
    assert (inside[..., 1] == 10.0).all() and (inside[..., 3] == 1.0).all()
    k = np.arange(16, 48, dtype=np.float64)
    want_x = (10.0 * ((k + 0.5) / 32.0 - 1.0)).astype(np.float32)          # -4.84375 ... 4.84375, exact in binary32
    assert np.array_equal(want_x.astype(np.float64), 10.0 * ((k + 0.5) / 32.0 - 1.0))
    assert np.array_equal(inside[..., 0], np.broadcast_to(want_x[None, :], (32, 32)))
    assert np.array_equal(inside[..., 2], np.broadcast_to(-want_x[:, None], (32, 32)))   # row 0 is up
    # the quad's own extent: the outermost pixel centres lie half a pixel inside +-5
    assert inside[..., 0].min() == -4.84375 and inside[..., 0].max() == 4.84375
    # identity pose: the world frame is the view frame; a translated camera moves every point by c, exactly here
    assert np.array_equal(pos.unproject(d, zero, ident, consts, 1, "world", False), p)
    c = np.array([[3.0, -2.0, 0.5]], np.float32)
    moved = pos.unproject(d, c, ident, consts, 1, "world", False)
    assert np.array_equal(moved[0, 16:48, 16:48, :3], inside[..., :3] + c[0])


def test_background_pixels_hold_four_zeros(native):
    d = _anchor_depth()
    d[0, 0, 0] = -0.0                                        # S9's background is depth == 0, whatever its sign
    consts = pos.constants(64, 64, False, [(90.0, None)])
    q, c = _unit_quats(np.random.default_rng(2), 1), np.array([[7.0, 8.0, 9.0]], np.float32)
    for frame in ("world", "view"):
        p = pos.unproject(d, c, q, consts, 1, frame, False)
        miss = d[0] == 0
        assert miss.sum() == 64 * 64 - 32 * 32
        assert (p[0][miss].view(np.uint32) == 0).all()      # +0.0 four times: not c, not -0.0, not NaN
        assert (p[0][~miss][:, 3] == 1.0).all()
    # ... also where the ray constants are not finite: 0 * inf must not leak
    with np.errstate(all="ignore"):
        p = pos.unproject(d, c, q, np.array([[np.inf, 0, np.inf, 0]], np.float32), 1, "world", False)
    assert (p[0][d[0] == 0].view(np.uint32) == 0).all()


@pytest.mark.parametrize("frame", ["world", "view"])
@pytest.mark.parametrize("s", [1, 2, 3])
def test_the_raytracer_result_is_the_transposed_rasterizer_result(native, frame, s):
    rng = np.random.default_rng(5 + s)
    d = rng.uniform(0.05, 500.0, (3, 12, 12)).astype(np.float32)
    d[rng.random(d.shape) < 0.25] = 0.0
    q, c = _unit_quats(rng, 3), rng.uniform(-9, 9, (3, 3)).astype(np.float32)
    projs = [(40.0, None), (90.0, None), (133.0, None)]
    # (a square view: the two modes share every constant but the near plane, which S13 does not read)
    cr, ct = pos.constants(12, 12, False, projs, s), pos.constants(12, 12, True, projs, s)
    assert np.array_equal(cr, ct)
    ra = pos.unproject(d, c, q, cr, s, frame, False)
    rt = pos.unproject(d.transpose(0, 2, 1), c, q, ct, s, frame, True)
    assert np.array_equal(rt, ra.transpose(0, 2, 1, 3))
    assert (ra[..., 3] == (d != 0)).all()


@pytest.mark.parametrize("s", [2, 3, 4])
def test_a_supersampled_pixel_stands_for_sample_s_half_s_half(native, s):
    """Native pixel (x, y) of a renderer at factor s holds the point of sample (s*x + s//2, s*y + s//2) of the s*W x s*H
    image: the reference at factor s equals the reference at factor 1 on the sample image, taken at those samples."""
    rng = np.random.default_rng(s)
    w, h = 7, 5
    sample_depth = rng.uniform(0.05, 500.0, (2, s * h, s * w)).astype(np.float32)
    q, c = _unit_quats(rng, 2), rng.uniform(-9, 9, (2, 3)).astype(np.float32)
    projs = [(70.0, None), (110.0, 0.5)]
    full = pos.unproject(sample_depth, c, q, pos.constants(s * w, s * h, False, projs, 1), 1, "world", False)
    native_depth = sample_depth[:, s // 2::s, s // 2::s]
    assert native_depth.shape == (2, h, w)
    got = pos.unproject(native_depth, c, q, pos.constants(w, h, False, projs, s), s, "world", False)
    assert np.array_equal(got, full[:, s // 2::s, s // 2::s])
    px, py = pos.pixel_centres(h, w, s, False)
    assert px[0, 1] == s + s // 2 and py[1, 0] == s + s // 2 and px[0, 0] == s // 2


def test_scene_desc_carries_the_option():
    d = scenes.synthetic_scene(3, width=40, height=24)
    assert d.positions is None
    d.positions = "view"
    assert d.shard(1, 2).positions == "view"


def test_the_new_abi_names_beside_the_unchanged_old_ones(native):
    m = native.load_module()
    assert m.MRX_FLAG_POSITIONS == POSITIONS and m.MRX_FLAG_POSITIONS_VIEW == POSITIONS_VIEW
    assert m.MRX_BUF_POSITION == 14 and m.MRX_NUM_BUFFERS_EXT4 == 15
    assert m.MRX_NUM_BUFFERS_EXT3 == 14 and m.MRX_FLAG_SUPERSAMPLE_MASK == 3 << 8
    assert m.MRX_CONFIG_SIZE == ctypes.sizeof(Cfg)         # mrx_config did not grow
    lib = native.load_capi()
    lib.mrx_abi_version.restype = ctypes.c_int
    assert lib.mrx_abi_version() == 4
    for name in ("mrx_unproject", "mrx_positions"):
        assert hasattr(lib, name)
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = [ctypes.c_void_p]
        assert getattr(lib, name)(None) == MRX_E_INVALID
    for name in ("positions", "position_tensor", "unproject"):
        assert hasattr(m.MadronaRenderer, name)


def test_mrx_create_checks_the_flags_ahead_of_the_device(native):
    lib = native.load_capi()
    lib.mrx_last_error.restype = ctypes.c_char_p
    ok = 0 if has_gpu() else MRX_E_NO_DEVICE
    size = ctypes.sizeof(Cfg)
    for desc in (scenes.synthetic_scene(2, width=16, height=12),
                 scenes.synthetic_scene(2, width=16, height=16, render_mode="Raytracer")):
        for flags in (POSITIONS, POSITIONS | POSITIONS_VIEW, POSITIONS_VIEW):
            assert _create(lib, desc, size, None, flags=flags | NO_DEPTH) == MRX_E_INVALID
            msg = lib.mrx_last_error()
            assert b"MRX_FLAG_POSITIONS" in msg and b"MRX_FLAG_NO_DEPTH" in msg, msg
            # ... beside everything else it combines: depth only, normals, labels, visibility ids, supersampling
            for more in (0, NO_RGB, 1 << 6, 1 << 7, 1 << 0, 1 << 8, 2 << 8, 3 << 8, NO_RGB | (1 << 6) | (2 << 8)):
                assert _create(lib, desc, size, None, flags=flags | more) == ok, (flags, more)
        assert _create(lib, desc, size, None, flags=POSITIONS, reserved=1) == MRX_E_INVALID


def test_the_python_constructor_refuses_anything_but_the_four_values(native):
    for bad in ("sideways", 2, 1.0, "World", b"view", ["view"]):
        desc = scenes.synthetic_scene(2)
        desc.positions = bad
        with pytest.raises(ValueError, match="positions"):
            scenes.make_renderer(desc)
    desc = scenes.synthetic_scene(2)
    desc.positions = True
    with pytest.raises(ValueError, match="positions"):       # computed from depth: an rgb-only renderer has none
        scenes.make_renderer(desc, render_outputs="RGB")
    if not has_gpu():
        for good in (True, "world", "view", False, None):
            desc = scenes.synthetic_scene(2)
            desc.positions = good
            with pytest.raises(RuntimeError, match="no HIP device"):
                scenes.make_renderer(desc)


def test_headless_refuses_a_malformed_frame_and_positions_without_depth(native, tmp_path):
    from madrona_renderer_amd import build
    exe = build.headless_path()
    args = ["4", "1", "rast", "64", "64"]
    for bad in (["--positions", "sideways"], ["--positions", "World"], ["--positions", ""], ["--positions", "2"],
                ["--positions", "--outputs", "rgb"], ["--outputs", "rgb", "--positions", "view"]):
        p = subprocess.run(["timeout", "-k", "5", "60", exe] + args + bad, cwd=tmp_path, capture_output=True, text=True)
        assert p.returncode not in (0, 124, 137), bad
        assert "--positions" in p.stderr, (bad, p.stderr)
    if not has_gpu():
        # a well-formed option gets as far as the device, with and without the frame
        for good in (["--positions"], ["--positions", "view"], ["--positions", "world", "--outputs", "depth"]):
            p = subprocess.run(["timeout", "-k", "5", "60", exe] + args + good, cwd=tmp_path, capture_output=True, text=True)
            assert p.returncode not in (0, 124, 137) and "--positions" not in p.stderr, (good, p.stderr)
    assert not list(tmp_path.iterdir())


def test_the_unproject_kernels_use_no_scratch_and_spill_nothing():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources
    kernels = kernel_resources.resources(os.path.join(ROOT, "madrona_renderer_amd", "csrc", "unproject.hip"))
    names = [k["name"] for k in kernels]
    assert len(kernels) == 4, names                          # frame (world / view) x storage (x fast / x slow)
    for frame in ("true", "false"):
        for order in ("true", "false"):
            assert sum("unprojectKernel<%s, %s>" % (frame, order) in n for n in names) == 1, names
    for k in kernels:
        assert int(k["ScratchSize [bytes/lane]"]) == 0, k
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, k
        assert int(k["Occupancy [waves/SIMD]"]) == 8, k      # a streaming kernel: every wave slot
    have = [l.rstrip("\n") for l in open(os.path.join(ROOT, "profiles", "kernel_resources_unproject.txt"))
            if not l.startswith("#")]
    assert have == [kernel_resources.line(k) for k in kernels], \
        "stale: regenerate profiles/kernel_resources_unproject.txt (its header says how)"
