"""Supersampling on the host (no GPU): the helper the GPU tests compare against
(tests/supersample_oracle.py) -- the identity at s = 1, alpha stays 255, round half up on both sides of every .5,
point samples at (s // 2, s // 2), resolving commutes with the Raytracer transposition -- the kernel's divide-by-9
multiply-shift over its whole range, the C ABI's new names beside the unchanged old ones, mrx_create's argument checks
ahead of the device probe, the Python constructor's ValueError, SceneDesc carrying the factor, the headless option's
refusals, and the resolve kernels' resources as the compiler reports them."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from madrona_renderer_amd import scenes
from tests import supersample_oracle as so
from tests.conftest import ROOT, has_gpu
from tests.test_color_cpu import Cfg, _create

MRX_E_INVALID, MRX_E_NO_DEVICE, MRX_E_UNSUPPORTED = -1, -2, -5
SHIFT, MASK = 8, 3 << 8


def _flag(s):
    return (s - 1) << SHIFT


def test_resolve_at_factor_1_is_the_identity():
    rng = np.random.default_rng(1)
    ref = {"rgb": rng.integers(0, 256, (2, 5, 7, 4), dtype=np.uint8), "depth": rng.random((2, 5, 7), dtype=np.float32),
           "tri_id": rng.integers(-1, 9, (2, 5, 7), dtype=np.int32), "threads": 3}
    out = so.resolve(ref, 1)
    assert set(out) == {"rgb", "depth", "tri_id"}
    for k in out:
        assert np.array_equal(out[k], ref[k]) and out[k].dtype == ref[k].dtype


@pytest.mark.parametrize("s", [2, 3, 4])
def test_round_half_up_on_both_sides_of_every_half(s):
    """Footprint sums k*s*s + ceil(s*s/2) - 1 (the largest that still rounds down to k) and k*s*s + ceil(s*s/2) (the
    smallest that rounds up to k + 1), for every k in 0 ... 254, spread over the s*s samples; the three colour bytes
    take three different spreads of the same sum."""
    n = s * s
    half = (n + 1) // 2
    sums = np.array([k * n + half - 1 + up for k in range(255) for up in (0, 1)], np.int64)
    want = np.array([k + up for k in range(255) for up in (0, 1)], np.uint8)
    img = np.zeros((1, s, s * len(sums), 4), np.uint8)
    img[..., 3] = 255
    for x, t in enumerate(sums):
        base, rem = divmod(int(t), n)
        for c in range(3):
            vals = np.full(n, base, np.int64)
            vals[(np.arange(rem) + 2 * c + x) % n] += 1    # rem < n samples one above the rest, rotated per byte
            assert vals.sum() == t and vals.max() <= 255
            img[0, :, s * x:s * x + s, c] = vals.reshape(s, s)
    out = so.box(img, s)
    assert out.shape == (1, 1, len(sums), 4)
    for c in range(3):
        assert np.array_equal(out[0, 0, :, c], want), c
    assert (out[..., 3] == 255).all()                      # alpha: 255 on every sample stays 255
    # the rule itself, the way S12 writes it
    assert all((int(t) + n // 2) // n == int(w) for t, w in zip(sums, want))


def test_the_divide_by_nine_of_the_kernel_is_exact_over_its_range():
    # resolve.hip: q = (h * 7282) >> 16 on the 16-bit halves, h <= 9 * 255 + 4; exact for every h < 32768
    h = np.arange(32768, dtype=np.uint64)
    assert np.array_equal((h * 7282) >> 16, h // 9)
    assert 9 * 255 + 4 < 32768 and 2299 * 7282 < 1 << 24   # ... and the product's quotient byte sits in bits 16 ... 23
    # the halves never carry into one another: 16 samples of 255 plus the rounding term
    assert 16 * 255 + 8 < 1 << 16


@pytest.mark.parametrize("s", [2, 3, 4])
def test_point_samples_take_sample_s_half_s_half_with_their_bits(s):
    rng = np.random.default_rng(s)
    bits = rng.integers(0, 2 ** 32, (3, 5 * s, 7 * s), dtype=np.uint64).astype(np.uint32)
    for view in (bits.view(np.float32), bits.view(np.int32)):
        out = so.point(view, s)
        assert out.shape == (3, 5, 7) and out.dtype == view.dtype
        for y in range(5):
            for x in range(7):
                assert np.array_equal(out[:, y, x].view(np.uint32), bits[:, s * y + s // 2, s * x + s // 2])
    res = so.resolve({"depth": bits.view(np.float32), "segmask": bits.view(np.int32),
                      "normal": bits.view(np.uint8).reshape(3, 5 * s, 7 * s, 4)}, s)
    assert np.array_equal(res["normal"].view(np.uint32)[..., 0], res["segmask"].view(np.uint32))
    assert np.array_equal(res["depth"].view(np.uint32), res["segmask"].view(np.uint32))


@pytest.mark.parametrize("s", [2, 3])
def test_resolving_commutes_with_the_raytracer_transposition(oracle_mod, s):
    # the anchor of tests/test_oracle_anchors.py, resolved: a square Raytracer view is the transposed Rasterizer view
    ra = so.render(scenes.demo_scene(num_worlds=2, render_mode="Rasterizer", width=24, height=24), s)
    rt = so.render(scenes.demo_scene(num_worlds=2, render_mode="Raytracer", width=24, height=24), s)
    assert ra["rgb"].shape == (2, 24, 24, 4)
    assert np.array_equal(rt["rgb"], ra["rgb"].transpose(0, 2, 1, 3))
    assert np.array_equal(rt["tri_id"], ra["tri_id"].transpose(0, 2, 1))
    np.testing.assert_allclose(rt["depth"], ra["depth"].transpose(0, 2, 1), rtol=1e-6)
    assert (ra["rgb"][..., 3] == 255).all()
    # not vacuous: the filter changes pixels of the native render, the point samples agree with one another
    native = so.render(scenes.demo_scene(num_worlds=2, render_mode="Rasterizer", width=24, height=24), 1)
    assert (native["rgb"] != ra["rgb"]).any()
    assert np.array_equal(ra["tri_id"] >= 0, ra["depth"] != 0)


def test_sample_desc_and_scene_desc_carry_the_factor():
    d = scenes.synthetic_scene(3, width=40, height=24)
    assert d.supersample == 1
    d.supersample = 3
    sd = so.sample_desc(d)
    assert (sd.width, sd.height, sd.supersample) == (120, 72, 1) and (d.width, d.height) == (40, 24)
    assert d.shard(1, 2).supersample == 3


def test_the_new_abi_names_beside_the_unchanged_old_ones(native):
    m = native.load_module()
    assert m.MRX_FLAG_SUPERSAMPLE_SHIFT == SHIFT and m.MRX_FLAG_SUPERSAMPLE_MASK == MASK
    assert m.MRX_FLAG_INSTANCE_LABELS == 1 << 7 and m.MRX_NUM_BUFFERS_EXT3 == 14
    assert m.MRX_CONFIG_SIZE == ctypes.sizeof(Cfg)         # mrx_config did not grow
    lib = native.load_capi()
    lib.mrx_abi_version.restype = ctypes.c_int
    assert lib.mrx_abi_version() == 4
    for name in ("mrx_supersample", "mrx_sample_buffer", "mrx_resolve"):
        assert hasattr(lib, name)
    for name in ("supersample", "sample_tensor", "resolve"):
        assert hasattr(m.MadronaRenderer, name)
    lib.mrx_supersample.restype = ctypes.c_int
    lib.mrx_supersample.argtypes = [ctypes.c_void_p]
    lib.mrx_resolve.restype = ctypes.c_int
    lib.mrx_resolve.argtypes = [ctypes.c_void_p]
    assert lib.mrx_supersample(None) == MRX_E_INVALID and lib.mrx_resolve(None) == MRX_E_INVALID


def test_mrx_create_checks_the_sample_size_ahead_of_the_device(native):
    lib = native.load_capi()
    ok = 0 if has_gpu() else MRX_E_NO_DEVICE
    size = ctypes.sizeof(Cfg)
    for desc in (scenes.synthetic_scene(2, width=16, height=12),
                 scenes.synthetic_scene(2, width=16, height=16, render_mode="Raytracer")):
        for s in (1, 2, 3, 4):
            assert _create(lib, desc, size, None, flags=_flag(s)) == ok, s
        assert _create(lib, desc, size, None, flags=_flag(3) | (1 << 6) | (1 << 7)) == ok   # beside normals and labels
        assert _create(lib, desc, size, None, flags=_flag(2), reserved=1) == MRX_E_INVALID
    lib.mrx_last_error.restype = ctypes.c_char_p
    # 16384 a side is the limit of the SAMPLE image, in either axis
    for w, h, s, want in ((8192, 8, 2, ok), (8193, 8, 2, MRX_E_INVALID), (8, 8193, 2, MRX_E_INVALID),
                          (5462, 8, 3, MRX_E_INVALID), (4097, 8, 4, MRX_E_INVALID), (16384, 8, 1, ok),
                          (16384, 8, 2, MRX_E_INVALID)):
        if want == 0:
            continue                                        # (a device would allocate gigabytes: the refusals are the test)
        desc = scenes.synthetic_scene(1, width=w, height=h)
        assert _create(lib, desc, size, None, flags=_flag(s)) == want, (w, h, s)
        if want == MRX_E_INVALID:
            assert b"16384" in lib.mrx_last_error()


def test_the_python_constructor_refuses_a_factor_outside_1_to_4(native):
    for bad in (0, 5, -1, 8):
        desc = scenes.synthetic_scene(2)
        desc.supersample = bad
        with pytest.raises(ValueError, match="supersample"):
            scenes.make_renderer(desc)
    if not has_gpu():
        for good in (1, 2, 3, 4):
            desc = scenes.synthetic_scene(2)
            desc.supersample = good
            with pytest.raises(RuntimeError, match="no HIP device"):
                scenes.make_renderer(desc)


def test_headless_refuses_a_malformed_or_out_of_range_factor(native, tmp_path):
    from madrona_renderer_amd import build
    exe = build.headless_path()
    args = ["4", "1", "rast", "64", "64"]
    for bad in (["--supersample", "two"], ["--supersample", "0"], ["--supersample", "5"], ["--supersample", "-2"],
                ["--supersample", "2.5"], ["--supersample", ""], ["--supersample", "+2"], ["--supersample"]):
        p = subprocess.run(["timeout", "-k", "5", "60", exe] + args + bad, cwd=tmp_path, capture_output=True, text=True)
        assert p.returncode not in (0, 124, 137), bad
        assert "--supersample" in p.stderr, (bad, p.stderr)
    p = subprocess.run(["timeout", "-k", "5", "60", exe, "4", "1", "rast", "8192", "64", "--supersample", "3"],
                       cwd=tmp_path, capture_output=True, text=True)
    assert p.returncode not in (0, 124, 137) and "16384" in p.stderr, p.stderr


def test_the_resolve_kernels_use_no_scratch_and_spill_nothing():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources
    kernels = kernel_resources.resources(os.path.join(ROOT, "madrona_renderer_amd", "csrc", "resolve.hip"))
    names = [k["name"] for k in kernels]
    assert len(kernels) == 6, names                          # S = 2, 3, 4, the vector and the scalar form of each
    for s in (2, 3, 4):
        assert sum("resolveVecKernel<%d>" % s in n for n in names) == 1, names
        assert sum("resolveScalarKernel<%d>" % s in n for n in names) == 1, names
    for k in kernels:
        assert int(k["ScratchSize [bytes/lane]"]) == 0, k
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, k
        assert int(k["Occupancy [waves/SIMD]"]) == 8, k      # a streaming kernel: every wave slot
    have = [l.rstrip("\n") for l in open(os.path.join(ROOT, "profiles", "kernel_resources_resolve.txt"))
            if not l.startswith("#")]
    assert have == [kernel_resources.line(k) for k in kernels], \
        "stale: regenerate profiles/kernel_resources_resolve.txt (its header says how)"
