"""The packed observation output on the host (no GPU): known answers of the NumPy restatement the
GPU tests compare against (tests/observation_oracle.py), its bfloat16 against torch's, the stack written out by hand,
the Raytracer transposition, SceneDesc carrying the option, the C ABI's new names beside the unchanged old ones,
mrx_create's argument checks ahead of the device probe, the Python constructor's ValueError, the headless options'
refusals, and the observation kernels' resources as the compiler reports them."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from madrona_renderer_amd import scenes
from tests import observation_oracle as ob
from tests.conftest import ROOT, has_gpu
from tests.test_color_cpu import Cfg, _create

MRX_E_INVALID, MRX_E_NO_DEVICE, MRX_E_UNSUPPORTED = -1, -2, -5
VISIBILITY_IDS, NO_RGB, NO_DEPTH, NORMALS, LABELS, POSITIONS = 1 << 0, 1 << 2, 1 << 3, 1 << 6, 1 << 7, 1 << 10
FLOATS = ("float32", "float16", "bfloat16")


def _as_f32(a, dtype):
    """the value an element stands for (bfloat16: its bits are the upper half of a float32)"""
    if dtype == "bfloat16":
        return (a.astype(np.uint32) << 16).view(np.float32)
    return a.astype(np.float32)


def _one(rgba=(0, 0, 0, 255), d=0.0):
    return np.array(rgba, np.uint8).reshape(1, 1, 1, 4), np.array(d, np.float32).reshape(1, 1, 1)


def test_known_answers_colour():
    levels = np.arange(256, dtype=np.uint8)
    rgb = np.zeros((1, 1, 256, 4), np.uint8)
    rgb[0, 0, :, 0] = levels
    assert np.float32(255.0) * ob.K == np.float32(1.0)
    for dtype in FLOATS:
        got = ob.pack(rgb, None, "rgb", dtype)[0, 0, 0]
        assert _as_f32(got[255:], dtype)[0] == 1.0                    # byte 255 is exactly one
        assert _as_f32(got[:1], dtype)[0] == 0.0
        assert len(np.unique(ob.bits(got))) == 256                     # no colour level is lost
        assert (np.diff(_as_f32(got, dtype)) > 0).all()
    assert np.array_equal(ob.pack(rgb, None, "rgb", "uint8")[0, 0, 0], levels)
    # white is 255; red, green and blue alone are their weights 77, 150, 29 times 255 / 256, rounded: 77, 149, 29 --
    # S15's formula gives green 149, (150 * 255 + 128) >> 8, not the 150 of its weight
    assert (150 * 255 + 128) >> 8 == 149 and 77 + 150 + 29 == 256
    for colour, want in (((255, 255, 255), 255), ((255, 0, 0), 77), ((0, 255, 0), 149), ((0, 0, 255), 29), ((0, 0, 0), 0)):
        c, _ = _one(colour + (255,))
        assert ob.pack(c, None, "y", "uint8").item() == want
        assert ob.pack(c, None, "y", "float32").item() == np.float32(want) * ob.K


def test_known_answers_depth():
    def d_of(d, dtype="float32", rng=(0.0, 20.0)):
        return ob.pack(None, np.array(d, np.float32).reshape(1, 1, 1), "d", dtype, rng)[0, 0, 0, 0]

    assert d_of(10.0) == np.float32(0.5)
    assert d_of(3.0, rng=(3.0, 20.0)) == 0.0 and ob.bits(d_of(3.0, rng=(3.0, 20.0))) == 0     # d = lo gives +0
    assert d_of(2.0, rng=(3.0, 20.0)) == 0.0 and ob.bits(d_of(2.0, rng=(3.0, 20.0))) == 0
    assert d_of(20.0) == 1.0 and d_of(500.0) == 1.0 and d_of(np.float32(np.inf)) == 1.0         # d >= hi gives 1
    assert d_of(0.0) == 1.0 and d_of(-0.0) == 1.0                                               # the background, with a range
    assert d_of(0.0, rng=None) == 0.0 and d_of(7.25, rng=None) == np.float32(7.25)            # ... and without
    assert d_of(10.0, "uint8") == 128 and d_of(0.0, "uint8") == 255 and d_of(0.0, "uint8", None) == 0
    assert d_of(0.7, "uint8", None) == int(np.float32(0.7) * np.float32(255.0) + np.float32(0.5)) == 179
    assert d_of(9.0, "uint8", None) == 255
    # raw depth above 65504 reaches inf in float16, and stays finite in the other two
    assert np.isinf(d_of(70000.0, "float16", None)) and ob.bits(d_of(70000.0, "float16", None)) == 0x7C00
    assert _as_f32(np.array([d_of(70000.0, "bfloat16", None)]), "bfloat16")[0] == np.float32(70144.0)
    # a normalised value below 2^-14 is a float16 subnormal, the one NumPy's conversion gives
    t = np.float32(0.001) * (np.float32(1.0) / np.float32(20.0))
    assert 0 < t < 2.0 ** -14
    sub = d_of(0.001, "float16")
    assert 0 < int(ob.bits(np.array([sub]))[0]) < 0x0400 and sub.tobytes() == np.float32(t).astype(np.float16).tobytes()
    for dtype in FLOATS:
        assert _as_f32(np.array([d_of(10.0, dtype)]), dtype)[0] == 0.5


def test_the_bfloat16_of_the_oracle_is_torch_s():
    import torch
    rng = np.random.default_rng(15)
    x = np.concatenate([rng.uniform(-3.0, 3.0, 4000), rng.uniform(0.0, 1.0, 4000), 10.0 ** rng.uniform(-30, 30, 4000),
                        np.arange(256) / 255.0, [0.0, 1.0, 65504.0, 70000.0, np.inf, 2.0 ** -133, 3.3895314e38]]).astype(np.float32)
    # ties: exactly half way between two bfloat16 values, on both parities
    ties = (np.arange(0x3F80, 0x3FC0, dtype=np.uint32) << 16 | 0x8000).view(np.float32)
    x = np.concatenate([x, ties, -ties])
    want = torch.tensor(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(ob.bf16_bits(x), want)


def test_the_stack_written_out_by_hand():
    """S = 3, four views of one pixel of one channel; frame k holds 10 * k + view.  Views 1 and 3 are reset at push 3."""
    st = ob.Stack(3)

    def frame(k):
        return (10 * k + np.arange(4)).astype(np.uint8).reshape(4, 1, 1, 1)

    want = {
        1: [[10, 10, 10], [11, 11, 11], [12, 12, 12], [13, 13, 13]],           # the first push fills every stack
        2: [[10, 10, 20], [11, 11, 21], [12, 12, 22], [13, 13, 23]],
        3: [[10, 20, 30], [31, 31, 31], [12, 22, 32], [33, 33, 33]],           # views 1 and 3 restart
        4: [[20, 30, 40], [31, 31, 41], [22, 32, 42], [33, 33, 43]],
        5: [[30, 40, 50], [31, 41, 51], [32, 42, 52], [33, 43, 53]],
    }
    for k in range(1, 6):
        t = st.push(frame(k), np.array([False, True, False, True]) if k == 3 else None)
        assert t.shape == (4, 3, 1, 1) and t[:, :, 0, 0].tolist() == want[k], k
    # two channels: channel f * C + c is channel c of frame f
    st = ob.Stack(2)
    a = np.array([1, 2], np.uint8).reshape(1, 2, 1, 1)
    st.push(a)
    assert st.push(a + 10)[0, :, 0, 0].tolist() == [1, 2, 11, 12]
    assert st.push(a + 20)[0, :, 0, 0].tolist() == [11, 12, 21, 22]
    # no stack: the tensor is the frame
    assert ob.Stack(1).push(a)[0, :, 0, 0].tolist() == [1, 2]


@pytest.mark.parametrize("layout", list(ob.LAYOUTS))
def test_the_raytracer_packing_is_the_rasterizer_packing_of_the_transposed_image(layout):
    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 256, (3, 12, 12, 4), dtype=np.uint8)
    d = rng.uniform(0.0, 30.0, (3, 12, 12)).astype(np.float32)
    d[rng.random(d.shape) < 0.25] = 0.0
    for dtype in ob.DTYPES:
        ra = ob.pack(rgb, d, layout, dtype, (0.5, 20.0), False)
        rt = ob.pack(rgb.transpose(0, 2, 1, 3), d.transpose(0, 2, 1), layout, dtype, (0.5, 20.0), True)
        assert ra.shape == (3, ob.CHANNELS[layout], 12, 12) and np.array_equal(ob.bits(ra), ob.bits(rt))


def test_scene_desc_carries_the_option():
    d = scenes.synthetic_scene(3, width=40, height=24)
    assert d.observations is None
    d.observations = dict(channels="rgbd", dtype="float16", stack=4, depth_range=(0.1, 20.0))
    assert d.shard(1, 2).observations == d.observations


def test_the_new_abi_names_beside_the_unchanged_old_ones(native):
    m = native.load_module()
    assert m.MRX_FLAG_OBS_SHIFT == 23 and m.MRX_FLAG_OBS_MASK == 0xFF << 23
    assert m.MRX_FLAG_OBS_LAYOUT_MASK == 7 << 23 and m.MRX_FLAG_OBS_DTYPE_MASK == 3 << 26 and m.MRX_FLAG_OBS_STACK_MASK == 7 << 28
    assert m.MRX_FLAG_OBSERVATIONS(2, 1, 4) == (2 << 23) | (1 << 26) | (3 << 28) == ob.field("rgbd", "float16", 4)
    assert m.MRX_FLAG_OBSERVATIONS(5, 3, 8) == (5 << 23) | (3 << 26) | (7 << 28) < 1 << 31
    assert m.MRX_BUF_OBSERVATION == 16 and m.MRX_BUF_OBSERVATION_RESET == 17 and m.MRX_NUM_BUFFERS_EXT6 == 18
    assert m.MRX_DTYPE_F16 == 3 and m.MRX_DTYPE_BF16 == 4
    assert m.MRX_BUF_BOXES == 15 and m.MRX_NUM_BUFFERS_EXT5 == 16 and m.MRX_FLAG_BOX_LABELS_MASK == 0x7FF << 12
    assert m.MRX_CONFIG_SIZE == ctypes.sizeof(Cfg)         # mrx_config did not grow
    lib = native.load_capi()
    lib.mrx_abi_version.restype = ctypes.c_int
    assert lib.mrx_abi_version() == 4
    lo, hi = ctypes.c_float(), ctypes.c_float()
    for name, types, args in (("mrx_observations", [ctypes.c_void_p], (None,)),
                              ("mrx_observe", [ctypes.c_void_p], (None,)),
                              ("mrx_set_observation_depth_range", [ctypes.c_void_p, ctypes.c_float, ctypes.c_float], (None, 0.1, 20.0)),
                              ("mrx_observation_depth_range", [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)],
                               (None, ctypes.byref(lo), ctypes.byref(hi)))):
        assert hasattr(lib, name)
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = types
        assert getattr(lib, name)(*args) == MRX_E_INVALID
    for name in ("observations", "observation_tensor", "observation_reset_tensor", "observe", "set_observation_depth_range"):
        assert hasattr(m.MadronaRenderer, name)


def _field(layout, dtype, stack):
    return (layout << 23) | (dtype << 26) | ((stack - 1) << 28)


def test_mrx_create_checks_the_field_ahead_of_the_device(native):
    lib = native.load_capi()
    lib.mrx_last_error.restype = ctypes.c_char_p
    ok = 0 if has_gpu() else MRX_E_NO_DEVICE
    size = ctypes.sizeof(Cfg)
    ras = scenes.synthetic_scene(2, width=16, height=12)
    ray = scenes.synthetic_scene(2, width=16, height=16, render_mode="Raytracer")
    colour, depth = (1, 2, 4, 5), (2, 3, 5)
    n = 0
    for desc in (ras, ray):
        for layout in range(1, 6):
            for dtype, stack in ((0, 1), (3, 8)):
                if layout in colour:
                    assert _create(lib, desc, size, None, flags=_field(layout, dtype, stack) | NO_RGB) == MRX_E_INVALID
                    msg = lib.mrx_last_error()
                    assert b"MRX_FLAG_OBSERVATIONS" in msg and b"MRX_FLAG_NO_RGB" in msg, msg
                if layout in depth:
                    assert _create(lib, desc, size, None, flags=_field(layout, dtype, stack) | NO_DEPTH) == MRX_E_INVALID
                    msg = lib.mrx_last_error()
                    assert b"MRX_FLAG_OBSERVATIONS" in msg and b"MRX_FLAG_NO_DEPTH" in msg, msg
        for layout in (6, 7):
            for dtype, stack in ((0, 1), (2, 5)):
                assert _create(lib, desc, size, None, flags=_field(layout, dtype, stack)) == MRX_E_INVALID
                assert b"MRX_FLAG_OBSERVATIONS" in lib.mrx_last_error()
        for dtype, stack in ((1, 1), (0, 2), (3, 8), (2, 1), (0, 8)):   # element type or stack bits without a layout
            assert _create(lib, desc, size, None, flags=_field(0, dtype, stack)) == MRX_E_INVALID
            assert b"MRX_FLAG_OBSERVATIONS" in lib.mrx_last_error()
        assert _create(lib, desc, size, None, flags=_field(2, 1, 4), reserved=1) == MRX_E_INVALID
    # every valid value of every part of the field beside each option it combines with: the output selections (where
    # the layout can be fed), normals, labels, visibility ids, supersampling, positions, boxes -- the element type and
    # the stack cycle, so that every option meets all 4 and all 8
    boxes = (8 << 12) | LABELS
    options = (0, NO_RGB, NO_DEPTH, NORMALS, LABELS, VISIBILITY_IDS, 1 << 8, 3 << 8, POSITIONS, boxes)
    for oi, more in enumerate(options):
        for layout in range(1, 6):
            if (more == NO_RGB and layout in colour) or (more == NO_DEPTH and layout in depth):
                continue
            for rep in range(2):
                n += 1
                dtype, stack = (n + oi) % 4, 1 + (3 * n + oi) % 8
                desc = ray if n % 2 else ras
                assert _create(lib, desc, size, None, flags=_field(layout, dtype, stack) | more) == ok, (layout, dtype, stack, more)
    # ... and the field zero: the renderer it always was
    assert _create(lib, ras, size, None, flags=0) == ok


def test_the_python_constructor_refuses_a_malformed_option(native):
    bad = ["rgba", "", "RGB", 3, 1.5, True, ["rgb"], b"rgb",
           dict(dtype="float16"), dict(channels="rgbx"), dict(channels=2), dict(channels="rgb", dtype="float64"),
           dict(channels="rgb", dtype=16), dict(channels="rgb", stack=0), dict(channels="rgb", stack=9),
           dict(channels="rgb", stack=2.0), dict(channels="rgb", stack=True), dict(channels="rgb", frames=4),
           dict(channels="rgb", Stack=4), {"channels": "rgb", 3: 4},
           dict(channels="rgbd", depth_range=(0.0, 0.0)), dict(channels="rgbd", depth_range=(5.0, 1.0)),
           dict(channels="rgbd", depth_range=(-1.0, 1.0)), dict(channels="rgbd", depth_range=(0.0, float("inf"))),
           dict(channels="rgbd", depth_range=(float("nan"), 1.0)), dict(channels="rgbd", depth_range=(1.0,)),
           dict(channels="rgbd", depth_range=(0.0, 1.0, 2.0)), dict(channels="rgbd", depth_range=5.0),
           dict(channels="rgbd", depth_range=("0", "1")), dict(channels="rgb", depth_range=(0.1, 20.0)),
           dict(channels="y", depth_range=(0.1, 20.0))]
    for arg in bad:
        desc = scenes.synthetic_scene(2)
        desc.observations = arg
        with pytest.raises(ValueError, match="observations"):
            scenes.make_renderer(desc)
    # a layout the render_outputs setting cannot feed
    for arg, outputs in (("rgb", "Depth"), ("y", "Depth"), ("rgbd", "Depth"), ("yd", "Depth"), ("d", "RGB"), ("rgbd", "RGB"),
                         (dict(channels="yd", dtype="uint8"), "RGB")):
        desc = scenes.synthetic_scene(2)
        desc.observations = arg
        with pytest.raises(ValueError, match="observations"):
            scenes.make_renderer(desc, render_outputs=outputs)
    if not has_gpu():
        good = [None, False, "rgb", "rgbd", "d", "y", "yd", dict(channels="rgbd", dtype="float16", stack=4, depth_range=(0.1, 20.0)),
                dict(channels="d", dtype="bfloat16", depth_range=[0, 1]), dict(channels="yd", dtype="uint8", stack=8, depth_range=None)]
        for arg in good:
            desc = scenes.synthetic_scene(2)
            desc.observations = arg
            with pytest.raises(RuntimeError, match="no HIP device"):
                scenes.make_renderer(desc)
        desc = scenes.synthetic_scene(2)
        desc.observations = "d"
        with pytest.raises(RuntimeError, match="no HIP device"):
            scenes.make_renderer(desc, render_outputs="Depth")


def test_headless_refuses_malformed_observation_options(native, tmp_path):
    from madrona_renderer_amd import build
    exe = build.headless_path()
    args = ["4", "1", "rast", "64", "64"]
    for bad, flag in ((["--observations", "rgba"], "--observations"), (["--observations", ""], "--observations"),
                      (["--observations", "rgb,float64"], "--observations"), (["--observations", "rgb,float16,0"], "--observations"),
                      (["--observations", "rgb,float16,9"], "--observations"), (["--observations", "rgb,float16,2,1"], "--observations"),
                      (["--observations", "rgb,,2"], "--observations"), (["--observations", "rgb,float16,two"], "--observations"),
                      (["--observations", "rgb", "--outputs", "depth"], "--observations"),
                      (["--outputs", "rgb", "--observations", "yd,uint8"], "--observations"),
                      (["--observations", "rgbd", "--obs-depth-range", "5"], "--obs-depth-range"),
                      (["--observations", "rgbd", "--obs-depth-range", "5,1"], "--obs-depth-range"),
                      (["--observations", "rgbd", "--obs-depth-range", "-1,1"], "--obs-depth-range"),
                      (["--observations", "rgbd", "--obs-depth-range", "0,inf"], "--obs-depth-range"),
                      (["--observations", "rgbd", "--obs-depth-range", "0,1,2"], "--obs-depth-range"),
                      (["--observations", "rgbd", "--obs-depth-range", "a,b"], "--obs-depth-range"),
                      (["--observations", "rgb", "--obs-depth-range", "0.1,20"], "--obs-depth-range"),
                      (["--obs-depth-range", "0.1,20"], "--obs-depth-range")):
        p = subprocess.run(["timeout", "-k", "5", "60", exe] + args + bad + ["--dump-last-frame", "out"], cwd=tmp_path,
                           capture_output=True, text=True)
        assert p.returncode not in (0, 124, 137), bad
        assert flag in p.stderr, (bad, p.stderr)
    if not has_gpu():
        # a well-formed option gets as far as the device
        for good in (["--observations", "rgb"], ["--observations", "rgbd,float16,4", "--obs-depth-range", "0.1,20"],
                     ["--observations", "d,bfloat16", "--outputs", "depth"], ["--observations", "y,uint8,8", "--outputs", "rgb"]):
            p = subprocess.run(["timeout", "-k", "5", "60", exe] + args + good, cwd=tmp_path, capture_output=True, text=True)
            assert p.returncode not in (0, 124, 137) and "--obs" not in p.stderr, (good, p.stderr)
    assert not list(tmp_path.iterdir())


def test_the_observe_kernels_use_no_scratch_and_spill_nothing():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources
    kernels = kernel_resources.resources(os.path.join(ROOT, "madrona_renderer_amd", "csrc", "observe.hip"))
    names = [k["name"] for k in kernels]
    assert len(kernels) == 12, names                         # element type (4) x form (narrow, wide, tile)
    for dtype in range(4):
        for form in range(3):
            assert sum("observeKernel<%du, %du>" % (dtype, form) in n for n in names) == 1, names
    for k in kernels:
        assert int(k["ScratchSize [bytes/lane]"]) == 0, k
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, k
        if ", 2u>" not in k["name"]:                         # the x-fast forms stream: every wave slot
            assert int(k["Occupancy [waves/SIMD]"]) == 8, k
        else:                                                # the LDS form's occupancy is recorded in the table below
            assert int(k["Occupancy [waves/SIMD]"]) >= 1, k
    have = [l.rstrip("\n") for l in open(os.path.join(ROOT, "profiles", "kernel_resources_observe.txt"))
            if not l.startswith("#")]
    assert have == [kernel_resources.line(k) for k in kernels], \
        "stale: regenerate profiles/kernel_resources_observe.txt (its header says how)"
