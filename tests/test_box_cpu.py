"""Box labels on the host (no GPU): known answers of the NumPy restatement the GPU tests compare
against (tests/box_oracle.py), the C ABI's new names beside the unchanged old ones, mrx_create's argument checks ahead
of the device probe, the box stage's launch checks and grid rule through mrx_box_plan, SceneDesc carrying the option,
the Python constructor's ValueError, the headless option's refusal, and the box kernels' resources as the compiler
reports them."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from madrona_renderer_amd import scenes
from tests import box_oracle as bx
from tests.conftest import ROOT, has_gpu
from tests.test_color_cpu import Cfg, _create

MRX_E_INVALID, MRX_E_NO_DEVICE, MRX_E_UNSUPPORTED = -1, -2, -5
VISIBILITY_IDS, NO_RGB, NO_DEPTH, NORMALS, LABELS, POSITIONS = 1 << 0, 1 << 2, 1 << 3, 1 << 6, 1 << 7, 1 << 10
SHIFT = 12


def K(k):
    return k << SHIFT


def _empty(views, k, w, h):
    return np.broadcast_to(np.array([w, h, -1, -1, 0], np.int32), (views, k, 5))


def test_known_answer_the_anchor_quad_labelled_2():
    # S3's anchor (tests/test_oracle_anchors.py): the quad fills exactly the pixels [16, 48)^2 of a 64 x 64 view
    ids = np.full((1, 64, 64), -1, np.int32)
    ids[0, 16:48, 16:48] = 2
    got = bx.boxes(ids, 5, False)
    assert got.dtype == np.int32 and got.shape == (1, 5, 5)
    assert got[0, 2].tolist() == [16, 16, 47, 47, 1024]
    others = np.delete(got, 2, axis=1)
    assert np.array_equal(others, _empty(1, 4, 64, 64))


def test_a_single_pixel_and_a_label_touching_all_four_borders():
    ids = np.full((2, 5, 7), -1, np.int32)                  # 7 wide, 5 high
    ids[0, 3, 6] = 0
    ids[1, 0, 2] = ids[1, 4, 3] = ids[1, 2, 0] = ids[1, 1, 6] = 1
    got = bx.boxes(ids, 2, False)
    assert got[0, 0].tolist() == [6, 3, 6, 3, 1] and got[0, 1].tolist() == [7, 5, -1, -1, 0]
    assert got[1, 1].tolist() == [0, 0, 6, 4, 4] and got[1, 0].tolist() == [7, 5, -1, -1, 0]


@pytest.mark.parametrize("k", [1, 5, 64, 1024])
def test_the_raytracer_result_of_a_transposed_tensor_is_the_rasterizer_result(k):
    rng = np.random.default_rng(k)
    ids = bx.labels(rng, (3, 12, 12), k)
    ra = bx.boxes(ids, k, False)
    rt = bx.boxes(np.ascontiguousarray(ids.transpose(0, 2, 1)), k, True)
    assert np.array_equal(ra, rt)
    assert (ra[:, k - 1, 4] > 0).any()                      # label K-1 is there ...
    if k > 1:
        assert (ra[..., 4] == 0).any()                      # ... and some row is empty


def test_out_of_range_and_negative_ids_count_nowhere_and_counts_add_up():
    rng = np.random.default_rng(3)
    for k in (1, 5, 64):
        ids = bx.labels(rng, (4, 9, 13), k)
        got = bx.boxes(ids, k, False)
        inrange = (ids.view(np.uint32) < k).reshape(4, -1).sum(axis=1)
        assert np.array_equal(got[..., 4].sum(axis=1), inrange)
        for odd in (-1, -2, k, k + 7, bx.INT32_MIN, bx.INT32_MAX):
            assert (ids == odd).any(), odd
        # the ids outside 0 ... K-1 replaced by background: the same tensor
        clean = np.where(ids.view(np.uint32) < k, ids, -1).astype(np.int32)
        assert np.array_equal(bx.boxes(clean, k, False), got)
        full = got[..., 4] > 0
        assert (got[full][:, 0] <= got[full][:, 2]).all() and (got[full][:, 1] <= got[full][:, 3]).all()
        assert np.array_equal(got[~full], _empty(1, int((~full).sum()), 13, 9)[0])


def test_scene_desc_carries_the_option():
    d = scenes.synthetic_scene(3, width=40, height=24)
    assert d.boxes is None
    d.boxes = 8
    assert d.shard(1, 2).boxes == 8


def test_the_new_abi_names_beside_the_unchanged_old_ones(native):
    m = native.load_module()
    assert m.MRX_FLAG_BOX_LABELS_SHIFT == 12 and m.MRX_FLAG_BOX_LABELS_MASK == 0x7FF << 12
    assert m.MRX_BUF_BOXES == 15 and m.MRX_NUM_BUFFERS_EXT5 == 16
    assert m.MRX_BUF_POSITION == 14 and m.MRX_NUM_BUFFERS_EXT4 == 15 and m.MRX_FLAG_POSITIONS == POSITIONS
    assert m.MRX_CONFIG_SIZE == ctypes.sizeof(Cfg)         # mrx_config did not grow
    lib = native.load_capi()
    lib.mrx_abi_version.restype = ctypes.c_int
    assert lib.mrx_abi_version() == 4
    for name in ("mrx_boxes", "mrx_box_labels"):
        assert hasattr(lib, name)
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = [ctypes.c_void_p]
        assert getattr(lib, name)(None) == MRX_E_INVALID
    for name in ("box_labels", "box_tensor", "boxes"):
        assert hasattr(m.MadronaRenderer, name)


def test_mrx_create_checks_the_field_ahead_of_the_device(native):
    lib = native.load_capi()
    lib.mrx_last_error.restype = ctypes.c_char_p
    ok = 0 if has_gpu() else MRX_E_NO_DEVICE
    size = ctypes.sizeof(Cfg)
    ras = scenes.synthetic_scene(2, width=16, height=12)
    ray = scenes.synthetic_scene(2, width=16, height=16, render_mode="Raytracer")
    for desc, need in ((ras, LABELS), (ray, 0), (ray, LABELS)):
        for k in (1, 8, 1024):
            # ... beside everything it combines with: each output selection, normals, positions, supersampling
            for more in (0, NO_RGB, NO_DEPTH, NORMALS, POSITIONS, 1 << 8, 3 << 8, NO_RGB | NORMALS | (2 << 8)):
                assert _create(lib, desc, size, None, flags=K(k) | need | more) == ok, (k, need, more)
            assert _create(lib, desc, size, None, flags=K(k) | need | VISIBILITY_IDS) == MRX_E_INVALID
            msg = lib.mrx_last_error()
            assert b"MRX_FLAG_BOX_LABELS" in msg and b"MRX_FLAG_VISIBILITY_IDS" in msg, msg
        for k in (1025, 2047):
            assert _create(lib, desc, size, None, flags=K(k) | need) == MRX_E_INVALID
            assert b"1024" in lib.mrx_last_error()
        assert _create(lib, desc, size, None, flags=K(8) | need, reserved=1) == MRX_E_INVALID
    assert _create(lib, ras, size, None, flags=K(8)) == MRX_E_INVALID
    msg = lib.mrx_last_error()
    assert b"MRX_FLAG_BOX_LABELS" in msg and b"MRX_FLAG_INSTANCE_LABELS" in msg, msg
    # the field zero: the renderer it always was
    assert _create(lib, ras, size, None, flags=0) == ok


def _plan(lib, views, nfast, nslow, k, cus=256, forced=0, null=0):
    lib.mrx_box_plan.restype = ctypes.c_int
    lib.mrx_box_plan.argtypes = [ctypes.c_uint32] * 6 + [ctypes.c_int]
    return lib.mrx_box_plan(views, nfast, nslow, k, cus, forced, null)


def test_the_launch_checks_and_the_grid_rule(native):
    lib = native.load_capi()
    assert _plan(lib, 0, 64, 64, 8) == 0 and _plan(lib, 3, 0, 64, 8) == 0       # zero views, no pixels: nothing to do
    for k in (0, 1025, 2 ** 31):
        assert _plan(lib, 3, 64, 64, k) == MRX_E_INVALID
    assert _plan(lib, 3, 64, 64, 8, null=1) == MRX_E_INVALID
    assert _plan(lib, 0, 64, 64, 8, null=1) == MRX_E_INVALID
    assert _plan(lib, 3, 64, 64, 8, cus=0) == MRX_E_INVALID
    # 2^32 - 1 native pixels is the most: 65537 * 65535 = 2^32 - 1
    assert _plan(lib, 65537, 65535, 1, 8) == 1
    assert _plan(lib, 65536, 65536, 1, 8) == MRX_E_INVALID
    assert _plan(lib, 1 << 16, 1 << 8, 1 << 8, 8) == MRX_E_INVALID
    # one workgroup per view from 2 * CUs views on; below, the smallest count that gives 2 * CUs, capped at ceil(nslow / 4)
    assert _plan(lib, 512, 64, 64, 8) == 1 and _plan(lib, 1024, 64, 64, 8) == 1
    assert _plan(lib, 511, 64, 64, 8) == 2 and _plan(lib, 256, 64, 64, 8) == 2 and _plan(lib, 255, 64, 64, 8) == 3
    assert _plan(lib, 3, 64, 64, 8) == 16 and _plan(lib, 3, 64, 65, 8) == 17 and _plan(lib, 3, 64, 4, 8) == 1
    assert _plan(lib, 3, 64, 5, 8) == 2 and _plan(lib, 3, 1, 1, 8) == 1
    assert _plan(lib, 2, 64, 64, 8, cus=1) == 1 and _plan(lib, 2, 64, 64, 8, cus=4) == 4
    assert _plan(lib, 40, 7, 5, 8, cus=1) == 1
    # MRX_BOX_PARTS forces the count, up to the cap
    assert _plan(lib, 3, 7, 5, 8, forced=3) == 2 and _plan(lib, 3, 40, 24, 8, forced=3) == 3
    assert _plan(lib, 1024, 64, 64, 8, forced=3) == 3 and _plan(lib, 3, 64, 64, 8, forced=1) == 1


def test_the_python_constructor_refuses_anything_but_a_count(native):
    for bad in (-1, 1025, "8", 2.5, True, [8]):
        desc = scenes.synthetic_scene(2, render_mode="Raytracer")
        desc.boxes = bad
        with pytest.raises(ValueError, match="boxes"):
            scenes.make_renderer(desc)
    if not has_gpu():
        for good in (1, 8, 1024, 0, False, None):
            desc = scenes.synthetic_scene(2, render_mode="Raytracer")
            desc.boxes = good
            with pytest.raises(RuntimeError, match="no HIP device"):
                scenes.make_renderer(desc)


def test_headless_refuses_boxes_without_a_segmask(native, tmp_path):
    from madrona_renderer_amd import build
    exe = build.headless_path()
    args = ["4", "1", "rast", "64", "64"]
    for bad in (["--boxes", "8"], ["--boxes", "0", "--instance-labels", "1"], ["--boxes", "1025", "--instance-labels", "1"],
                ["--boxes", "-3", "--instance-labels", "1"], ["--boxes", "eight", "--instance-labels", "1"]):
        p = subprocess.run(["timeout", "-k", "5", "60", exe] + args + bad, cwd=tmp_path, capture_output=True, text=True)
        assert p.returncode not in (0, 124, 137), bad
        assert "--boxes" in p.stderr, (bad, p.stderr)
    if not has_gpu():
        # a well-formed option gets as far as the device
        for good in (args + ["--boxes", "8", "--instance-labels", "1"], ["4", "1", "rt", "64", "64", "--boxes", "8"]):
            p = subprocess.run(["timeout", "-k", "5", "60", exe] + good, cwd=tmp_path, capture_output=True, text=True)
            assert p.returncode not in (0, 124, 137) and "--boxes" not in p.stderr, (good, p.stderr)
    assert not list(tmp_path.iterdir())


def test_the_box_kernels_use_no_scratch_and_spill_nothing():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources
    kernels = kernel_resources.resources(os.path.join(ROOT, "madrona_renderer_amd", "csrc", "boxes.hip"))
    names = [k["name"] for k in kernels]
    assert len(kernels) == 2, names                          # the reduction and the fill
    assert sum("boxKernel(" in n for n in names) == 1 and sum("boxFillKernel(" in n for n in names) == 1, names
    for k in kernels:
        assert int(k["ScratchSize [bytes/lane]"]) == 0, k
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, k
        assert int(k["Occupancy [waves/SIMD]"]) == 8, k
    have = [l.rstrip("\n") for l in open(os.path.join(ROOT, "profiles", "kernel_resources_boxes.txt"))
            if not l.startswith("#")]
    assert have == [kernel_resources.line(k) for k in kernels], \
        "stale: regenerate profiles/kernel_resources_boxes.txt (its header says how)"
