"""Per-instance labels on the host (no GPU): the helper the GPU tests compare against
(tests/label_oracle.py) is pinned to the C oracle -- with every row at the sentinel it is the oracle's segmask byte for
byte on every golden scene, in both modes, with hidden rows and after refresh_objects(), which pins its row numbering
-- labels are stored as they are and a sentinel row follows its binding, SceneDesc and its shards carry the labels with
their rows, the C ABI's new names are there beside the unchanged old ones, the setters check their arguments,
make_renderer rejects a wrong length before the device is touched and the headless binary refuses a malformed
--instance-labels."""
import ctypes
import subprocess

import numpy as np
import pytest

from madrona_renderer_amd import scenes
from tests import label_oracle as lb
from tests import meshes
from tests.conftest import has_gpu
from tests.golden.make_golden import cases
from tests.test_color_cpu import Cfg, _create

MRX_E_INVALID, MRX_E_NO_DEVICE, MRX_E_UNSUPPORTED = -1, -2, -3
FLAG = 1 << 7


def test_the_new_abi_names_beside_the_unchanged_old_ones(native):
    m = native.load_module()
    assert m.MRX_FLAG_INSTANCE_LABELS == FLAG
    assert m.MRX_BUF_INSTANCE_LABEL == 13 and m.MRX_NUM_BUFFERS_EXT3 == 14
    assert m.MRX_LABEL_OBJECT == -2 ** 31 == lb.SENTINEL == scenes.LABEL_OBJECT
    assert m.MRX_NUM_BUFFERS == 11 and m.MRX_NUM_BUFFERS_EXT == 12 and m.MRX_NUM_BUFFERS_EXT2 == 13
    assert m.MRX_BUF_NORMAL == 12 and m.MRX_BUF_INSTANCE_MATERIAL == 11 and m.MRX_BUF_INSTANCE_COLOR == 10
    assert m.MRX_FLAG_NORMALS == 1 << 6 and m.MRX_FLAG_INSTANCE_MATERIALS == 1 << 5 and m.MRX_FLAG_INSTANCE_COLORS == 1 << 4
    assert m.MRX_CONFIG_SIZE == ctypes.sizeof(Cfg)         # mrx_config did not grow
    lib = native.load_capi()
    lib.mrx_abi_version.restype = ctypes.c_int
    assert lib.mrx_abi_version() == 4
    ok = 0 if has_gpu() else MRX_E_NO_DEVICE
    for desc in (scenes.synthetic_scene(3), scenes.synthetic_scene(3, render_mode="Raytracer")):
        assert _create(lib, desc, ctypes.sizeof(Cfg), None, flags=FLAG) == ok
        assert _create(lib, desc, ctypes.sizeof(Cfg), None, flags=FLAG | 1) == ok          # beside visibility ids
        assert _create(lib, desc, ctypes.sizeof(Cfg), None, flags=FLAG | (1 << 2)) == ok   # depth only
        assert _create(lib, desc, ctypes.sizeof(Cfg), None, flags=FLAG, reserved=1) == MRX_E_INVALID
    for name in ("instance_label_tensor", "set_instance_labels", "instance_labels"):
        assert hasattr(m.MadronaRenderer, name)


def test_the_setters_check_their_arguments(native):
    lib = native.load_capi()
    labels = (ctypes.c_int32 * 4)(1000, -1, -2 ** 31, 2 ** 31 - 1)
    for fn in (lib.mrx_set_instance_labels, lib.mrx_instance_labels):
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_int32)]
        assert fn(None, 0, 4, labels) == MRX_E_INVALID
        assert fn(None, 0, 0, None) == MRX_E_INVALID
    lib.mrx_last_error.restype = ctypes.c_char_p
    assert b"null renderer" in lib.mrx_last_error()


SCENES = dict(cases())
SCENES["cube-field"] = meshes.cube_field(3, 40)
SCENES["cube-field-rt"] = meshes.cube_field(2, 40, mode="Raytracer", textured=True)


@pytest.mark.parametrize("name", list(SCENES))
def test_an_all_sentinel_column_is_the_oracles_segmask_byte_for_byte(oracle_mod, name):
    desc = SCENES[name]
    fs = oracle_mod.FlatScene(desc)
    ref = fs.render()
    got = lb.segmask(fs, lb.expand(desc), ref["tri_id"])
    assert got.dtype == np.int32 and np.array_equal(got.view(np.uint8), ref["segmask"].view(np.uint8))
    assert (ref["tri_id"] >= 0).any()
    # hidden rows: they keep their slots, the rows behind them keep their numbers
    rows = len(fs.inst_obj)
    hidden = list(range(0, rows, 3))
    fs.inst_obj[hidden] = -1 - np.arange(len(hidden), dtype=np.int32)
    hid = fs.render()
    assert not np.array_equal(hid["tri_id"], ref["tri_id"])
    got = lb.segmask(fs, lb.expand(desc), hid["tri_id"])
    assert np.array_equal(got.view(np.uint8), hid["segmask"].view(np.uint8))


def test_an_all_sentinel_column_follows_refresh_objects(oracle_mod):
    desc = scenes.synthetic_scene(6, with_wall=True)
    desc.max_instances_per_world = 4                      # three rows bound, one spare
    fs = oracle_mod.FlatScene(desc)
    col = lb.expand(desc)
    assert col.shape == (24,) and (col == lb.SENTINEL).all()
    ref = fs.render()
    assert np.array_equal(lb.segmask(fs, col, ref["tri_id"]), ref["segmask"])     # the unbound rows: no slots
    spare = list(range(3, 24, 4))
    fs.inst_obj[spare] = 0
    fs.inst_pos[spare] = (1.5, -2.0, 2.0)
    fs.inst_obj[0::4] = fs.inst_obj0[1::4]                # ... and the first row of every world swaps its object
    fs.refresh_objects()
    new = fs.render()
    assert not np.array_equal(new["segmask"], ref["segmask"])
    assert np.array_equal(lb.segmask(fs, col, new["tri_id"]).view(np.uint8), new["segmask"].view(np.uint8))


def test_labels_are_stored_as_they_are_and_sentinel_rows_resolve_to_their_object(oracle_mod):
    desc = scenes.synthetic_scene(5, with_wall=True)
    fs = oracle_mod.FlatScene(desc)
    ref = fs.render()
    labels = np.resize(np.array([-1, -2, 2 ** 31 - 1, -2 ** 31 + 1, lb.SENTINEL, 7], np.int64), len(desc.instances))
    col = lb.expand(desc, labels.astype(np.int32))
    got = lb.segmask(fs, col, ref["tri_id"])
    owner = lb.owner_rows(fs, ref["tri_id"], 0, fs.num_views)
    assert np.array_equal(owner >= 0, ref["tri_id"] >= 0) and (got[owner < 0] == -1).all()
    for row in np.unique(owner[owner >= 0]):
        want = int(fs.inst_obj0[row]) if col[row] == lb.SENTINEL else int(col[row])
        assert (got[owner == row] == want).all(), row
    assert {-2, 2 ** 31 - 1, -2 ** 31 + 1, 7} <= set(np.unique(got).tolist())
    m = lb.mixed(40)
    assert m.dtype == np.int32 and (m[1::4] == lb.SENTINEL).all()
    rest = np.delete(m, np.arange(1, 40, 4))
    assert ((rest >= 1000) & (rest < 2000)).all()


def test_scene_desc_and_its_shards_carry_the_labels_with_the_rows():
    assert scenes.synthetic_scene(2).instance_labels is None
    for desc in (scenes.synthetic_scene(7, with_wall=True), scenes.demo_scene(5)):
        desc.instance_labels = lb.mixed(len(desc.instances))
        desc.max_instances_per_world = 4
        whole = lb.expand(desc)
        assert whole.shape == (4 * desc.num_worlds,) and whole.dtype == np.int32
        parts = [lb.expand(desc.shard(r, 3)) for r in range(3)]
        assert np.array_equal(np.concatenate(parts), whole)
        for w, (ni, io, _, _) in enumerate(desc.worlds):   # worlds that alias rows share their labels
            assert np.array_equal(whole[4 * w:4 * w + ni], desc.instance_labels[io:io + ni])
            assert (whole[4 * w + ni:4 * w + 4] == lb.SENTINEL).all()   # spare rows: the sentinel
    desc.instance_labels = True
    assert (lb.expand(desc) == lb.SENTINEL).all()


def test_make_renderer_checks_the_labels_before_the_device(native):
    desc = scenes.synthetic_scene(4)
    for bad in (np.zeros(7, np.int32), np.zeros((8, 2), np.int32), np.zeros((2, 4), np.int32)):
        desc.instance_labels = bad
        with pytest.raises(ValueError):
            scenes.make_renderer(desc)
    if not has_gpu():
        for good in (True, lb.mixed(8)):
            desc.instance_labels = good
            with pytest.raises(RuntimeError, match="no HIP device"):
                scenes.make_renderer(desc)


def test_headless_rejects_a_malformed_seed(native, tmp_path):
    from madrona_renderer_amd import build
    exe = build.headless_path()
    args = ["4", "1", "rast", "64", "64"]
    for bad in (["--instance-labels", "red"], ["--instance-labels", "-1"], ["--instance-labels", "1.5"],
                ["--instance-labels", ""], ["--instance-labels", "99999999999999999999999"],
                ["--instance-labels"]):
        p = subprocess.run(["timeout", "-k", "5", "60", exe] + args + bad, cwd=tmp_path, capture_output=True, text=True)
        assert p.returncode not in (0, 124, 137), bad
        assert "--instance-labels" in p.stderr, (bad, p.stderr)
