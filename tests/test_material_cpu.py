"""Per-instance material override on the host (no GPU): the helper the GPU tests compare against
(tests/material_oracle.py) is anchored -- with every id outside the table it is the plain oracle byte for byte, with
ids set only RGB changes, and a scene that imports the objects with those materials directly gives the same images,
which does not depend on the clone mechanism -- it composes with colours, lights and projections, SceneDesc and its
shards carry the ids with the rows, the C ABI's new names are there beside the unchanged old ones, the setters check
their arguments, and the headless binary refuses a malformed --instance-materials."""
import ctypes
import dataclasses
import os
import subprocess

import numpy as np
import pytest

from madrona_renderer_amd import scenes
from tests import color_oracle as co
from tests import light_oracle as lo
from tests import material_oracle as mo
from tests import projection_oracle as po
from tests.conftest import has_gpu
from tests.test_color_cpu import Cfg, _authored, _create

MRX_E_INVALID, MRX_E_NO_DEVICE, MRX_E_UNSUPPORTED = -1, -2, -3

SCENES = {
    "raster-wall": lambda: scenes.synthetic_scene(8, with_wall=True),
    "raytracer-textured": lambda: scenes.synthetic_scene(8, textured=True, render_mode="Raytracer"),
    "cube-field-textured": lambda: scenes.cube_field(4, 20, textured=True),
    "demo-aliased": lambda: scenes.demo_scene(3),
}


def test_the_new_abi_names_beside_the_unchanged_old_ones(native):
    m = native.load_module()
    assert m.MRX_FLAG_INSTANCE_MATERIALS == 1 << 5
    assert m.MRX_BUF_INSTANCE_MATERIAL == 11 and m.MRX_NUM_BUFFERS_EXT == 12
    assert m.MRX_NUM_BUFFERS == 11 and m.MRX_BUF_INSTANCE_COLOR == 10 and m.MRX_FLAG_INSTANCE_COLORS == 1 << 4
    assert m.MRX_CONFIG_SIZE == ctypes.sizeof(Cfg)         # mrx_config did not grow
    lib = native.load_capi()
    lib.mrx_abi_version.restype = ctypes.c_int
    assert lib.mrx_abi_version() == 4
    desc = scenes.synthetic_scene(3, textured=True)
    ok = 0 if has_gpu() else MRX_E_NO_DEVICE
    assert _create(lib, desc, ctypes.sizeof(Cfg), None, flags=1 << 5) == ok
    assert _create(lib, desc, ctypes.sizeof(Cfg), None, flags=(1 << 5) | (1 << 4)) == ok
    assert _create(lib, desc, ctypes.sizeof(Cfg), None, flags=1 << 5, reserved=1) == MRX_E_INVALID
    assert hasattr(m.MadronaRenderer, "instance_material_tensor")
    assert hasattr(m.MadronaRenderer, "set_instance_materials") and hasattr(m.MadronaRenderer, "instance_materials")


def test_the_setters_check_their_arguments(native):
    lib = native.load_capi()
    ids = (ctypes.c_int32 * 4)(0, 1, -1, 2)
    for fn in (lib.mrx_set_instance_materials, lib.mrx_instance_materials):
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_int32)]
        assert fn(None, 0, 4, ids) == MRX_E_INVALID
        assert fn(None, 0, 0, None) == MRX_E_INVALID
    lib.mrx_last_error.restype = ctypes.c_char_p
    assert b"null renderer" in lib.mrx_last_error()


@pytest.mark.parametrize("name", list(SCENES))
def test_ids_outside_the_table_are_the_plain_oracle_byte_for_byte(oracle_mod, name):
    desc = mo.with_table(SCENES[name]())
    n, nm = len(desc.instances), mo.num_materials(desc)
    plain = oracle_mod.FlatScene(desc).render()
    outside = np.resize(np.array([-1, -7, nm, nm + 5, 2 ** 31 - 1, -2 ** 31], np.int64), n).astype(np.int32)
    for got in (mo.render(desc, outside), mo.render(desc), mo.render(dataclasses.replace(desc, instance_materials=True)),
                mo.render_flat(oracle_mod.FlatScene(desc), mo.expand(desc, outside))):
        for k in ("rgb", "depth", "tri_id", "segmask"):
            assert np.array_equal(got[k].view(np.uint8), plain[k].view(np.uint8)), k


@pytest.mark.parametrize("name", list(SCENES))
def test_materials_change_rgb_and_nothing_else(oracle_mod, name):
    desc = mo.with_table(SCENES[name]())
    nm = mo.num_materials(desc)
    plain = oracle_mod.FlatScene(desc).render()
    ids = mo.mixed(len(desc.instances), nm)
    if name == "demo-aliased":
        ids[:] = [nm - 4, nm - 2][:len(ids)]               # (two rows: both overridden)
    got = mo.render(desc, ids)
    for k in ("depth", "tri_id", "segmask"):
        assert np.array_equal(got[k].view(np.uint8), plain[k].view(np.uint8)), k
    covered = plain["tri_id"] >= 0
    assert np.array_equal(got["rgb"][~covered], plain["rgb"][~covered])
    assert (got["rgb"][..., 3] == 255).all()
    # rows 1::4 are left alone: what only they cover keeps its colour
    rows = mo.expand(desc, ids)
    fs = oracle_mod.FlatScene(desc)
    for v in range(fs.num_views):
        w = int(fs.view_world[v])
        k = 0
        for i in range(fs.world_inst_start[w], fs.world_inst_start[w + 1]):
            n = int(fs.obj_num_tris[fs.inst_obj0[i]])
            mine = (plain["tri_id"][v] >= k) & (plain["tri_id"][v] < k + n)
            if rows[i] < 0:
                assert np.array_equal(got["rgb"][v][mine], plain["rgb"][v][mine])
            k += n
    assert mo.changed_fraction(got, plain) >= 0.4


def _table():
    tex = [os.path.join(scenes.DATA_DIR, "cube.png"), os.path.join(mo.GOLDEN, "rgba8_5x3.ktx2")]
    mats = [((1.0, 1.0, 1.0, 1.0), -1, 0.5, 0.5), ((1.0, 0.0, 0.0, 1.0), -1, 0.5, 0.5), ((0.3, 0.9, 0.6, 1.0), 0, 0.5, 0.5),
            ((0.9, 0.8, 0.2, 1.0), 1, 0.5, 0.5), ((0.2, 0.4, 0.8, 1.0), 7, 0.5, 0.5)]   # (the last: no such texture)
    return mats, tex


@pytest.mark.parametrize("mode", ["Rasterizer", "Raytracer"])
@pytest.mark.parametrize("ids", [(1, 2, 3), (-1, 3, 4), (2, 2, 0)])
def test_an_override_is_the_same_scene_imported_with_that_material(oracle_mod, mode, ids):
    """The anchor that does not depend on the clone mechanism: three objects of the same cube whose meshes name
    materials ids[0..2] directly, against one object under the column.  The cube's uvs are all zero: a textured material
    on it samples the texel S8 gives for (0, 0), in both."""
    mats, tex = _table()
    own = 0
    direct = [own if i < 0 else i for i in ids]
    a = _authored(1, mats, [0, 0, 0])
    a.texture_paths = tex
    a.instance_materials = np.array(ids, np.int32)
    # (_authored gives mesh m material m: permute the table so that mesh k finds material direct[k] at index k)
    others = [m for j, m in enumerate(mats) if j not in direct]
    b = _authored(3, [mats[j] for j in direct] + others, [0, 1, 2])
    b.texture_paths = tex
    a.render_mode = b.render_mode = mode
    ra, rb = mo.render(a), oracle_mod.FlatScene(b).render()
    for k in ("rgb", "depth", "tri_id"):
        assert np.array_equal(ra[k].view(np.uint8), rb[k].view(np.uint8)), k
    assert (ra["tri_id"] >= 0).mean() > 0.05 and len(np.unique(ra["rgb"].reshape(-1, 4), axis=0)) > 3
    assert set(np.unique(ra["segmask"])) == {-1, 0} and set(np.unique(rb["segmask"])) == {-1, 0, 1, 2}
    plain = oracle_mod.FlatScene(dataclasses.replace(a, instance_materials=None)).render()
    assert not np.array_equal(plain["rgb"], ra["rgb"])


def test_a_colour_override_replaces_the_rgb_of_the_material_in_effect(oracle_mod):
    mats, tex = _table()
    cs = np.array([[255, 0, 0, 255], [13, 200, 77, 0], [90, 90, 255, 128]], np.uint8)
    ids = np.array([2, 3, -1], np.int32)
    a = _authored(1, mats, [0, 0, 0])
    a.texture_paths = tex
    a.instance_materials, a.instance_colors = ids, cs
    # directly: row 0 = texture 0 under the override colour, row 1 = material 3 as it is, row 2 = the colour, untextured
    k = lambda c: tuple(float(np.float32(x) * co.K255) for x in c[:3]) + (1.0,)
    b = _authored(3, [(k(cs[0]), 0, 0.5, 0.5), mats[3], (k(cs[2]), -1, 0.5, 0.5)], [0, 1, 2])
    b.texture_paths = tex
    ra, rb = mo.render(a), oracle_mod.FlatScene(b).render()
    for key in ("rgb", "depth", "tri_id"):
        assert np.array_equal(ra[key].view(np.uint8), rb[key].view(np.uint8)), key
    assert set(np.unique(ra["segmask"])) == {-1, 0}
    fs = oracle_mod.FlatScene(a)
    rf = mo.render_flat(fs, mo.expand(a), co.expand(a))
    assert np.array_equal(rf["rgb"], ra["rgb"]) and np.array_equal(rf["segmask"], ra["segmask"])


def test_the_helper_composes_with_colours_lights_and_projections(oracle_mod):
    desc = mo.with_table(scenes.synthetic_scene(6, with_wall=True))
    ids = mo.mixed(len(desc.instances), mo.num_materials(desc))
    colors = co.mixed(len(desc.instances))
    lights, projs = lo.mixed(6, shift=1), po.mixed(6)
    got = mo.render(desc, ids, None, lights, projs)
    both = mo.render(desc, ids, colors, lights, projs)
    plain = lo.render(desc, lights, projs)
    assert oracle_mod.FlatScene.__name__ == "FlatScene"   # (the helpers' hooks are gone again)
    for k in ("depth", "tri_id", "segmask"):
        assert np.array_equal(got[k].view(np.uint8), plain[k].view(np.uint8)), k
        assert np.array_equal(both[k].view(np.uint8), plain[k].view(np.uint8)), k
    assert mo.changed_fraction(got, plain) >= 0.4
    assert mo.changed_fraction(both, got) >= 0.5          # the colours on top decide pixels too
    none = mo.render(desc, np.full(len(desc.instances), -1, np.int32), None, lights, projs)
    assert np.array_equal(none["rgb"], plain["rgb"])
    only = co.render(desc, colors, lights, projs)
    assert np.array_equal(mo.render(desc, None, colors, lights, projs)["rgb"], only["rgb"])


def test_scene_desc_and_its_shards_carry_the_ids_with_the_rows():
    assert scenes.synthetic_scene(2).instance_materials is None
    for desc in (scenes.synthetic_scene(7, with_wall=True), scenes.demo_scene(5)):
        desc.instance_materials = mo.mixed(len(desc.instances), 2)
        desc.max_instances_per_world = 4
        whole = mo.expand(desc)
        assert whole.shape == (4 * desc.num_worlds,) and whole.dtype == np.int32
        parts = [mo.expand(desc.shard(r, 3)) for r in range(3)]
        assert np.array_equal(np.concatenate(parts), whole)
        for w, (ni, io, _, _) in enumerate(desc.worlds):   # worlds that alias rows share their ids
            assert np.array_equal(whole[4 * w:4 * w + ni], desc.instance_materials[io:io + ni])
            assert (whole[4 * w + ni:4 * w + 4] == -1).all()   # spare rows: no override
    desc.instance_materials = True
    assert (mo.expand(desc) == -1).all()


def test_apply_clones_per_object_and_material_and_leaves_unbound_rows(oracle_mod):
    desc = mo.with_table(scenes.synthetic_scene(3, with_wall=True))
    desc.max_instances_per_world = 4
    fs = oracle_mod.FlatScene(desc)
    nm, nobj = len(fs.mat_tex), len(fs.obj_first_tri)
    rows = np.full(12, -1, np.int32)
    rows[[0, 4, 5, 3]] = [nm - 1, nm - 1, 2, 1]            # rows 0 and 4: the same object and material; row 3: spare
    out, back = mo.apply(fs, rows)
    assert len(out.obj_first_tri) == nobj + 2 and set(back.values()) == {int(fs.inst_obj0[0]), int(fs.inst_obj0[5])}
    assert out.inst_obj0[0] == out.inst_obj0[4] >= nobj and out.inst_obj0[3] == -1
    f, c = int(out.obj_first_tri[out.inst_obj0[5]]), int(out.obj_num_tris[out.inst_obj0[5]])
    assert c == int(fs.obj_num_tris[fs.inst_obj0[5]]) and (out.tri_mat[f:f + c] == 2).all()
    assert np.array_equal(fs.inst_obj0, oracle_mod.FlatScene(desc).inst_obj0)      # `fs` itself is not changed


def test_make_renderer_checks_the_ids_before_the_device(native):
    desc = scenes.synthetic_scene(4)
    for bad in (np.zeros(7, np.int32), np.zeros((8, 2), np.int32), np.zeros((2, 4), np.int32)):
        desc.instance_materials = bad
        with pytest.raises(ValueError):
            scenes.make_renderer(desc)
    if not has_gpu():
        for good in (True, mo.mixed(8, 2)):
            desc.instance_materials = good
            with pytest.raises(RuntimeError, match="no HIP device"):
                scenes.make_renderer(desc)


def test_headless_rejects_a_malformed_seed(native, tmp_path):
    from madrona_renderer_amd import build
    exe = build.headless_path()
    args = ["4", "1", "rast", "64", "64"]
    for bad in (["--instance-materials", "red"], ["--instance-materials", "-1"], ["--instance-materials", "1.5"],
                ["--instance-materials", ""], ["--instance-materials", "99999999999999999999999"],
                ["--instance-materials"]):
        p = subprocess.run(["timeout", "-k", "5", "60", exe] + args + bad, cwd=tmp_path, capture_output=True, text=True)
        assert p.returncode not in (0, 124, 137), bad
        assert "--instance-materials" in p.stderr, (bad, p.stderr)
