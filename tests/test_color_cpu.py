"""Per-instance colour override on the host (no GPU): the helper the GPU tests compare against
(tests/color_oracle.py) is anchored -- with every alpha zero it is the plain oracle byte for byte, with colours set
only RGB changes, and a scene authored with the colours as materials gives the same images -- SceneDesc and its
shards carry the colours with the rows, the C ABI's new names and struct sizes are there, and the headless binary
refuses a malformed --instance-colors."""
import ctypes
import subprocess

import numpy as np
import pytest

from madrona_renderer_amd import scenes
from tests import color_oracle as co
from tests import light_oracle as lo
from tests import projection_oracle as po
from tests.conftest import has_gpu
from tests.test_light_cpu import V2_SIZE
from tests.test_light_cpu import Cfg as CfgLight
from tests.test_output_select_cpu import small_config

MRX_E_INVALID, MRX_E_NO_DEVICE, MRX_E_UNSUPPORTED = -1, -2, -3

SCENES = {
    "raster-wall": lambda: scenes.synthetic_scene(8, with_wall=True),
    "raytracer-textured": lambda: scenes.synthetic_scene(8, textured=True, render_mode="Raytracer"),
    "cube-field-textured": lambda: scenes.cube_field(4, 20, textured=True),
    "demo-aliased": lambda: scenes.demo_scene(3),
}


@pytest.mark.parametrize("name", list(SCENES))
def test_alpha_zero_is_the_plain_oracle_byte_for_byte(oracle_mod, name):
    desc = SCENES[name]()
    plain = oracle_mod.FlatScene(desc).render()
    colors = np.random.default_rng(1).integers(0, 256, (len(desc.instances), 4), dtype=np.uint8)
    colors[:, 3] = 0
    for got in (co.render(desc, colors), co.render(desc), co.render_flat(oracle_mod.FlatScene(desc), co.expand(desc, colors))):
        for k in ("rgb", "depth", "tri_id", "segmask"):
            assert np.array_equal(got[k].view(np.uint8), plain[k].view(np.uint8)), k


@pytest.mark.parametrize("name", list(SCENES))
def test_colours_change_rgb_and_nothing_else(oracle_mod, name):
    desc = SCENES[name]()
    plain = oracle_mod.FlatScene(desc).render()
    colors = co.mixed(len(desc.instances))
    if name == "demo-aliased":
        colors[:, 3] = 255                                # (two rows: both overridden)
    got = co.render(desc, colors)
    for k in ("depth", "tri_id", "segmask"):
        assert np.array_equal(got[k].view(np.uint8), plain[k].view(np.uint8)), k
    covered = plain["tri_id"] >= 0
    assert np.array_equal(got["rgb"][~covered], plain["rgb"][~covered])
    assert (got["rgb"][..., 3] == 255).all()
    # rows 1::4 are left alone: what only they cover keeps its colour
    rows = co.expand(desc, colors)
    fs = oracle_mod.FlatScene(desc)
    for v in range(fs.num_views):
        w = int(fs.view_world[v])
        k = 0
        for i in range(fs.world_inst_start[w], fs.world_inst_start[w + 1]):
            n = int(fs.obj_num_tris[fs.inst_obj0[i]])
            mine = (plain["tri_id"][v] >= k) & (plain["tri_id"][v] < k + n)
            if rows[i, 3] == 0:
                assert np.array_equal(got["rgb"][v][mine], plain["rgb"][v][mine])
            k += n
    assert co.changed_fraction(got, plain) >= 0.5


def _cube():
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    idx = np.array([t for a, b, c, d in quads for t in (a, b, c, a, c, d)], np.uint32)
    return v, np.zeros((8, 2), np.float32), idx


def _authored(num_objects, mats, objs):
    from tests import meshes
    v, t, i = _cube()
    geo = meshes.pack_meshes([(v, t, i, m) for m in range(num_objects)])
    inst = [((-3.0, 0.0, 1.0), (1.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0), objs[0]),
            ((0.0, 0.5, 1.5), (0.9238795, 0.0, 0.0, 0.3826834), (1.0, 1.5, 0.5), objs[1]),
            ((3.0, -0.5, 1.0), (0.9659258, 0.2588190, 0.0, 0.0), (0.7, 0.7, 0.7), objs[2])]
    eye = (1.0, -6.5, 3.0)
    return scenes.SceneDesc(num_worlds=2, width=96, height=64, materials=mats, instances=inst,
                            cameras=[(eye, scenes.look_at(eye, (0.0, 0.0, 1.0)))], worlds=[(3, 0, 1, 0)] * 2, **geo)


@pytest.mark.parametrize("mode", ["Rasterizer", "Raytracer"])
def test_an_override_is_the_same_scene_authored_with_that_material(oracle_mod, mode):
    cs = np.array([[255, 0, 0, 255], [13, 200, 77, 1], [90, 90, 255, 128]], np.uint8)
    a = _authored(1, [((1.0, 1.0, 1.0, 1.0), -1, 0.5, 0.5)], [0, 0, 0])
    a.instance_colors = cs
    b = _authored(3, [(tuple(float(np.float32(x) * co.K255) for x in c[:3]) + (1.0,), -1, 0.5, 0.5) for c in cs], [0, 1, 2])
    a.render_mode = b.render_mode = mode
    ra, rb = co.render(a), oracle_mod.FlatScene(b).render()
    for k in ("rgb", "depth", "tri_id"):
        assert np.array_equal(ra[k].view(np.uint8), rb[k].view(np.uint8)), k
    assert (ra["tri_id"] >= 0).mean() > 0.05 and len(np.unique(ra["rgb"].reshape(-1, 4), axis=0)) > 6
    assert set(np.unique(ra["segmask"])) == {-1, 0} and set(np.unique(rb["segmask"])) == {-1, 0, 1, 2}


def test_the_helper_composes_with_lights_and_projections(oracle_mod):
    desc = scenes.synthetic_scene(6, with_wall=True)
    colors = co.mixed(len(desc.instances))
    lights, projs = lo.mixed(6, shift=1), po.mixed(6)
    got = co.render(desc, colors, lights, projs)
    plain = lo.render(desc, lights, projs)
    assert oracle_mod.FlatScene.__name__ == "FlatScene"   # (the helper's hook is gone again)
    for k in ("depth", "tri_id", "segmask"):
        assert np.array_equal(got[k].view(np.uint8), plain[k].view(np.uint8)), k
    assert co.changed_fraction(got, plain) >= 0.5
    none = co.render(desc, np.zeros((len(desc.instances), 4), np.uint8), lights, projs)
    assert np.array_equal(none["rgb"], plain["rgb"])


def test_scene_desc_and_its_shards_carry_the_colours_with_the_rows():
    assert scenes.synthetic_scene(2).instance_colors is None
    for desc in (scenes.synthetic_scene(7, with_wall=True), scenes.demo_scene(5)):
        desc.instance_colors = co.mixed(len(desc.instances))
        desc.max_instances_per_world = 4
        whole = co.expand(desc)
        assert whole.shape == (4 * desc.num_worlds, 4)
        parts = [co.expand(desc.shard(r, 3)) for r in range(3)]
        assert np.array_equal(np.concatenate(parts), whole)
        for w, (ni, io, _, _) in enumerate(desc.worlds):   # worlds that alias rows share their colours
            assert np.array_equal(whole[4 * w:4 * w + ni], desc.instance_colors[io:io + ni])
            assert not whole[4 * w + ni:4 * w + 4].any()   # spare rows: no override


def test_make_renderer_checks_the_colours_before_the_device(native):
    desc = scenes.synthetic_scene(4)
    for bad in (np.zeros((7, 4), np.uint8), np.zeros((8, 3), np.uint8), np.zeros(32, np.uint8)):
        desc.instance_colors = bad
        with pytest.raises(ValueError):
            scenes.make_renderer(desc)
    m = native.load_module()
    with pytest.raises(ValueError, match="instance_colors"):
        _module_renderer(m, desc, np.zeros((8, 2), np.uint8))
    if not has_gpu():
        for good in (True, co.mixed(8)):
            desc.instance_colors = good
            with pytest.raises(RuntimeError, match="no HIP device"):
                scenes.make_renderer(desc)


def _module_renderer(m, desc, colors):
    return m.MadronaRenderer(
        gpu_id=0, num_worlds=desc.num_worlds, render_mode=m.RenderMode.Rasterizer, batch_render_view_width=64,
        batch_render_view_height=64, asset_paths=[m.ImportedAsset(path=p, mat_id=i) for p, i in desc.asset_paths],
        mesh_vertices=desc.mesh_vertices, mesh_uvs=desc.mesh_uvs, mesh_indices=desc.mesh_indices,
        mesh_vertex_offsets=desc.mesh_vertex_offsets, mesh_indices_offsets=desc.mesh_indices_offsets,
        mesh_materials=desc.mesh_materials,
        materials=[m.AdditionalMaterial(color=list(c), texture_id=t, roughness=r, metalness=me) for c, t, r, me in desc.materials],
        texture_paths=list(desc.texture_paths),
        instances=[m.ImportedInstance(position=list(p), rotation=list(q), scale=list(s), object_id=o)
                   for p, q, s, o in desc.instances],
        cameras=[m.ImportedCamera(position=list(p), rotation=list(q)) for p, q in desc.cameras],
        worlds=[m.WorldInit(num_instances=a, instance_offset=b, num_cameras=c, camera_offset=d) for a, b, c, d in desc.worlds],
        instance_colors=colors)


class Cfg(ctypes.Structure):      # the whole mrx_config: the struct as it was with world_lights, instance_colors, reserved0
    _fields_ = [("prev", CfgLight), ("instance_colors", ctypes.POINTER(ctypes.c_uint8)), ("reserved0", ctypes.c_uint64)]


def _create(lib, desc, size, colors=None, flags=0, reserved=0):
    v2, keep = small_config(desc, flags)
    cfg = Cfg()
    cfg.prev.prev.v2 = v2
    cfg.prev.prev.v2.struct_size = size
    if colors is not None:
        arr = np.ascontiguousarray(colors, np.uint8)
        cfg.instance_colors = arr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        keep = keep + (arr,)
    cfg.reserved0 = reserved
    h = ctypes.c_void_p()
    rc = lib.mrx_create(ctypes.byref(cfg), ctypes.byref(h))
    if h.value:
        lib.mrx_destroy.argtypes = [ctypes.c_void_p]
        lib.mrx_destroy(h)
    return rc


def test_the_new_abi_names_and_struct_sizes(native):
    """The names are there with the issue's values; the accepted struct sizes are an exact set -- V2, V4, the struct
    as it was with camera_projections, as it was with world_lights (MRX_CONFIG_V4_LIGHT_SIZE) and the current one --
    and on a machine without a GPU mrx_create then fails on the device probe, after every argument check."""
    m = native.load_module()
    assert m.MRX_FLAG_INSTANCE_COLORS == 1 << 4
    assert m.MRX_BUF_INSTANCE_COLOR == 10 and m.MRX_NUM_BUFFERS == 11
    light_size = ctypes.sizeof(CfgLight)
    assert m.MRX_CONFIG_V4_LIGHT_SIZE == light_size == Cfg.instance_colors.offset
    assert m.MRX_CONFIG_SIZE == ctypes.sizeof(Cfg) == light_size + 16
    lib = native.load_capi()
    lib.mrx_abi_version.restype = ctypes.c_int
    assert lib.mrx_abi_version() == 4
    desc = scenes.synthetic_scene(3, textured=True)
    ok = 0 if has_gpu() else MRX_E_NO_DEVICE
    v4 = light_size - 16
    accepted = (V2_SIZE, v4, v4 + 8, light_size, ctypes.sizeof(Cfg))
    for size in accepted:
        assert _create(lib, desc, size) == ok, size
    for size in range(v4 - 8, ctypes.sizeof(Cfg) + 12, 4):
        if size not in accepted:
            assert _create(lib, desc, size) == MRX_E_INVALID, size
    colors = co.mixed(len(desc.instances))
    assert _create(lib, desc, ctypes.sizeof(Cfg), colors) == ok
    assert _create(lib, desc, ctypes.sizeof(Cfg), None, flags=1 << 4) == ok
    assert _create(lib, desc, ctypes.sizeof(Cfg), colors, reserved=1) == MRX_E_INVALID
    # (a caller of an older size passes no colours: the field is not read)
    assert _create(lib, desc, light_size, colors, reserved=1) == ok


def test_headless_rejects_a_malformed_seed(native, tmp_path):
    from madrona_renderer_amd import build
    exe = build.headless_path()
    args = ["4", "1", "rast", "64", "64"]
    for bad in (["--instance-colors", "red"], ["--instance-colors", "-1"], ["--instance-colors", "1.5"],
                ["--instance-colors", ""], ["--instance-colors", "99999999999999999999999"], ["--instance-colors"]):
        p = subprocess.run(["timeout", "-k", "5", "60", exe] + args + bad, cwd=tmp_path, capture_output=True, text=True)
        assert p.returncode not in (0, 124, 137), bad
        assert "--instance-colors" in p.stderr, (bad, p.stderr)
