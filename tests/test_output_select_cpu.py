"""Output selection (MRX_FLAG_NO_RGB / MRX_FLAG_NO_DEPTH, Manager::RenderOutputs) on the host side:
argument checks that run before the device probe, the Python surface, and the compiled kernels
the setting adds (the compiler's resource report, committed as profiles/kernel_resources_latest.txt
and checked against HEAD by tests/test_kernel_resources.py).  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest

from madrona_renderer_amd import scenes
from tests.conftest import ROOT, has_gpu

MRX_FLAG_NO_RGB = 1 << 2
MRX_FLAG_NO_DEPTH = 1 << 3
MRX_E_INVALID, MRX_E_NO_DEVICE = -1, -2


class Geo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("vertices", "uvs", "indices", "mvo", "mio", "mm")] + \
               [(n, ctypes.c_uint32) for n in ("nv", "ni", "nm")]


class Cfg(ctypes.Structure):      # mrx_config up to kernel_variant (MRX_CONFIG_V2_SIZE)
    _fields_ = [("struct_size", ctypes.c_uint32), ("gpu_id", ctypes.c_int32),
                ("num_worlds", ctypes.c_uint32), ("render_mode", ctypes.c_int32),
                ("view_width", ctypes.c_uint32), ("view_height", ctypes.c_uint32),
                ("geo", Geo),
                ("asset_paths", ctypes.POINTER(ctypes.c_char_p)), ("num_asset_paths", ctypes.c_uint32),
                ("mat_assignments", ctypes.POINTER(ctypes.c_int32)), ("num_mat_assignments", ctypes.c_uint32),
                ("materials", ctypes.c_void_p), ("num_materials", ctypes.c_uint32),
                ("texture_paths", ctypes.POINTER(ctypes.c_char_p)), ("num_textures", ctypes.c_uint32),
                ("instances", ctypes.c_void_p), ("num_instances", ctypes.c_uint32),
                ("cameras", ctypes.c_void_p), ("num_cameras", ctypes.c_uint32),
                ("worlds", ctypes.c_void_p),
                ("stream", ctypes.c_void_p), ("flags", ctypes.c_uint32),
                ("kernel_variant", ctypes.c_int32)]


def small_config(desc, flags):
    """A valid mrx_config of `desc` (and the arrays it points into, which must stay alive)."""
    inst = np.zeros((len(desc.instances), 11), np.float32)
    for i, (p, q, s, o) in enumerate(desc.instances):
        inst[i, :3], inst[i, 3:7], inst[i, 7:10] = p, q, s
        inst[i, 10:11].view(np.int32)[0] = o
    cams = np.array([list(p) + list(q) for p, q in desc.cameras], np.float32)
    worlds = np.array(desc.worlds, np.uint32)
    mats = np.zeros((len(desc.materials), 7), np.float32)
    for i, (c, t, ro, me) in enumerate(desc.materials):
        mats[i, :4] = c
        mats[i, 4:5].view(np.int32)[0] = t
        mats[i, 5], mats[i, 6] = ro, me
    n = len(desc.asset_paths)
    paths = (ctypes.c_char_p * n)(*[p.encode() for p, _ in desc.asset_paths])
    assign = (ctypes.c_int32 * n)(*[i for _, i in desc.asset_paths])
    tex = (ctypes.c_char_p * 1)(desc.texture_paths[0].encode())
    cfg = Cfg()
    cfg.struct_size = ctypes.sizeof(Cfg)
    cfg.gpu_id, cfg.num_worlds = 0, desc.num_worlds
    cfg.render_mode = 1 if desc.render_mode == "Raytracer" else 0
    cfg.view_width, cfg.view_height = desc.width, desc.height
    cfg.asset_paths, cfg.num_asset_paths = paths, n
    cfg.mat_assignments, cfg.num_mat_assignments = assign, n
    cfg.materials, cfg.num_materials = mats.ctypes.data, len(mats)
    cfg.texture_paths, cfg.num_textures = tex, 1
    cfg.instances, cfg.num_instances = inst.ctypes.data, len(inst)
    cfg.cameras, cfg.num_cameras = cams.ctypes.data, len(cams)
    cfg.worlds = worlds.ctypes.data
    cfg.flags = flags
    return cfg, (inst, cams, worlds, mats, paths, assign, tex)


@pytest.mark.parametrize("mode", ["Rasterizer", "Raytracer"])
def test_both_outputs_off_is_rejected_before_the_device_probe(native, mode):
    lib = native.load_capi()
    lib.mrx_last_error.restype = ctypes.c_char_p
    cfg, keep = small_config(scenes.synthetic_scene(3, render_mode=mode), MRX_FLAG_NO_RGB | MRX_FLAG_NO_DEPTH)
    h = ctypes.c_void_p()
    assert lib.mrx_create(ctypes.byref(cfg), ctypes.byref(h)) == MRX_E_INVALID
    assert not h.value
    msg = lib.mrx_last_error().decode()
    assert "no output selected" in msg and "MRX_FLAG_NO_RGB" in msg and "MRX_FLAG_NO_DEPTH" in msg
    # (with visibility ids asked for as well: still no output to render)
    cfg.flags |= 1
    assert lib.mrx_create(ctypes.byref(cfg), ctypes.byref(h)) == MRX_E_INVALID


@pytest.mark.parametrize("flag", [MRX_FLAG_NO_RGB, MRX_FLAG_NO_DEPTH], ids=["depth-only", "rgb-only"])
def test_one_output_off_passes_the_argument_checks(native, flag):
    lib = native.load_capi()
    lib.mrx_last_error.restype = ctypes.c_char_p
    lib.mrx_destroy.argtypes = [ctypes.c_void_p]
    cfg, keep = small_config(scenes.synthetic_scene(3), flag)
    h = ctypes.c_void_p()
    rc = lib.mrx_create(ctypes.byref(cfg), ctypes.byref(h))
    if has_gpu():
        assert rc == 0, lib.mrx_last_error()
        lib.mrx_destroy(h)
    else:
        assert rc == MRX_E_NO_DEVICE, lib.mrx_last_error()


def test_module_exports_render_outputs(native):
    m = native.load_module()
    assert set(m.RenderOutputs.__members__) == {"RGBD", "Depth", "RGB"}
    assert m.RenderOutputs.RGBD != m.RenderOutputs.Depth != m.RenderOutputs.RGB


@pytest.mark.parametrize("outputs", ["Depth", "RGB"])
def test_make_renderer_passes_render_outputs_through(native, outputs):
    m = native.load_module()
    desc = scenes.demo_scene(num_worlds=2, render_mode="Rasterizer")
    for sel in (getattr(m.RenderOutputs, outputs), outputs):      # the member or its name
        if has_gpu():
            r = scenes.make_renderer(desc, render_outputs=sel)
            with pytest.raises(RuntimeError, match="not rendered"):
                (r.rgb_tensor if outputs == "Depth" else r.depth_tensor)()
        else:
            # past argument parsing (a wrong kwarg would raise TypeError) to the device probe
            with pytest.raises(RuntimeError, match="no HIP device"):
                scenes.make_renderer(desc, render_outputs=sel)
    with pytest.raises(AttributeError):
        scenes.make_renderer(desc, render_outputs="Colour")


def _table():
    """{source: {instantiation name: (VGPR, scratch, vgpr spill)}} of the committed resource table."""
    out, src = {}, None
    with open(os.path.join(ROOT, "profiles", "kernel_resources_latest.txt")) as f:
        for line in f:
            if line.startswith("##"):
                continue
            if line.startswith("# "):
                src = os.path.basename(line[2:].strip())
                out[src] = {}
                continue
            m = re.match(r"(.*?)\s+VGPR\s+(\d+)\s+SGPR\s+\d+\s+scratch\s+(\d+) B/lane\s+vgpr-spill\s+(\d+)", line)
            assert m, line
            out[src][m.group(1).split("(")[0]] = tuple(int(m.group(i)) for i in (2, 3, 4))
    return out


def test_resource_report_has_the_output_selection_instantiations():
    t = _table()
    fast = {k: v for k, v in t["raster.hip"].items() if k.startswith("rasterGroupKernelFast<")}
    flat = {k: v for k, v in t["bvh.hip"].items() if k.startswith("bvhFlatKernel<")}
    # rasterGroupKernelFast<IDS, TEX, XMODE, OUT>, bvhFlatKernel<IDS, TEX, OUT>; OUT 0 RGBD, 1 Depth, 2 RGB
    for out in (1, 2):
        for ids in ("true", "false"):
            for tex in ("true", "false"):
                for xmode in range(4):
                    assert f"rasterGroupKernelFast<{ids}, {tex}, {xmode}, {out}>" in fast
        for ids in range(3):
            for tex in ("true", "false"):
                assert f"bvhFlatKernel<{ids}, {tex}, {out}>" in flat
    for name, (vgpr, scratch, spill) in list(fast.items()) + list(flat.items()):
        assert scratch == 0 and spill == 0, name
    for name, (vgpr, _, _) in fast.items():
        assert vgpr <= 64, name
        if name.endswith(", 1>"):
            twin = name[:-len("1>")] + "0>"
            assert vgpr <= fast[twin][0], (name, vgpr, fast[twin][0])
    for name, (vgpr, _, _) in flat.items():
        assert vgpr <= 128, name
