"""Output selection on the MI355X (-m gpu): a renderer created depth-only or rgb-only stores, in the
output it renders, exactly the bytes an RGBD renderer of the same scene and poses stores -- and
visibility ids / segmask as well -- and that output meets the oracle at the parity bar (RGBA8
equal, depth within 1 ulp and rtol 1e-4).  The output it does not render has no tensor."""
import ctypes
import dataclasses
import os

import numpy as np
import pytest

from madrona_renderer_amd import scenes
from tests import meshes as tmeshes
from tests.test_output_select_cpu import MRX_FLAG_NO_DEPTH, MRX_FLAG_NO_RGB, small_config
from tests.util import depth_ulps, render_oracle

pytestmark = pytest.mark.gpu

MRX_E_UNSUPPORTED = -5
MRX_BUF_RGB, MRX_BUF_DEPTH, MRX_BUF_SEGMASK, MRX_BUF_VISIBILITY = 0, 1, 2, 7


def _make(desc, outputs=None, visibility=False, variant=None, **kw):
    old = {k: os.environ.get(k) for k in ("MADRONA_MI355_VISIBILITY", "MADRONA_MI355_KERNEL")}
    os.environ["MADRONA_MI355_VISIBILITY"] = "1" if visibility else "0"
    if variant is not None:
        os.environ["MADRONA_MI355_KERNEL"] = str(variant)
    try:
        return scenes.make_renderer(desc, render_outputs=outputs, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _t(x):
    return x.to_torch()


def _same_bits(a, b):
    import torch
    assert a.shape == b.shape and a.dtype == b.dtype
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return bool(torch.equal(a, b))


def _compare(full, sel, outputs, visibility, raytracer, **shard):
    """The selected output and the ids of `sel` are the bytes `full` (RGBD) holds."""
    full.sync()
    sel.sync()
    if outputs == "Depth":
        assert _same_bits(_t(sel.depth_tensor(**shard)), _t(full.depth_tensor(**shard))), "depth bytes differ"
        with pytest.raises(RuntimeError, match="not rendered"):
            sel.rgb_tensor(**shard)
    else:
        assert _same_bits(_t(sel.rgb_tensor(**shard)), _t(full.rgb_tensor(**shard))), "rgb bytes differ"
        with pytest.raises(RuntimeError, match="not rendered"):
            sel.depth_tensor(**shard)
    if visibility:
        assert _same_bits(_t(sel.visibility_tensor(**shard)), _t(full.visibility_tensor(**shard)))
    elif raytracer:
        assert _same_bits(_t(sel.segmask_tensor(**shard)), _t(full.segmask_tensor(**shard)))


def _against_oracle(sel, desc, outputs, visibility, raytracer, views=None):
    ref = render_oracle(desc, view_end=views, want_ids=visibility or raytracer)
    n = views or desc.num_views
    if outputs == "Depth":
        d = _t(sel.depth_tensor())[:n].cpu().numpy().reshape(ref["depth"][:n].shape)
        np.testing.assert_allclose(d, ref["depth"][:n], rtol=1e-4, atol=0)
        ulps = depth_ulps(d, ref["depth"][:n])
        assert ulps <= 1, f"depth differs by {ulps} ulp"
    else:
        rgb = _t(sel.rgb_tensor())[:n].cpu().numpy()
        bad = int((rgb != ref["rgb"][:n]).any(axis=-1).sum())
        assert bad == 0, f"{bad} pixels differ in colour"
    if visibility:
        assert np.array_equal(_t(sel.visibility_tensor())[:n].cpu().numpy(), ref["tri_id"][:n])
    elif raytracer:
        assert np.array_equal(_t(sel.segmask_tensor())[:n].cpu().numpy(), ref["segmask"][:n])


def _check(desc, outputs, visibility=True, variant=None, oracle_views=None, path=None):
    raytracer = desc.render_mode == "Raytracer"
    full = _make(desc, None, visibility, variant)
    sel = _make(desc, outputs, visibility, variant)
    if path is not None:
        assert sel.render_path() == full.render_path() == path
    _compare(full, sel, outputs, visibility, raytracer)
    # a second render of the same poses stores the same bytes again
    sel.step()
    full.step()
    _compare(full, sel, outputs, visibility, raytracer)
    del full
    _against_oracle(sel, desc, outputs, visibility, raytracer, oracle_views)
    return sel


def _multi_camera_non_square():
    d = scenes.synthetic_scene(12, width=96, height=48, with_wall=True, textured=True)
    cams, worlds = [], []
    for i, ((eye, _), (ni, io, _, _)) in enumerate(zip(d.cameras, d.worlds)):
        eye2 = (-eye[1], eye[0], eye[2] + 2.0)
        cams += [d.cameras[i], (eye2, scenes.look_at(eye2, (0.0, 0.0, 0.5)))]
        worlds.append((ni, io, 2, 2 * i))
    return dataclasses.replace(d, cameras=cams, worlds=worlds)


SCENES = {
    "demo-rasterizer": lambda: scenes.demo_scene(num_worlds=4, render_mode="Rasterizer"),
    "demo-raytracer": lambda: scenes.demo_scene(num_worlds=4, render_mode="Raytracer"),
    "headline-64": lambda: scenes.synthetic_scene(64),
    "configs2-slice": lambda: scenes.synthetic_scene(256, width=128, height=128, with_wall=True),
    "bvh-40-cubes": lambda: tmeshes.cube_field(num_worlds=20, cubes=40),
    "bvh-40-cubes-textured": lambda: tmeshes.cube_field(num_worlds=20, cubes=40, textured=True),
    "multi-camera-96x48": _multi_camera_non_square,
}


@pytest.mark.parametrize("outputs", ["Depth", "RGB"])
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_selected_output_is_byte_identical_to_rgbd(native, scene, outputs):
    desc = SCENES[scene]()
    path = "bvh" if scene.startswith("bvh") else None
    _check(desc, outputs, visibility=True, path=path)
    if desc.render_mode == "Raytracer":
        _check(desc, outputs, visibility=False)        # the segmask instead of visibility ids


@pytest.mark.parametrize("outputs", ["Depth", "RGB"])
def test_headline_full_size(native, outputs):
    # 4096 worlds x 64x64 without visibility ids: the benchmarked kernel (FAST, XCD split)
    _check(scenes.synthetic_scene(4096), outputs, visibility=False, oracle_views=512)


@pytest.mark.parametrize("outputs", ["Depth", "RGB"])
@pytest.mark.parametrize("variant", [0, 3], ids=["default-dispatch-flat-kernel", "raster-kernels"])
def test_configs4_textured_raytracer(native, variant, outputs):
    desc = scenes.synthetic_scene(4096, width=256, height=256, textured=True, render_mode="Raytracer")
    _check(desc, outputs, visibility=False, variant=variant, oracle_views=48,
           path="raster" if variant else "bvh")


@pytest.mark.parametrize("outputs", ["Depth", "RGB"])
def test_configs4_slice_through_the_flat_kernel(native, outputs):
    # a slice of configs[4] on the BVH path (its flat kernel: worlds of <= 64 triangles), visibility ids too
    desc = scenes.synthetic_scene(96, width=256, height=256, textured=True, render_mode="Raytracer")
    _check(desc, outputs, visibility=True, variant=2, path="bvh")
    _check(desc, outputs, visibility=False, variant=2, path="bvh")


@pytest.mark.parametrize("flag", [MRX_FLAG_NO_RGB, MRX_FLAG_NO_DEPTH], ids=["depth-only", "rgb-only"])
@pytest.mark.parametrize("mode", ["Rasterizer", "Raytracer"])
def test_raw_c_abi(native, flag, mode):
    """Visibility ids (MRX_FLAG_VISIBILITY_IDS) with each setting through the C-ABI itself; the
    missing buffer is NULL / MRX_E_UNSUPPORTED and never allocated, the segmask stays."""
    lib = native.load_capi()
    lib.mrx_last_error.restype = ctypes.c_char_p
    lib.mrx_buffer.restype = ctypes.c_void_p
    lib.mrx_destroy.argtypes = [ctypes.c_void_p]
    desc = scenes.synthetic_scene(40, with_wall=True, textured=True, render_mode=mode)
    px = 40 * 64 * 64
    dims = (ctypes.c_int64 * 4)()
    nd, dt, dev = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()

    def create(flags):
        cfg, keep = small_config(desc, flags)
        h = ctypes.c_void_p()
        assert lib.mrx_create(ctypes.byref(cfg), ctypes.byref(h)) == 0, lib.mrx_last_error()
        assert lib.mrx_step(h) == 0 and lib.mrx_sync(h) == 0
        return h

    def read(h, which):
        out = np.empty(px, np.int32)
        assert lib.mrx_copy_to_host(h, which, out.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(out.nbytes)) == 0
        return out

    full, sel = create(1), create(1 | flag)
    try:
        missing, present = (MRX_BUF_RGB, MRX_BUF_DEPTH) if flag == MRX_FLAG_NO_RGB else (MRX_BUF_DEPTH, MRX_BUF_RGB)
        assert lib.mrx_buffer(sel, missing, dims, ctypes.byref(nd), ctypes.byref(dt), ctypes.byref(dev)) is None
        assert b"not rendered" in lib.mrx_last_error()
        host = np.empty(16, np.uint8)
        assert lib.mrx_copy_to_host(sel, missing, host.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(16)) == \
            MRX_E_UNSUPPORTED
        assert lib.mrx_buffer(sel, present, dims, ctypes.byref(nd), ctypes.byref(dt), ctypes.byref(dev))
        assert np.array_equal(read(sel, present), read(full, present))
        assert np.array_equal(read(sel, MRX_BUF_VISIBILITY), read(full, MRX_BUF_VISIBILITY))
        # bytes_per_step counts the tensors written: one 4-byte output fewer
        class Info(ctypes.Structure):
            _fields_ = [(n, ctypes.c_uint32) for n in ("nw", "nv", "ni", "no", "nt", "nm", "ntex", "mwt", "sf", "ss")] + \
                       [("dev", ctypes.c_int32), ("kv", ctypes.c_int32), ("bytes", ctypes.c_uint64),
                        ("rest", ctypes.c_uint8 * 256)]      # (mrx_info writes the whole ABI 2 struct)
        a, b = Info(), Info()
        assert lib.mrx_info(full, ctypes.byref(a)) == 0 and lib.mrx_info(sel, ctypes.byref(b)) == 0
        assert a.bytes - b.bytes == 4 * px
    finally:
        lib.mrx_destroy(full)
        lib.mrx_destroy(sel)
    if mode == "Raytracer":
        # without visibility ids the ids buffer holds the segmask, under every setting
        full, sel = create(0), create(flag)
        try:
            assert lib.mrx_buffer(sel, MRX_BUF_SEGMASK, dims, ctypes.byref(nd), ctypes.byref(dt), ctypes.byref(dev))
            assert np.array_equal(read(sel, MRX_BUF_SEGMASK), read(full, MRX_BUF_SEGMASK))
        finally:
            lib.mrx_destroy(full)
            lib.mrx_destroy(sel)


@pytest.mark.parametrize("outputs", ["Depth", "RGB"])
@pytest.mark.parametrize("mode", ["Rasterizer", "Raytracer"])
def test_pose_loop_with_a_hidden_instance(native, outputs, mode):
    desc = scenes.synthetic_scene(24, with_wall=True, textured=True, render_mode=mode)
    full = _make(desc, None, visibility=False)
    sel = _make(desc, outputs, visibility=False)
    for step in range(3):
        for r in (full, sel):
            pos = _t(r.instance_position_tensor())
            cpos = _t(r.camera_position_tensor())
            obj = _t(r.instance_object_tensor())
            pos[1::3, 2] += 0.4
            pos[2::3, 0] -= 0.3 * (step + 1)
            cpos[:, 2] += 0.5
            obj[4] = -1 if step < 2 else 0          # world 1's cube: hidden for two steps, then shown again
            r.step()
        _compare(full, sel, outputs, visibility=False, raytracer=mode == "Raytracer")


def test_several_shards_on_one_device_depth_only(native):
    desc = scenes.synthetic_scene(66, with_wall=True)
    one = _make(desc, "Depth")
    many = _make(desc, "Depth", device_ids=[0, 0, 0, 0])
    assert many.num_shards == 4
    one.sync()
    many.sync()
    whole = _t(one.depth_tensor())
    for i in range(4):
        lo, hi = many.shard_first_world(i), many.shard_first_world(i + 1)
        assert _same_bits(_t(many.depth_tensor(shard=i)), whole[lo:hi].contiguous()), i
        with pytest.raises(RuntimeError, match="not rendered"):
            many.rgb_tensor(shard=i)
