"""Surface-normal output on the MI355X (-m gpu): normals=True through every kernel family against
tests/normal_oracle.py -- the float32 restatement scattered through the C oracle's tri_id image -- byte for byte, with
rgb, depth, ids and segmask still at parity with the oracle and byte-identical to a renderer of the same desc without
the flag, which also launches the same entry and BVH kernel; depth + normals and rgb + normals; normals beside mixed
projections, lights, colour and material overrides; poses, cameras, hidden and spare rows changed between steps; a
renderer without the flag; two shards; the headless binary.  Every compared view must show at least 2 distinct
normals among its covered pixels, a slice at least 3, and the image must differ from rgb: a kernel that wrote a
constant, or the colour, passes nothing here."""
import ctypes
import dataclasses
import subprocess

import numpy as np
import pytest

from madrona_renderer_amd import scenes
from tests import color_oracle as co
from tests import light_oracle as lo
from tests import material_oracle as mo
from tests import normal_oracle as no
from tests import projection_oracle as po
from tests.test_material_gpu import FLAT
from tests.test_projection_gpu import CASES, _make
from tests.util import assert_parity, fetch

pytestmark = pytest.mark.gpu

FAMILIES = dict(CASES, flat=FLAT)
FAMILIES["group-fast-48"] = (lambda: scenes.synthetic_scene(48), None, "group-fast", "none", False)
# views the CPU side compares: at most 64 per case
SLICE = {"flat": (0, 16)}


def _on(desc):
    d = dataclasses.replace(desc)
    d.normals = True
    return d


def _views(case, desc):
    a, b = SLICE.get(case, (0, min(64, desc.num_views)))
    return a, min(b, desc.num_views)


def _normals(r, views=None, shard=None):
    r.sync()
    t = r.normal_tensor() if shard is None else r.normal_tensor(shard=shard)
    t = t.to_torch()
    if views is not None:
        t = t[views[0]:views[1]]
    return t.cpu().numpy()


def _cut(images, views):
    a, b = views
    return {k: v[a:b] for k, v in images.items() if isinstance(v, np.ndarray)}


def _fetch_cut(r, rt, views):
    """The slice of every output but the normals, oracle layout (copied from the device slice by slice)."""
    r.sync()
    a, b = views
    out = {"rgb": r.rgb_tensor().to_torch()[a:b].cpu().numpy()}
    d = r.depth_tensor().to_torch()[a:b].cpu().numpy()
    out["depth"] = d.reshape(d.shape[0], d.shape[1], d.shape[2])
    if rt:
        out["segmask"] = r.segmask_tensor().to_torch()[a:b].cpu().numpy()
    else:
        out["tri_id"] = r.visibility_tensor().to_torch()[a:b].cpu().numpy()
    return out


def _assert_normals_decide(got, rgb, tri_id, per_view=True):
    """At least 2 distinct normals among the covered pixels of every view, at least 3 in the slice, not the colour.
    per_view=False (views under mixed projections: a narrow field of view or a far near plane leaves some of them a
    single triangle -- the ground -- or nothing at all in the oracle's image too): at least 2 in most views, and the
    slice's count."""
    packed = np.ascontiguousarray(got).view(np.uint32)[..., 0]
    whole, several = set(), 0
    for v in range(len(packed)):
        cov = tri_id[v] >= 0
        distinct = np.unique(packed[v][cov])
        if per_view:
            assert len(distinct) >= 2, (v, distinct)
        several += len(distinct) >= 2
        whole.update(distinct.tolist())
    assert 2 * several > len(packed)
    assert len(whole) >= 3
    if rgb is not None:
        assert (got != rgb).any()


def _same_bytes_on_device(a, b, rt, selected=("rgb", "depth", "ids")):
    import torch
    a.sync()
    b.sync()
    if "rgb" in selected:
        assert torch.equal(a.rgb_tensor().to_torch(), b.rgb_tensor().to_torch())
    if "depth" in selected:
        assert torch.equal(a.depth_tensor().to_torch().view(torch.int32), b.depth_tensor().to_torch().view(torch.int32))
    if "ids" in selected:
        if rt:
            assert torch.equal(a.segmask_tensor().to_torch(), b.segmask_tensor().to_torch())
        else:
            assert torch.equal(a.visibility_tensor().to_torch(), b.visibility_tensor().to_torch())


@pytest.mark.parametrize("case", list(FAMILIES))
def test_normals_match_the_oracle_in_every_family(native, oracle_mod, case):
    build, variant, entry, bvh, rt = FAMILIES[case]
    base = build()
    r = _make(_on(base), visibility=not rt, variant=variant)
    plain = _make(base, visibility=not rt, variant=variant)
    assert r.raster_entry() == entry and r.bvh_launch()["kernel"] == bvh
    assert plain.raster_entry() == entry and plain.bvh_launch()["kernel"] == bvh
    if case == "bvh-tile-pairs":
        assert r.bvh_launch()["group_views"] == plain.bvh_launch()["group_views"] == 2
    views = _views(case, base)
    ref = lo.render(base, None, None, views[0], views[1], want_ids=True)
    got = _normals(r, views)
    want = no.normals(oracle_mod.FlatScene(base), ref["tri_id"], views[0], views[1])
    assert got.shape == want.shape and got.dtype == np.uint8
    bad = int((got != want).any(axis=-1).sum())
    assert bad == 0, f"{bad} pixels differ in normals"
    others = _fetch_cut(r, rt, views)
    assert_parity(others, {k: ref[k][views[0]:views[1]] for k in others})
    _same_bytes_on_device(r, plain, rt)
    _assert_normals_decide(got, others["rgb"], ref["tri_id"][views[0]:views[1]])
    # the whole tensor: what the compared slice shows holds past it (background alpha 0, hits alpha 255)
    import torch
    t = r.normal_tensor().to_torch()
    assert tuple(t.shape) == tuple(r.rgb_tensor().to_torch().shape) and t.dtype == torch.uint8
    hit = (r.depth_tensor().to_torch().reshape(t.shape[:3]) != 0)
    assert bool((t[..., 3][hit] == 255).all()) and bool((t[~hit] == torch.tensor([128, 128, 128, 0], dtype=torch.uint8,
                                                                                 device=t.device)).all())


SELECT = {
    "group-fast": (lambda: scenes.synthetic_scene(1024), None, False),
    "group": (CASES["group"][0], CASES["group"][1], False),
    "bvh-tile": (CASES["bvh-tile"][0], CASES["bvh-tile"][1], False),
    "flat": (FLAT[0], FLAT[1], True),
}


@pytest.mark.parametrize("outputs", ["Depth", "RGB"])
@pytest.mark.parametrize("case", list(SELECT))
def test_normals_beside_one_selected_output(native, oracle_mod, case, outputs):
    build, variant, rt = SELECT[case]
    base = build()
    r = _make(_on(base), visibility=not rt, variant=variant, outputs=outputs)
    full = _make(base, visibility=not rt, variant=variant)
    assert r.raster_entry() == full.raster_entry() and r.bvh_launch()["kernel"] == full.bvh_launch()["kernel"]
    views = (0, 40) if case == "flat" else _views(case, base)
    ref = lo.render(base, None, None, views[0], views[1], want_ids=True)
    got = _normals(r, views)
    want = no.normals(oracle_mod.FlatScene(base), ref["tri_id"], views[0], views[1])
    assert int((got != want).any(axis=-1).sum()) == 0
    _assert_normals_decide(got, None, ref["tri_id"][views[0]:views[1]])
    _same_bytes_on_device(r, full, rt, ("depth", "ids") if outputs == "Depth" else ("rgb", "ids"))
    with pytest.raises(RuntimeError, match="not rendered"):
        (r.rgb_tensor if outputs == "Depth" else r.depth_tensor)()


@pytest.mark.parametrize("case", ["group-fast", "bvh-tile", "flat"])
def test_normals_do_not_depend_on_projection_light_colour_or_material(native, oracle_mod, case):
    build, variant, entry, bvh, rt = FAMILIES[case]
    base = mo.with_table(build())
    ni, nc = len(base.instances), len(base.cameras)
    ids = mo.mixed(ni, mo.num_materials(base))
    colors = co.mixed(ni)
    lights = lo.mixed(base.num_worlds)
    projs = po.mixed(nc, znears=(None, 0.5, 2.0, 999.0, 3.0)) if rt else po.mixed(nc)
    d = _on(base)
    d.instance_materials, d.instance_colors, d.world_lights, d.camera_projections = ids, colors, lights, list(projs)
    r = _make(d, visibility=not rt, variant=variant)
    assert r.raster_entry() == entry and r.bvh_launch()["kernel"] == bvh
    # (the composed oracle renders a group of views per light: a slice of 24 keeps the CPU side to a few seconds)
    views = (0, 16) if case == "flat" else (0, 24)
    ref = mo.render(base, ids, colors, lights, projs, view_begin=views[0], view_end=views[1], want_ids=True)
    got = _normals(r, views)
    want = no.normals(oracle_mod.FlatScene(base), ref["tri_id"], views[0], views[1])
    assert int((got != want).any(axis=-1).sum()) == 0
    others = _fetch_cut(r, rt, views)
    assert_parity(others, {k: ref[k][views[0]:views[1]] for k in others})
    _assert_normals_decide(got, others["rgb"], ref["tri_id"][views[0]:views[1]], per_view=False)
    # ... and are those of the same views without lights and overrides
    bare = _on(build())
    bare.camera_projections = list(projs)
    q = _make(bare, visibility=not rt, variant=variant)
    import torch
    r.sync()
    q.sync()
    assert torch.equal(r.normal_tensor().to_torch(), q.normal_tensor().to_torch())


@pytest.mark.parametrize("tables", [False, True], ids=["uniform", "tables"])
def test_normals_through_the_plain_entry_at_16_slots(native, oracle_mod, monkeypatch, tables):
    # both normals forms (over the uniform constants, over the tables) behind the plain entry of a 16-slot world (the
    # FAST entry switched off): two one-tile views
    monkeypatch.setenv("MRX_GROUP_FAST", "0")
    base = scenes.synthetic_scene(2)
    lights = lo.mixed(base.num_worlds) if tables else None
    projs = po.mixed(len(base.cameras)) if tables else None
    d = _on(base)
    if tables:
        d.world_lights, d.camera_projections = list(lights), list(projs)
    r = _make(d)
    assert r.raster_entry() == "group"
    views = (0, base.num_views)
    ref = lo.render(base, lights, projs, views[0], views[1], want_ids=True)
    want = no.normals(oracle_mod.FlatScene(base), ref["tri_id"], views[0], views[1])
    assert int((_normals(r, views) != want).any(axis=-1).sum()) == 0
    others = _fetch_cut(r, False, views)
    assert_parity(others, {k: ref[k][views[0]:views[1]] for k in others})


def test_textured_tile_kernel_with_per_strip_classification(native, oracle_mod, monkeypatch):
    """A textured world on the BVH tile kernel with the per-strip classification of large triangles on (as scenes with
    BLAS meshes have it).  Over the uniform constants the normals form classifies like the plain kernel; over per-view
    tables its classifying instantiation does not exist and the launch takes the plain one:
    `classify` reports False, every pixel is the same.  The textured record cap is smaller under the flag -- 52 bytes
    a record -- so that the workgroup keeps to half a CU's LDS."""
    from tests import meshes
    monkeypatch.setenv("MRX_BVH_CLASSIFY", "1")
    base = meshes.cube_field(num_worlds=24, cubes=40, textured=True)
    views = (0, 24)
    for projs, classify in ((None, True), (po.mixed(len(base.cameras)), False)):
        d = dataclasses.replace(base)
        d.camera_projections = None if projs is None else list(projs)
        r, plain = _make(_on(d)), _make(d)
        a, b = r.bvh_launch(), plain.bvh_launch()
        assert a["kernel"] == b["kernel"] == "tile" and a["textured"] and b["textured"] and a["tile"] == b["tile"] == (64, 64)
        assert b["classify"] is True and a["classify"] is classify
        assert a["group_views"] == b["group_views"] and a["workgroups"] == b["workgroups"]
        # 48 bytes a record without the flag, 52 with: the cap shrinks by about a thirteenth, in steps of 32
        assert 0 < b["tex_cap"] - a["tex_cap"] <= b["tex_cap"] // 13 + 32 and a["tex_cap"] % 32 == 0
        ref = lo.render(base, None, projs, views[0], views[1], want_ids=True)
        got = _normals(r, views)
        want = no.normals(oracle_mod.FlatScene(base), ref["tri_id"], views[0], views[1])
        assert int((got != want).any(axis=-1).sum()) == 0
        others = _fetch_cut(r, False, views)
        assert_parity(others, {k: ref[k][views[0]:views[1]] for k in others})
        _same_bytes_on_device(r, plain, False)
        _assert_normals_decide(got, others["rgb"], ref["tri_id"][views[0]:views[1]], per_view=projs is None)


def test_normals_follow_poses_cameras_hidden_and_spare_rows(native, oracle_mod):
    import torch
    base = scenes.synthetic_scene(64, with_wall=True)
    base.max_instances_per_world = 4                      # three rows bound, one spare
    r = _make(_on(base))
    fs = oracle_mod.FlatScene(base)
    V = base.num_views

    def check():
        ref = fs.render(want_ids=True)
        got = _normals(r)
        want = no.normals(fs, ref["tri_id"])
        assert int((got != want).any(axis=-1).sum()) == 0
        assert_parity(fetch(r), ref)
        return ref, got

    first, img0 = check()
    # new rotations of the cubes and new camera poses, written from torch
    rng = np.random.default_rng(3)
    rot = r.instance_rotation_tensor().to_torch()
    cubes = list(range(1, 4 * V, 4))
    ang = rng.uniform(0, 2 * np.pi, len(cubes))
    axis = rng.standard_normal((len(cubes), 3))
    axis /= np.linalg.norm(axis, axis=1)[:, None]
    q = np.concatenate([np.cos(ang / 2)[:, None], np.sin(ang / 2)[:, None] * axis], axis=1).astype(np.float32)
    rot[cubes] = torch.from_numpy(q).to(rot.device)
    fs.inst_rot[cubes] = q
    cam = r.camera_position_tensor().to_torch()
    shift = rng.uniform(-0.5, 0.5, (V, 3)).astype(np.float32)
    cam += torch.from_numpy(shift).to(cam.device)
    fs.cam_pos += shift
    r.step()
    moved, img1 = check()
    assert (img1 != img0).any()
    # a hidden row: what is behind it shows, or the background
    obj = r.instance_object_tensor().to_torch()
    hidden = cubes[::2]
    obj[hidden] = -1
    fs.inst_obj[hidden] = -1
    r.step()
    ref, img2 = check()
    gone = (moved["tri_id"] >= 2) & (moved["tri_id"] < 14) & (np.arange(V) % 2 == 0)[:, None, None]
    assert gone.any() and ((ref["tri_id"][gone] < 2) | (ref["tri_id"][gone] >= 14)).all()
    bg = ref["tri_id"][gone] < 0
    assert (img2[gone][bg] == np.array([128, 128, 128, 0], np.uint8)).all()
    # a spare row bound through refresh_objects(): a cube of its own
    spare = list(range(3, 4 * V, 4))
    pos = r.instance_position_tensor().to_torch()
    obj[spare] = 0
    pos[spare] = torch.tensor([1.5, -2.0, 2.0], device=pos.device)
    r.refresh_objects()
    r.step()
    fs.inst_obj[spare] = 0
    fs.inst_pos[spare] = (1.5, -2.0, 2.0)
    fs.refresh_objects()
    ref, img3 = check()
    new = ref["tri_id"] >= int(fs.obj_num_tris[[1, 0, 2]].sum())
    assert new.any() and (img3[new][:, 3] == 255).all()


def test_off_means_off(native):
    base = scenes.synthetic_scene(256)
    off = _make(base)
    with pytest.raises(RuntimeError, match="MRX_FLAG_NORMALS"):
        off.normal_tensor()
    lib = native.load_capi()
    lib.mrx_buffer.restype = ctypes.c_void_p
    lib.mrx_buffer.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int),
                               ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    lib.mrx_last_error.restype = ctypes.c_char_p
    dims = (ctypes.c_int64 * 4)()
    nd, dt, dev = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    handle = ctypes.c_void_p(off.native_handle())
    assert lib.mrx_buffer(handle, 12, dims, ctypes.byref(nd), ctypes.byref(dt), ctypes.byref(dev)) is None
    assert b"MRX_FLAG_NORMALS" in lib.mrx_last_error()
    host = (ctypes.c_uint8 * 16)()
    lib.mrx_copy_to_host.restype = ctypes.c_int
    lib.mrx_copy_to_host.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64]
    assert lib.mrx_copy_to_host(handle, 12, host, 16) == -5          # MRX_E_UNSUPPORTED
    # the flag costs a launch form, not a kernel family or a launch shape, and no other output a byte
    for build, variant, rt in ((lambda: scenes.synthetic_scene(256), None, False),
                               (lambda: scenes.synthetic_scene(64, width=128, height=128, render_mode="Raytracer"), None, True)):
        d = build()
        a, b = _make(d, visibility=not rt, variant=variant), _make(_on(d), visibility=not rt, variant=variant)
        assert a.raster_entry() == b.raster_entry() and a.bvh_launch() == b.bvh_launch()
        _same_bytes_on_device(a, b, rt)
        assert_parity(fetch(a, visibility=not rt, raytracer=rt),
                      {k: v for k, v in lo.render(d, want_ids=True).items() if isinstance(v, np.ndarray)})


def test_two_shards_hold_their_own_views(native, oracle_mod):
    base = scenes.synthetic_scene(301)
    one = _make(_on(base))
    r = _make(_on(base), device_ids=[0, 0])
    assert r.num_shards == 2
    whole = _normals(one)
    ref = lo.render(base, want_ids=True)
    want = no.normals(oracle_mod.FlatScene(base), ref["tri_id"])
    assert np.array_equal(whole, want)
    parts = []
    for sh in range(2):
        a, b = r.shard_first_world(sh), r.shard_first_world(sh + 1)
        part = _normals(r, shard=sh)
        assert part.shape[0] == b - a
        parts.append(part)
    assert np.array_equal(np.concatenate(parts), whole)


def test_headless_normals(native, oracle_mod, tmp_path):
    from madrona_renderer_amd import build
    from tests.test_headless_gpu import _tiles
    exe = build.headless_path()
    p = subprocess.run(["timeout", "-k", "5", "120", exe, "16", "2", "rast", "64", "64", "--normals", "--dump-last-frame",
                        "frame"], cwd=tmp_path, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    desc = scenes.synthetic_scene(16)
    ref = po.render(desc, want_ids=True)
    assert np.array_equal(np.stack(_tiles(tmp_path / "frame.png", 16, 64, 64)), ref["rgb"])
    got = np.stack(_tiles(tmp_path / "frame.normals.png", 16, 64, 64))
    assert np.array_equal(got, no.normals(oracle_mod.FlatScene(desc), ref["tri_id"]))
