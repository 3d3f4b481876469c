"""Surface-normal output on the host (no GPU): the helper the GPU tests compare against
(tests/normal_oracle.py) is anchored -- its fused multiply-add is glibc's fmaf bit for bit, its n, len and sign rule
reproduce the C oracle's S7 colour bytes on every covered pixel under every light of the cycle, its decoded normals
are the float64 unit normals of the transformed triangles turned towards the eye to half a quantisation step, and
face every primary ray -- the background and the byte range are S10's, the C ABI's new names are there beside the
unchanged old ones, SceneDesc and its shards carry the flag, make_renderer passes it on and the headless binary
knows --normals."""
import ctypes
import ctypes.util
import dataclasses
import subprocess

import numpy as np
import pytest

from madrona_renderer_amd import scenes
from tests import light_oracle as lo
from tests import meshes
from tests import normal_oracle as no
from tests.conftest import has_gpu
from tests.test_color_cpu import Cfg, _create

MRX_E_INVALID, MRX_E_NO_DEVICE = -1, -2
F32 = np.float32


def _white(desc):
    """`desc` untextured with every material white."""
    d = dataclasses.replace(desc)
    d.materials = [((1.0, 1.0, 1.0, 1.0), -1, r, m) for _, _, r, m in desc.materials]
    return d


SCENES = {
    "raster-wall": lambda: scenes.synthetic_scene(8, with_wall=True),
    "raytracer-128": lambda: scenes.synthetic_scene(8, width=128, height=128, render_mode="Raytracer"),
    "cube-field": lambda: meshes.cube_field(4, 40),
    "demo-aliased": lambda: scenes.demo_scene(3),
}


def _scaled():
    """Worlds with a mirrored (negative-scale) and a non-uniformly scaled instance."""
    d = scenes.synthetic_scene(8, with_wall=True)
    inst = list(d.instances)
    for w, (ni, io, _, _) in enumerate(d.worlds):
        p, q, s, o = inst[io + 1]
        inst[io + 1] = (p, q, (-s[0], s[1], s[2]) if w % 2 == 0 else (0.5 * s[0], 2.0 * s[1], 1.25 * s[2]), o)
        p, q, s, o = inst[io + 2]
        inst[io + 2] = (p, q, (1.0, -1.5, 0.75) if w % 3 == 0 else (2.0, 1.0, -0.5), o)
    d.instances = inst
    return d


GEOMETRY = dict(SCENES, scaled=_scaled)


def test_the_fma_helper_is_fmaf_bit_for_bit():
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    rng = np.random.default_rng(12)
    n = 6000
    a = (rng.standard_normal(4 * n) * np.exp2(rng.integers(-20, 20, 4 * n))).astype(F32)
    b = (rng.standard_normal(4 * n) * np.exp2(rng.integers(-20, 20, 4 * n))).astype(F32)
    c = (rng.standard_normal(4 * n) * np.exp2(rng.integers(-40, 40, 4 * n))).astype(F32)
    # heavy cancellation: c is the rounded product negated, exactly or a few ulps off
    c[n:2 * n] = -(a[n:2 * n] * b[n:2 * n])
    c[2 * n:3 * n] = np.nextafter(-(a[2 * n:3 * n] * b[2 * n:3 * n]), F32(rng.choice([-np.inf, np.inf])))
    # midpoints: (1 + m 2^-12)^2 lies exactly between two floats for odd m; c = 0 or far below the last bit (a float64
    # sum would lose it and land on the tie)
    m = rng.integers(1, 4096, n) | 1
    a[3 * n:] = b[3 * n:] = (1.0 + m * 2.0 ** -12).astype(F32)
    c[3 * n:] = rng.choice(np.array([0.0, 2.0 ** -60, -2.0 ** -60, 2.0 ** -100, -2.0 ** -100, 2.0 ** -30], F32), n)
    assert len(a) >= 20000
    got = no.fma32(a, b, c)
    want = np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], F32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # (the constructed ties are ties: the float64 product has exactly one bit below the float32 grid)
    p = a[3 * n:].astype(np.float64) * b[3 * n:].astype(np.float64)
    assert (np.abs(p - p.astype(F32).astype(np.float64)) == 2.0 ** -24).all()


@pytest.mark.parametrize("name", list(SCENES))
def test_the_restated_s7_byte_is_the_oracles_rgb_on_every_covered_pixel(oracle_mod, name):
    """Pins n, len and the sign rule S10 reuses: white untextured materials, every light of the cycle."""
    desc = _white(SCENES[name]())
    fs = oracle_mod.FlatScene(desc)
    covered = 0
    for light in lo.CYCLE:
        ref = lo.render(desc, [light] * desc.num_worlds, want_ids=True)
        d, a, f = lo._key(light)
        saved = oracle_mod.LIGHT_DIR
        try:
            oracle_mod.LIGHT_DIR = d
            tl = oracle_mod.to_light_vector()
        finally:
            oracle_mod.LIGHT_DIR = saved
        for v in range(fs.num_views):
            tid = ref["tri_id"][v]
            hit = tid >= 0
            assert hit.any()
            table = no.lit_table(fs, v, tl, F32(a), F32(f))
            want = ref["rgb"][v][hit]
            got = table[tid[hit]]
            assert (want[:, 3] == 255).all()
            bad = int((want[:, :3] != got[:, None]).any(axis=-1).sum())
            assert bad == 0, (name, light, v, bad)
            covered += int(hit.sum())
    print("covered pixels compared", name, covered)


def _float64_normals(fs, v):
    """Unit normals, turned towards the eye, of the transformed triangles of view v, in float64 from the float32 inputs."""
    _, _, _, _, _ = no.view_geometry(fs, v)        # (slot numbering is shared: recomputed below in float64)
    w = int(fs.view_world[v])

    def rot(q):
        q = np.asarray(q, np.float64)
        ww, x, y, z = q
        return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - ww * z), 2 * (x * z + ww * y)],
                         [2 * (x * y + ww * z), 1 - 2 * (x * x + z * z), 2 * (y * z - ww * x)],
                         [2 * (x * z - ww * y), 2 * (y * z + ww * x), 1 - 2 * (x * x + y * y)]])
    Rc = rot(fs.cam_rot[v])
    c = np.asarray(fs.cam_pos[v], np.float64)
    out = []
    for i in range(int(fs.world_inst_start[w]), int(fs.world_inst_start[w + 1])):
        obj = int(fs.inst_obj0[i])
        if obj < 0 or obj >= len(fs.obj_first_tri):
            continue
        first, cnt = int(fs.obj_first_tri[obj]), int(fs.obj_num_tris[obj])
        M = rot(fs.inst_rot[i]) * np.asarray(fs.inst_scale[i], np.float64)[None, :]
        op = np.asarray(fs.tri_pos, np.float64).reshape(-1, 3, 3)[first:first + cnt]
        P = ((op @ M.T) + np.asarray(fs.inst_pos[i], np.float64) - c) @ Rc      # rows: Rc^T (M p + t - c)
        n = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
        n /= np.linalg.norm(n, axis=1)[:, None]
        n[np.einsum("ij,ij->i", n, P[:, 0]) > 0] *= -1.0
        out.append(n)
    return np.concatenate(out)


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_decoded_normals_against_float64_geometry_and_the_primary_rays(oracle_mod, name):
    desc = GEOMETRY[name]()
    fs = oracle_mod.FlatScene(desc)
    ref = fs.render(want_ids=True)
    sx, ox, sz, oz = (float(x) for x in oracle_mod.projection_constants(fs.width, fs.height, fs.raytracer))
    nslow, nfast = ref["tri_id"].shape[1:]
    slow, fast = np.meshgrid(np.arange(nslow), np.arange(nfast), indexing="ij")
    ix, iy = (slow, fast) if fs.raytracer else (fast, slow)      # Raytracer storage is [x][y]
    rx, rz = sx * ix + ox, sz * iy + oz
    worst = 0.0
    for v in range(fs.num_views):
        tid = ref["tri_id"][v]
        hit = tid >= 0
        assert hit.any()
        dec = no.decode(no.view_table(fs, v))
        n64 = _float64_normals(fs, v)
        seen = np.unique(tid[hit])
        err = np.abs(dec[seen] - n64[seen]).max()
        worst = max(worst, float(err))
        assert err <= 0.004, (name, v, err)
        img = no.decode(no.scatter(no.view_table(fs, v), tid))
        facing = img[..., 0] * rx + img[..., 1] + img[..., 2] * rz
        assert (facing[hit] <= 0.004 * (np.abs(rx) + 1.0 + np.abs(rz))[hit]).all(), (name, v)
    print("largest component error", name, worst)


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_background_alpha_and_byte_range(oracle_mod, name):
    desc = GEOMETRY[name]()
    fs = oracle_mod.FlatScene(desc)
    ref = fs.render(want_ids=True)
    img = no.normals(fs, ref["tri_id"])
    hit = ref["tri_id"] >= 0
    assert hit.any() and (~hit).any()
    assert (img[~hit] == np.array([128, 128, 128, 0], np.uint8)).all()
    assert (img[hit][:, 3] == 255).all()
    assert img[hit][:, :3].min() >= 1
    assert (no.decode(img[~hit]) == 0.0).all()
    # unit length to the quantisation: |decoded| within sqrt(3) half steps of 1
    ln = np.linalg.norm(no.decode(img[hit]), axis=-1)
    assert np.abs(ln - 1.0).max() <= np.sqrt(3.0) * 0.5 / 127.0 + 1e-6


def test_hidden_and_unbound_rows_keep_the_slot_numbering(oracle_mod):
    desc = scenes.synthetic_scene(4, with_wall=True)
    desc.max_instances_per_world = 5                     # two spare, unbound rows per world
    fs = oracle_mod.FlatScene(desc)
    fs.inst_obj[1::5] = -1                               # the cube of every world hidden
    ref = fs.render(want_ids=True)
    full = oracle_mod.FlatScene(desc).render(want_ids=True)
    assert (ref["tri_id"] != full["tri_id"]).any()
    img = no.normals(fs, ref["tri_id"])
    for v in range(fs.num_views):
        table = no.view_table(fs, v)
        assert len(table) == 2 + 12 + int(fs.obj_num_tris[2])      # plane, (hidden) cube, wall: spare rows have no slots
        hit = ref["tri_id"][v] >= 0
        assert np.array_equal(img[v][hit], table[ref["tri_id"][v][hit]])


def test_the_new_abi_names_beside_the_unchanged_old_ones(native):
    m = native.load_module()
    assert m.MRX_FLAG_NORMALS == 1 << 6
    assert m.MRX_BUF_NORMAL == 12 and m.MRX_NUM_BUFFERS_EXT2 == 13
    assert m.MRX_NUM_BUFFERS == 11 and m.MRX_NUM_BUFFERS_EXT == 12
    assert m.MRX_CONFIG_SIZE == ctypes.sizeof(Cfg)         # mrx_config did not grow
    lib = native.load_capi()
    lib.mrx_abi_version.restype = ctypes.c_int
    assert lib.mrx_abi_version() == 4
    desc = scenes.synthetic_scene(3)
    ok = 0 if has_gpu() else MRX_E_NO_DEVICE
    assert _create(lib, desc, ctypes.sizeof(Cfg), None, flags=1 << 6) == ok
    assert _create(lib, desc, ctypes.sizeof(Cfg), None, flags=(1 << 6) | (1 << 2)) == ok
    assert _create(lib, desc, ctypes.sizeof(Cfg), None, flags=(1 << 6) | (1 << 3)) == ok
    assert _create(lib, desc, ctypes.sizeof(Cfg), None, flags=(1 << 6) | (1 << 2) | (1 << 3)) == MRX_E_INVALID
    assert hasattr(m.MadronaRenderer, "normal_tensor")


def test_scene_desc_and_its_shards_carry_the_flag():
    assert scenes.synthetic_scene(2).normals is False
    for desc in (scenes.synthetic_scene(7, with_wall=True), scenes.demo_scene(5)):
        desc.normals = True
        for rank in range(3):
            assert desc.shard(rank, 3).normals is True
        assert dataclasses.replace(desc).normals is True


def test_make_renderer_passes_the_flag_on(monkeypatch):
    import madrona_renderer_amd

    class Anything:
        def __getattr__(self, name):
            return Anything()

        def __call__(self, *a, **kw):
            return kw

    monkeypatch.setattr(madrona_renderer_amd, "load_module", lambda: Anything())
    desc = scenes.synthetic_scene(2)
    assert "normals" not in scenes.make_renderer(desc)
    desc.normals = True
    assert scenes.make_renderer(desc)["normals"] is True
    assert scenes.make_renderer(desc.shard(1, 2))["normals"] is True


def test_headless_knows_normals_ahead_of_any_device_work(native, tmp_path):
    from madrona_renderer_amd import build
    exe = build.headless_path()
    args = ["4", "1", "rast", "64", "64"]
    # the usage text names it ...
    p = subprocess.run(["timeout", "-k", "5", "60", exe] + args + ["--no-such-option"], cwd=tmp_path, capture_output=True,
                       text=True)
    assert p.returncode not in (0, 124, 137) and "[--normals]" in p.stderr, p.stderr
    # ... and the parser takes it: what it complains about is the option after it, not the usage
    p = subprocess.run(["timeout", "-k", "5", "60", exe] + args + ["--normals", "--vfov", "0"], cwd=tmp_path,
                       capture_output=True, text=True)
    assert p.returncode not in (0, 124, 137), p.stderr
    assert "--vfov" in p.stderr and "NUM_WORLDS" not in p.stderr, p.stderr
