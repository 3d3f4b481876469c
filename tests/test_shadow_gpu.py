"""Cast shadows on the MI355X (-m gpu).

The shadow stage against tests/shadow_oracle.py applied to the renderer's own depth, cameras, projections and lights, on
every byte of the mask and of the darkened rgb; everything else against a twin renderer without the stage; the ray-cast
sensor as a second kernel that must agree; Raytracer mode, passes of one row, the brute form, an object with a BLAS,
supersampling, lights and poses changed between steps, two shards, the packed observation, cast(), a captured step, the
refusals and the yardstick against the trace stage."""
import dataclasses
import os
import statistics

import numpy as np
import pytest

from madrona_renderer_amd import scenes
from tests import observation_oracle as ob
from tests import position_oracle as pos
from tests import ray_oracle as ro
from tests import shadow_oracle as so
from tests.test_projection_gpu import _make
from tests.test_shadow_cpu import cube_scene, sphere_scene

pytestmark = pytest.mark.gpu

F = np.float32
WORLDS = 8
SIZES = [(24, 20), (64, 64)]

# the yardstick's bound: cast() took 88.50 us against 107.16 us for trace() of as many rays on one MI355X, ratio 0.826
# (profiles/shadow_latest.txt); times 1.5, rounded up to one decimal
YARDSTICK_RATIO = 1.3


def _np(t):
    return t.to_torch().cpu().numpy()


def _depth(r, **kw):
    d = _np(r.depth_tensor(**kw))
    return d.reshape(d.shape[:3])


@pytest.fixture()
def env():
    """MRX_SHADOW_* are read at attach: set through this, they are gone again after the test"""
    old = {k: os.environ.get(k) for k in ("MRX_SHADOW_BRUTE", "MRX_SHADOW_PASS_ROWS")}
    yield os.environ
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def _attach(r, **kw):
    from madrona_renderer_amd import shadows
    return shadows.attach(r, **kw)


def _state(r, desc, fs, s=1, shard=None):
    """what the stage reads NOW: the FlatScene with the rows of the renderer's pose tensors, its depth, its camera
    tensors, its projections and the light records of its views"""
    kw = {} if shard is None else {"shard": shard}
    fs.inst_pos[:] = _np(r.instance_position_tensor(**kw))
    fs.inst_rot[:] = _np(r.instance_rotation_tensor(**kw))
    fs.inst_scale[:] = _np(r.instance_scale_tensor(**kw))
    fs.inst_obj[:] = _np(r.instance_object_tensor(**kw))
    f, z = r.camera_projection()
    consts = pos.constants(desc.width, desc.height, fs.raytracer, list(zip(f.tolist(), z.tolist())), s)
    d, a, fl = r.world_light()
    lights = so.light_records(list(zip(d.tolist(), a.tolist(), fl.tolist())))[np.asarray(fs.view_world)]
    return dict(depth=_depth(r, **kw), cam_pos=_np(r.camera_position_tensor(**kw)),
                cam_rot=_np(r.camera_rotation_tensor(**kw)), consts=consts, lights=lights)


def _expected(r, desc, fs, s=1, bias=so.DEFAULT_BIAS, max_distance=None):
    st = _state(r, desc, fs, s)
    want = so.mask(fs, st["depth"], st["cam_pos"], st["cam_rot"], st["consts"], s, fs.raytracer, fs.view_world,
                   st["lights"], bias, max_distance)
    return want, st


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} of {got.size} bytes differ, first at {bad[:4].tolist()}"


OUTPUTS = ("rgb_tensor", "depth_tensor", "visibility_tensor", "normal_tensor", "position_tensor")


def _twin_equal(r, twin, getters, what):
    import torch
    for g in getters:
        a, b = getattr(r, g)().to_torch(), getattr(twin, g)().to_torch()
        assert a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (what, g)


# ---- the mask ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
def test_mask_only_is_the_oracle_s_and_every_other_tensor_the_twin_s(native, oracle_mod, w, h):
    desc = dataclasses.replace(cube_scene(WORLDS, width=w, height=h, vary=True), normals=True, positions="world")
    fs = oracle_mod.FlatScene(desc)
    r, twin = _make(desc), _make(desc)
    before = r.bytes_per_step()
    sh = _attach(r, apply=False)
    assert (sh.apply, sh.bias, sh.max_distance) == (False, 2.0 ** -10, None)
    assert r.bytes_per_step() == before + WORLDS * w * h * 5
    m = sh.mask_tensor()
    assert tuple(m.shape) == (WORLDS, h, w) and str(m.dtype) == "torch.uint8" and m.is_cuda
    r.sync()
    want, _ = _expected(r, desc, fs)
    _same(m.cpu().numpy(), want, "at attach")                   # it ran once
    for x in (r, twin):
        x.step()
        x.sync()
    want, st = _expected(r, desc, fs)
    _same(sh.mask_tensor().cpu().numpy(), want, "after a step")
    hit = st["depth"] > 0
    dark, lit = float((want[hit] == 0).mean()), float((want[hit] == 255).mean())
    print("%dx%d: occluded %.1f %% of the hit pixels, lit %.1f %%" % (w, h, 100 * dark, 100 * lit))
    assert dark >= 0.05 and lit >= 0.05
    _twin_equal(r, twin, OUTPUTS, "mask only")


@pytest.mark.parametrize("w,h", SIZES)
def test_apply_darkens_rgb_by_the_oracle_s_formula_and_nothing_else(native, oracle_mod, w, h):
    desc = dataclasses.replace(cube_scene(WORLDS, width=w, height=h, vary=True), normals=True, positions="world")
    fs = oracle_mod.FlatScene(desc)
    r, twin = _make(desc), _make(desc)
    sh = _attach(r, apply=True)
    for x in (r, twin):
        x.step()
        x.sync()
    want, st = _expected(r, desc, fs)
    mask = sh.mask_tensor().cpu().numpy()
    _same(mask, want, "mask")
    rgb0, normal = _np(twin.rgb_tensor()), _np(twin.normal_tensor())
    want_rgb, kept = so.apply(rgb0, normal, want, st["cam_rot"], st["lights"])
    got = _np(r.rgb_tensor())
    _same(got, want_rgb, "rgb")
    changed = (got != rgb0).any(axis=-1)
    print("%dx%d: apply changed %d pixels, kept %d occluded ones" % (w, h, changed.sum(), kept.sum()))
    assert changed.any() and kept.any() and not changed[mask == 255].any()
    _twin_equal(r, twin, [g for g in OUTPUTS if g != "rgb_tensor"], "apply")


def test_the_ray_sensor_agrees_on_every_hit_pixel(native, oracle_mod):
    """two kernels, one answer: the ray-cast sensor with R = H * W rays (position_tensor's point, bias * z, toLight,
    FLT_MAX) hits something exactly where the mask is 0"""
    import torch
    w, h = 24, 20
    desc = dataclasses.replace(cube_scene(WORLDS, width=w, height=h, vary=True), positions="world", rays=w * h)
    r = _make(desc)
    sh = _attach(r, apply=False)
    r.step()
    r.sync()
    p = r.position_tensor().to_torch().reshape(WORLDS, w * h, 4)
    z = r.depth_tensor().to_torch().reshape(WORLDS, w * h)
    d, a, f = r.world_light()
    to_light = torch.from_numpy(so.light_records(list(zip(d.tolist(), a.tolist(), f.tolist())))[:, :3]).to(p.device)
    rays = r.ray_tensor().to_torch()
    rays[:, :, 0:3] = p[:, :, 0:3]
    rays[:, :, 3] = z * float(so.DEFAULT_BIAS)
    rays[:, :, 4:7] = to_light[:, None, :]
    rays[:, :, 7] = float(so.FLT_MAX)
    r.trace()
    r.sync()
    ident = _np(r.ray_id_tensor()).reshape(WORLDS, h, w)
    mask = sh.mask_tensor().cpu().numpy()
    hit = _depth(r) > 0
    assert hit.any() and (mask[hit] == 0).any() and (mask[hit] == 255).any()
    assert np.array_equal(mask[hit] == 0, ident[hit] != -1)
    assert (mask[~hit] == 255).all()


# ---- small variants -----------------------------------------------------------------------------------------------------------
def _variant(oracle_mod, desc, s=1, apply=True, **attach_kw):
    desc = dataclasses.replace(desc, normals=True, supersample=s)
    fs = oracle_mod.FlatScene(desc)
    r, twin = _make(desc, visibility=False), _make(desc, visibility=False)
    sh = _attach(r, apply=apply, **attach_kw)
    for x in (r, twin):
        x.step()
        x.sync()
    want, st = _expected(r, desc, fs, s, attach_kw.get("bias", so.DEFAULT_BIAS), attach_kw.get("max_distance"))
    _same(sh.mask_tensor().cpu().numpy(), want, "mask")
    hit = st["depth"] > 0
    assert (want[hit] == 0).any() and (want[hit] == 255).any()
    if apply:
        want_rgb, _ = so.apply(_np(twin.rgb_tensor()), _np(twin.normal_tensor()), want, st["cam_rot"], st["lights"])
        _same(_np(r.rgb_tensor()), want_rgb, "rgb")
    return r, sh, fs, desc


def test_raytracer_mode(native, oracle_mod):
    r, sh, _, _ = _variant(oracle_mod, cube_scene(WORLDS, mode="Raytracer", vary=True))
    assert tuple(sh.mask_tensor().shape) == (WORLDS, 24, 24)


def test_passes_of_one_row(native, oracle_mod, env):
    env["MRX_SHADOW_PASS_ROWS"] = "1"
    _variant(oracle_mod, cube_scene(WORLDS, rows3=True, vary=True))


def test_the_brute_form(native, oracle_mod, env):
    env["MRX_SHADOW_BRUTE"] = "1"
    _variant(oracle_mod, cube_scene(WORLDS, rows3=True, vary=True))
    _variant(oracle_mod, sphere_scene(WORLDS))


def test_an_object_with_a_blas(native, oracle_mod):
    _, _, fs, _ = _variant(oracle_mod, sphere_scene(WORLDS))
    assert int(fs.obj_num_tris[0]) > 32


def test_supersample_2_and_a_short_max_distance(native, oracle_mod):
    _variant(oracle_mod, cube_scene(WORLDS, vary=True), s=2)
    _variant(oracle_mod, cube_scene(WORLDS, vary=True), bias=0.0, max_distance=1.25)


def test_lights_changed_between_steps_move_the_shadow(native, oracle_mod):
    r, sh, fs, desc = _variant(oracle_mod, cube_scene(WORLDS, vary=True))
    first = sh.mask_tensor().cpu().numpy().copy()
    lights = [((-0.5 + 0.125 * w, 0.25, -1.0), 0.0 if w == 3 else 0.2, 0.8) for w in range(WORLDS)]
    r.set_world_light(np.array([l[0] for l in lights], F), [l[1] for l in lights], [l[2] for l in lights])
    twin = _make(dataclasses.replace(desc, world_lights=lights), visibility=False)
    for x in (r, twin):
        x.step()
        x.sync()
    want, st = _expected(r, desc, fs)
    got = sh.mask_tensor().cpu().numpy()
    _same(got, want, "mask under the new lights")
    assert all((got[w] != first[w]).any() for w in range(WORLDS))       # no re-attach: every world's shadow moved
    want_rgb, _ = so.apply(_np(twin.rgb_tensor()), _np(twin.normal_tensor()), want, st["cam_rot"], st["lights"])
    _same(_np(r.rgb_tensor()), want_rgb, "rgb under the new lights")


def test_a_pose_write_between_steps(native, oracle_mod):
    import torch
    r, sh, fs, desc = _variant(oracle_mod, cube_scene(WORLDS, vary=True), apply=False)
    first = sh.mask_tensor().cpu().numpy().copy()
    p = r.instance_position_tensor().to_torch()
    p[1::2] += torch.tensor([0.375, 0.25, 0.125], device=p.device)     # every cube
    r.instance_object_tensor().to_torch()[1] = -1                       # and world 0's is hidden
    r.step()
    r.sync()
    want, st = _expected(r, desc, fs)
    got = sh.mask_tensor().cpu().numpy()
    _same(got, want, "mask after the pose write")
    assert (got != first).any() and (got[0] == 255).all() and (got[1][st["depth"][1] > 0] == 0).any()


def test_two_shards_on_one_device(native, oracle_mod):
    import torch
    desc = dataclasses.replace(cube_scene(5, vary=True), normals=True)
    one, two = _make(desc, visibility=False), _make(desc, visibility=False, device_ids=[0, 0])
    assert two.num_shards == 2
    sa, sb = _attach(one), _attach(two)
    for x in (one, two):
        x.step()
        x.sync()
    whole = sa.mask_tensor()
    parts = torch.cat([sb.mask_tensor(shard=i) for i in range(2)])
    assert torch.equal(whole, parts) and (whole == 0).any()
    assert torch.equal(one.rgb_tensor().to_torch(), torch.cat([two.rgb_tensor(shard=i).to_torch() for i in range(2)]))
    with pytest.raises(ValueError, match="say which shard"):
        sb.mask_tensor()
    # cast() reaches every shard: scribble over shard 1's mask, cast(), the same mask again
    sb.mask_tensor(shard=1).fill_(7)
    sb.cast()
    two.sync()
    assert torch.equal(whole, torch.cat([sb.mask_tensor(shard=i) for i in range(2)]))


def test_the_observation_packs_the_shadowed_rgb(native, oracle_mod):
    desc = dataclasses.replace(cube_scene(WORLDS, vary=True), normals=True, observations="rgb")
    r, twin = _make(desc, visibility=False), _make(desc, visibility=False)
    _attach(r, apply=True)
    for x in (r, twin):
        x.step()
        x.sync()
    rgb = _np(r.rgb_tensor())
    assert (rgb != _np(twin.rgb_tensor())).any()
    got = _np(r.observation_tensor())
    assert np.array_equal(ob.bits(got), ob.bits(ob.pack(rgb, None, "rgb", "float32")))
    assert not np.array_equal(got, _np(twin.observation_tensor()))


def test_cast_twice_leaves_rgb_as_the_step_left_it(native, oracle_mod):
    r, sh, _, _ = _variant(oracle_mod, cube_scene(WORLDS, vary=True))
    rgb, mask = _np(r.rgb_tensor()).copy(), sh.mask_tensor().cpu().numpy().copy()
    for _ in range(2):
        sh.mask_tensor().fill_(9)
        sh.cast()
        r.sync()
        assert np.array_equal(sh.mask_tensor().cpu().numpy(), mask)
        assert np.array_equal(_np(r.rgb_tensor()), rgb)              # never darkened twice


def test_a_captured_step_equals_the_eager_twin(native, oracle_mod):
    """a step with the stage attached, captured with torch.cuda.graph on the renderer's single stream and replayed, against
    the same motion and step() run eagerly (the pattern of tests/test_captured_step_gpu.py)"""
    import torch
    desc = dataclasses.replace(cube_scene(WORLDS, width=64, height=64, vary=True), normals=True, observations="rgb")
    twins = []
    for _ in range(2):
        r = _make(desc, visibility=False)
        side = torch.cuda.Stream()
        r.set_stream(side.cuda_stream)
        sh = _attach(r, apply=True)
        cam = r.camera_position_tensor().to_torch()
        with torch.cuda.stream(side):
            delta = torch.zeros_like(cam)
            for _ in range(2):                                  # warm-up
                r.step()
        side.synchronize()
        twins.append((r, side, sh, cam, delta))
    r, side, sh, cam, delta = twins[0]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        cam.add_(delta)
        r.step()
    rng = np.random.default_rng(1)
    for rep in range(3):
        step = rng.uniform(-0.05, 0.05, tuple(cam.shape)).astype(F)
        for i, (x, s, _, c, dl) in enumerate(twins):
            with torch.cuda.stream(s):
                dl.copy_(torch.from_numpy(step).to(dl.device))
                if i == 0:
                    graph.replay()
                else:
                    c.add_(dl)
                    x.step()
            s.synchronize()
            x.sync()
        a, b = twins
        assert torch.equal(a[2].mask_tensor(), b[2].mask_tensor()), rep
        for g in ("rgb_tensor", "depth_tensor", "normal_tensor", "observation_tensor"):
            ta, tb = getattr(a[0], g)().to_torch(), getattr(b[0], g)().to_torch()
            assert torch.equal(ta.view(torch.uint8), tb.view(torch.uint8)), (rep, g)
        assert (a[2].mask_tensor() == 0).any()


def test_refusals(native):
    from madrona_renderer_amd import shadows
    desc = cube_scene(3)
    r = _make(dataclasses.replace(desc, normals=True), visibility=False)
    shadows.attach(r)
    with pytest.raises(RuntimeError, match="already casts shadows"):
        shadows.attach(r)
    rgb_only = _make(desc, visibility=False, outputs="RGB")
    with pytest.raises(RuntimeError, match="shadows need depth"):
        shadows.attach(rgb_only, apply=False)
    plain = _make(desc, visibility=False)
    with pytest.raises(RuntimeError, match="need the normal tensor"):
        shadows.attach(plain, apply=True)
    depth_only = _make(dataclasses.replace(desc, normals=True), visibility=False, outputs="Depth")
    with pytest.raises(RuntimeError, match="apply need rgb"):
        shadows.attach(depth_only, apply=True)
    # the refused renderers work on, and take what they can have; a renderer without the stage says so
    for x in (rgb_only, plain, depth_only):
        x.step()
        x.sync()
    lib = shadows._capi()
    assert lib.mrx_shadows(plain.native_handle()) == 0 and lib.mrx_shadows(r.native_handle()) == 2
    assert lib.mrx_shadow(plain.native_handle()) == -5                      # MRX_E_UNSUPPORTED
    assert b"mrx_shadow_create was not called" in lib.mrx_last_error()
    shadows.attach(depth_only, apply=False)
    assert lib.mrx_shadows(depth_only.native_handle()) == 1
    depth_only.step()
    depth_only.sync()


def _measure(reps=20):
    """(cast us, trace us): 1024 worlds of 64 x 64 synthetic_scene, H * W pinhole rays per world for the sensor, in one
    process, alternating, the median of `reps` after a warm-up"""
    import torch
    from oracle import oracle
    desc = scenes.synthetic_scene(1024)
    fs = oracle.FlatScene(desc)
    R = desc.width * desc.height
    rays = np.stack([ro.pinhole(fs, v, tmin=oracle.RASTER_ZNEAR) for v in range(desc.num_worlds)])
    r = scenes.make_renderer(dataclasses.replace(desc, rays=R), render_outputs="Depth")
    t = r.ray_tensor().to_torch()
    t.copy_(torch.from_numpy(rays).to(t.device))
    sh = _attach(r, apply=False)
    r.sync()

    def timed(fn):
        r.mark(0)
        fn()
        r.mark(1)
        return r.elapsed_ms() * 1000.0

    for fn in (sh.cast, r.trace):
        for _ in range(5):
            timed(fn)
    cast, trace = [], []
    for _ in range(reps):                                       # alternating, so that a clock change hits both
        cast.append(timed(sh.cast))
        trace.append(timed(r.trace))
    occluded = float((sh.mask_tensor() == 0).float().mean())
    return statistics.median(cast), statistics.median(trace), occluded


def test_yardstick_cast_against_trace(native):
    """cast() against trace() of the ray-cast sensor with as many rays: the trace stage is the parent's, the comparison
    is not of the stage against itself.  Measured 88.50 us against 107.16 us, ratio 0.826 (profiles/shadow_latest.txt,
    DESIGN.md 4.25); the bound is that ratio times 1.5, rounded up to one decimal: 1.3."""
    c, t, occluded = _measure()
    print(f"cast {c:.2f} us, trace {t:.2f} us, ratio {c / t:.3f}, occluded share {occluded:.3f} (1024 x 64x64)")
    assert occluded > 0
    assert c <= YARDSTICK_RATIO * t, (c, t)
