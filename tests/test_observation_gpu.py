"""The packed observation output on the MI355X (-m gpu).

The observation kernel alone: the rgb and depth tensors filled with seeded values (depth a quarter exact zeros, values
below lo, above hi and equal to each, one that normalises to a float16 subnormal and one above 65504), observe(),
compared bit for bit with tests/observation_oracle.pack of what was written -- both modes at sizes that take the narrow
form, the wide form and the LDS tiles with and without edges, and the full cross of layouts, element types and range at
three of them.  The stack against the oracle's over six runs with resets through the column, the grid-stride loop on a
one-CU grid, the whole renderer through the raster kernels, the BVH tile kernel and the flat kernel with every other
output unchanged, the output selections, two shards against one, the option off, the headless tool's .npy, and the
yardstick: one observe() against the torch chain that produces the same tensor."""
import dataclasses
import statistics
import subprocess

import numpy as np
import pytest

from madrona_renderer_amd import scenes
from tests import observation_oracle as ob
from tests.test_projection_gpu import _make
from tests.test_supersample_gpu import PARITY, SIZES, _scene

pytestmark = pytest.mark.gpu

RT_SIZES = (5, 6, 7, 12, 33, 40, 64)
RANGE = (0.5, 20.0)


def _bits(t):
    """the bit patterns of a device tensor of any of the four element types, on the host"""
    import torch
    x = t.to_torch() if hasattr(t, "to_torch") else t
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[x.element_size()]
    return ob.bits(x.view(view).cpu().numpy())


def _opt(channels, dtype="float32", stack=1, depth_range=None):
    return dict(channels=channels, dtype=dtype, stack=stack, depth_range=depth_range)


def _fill(r, rng, channels, rt):
    """seeded rgb bytes and depth -- a quarter zeros, and the special values planted over the first pixels -- into the
    tensors the caller sees; returns what was written (None for a tensor the layout does not read)"""
    import torch
    rgb = depth = None
    if channels != "d":
        t = r.rgb_tensor().to_torch()
        rgb = rng.integers(0, 256, tuple(t.shape), dtype=np.uint8)
        t.copy_(torch.from_numpy(rgb).to(t.device))
    if channels in ("rgbd", "d", "yd"):
        t = r.depth_tensor().to_torch()
        depth = rng.uniform(0.01, 40.0, tuple(t.shape)).astype(np.float32)
        depth[rng.random(depth.shape) < 0.25] = 0.0
        lo, hi = np.float32(RANGE[0]), np.float32(RANGE[1])
        special = [0.0, -0.0, 0.25, lo, hi, 33.0, lo + np.float32(0.0005), 70000.0, np.nextafter(lo, np.float32(0)),
                   np.nextafter(hi, np.float32(100))]
        flat = depth.reshape(-1)
        at = rng.choice(flat.size, len(special), replace=False)
        flat[at] = np.array(special, np.float32)
        t.copy_(torch.from_numpy(depth).to(t.device))
    return rgb, depth


def _want(rgb, depth, opt, rt):
    return ob.pack(rgb, depth, opt["channels"], opt["dtype"], opt["depth_range"], rt)


def _assert_bits(got, want, what=""):
    want = ob.bits(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = int((got != want).sum())
    assert bad == 0, f"{what}: {bad} of {got.size} elements differ in their bits"


def _shape(desc, opt, rt):
    side = (desc.width, desc.width) if rt else (desc.height, desc.width)
    return (desc.num_views, opt["stack"] * ob.CHANNELS[opt["channels"]]) + side


def _kernel_alone(desc, opt, rng, outputs=None):
    rt = desc.render_mode == "Raytracer"
    r = _make(dataclasses.replace(desc, observations=opt), visibility=False, outputs=outputs)
    got_opt = r.observations
    assert got_opt["channels"] == opt["channels"] and got_opt["dtype"] == opt["dtype"] and got_opt["stack"] == opt["stack"]
    assert got_opt["depth_range"] == (None if opt["depth_range"] is None else tuple(np.float32(v) for v in opt["depth_range"]))
    t = r.observation_tensor().to_torch()
    assert tuple(t.shape) == _shape(desc, opt, rt), (tuple(t.shape), _shape(desc, opt, rt))
    assert t.element_size() == ob.ELEM_BYTES[opt["dtype"]] and str(t.dtype) == "torch." + opt["dtype"]
    r.sync()
    rgb, depth = _fill(r, rng, opt["channels"], rt)
    r.observe()
    r.sync()
    what = f"{desc.render_mode} {desc.width}x{desc.height} {opt}"
    _assert_bits(_bits(r.observation_tensor()), _want(rgb, depth, opt, rt), what)
    # rgb and depth are read, not written
    if rgb is not None:
        assert np.array_equal(r.rgb_tensor().to_torch().cpu().numpy(), rgb), what
    if depth is not None:
        assert np.array_equal(_bits(r.depth_tensor()), ob.bits(depth)), what
    return r


@pytest.mark.parametrize("mode", ["Rasterizer", "Raytracer"])
@pytest.mark.parametrize("channels,dtype", [("rgbd", "float16"), ("yd", "uint8")])
def test_the_observe_kernel_is_exact_on_random_frames(native, channels, dtype, mode):
    """Rasterizer: (5, 3) and (7, 5) take the narrow form -- views smaller than a wave, view boundaries inside a wave --
    (6, 6), (12, 8) and (40, 24) the wide one.  Raytracer: a view smaller than a tile, tile edges, one column past a
    tile (33) and exact tiles."""
    rng = np.random.default_rng(1500 + 10 * (dtype == "uint8") + (mode == "Raytracer"))
    sizes = SIZES if mode == "Rasterizer" else [(res, res) for res in RT_SIZES]
    for w, h in sizes:
        _kernel_alone(_scene(mode, w, h, worlds=3), _opt(channels, dtype, 1, RANGE), rng)


@pytest.mark.parametrize("dtype", list(ob.DTYPES))
@pytest.mark.parametrize("mode,w,h", [("Rasterizer", 7, 5), ("Rasterizer", 12, 8), ("Raytracer", 33, 33)])
def test_every_layout_and_element_type_with_and_without_a_range(native, mode, w, h, dtype):
    rng = np.random.default_rng(1000 * w + list(ob.DTYPES).index(dtype))
    for channels in ob.LAYOUTS:
        for depth_range in ((None, RANGE) if channels in ("rgbd", "d", "yd") else (None,)):
            _kernel_alone(_scene(mode, w, h, worlds=3), _opt(channels, dtype, 1, depth_range), rng)


@pytest.mark.parametrize("mode", ["Rasterizer", "Raytracer"])
@pytest.mark.parametrize("stack", [3, 8])
@pytest.mark.parametrize("w,h", [(5, 3), (12, 8)])
def test_the_stack_over_six_runs_with_resets(native, w, h, stack, mode):
    rng = np.random.default_rng(100 * stack + w + (mode == "Raytracer"))
    rt = mode == "Raytracer"
    desc = _scene(mode, w, h, worlds=3)
    opt = _opt("rgbd", "float16", stack, RANGE)
    r = _make(dataclasses.replace(desc, observations=opt), visibility=False)
    r.sync()
    col = r.observation_reset_tensor().to_torch()
    assert tuple(col.shape) == (3,) and str(col.dtype) == "torch.uint8"
    st = ob.Stack(stack)

    def current():
        d = r.depth_tensor().to_torch().cpu().numpy()
        return _want(r.rgb_tensor().to_torch().cpu().numpy(), d, opt, rt)

    # after creation every frame is the creation frame, and the column has been consumed
    _assert_bits(_bits(r.observation_tensor()), st.push(current()), "after creation")
    first = _bits(r.observation_tensor())
    C = ob.CHANNELS["rgbd"]
    for f in range(1, stack):
        assert np.array_equal(first[:, f * C:(f + 1) * C], first[:, :C])
    assert not col.cpu().numpy().any()
    for run in range(1, 7):
        rgb, depth = _fill(r, rng, "rgbd", rt)
        mask = None
        if run == 3:
            col[0] = 1
            col[2] = 1
            mask = np.array([True, False, True])
        r.observe()
        r.sync()
        assert not col.cpu().numpy().any(), run                 # consumed by exactly this run
        _assert_bits(_bits(r.observation_tensor()), st.push(_want(rgb, depth, opt, rt), mask), f"run {run}")
    # a new range restarts every stack from the frame packed under it
    r.set_observation_depth_range(1.0, 30.0)
    r.sync()
    assert r.observations["depth_range"] == (1.0, 30.0) and not col.cpu().numpy().any()
    opt2 = dict(opt, depth_range=(1.0, 30.0))
    _assert_bits(_bits(r.observation_tensor()), ob.Stack(stack).push(_want(rgb, depth, opt2, rt)), "new range")
    r.set_observation_depth_range(None)
    r.sync()
    assert r.observations["depth_range"] is None
    _assert_bits(_bits(r.observation_tensor()), ob.Stack(stack).push(_want(rgb, depth, dict(opt, depth_range=None), rt)), "no range")
    # step() pushes the rendered frame
    before = ob.bits(_bits(r.observation_tensor())).copy()
    r.step()
    r.sync()
    after = _bits(r.observation_tensor())
    assert np.array_equal(after[:, :-C], before[:, C:])
    _assert_bits(after[:, -C:], _want(r.rgb_tensor().to_torch().cpu().numpy(), r.depth_tensor().to_torch().cpu().numpy(),
                                      dict(opt, depth_range=None), rt), "step")


def test_the_grid_stride_loop_on_a_one_cu_grid(native, monkeypatch):
    """MRX_FAKE_CUS=1: eight workgroups.  4 views of 64 x 64 in the wide form: 4096 items, a stride of 2048; 5 views of
    40 x 24; 5 views of 41 x 25 in the narrow form, where the stride of 2048 pixels carries into the view; 5 views of
    res 40 in the tile form: 20 tiles on 8 workgroups."""
    monkeypatch.setenv("MRX_FAKE_CUS", "1")
    rng = np.random.default_rng(77)
    for mode, w, h, worlds in (("Rasterizer", 64, 64, 4), ("Rasterizer", 40, 24, 5), ("Rasterizer", 41, 25, 5),
                               ("Raytracer", 40, 40, 5)):
        rt = mode == "Raytracer"
        opt = _opt("rgbd", "float16", 2, RANGE)
        r = _kernel_alone(_scene(mode, w, h, worlds=worlds), dict(opt, stack=1), rng)
        del r
        r = _make(dataclasses.replace(_scene(mode, w, h, worlds=worlds), observations=opt), visibility=False)
        r.sync()
        st = ob.Stack(2)
        st.push(_want(r.rgb_tensor().to_torch().cpu().numpy(), r.depth_tensor().to_torch().cpu().numpy(), opt, rt))
        for run in range(2):
            rgb, depth = _fill(r, rng, "rgbd", rt)
            r.observe()
            r.sync()
            _assert_bits(_bits(r.observation_tensor()), st.push(_want(rgb, depth, opt, rt)), f"{mode} {w}x{h} run {run}")


@pytest.mark.parametrize("case", list(PARITY))
def test_the_whole_renderer_packs_its_own_frame(native, case):
    import torch
    build, variant, entry, bvh, rt, _ = PARITY[case]
    i = list(PARITY).index(case)
    s = 1 + i % 3
    opt = [_opt("rgbd", "float16", 2, RANGE), _opt("yd", "uint8", 1, RANGE), _opt("rgbd", "bfloat16", 3, None),
           _opt("rgb", "float32", 1, None)][i % 4]
    base = dataclasses.replace(build(), supersample=s, normals=True)
    r = _make(dataclasses.replace(base, observations=opt), visibility=not rt, variant=variant)
    plain = _make(base, visibility=not rt, variant=variant)
    if entry is not None:
        assert r.raster_entry() == entry
    assert r.bvh_launch()["kernel"] == bvh and plain.bvh_launch() == r.bvh_launch()
    assert plain.raster_entry() == r.raster_entry()
    r.sync()
    plain.sync()
    rgb, depth = r.rgb_tensor().to_torch().cpu().numpy(), r.depth_tensor().to_torch().cpu().numpy()
    assert (depth != 0).any() and (depth == 0).any()
    _assert_bits(_bits(r.observation_tensor()), ob.Stack(opt["stack"]).push(_want(rgb, depth, opt, rt)), case)
    # every other output is bit for bit that of the renderer without the option
    for getter in ("rgb_tensor", "depth_tensor", "normal_tensor", "segmask_tensor" if rt else "visibility_tensor"):
        a, b = getattr(r, getter)().to_torch(), getattr(plain, getter)().to_torch()
        assert a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), getter
    # ... and so are the bytes of a step, but for the stage's: its inputs and (2S - 1) * C * e per native pixel
    C, e, S = ob.CHANNELS[opt["channels"]], ob.ELEM_BYTES[opt["dtype"]], opt["stack"]
    inputs = 4 * (opt["channels"] != "d") + 4 * (opt["channels"] in ("rgbd", "d", "yd"))
    assert r.bytes_per_step() == plain.bytes_per_step() + depth.size * (inputs + (2 * S - 1) * C * e)


@pytest.mark.parametrize("mode", ["Rasterizer", "Raytracer"])
def test_the_output_selections_feed_the_layouts_they_can(native, mode):
    rng = np.random.default_rng(31 + (mode == "Raytracer"))
    base = _scene(mode, 40, 24, worlds=3)
    r = _kernel_alone(base, _opt("d", "float16", 1, RANGE), rng, outputs="Depth")
    with pytest.raises(RuntimeError):
        r.rgb_tensor()
    for channels in ("rgb", "y"):
        r = _kernel_alone(base, _opt(channels, "bfloat16"), rng, outputs="RGB")
        with pytest.raises(RuntimeError):
            r.depth_tensor()
    for channels, outputs in (("rgb", "Depth"), ("yd", "Depth"), ("d", "RGB"), ("rgbd", "RGB")):
        with pytest.raises(ValueError, match="observations"):
            _make(dataclasses.replace(base, observations=channels), visibility=False, outputs=outputs)


def test_two_shards_on_one_device_equal_one(native):
    import torch
    opt = _opt("rgbd", "float16", 3, RANGE)
    base = dataclasses.replace(_scene("Rasterizer", 40, 24, worlds=5), supersample=2, observations=opt)
    one = _make(base, visibility=True)
    two = _make(base, visibility=True, device_ids=[0, 0])
    assert two.num_shards == 2 and two.observations == one.observations
    two.step()
    one.step()
    one.sync()
    two.sync()

    def parts(getter):
        return torch.cat([getattr(two, getter)(shard=i).to_torch() for i in range(2)])

    for getter in ("observation_tensor", "depth_tensor", "rgb_tensor", "observation_reset_tensor"):
        whole = getattr(one, getter)().to_torch()
        assert whole.shape == parts(getter).shape and torch.equal(whole.view(torch.uint8), parts(getter).view(torch.uint8)), getter
    with pytest.raises(ValueError):
        two.observation_tensor()                            # several shards: say which
    # the reset column and observe() reach every shard: scribble over the two oldest frames, reset one view of each
    # shard, observe, and those views -- and only those -- are whole again (elsewhere one scribbled frame is left)
    C = 4
    for rr, cols in ((one, [(None, 1), (None, 4)]), (two, [(0, 1), (1, 1)])):
        for shard, view in cols:
            rr.observation_reset_tensor(shard=shard).to_torch()[view] = 1
        for shard in ({s for s, _ in cols}):
            rr.observation_tensor(shard=shard).to_torch()[:, :2 * C] = 0.25
        rr.observe()
        rr.sync()
    whole, split = one.observation_tensor().to_torch(), parts("observation_tensor")
    assert torch.equal(whole.view(torch.uint8), split.view(torch.uint8))
    assert not parts("observation_reset_tensor").any()
    for v in range(5):
        restarted = torch.equal(split[v, :C], split[v, -C:])
        assert restarted == (v in (1, 4)), v
    # the range setter reaches every shard too
    two.set_observation_depth_range(1.0, 9.0)
    one.set_observation_depth_range(1.0, 9.0)
    one.sync()
    two.sync()
    assert two.observations["depth_range"] == (1.0, 9.0)
    assert torch.equal(one.observation_tensor().to_torch().view(torch.uint8), parts("observation_tensor").view(torch.uint8))


def test_the_option_off_is_the_renderer_without_the_argument(native):
    import torch
    base = _scene("Raytracer", 40, 40, worlds=3)
    a = _make(base, visibility=False)
    b = _make(dataclasses.replace(base, observations=None), visibility=False)
    a.sync()
    b.sync()
    assert a.observations is None and b.observations is None
    assert a.raster_entry() == b.raster_entry() and a.bvh_launch() == b.bvh_launch() and a.bytes_per_step() == b.bytes_per_step()
    for getter in ("rgb_tensor", "depth_tensor", "segmask_tensor"):
        x, y = getattr(a, getter)().to_torch(), getattr(b, getter)().to_torch()
        assert x.shape == y.shape and torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    for r in (a, b):
        for call in (r.observation_tensor, r.observation_reset_tensor, r.observe, lambda: r.set_observation_depth_range(0.1, 20.0)):
            with pytest.raises(RuntimeError, match="MRX_FLAG_OBSERVATIONS"):
                call()
    px = 3 * 40 * 40
    for opt, extra in ((_opt("rgb"), 4 + 3 * 4), (_opt("rgbd", "float16", 4, RANGE), 8 + 7 * 4 * 2), (_opt("d", "uint8", 8), 4 + 15),
                       (_opt("yd", "bfloat16", 2), 8 + 3 * 2 * 2), ("y", 4 + 4)):
        c = _make(dataclasses.replace(base, observations=opt), visibility=False)
        assert c.bytes_per_step() == a.bytes_per_step() + px * extra, opt
        assert c.raster_entry() == a.raster_entry() and c.bvh_launch() == a.bvh_launch()
        if isinstance(opt, str) or opt["stack"] == 1:
            with pytest.raises(RuntimeError, match="MRX_FLAG_OBSERVATIONS"):        # no stack, no column
                c.observation_reset_tensor()
    assert _make(dataclasses.replace(base, observations="y"), visibility=False).observations == _opt("y")


@pytest.mark.parametrize("mode,spec,opt", [("rast", "rgbd,float16,2", _opt("rgbd", "float16", 2, (0.1, 20.0))),
                                           ("rt", "yd,bfloat16", _opt("yd", "bfloat16", 1, (0.1, 20.0)))])
def test_headless_writes_the_tensor_as_npy(native, tmp_path, mode, spec, opt):
    from madrona_renderer_amd import build
    cmd = ["timeout", "-k", "10", "120", build.headless_path(), "4", "1", mode, "64", "64", "--observations", spec,
           "--obs-depth-range", "0.1,20", "--dump-last-frame", "frame"]
    p = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    raw = open(tmp_path / "frame.obs.npy", "rb").read()
    assert raw[:8] == b"\x93NUMPY\x01\x00"
    hlen = int.from_bytes(raw[8:10], "little")
    header = raw[10:10 + hlen].decode()
    descr = {"float16": "<f2", "bfloat16": "<u2"}[opt["dtype"]]
    shape = (4, opt["stack"] * ob.CHANNELS[opt["channels"]], 64, 64)
    assert (10 + hlen) % 64 == 0 and header.endswith("\n")
    assert "'descr': '%s'" % descr in header and "'fortran_order': False" in header and "'shape': %r" % (shape,) in header
    got = np.load(tmp_path / "frame.obs.npy")
    assert got.shape == shape and got.dtype == np.dtype(descr)
    desc = scenes.synthetic_scene(4, render_mode="Raytracer" if mode == "rt" else "Rasterizer")
    r = _make(dataclasses.replace(desc, observations=opt), visibility=False)
    r.step()
    r.sync()
    want = _bits(r.observation_tensor())
    assert len(raw) == 10 + hlen + want.nbytes and np.array_equal(ob.bits(got), want)
    assert want.any()


def test_yardstick_one_observe_against_the_torch_chain(native):
    """1024 views of 64 x 64, rgbd, float16, a stack of 4, a range: one observe() against the torch chain that produces
    the same tensor from the same rgb and depth -- slice, permute, float, multiply by k, normalise and clamp depth, cat,
    half, and cat([old[:, C:], new], 1) into a second buffer.  Same process, same stream, mark / elapsed_ms around
    batches of 10, the median of 9 alternating batches.  The chain is the reference: first the two results are bit
    equal, then the stage takes no longer than the chain -- no margin."""
    import torch
    lo, hi = 0.1, 20.0
    opt = _opt("rgbd", "float16", 4, (lo, hi))
    r = _make(dataclasses.replace(scenes.synthetic_scene(1024), observations=opt), visibility=False)
    obs = r.observation_tensor().to_torch()
    rgb, depth = r.rgb_tensor().to_torch(), r.depth_tensor().to_torch()
    assert tuple(obs.shape) == (1024, 16, 64, 64) and obs.dtype == torch.float16
    assert tuple(rgb.shape) == (1024, 64, 64, 4) and tuple(depth.shape) == (1024, 64, 64, 1)
    C = 4
    k = float(ob.K)
    inv = float(np.float32(1.0) / (np.float32(hi) - np.float32(lo)))
    lo32 = float(np.float32(lo))
    old = torch.empty_like(obs)
    second = torch.empty_like(obs)
    one = torch.ones((), dtype=torch.float32, device=obs.device)

    def chain():
        colour = rgb[..., :3].permute(0, 3, 1, 2).float() * k
        d = depth.permute(0, 3, 1, 2)
        t = torch.where(d == 0, one, ((d - lo32) * inv).clamp(0.0, 1.0))
        new = torch.cat([colour, t], 1).half()
        torch.cat([old[:, C:], new], 1, out=second)

    # a few steps so that the stack holds history, then: the chain on the tensor as it is, observe(), equal bits
    for _ in range(2):
        r.step()
    r.sync()
    old.copy_(obs)
    chain()
    r.observe()
    r.sync()
    torch.cuda.synchronize()
    assert torch.equal(obs.view(torch.int16), second.view(torch.int16))
    assert (depth == 0).any() and (depth != 0).any()

    def timed(fn, batch=10):
        r.mark(0)
        for _ in range(batch):
            fn()
        r.mark(1)
        return r.elapsed_ms() * 1000.0 / batch

    def copy():
        second.copy_(obs)

    for fn in (r.observe, chain, copy):
        timed(fn, 20)                                       # warm-up
    stage, ch, cop = [], [], []
    for _ in range(9):                                      # alternating, so that a clock change hits all three
        stage.append(timed(r.observe))
        ch.append(timed(chain))
        cop.append(timed(copy))
    stage_us, chain_us, copy_us = statistics.median(stage), statistics.median(ch), statistics.median(cop)
    print(f"observe {stage_us:.2f} us, torch chain {chain_us:.2f} us, copy of the observation tensor {copy_us:.2f} us "
          f"(1024 x 64x64, rgbd float16 stack 4)")
    assert stage_us <= chain_us, (stage_us, chain_us)
