"""A captured step with every stage on, held to the eager step (-m gpu; INTEGRATION.md "What a captured step reads live").

step() is a chain of launches -- render, resolve, unproject, box fill, boxes, observe, the reset column's memset, rays, flow,
flow snapshot -- and two of its stages carry state from one step to the next.  Twins: two renderers of one description,
each on a torch side stream of its own; one replays "motion, step()" from a hipGraph captured once, the other runs the same
motion and step() eagerly.  After every repetition every tensor of the two is compared by its bits, and the replayed twin
is held to the NumPy oracles of the stages with memory (flow, observation stack) after every replay -- with flow and
snapshot swapped in launch() the first replay's flow fails -- and, on the last frame, to those of the boxes, the positions
and the rays.

Boxes need label or segmask ids and flow needs visibility ids, so "everything on" is two descriptions: the label side and
the flow side.  Both on the three render paths at the smallest shapes at which each is still itself, with mixed per-view
projections set at creation, so that the table forms are the ones captured.  What a replay must read live -- the reset
column, the flow snapshot, the rays, the ObjectID sign, the projection tables -- is written between two replays, test by
test.  And eagerly: every output of the two widest renderers is that of a renderer with only that one stage on."""
import dataclasses

import numpy as np
import pytest

from tests import box_oracle as bo
from tests import meshes  # noqa: F401  (the BVH case's builder, through PARITY)
from tests import position_oracle as pos
from tests import projection_oracle as po
from tests import ray_oracle as ro
from tests.observation_oracle import CHANNELS, Stack, bits, pack
from tests.test_flow_gpu import _assert_bits, _consts, _expected, _state, _tables
from tests.test_projection_gpu import _make
from tests.test_supersample_gpu import PARITY, _scene

pytestmark = pytest.mark.gpu

F = np.float32
RANGE = (0.5, 20.0)
RAYS = 100
K = 8
REPETITIONS = 5                     # more than the stack depth
FRAMES = np.array([-1, 1, 0], np.int32)     # world 0's rays in the world frame, the others mounted on a moving row

# name: (builder, kernel variant, raster entry, bvh kernel, raytracer, s) -- the smallest shapes of the existing case
# tables at which the group kernel, the BVH tile kernel and the flat kernel are still themselves
CASES = {
    "group": (lambda: _scene("Rasterizer", 40, 24, worlds=3), None, "group", "none", False, 2),
    "bvh-tile": (PARITY["bvh-tile-40x24"][0], None, "bvh", "tile", False, 2),
    "flat": (lambda: _scene("Raytracer", 40, 40, worlds=3), 2, "bvh", "flat", True, 3),
}

COMMON = ("rgb_tensor", "depth_tensor", "normal_tensor", "position_tensor", "observation_tensor",
          "observation_reset_tensor", "ray_distance_tensor", "ray_id_tensor")
OUTPUTS = {"label": COMMON + ("segmask_tensor", "box_tensor"), "flow": COMMON + ("visibility_tensor", "flow_tensor")}
OBS = {"label": dict(channels="rgbd", dtype="float16", stack=3, depth_range=RANGE),
       "flow": dict(channels="yd", dtype="uint8", stack=3, depth_range=RANGE)}
FRAME = {"label": "view", "flow": "world"}


def _base(case):
    """the case's scene at its factor with mixed per-view projections, and nothing else on"""
    build, variant, entry, bvh, rt, s = CASES[case]
    base = build()
    return dataclasses.replace(base, supersample=s, camera_projections=po.mixed(len(base.cameras)))


def _wide(base, side):
    """the widest renderer of a side: every stage the side admits"""
    if side == "label":
        return dataclasses.replace(base, normals=True, positions="view", instance_labels=True, boxes=K,
                                   observations=OBS["label"], rays=RAYS)
    return dataclasses.replace(base, normals=True, positions="world", observations=OBS["flow"], rays=RAYS, flow=True)


def _np(t):
    return t.to_torch().cpu().numpy()


def _raw(t):
    """the bytes of a device tensor, on the host"""
    import torch
    return t.to_torch().contiguous().view(torch.uint8).cpu().numpy().copy()


class Twin:
    """a renderer on a torch side stream of its own, the device tensors of the motion, and -- once captured -- the graph
    of "motion, step()" """

    def __init__(self, desc, case, rays, visibility=False):
        import torch
        build, variant, entry, bvh, rt, s = CASES[case]
        # (visibility: the renderers of the flow side without flow=, which sets the flag itself)
        self.r = r = _make(desc, visibility=visibility, variant=variant)
        assert r.raster_entry() == entry and r.bvh_launch()["kernel"] == bvh and r.supersample == s
        assert r.num_shards == 1
        self.side = torch.cuda.Stream()
        r.set_stream(self.side.cuda_stream)
        self.pos, self.rot, self.cam = (getattr(r, g)().to_torch() for g in (
            "instance_position_tensor", "instance_rotation_tensor", "camera_position_tensor"))
        with torch.cuda.stream(self.side):
            self.d_pos, self.d_q, self.d_cam = (torch.zeros_like(t) for t in (self.pos, self.rot, self.cam))
        self.graph = None
        if rays is not None:
            self.put("ray_tensor", rays)
            self.put("ray_frame_tensor", FRAMES)

    def put(self, getter, array):
        """a host array into one of the renderer's tensors, on the renderer's stream"""
        import torch
        with torch.cuda.stream(self.side):
            t = getattr(self.r, getter)().to_torch()
            a = torch.from_numpy(np.array(array))
            assert tuple(t.shape) == tuple(a.shape) and t.dtype == a.dtype, (getter, t.shape, a.shape, t.dtype, a.dtype)
            t.copy_(a.to(t.device))

    def deltas(self, d_pos, d_q, d_cam):
        import torch
        with torch.cuda.stream(self.side):
            for t, a in ((self.d_pos, d_pos), (self.d_q, d_q), (self.d_cam, d_cam)):
                t.copy_(torch.from_numpy(np.ascontiguousarray(a, F)).to(t.device))

    def motion(self):
        self.pos.add_(self.d_pos)
        self.cam.add_(self.d_cam)
        q = self.rot + self.d_q
        self.rot.copy_(q / q.norm(dim=1, keepdim=True))

    def capture(self):
        import torch
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=self.side):
            self.motion()
            self.r.step()

    def advance(self):
        """one repetition: the replay if there is a graph, else the motion and step() eagerly; on the side stream"""
        import torch
        with torch.cuda.stream(self.side):
            if self.graph is not None:
                self.graph.replay()
            else:
                self.motion()
                self.r.step()

    def call(self, fn):
        """fn(renderer) with the side stream current"""
        import torch
        with torch.cuda.stream(self.side):
            return fn(self.r)

    def sync(self):
        self.side.synchronize()
        self.r.sync()

    def outputs(self, side):
        return {g: _raw(getattr(self.r, g)()) for g in OUTPUTS[side]}


def _zero(shape):
    return np.zeros(shape, F)


class Pair:
    """the replayed twin and the eager twin of one case and side, warmed up and captured, with the observation oracle
    of the replayed twin's stack kept alongside"""

    def __init__(self, case, side, oracle_mod):
        build, variant, entry, bvh, rt, s = CASES[case]
        self.case, self.side, self.rt, self.s = case, side, rt, s
        self.base = _base(case)
        self.desc = _wide(self.base, side)
        self.fs = oracle_mod.FlatScene(self.base)
        self.tables = _tables(self.fs)
        self.rng = np.random.default_rng(1000 * len(case) + len(side))
        rays = ro.mixed(self.fs, RAYS, seed=3)
        self.replayed, self.eager = Twin(self.desc, case, rays), Twin(self.desc, case, rays)
        self.twins = (self.replayed, self.eager)
        self.stack = Stack(3)
        r = self.replayed.r
        assert r.observations["stack"] == 3 and r.rays == RAYS and r.positions == FRAME[side]
        assert (r.flows is True) == (side == "flow") and (r.box_labels == K) == (side == "label")
        f, _ = r.camera_projection()
        # the tables vary, and the form that reads them is what is captured: normals over the label column (the group
        # kernel of the label side) or over the per-view tables
        assert len(set(f.tolist())) > 1
        assert r.kernel_form()["form"] == ("LN" if (case, side) == ("group", "label") else "NPV"), r.kernel_form()
        for t in self.twins:
            t.sync()
        self._observe("as created")
        # the warm-up: one eager repetition on both, so that every instantiation has its function attributes
        self._deltas()
        for t in self.twins:
            t.advance()
        for t in self.twins:
            t.sync()
        self._observe("warm-up")
        self._same("warm-up")
        self.replayed.capture()
        for t in self.twins:
            t.sync()
        self._same("captured")                                  # a capture runs nothing

    def _deltas(self, zero=False):
        n, v = len(self.fs.inst_pos), self.fs.num_views
        if zero:
            d = (_zero((n, 3)), _zero((n, 4)), _zero((v, 3)))
        else:
            d = (self.rng.uniform(-0.3, 0.3, (n, 3)), self.rng.normal(scale=0.05, size=(n, 4)),
                 self.rng.uniform(-0.2, 0.2, (v, 3)))
        for t in self.twins:
            t.deltas(*d)

    def frame(self):
        """the replayed twin's current frame, packed as its observation stage packs it"""
        r = self.replayed.r
        o = OBS[self.side]
        return pack(_np(r.rgb_tensor()), _np(r.depth_tensor()), o["channels"], o["dtype"], o["depth_range"], self.rt)

    def _observe(self, what, reset=None):
        """push the replayed twin's frame onto the oracle stack; its tensor is the oracle's, its reset column consumed"""
        import torch
        r = self.replayed.r
        want = bits(self.stack.push(self.frame(), reset))
        t = r.observation_tensor().to_torch()
        view = {1: torch.uint8, 2: torch.int16}[t.element_size()]
        got = bits(t.view(view).cpu().numpy())
        assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
        bad = int((got != want).sum())
        assert bad == 0, f"{self.case} {self.side} {what}: {bad} of {got.size} observation elements differ in their bits"
        for t in self.twins:
            assert not _np(t.r.observation_reset_tensor()).any(), (what, "the reset column is consumed by every run")

    def _same(self, what):
        a, b = self.replayed.outputs(self.side), self.eager.outputs(self.side)
        for g in OUTPUTS[self.side]:
            assert a[g].shape == b[g].shape, (what, g)
            bad = int((a[g] != b[g]).sum())
            assert bad == 0, f"{self.case} {self.side} {what}: {g}: {bad} of {a[g].size} bytes differ, replayed against eager"
        return a

    def step(self, what, zero=False, reset=None):
        """one repetition: new deltas, the replay on one twin and the eager motion and step on the other, everything
        compared; returns the replayed twin's outputs as bytes"""
        self._deltas(zero)
        for t in self.twins:
            t.advance()
        for t in self.twins:
            t.sync()
        out = self._same(what)
        self._observe(what, reset)
        return out

    def on_both(self, fn):
        for t in self.twins:
            t.call(fn)

    def put_both(self, getter, array):
        for t in self.twins:
            t.put(getter, array)

    # ---- the oracles of the replayed twin's current frame ----
    def live_scene(self):
        """the FlatScene with the rows of the replayed twin's pose tensors"""
        r, fs = self.replayed.r, self.fs
        fs.inst_pos, fs.inst_rot, fs.inst_scale = (_np(getattr(r, g)()).copy() for g in (
            "instance_position_tensor", "instance_rotation_tensor", "instance_scale_tensor"))
        fs.inst_obj = _np(r.instance_object_tensor()).copy()
        return fs

    def check_rays(self, what):
        r = self.replayed.r
        labels = _np(r.instance_label_tensor()) if self.side == "label" else None
        want_t, want_id = ro.trace(self.live_scene(), _np(r.ray_tensor()), _np(r.ray_frame_tensor()), labels)
        got_t, got_id = _np(r.ray_distance_tensor()), _np(r.ray_id_tensor())
        bad = ~((got_t.view(np.uint32) == want_t.view(np.uint32)) | (np.isnan(got_t) & np.isnan(want_t))) | (got_id != want_id)
        assert not bad.any(), (self.case, self.side, what, int(bad.sum()), np.argwhere(bad)[:5])
        return got_id

    def check_positions(self, what):
        r = self.replayed.r
        d = _np(r.depth_tensor())
        want = pos.unproject(d.reshape(d.shape[:3]), _np(r.camera_position_tensor()), _np(r.camera_rotation_tensor()),
                             _consts(r, self.base, self.s, self.rt), self.s, FRAME[self.side], self.rt)
        _assert_bits(_np(r.position_tensor()), want, f"{self.case} {self.side} {what}: positions")

    def check_boxes(self, what):
        r = self.replayed.r
        got, want = _np(r.box_tensor()), bo.boxes(_np(r.segmask_tensor()), K, self.rt)
        assert got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want), (self.case, what)
        return got

    def flow_before(self):
        """what the flow of the next step is measured against: the state and constants as they are now"""
        r = self.replayed.r
        return _state(r), _consts(r, self.base, self.s, self.rt)

    def check_flow(self, what, prev, prev_consts):
        r = self.replayed.r
        got = _np(r.flow_tensor())
        _assert_bits(got, _expected(r, self.base, self.tables, self.s, self.rt, prev, prev_consts),
                     f"{self.case} {self.side} {what}: flow")
        return got

    def check_frame(self, what):
        self.check_positions(what)
        ids = self.check_rays(what)
        if self.side == "label":
            self.check_boxes(what)
        return ids


# ---- 2. five replays against five eager steps -----------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["label", "flow"])
@pytest.mark.parametrize("case", list(CASES))
def test_five_replays_equal_five_eager_steps(native, oracle_mod, case, side):
    p = Pair(case, side, oracle_mod)
    frames, moving, counted, hits = [], False, False, False
    for rep in range(REPETITIONS):
        before = p.flow_before() if side == "flow" else None
        out = p.step(f"replay {rep}")
        if side == "flow":                                      # every replay's flow is the oracle's, from the first on:
            p.check_flow(f"replay {rep}", *before)              # the snapshot kernel runs behind the flow kernel
        frames.append(out["rgb_tensor"])
        r = p.replayed.r
        hits = hits or bool((_np(r.ray_id_tensor()) != -1).any())
        if side == "label":
            counted = counted or bool((_np(r.box_tensor())[..., 4] > 0).any())
        else:
            fl = _np(r.flow_tensor())
            moving = moving or bool((fl[fl[..., 3] == 1][:, :3] != 0).any())
    # the replayed twin's last frame against the oracles
    ids = p.check_frame("last replay")
    # ... and none of it vacuous
    assert all((frames[i] != frames[i - 1]).any() for i in range(1, REPETITIONS)), "the frames differ between repetitions"
    assert hits and (ids != -1).any() and (ids == -1).any()
    assert counted if side == "label" else moving


# ---- 3. what a replay must read live ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["label", "flow"])
def test_a_replay_reads_the_reset_column_and_its_memset_clears_it(native, oracle_mod, side):
    p = Pair("group", side, oracle_mod)
    for rep in range(3):
        p.step(f"replay {rep}")
    C = CHANNELS[OBS[side]["channels"]]
    shifted = p.stack.tensor.copy()
    assert (shifted[:, :C] != shifted[:, -C:]).any()            # the stack holds different frames
    col = np.array([1, 0, 1], np.uint8)
    p.put_both("observation_reset_tensor", col)
    p.step("reset", reset=col.astype(bool))                     # compared with Stack.push(frame, mask); the column all zero
    got = p.stack.tensor
    for v in (0, 2):                                            # the current frame in every slot
        assert all(np.array_equal(got[v, f * C:(f + 1) * C], got[v, -C:]) for f in range(3))
    assert np.array_equal(got[1, :-C], shifted[1, C:]) and (got[1, :C] != got[1, -C:]).any()   # the other has shifted
    p.step("after the reset")                                   # nothing sticks: every view shifts again


def test_a_replay_reads_the_flow_snapshot(native, oracle_mod):
    import torch
    p = Pair("group", "flow", oracle_mod)
    p.step("replay 0")
    old = p.flow_before()                                       # what the last step's snapshot holds
    # a teleport, then flow_snapshot() eagerly: the next replay, with zero deltas, shows the still scene
    p.on_both(lambda r: r.instance_position_tensor().to_torch().add_(
        torch.tensor([0.5, -0.25, 0.125], device="cuda")))
    p.on_both(lambda r: r.flow_snapshot())
    for t in p.twins:
        t.sync()
    new = p.flow_before()
    assert (new[0][0] != old[0][0]).any()
    p.step("after flow_snapshot()", zero=True)
    still = p.check_flow("after flow_snapshot()", *new)
    r = p.replayed.r
    valid = still[..., 3] == 1
    assert valid.any() and (~valid).any()
    # zero motion up to the rounding of a round trip: far below the teleport's, which the old snapshot would have shown
    teleport = _expected(r, p.base, p.tables, p.s, p.rt, *old)
    assert np.abs(still[valid][:, :3]).max() < 1e-2 < np.abs(teleport[teleport[..., 3] == 1][:, :3]).max()
    assert np.array_equal(still[..., 3], teleport[..., 3])      # w is unchanged
    p.step("the replay after")                                  # ... and the snapshot goes on following the steps


@pytest.mark.parametrize("side", ["label", "flow"])
def test_a_replay_reads_the_rays(native, oracle_mod, side):
    p = Pair("group", side, oracle_mod)
    p.step("replay 0")
    before = p.check_rays("replay 0")
    rays = ro.mixed(p.live_scene(), RAYS, seed=11)
    assert all(n > 0 for n in ro.degenerate_kinds(rays)), ro.degenerate_kinds(rays)
    frames = np.array([2, -1, 0], np.int32)
    p.put_both("ray_tensor", rays)
    p.put_both("ray_frame_tensor", frames)
    p.step("new rays")
    after = p.check_rays("new rays")
    r = p.replayed.r
    assert np.array_equal(_np(r.ray_tensor()).view(np.uint32), rays.view(np.uint32))
    assert np.array_equal(_np(r.ray_frame_tensor()), frames)
    assert (after != -1).any() and not np.array_equal(after, before)


@pytest.mark.parametrize("side", ["label", "flow"])
def test_a_replay_reads_the_sign_of_the_objectid_column(native, oracle_mod, side):
    p = Pair("group", side, oracle_mod)
    p.step("replay 0")
    row, world, obj = 3, 1, 1                                   # world 1's ground quad: object 1, rows 3 ... 5
    shown = _np(p.replayed.r.instance_object_tensor()).copy()
    assert shown[row] == obj and p.fs.world_inst_start[world] == row
    lo = int(p.tables[0][row])
    hi = lo + int(p.fs.obj_num_tris[obj])

    def seen():
        """is the row in the ids of its view, and in the ids of its world's rays"""
        r = p.replayed.r
        if side == "label":
            ids = _np(r.segmask_tensor())[world]
            in_view = bool((ids == obj).any())
            assert in_view == bool(_np(r.box_tensor())[world, obj, 4] > 0)
        else:
            ids = _np(r.visibility_tensor())[world]
            in_view = bool(((ids >= lo) & (ids < hi)).any())
        return in_view, bool((_np(r.ray_id_tensor())[world] == obj).any())

    assert seen() == (True, True)
    hidden = shown.copy()
    hidden[row] = -hidden[row]
    p.put_both("instance_object_tensor", hidden)                # no refresh_objects(): only the sign is read
    p.step("hidden", zero=True)
    p.check_frame("hidden")
    assert seen() == (False, False)
    p.put_both("instance_object_tensor", shown)
    p.step("shown again", zero=True)
    p.check_frame("shown again")
    assert seen() == (True, True)


@pytest.mark.parametrize("side", ["label", "flow"])
def test_a_replay_reads_the_projection_tables(native, oracle_mod, side):
    p = Pair("group", side, oracle_mod)
    p.step("replay 0")
    old = p.flow_before()
    first = p.replayed.outputs(side)
    # every view's constants change, the first view's -- the ones a launch holds as uniform arguments -- among them
    p.on_both(lambda r: r.set_camera_projection([100.0, 40.0, 75.0], [0.25, 0.5, 2.0]))
    for t in p.twins:
        t.sync()
    new_consts = _consts(p.replayed.r, p.base, p.s, p.rt)
    assert (new_consts != old[1]).any(axis=1).all()
    out = p.step("new projections", zero=True)                  # the twin: the render, the positions and the flow agree
    assert (out["rgb_tensor"] != first["rgb_tensor"]).any() and (out["depth_tensor"] != first["depth_tensor"]).any()
    p.check_frame("new projections")                            # positions unproject with the new constants
    if side == "flow":
        p.check_flow("new projections", *old)                   # ... and the flow takes the old ones as its previous
    before = p.flow_before()
    p.step("the replay after")
    if side == "flow":
        p.check_flow("the replay after", *before)


# ---- 5. eagerly: the widest renderers against renderers with one stage each -----------------------------------------------
# stage: (what it adds to the base, the tensors it is compared on)
STAGES = {
    "label": {
        "none": ({}, ("rgb_tensor", "depth_tensor", "segmask_tensor")),
        "normals": (dict(normals=True), ("normal_tensor",)),
        "positions": (dict(positions="view"), ("position_tensor",)),
        "boxes": (dict(boxes=K), ("box_tensor",)),
        "observations": (dict(observations=OBS["label"]), ("observation_tensor", "observation_reset_tensor")),
        "rays": (dict(rays=RAYS), ("ray_distance_tensor", "ray_id_tensor")),
    },
    "flow": {
        "none": ({}, ("rgb_tensor", "depth_tensor", "visibility_tensor")),
        "normals": (dict(normals=True), ("normal_tensor",)),
        "positions": (dict(positions="world"), ("position_tensor",)),
        "observations": (dict(observations=OBS["flow"]), ("observation_tensor", "observation_reset_tensor")),
        "rays": (dict(rays=RAYS), ("ray_distance_tensor", "ray_id_tensor")),
        "flow": (dict(flow=True), ("flow_tensor", "visibility_tensor")),
    },
}


@pytest.mark.parametrize("side", ["label", "flow"])
@pytest.mark.parametrize("case", list(CASES))
def test_every_output_of_the_widest_renderer_is_that_of_a_renderer_with_one_stage(native, oracle_mod, case, side):
    base = _base(case)
    if side == "label":
        base = dataclasses.replace(base, instance_labels=True)          # (a column, not a stage: the segmask's ids)
    fs = oracle_mod.FlatScene(base)
    rays = ro.mixed(fs, RAYS, seed=3)
    rng = np.random.default_rng(len(case) + 10 * len(side))
    n, v = len(fs.inst_pos), fs.num_views
    deltas = [(rng.uniform(-0.3, 0.3, (n, 3)), rng.normal(scale=0.05, size=(n, 4)), rng.uniform(-0.2, 0.2, (v, 3)))
              for _ in range(3)]

    def run(desc, with_rays, visibility):
        t = Twin(desc, case, rays if with_rays else None, visibility=visibility)
        for d in deltas:                                        # three steps: the stack fills, the snapshot follows
            t.deltas(*d)
            t.advance()
        t.sync()
        return t

    wide = run(_wide(base, side), True, False)
    got = wide.outputs(side)
    assert got["observation_tensor"].any() and (got["ray_id_tensor"] != 0xFF).any()
    seen = set()
    for stage, (extra, getters) in STAGES[side].items():
        narrow = run(dataclasses.replace(base, **extra), "rays" in extra, side == "flow" and "flow" not in extra)
        for g in getters:
            want = _raw(getattr(narrow.r, g)())
            assert got[g].shape == want.shape, (stage, g)
            bad = int((got[g] != want).sum())
            assert bad == 0, f"{case} {side}: {g}: {bad} of {want.size} bytes differ from the renderer with {stage} alone"
            seen.add(g)
        del narrow
    assert seen == set(OUTPUTS[side])

