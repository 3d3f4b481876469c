"""Parity at the ends of the view-size range, 1 to 16384 pixels a side (-m gpu).

tests/view_shapes.CASES takes thirty-one view shapes -- below a lane's four pixels, an 8-row strip, a 32 x 8 region and a
64 x 64 tile; strips that reach x or y 16383; views of up to 1024 tiles -- through every kernel family: the group
kernel's FAST and plain entries, the brute and the chunked kernel, the BVH tile kernel at its three tile shapes and
the BVH flat kernel, under the defaults, a shared vfov (the uniform argument form) and two vfovs a case (the per-view
table).  Every case asserts the entry (raster_entry), the BVH kernel and its launch shape (bvh_launch) and the form
(kernel_form) it reached, and compares every view with the oracle under the same projections as
tests.util.assert_parity has it: rgb and ids bit for bit, depth within 1 ulp beside rtol 1e-4.
tests/test_view_shapes_cpu.py holds that no reference is vacuous.

The post-render stages run on the renderer's own frames at 16384 x 8 (the vector forms), 16383 x 3 (the scalar ones),
2 x 8191, 7 x 5 and Raytracer 7 and 1024: normals, labels, positions in both frames, boxes and a packed observation
against the NumPy restatements their own tests use; a supersampled renderer whose sample image is 16384 pixels wide
(s = 2, 3, 4) against the oracle's sample image resolved; flow, the point cloud (N = 100 and 1024) and cast shadows
attached at 16384 x 8 and 16383 x 3.

135 cases: 118 of tests/view_shapes.CASES, 6 + 3 of the stages, 8 of the attached stages.  On one MI355X the longest is
the first, group-fast at 1 x 1, at 1.8 s with the library's load; then chunked at 16384 x 65 at 1.1 s (a 482-triangle reference of
2 M pixels); every other case stays under 0.6 s, the module under 30 s.

Findings.  No case fails: every shape renders the oracle's bytes through every family, and no kernel or launcher
changed.  Two things the cases were shaped by:
  - `tileSetup` (raster.hip: the brute and the chunked kernel) decodes `tile % tilesFast`, as the group kernel's S1 and
    the BVH kernels do; on a view of one tile row the tile index never reaches tilesFast, so an error in the modulus is
    invisible there.  16384 x 65 -- 256 tile columns and a second tile row -- is in the table for that, beside the
    issue's strips, through every family that takes several tiles.
  - `walkSmallRows` (bvh.hip) keeps an absolute pixel x in the low 16 bits of `packedBox`; x < 16384 = 2^14 for every size
    mrx_create accepts, so the field has two bits to spare and 16384 x 8 / 16383 x 3 (x up to 16383, every bit of the 14
    set) are the largest values it can be given.
"""
import dataclasses

import numpy as np
import pytest

from madrona_renderer_amd import scenes
from tests import box_oracle as bx
from tests import label_oracle as lb
from tests import normal_oracle as no
from tests import observation_oracle as ob
from tests import projection_oracle as po
from tests import view_shapes as vs
from tests.test_box_gpu import _some_labels
from tests.test_cloud_gpu import _assert_same as cloud_same
from tests.test_cloud_gpu import _attach as cloud_attach
from tests.test_cloud_gpu import _expected as cloud_expected
from tests.test_cloud_gpu import _got as cloud_got
from tests.test_flow_gpu import _assert_bits as flow_bits
from tests.test_flow_gpu import _consts as flow_consts
from tests.test_flow_gpu import _expected as flow_expected
from tests.test_flow_gpu import _state as flow_state
from tests.test_flow_gpu import _tables as flow_tables
from tests.test_observation_gpu import RANGE, _bits, _opt, _want
from tests.test_observation_gpu import _assert_bits as observation_bits
from tests.test_position_gpu import _assert_bits as position_bits
from tests.test_position_gpu import _reference as position_reference
from tests.test_projection_gpu import _make
from tests.test_shadow_cpu import CUBE_AT, LIGHT, cube_scene
from tests.test_shadow_gpu import _attach as shadow_attach
from tests.test_shadow_gpu import _expected as shadow_expected
from tests.test_shadow_gpu import _same as shadow_same
from tests.test_supersample_gpu import _reference as resolved_reference
from tests.util import assert_parity, fetch

pytestmark = pytest.mark.gpu

KNOBS = ("MRX_DEBUG_SLOTS", "MRX_GROUP_VIEWS", "MRX_GROUP_TILES", "MRX_GROUP_FAST", "MRX_BVH_FLAT", "MRX_BVH_TILE",
         "MRX_BVH_CLASSIFY", "MRX_BVH_GROUP_VIEWS", "MRX_BVH_GROUP_TILES", "MRX_BVH_PASS_INST", "MRX_BVH_MIN_TRIS")


def _np(t):
    return t.to_torch().cpu().numpy()


def _knobs(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        assert k in KNOBS, k
        monkeypatch.setenv(k, v)


# ---- every shape through every family ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", vs.CASES, ids=[c.name for c in vs.CASES])
def test_every_view_matches_the_oracle(native, oracle_mod, monkeypatch, case):
    _knobs(monkeypatch, case.env)
    desc = vs.desc_of(case)
    rt = case.shape.mode == vs.RT
    r = _make(desc, visibility=not rt, variant=case.variant)
    entry, bvh = vs.ENTRY[case.family]
    launch = r.bvh_launch()
    assert r.raster_entry() == entry and launch["kernel"] == bvh, (case.name, r.raster_entry(), launch["kernel"])
    assert r.kernel_form()["form"] == case.form, (case.name, r.kernel_form())
    if bvh != "none":
        assert launch["textured"] == case.textured, (case.name, launch)
    for k, v in case.launch.items():
        assert launch[k] == v, (case.name, k, launch[k])
    got = fetch(r, visibility=not rt, raytracer=rt)
    ref = vs.reference(case)
    assert got["rgb"].shape == (desc.num_views,) + vs.storage(case.shape) + (4,), case.name
    assert_parity(got, {k: ref[k] for k in got})


# ---- the stages on the renderer's own frames --------------------------------------------------------------------------------
STAGE_SHAPES = (vs.SHAPE["16384x8"], vs.SHAPE["16383x3"], vs.SHAPE["2x8191"], vs.SHAPE["7x5"],
                vs.Shape("rt7", 7, 7, vs.RT, None), vs.SHAPE["rt1024"])
BOX_LABELS = 8


def _stage_desc(shape, **kw):
    """the textured wall scene of the shape (a strip's under two vfovs), every row labelled"""
    base = vs.scene_desc(shape, "wall", True, "per-view" if shape.vfov is not None else None)
    return dataclasses.replace(base, normals=True, instance_labels=_some_labels(len(base.instances)), **kw)


def _stage_reference(desc, oracle_mod):
    fs = oracle_mod.FlatScene(desc)
    ref = po.render(desc, None, 0, desc.num_views, want_ids=True)
    ref = {k: ref[k] for k in ("rgb", "depth", "tri_id")}
    ref["segmask"] = lb.segmask(fs, lb.expand(desc), ref["tri_id"])
    ref["normal"] = no.normals(fs, ref["tri_id"])
    return ref


@pytest.mark.parametrize("shape", STAGE_SHAPES, ids=[s.name for s in STAGE_SHAPES])
def test_the_stages_on_the_renderer_s_own_frames(native, oracle_mod, monkeypatch, shape):
    _knobs(monkeypatch, {})
    i = STAGE_SHAPES.index(shape)
    rt = shape.mode == vs.RT
    frame = ("world", "view")[i % 2]
    opt = (_opt("rgbd", "float16", 2, RANGE), _opt("yd", "uint8", 1, RANGE))[i % 2]
    desc = _stage_desc(shape, positions=frame, boxes=BOX_LABELS, observations=opt)
    r = _make(desc, visibility=False)
    assert r.raster_entry() in (("group-fast", "group") if vs.one_tile(shape) else ("group",)) and \
        r.kernel_form()["form"] in ("L", "LN")
    r.sync()
    ref = _stage_reference(desc, oracle_mod)
    got = {"rgb": _np(r.rgb_tensor()), "segmask": _np(r.segmask_tensor())}
    got["depth"] = _np(r.depth_tensor()).reshape(got["segmask"].shape)
    assert_parity(got, ref)
    normal = _np(r.normal_tensor())
    assert int((normal != ref["normal"]).any(axis=-1).sum()) == 0
    hit = got["depth"] != 0
    assert hit.any() and (~hit).any() and len(np.unique(got["segmask"])) >= 3
    # positions, boxes and the observation of what the renderer holds
    position = _np(r.position_tensor())
    position_bits(position, position_reference(r, desc, 1, frame, rt), shape.name)
    assert np.array_equal(position[..., 3], hit.astype(np.float32))
    boxes = _np(r.box_tensor())
    assert boxes.shape == (desc.num_views, BOX_LABELS, 5) and np.array_equal(boxes, bx.boxes(got["segmask"], BOX_LABELS, rt))
    assert (boxes[..., 4] > 0).any()
    if shape in vs.STRIPS:                                              # a box reaches the last pixel of the long side
        assert int(boxes[..., 2:4].max()) == max(vs.storage(shape)) - 1
    observation_bits(_bits(r.observation_tensor()), ob.Stack(opt["stack"]).push(_want(got["rgb"], _np(r.depth_tensor()), opt, rt)),
                     shape.name)


SUPERSAMPLED = ((2, vs.Shape("8192x4", 8192, 4, vs.RAST, 0.1)), (3, vs.Shape("5461x1", 5461, 1, vs.RAST, 0.0375)),
                (4, vs.Shape("4096x2", 4096, 2, vs.RAST, 0.1)))


@pytest.mark.parametrize("s,shape", SUPERSAMPLED, ids=["s%d-%s" % (s, shape.name) for s, shape in SUPERSAMPLED])
def test_a_sample_image_16384_pixels_wide_resolves_to_the_oracle_s(native, oracle_mod, monkeypatch, s, shape):
    _knobs(monkeypatch, {})
    assert 16384 - s < s * shape.width <= 16384
    base = _stage_desc(shape)
    r = _make(dataclasses.replace(base, supersample=s), visibility=False)
    assert r.supersample == s and r.raster_entry() == "group"
    assert tuple(r.sample_tensor("rgb").shape) == (base.num_views, s * shape.height, s * shape.width, 4)
    r.sync()
    ref = resolved_reference(base, s, projections=po.view_projections(base), normals=True, labels=True)
    got = {"rgb": _np(r.rgb_tensor()), "segmask": _np(r.segmask_tensor())}
    got["depth"] = _np(r.depth_tensor()).reshape(got["segmask"].shape)
    assert_parity(got, {k: ref[k] for k in got})
    assert int((_np(r.normal_tensor()) != ref["normal"]).any(axis=-1).sum()) == 0
    assert (got["depth"] != 0).any() and (got["depth"] == 0).any()


# ---- the attached stages ------------------------------------------------------------------------------------------------------
ATTACHED = (vs.SHAPE["16384x8"], vs.SHAPE["16383x3"])


@pytest.mark.parametrize("shape", ATTACHED, ids=[s.name for s in ATTACHED])
def test_flow_at_the_strips(native, oracle_mod, monkeypatch, shape):
    import torch
    _knobs(monkeypatch, {})
    base = dataclasses.replace(vs.scene_desc(shape, "wall", True, "per-view"), normals=True)
    r = _make(dataclasses.replace(base, flow=True), visibility=False)
    assert r.flows is True and r.raster_entry() == "group"
    tables = flow_tables(oracle_mod.FlatScene(base))
    assert tuple(r.flow_tensor().shape) == (base.num_views, shape.height, shape.width, 4)
    r.sync()
    flow_bits(_np(r.flow_tensor()), flow_expected(r, base, tables, 1, False, flow_state(r), flow_consts(r, base, 1, False)),
              shape.name + " first")
    # motion between two steps: the rows and the cameras by a little, and the vfovs of the views
    prev, prev_consts = flow_state(r), flow_consts(r, base, 1, False)
    rng = np.random.default_rng(shape.width)
    for getter, scale in (("instance_position_tensor", 0.05), ("camera_position_tensor", 0.02)):
        t = getattr(r, getter)().to_torch()
        t.copy_(torch.from_numpy((t.cpu().numpy() + rng.uniform(-scale, scale, tuple(t.shape))).astype(np.float32)).to(t.device))
    r.set_camera_projection([shape.vfov * (0.95, 1.05)[v % 2] for v in range(base.num_views)])
    r.step()
    r.sync()
    moved = _np(r.flow_tensor())
    flow_bits(moved, flow_expected(r, base, tables, 1, False, prev, prev_consts), shape.name + " moved")
    valid = moved[..., 3] == 1
    assert valid.any() and (~valid).any() and (moved[valid][:, :3] != 0).any()
    assert valid[:, :, -64:].any()                                       # the far end of the long side


@pytest.mark.parametrize("n", [100, 1024])
@pytest.mark.parametrize("shape", ATTACHED, ids=[s.name for s in ATTACHED])
def test_the_point_cloud_at_the_strips(native, monkeypatch, shape, n):
    _knobs(monkeypatch, {})
    base = vs.scene_desc(shape, "wall", True, "per-view")
    r = _make(base, visibility=False)
    frame = "world" if n == 100 else "view"
    c = cloud_attach(r, n, frame, None, None)
    assert tuple(c.points_tensor().shape) == (base.num_views, n, 4)
    r.step()
    r.sync()
    got = cloud_got(c)
    cloud_same(got, cloud_expected(r, base, 1, frame, False, n), "%s N=%d" % (shape.name, n))
    assert (got[2] > n).all()                                          # more valid pixels than points: every slot is filled
    assert int(got[1].max()) > shape.width * shape.height - 2 * (shape.width * shape.height // n)


@pytest.mark.parametrize("shape", ATTACHED, ids=[s.name for s in ATTACHED])
def test_cast_shadows_at_the_strips(native, oracle_mod, monkeypatch, shape):
    _knobs(monkeypatch, {})
    desc = cube_scene(2, cams=2, width=shape.width, height=shape.height, vary=True)
    # (the strip is the middle of cube_scene's image: aimed at the middle of the cube's shadow on the floor)
    shadow = (CUBE_AT[0] - CUBE_AT[2] * LIGHT[0][0] / LIGHT[0][2], CUBE_AT[1] - CUBE_AT[2] * LIGHT[0][1] / LIGHT[0][2], 0.0)
    desc.cameras = [(eye, scenes.look_at(eye, shadow)) for eye, _ in desc.cameras]
    desc.camera_projections = [(shape.vfov * (1.0, 1.1)[c % 2], None) for c in range(len(desc.cameras))]
    desc = dataclasses.replace(desc, normals=True, positions="world")
    fs = oracle_mod.FlatScene(desc)
    r = _make(desc)
    sh = shadow_attach(r, apply=False)
    assert tuple(sh.mask_tensor().shape) == (desc.num_views, shape.height, shape.width)
    r.step()
    r.sync()
    want, st = shadow_expected(r, desc, fs)
    shadow_same(sh.mask_tensor().cpu().numpy(), want, shape.name)
    hit = st["depth"] > 0
    dark, lit = float((want[hit] == 0).mean()), float((want[hit] == 255).mean())
    print("%s: occluded %.1f %% of the hit pixels, lit %.1f %%" % (shape.name, 100 * dark, 100 * lit))
    assert dark > 0.02 and lit > 0.02
