"""Per-instance colour override on the MI355X (-m gpu): three rows of four overridden, through every kernel family,
against the oracle whose overridden rows draw recoloured clones (tests/color_oracle.py); the column written from
torch between steps; colours beside mixed lights and projections; hidden and spare rows; a renderer without the
column and a depth-only one; two shards; the headless binary.  Colour, visibility and segmask bit for bit, depth to
1 ulp (tests.util.assert_parity, unchanged).  In every scene at least half of the covered pixels must differ from the
image without overrides: a kernel that ignored the column would pass nothing here."""
import dataclasses
import subprocess

import numpy as np
import pytest

from madrona_renderer_amd import scenes
from tests import color_oracle as co
from tests import light_oracle as lo
from tests import projection_oracle as po
from tests.test_projection_gpu import CASES, _make
from tests.util import assert_parity, depth_ulps, fetch

pytestmark = pytest.mark.gpu

FLAT = (lambda: scenes.synthetic_scene(4096, width=256, height=256, render_mode="Raytracer"), None, "bvh", "flat", True)
FAMILIES = dict(CASES, flat=FLAT)
# views compared with the oracle (the CPU renders them): all, but a slice of the large batches
SLICE = {"flat": (0, 40), "group-fast": (0, 1000)}


def _with(desc, colors, lights=None, projections=None):
    d = dataclasses.replace(desc)
    d.instance_colors = colors
    if lights is not None:
        d.world_lights = list(lights)
    if projections is not None:
        d.camera_projections = list(projections)
    return d


def _cut(images, views):
    a, b = views
    return {k: v[a:b] for k, v in images.items() if isinstance(v, np.ndarray)}


def _check(r, ref, rt, views):
    got = _cut(fetch(r, visibility=not rt, raytracer=rt), views)
    assert_parity(got, {k: ref[k][views[0]:views[1]] for k in got})


def _assert_colours_decided_pixels(desc, ref, views, lights=None, projections=None):
    """`ref` against the oracle without overrides: at least half of the covered pixels change colour, nothing else
    changes."""
    a, b = views[0], min(views[1], views[0] + 50)
    plain = lo.render(desc, lights, projections, a, b, want_ids=True)
    assert co.changed_fraction(_cut(ref, (a, b)), _cut(plain, (a, b))) >= 0.5
    for k in ("tri_id", "segmask"):
        assert np.array_equal(plain[k][a:b], ref[k][a:b]), k
    assert np.array_equal(plain["depth"][a:b].view(np.uint32), ref["depth"][a:b].view(np.uint32))
    assert (ref["rgb"][a:b][..., 3][plain["tri_id"][a:b] >= 0] == 255).all()


@pytest.mark.parametrize("case", list(FAMILIES))
def test_overrides_match_the_oracle_in_every_family(native, case):
    build, variant, entry, bvh, rt = FAMILIES[case]
    base = build()
    colors = co.mixed(len(base.instances))
    plain = _make(base, visibility=not rt, variant=variant)
    r = _make(_with(base, colors), visibility=not rt, variant=variant)
    # the column never changes which kernel runs
    assert r.raster_entry() == entry == plain.raster_entry()
    assert r.bvh_launch() == plain.bvh_launch() and r.bvh_launch()["kernel"] == bvh
    if case == "bvh-tile-pairs":
        assert r.bvh_launch()["group_views"] == 2
    del plain
    assert np.array_equal(r.instance_color_tensor().to_torch().cpu().numpy(), co.expand(base, colors))
    views = SLICE.get(case, (0, base.num_views))
    ref = co.render(base, colors, view_begin=views[0], view_end=views[1], want_ids=True)
    _check(r, ref, rt, views)
    _assert_colours_decided_pixels(base, ref, views)


def test_the_column_is_mutable_between_steps(native):
    import torch
    base = scenes.synthetic_scene(512, with_wall=True)
    views = (0, base.num_views)
    r = _make(_with(base, True))
    assert r.raster_entry() == "group"
    t = r.instance_color_tensor().to_torch()
    assert t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == (3 * 512, 4) and int(t.count_nonzero()) == 0
    plain = lo.render(base, want_ids=True)
    _check(r, plain, False, views)                       # an all-zero column: the images without one
    rows = co.mixed(len(base.instances), seed=11)
    t.copy_(torch.from_numpy(rows).to(t.device))          # (the renderer's stream is torch's current one: the null stream)
    r.step()
    ref = co.render(base, rows, want_ids=True)
    _check(r, ref, False, views)
    _assert_colours_decided_pixels(base, ref, views)
    t[:, 3] = 0                                           # alpha alone decides: the colour bytes stay
    r.step()
    _check(r, plain, False, views)
    t.zero_()
    r.step()
    _check(r, plain, False, views)


@pytest.mark.parametrize("case", ["group-fast", "group", "bvh-tile", "bvh-tile-pairs", "flat"])
def test_colours_mixed_lights_and_mixed_projections_together(native, case):
    build, variant, entry, bvh, rt = FAMILIES[case]
    base = build()
    colors = co.mixed(len(base.instances), seed=3)
    lights = lo.mixed(base.num_worlds, shift=2)
    projs = po.mixed(len(base.cameras))
    r = _make(_with(base, colors, lights, projs), visibility=not rt, variant=variant)
    assert r.raster_entry() == entry and r.bvh_launch()["kernel"] == bvh
    views = {"flat": (0, 40), "group-fast": (0, 600), "bvh-tile-pairs": (0, 120)}.get(case, (0, base.num_views))
    ref = co.render(base, colors, lights, projs, view_begin=views[0], view_end=views[1], want_ids=True)
    _check(r, ref, rt, views)
    _assert_colours_decided_pixels(base, ref, views, lights, projs)


@pytest.mark.parametrize("tables", [False, True], ids=["uniform", "tables"])
def test_colours_through_the_plain_entry_at_16_slots(native, monkeypatch, tables):
    # both colour forms (over the uniform constants, over the tables) behind the plain entry of a 16-slot world (the
    # FAST entry switched off): two one-tile views
    monkeypatch.setenv("MRX_GROUP_FAST", "0")
    base = scenes.synthetic_scene(2)
    colors = co.mixed(len(base.instances))
    lights = lo.mixed(base.num_worlds, shift=2) if tables else None
    projs = po.mixed(len(base.cameras)) if tables else None
    r = _make(_with(base, colors, lights, projs))
    assert r.raster_entry() == "group"
    _check(r, co.render(base, colors, lights, projs, want_ids=True), False, (0, base.num_views))


def test_colours_beside_projections_alone_and_a_uniform_light(native):
    # projections differ, lights do not: the group kernels' table form with colours
    base = scenes.synthetic_scene(256, textured=True)
    colors = co.mixed(len(base.instances), seed=5)
    projs = po.mixed(len(base.cameras))
    light = [((0.0, 0.0, -1.0), 0.1, 0.9)] * base.num_worlds
    r = _make(_with(base, colors, light, projs))
    assert r.raster_entry() == "group-fast"
    ref = co.render(base, colors, light, projs, want_ids=True)
    _check(r, ref, False, (0, base.num_views))


def test_a_hidden_row_keeps_its_colour(native, oracle_mod):
    import torch
    base = scenes.synthetic_scene(64, with_wall=True)
    colors = co.mixed(len(base.instances))
    rows = co.expand(base, colors)
    r = _make(_with(base, colors))
    obj = r.instance_object_tensor().to_torch()
    hidden = [i for i in range(len(rows)) if rows[i, 3] and i % 5 == 0]
    assert hidden
    saved = obj[hidden].clone()
    obj[hidden] = -1 - torch.arange(len(hidden), dtype=obj.dtype, device=obj.device)
    r.step()
    fs = oracle_mod.FlatScene(base)
    fs.inst_obj[hidden] = -1
    ref = co.render_flat(fs, rows)
    assert not np.array_equal(ref["tri_id"], co.render(base, colors)["tri_id"])
    _check(r, ref, False, (0, base.num_views))
    obj[hidden] = saved                                   # shown again, in the colour that stayed with the row
    r.step()
    _check(r, co.render(base, colors, want_ids=True), False, (0, base.num_views))


def test_a_spare_row_has_a_colour_of_its_own(native, oracle_mod):
    import torch
    base = scenes.synthetic_scene(32, with_wall=True)
    base.max_instances_per_world = 4                      # three rows bound, one spare
    r = _make(_with(base, True))
    t = r.instance_color_tensor().to_torch()
    assert tuple(t.shape) == (4 * 32, 4) and int(t.count_nonzero()) == 0
    rows = co.mixed(4 * 32, seed=9)
    rows[3::4] = (250, 20, 200, 255)                      # the spare rows
    t.copy_(torch.from_numpy(rows).to(t.device))
    r.step()
    fs = oracle_mod.FlatScene(base)
    _check(r, co.render_flat(fs, rows), False, (0, 32))    # unbound: its colour shows nowhere
    spare = list(range(3, 4 * 32, 4))
    obj, pos = r.instance_object_tensor().to_torch(), r.instance_position_tensor().to_torch()
    obj[spare] = 0
    pos[spare] = torch.tensor([1.5, -2.0, 2.0], device=pos.device)
    r.refresh_objects()
    r.step()
    assert np.array_equal(t.cpu().numpy(), rows)           # refresh_objects keeps the column
    fs.inst_obj[spare] = 0
    fs.inst_pos[spare] = (1.5, -2.0, 2.0)
    fs.refresh_objects()
    ref = co.render_flat(fs, rows)
    _check(r, ref, False, (0, 32))
    new = ref["tri_id"] >= int(fs.obj_num_tris[[1, 0, 2]].sum())   # the spawned cubes' triangles: after the bound rows'
    assert new.any() and (ref["rgb"][new][:, 0] > ref["rgb"][new][:, 1]).all()


def test_off_means_off(native):
    base = scenes.synthetic_scene(256)
    off = _make(base)
    with pytest.raises(RuntimeError, match="MRX_FLAG_INSTANCE_COLORS"):
        off.instance_color_tensor()
    with pytest.raises(RuntimeError):
        off.segmask_tensor()                              # (what the other unavailable tensors raise)
    on = _make(_with(base, True))
    assert off.raster_entry() == on.raster_entry() == "group-fast" and off.bvh_launch() == on.bvh_launch()
    a, b = fetch(off), fetch(on)
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    # depth only: the column exists and is never read
    colors = co.mixed(len(base.instances))
    d_off = _make(base, visibility=False, outputs="Depth")
    d_on = _make(_with(base, colors), visibility=False, outputs="Depth")
    assert np.array_equal(d_on.instance_color_tensor().to_torch().cpu().numpy(), co.expand(base, colors))
    d_off.sync()
    d_on.sync()
    x, y = d_off.depth_tensor().to_torch().cpu().numpy(), d_on.depth_tensor().to_torch().cpu().numpy()
    assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    ref = lo.render(base, want_ids=False)["depth"]
    assert depth_ulps(y.reshape(ref.shape), ref) <= 1


def test_two_shards_hold_their_own_rows(native):
    base = scenes.synthetic_scene(301, with_wall=True)
    colors = co.mixed(len(base.instances))
    one = _make(_with(base, colors))
    r = _make(_with(base, colors), device_ids=[0, 0])
    assert r.num_shards == 2
    rows = co.expand(base, colors)
    whole = fetch(one)
    ref = co.render(base, colors, want_ids=True)
    r.sync()
    for sh in range(2):
        a, b = r.shard_first_world(sh), r.shard_first_world(sh + 1)
        assert np.array_equal(r.instance_color_tensor(shard=sh).to_torch().cpu().numpy(), rows[3 * a:3 * b])
        ids = r.visibility_tensor(shard=sh).to_torch().cpu().numpy()
        rgb = r.rgb_tensor(shard=sh).to_torch().cpu().numpy()
        assert np.array_equal(ids, whole["tri_id"][a:b]) and np.array_equal(rgb, whole["rgb"][a:b])
        assert np.array_equal(rgb, ref["rgb"][a:b])


def test_headless_instance_colors(native, tmp_path):
    from madrona_renderer_amd import build
    from tests.test_headless_gpu import _tiles
    exe = build.headless_path()
    args = ["16", "2", "rast", "64", "64"]
    for name, extra in (("plain", []), ("coloured", ["--instance-colors", "1"])):
        p = subprocess.run(["timeout", "-k", "5", "120", exe] + args + extra + ["--dump-last-frame", name], cwd=tmp_path,
                           capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
    plain = np.stack(_tiles(tmp_path / "plain.png", 16, 64, 64))
    got = np.stack(_tiles(tmp_path / "coloured.png", 16, 64, 64))
    assert np.array_equal(plain, po.render(scenes.synthetic_scene(16))["rgb"])
    covered = (plain[..., :3] != 0).any(axis=-1)
    assert ((got != plain).any(axis=-1) & covered).sum() >= 0.5 * covered.sum()
    assert np.array_equal(got[~covered], plain[~covered])
