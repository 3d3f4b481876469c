"""Per-instance material override on the MI355X (-m gpu): three rows of four overridden with materials of a table that
holds untextured and textured ones (PNG, non-power-of-two RGBA8 KTX2, BC7 KTX2), through every kernel family, against
the oracle whose overridden rows draw clones that name the material on every triangle (tests/material_oracle.py); the
column written from torch and through the setter between steps; materials beside colours, mixed lights and mixed
projections; hidden and spare rows; ids outside the table; a renderer without the column and a depth-only one; two
shards; the headless binary.  Colour, visibility and segmask bit for bit, depth to 1 ulp (tests.util.assert_parity,
unchanged).  In every scene at least 0.4 of the covered pixels must differ from the image without overrides, with
visibility, segmask and depth bits identical to it: a kernel that ignored the column would pass nothing here."""
import dataclasses
import subprocess

import numpy as np
import pytest

from madrona_renderer_amd import scenes
from tests import color_oracle as co
from tests import light_oracle as lo
from tests import material_oracle as mo
from tests import projection_oracle as po
from tests.test_projection_gpu import CASES, _make
from tests.util import assert_parity, depth_ulps, fetch

pytestmark = pytest.mark.gpu

FLAT = (lambda: scenes.synthetic_scene(4096, width=256, height=256, render_mode="Raytracer"), None, "bvh", "flat", True)
FAMILIES = dict(CASES, flat=FLAT)
# views compared with the oracle (the CPU renders them): all, but a slice of the large batches
SLICE = {"flat": (0, 40), "group-fast": (0, 1000), "bvh-tile-pairs": (0, 300)}
# the scenes that draw textured triangles themselves: no table makes their launches untextured
TEXTURED_SCENES = ("textured", "bvh-tile-rt")
FAMILY_TABLES = [(c, True) for c in FAMILIES] + [(c, False) for c in FAMILIES if c not in TEXTURED_SCENES]


def _with(desc, materials, colors=None, lights=None, projections=None):
    d = dataclasses.replace(desc)
    d.instance_materials = materials
    if colors is not None:
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


def _assert_materials_decided_pixels(desc, ref, views, lights=None, projections=None, colors=None, share=0.4):
    """`ref` against the oracle without material overrides: at least `share` of the covered pixels change colour,
    nothing else changes."""
    a, b = views[0], min(views[1], views[0] + 50)
    plain = (lo.render(desc, lights, projections, a, b, want_ids=True) if colors is None else
             co.render(desc, colors, lights, projections, view_begin=a, view_end=b, want_ids=True))
    changed = mo.changed_fraction(_cut(ref, (a, b)), _cut(plain, (a, b)))
    print("changed share of covered pixels: %.3f" % changed)
    assert changed >= share
    for k in ("tri_id", "segmask"):
        assert np.array_equal(plain[k][a:b], ref[k][a:b]), k
    assert np.array_equal(plain["depth"][a:b].view(np.uint32), ref["depth"][a:b].view(np.uint32))
    assert (ref["rgb"][a:b][..., 3][plain["tri_id"][a:b] >= 0] == 255).all()


@pytest.mark.parametrize("case,textured", FAMILY_TABLES)
def test_overrides_match_the_oracle_in_every_family(native, case, textured):
    build, variant, entry, bvh, rt = FAMILIES[case]
    base = mo.with_table(build(), textured=textured)
    nm = mo.num_materials(base)
    ids = mo.mixed(len(base.instances), nm)
    r = _make(_with(base, ids), visibility=not rt, variant=variant)
    assert r.raster_entry() == entry and r.bvh_launch()["kernel"] == bvh
    if textured:
        # some material of the table is textured: the textured instantiations, whatever the scene draws
        assert r.bvh_launch()["textured"] == 1
    else:
        # a table without a textured material: exactly the launches of a renderer without the column
        plain = _make(base, visibility=not rt, variant=variant)
        assert r.raster_entry() == plain.raster_entry() and r.bvh_launch() == plain.bvh_launch()
        assert r.bvh_launch()["textured"] == 0
        if case == "bvh-tile-pairs":
            assert r.bvh_launch()["group_views"] == 2
        del plain
    assert np.array_equal(r.instance_material_tensor().to_torch().cpu().numpy(), mo.expand(base, ids))
    views = SLICE.get(case, (0, base.num_views))
    if not textured:
        views = (views[0], min(views[1], views[0] + 200))
    ref = mo.render(base, ids, view_begin=views[0], view_end=views[1], want_ids=True)
    _check(r, ref, rt, views)
    _assert_materials_decided_pixels(base, ref, views)


def test_the_column_is_mutable_between_steps(native):
    import torch
    base = mo.with_table(scenes.synthetic_scene(512, with_wall=True))
    nm = mo.num_materials(base)
    views = (0, base.num_views)
    r = _make(_with(base, True))
    assert r.raster_entry() == "group"
    t = r.instance_material_tensor().to_torch()
    assert t.is_cuda and t.dtype == torch.int32 and tuple(t.shape) == (3 * 512,) and bool((t == -1).all())
    plain = lo.render(base, want_ids=True)
    _check(r, plain, False, views)                       # a column of -1: the images without one
    rows = mo.mixed(len(base.instances), nm, seed=5)
    t.copy_(torch.from_numpy(rows).to(t.device))          # (the renderer's stream is torch's current one: the null stream)
    r.step()
    ref = mo.render(base, rows, want_ids=True)
    _check(r, ref, False, views)
    _assert_materials_decided_pixels(base, ref, views)
    t[::2] = -1                                           # half of the rows back to their own materials
    rows2 = rows.copy()
    rows2[::2] = -1
    r.step()
    _check(r, mo.render(base, rows2, want_ids=True), False, views)
    t.fill_(-1)
    r.step()
    _check(r, plain, False, views)


def test_the_setter_is_stream_ordered_and_reads_back(native):
    base = mo.with_table(scenes.synthetic_scene(2048))
    nm = mo.num_materials(base)
    views = (0, 600)
    first = mo.mixed(len(base.instances), nm, seed=2)
    second = mo.mixed(len(base.instances), nm, seed=3)
    assert (first != second).mean() > 0.3
    r = _make(_with(base, first))
    assert r.raster_entry() == "group-fast"
    assert np.array_equal(r.instance_materials(), mo.expand(base, first))
    ref_first = mo.render(base, first, view_begin=0, view_end=600, want_ids=True)
    _check(r, ref_first, False, views)                    # the first frame already shows the initial ids
    r.render()                                            # enqueued ahead of the setter: it keeps the old ids
    r.set_instance_materials(second)
    _check(r, ref_first, False, views)
    assert np.array_equal(r.instance_materials(), second)                 # the round trip through the C ABI
    assert np.array_equal(r.instance_material_tensor().to_torch().cpu().numpy(), second)
    r.step()
    ref_second = mo.render(base, second, view_begin=0, view_end=600, want_ids=True)
    assert not np.array_equal(ref_first["rgb"], ref_second["rgb"])
    _check(r, ref_second, False, views)
    # a sub-range, any int32
    part = np.array([-7, nm, 2 ** 31 - 1, -2 ** 31, nm - 1], np.int32)
    r.set_instance_materials(part, first_row=4)
    third = second.copy()
    third[4:9] = part
    assert np.array_equal(r.instance_materials(), third)
    r.step()
    _check(r, mo.render(base, third, view_begin=0, view_end=600, want_ids=True), False, views)
    with pytest.raises(ValueError):
        r.set_instance_materials(np.zeros(3, np.int32), first_row=len(third) - 2)


@pytest.mark.parametrize("case", ["group-fast", "group", "chunked", "bvh-tile", "bvh-tile-pairs", "flat"])
def test_materials_colours_mixed_lights_and_mixed_projections_together(native, case):
    build, variant, entry, bvh, rt = FAMILIES[case]
    base = mo.with_table(build())
    ids = mo.mixed(len(base.instances), mo.num_materials(base), seed=4)
    # (rolled by two rows: rows 0::4 and 2::4 carry both overrides, 1::4 a colour alone, 3::4 a material alone)
    colors = np.roll(co.mixed(len(base.instances), seed=3), 2, axis=0)
    lights = lo.mixed(base.num_worlds, shift=2)
    projs = po.mixed(len(base.cameras))
    r = _make(_with(base, ids, colors, lights, projs), visibility=not rt, variant=variant)
    assert r.raster_entry() == entry and r.bvh_launch()["kernel"] == bvh
    views = {"flat": (0, 40), "group-fast": (0, 600), "bvh-tile-pairs": (0, 120)}.get(case, (0, base.num_views))
    ref = mo.render(base, ids, colors, lights, projs, view_begin=views[0], view_end=views[1], want_ids=True)
    _check(r, ref, rt, views)
    # the colours decide pixels on top of the materials, and the materials decide pixels under the colours (a row of
    # both keeps the colour and takes the material's texture; rows 3::4 take the whole material)
    a, b = views[0], min(views[1], views[0] + 50)
    only = mo.render(base, ids, None, lights, projs, view_begin=a, view_end=b, want_ids=True)
    assert mo.changed_fraction(_cut(ref, (a, b)), _cut(only, (a, b))) >= 0.5
    _assert_materials_decided_pixels(base, ref, views, lights, projs, colors, share=0.1)


@pytest.mark.parametrize("tables", [False, True], ids=["uniform", "tables"])
def test_materials_through_the_plain_entry_at_16_slots(native, monkeypatch, tables):
    # both material forms (over the uniform constants, over the tables and beside colours) behind the plain entry of a
    # 16-slot world (the FAST entry switched off): two one-tile views
    monkeypatch.setenv("MRX_GROUP_FAST", "0")
    base = mo.with_table(scenes.synthetic_scene(2))
    ids = mo.mixed(len(base.instances), mo.num_materials(base))
    colors = np.roll(co.mixed(len(base.instances), seed=3), 2, axis=0) if tables else None
    lights = lo.mixed(base.num_worlds, shift=2) if tables else None
    projs = po.mixed(len(base.cameras)) if tables else None
    r = _make(_with(base, ids, colors, lights, projs))
    assert r.raster_entry() == "group"
    _check(r, mo.render(base, ids, colors, lights, projs, want_ids=True), False, (0, base.num_views))


def test_materials_alone_over_uniform_tables_and_beside_colours(native):
    # no lights, no projections: the group kernels' uniform material form, with and without a colour column
    base = mo.with_table(scenes.synthetic_scene(256, textured=True))
    ids = mo.mixed(len(base.instances), mo.num_materials(base), seed=6)
    colors = co.mixed(len(base.instances), seed=5)
    for cols in (None, colors):
        r = _make(_with(base, ids, cols))
        assert r.raster_entry() == "group-fast"
        _check(r, mo.render(base, ids, cols, want_ids=True), False, (0, base.num_views))


def test_a_hidden_row_keeps_its_material(native, oracle_mod):
    import torch
    base = mo.with_table(scenes.synthetic_scene(64, with_wall=True))
    ids = mo.mixed(len(base.instances), mo.num_materials(base))
    rows = mo.expand(base, ids)
    r = _make(_with(base, ids))
    obj = r.instance_object_tensor().to_torch()
    hidden = [i for i in range(len(rows)) if rows[i] >= 0 and i % 5 == 0]
    assert hidden
    saved = obj[hidden].clone()
    obj[hidden] = -1 - torch.arange(len(hidden), dtype=obj.dtype, device=obj.device)
    r.step()
    fs = oracle_mod.FlatScene(base)
    fs.inst_obj[hidden] = -1
    ref = mo.render_flat(fs, rows)
    assert not np.array_equal(ref["tri_id"], mo.render(base, ids)["tri_id"])
    _check(r, ref, False, (0, base.num_views))
    obj[hidden] = saved                                   # shown again, in the material that stayed with the row
    r.step()
    _check(r, mo.render(base, ids, want_ids=True), False, (0, base.num_views))


def test_a_spare_row_has_a_material_of_its_own(native, oracle_mod):
    import torch
    base = mo.with_table(scenes.synthetic_scene(32, with_wall=True))
    base.max_instances_per_world = 4                      # three rows bound, one spare
    nm = mo.num_materials(base)
    r = _make(_with(base, True))
    t = r.instance_material_tensor().to_torch()
    assert tuple(t.shape) == (4 * 32,) and bool((t == -1).all())
    rows = mo.mixed(4 * 32, nm, seed=9)
    rows[3::4] = nm - 4                                   # the spare rows: the table's red
    t.copy_(torch.from_numpy(rows).to(t.device))
    r.step()
    fs = oracle_mod.FlatScene(base)
    _check(r, mo.render_flat(fs, rows), False, (0, 32))    # unbound: its material shows nowhere
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
    ref = mo.render_flat(fs, rows)
    _check(r, ref, False, (0, 32))
    new = ref["tri_id"] >= int(fs.obj_num_tris[[1, 0, 2]].sum())   # the spawned cubes' triangles: after the bound rows'
    assert new.any() and (ref["rgb"][new][:, 1] == 0).all() and (ref["rgb"][new][:, 0] > 0).all()


@pytest.mark.parametrize("case", ["textured", "chunked", "bvh-tile", "flat"])
def test_ids_outside_the_table_render_as_no_override(native, case):
    build, variant, entry, bvh, rt = FAMILIES[case]
    base = mo.with_table(build())
    nm = mo.num_materials(base)
    n = len(base.instances)
    outside = np.resize(np.array([-7, nm, 2 ** 31 - 1], np.int64), n).astype(np.int32)
    r = _make(_with(base, outside), visibility=not rt, variant=variant)
    assert r.raster_entry() == entry
    views = {"flat": (0, 40)}.get(case, (0, base.num_views))
    plain = lo.render(base, None, None, views[0], views[1], want_ids=True)
    _check(r, plain, rt, views)
    got = _cut(fetch(r, visibility=not rt, raytracer=rt), views)
    assert np.array_equal(got["rgb"], plain["rgb"][views[0]:views[1]])     # bit-equal to the plain image


def test_off_means_off(native):
    base = mo.with_table(scenes.synthetic_scene(256))
    off = _make(base)
    with pytest.raises(RuntimeError, match="MRX_FLAG_INSTANCE_MATERIALS"):
        off.instance_material_tensor()
    with pytest.raises(RuntimeError, match="MRX_FLAG_INSTANCE_MATERIALS"):
        off.set_instance_materials(np.zeros(4, np.int32))
    assert off.raster_entry() == "group-fast" and off.bvh_launch()["textured"] == 0
    _check(off, lo.render(base, want_ids=True), False, (0, base.num_views))
    # a table without a textured material: the column costs a launch form, not a kernel family or a launch shape
    bare = mo.with_table(scenes.synthetic_scene(256), textured=False)
    b_off, b_on = _make(bare), _make(_with(bare, True))
    assert b_off.raster_entry() == b_on.raster_entry() == "group-fast" and b_off.bvh_launch() == b_on.bvh_launch()
    a, b = fetch(b_off), fetch(b_on)
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    # depth only: the column exists and is never read -- the launches of a renderer without one, textured table or not
    ids = mo.mixed(len(base.instances), mo.num_materials(base))
    d_off = _make(base, visibility=False, outputs="Depth")
    d_on = _make(_with(base, ids), visibility=False, outputs="Depth")
    assert d_off.raster_entry() == d_on.raster_entry() and d_off.bvh_launch() == d_on.bvh_launch()
    assert np.array_equal(d_on.instance_material_tensor().to_torch().cpu().numpy(), mo.expand(base, ids))
    d_off.sync()
    d_on.sync()
    x, y = d_off.depth_tensor().to_torch().cpu().numpy(), d_on.depth_tensor().to_torch().cpu().numpy()
    assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    ref = lo.render(base, want_ids=False)["depth"]
    assert depth_ulps(y.reshape(ref.shape), ref) <= 1


def test_two_shards_hold_their_own_rows(native):
    base = mo.with_table(scenes.synthetic_scene(301, with_wall=True))
    nm = mo.num_materials(base)
    ids = mo.mixed(len(base.instances), nm)
    one = _make(_with(base, ids))
    r = _make(_with(base, ids), device_ids=[0, 0])
    assert r.num_shards == 2
    whole = fetch(one)
    ref = mo.render(base, ids, want_ids=True)
    r.sync()

    def per_shard(rows, whole, ref):
        for sh in range(2):
            a, b = r.shard_first_world(sh), r.shard_first_world(sh + 1)
            assert np.array_equal(r.instance_material_tensor(shard=sh).to_torch().cpu().numpy(), rows[3 * a:3 * b])
            vis = r.visibility_tensor(shard=sh).to_torch().cpu().numpy()
            rgb = r.rgb_tensor(shard=sh).to_torch().cpu().numpy()
            assert np.array_equal(vis, whole["tri_id"][a:b]) and np.array_equal(rgb, whole["rgb"][a:b])
            assert np.array_equal(rgb, ref["rgb"][a:b])

    per_shard(mo.expand(base, ids), whole, ref)
    assert np.array_equal(r.instance_materials(), ids)
    # the setter splits a range that spans the shards at their world boundary
    cut = 3 * r.shard_first_world(1)
    again = mo.mixed(len(base.instances), nm, seed=8)
    part = again[cut - 50:cut + 70]
    for x in (one, r):
        x.set_instance_materials(part, first_row=cut - 50)
        x.step()
    now = ids.copy()
    now[cut - 50:cut + 70] = part
    assert np.array_equal(r.instance_materials(), now) and np.array_equal(one.instance_materials(), now)
    r.sync()
    per_shard(now, fetch(one), mo.render(base, now, want_ids=True))


def test_headless_instance_materials(native, tmp_path):
    from madrona_renderer_amd import build
    from tests.test_headless_gpu import _tiles
    exe = build.headless_path()
    args = ["16", "2", "rast", "64", "64"]
    for name, extra in (("plain", []), ("overridden", ["--instance-materials", "3"])):
        p = subprocess.run(["timeout", "-k", "5", "120", exe] + args + extra + ["--dump-last-frame", name], cwd=tmp_path,
                           capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
    plain = np.stack(_tiles(tmp_path / "plain.png", 16, 64, 64))
    got = np.stack(_tiles(tmp_path / "overridden.png", 16, 64, 64))
    desc = scenes.synthetic_scene(16)
    assert np.array_equal(plain, po.render(desc)["rgb"])
    # the ids the binary draws: splitmix64(splitmix64(SEED) ^ row) % materials, rows 1::4 left at -1
    nm = len(desc.materials)
    base = scenes._splitmix64(np.uint64(3))
    ids = (scenes._splitmix64(base ^ np.arange(len(desc.instances), dtype=np.uint64)) % np.uint64(nm)).astype(np.int32)
    ids[1::4] = -1
    assert np.array_equal(got, mo.render(desc, ids)["rgb"])
    covered = (plain[..., :3] != 0).any(axis=-1)
    assert ((got != plain).any(axis=-1) & covered).sum() >= 0.1 * covered.sum()
    assert np.array_equal(got[~covered], plain[~covered])
