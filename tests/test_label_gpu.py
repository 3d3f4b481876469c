"""Per-instance labels on the MI355X (-m gpu): a label column through every kernel family, in
both render modes, against tests/label_oracle.py -- the labels scattered through the C oracle's own tri_id image --
bit for bit, with rgb and depth still at parity with the oracle; the column written from torch and through the setter
between steps; the default column; values stored as they are; labels beside mixed projections, lights, colours,
materials and normals and in depth-only and rgb-only renderers, every other output byte-identical to the same renderer
without labels; poses, cameras, hidden rows, spare rows bound by refresh_objects(); a renderer without the column;
labels beside visibility ids; two shards; the headless binary.  In every family at least 0.4 of the covered pixels
must differ from the object-id segmask and some covered pixel must belong to a sentinel row: a kernel that ignored the
column, or the sentinel, passes nothing here."""
import dataclasses
import subprocess

import numpy as np
import pytest

from madrona_renderer_amd import scenes
from tests import color_oracle as co
from tests import label_oracle as lb
from tests import light_oracle as lo
from tests import material_oracle as mo
from tests import normal_oracle as no
from tests import projection_oracle as po
from tests.test_material_gpu import FAMILIES, SLICE
from tests.test_projection_gpu import _make
from tests.util import assert_parity, depth_ulps

pytestmark = pytest.mark.gpu

# The share of covered pixels owned by labelled rows under lb.mixed, measured on the CPU oracle over the compared views
# of each scene (printed by the tests): group-fast 0.99, group 0.75, textured 0.99, chunked 0.74, brute 0.75, bvh-tile
# and bvh-tile-pairs 0.75, bvh-tile-rt 0.77, flat 0.99 -- every scene shows labelled and sentinel rows; the bound is 0.4.


def _with(desc, labels, **more):
    d = dataclasses.replace(desc)
    d.instance_labels = labels
    for k, v in more.items():
        setattr(d, k, v)
    return d


def _views(case, desc):
    a, b = SLICE.get(case, (0, desc.num_views))
    return a, min(b, desc.num_views)


def _fetch(r, views, outputs=None):
    """The slice of rgb, depth and the segmask, oracle layout."""
    r.sync()
    a, b = views
    out = {"segmask": r.segmask_tensor().to_torch()[a:b].cpu().numpy()}
    if outputs != "Depth":
        out["rgb"] = r.rgb_tensor().to_torch()[a:b].cpu().numpy()
    if outputs != "RGB":
        d = r.depth_tensor().to_torch()[a:b].cpu().numpy()
        out["depth"] = d.reshape(d.shape[0], d.shape[1], d.shape[2])
    return out


def _expected(fs, col, ref, views):
    """`ref` (the oracle's render of views `views`) with its segmask replaced by the labelled one."""
    a, b = views
    out = {k: ref[k][a:b] for k in ("rgb", "depth", "tri_id")}
    out["segmask"] = lb.segmask(fs, col, ref["tri_id"], a, b)
    return out


def _check(r, fs, col, ref, views):
    got = _fetch(r, views)
    want = _expected(fs, col, ref, views)
    assert got["segmask"].dtype == np.int32 and got["segmask"].shape == want["segmask"].shape
    assert_parity(got, want)
    return got, want


def _assert_labels_decide(fs, col, ref, views, want, share=0.4):
    a, b = views
    tri = ref["tri_id"][a:b]
    covered = tri >= 0
    changed = ((want["segmask"] != ref["segmask"][a:b]) & covered).sum() / max(int(covered.sum()), 1)
    owner = lb.owner_rows(fs, ref["tri_id"], a, b)
    sentinel = (np.asarray(col)[owner[covered]] == lb.SENTINEL).sum()
    print("labelled share of covered pixels: %.3f; pixels of sentinel rows: %d" % (changed, sentinel))
    assert changed >= share
    assert sentinel >= 1
    assert (want["segmask"][~covered] == -1).all()


@pytest.mark.parametrize("case", list(FAMILIES))
def test_labels_match_the_oracle_in_every_family(native, oracle_mod, case):
    build, variant, entry, bvh, rt = FAMILIES[case]
    base = build()
    labels = lb.mixed(len(base.instances))
    r = _make(_with(base, labels), visibility=False, variant=variant)
    plain = _make(base, visibility=False, variant=variant)
    assert r.raster_entry() == entry and r.bvh_launch()["kernel"] == bvh
    assert plain.raster_entry() == entry and r.bvh_launch() == plain.bvh_launch()
    if case == "bvh-tile-pairs":
        assert r.bvh_launch()["group_views"] == 2
    col = lb.expand(base, labels)
    assert np.array_equal(r.instance_label_tensor().to_torch().cpu().numpy(), col)
    views = _views(case, base)
    fs = oracle_mod.FlatScene(base)
    ref = lo.render(base, None, None, views[0], views[1], want_ids=True)
    got, want = _check(r, fs, col, ref, views)
    _assert_labels_decide(fs, col, ref, views, want)
    # the whole tensor: the background is -1 exactly where nothing is hit; rgb and depth are the plain renderer's bytes
    import torch
    t = r.segmask_tensor().to_torch()
    depth = r.depth_tensor().to_torch()
    assert t.dtype == torch.int32 and tuple(t.shape) == tuple(depth.shape[:3])
    hit = depth.reshape(t.shape) != 0
    assert bool((t[~hit] == -1).all())
    vals = torch.unique(t[hit]).cpu().numpy()
    nobj = len(fs.obj_first_tri)
    assert (((vals >= 1000) & (vals < 2000)) | ((vals >= 0) & (vals < nobj))).all()
    plain.sync()
    assert torch.equal(r.rgb_tensor().to_torch(), plain.rgb_tensor().to_torch())
    assert torch.equal(depth.view(torch.int32), plain.depth_tensor().to_torch().view(torch.int32))


def test_the_column_is_mutable_between_steps(native, oracle_mod):
    import torch
    base = scenes.synthetic_scene(512, with_wall=True)
    views = (0, base.num_views)
    r = _make(_with(base, True), visibility=False)
    assert r.raster_entry() == "group"
    t = r.instance_label_tensor().to_torch()
    assert t.is_cuda and t.dtype == torch.int32 and tuple(t.shape) == (3 * 512,) and bool((t == lb.SENTINEL).all())
    fs = oracle_mod.FlatScene(base)
    ref = lo.render(base, want_ids=True)
    got, _ = _check(r, fs, lb.expand(base), ref, views)
    assert np.array_equal(got["segmask"], ref["segmask"])  # a column of sentinels: the object ids
    rows = lb.mixed(len(base.instances), seed=5)
    t.copy_(torch.from_numpy(rows).to(t.device))           # (the renderer's stream is torch's current one: the null stream)
    r.step()
    _, want = _check(r, fs, rows, ref, views)
    _assert_labels_decide(fs, rows, ref, views, want)
    t[::2] = lb.SENTINEL                                   # half of the rows back to their objects' ids
    rows2 = rows.copy()
    rows2[::2] = lb.SENTINEL
    r.step()
    _check(r, fs, rows2, ref, views)
    t.fill_(lb.SENTINEL)
    r.step()
    got, _ = _check(r, fs, lb.expand(base), ref, views)
    assert np.array_equal(got["segmask"], ref["segmask"])


def test_the_setter_is_stream_ordered_and_reads_back(native, oracle_mod):
    base = scenes.synthetic_scene(2048)
    views = (0, 600)
    first, second = lb.mixed(len(base.instances), seed=2), lb.mixed(len(base.instances), seed=3)
    assert (first != second).mean() > 0.3
    r = _make(_with(base, first), visibility=False)
    assert r.raster_entry() == "group-fast"
    assert np.array_equal(r.instance_labels(), lb.expand(base, first))
    fs = oracle_mod.FlatScene(base)
    ref = lo.render(base, None, None, 0, 600, want_ids=True)
    _check(r, fs, first, ref, views)                       # the first frame already shows the initial labels
    r.render()                                             # enqueued ahead of the setter: it keeps the old labels
    r.set_instance_labels(second)
    _check(r, fs, first, ref, views)
    assert np.array_equal(r.instance_labels(), second)     # the round trip through the C ABI
    assert np.array_equal(r.instance_label_tensor().to_torch().cpu().numpy(), second)
    r.step()
    got, _ = _check(r, fs, second, ref, views)
    assert not np.array_equal(got["segmask"], lb.segmask(fs, first, ref["tri_id"], 0, 600))
    part = np.array([-7, 0, 2 ** 31 - 1, -2 ** 31, 5], np.int32)       # a sub-range, any int32
    r.set_instance_labels(part, first_row=4)
    third = second.copy()
    third[4:9] = part
    assert np.array_equal(r.instance_labels(), third)
    r.step()
    _check(r, fs, third, ref, views)
    with pytest.raises(ValueError):
        r.set_instance_labels(np.zeros(3, np.int32), first_row=len(third) - 2)


@pytest.mark.parametrize("case", ["group-fast", "chunked", "bvh-tile", "bvh-tile-rt", "flat"])
def test_the_default_column_is_the_object_id_segmask(native, oracle_mod, case):
    import torch
    build, variant, entry, bvh, rt = FAMILIES[case]
    base = build()
    r = _make(_with(base, True), visibility=False, variant=variant)
    assert r.raster_entry() == entry and r.bvh_launch()["kernel"] == bvh
    views = (0, min(40, base.num_views))
    ref = lo.render(base, None, None, views[0], views[1], want_ids=True)
    got = _fetch(r, views)
    assert_parity(got, {k: ref[k][views[0]:views[1]] for k in got})       # the oracle's segmask
    if rt:
        plain = _make(base, visibility=False, variant=variant)             # byte-identical to a renderer without the flag
        plain.sync()
        assert torch.equal(r.segmask_tensor().to_torch(), plain.segmask_tensor().to_torch())
        assert torch.equal(r.rgb_tensor().to_torch(), plain.rgb_tensor().to_torch())


@pytest.mark.parametrize("case", ["group", "brute", "bvh-tile", "flat"])
def test_values_are_stored_as_they_are(native, oracle_mod, case):
    build, variant, entry, bvh, rt = FAMILIES[case]
    base = build()
    special = np.array([-1, -2, 2 ** 31 - 1, -2 ** 31 + 1], np.int64)
    labels = np.resize(special, len(base.instances)).astype(np.int32)
    r = _make(_with(base, labels), visibility=False, variant=variant)
    assert r.raster_entry() == entry
    views = (0, min(40, base.num_views))
    fs = oracle_mod.FlatScene(base)
    ref = lo.render(base, None, None, views[0], views[1], want_ids=True)
    got, want = _check(r, fs, lb.expand(base, labels), ref, views)
    covered = ref["tri_id"][views[0]:views[1]] >= 0
    seen = set(np.unique(got["segmask"][covered]).tolist())
    assert seen <= set(special.tolist()) and len(seen) >= 3, seen
    owner = lb.owner_rows(fs, ref["tri_id"], views[0], views[1])
    assert np.array_equal(got["segmask"][covered], lb.expand(base, labels)[owner[covered]])


@pytest.mark.parametrize("case", ["group", "bvh-tile"])
def test_labels_beside_every_other_column_and_output(native, oracle_mod, case):
    import torch
    build, variant, entry, bvh, rt = FAMILIES[case]
    base = mo.with_table(build())
    n = len(base.instances)
    labels = lb.mixed(n, seed=4)
    more = dict(instance_materials=mo.mixed(n, mo.num_materials(base), seed=4),
                instance_colors=np.roll(co.mixed(n, seed=3), 2, axis=0),
                world_lights=list(lo.mixed(base.num_worlds, shift=2)),
                camera_projections=list(po.mixed(len(base.cameras))), normals=True)
    full = _with(base, labels, **more)
    r = _make(full, visibility=False, variant=variant)
    plain = _make(_with(full, None), visibility=rt is False, variant=variant)
    assert r.raster_entry() == entry and r.bvh_launch() == plain.bvh_launch() and plain.raster_entry() == entry
    views = (0, 12)                                       # (the CPU side restates materials, colours and normals per view)
    ref = mo.render(base, more["instance_materials"], more["instance_colors"], more["world_lights"],
                    more["camera_projections"], view_begin=views[0], view_end=views[1], want_ids=True)
    fs = oracle_mod.FlatScene(base)
    col = lb.expand(base, labels)
    got, want = _check(r, fs, col, ref, views)
    _assert_labels_decide(fs, col, ref, views, want)
    r.sync()
    plain.sync()
    nrm = r.normal_tensor().to_torch()
    assert torch.equal(r.rgb_tensor().to_torch(), plain.rgb_tensor().to_torch())
    assert torch.equal(r.depth_tensor().to_torch().view(torch.int32), plain.depth_tensor().to_torch().view(torch.int32))
    assert torch.equal(nrm, plain.normal_tensor().to_torch())
    wantn = no.normals(fs, ref["tri_id"], views[0], views[1])
    assert np.array_equal(nrm[views[0]:views[1]].cpu().numpy(), wantn)


@pytest.mark.parametrize("case", ["group-fast", "textured", "chunked", "brute", "bvh-tile-pairs", "bvh-tile-rt", "flat"])
def test_the_label_forms_beside_every_column_in_the_other_families(native, oracle_mod, case):
    """The same renderer as above in the other families, the CPU side kept cheap: the segmask against the label oracle
    through the tri_id of the oracle under the same projections (materials, colours and lights change no tri_id), every
    other output byte-identical on the device to the same renderer without labels -- whose parity with the oracle
    tests/test_normal_gpu.py and tests/test_material_gpu.py hold."""
    import torch
    build, variant, entry, bvh, rt = FAMILIES[case]
    base = mo.with_table(build())
    n = len(base.instances)
    labels = lb.mixed(n, seed=4)
    projs = list(po.mixed(len(base.cameras)))
    full = _with(base, labels, instance_materials=mo.mixed(n, mo.num_materials(base), seed=4),
                 instance_colors=np.roll(co.mixed(n, seed=3), 2, axis=0),
                 world_lights=list(lo.mixed(base.num_worlds, shift=2)), camera_projections=projs, normals=True)
    r = _make(full, visibility=False, variant=variant)
    plain = _make(_with(full, None), visibility=False, variant=variant)
    assert r.raster_entry() == entry == plain.raster_entry() and r.bvh_launch() == plain.bvh_launch()
    views = (0, min(40, base.num_views))
    ref = po.render(base, projs, views[0], views[1], want_ids=True)
    fs = oracle_mod.FlatScene(base)
    col = lb.expand(base, labels)
    want = lb.segmask(fs, col, ref["tri_id"], views[0], views[1])
    r.sync()
    plain.sync()
    got = r.segmask_tensor().to_torch()[views[0]:views[1]].cpu().numpy()
    assert int((got != want).sum()) == 0
    _assert_labels_decide(fs, col, ref, views, {"segmask": want})
    assert torch.equal(r.rgb_tensor().to_torch(), plain.rgb_tensor().to_torch())
    assert torch.equal(r.depth_tensor().to_torch().view(torch.int32), plain.depth_tensor().to_torch().view(torch.int32))
    assert torch.equal(r.normal_tensor().to_torch(), plain.normal_tensor().to_torch())
    if rt:
        t = r.segmask_tensor().to_torch()
        p = plain.segmask_tensor().to_torch()
        assert torch.equal(t == -1, p == -1)               # the same pixels covered as in the object-id segmask


@pytest.mark.parametrize("normals", [False, True], ids=["labels", "labels-normals"])
def test_labels_through_the_plain_entry_at_16_slots(native, oracle_mod, monkeypatch, normals):
    # both label forms (without and with the normals output) behind the plain entry of a 16-slot world (the FAST entry
    # switched off): two one-tile views
    monkeypatch.setenv("MRX_GROUP_FAST", "0")
    base = scenes.synthetic_scene(2)
    labels = lb.mixed(len(base.instances))
    r = _make(_with(base, labels, normals=normals), visibility=False)
    assert r.raster_entry() == "group"
    views = (0, base.num_views)
    fs = oracle_mod.FlatScene(base)
    ref = lo.render(base, None, None, views[0], views[1], want_ids=True)
    _check(r, fs, lb.expand(base, labels), ref, views)
    if normals:
        assert np.array_equal(r.normal_tensor().to_torch().cpu().numpy(), no.normals(fs, ref["tri_id"], views[0], views[1]))


@pytest.mark.parametrize("outputs", ["Depth", "RGB"])
@pytest.mark.parametrize("case", ["group-fast", "group", "bvh-tile", "flat"])
def test_labels_in_depth_only_and_rgb_only_renderers(native, oracle_mod, case, outputs):
    import torch
    build, variant, entry, bvh, rt = FAMILIES[case]
    base = build()
    labels = lb.mixed(len(base.instances), seed=6)
    r = _make(_with(base, labels), visibility=False, variant=variant, outputs=outputs)
    plain = _make(base, visibility=False, variant=variant, outputs=outputs)
    assert r.raster_entry() == entry == plain.raster_entry() and r.bvh_launch() == plain.bvh_launch()
    views = (0, min(40, base.num_views))
    fs = oracle_mod.FlatScene(base)
    ref = lo.render(base, None, None, views[0], views[1], want_ids=True)
    got = _fetch(r, views, outputs)
    want = lb.segmask(fs, lb.expand(base, labels), ref["tri_id"], views[0], views[1])
    assert int((got["segmask"] != want).sum()) == 0
    assert (want != ref["segmask"][views[0]:views[1]]).any()
    plain.sync()
    if outputs == "Depth":
        assert depth_ulps(got["depth"], ref["depth"][views[0]:views[1]]) <= 1
        assert torch.equal(r.depth_tensor().to_torch().view(torch.int32), plain.depth_tensor().to_torch().view(torch.int32))
        with pytest.raises(RuntimeError):
            r.rgb_tensor()
    else:
        assert int((got["rgb"] != ref["rgb"][views[0]:views[1]]).any(axis=-1).sum()) == 0
        assert torch.equal(r.rgb_tensor().to_torch(), plain.rgb_tensor().to_torch())
        with pytest.raises(RuntimeError):
            r.depth_tensor()


def test_poses_cameras_and_hidden_rows(native, oracle_mod):
    import torch
    base = scenes.synthetic_scene(64, with_wall=True)
    labels = lb.mixed(len(base.instances))
    col = lb.expand(base, labels)
    r = _make(_with(base, labels), visibility=False)
    views = (0, base.num_views)
    fs = oracle_mod.FlatScene(base)
    pos, cam = r.instance_position_tensor().to_torch(), r.camera_position_tensor().to_torch()
    pos[1::3, 0] += 0.75                                   # the cubes move, the cameras rise
    cam[:, 2] += 0.5
    r.step()
    fs.inst_pos[1::3, 0] += np.float32(0.75)
    fs.cam_pos[:, 2] += np.float32(0.5)
    moved = fs.render()
    assert not np.array_equal(moved["tri_id"], lo.render(base, want_ids=True)["tri_id"])
    _check(r, fs, col, moved, views)
    obj = r.instance_object_tensor().to_torch()
    hidden = [i for i in range(len(col)) if i % 5 == 0]
    saved = obj[hidden].clone()
    obj[hidden] = -1 - torch.arange(len(hidden), dtype=obj.dtype, device=obj.device)
    r.step()
    fs.inst_obj[hidden] = -1
    hid = fs.render()
    assert not np.array_equal(hid["tri_id"], moved["tri_id"])
    _check(r, fs, col, hid, views)
    obj[hidden] = saved                                    # shown again, under the label that stayed with the row
    r.step()
    fs.inst_obj[hidden] = fs.inst_obj0[hidden]
    _check(r, fs, col, moved, views)
    assert np.array_equal(r.instance_labels(), col)


def test_refresh_objects_sentinel_rows_follow_labelled_rows_keep(native, oracle_mod):
    import torch
    base = scenes.synthetic_scene(32, with_wall=True)
    base.max_instances_per_world = 4                      # three rows bound, one spare
    r = _make(_with(base, True), visibility=False)
    t = r.instance_label_tensor().to_torch()
    assert tuple(t.shape) == (4 * 32,) and bool((t == lb.SENTINEL).all())
    rows = lb.mixed(4 * 32, seed=9)
    rows[3::4] = lb.SENTINEL                               # the spare rows stay at the sentinel; rows 1::4 are there too
    rows[0::4] = 1500 + np.arange(32, dtype=np.int32)      # the first row of every world: a label of its own
    t.copy_(torch.from_numpy(rows).to(t.device))
    r.step()
    fs = oracle_mod.FlatScene(base)
    views = (0, 32)
    _check(r, fs, rows, fs.render(), views)                # unbound rows draw nothing
    spare = list(range(3, 4 * 32, 4))
    first = list(range(0, 4 * 32, 4))
    obj, pos = r.instance_object_tensor().to_torch(), r.instance_position_tensor().to_torch()
    obj[spare] = 0
    pos[spare] = torch.tensor([1.5, -2.0, 2.0], device=pos.device)
    swap = int(fs.inst_obj0[1])                            # (the object of the worlds' second rows)
    assert swap != int(fs.inst_obj0[0])
    obj[first] = swap
    r.refresh_objects()
    r.step()
    assert np.array_equal(t.cpu().numpy(), rows)           # refresh_objects keeps the column
    fs.inst_obj[spare] = 0
    fs.inst_pos[spare] = (1.5, -2.0, 2.0)
    fs.inst_obj[first] = swap
    fs.refresh_objects()
    ref = fs.render()
    got, want = _check(r, fs, rows, ref, views)
    owner = lb.owner_rows(fs, ref["tri_id"], 0, 32)
    mine = np.isin(owner, spare)
    assert mine.any() and (got["segmask"][mine] == 0).all()             # the sentinel row shows its new object's id
    swapped = np.isin(owner, first)
    assert swapped.any() and (got["segmask"][swapped] >= 1500).all()     # the labelled row keeps its label


def test_off_means_off(native):
    import torch
    base = scenes.synthetic_scene(256)
    off = _make(base, visibility=False)
    with pytest.raises(RuntimeError, match="Segmask not implemented for rasterizer"):
        off.segmask_tensor()
    with pytest.raises(RuntimeError, match="MRX_FLAG_INSTANCE_LABELS"):
        off.instance_label_tensor()
    with pytest.raises(RuntimeError, match="MRX_FLAG_INSTANCE_LABELS"):
        off.set_instance_labels(np.zeros(4, np.int32))
    on = _make(_with(base, lb.mixed(len(base.instances))), visibility=False)
    assert off.raster_entry() == on.raster_entry() == "group-fast" and off.bvh_launch() == on.bvh_launch()
    off.sync()
    on.sync()
    assert torch.equal(off.rgb_tensor().to_torch(), on.rgb_tensor().to_torch())
    assert torch.equal(off.depth_tensor().to_torch().view(torch.int32), on.depth_tensor().to_torch().view(torch.int32))
    # the ids tensor is the only thing the flag adds to a step besides the column
    assert on.bytes_per_step() - off.bytes_per_step() == 4 * 256 * 64 * 64 + 4 * len(on.instance_labels())


def test_labels_beside_visibility_ids(native, oracle_mod):
    for mode in ("Rasterizer", "Raytracer"):
        base = scenes.synthetic_scene(64, with_wall=True, render_mode=mode)
        labels = lb.mixed(len(base.instances))
        r = _make(_with(base, labels), visibility=True)
        ref = lo.render(base, want_ids=True)
        r.sync()
        assert np.array_equal(r.visibility_tensor().to_torch().cpu().numpy(), ref["tri_id"])
        with pytest.raises(RuntimeError, match="visibility ids"):
            r.segmask_tensor()
        assert np.array_equal(r.instance_labels(), labels)             # the column exists and is mutable
        r.set_instance_labels(labels[::-1].copy())
        r.step()
        r.sync()
        assert np.array_equal(r.instance_labels(), labels[::-1])
        assert np.array_equal(r.visibility_tensor().to_torch().cpu().numpy(), ref["tri_id"])
        assert np.array_equal(r.rgb_tensor().to_torch().cpu().numpy(), ref["rgb"])


def test_two_shards_hold_their_own_rows(native, oracle_mod):
    base = scenes.synthetic_scene(301, with_wall=True)
    labels = lb.mixed(len(base.instances))
    r = _make(_with(base, labels), visibility=False, device_ids=[0, 0])
    assert r.num_shards == 2
    fs = oracle_mod.FlatScene(base)
    ref = lo.render(base, want_ids=True)
    r.sync()

    def per_shard(rows):
        want = lb.segmask(fs, rows, ref["tri_id"])
        for sh in range(2):
            a, b = r.shard_first_world(sh), r.shard_first_world(sh + 1)
            assert np.array_equal(r.instance_label_tensor(shard=sh).to_torch().cpu().numpy(), rows[3 * a:3 * b])
            seg = r.segmask_tensor(shard=sh).to_torch().cpu().numpy()
            rgb = r.rgb_tensor(shard=sh).to_torch().cpu().numpy()
            assert np.array_equal(seg, want[a:b]) and np.array_equal(rgb, ref["rgb"][a:b])

    per_shard(lb.expand(base, labels))
    assert np.array_equal(r.instance_labels(), labels)
    # the setter splits a range that spans the shards at their world boundary
    cut = 3 * r.shard_first_world(1)
    again = lb.mixed(len(base.instances), seed=8)
    r.set_instance_labels(again[cut - 50:cut + 70], first_row=cut - 50)
    r.step()
    now = labels.copy()
    now[cut - 50:cut + 70] = again[cut - 50:cut + 70]
    assert np.array_equal(r.instance_labels(), now)
    r.sync()
    per_shard(now)


def test_headless_instance_labels(native, oracle_mod, tmp_path):
    from madrona_renderer_amd import build
    from tests.test_headless_gpu import _tiles
    exe = build.headless_path()
    for mode, name in (("rast", "ras"), ("rt", "ray")):
        p = subprocess.run(["timeout", "-k", "5", "120", exe, "16", "2", mode, "64", "64", "--instance-labels", "7",
                            "--dump-last-frame", name], cwd=tmp_path, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        desc = scenes.synthetic_scene(16, render_mode="Raytracer" if mode == "rt" else "Rasterizer")
        ref = po.render(desc, want_ids=True)
        assert np.array_equal(np.stack(_tiles(tmp_path / (name + ".png"), 16, 64, 64)), _upright(ref["rgb"], mode))
        # the labels the binary draws: 1000 + splitmix64(splitmix64(SEED) ^ row) % 1000, rows 1::4 left at the sentinel
        base = scenes._splitmix64(np.uint64(7))
        draw = scenes._splitmix64(base ^ np.arange(len(desc.instances), dtype=np.uint64)) % np.uint64(1000)
        labels = (1000 + draw.astype(np.int64)).astype(np.int32)
        labels[1::4] = lb.SENTINEL
        want = lb.segmask(oracle_mod.FlatScene(desc), lb.expand(desc, labels), ref["tri_id"])
        png = np.stack(_tiles(tmp_path / (name + ".labels.png"), 16, 64, 64))
        want = _upright(want, mode)
        decoded = (png[..., 0].astype(np.int32) | (png[..., 1].astype(np.int32) << 8) | (png[..., 2].astype(np.int32) << 16))
        hit = want != -1
        assert hit.any() and np.array_equal(decoded[hit], want[hit] & 0xFFFFFF) and (png[..., 3][hit] == 255).all()
        assert (png[~hit] == 0).all()
        assert ((want >= 1000) & hit).sum() >= 0.4 * hit.sum() and ((want < 1000) & hit).any()


def _upright(img, mode):
    """Oracle storage -> the image as the dump writes it: Raytracer storage is [x][y]."""
    return np.swapaxes(img, 1, 2) if mode == "rt" else img
