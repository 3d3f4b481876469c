"""The expected segmask under per-instance labels: a scatter through the C oracle's own tri_id
image,

    expected[v][pixel] = resolve(label[row_of(v, tri_id[v][pixel])]),   -1 where tri_id < 0,

where row_of numbers a view's world-local triangle slots as oracle/raster_oracle.c's setup_view does (rows of the
view's world in order, a hidden row keeps its slots, an unbound row has none, slots follow inst_obj0 -- the walk of
tests/normal_oracle.view_geometry) and resolve maps the sentinel to the id of the object the row is bound to.  With
every row at the sentinel this is the C oracle's segmask byte for byte (tests/test_label_cpu.py), which pins row_of.
Nothing under oracle/ changes; it composes with the projection, light, colour and material oracles by taking tri_id
from their renders: none of them changes which row wins a pixel."""
import numpy as np

SENTINEL = -2 ** 31


def expand(desc, labels=None):
    """[rows] int32, world-major as the instance tensors are (spare rows at the sentinel), from labels parallel to
    desc.instances (default: the desc's own; None or True = the sentinel everywhere)."""
    if labels is None:
        labels = getattr(desc, "instance_labels", None)
    if labels is True:
        labels = None
    cap = int(getattr(desc, "max_instances_per_world", 0) or 0)
    src = None if labels is None else np.asarray(labels, np.int32).reshape(-1)
    rows = []
    for ni, io, _, _ in desc.worlds:
        rows.append(np.full(ni, SENTINEL, np.int32) if src is None else src[io:io + ni])
        if cap > ni:
            rows.append(np.full(cap - ni, SENTINEL, np.int32))
    return np.concatenate(rows) if rows else np.zeros(0, np.int32)


def mixed(n, seed=11):
    """n labels in [1000, 2000): three rows of four labelled at random, rows 1::4 left at the sentinel."""
    rng = np.random.default_rng(seed)
    m = rng.integers(1000, 2000, n).astype(np.int32)
    m[1::4] = SENTINEL
    return m


def row_of(fs, v):
    """[K] int64: the instance row that draws world-local triangle slot k of view v of FlatScene `fs`."""
    w = int(fs.view_world[v])
    nobj = len(fs.obj_first_tri)
    rows = []
    for i in range(int(fs.world_inst_start[w]), int(fs.world_inst_start[w + 1])):
        obj = int(fs.inst_obj0[i])
        if obj < 0 or obj >= nobj:
            continue                                  # unbound: no slots
        rows.append(np.full(int(fs.obj_num_tris[obj]), i, np.int64))   # (a hidden row keeps its slots)
    return np.concatenate(rows) if rows else np.zeros(0, np.int64)


def resolve(fs, row_labels):
    """[rows] int32: what the segmask holds for each row -- its label, or the bound object's id at the sentinel."""
    lab = np.asarray(row_labels, np.int32).reshape(-1)
    assert len(lab) == len(fs.inst_obj0), (len(lab), len(fs.inst_obj0))
    return np.where(lab == SENTINEL, fs.inst_obj0.astype(np.int32), lab).astype(np.int32)


def segmask(fs, row_labels, tri_id, view_begin=0, view_end=None):
    """[view_end - view_begin, slow, fast] int32: the expected segmask of views [view_begin, view_end) of FlatScene
    `fs` (hidden rows and bindings as it holds them now) under the world-major column `row_labels`, through
    tri_id[view_begin:view_end] of a render of the same state -- `tri_id` is indexed by view of the whole job."""
    if view_end is None:
        view_end = fs.num_views
    value = resolve(fs, row_labels)
    out = []
    for v in range(view_begin, view_end):
        table = value[row_of(fs, v)]
        t = tri_id[v]
        img = np.full(t.shape, -1, np.int32)
        hit = t >= 0
        img[hit] = table[t[hit]]
        out.append(img)
    return np.stack(out)


def owner_rows(fs, tri_id, view_begin, view_end):
    """[views, slow, fast] int64: the row that owns each pixel of views [view_begin, view_end), -1 on the background."""
    out = []
    for v in range(view_begin, view_end):
        rows = row_of(fs, v)
        t = tri_id[v]
        img = np.full(t.shape, -1, np.int64)
        hit = t >= 0
        img[hit] = rows[t[hit]]
        out.append(img)
    return np.stack(out)


def flat_scene(desc):
    from oracle import oracle
    return oracle.FlatScene(desc)
