"""The oracle under per-instance colour overrides: oracle/raster_oracle.c resolves colour
per triangle through tri_mat -> mat_color, so every overridden row is pointed at a clone of the object it is bound
to whose materials carry float32(byte) * float32(1 / 255) and the original materials' textures.  Triangle counts per
row do not change (tri_id needs no remapping); clone ids in the segmask are mapped back to the object cloned.
Nothing under oracle/ changes.

`render` composes with tests/light_oracle.py and tests/projection_oracle.py, which render sub-descs: while it runs,
the FlatScene those build applies the colours of their desc's `instance_colors` (parallel to `instances`, so worlds
that alias rows share them)."""
import contextlib
import copy

import numpy as np

K255 = np.float32(1.0) / np.float32(255.0)


def expand(desc, colors=None):
    """[rows, 4] uint8, world-major as the instance tensors are (spare rows 0), from colours parallel to
    desc.instances (default: the desc's own; None = no override anywhere)."""
    if colors is None:
        colors = getattr(desc, "instance_colors", None)
    cap = int(getattr(desc, "max_instances_per_world", 0) or 0)
    rows = []
    src = None if colors is None else np.asarray(colors, np.uint8).reshape(-1, 4)
    for ni, io, _, _ in desc.worlds:
        rows.append(np.zeros((ni, 4), np.uint8) if src is None else src[io:io + ni])
        if cap > ni:
            rows.append(np.zeros((cap - ni, 4), np.uint8))
    return np.concatenate(rows) if rows else np.zeros((0, 4), np.uint8)


def apply(fs, row_colors):
    """A copy of FlatScene `fs` in which every row whose alpha is not zero draws a clone of its bound object in
    its colour; -> (copy, {clone id: object id})."""
    rc = np.asarray(row_colors, np.uint8).reshape(-1, 4)
    assert len(rc) == len(fs.inst_obj0), (len(rc), len(fs.inst_obj0))
    out = copy.copy(fs)
    tri_pos, tri_uv, tri_mat = [fs.tri_pos], [fs.tri_uv], [fs.tri_mat]
    orient, bbmin, bbmax = [fs.tri_orient], [fs.tri_bbmin], [fs.tri_bbmax]
    first, count = list(fs.obj_first_tri), list(fs.obj_num_tris)
    mat_color, mat_tex = [fs.mat_color.reshape(-1, 4)], list(fs.mat_tex)
    inst_obj, inst_obj0 = fs.inst_obj.copy(), fs.inst_obj0.copy()
    ntri, nmat, nobj = len(fs.tri_pos), len(fs.mat_tex), len(fs.obj_first_tri)
    # A row bound to an object id outside the table draws nothing and has no triangle slots (setup_view).  The clones
    # are appended behind the table, where such an id would come to name one: the row becomes an unbound row first,
    # which numbers the triangles of its world as before.
    outside = (inst_obj0 < 0) | (inst_obj0 >= nobj)
    inst_obj0[outside] = -1
    inst_obj[outside] = -1
    clones, back = {}, {}
    for row in np.nonzero(rc[:, 3])[0]:
        obj = int(fs.inst_obj0[row])
        if obj < 0 or obj >= nobj:
            continue                                  # an unbound spare row draws nothing
        rgb = tuple(int(x) for x in rc[row, :3])
        if (obj, rgb) not in clones:
            f, c = int(fs.obj_first_tri[obj]), int(fs.obj_num_tris[obj])
            col = [np.float32(b) * K255 for b in rgb] + [np.float32(1.0)]
            by_tex, tm = {}, np.empty(c, np.int32)
            for i, m in enumerate(fs.tri_mat[f:f + c]):
                tex = int(fs.mat_tex[m]) if 0 <= m < nmat else -1
                if tex not in by_tex:                 # one new material per distinct texture
                    by_tex[tex] = len(mat_tex)
                    mat_color.append(np.asarray([col], np.float32))
                    mat_tex.append(tex)
                tm[i] = by_tex[tex]
            tri_pos.append(fs.tri_pos[f:f + c]); tri_uv.append(fs.tri_uv[f:f + c]); tri_mat.append(tm)
            orient.append(fs.tri_orient[f:f + c]); bbmin.append(fs.tri_bbmin[f:f + c]); bbmax.append(fs.tri_bbmax[f:f + c])
            clones[(obj, rgb)] = len(first)
            back[len(first)] = obj
            first.append(ntri)
            count.append(c)
            ntri += c
        inst_obj0[row] = clones[(obj, rgb)]
        if inst_obj[row] >= 0:
            inst_obj[row] = clones[(obj, rgb)]
    out.tri_pos = np.ascontiguousarray(np.concatenate(tri_pos), np.float32)
    out.tri_uv = np.ascontiguousarray(np.concatenate(tri_uv), np.float32)
    out.tri_mat = np.ascontiguousarray(np.concatenate(tri_mat), np.int32)
    out.tri_orient = np.ascontiguousarray(np.concatenate(orient), np.float32)
    out.tri_bbmin = np.ascontiguousarray(np.concatenate(bbmin), np.float32)
    out.tri_bbmax = np.ascontiguousarray(np.concatenate(bbmax), np.float32)
    out.obj_first_tri = np.asarray(first, np.int32)
    out.obj_num_tris = np.asarray(count, np.int32)
    out.mat_color = np.ascontiguousarray(np.concatenate(mat_color), np.float32).reshape(-1, 4)
    out.mat_tex = np.asarray(mat_tex, np.int32)
    out.inst_obj, out.inst_obj0 = inst_obj, inst_obj0
    return out, back


def _unmap(res, back):
    seg = res.get("segmask")
    if seg is not None and back:
        fixed = seg.copy()
        for clone, obj in back.items():
            fixed[seg == clone] = obj
        res["segmask"] = fixed
    return res


def render_flat(fs, row_colors, **kw):
    """fs.render(**kw) with row i of the scene's instance tables under row_colors[i]; `fs` itself is not changed
    (set hidden rows and refresh_objects() on it first, as on the renderer)."""
    coloured, back = apply(fs, row_colors)
    return _unmap(coloured.render(**kw), back)


@contextlib.contextmanager
def _coloured_flat_scenes():
    from oracle import oracle
    base = oracle.FlatScene

    class ColouredFlatScene(base):
        def __init__(self, desc, *a, **kw):
            super().__init__(desc, *a, **kw)
            self.row_colors = expand(desc)

        def render(self, *a, **kw):
            coloured, back = apply(self, self.row_colors)
            return _unmap(base.render(coloured, *a, **kw), back)

    oracle.FlatScene = ColouredFlatScene
    try:
        yield
    finally:
        oracle.FlatScene = base


def render(desc, colors=None, lights=None, projections=None, **kw):
    """The oracle's images of `desc` with instance row i (of desc.instances) under colors[i] (default: the desc's
    instance_colors), world w under lights[w] and view v under projections[v] (defaults: the desc's own)."""
    import dataclasses

    from tests import light_oracle
    d = dataclasses.replace(desc)
    if colors is not None:
        d.instance_colors = np.asarray(colors, np.uint8).reshape(-1, 4)
    with _coloured_flat_scenes():
        return light_oracle.render(d, lights, projections, **kw)


def mixed(n, seed=7):
    """n colours: three rows of four overridden with opaque random colours (and any non-zero alpha), rows 1::4
    left alone (alpha 0 over random bytes: they must not show)."""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 256, (n, 4), dtype=np.uint8)
    c[:, 3] = np.maximum(c[:, 3], 1)
    c[1::4, 3] = 0
    return c


def changed_fraction(ref, plain):
    """Of the pixels covered in the plain image, the share whose colour the override changed."""
    cov = plain["tri_id"] >= 0
    return float((ref["rgb"][cov] != plain["rgb"][cov]).any(axis=-1).mean())
