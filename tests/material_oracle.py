"""The oracle under per-instance material overrides: oracle/raster_oracle.c resolves colour
and texture per triangle through tri_mat -> mat_color / mat_tex, so every overridden row is pointed at a clone of the
object it is bound to whose triangles all name the overriding material.  Triangle counts per row do not change (tri_id
needs no remapping); clone ids in the segmask are mapped back to the object cloned.  Nothing under oracle/ changes.

`render` composes with tests/color_oracle.py -- material first, then colour: the colour helper clones the material
clones and keeps the texture of the material in effect -- and through it with tests/light_oracle.py and
tests/projection_oracle.py."""
import contextlib
import copy
import dataclasses
import os

import numpy as np

from tests import color_oracle as co

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def expand(desc, materials=None):
    """[rows] int32, world-major as the instance tensors are (spare rows -1), from ids parallel to desc.instances
    (default: the desc's own; None or True = no override anywhere)."""
    if materials is None:
        materials = getattr(desc, "instance_materials", None)
    if materials is True:
        materials = None
    cap = int(getattr(desc, "max_instances_per_world", 0) or 0)
    src = None if materials is None else np.asarray(materials, np.int32).reshape(-1)
    rows = []
    for ni, io, _, _ in desc.worlds:
        rows.append(np.full(ni, -1, np.int32) if src is None else src[io:io + ni])
        if cap > ni:
            rows.append(np.full(cap - ni, -1, np.int32))
    return np.concatenate(rows) if rows else np.zeros(0, np.int32)


def apply(fs, row_mats):
    """A copy of FlatScene `fs` in which every row whose id names a material of the table draws a clone of its bound
    object with that material on every triangle; -> (copy, {clone id: object id})."""
    rm = np.asarray(row_mats, np.int64).reshape(-1)
    assert len(rm) == len(fs.inst_obj0), (len(rm), len(fs.inst_obj0))
    out = copy.copy(fs)
    tri_pos, tri_uv, tri_mat = [fs.tri_pos], [fs.tri_uv], [fs.tri_mat]
    orient, bbmin, bbmax = [fs.tri_orient], [fs.tri_bbmin], [fs.tri_bbmax]
    first, count = list(fs.obj_first_tri), list(fs.obj_num_tris)
    inst_obj, inst_obj0 = fs.inst_obj.copy(), fs.inst_obj0.copy()
    ntri, nmat, nobj = len(fs.tri_pos), len(fs.mat_tex), len(fs.obj_first_tri)
    # A row bound to an object id outside the table draws nothing and has no triangle slots (setup_view).  The clones
    # are appended behind the table, where such an id would come to name one: the row becomes an unbound row first,
    # which numbers the triangles of its world as before.
    outside = (inst_obj0 < 0) | (inst_obj0 >= nobj)
    inst_obj0[outside] = -1
    inst_obj[outside] = -1
    clones, back = {}, {}
    for row in np.nonzero((rm >= 0) & (rm < nmat))[0]:
        obj, m = int(fs.inst_obj0[row]), int(rm[row])
        if obj < 0 or obj >= nobj:
            continue                                  # an unbound spare row draws nothing
        if (obj, m) not in clones:
            f, c = int(fs.obj_first_tri[obj]), int(fs.obj_num_tris[obj])
            tri_pos.append(fs.tri_pos[f:f + c]); tri_uv.append(fs.tri_uv[f:f + c]); tri_mat.append(np.full(c, m, np.int32))
            orient.append(fs.tri_orient[f:f + c]); bbmin.append(fs.tri_bbmin[f:f + c]); bbmax.append(fs.tri_bbmax[f:f + c])
            clones[(obj, m)] = len(first)
            back[len(first)] = obj
            first.append(ntri)
            count.append(c)
            ntri += c
        inst_obj0[row] = clones[(obj, m)]
        if inst_obj[row] >= 0:
            inst_obj[row] = clones[(obj, m)]
    out.tri_pos = np.ascontiguousarray(np.concatenate(tri_pos), np.float32)
    out.tri_uv = np.ascontiguousarray(np.concatenate(tri_uv), np.float32)
    out.tri_mat = np.ascontiguousarray(np.concatenate(tri_mat), np.int32)
    out.tri_orient = np.ascontiguousarray(np.concatenate(orient), np.float32)
    out.tri_bbmin = np.ascontiguousarray(np.concatenate(bbmin), np.float32)
    out.tri_bbmax = np.ascontiguousarray(np.concatenate(bbmax), np.float32)
    out.obj_first_tri = np.asarray(first, np.int32)
    out.obj_num_tris = np.asarray(count, np.int32)
    out.inst_obj, out.inst_obj0 = inst_obj, inst_obj0
    return out, back


def render_flat(fs, row_mats, row_colors=None, **kw):
    """fs.render(**kw) with row i of the scene's instance tables under material row_mats[i], then under colour
    row_colors[i]; `fs` itself is not changed (set hidden rows and refresh_objects() on it first, as on the renderer)."""
    matd, back = apply(fs, row_mats)
    if row_colors is None:
        return co._unmap(matd.render(**kw), back)
    return co._unmap(co.render_flat(matd, row_colors, **kw), back)


@contextlib.contextmanager
def _material_flat_scenes():
    from oracle import oracle
    base = oracle.FlatScene

    class MaterialFlatScene(base):
        def __init__(self, desc, *a, **kw):
            super().__init__(desc, *a, **kw)
            self.row_mats = expand(desc)

        def render(self, *a, **kw):
            matd, back = apply(self, self.row_mats)
            return co._unmap(base.render(matd, *a, **kw), back)

    oracle.FlatScene = MaterialFlatScene
    try:
        yield
    finally:
        oracle.FlatScene = base


def render(desc, materials=None, colors=None, lights=None, projections=None, **kw):
    """The oracle's images of `desc` with instance row i (of desc.instances) under material materials[i] and then
    colour colors[i] (defaults: the desc's instance_materials / instance_colors), world w under lights[w] and view v
    under projections[v] (defaults: the desc's own)."""
    from tests import light_oracle
    d = dataclasses.replace(desc)
    if materials is not None:
        d.instance_materials = np.asarray(materials, np.int32).reshape(-1)
    if colors is not None:
        d.instance_colors = np.asarray(colors, np.uint8).reshape(-1, 4)
    # (the colour hook inside: the material scene's render hands its clones on to the coloured render)
    with co._coloured_flat_scenes():
        with _material_flat_scenes():
            return light_oracle.render(d, lights, projections, **kw)


def mixed(n, num_materials, seed=11):
    """n ids: three rows of four overridden with random materials of the table, rows 1::4 left alone (-1)."""
    rng = np.random.default_rng(seed)
    m = rng.integers(0, num_materials, n).astype(np.int32)
    m[1::4] = -1
    return m


def with_table(desc, textured=True):
    """A copy of `desc` whose material table has four more materials.  textured (the default): one untextured red and
    three textured ones over data/cube.png, tests/golden/rgba8_5x3.ktx2 (non-power-of-two) and
    tests/golden/cube64_bc7.ktx2, their textures appended to the API textures.  Not textured: four untextured colours,
    and the textures of the scene's own materials dropped -- a table without a textured material (for scenes that
    draw none)."""
    from madrona_renderer_amd import scenes
    d = dataclasses.replace(desc)
    mats, paths = list(desc.materials), list(desc.texture_paths)
    if textured:
        t0 = len(paths)
        paths += [os.path.join(scenes.DATA_DIR, "cube.png"), os.path.join(GOLDEN, "rgba8_5x3.ktx2"),
                  os.path.join(GOLDEN, "cube64_bc7.ktx2")]
        mats += [((1.0, 0.0, 0.0, 1.0), -1, 0.5, 0.5), ((1.0, 1.0, 1.0, 1.0), t0, 0.5, 0.5),
                 ((0.2, 0.9, 1.0, 1.0), t0 + 1, 0.5, 0.5), ((1.0, 0.5, 0.1, 1.0), t0 + 2, 0.5, 0.5)]
    else:
        mats = [(c, -1, ro, me) for c, _, ro, me in mats]
        mats += [((1.0, 0.0, 0.0, 1.0), -1, 0.5, 0.5), ((0.1, 0.2, 1.0, 1.0), -1, 0.5, 0.5),
                 ((0.0, 0.8, 0.2, 1.0), -1, 0.5, 0.5), ((1.0, 0.9, 0.0, 1.0), -1, 0.5, 0.5)]
    d.materials, d.texture_paths = mats, paths
    return d


def num_materials(desc):
    """Materials of the desc's table as the renderer counts them (API materials, then the ones of MTL files)."""
    from oracle import oracle
    return len(oracle.FlatScene(dataclasses.replace(desc, worlds=desc.worlds[:1], num_worlds=1)).mat_tex)


changed_fraction = co.changed_fraction
