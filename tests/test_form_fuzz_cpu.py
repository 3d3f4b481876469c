"""The form-kernel fuzz (tests/form_fuzz.py, tests/test_form_fuzz_gpu.py) checked without a device: the case table
covers the form-kernel rows of the committed resource table by construction, the Python restatement of DESIGN.md
4.17's rule agrees with every case, the composed oracle helper draws nothing for rows bound outside the object table,
and the references are not vacuous.

Measured on the CPU oracle over the compared views of each (scene, recipe) of the case table (printed by
test_references_are_not_vacuous; the bounds are 0.01 of the pixels covered, a non-zero changed share, one view with a
winning triangle across its own near plane under mixed projections, one covered pixel on either side of S10's sign
rule under a normals recipe):

  mesh-300-48x48-Rast-notex     6 recipes: covered 0.520 - 0.558, changed 0.630 - 1.000, near-plane views 1 - 1, d > 0 / d < 0 pixels at least 2313 / 7277
  mesh-300-48x48-Rayt-notex     4 recipes: covered 0.520 - 0.558, changed 0.933 - 1.000, near-plane views 1 - 1, d > 0 / d < 0 pixels at least 2350 / 7839
  soup-100-128x64-Rast-notex    9 recipes: covered 0.185 - 0.263, changed 0.243 - 1.000, near-plane views 3 - 3, d > 0 / d < 0 pixels at least 7707 / 3277
  soup-100-128x64-Rast-tex     13 recipes: covered 0.185 - 0.263, changed 0.243 - 1.000, near-plane views 3 - 3, d > 0 / d < 0 pixels at least 7707 / 3277
  soup-109-37x53-Rast-notex    14 recipes: covered 0.241 - 0.286, changed 0.298 - 1.000, near-plane views 13 - 13, d > 0 / d < 0 pixels at least 8226 / 7130
  soup-109-37x53-Rast-tex      11 recipes: covered 0.241 - 0.286, changed 0.307 - 1.000, near-plane views 13 - 13, d > 0 / d < 0 pixels at least 8226 / 7130
  soup-109-64x64-Rayt-notex     6 recipes: covered 0.219 - 0.250, changed 0.645 - 1.000, near-plane views 7 - 7, d > 0 / d < 0 pixels at least 7205 / 8043
  soup-109-64x64-Rayt-tex       5 recipes: covered 0.219 - 0.250, changed 0.658 - 1.000, near-plane views 7 - 7, d > 0 / d < 0 pixels at least 6118 / 8043
  soup-144-64x64-Rast-notex    10 recipes: covered 0.289 - 0.359, changed 0.201 - 1.000, near-plane views 7 - 7, d > 0 / d < 0 pixels at least 12834 / 7311
  soup-144-64x64-Rast-tex       9 recipes: covered 0.289 - 0.359, changed 0.484 - 1.000, near-plane views 7 - 7, d > 0 / d < 0 pixels at least 12834 / 7311
  soup-144-96x130-Rast-notex    7 recipes: covered 0.278 - 0.381, changed 0.338 - 1.000, near-plane views 3 - 3, d > 0 / d < 0 pixels at least 8289 / 9028
  soup-144-96x130-Rast-tex      7 recipes: covered 0.278 - 0.381, changed 0.980 - 1.000, near-plane views 3 - 3, d > 0 / d < 0 pixels at least 8289 / 9028
  uniform-10-64x64-Rast-notex   9 recipes: covered 0.215 - 0.343, changed 0.475 - 0.931, near-plane views 8 - 8, d > 0 / d < 0 pixels at least 5523 / 9457
  uniform-10-64x64-Rast-tex     9 recipes: covered 0.208 - 0.215, changed 0.928 - 0.998, near-plane views 8 - 8, d > 0 / d < 0 pixels at least 1175 / 9457
  uniform-11-50x30-Rast-notex   9 recipes: covered 0.174 - 0.199, changed 0.832 - 1.000, near-plane views 20 - 20, d > 0 / d < 0 pixels at least 5935 / 6094
  uniform-11-50x30-Rast-tex     9 recipes: covered 0.199 - 0.335, changed 0.509 - 0.936, near-plane views 20 - 20, d > 0 / d < 0 pixels at least 6641 / 7096

(scene-seed-size-mode-textures; `changed` leaves out the recipe of normals alone, which changes no other output.)
The soups cover less under mixed projections than under the defaults (64 x 64, seed 144: 0.289 against 0.327).
"""
import os

import numpy as np
import pytest

from tests import color_oracle as co
from tests import form_fuzz as ff
from tests import light_oracle as lo
from tests import material_oracle as mo
from tests import normal_oracle as no
from tests.test_fuzz_gpu import _scene
from tests.util import render_oracle


def test_the_case_table_is_the_form_rows_of_the_resource_table():
    rows = ff.resource_rows()
    assert len(rows) == len(set(rows)) == 390
    unreached = {row for row, _ in ff.UNREACHED}
    assert all(reason for _, reason in ff.UNREACHED) and unreached <= set(rows)
    targeted = {c.row for c in ff.CASES}
    assert not targeted & unreached
    assert targeted | unreached == set(rows), (sorted(set(rows) - targeted - unreached), sorted(targeted - set(rows)))
    for template in ff.FORM_TEMPLATES:
        of = [r for r in rows if r.startswith(template + "<")]
        left = [r for r in unreached if r.startswith(template + "<")]
        print("%-26s %3d rows, %3d launched, %d unreached" % (template, len(of), len(of) - len(left), len(left)))
        if template.startswith("rasterGroupFormKernel"):
            assert not left
        assert 10 * len(left) <= len(of)
    assert len({c.name for c in ff.CASES}) == len(ff.CASES)
    # one case in five, seeded, selects an output
    share = sum(c.outputs is not None for c in ff.CASES) / len(ff.CASES)
    assert 0.1 < share < 0.3 and {c.outputs for c in ff.CASES} == {None, "Depth", "RGB"}


def test_recipes_select_their_form_under_the_rule():
    """Every case's recipe selects the case's form (with its ids and output selection); the smallest recipe of a form
    is a subset of the largest, and dropping any element of the smallest selects another form."""
    for c in ff.CASES:
        desc = ff.scene_desc(c.scene, c.textured, c.recipe)
        family = ff.RULE_FAMILY.get(c.family, c.family)
        assert ff.expected_form(family, desc, c.ids, c.outputs) == c.form, c.name
        assert ff.expected_textured(desc, c.outputs) in (None, c.textured), c.name
        tris = ff.max_world_triangles(desc)
        if c.family == "group":
            assert 0 < tris <= 16, c.name                 # (every slot count from 16 on is MRX_DEBUG_SLOTS' to force)
        if c.family == "brute":
            assert (tris > 64) == c.row.endswith("true>"), c.name
        if c.family == "chunked":
            assert tris > 256, c.name
        if c.family == "bvh-flat":
            assert 0 < tris <= 64, c.name
    for family, forms in (("group", ff.GROUP_FORMS), ("brute", ff.TILE_FORMS), ("bvh-tile", ff.BVH_TILE_FORMS)):
        base = ff.base_scene(ff.SOUPS[0], False)
        for form in forms:
            small, large = ff.recipes(form, family)
            ids = "segmask" if form in ("L", "LN") else "visibility"
            for r in (small, large):
                assert ff.expected_form(family, ff.with_recipe(base, r, False), ids) == form, (family, form, r)
            for field in ff.Recipe._fields:
                if getattr(small, field):
                    assert getattr(large, field), (form, field)
                    less = small._replace(**{field: None if field in ("proj", "light") else False})
                    assert ff.expected_form(family, ff.with_recipe(base, less, False), ids) != form, (form, field)
    # the tables vary with the lights alone, and only a light that differs makes a light table
    base = ff.base_scene(ff.SOUPS[0], False)
    assert ff.expected_form("group", ff.with_recipe(base, ff.Recipe(light="same"), False), "none") == "Uniform"
    assert ff.expected_form("group", ff.with_recipe(base, ff.Recipe(proj="same"), False), "none") == "Uniform"
    assert ff.expected_form("group", ff.with_recipe(base, ff.Recipe(light="mixed", normals=True), False), "none") == "NPV"
    # a depth-only renderer never reads the colour and material columns; visibility ids win over the label column
    both = ff.with_recipe(base, ff.Recipe(color=True, mat=True), False)
    assert ff.expected_form("group", both, "none", "Depth") == "Uniform"
    assert ff.expected_form("bvh-tile", both, "none", "Depth") == "Uniform"
    assert ff.expected_form("group", ff.with_recipe(base, ff.Recipe(labels=True), False), "visibility") == "Uniform"


@pytest.mark.parametrize("seed,worlds,size", [(21, 12, (33, 64)), (144, 24, (64, 64)), (109, 24, (37, 53))])
def test_rows_bound_outside_the_object_table_draw_nothing_under_overrides(oracle_mod, seed, worlds, size):
    d = _scene(seed, worlds, size[0], size[1], "Rasterizer")
    fs = oracle_mod.FlatScene(d)
    nobj, n = len(fs.obj_first_tri), len(d.instances)
    assert (fs.inst_obj0 >= nobj).sum() >= 3              # the soup binds rows to the id one past the table
    plain = render_oracle(d)
    # every column at "no override", default light and projections: the oracle itself, bit for bit
    quiet = mo.render(d, np.full(n, -1, np.int32), np.zeros((n, 4), np.uint8), [lo.DEFAULT] * d.num_worlds,
                      [(90.0, None)] * len(d.cameras), want_ids=True)
    for k in ("rgb", "tri_id", "segmask"):
        assert np.array_equal(quiet[k], plain[k]), k
    assert np.array_equal(quiet["depth"].view(np.uint32), plain["depth"].view(np.uint32))
    # overrides on three rows of four, out-of-range rows among them: no view names a triangle its world has not
    base = mo.with_table(d)
    mats, cols = mo.mixed(n, mo.num_materials(base)), co.mixed(n)
    bound_outside = np.asarray([o >= nobj for _, _, _, o in d.instances])
    assert (bound_outside & (mats >= 0)).any() and (bound_outside & (cols[:, 3] != 0)).any()
    for ref in (mo.render(base, mats, cols, want_ids=True), mo.render(base, mats, want_ids=True),
                co.render(d, cols, want_ids=True)):
        bfs = oracle_mod.FlatScene(base)
        for v in range(bfs.num_views):
            slots = len(no.view_geometry(bfs, v)[1])
            assert int(ref["tri_id"][v].max()) < slots, (v, int(ref["tri_id"][v].max()), slots)
        assert np.array_equal(ref["tri_id"], plain["tri_id"])           # no override changes which triangle wins
        assert np.array_equal(ref["segmask"], plain["segmask"])
        no.normals(bfs, ref["tri_id"])                                  # indexes without error


def _witness_keys():
    seen = {}
    for c in ff.CASES:
        seen.setdefault((c.scene, c.textured, c.recipe), c)
    return seen


def test_references_are_not_vacuous(oracle_mod):
    lines = []
    plain_cache = {}
    for (scene, textured, recipe), c in sorted(_witness_keys().items(), key=lambda kv: str(kv[0])):
        desc = ff.scene_desc(scene, textured, recipe)
        views = ff.compared_views(scene, desc)
        ref = ff.cached_reference(scene, textured, recipe)
        covered = ref["tri_id"] >= 0
        cov = float(covered.mean())
        pkey = (scene, textured)
        if pkey not in plain_cache:
            base = ff.base_scene(scene, textured and scene.kind != "mesh")
            p = render_oracle(base, view_begin=views[0], view_end=views[1])
            plain_cache[pkey] = {k: p[k][views[0]:views[1]] for k in ("rgb", "tri_id", "segmask")}
        plain = plain_cache[pkey]
        changed = ((ref["rgb"] != plain["rgb"]).any(axis=-1) | (ref["tri_id"] != plain["tri_id"]) |
                   (ref["segmask"] != plain["segmask"]))
        share = float(changed[covered].mean()) if covered.any() else 0.0
        near = ff.near_crossing_views(desc, ref["tri_id"], views) if recipe.proj == "mixed" else None
        sides = ff.normal_sides(desc, ref["tri_id"], views) if recipe.normals else None
        name = "%s-%d-%dx%d-%s-%s %s" % (scene.kind, scene.seed, scene.width, scene.height, scene.mode[:4],
                                         "tex" if textured else "notex",
                                         "+".join("%s=%s" % (f, getattr(recipe, f)) if f in ("proj", "light") else f
                                                  for f in ff.Recipe._fields if getattr(recipe, f)))
        lines.append("%-78s covered %.3f changed %.3f near %s sides %s" % (name, cov, share, near, sides))
        assert cov >= 0.01, lines[-1]
        if recipe != ff.Recipe(normals=True):              # (normals alone change no other output: `sides` is its witness)
            assert share > 0, lines[-1]
        if near is not None:
            assert near >= 1, lines[-1]
        if sides is not None:
            assert sides[0] >= 1 and sides[1] >= 1, lines[-1]
    print("\n".join(lines))


def test_kernel_form_checks_its_arguments_and_names_the_forms(native):
    # mrx_kernel_form (include/mrx.h), as mrx_raster_entry and mrx_bvh_launch: argument checks before anything touches HIP
    import ctypes
    import re
    from tests.conftest import ROOT
    from tests.test_kernel_forms_cpu import FORMS
    lib = native.load_capi()
    lib.mrx_last_error.restype = ctypes.c_char_p
    lib.mrx_kernel_form.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    out = (ctypes.c_int32 * 2)()
    assert lib.mrx_kernel_form(None, ctypes.byref(out)) == -1 and b"null renderer" in lib.mrx_last_error()
    assert lib.mrx_kernel_form(None, None) == -1
    assert hasattr(native.load_module().MadronaRenderer, "kernel_form")
    # MRX_FORM_* are numbered as the resource table's legend and tests/test_kernel_forms_cpu.FORMS name the forms
    header = open(os.path.join(ROOT, "include", "mrx.h")).read()
    values = {n: int(v) for n, v in re.findall(r"MRX_FORM_(\w+) = (\d+)", header)}
    assert values == {name.upper(): i for i, name in enumerate(FORMS)}
