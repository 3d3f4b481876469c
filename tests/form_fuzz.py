"""Shared by tests/test_form_fuzz_cpu.py and tests/test_form_fuzz_gpu.py (not collected): the form kernels of
DESIGN.md 4.17 on adversarial scenes under drawn launch shapes.

  scenes      `soup` (tests.test_fuzz_gpu._scene: eye-plane crossings, degenerate and coincident triangles, mirrored
              scales, rows bound to an object id outside the table), with and without textures; `uniform`
              (tests.uniform_worlds.uniform_scene, the FAST entry's batches); `mesh`
              (tests.meshes.mesh_scene_random_cameras: worlds of 2,816 triangles)
  recipes     per form the smallest and the largest set of tables, columns and outputs that selects it under 4.17's
              first-match rule (`recipes`), applied to a scene by `with_recipe`
  rule        `expected_form` restates 4.17 from the SceneDesc alone
  reference   `reference(desc, views)`: tests/material_oracle.render (materials, then colours, lights, projections)
              with the normals and the labelled segmask scattered through its tri_id
  CASES       one explicit table; every case names the row of profiles/kernel_resources_latest.txt it launches

The seeds below are among the first (soups from 100, uniform worlds from 10, mesh worlds from 300) whose compared
views meet the witnesses tests/test_form_fuzz_cpu.py asserts under the default, the common and the mixed projections,
with no soup world above 16 triangles; that module's docstring has the measured shares."""
import dataclasses
import functools
import os
import zlib
from collections import namedtuple

import numpy as np

from tests import color_oracle as co
from tests import label_oracle as lb
from tests import light_oracle as lo
from tests import material_oracle as mo
from tests import meshes
from tests import normal_oracle as no
from tests import projection_oracle as po
from tests import uniform_worlds as uw
from tests.test_kernel_forms_cpu import FORMS

GROUP_FORMS = ("PV", "PVL", "C", "PVLC", "M", "PVLM", "N", "NPV", "L", "LN")
TILE_FORMS = ("PV", "N", "NPV")                  # brute, chunked, BVH flat
BVH_TILE_FORMS = ("PV", "PVM", "N", "NPV")
FORM_TEMPLATES = ("rasterGroupFormKernel", "rasterGroupFormKernelFast", "rasterBruteFormKernel",
                  "rasterChunkedFormKernel", "bvhTileFormKernel", "bvhFlatFormKernel")

# ---- scenes -----------------------------------------------------------------------------------------------------------
# (kind, seed, width, height, mode).  Soups: 24 worlds, none of more than 16 triangles (the 16-slot group kernel),
# one-tile views (64 x 64, 37 x 53) and views of several tiles with tile tails (128 x 64, 96 x 130).
Scene = namedtuple("Scene", "kind seed width height mode")
SOUP_WORLDS, UNIFORM_WORLDS = 24, 130
SOUPS = (Scene("soup", 144, 64, 64, "Rasterizer"), Scene("soup", 109, 37, 53, "Rasterizer"),
         Scene("soup", 100, 128, 64, "Rasterizer"), Scene("soup", 144, 96, 130, "Rasterizer"))
SOUP_RT = Scene("soup", 109, 64, 64, "Raytracer")
UNIFORMS = (Scene("uniform", 10, 64, 64, "Rasterizer"), Scene("uniform", 11, 50, 30, "Rasterizer"))
MESH = Scene("mesh", 300, 48, 48, "Rasterizer")
MESH_RT = Scene("mesh", 300, 48, 48, "Raytracer")
# views compared with the reference, by pixels of a view: about 70,000 pixels per (scene, recipe)
COMPARED_PIXELS = 70000


def compared_views(scene, desc):
    return 0, max(1, min(desc.num_views, COMPARED_PIXELS // (scene.width * scene.height)))


def untextured(desc):
    """The same geometry without textures: no texture paths, every material's texture -1."""
    d = dataclasses.replace(desc)
    d.materials = [(c, -1, ro, me) for c, _, ro, me in desc.materials]
    d.texture_paths = []
    return d


@functools.lru_cache(maxsize=None)
def base_scene(scene, textured):
    if scene.kind == "soup":
        from tests.test_fuzz_gpu import _scene
        d = _scene(scene.seed, SOUP_WORLDS, scene.width, scene.height, scene.mode)
        return d if textured else untextured(d)
    if scene.kind == "uniform":
        return uw.uniform_scene(scene.seed, UNIFORM_WORLDS, scene.width, scene.height, scene.mode, textured=textured)
    assert scene.kind == "mesh" and not textured     # (its materials have no texture; a table brings one: with_recipe)
    return meshes.mesh_scene_random_cameras(scene.seed, scene.width, scene.height, scene.mode)


# ---- recipes ----------------------------------------------------------------------------------------------------------
# proj, light: None (the defaults), "same" (one non-default value for every view / world: the tables do not vary) or
# "mixed" (po.mixed / lo.mixed); color, mat, normals, labels: the column or output is there or not.
Recipe = namedtuple("Recipe", "proj light color mat normals labels", defaults=(None, None, False, False, False, False))
SAME_PROJ = (60.0, 0.5)
SAME_LIGHT = ((0.5, -0.25, -2.0), 0.1, 0.8)

_GROUP = {
    "PV": (Recipe(proj="mixed"), Recipe(proj="mixed", light="same")),
    "PVL": (Recipe(light="mixed"), Recipe(proj="mixed", light="mixed")),
    "C": (Recipe(color=True), Recipe(proj="same", light="same", color=True)),
    "PVLC": (Recipe(proj="mixed", color=True), Recipe(proj="mixed", light="mixed", color=True)),
    "M": (Recipe(mat=True), Recipe(proj="same", light="same", color=True, mat=True)),
    "PVLM": (Recipe(light="mixed", mat=True), Recipe(proj="mixed", light="mixed", color=True, mat=True)),
    "N": (Recipe(normals=True), Recipe(proj="same", light="same", color=True, mat=True, normals=True)),
    "NPV": (Recipe(proj="mixed", normals=True),
            Recipe(proj="mixed", light="mixed", color=True, mat=True, normals=True)),
    "L": (Recipe(labels=True), Recipe(proj="mixed", light="mixed", color=True, mat=True, labels=True)),
    "LN": (Recipe(normals=True, labels=True),
           Recipe(proj="mixed", light="mixed", color=True, mat=True, normals=True, labels=True)),
}
# The brute, chunked and flat kernels launch with the tables as soon as a column is there (4.17: `viewProj`), so their
# uniform normals form has no column; the tile kernel's PV has no material column (PVM comes first).  The label column
# is left to the caller: it needs the segmask (`with_labels`).
_TILE = {
    "PV": (Recipe(proj="mixed"), Recipe(proj="mixed", light="mixed", color=True, mat=True)),
    "N": (Recipe(normals=True), Recipe(proj="same", light="same", normals=True)),
    "NPV": (Recipe(color=True, normals=True), Recipe(proj="mixed", light="mixed", color=True, mat=True, normals=True)),
}
_BVH_TILE = dict(_TILE, PV=(Recipe(proj="mixed"), Recipe(proj="mixed", light="mixed", color=True)),
                 PVM=(Recipe(mat=True), Recipe(proj="mixed", light="mixed", color=True, mat=True)))


def recipes(form, family="group"):
    """(smallest, largest): the column sets that select `form` in `family` under 4.17's first-match rule."""
    return {"group": _GROUP, "brute": _TILE, "chunked": _TILE, "bvh-flat": _TILE, "bvh-tile": _BVH_TILE}[family][form]


def with_labels(recipe):
    return recipe._replace(labels=True)


def with_recipe(base, recipe, textured):
    """A copy of `base` with the tables, columns and outputs of `recipe`; the generators are the feature tests' own."""
    d = dataclasses.replace(base)
    n = len(base.instances)
    if recipe.mat:
        d = mo.with_table(d, textured=textured)
        d.instance_materials = mo.mixed(n, mo.num_materials(d), seed=4)
    if recipe.color:
        d.instance_colors = np.roll(co.mixed(n, seed=3), 2, axis=0)
    if recipe.light:
        d.world_lights = list(lo.mixed(base.num_worlds, shift=2)) if recipe.light == "mixed" else \
            [SAME_LIGHT] * base.num_worlds
    if recipe.proj:
        d.camera_projections = list(po.mixed(len(base.cameras))) if recipe.proj == "mixed" else \
            [SAME_PROJ] * len(base.cameras)
    if recipe.labels:
        d.instance_labels = lb.mixed(n, seed=4)
    d.normals = bool(recipe.normals)
    return d


@functools.lru_cache(maxsize=None)
def scene_desc(scene, textured, recipe):
    return with_recipe(base_scene(scene, textured and scene.kind != "mesh"), recipe, textured)


# ---- the rule of DESIGN.md 4.17, from the SceneDesc -------------------------------------------------------------------
def _tables(desc):
    """(tables vary, lights vary) as applyViewTables compares them: the values the renderer is given, as float32."""
    f32 = lambda x: float(np.float32(x))
    projs = {(f32(f), 0.0 if z is None else f32(z)) for f, z in po.view_projections(desc)}
    lights = {(tuple(f32(x) for x in d), f32(a), f32(f)) for d, a, f in lo.world_lights(desc)}
    return len(projs) > 1 or len(lights) > 1, len(lights) > 1


def expected_form(family, desc, ids, outputs=None):
    """The form name a launch of `family` ("group", "brute", "chunked", "bvh-tile", "bvh-flat") takes for `desc` with
    the ids tensor `ids` ("none", "visibility", "segmask") and the output selection `outputs`."""
    vary, light_table = _tables(desc)
    shades = outputs != "Depth"                      # a depth-only renderer never reads the colour or material column
    col = desc.instance_colors is not None and shades
    mat = desc.instance_materials is not None and shades
    lab = desc.instance_labels is not None and ids != "visibility"     # visibility ids win over the segmask
    nrm = bool(desc.normals)
    pv = vary or col or mat or lab                   # the tables are launched with: they vary, or a column needs them
    if family == "group":
        if lab and ids != "none" and pv:
            return "LN" if nrm else "L"
        if nrm:
            return "NPV" if pv and vary else "N"
        if mat:
            return "PVLM" if pv and vary else "M"
        if col:
            return "PVLC" if pv and vary else "C"
        if pv:
            return "PVL" if light_table else "PV"
        return "Uniform"
    assert family in ("brute", "chunked", "bvh-tile", "bvh-flat"), family
    if nrm:
        return "NPV" if pv else "N"
    if family == "bvh-tile" and pv and mat:
        return "PVM"
    return "PV" if pv else "Uniform"


def expected_textured(desc, outputs=None):
    """Does the launch take the textured instantiations: a drawn triangle's material has a texture that exists, or
    the renderer shades with a material column whose table holds one."""
    ntex = len(desc.texture_paths)
    textured_mat = [0 <= t < ntex for _, t, _, _ in desc.materials]
    if desc.instance_materials is not None and outputs != "Depth" and any(textured_mat):
        return True
    nobj = len(desc.asset_paths) + len(desc.mesh_materials)
    used = {o for ni, io, _, _ in desc.worlds for _, _, _, o in desc.instances[io:io + ni] if 0 <= o < nobj}
    for o in used:
        if o < len(desc.asset_paths):
            return None                              # (an asset's MTL decides: not worked out here)
        m = int(desc.mesh_materials[o - len(desc.asset_paths)])
        if 0 <= m < len(textured_mat) and textured_mat[m]:
            return True
    return False


def max_world_triangles(desc):
    """Triangles of the largest world (raw meshes; -1 when an asset is bound)."""
    if desc.asset_paths:
        return -1
    ioff = list(desc.mesh_indices_offsets) + [len(desc.mesh_indices)]
    tris = [(ioff[i + 1] - ioff[i]) // 3 for i in range(len(desc.mesh_materials))]
    return max(sum(tris[o] for _, _, _, o in desc.instances[io:io + ni] if 0 <= o < len(tris))
               for ni, io, _, _ in desc.worlds)


# ---- the reference ----------------------------------------------------------------------------------------------------
def reference(desc, views):
    """The images of views [a, b) of `desc` under its own tables and columns, indexed from 0: rgb, depth, tri_id,
    segmask (labelled where the desc has the column), and normals where it has the output."""
    from oracle import oracle
    a, b = views
    ref = mo.render(desc, view_begin=a, view_end=b, want_ids=True)
    out = {k: ref[k][a:b] for k in ("rgb", "depth", "tri_id", "segmask")}
    fs = oracle.FlatScene(desc)
    if desc.instance_labels is not None:
        out["segmask"] = lb.segmask(fs, lb.expand(desc), ref["tri_id"], a, b)
    if desc.normals:
        out["normals"] = no.normals(fs, ref["tri_id"], a, b)
    return out


@functools.lru_cache(maxsize=None)
def cached_reference(scene, textured, recipe):
    """`reference` of the compared views, once per (scene, recipe): slots, ids and launch shapes do not change it."""
    desc = scene_desc(scene, textured, recipe)
    ref = reference(desc, compared_views(scene, desc))
    for v in ref.values():
        v.setflags(write=False)
    return ref


# ---- witnesses (CPU) --------------------------------------------------------------------------------------------------
def near_crossing_views(desc, tri_id, views):
    """How many of the views [a, b) show a winning triangle that crosses the view's own near plane (float64, the
    camera-space forward coordinate as tests/uniform_worlds.edge_counts takes it); tri_id indexed from 0."""
    from oracle import oracle
    fs = oracle.FlatScene(desc)
    projs = po.view_projections(desc)
    dflt = uw.RT_NEAR if fs.raytracer else uw.RASTER_NEAR
    count = 0
    for v in range(*views):
        ids = tri_id[v - views[0]]
        won = np.unique(ids[ids >= 0])
        if not len(won):
            continue
        tris = uw.world_triangles(fs, int(fs.view_world[v]))
        near = dflt if projs[v][1] is None else float(np.float32(projs[v][1]))
        Rc = uw._quat_mat(fs.cam_rot[v])
        eye = fs.cam_pos[v].astype(np.float64)
        for k in won:
            i, t = tris[int(k)]
            M = uw._quat_mat(fs.inst_rot[i]) * fs.inst_scale[i].astype(np.float64)[None, :]
            y = ((fs.tri_pos[t].astype(np.float64) @ M.T + fs.inst_pos[i].astype(np.float64)) - eye) @ Rc[:, 1]
            if y.min() < near < y.max():
                count += 1
                break
    return count


def normal_sides(desc, tri_id, views):
    """(covered pixels whose triangle has d > 0, those with d < 0): both branches of S10's sign rule."""
    from oracle import oracle
    fs = oracle.FlatScene(desc)
    pos = neg = 0
    for v in range(*views):
        ids = tri_id[v - views[0]]
        hit = ids[ids >= 0]
        if len(hit):
            d = no.view_geometry(fs, v)[1][hit]
            pos += int((d > 0).sum())
            neg += int((d < 0).sum())
    return pos, neg


# ---- the case table ---------------------------------------------------------------------------------------------------
# family: group, group-fast, brute, chunked, bvh-tile, bvh-flat.  ids: none, visibility, segmask.  shape: the group
# kernel's slots, or the tile kernel's (TW, TH, CLS, MULTI), else None.  env: the launch-shape knobs, drawn per case.
# outputs: None (rgb and depth), "Depth" or "RGB".  row: the instantiation as profiles/kernel_resources_latest.txt
# spells it.
Case = namedtuple("Case", "name family form recipe scene ids textured shape variant env outputs row")
VARIANT = {"group": None, "group-fast": None, "brute": 1, "chunked": 3, "bvh-tile": 2, "bvh-flat": 2}
RULE_FAMILY = {"group-fast": "group"}
ENTRY = {"group": ("group", "none"), "group-fast": ("group-fast", "none"), "brute": ("brute", "none"),
         "chunked": ("chunked", "none"), "bvh-tile": ("bvh", "tile"), "bvh-flat": ("bvh", "flat")}
TILE_SHAPES = ((64, 64, False, False), (64, 64, True, False), (64, 64, False, True), (64, 64, True, True),
               (64, 32, False, False), (32, 32, False, False))


def _b(x):
    return "true" if x else "false"


def _row(template, form, *args):
    return "%s<(mrx::KernelForm)%d, %s>" % (template, FORMS.index(form), ", ".join(
        _b(a) if isinstance(a, bool) else str(a) for a in args))


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _outputs(rng, recipe):
    """One case in five renders depth only or rgb only -- rgb only where the recipe has a colour or material column:
    a depth-only renderer never reads them, and launches another form (tests/test_form_fuzz_cpu.py checks the rule
    under the selection too)."""
    if rng.integers(0, 5) != 0:
        return None
    pick = ("Depth", "RGB")[int(rng.integers(0, 2))]
    return "RGB" if recipe.color or recipe.mat else pick


def _group_env(rng, slots):
    env = {"MRX_DEBUG_SLOTS": str(slots)}
    if rng.integers(0, 2):
        env["MRX_GROUP_VIEWS"] = str((1, 2, 4)[int(rng.integers(0, 3))])
        env["MRX_XCD_SKEW"] = str(int(rng.integers(0, 8)))
        env["MRX_XCD_ROTATE"] = str(int(rng.integers(0, 2)))
    else:
        env["MRX_GROUP_TILES"] = str(int(rng.integers(1, 17)))
    if rng.integers(0, 4) == 0:
        env["MRX_WRITE_THROUGH"] = "0"
    return env


def _bvh_env(rng, shape, scene):
    tw, th, cls, multi = shape
    env = {"MRX_BVH_FLAT": "0", "MRX_BVH_TILE": str(0 if th == 64 else 1 if tw == 64 else 2),
           "MRX_BVH_CLASSIFY": "1" if cls else "0",
           "MRX_BVH_SMALL_AREA": str((0, 8, 200, 4096)[int(rng.integers(0, 4))]),
           "MRX_BVH_GROUP_VIEWS": str((2, 4, 8)[int(rng.integers(0, 3))] if multi else 1)}
    if rng.integers(0, 2):
        env["MRX_BVH_PASS_INST"] = str((8, 16, 64)[int(rng.integers(0, 2 if multi else 3))])   # (MULTI: a block per view)
    if rng.integers(0, 2):
        env["MRX_BVH_TEX_CAP"] = str((64, 96, 256)[int(rng.integers(0, 3))])
    if scene.kind == "mesh":
        env.pop("MRX_BVH_PASS_INST", None)
    return env


def _ids_recipe(recipe, form, ids, scene):
    """A segmask in Rasterizer mode comes with the label column; where the form allows a column it goes along in
    Raytracer mode too."""
    if ids == "segmask" and (scene.mode != "Raytracer" or form != "N"):
        return with_labels(recipe)
    return recipe


def _cases():
    out = []

    def add(family, form, recipe, scene, ids, textured, shape, env, row, tag=""):
        name = "-".join(str(x) for x in (family, form, scene.kind, "%dx%d" % (scene.width, scene.height), ids,
                                         "tex" if textured else "notex", tag) if x != "")
        rng = _rng(name + "/outputs")
        outputs = _outputs(rng, recipe)
        out.append(Case(name, family, form, recipe, scene, ids, textured, shape, VARIANT[family], env, outputs, row))

    # group kernel, plain entry: form x slots x ids x textured on soups
    for fi, form in enumerate(GROUP_FORMS):
        for textured in (True, False):
            scene = SOUPS[(fi + int(textured)) % len(SOUPS)]
            for si, slots in enumerate((16, 32, 64, 128, 256)):
                for ii, ids in enumerate(("segmask",) if form in ("L", "LN") else ("none", "visibility")):
                    recipe = recipes(form)[(si + ii) % 2]
                    tag = "s%d" % slots
                    env = _group_env(_rng("group/%s/%s/%s/%s" % (form, textured, slots, ids)), slots)
                    add("group", form, recipe, scene, ids, textured, slots, env,
                        _row("rasterGroupFormKernel", form, ids != "none", slots, textured), tag)
    # group kernel, FAST entry: form x ids x textured on uniform worlds
    for fi, form in enumerate(GROUP_FORMS):
        for textured in (True, False):
            for ii, ids in enumerate(("segmask",) if form in ("L", "LN") else ("none", "visibility")):
                rng = _rng("fast/%s/%s/%s" % (form, textured, ids))
                scene = UNIFORMS[(fi + ii) % 2]
                env = {"MRX_GROUP_VIEWS": str((1, 2, 4)[int(rng.integers(0, 3))]),
                       "MRX_XCD_SKEW": str(int(rng.integers(0, 8))), "MRX_XCD_PHASE": str(int(rng.integers(0, 2)))}
                add("group-fast", form, recipes(form)[(fi + ii + int(textured)) % 2], scene, ids, textured, 16, env,
                    _row("rasterGroupFormKernelFast", form, ids != "none", textured))
    # brute: both sides of the chunk loop's threshold (soups of at most 16 triangles, mesh worlds of 2,816)
    for form in TILE_FORMS:
        for ii, ids in enumerate(("none", "visibility")):
            for multi, scene in ((False, SOUPS[1]), (True, MESH)):
                add("brute", form, recipes(form, "brute")[(ii + int(multi)) % 2], scene, ids, False, None, {},
                    _row("rasterBruteFormKernel", form, ids != "none", multi))
    # chunked: mesh worlds
    for fi, form in enumerate(TILE_FORMS):
        for ii, ids in enumerate(("none", "visibility")):
            add("chunked", form, recipes(form, "chunked")[(fi + ii) % 2], MESH, ids, False, None, {},
                _row("rasterChunkedFormKernel", form, ids != "none"))
    # BVH tile kernel: form x ids x textured x tile shape on soups; the untextured classifying shapes on mesh worlds too
    for fi, form in enumerate(BVH_TILE_FORMS):
        for ii, ids in enumerate(("none", "visibility", "segmask")):
            for textured in (True, False):
                for hi, shape in enumerate(TILE_SHAPES):
                    if form == "NPV" and textured and shape[2]:
                        continue                     # (no classifying instantiation: tileFormClassifies)
                    scene = SOUP_RT if ids == "segmask" and (fi + hi) % 2 else SOUPS[(hi + ii) % 2] if shape[3] else \
                        SOUPS[(fi + hi + ii) % len(SOUPS)]
                    recipe = _ids_recipe(recipes(form, "bvh-tile")[(hi + ii + int(textured)) % 2], form, ids, scene)
                    if form == "N" and ids == "segmask":
                        scene = SOUP_RT              # (no column: the segmask is Raytracer mode's)
                        recipe = recipes(form, "bvh-tile")[(hi + int(textured)) % 2]
                    tag = "%dx%d%s%s" % (shape[0], shape[1], "c" if shape[2] else "", "m" if shape[3] else "")
                    env = _bvh_env(_rng("tile/%s/%s/%s/%s" % (form, ids, textured, tag)), shape, scene)
                    add("bvh-tile", form, recipe, scene, ids, textured, shape, env,
                        _row("bvhTileFormKernel", form, ("none", "visibility", "segmask").index(ids), textured,
                             *shape), tag)
    for fi, form in enumerate(BVH_TILE_FORMS):
        for ii, ids in enumerate(("visibility", "segmask")):
            shape = TILE_SHAPES[1 if ii == 0 else 0]
            scene = MESH_RT if ids == "segmask" else MESH
            recipe = _ids_recipe(recipes(form, "bvh-tile")[(fi + ii) % 2], form, ids, scene)
            tag = "%dx%d%s" % (shape[0], shape[1], "c" if shape[2] else "")
            env = _bvh_env(_rng("tile-mesh/%s/%s" % (form, ids)), shape, scene)
            add("bvh-tile", form, recipe, scene, ids, False, shape, env,
                _row("bvhTileFormKernel", form, ("none", "visibility", "segmask").index(ids), False, *shape), tag)
    # BVH flat kernel: form x ids x textured on soups (each also against the tile kernel's bytes)
    for fi, form in enumerate(TILE_FORMS):
        for ii, ids in enumerate(("none", "visibility", "segmask")):
            for textured in (True, False):
                scene = SOUP_RT if ids == "segmask" else SOUPS[(fi + ii + int(textured)) % len(SOUPS)]
                recipe = _ids_recipe(recipes(form, "bvh-flat")[(fi + ii + int(textured)) % 2], form, ids, scene)
                rng = _rng("flat/%s/%s/%s" % (form, ids, textured))
                env = {"MRX_BVH_SMALL_AREA": str((0, 8, 200, 4096)[int(rng.integers(0, 4))])}
                if rng.integers(0, 2):
                    env["MRX_BVH_GROUP_TILES"] = str(int(rng.integers(1, 5)))
                add("bvh-flat", form, recipe, scene, ids, textured, None, env,
                    _row("bvhFlatFormKernel", form, ("none", "visibility", "segmask").index(ids), textured))
    return out


CASES = _cases()
# Form-kernel rows no case launches, each with its reason.  None for the two group templates; at most a tenth of any
# other template's rows.
UNREACHED = []


def cases_of(family, **match):
    return [c for c in CASES if c.family == family and all(getattr(c, k) == v for k, v in match.items())]


def resource_rows():
    """The form-kernel rows of profiles/kernel_resources_latest.txt, as `Case.row` spells them."""
    import re
    from tests.conftest import ROOT
    rows = []
    for line in open(os.path.join(ROOT, "profiles", "kernel_resources_latest.txt")):
        m = re.match(r"((\w+)<[^>]*>)", line)
        if m and m.group(2) in FORM_TEMPLATES:
            rows.append(m.group(1))
    return rows
