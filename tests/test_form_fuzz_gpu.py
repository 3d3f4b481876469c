"""Every form-kernel instantiation against the composed oracle on adversarial scenes (-m gpu).

tests/form_fuzz.CASES names, for each of the 390 form-kernel rows of profiles/kernel_resources_latest.txt, a scene
(triangle soups with rows bound outside the object table, adversarial uniform worlds, mesh worlds), a recipe of tables,
columns and outputs that selects the form, the ids tensor, a slot count or tile shape and a launch shape drawn per
case.  Every case asserts the entry (raster_entry, bvh_launch), the instantiation (kernel_form: form and slots;
bvh_launch: textured, tile, classify, group_views) and compares with form_fuzz.reference: rgb, ids / segmask and
normals bit for bit, depth as tests.util.assert_parity has it (1 ulp and 1e-4).  One case in five selects depth only
or rgb only: the tensors that exist are compared, the missing one raises.  tests/test_form_fuzz_cpu.py holds that the
table covers the rows and that the references decide pixels."""
import contextlib
import os

import numpy as np
import pytest

from tests import form_fuzz as ff
from tests.test_projection_gpu import _make
from tests.util import assert_parity, depth_ulps

pytestmark = pytest.mark.gpu

KNOBS = ("MRX_DEBUG_SLOTS", "MRX_GROUP_VIEWS", "MRX_GROUP_TILES", "MRX_XCD_SKEW", "MRX_XCD_ROTATE", "MRX_XCD_PHASE",
         "MRX_WRITE_THROUGH", "MRX_GROUP_FAST", "MRX_BVH_FLAT", "MRX_BVH_TILE", "MRX_BVH_CLASSIFY", "MRX_BVH_SMALL_AREA",
         "MRX_BVH_GROUP_VIEWS", "MRX_BVH_GROUP_TILES", "MRX_BVH_PASS_INST", "MRX_BVH_TEX_CAP")


@contextlib.contextmanager
def _knobs(env):
    """The process environment with exactly the launch-shape knobs of `env`."""
    assert set(env) <= set(KNOBS), env
    old = {k: os.environ.pop(k, None) for k in KNOBS + ("MRX_PLACEMENT_TRIES",)}
    os.environ.update(env)
    os.environ["MRX_PLACEMENT_TRIES"] = "1"               # (no search for where the outputs land: it changes no byte)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _renderer(case, **more):
    desc = ff.scene_desc(case.scene, case.textured, case.recipe)
    with _knobs(dict(case.env, **more)):
        r = _make(desc, visibility=case.ids == "visibility", variant=case.variant, outputs=case.outputs)
        r.sync()
    return r, desc


def _fetch(r, case, desc, views):
    """The compared views of every tensor the case's renderer has, oracle layout; a tensor it has not raises."""
    a, b = views
    out = {}
    for name, tensor, missing in (("rgb", r.rgb_tensor, "Depth"), ("depth", r.depth_tensor, "RGB")):
        if case.outputs == missing:
            with pytest.raises(RuntimeError, match="not rendered"):
                tensor()
            continue
        out[name] = tensor().to_torch()[a:b].cpu().numpy()
    if "depth" in out:
        out["depth"] = out["depth"].reshape(out["depth"].shape[:3])
    if case.ids == "visibility":
        out["tri_id"] = r.visibility_tensor().to_torch()[a:b].cpu().numpy()
    elif case.ids == "segmask":
        out["segmask"] = r.segmask_tensor().to_torch()[a:b].cpu().numpy()
    if desc.normals:
        out["normals"] = r.normal_tensor().to_torch()[a:b].cpu().numpy()
    return out


def _compare(got, ref, name):
    for k in ("tri_id", "segmask", "normals"):
        if k in got:
            assert got[k].shape == ref[k].shape, (name, k)
            bad = int((got[k] != ref[k]).sum())
            assert bad == 0, f"{name}: {bad} values differ in {k}"
    if "rgb" in got and "depth" in got:
        assert_parity({k: got[k] for k in ("rgb", "depth")}, ref)
    elif "rgb" in got:
        bad = int((got["rgb"] != ref["rgb"]).any(axis=-1).sum())
        assert bad == 0, f"{name}: {bad} pixels differ in colour"
    else:                                                  # (assert_parity's depth half)
        np.testing.assert_allclose(got["depth"], ref["depth"], rtol=1e-4, atol=0)
        ulps = depth_ulps(got["depth"], ref["depth"])
        assert ulps <= 1, f"{name}: depth differs by {ulps} ulp (bound 1)"


def _same_bytes(a, b, name):
    assert a.keys() == b.keys(), name
    for k in a:
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), (name, k)


def _assert_launch(r, case, family=None):
    family = family or case.family
    entry, bvh = ff.ENTRY[family]
    launch = r.bvh_launch()
    assert r.raster_entry() == entry and launch["kernel"] == bvh, (case.name, r.raster_entry(), launch["kernel"])
    slots = case.shape if family in ("group", "group-fast") else 0
    assert r.kernel_form() == {"form": case.form, "slots": slots}, (case.name, r.kernel_form())
    assert launch["textured"] == case.textured, case.name
    if family == "bvh-tile":
        tw, th, cls, multi = case.shape
        assert launch["tile"] == (tw, th) and launch["classify"] == cls, (case.name, launch)
        assert launch["group_views"] == int(case.env["MRX_BVH_GROUP_VIEWS"]) and (launch["group_views"] > 1) == multi, \
            (case.name, launch)


def _run(case, family=None, **more):
    r, desc = _renderer(case, **more)
    _assert_launch(r, case, family)
    views = ff.compared_views(case.scene, desc)
    got = _fetch(r, case, desc, views)
    print("%-58s %-5s slots %3d %s" % (case.name, r.kernel_form()["form"], r.kernel_form()["slots"], case.row))
    return got


def _check(case):
    got = _run(case)
    _compare(got, ff.cached_reference(case.scene, case.textured, case.recipe), case.name)
    return got


def _ids(xs):
    return ["-".join(str(x) for x in t) for t in xs]


FORM_TEX = [(form, textured, ids) for form in ff.GROUP_FORMS for textured in (True, False)
            for ids in (("segmask",) if form in ("L", "LN") else ("none", "visibility"))]


@pytest.mark.parametrize("form,textured,ids", FORM_TEX, ids=_ids(FORM_TEX))
def test_group_forms_at_every_slot_count(native, oracle_mod, form, textured, ids):
    # (the soups are no uniform worlds: 16 slots are the plain entry's too; both recipes of the form alternate)
    cases = ff.cases_of("group", form=form, textured=textured, ids=ids)
    assert [c.shape for c in cases] == [16, 32, 64, 128, 256] and len({c.recipe for c in cases}) == 2
    for case in cases:
        _check(case)


@pytest.mark.parametrize("form,textured,ids", FORM_TEX, ids=_ids(FORM_TEX))
def test_group_forms_on_the_fast_entry(native, oracle_mod, form, textured, ids):
    cases = ff.cases_of("group-fast", form=form, textured=textured, ids=ids)
    assert len(cases) == 1
    for case in cases:
        got = _check(case)
        # the plain entry stores the same bytes
        _same_bytes(_run(case, family="group", MRX_GROUP_FAST="0"), got, case.name)


@pytest.mark.parametrize("form", ff.TILE_FORMS)
def test_brute_forms_on_both_sides_of_the_chunk_loop(native, oracle_mod, form):
    cases = ff.cases_of("brute", form=form)
    assert len(cases) == 4
    for case in cases:
        _check(case)


@pytest.mark.parametrize("form", ff.TILE_FORMS)
def test_chunked_forms(native, oracle_mod, form):
    for case in ff.cases_of("chunked", form=form):
        _check(case)


TILE = [(form, ids, textured) for form in ff.BVH_TILE_FORMS for ids in ("none", "visibility", "segmask")
        for textured in (True, False)]


@pytest.mark.parametrize("form,ids,textured", TILE, ids=_ids(TILE))
def test_bvh_tile_forms_at_every_tile_shape(native, oracle_mod, form, ids, textured):
    cases = ff.cases_of("bvh-tile", form=form, ids=ids, textured=textured)
    assert {c.shape for c in cases} == {s for s in ff.TILE_SHAPES if not (form == "NPV" and textured and s[2])}
    for case in cases:
        _check(case)


FLAT = [(form, textured) for form in ff.TILE_FORMS for textured in (True, False)]


@pytest.mark.parametrize("form,textured", FLAT, ids=_ids(FLAT))
def test_bvh_flat_forms_and_the_tile_kernel_on_the_same_scene(native, oracle_mod, form, textured):
    for case in ff.cases_of("bvh-flat", form=form, textured=textured):
        got = _check(case)
        # (the tile kernel has a form of its own for the material column)
        desc = ff.scene_desc(case.scene, case.textured, case.recipe)
        tile = _run(case._replace(shape=(64, 64, False, False), env=dict(case.env, MRX_BVH_GROUP_VIEWS="1"),
                                  form=ff.expected_form("bvh-tile", desc, case.ids, case.outputs)),
                    family="bvh-tile", MRX_BVH_FLAT="0", MRX_BVH_GROUP_VIEWS="1", MRX_BVH_CLASSIFY="0")
        _same_bytes(tile, got, case.name)
