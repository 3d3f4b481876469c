#!/usr/bin/env python3
"""Cost of the per-instance material column, all in one process: for each shape, a renderer without
the column (off), one with the column at -1 over a table without textured materials (unset: the same images, the cost
of the read alone), one with three rows of four overridden from that table (mixed-untextured), and one with three rows
of four overridden from a table with textured materials (mixed-textured: the textured kernels) -- time_renders
alternated round by round, median of the rounds, and the spread of the rounds beside it.

Then the comparison the column exists for (--swap, on by default with every form): 4096 worlds of 64x64 whose cube
shows one of three textures per world, (a) as three cube objects imported with three materials and bound per world --
the worlds are no longer uniform -- and (b) as one cube object and the column; both time per render, the raster entry
each reached, and whether their images are the same.

  python scripts/bench_material.py [--rounds 5] [--steps 200] [--forms off,unset,mixed-untextured,mixed-textured]
                                   [--no-swap] [--out profiles/r11_material.json]

--forms off alone runs on a build without the feature too: the baseline the off column is compared with.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from madrona_renderer_amd import scenes  # noqa: E402
from scripts.bench_projection import SHAPES  # noqa: E402

FORMS = ("off", "unset", "mixed-untextured", "mixed-textured")


def _copy(desc, **kw):
    d = scenes.SceneDesc(**{k: getattr(desc, k) for k in desc.__dataclass_fields__})
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _forms(base, names):
    out = {}
    for k in names:
        if k == "off":
            out[k] = base
            continue
        from tests import material_oracle as mo
        bare, full = mo.with_table(base, textured=False), mo.with_table(base)
        if k == "unset":
            out[k] = _copy(bare, instance_materials=True)
        elif k == "mixed-untextured":
            out[k] = _copy(bare, instance_materials=mo.mixed(len(base.instances), len(bare.materials)))
        else:
            out[k] = _copy(full, instance_materials=mo.mixed(len(base.instances), len(full.materials)))
    return out


def _timed(rs, rounds, steps):
    for r in rs.values():
        r.time_renders(20)                    # warm-up of every instantiation the window uses
    us = {k: [] for k in rs}
    for _ in range(rounds):
        for k, r in rs.items():
            us[k].append(r.time_renders(steps) * 1000.0 / steps)
    med = {k: statistics.median(v) for k, v in us.items()}
    spread = {k: (max(v) - min(v)) / statistics.median(v) for k, v in us.items()}
    return {"us_median": med, "us_rounds": us, "spread": spread}


def _swap_descs(num_worlds=4096):
    """(a) three cube objects with three textured materials, bound per world; (b) one cube object and the column."""
    from tests import material_oracle as mo
    base = mo.with_table(scenes.synthetic_scene(num_worlds, textured=True))
    nm = len(base.materials)
    three = [nm - 3, nm - 2, nm - 1]
    cube = base.asset_paths[0][0]
    # objects: 0 cube (first texture), 1 plane, 2 and 3 the cube again with the other two
    a = _copy(base, asset_paths=[(cube, three[0]), base.asset_paths[1], (cube, three[1]), (cube, three[2])])
    inst = list(base.instances)
    mats = [-1] * len(inst)
    for w, (ni, io, _, _) in enumerate(base.worlds):
        for i in range(io, io + ni):
            if inst[i][3] == 0:
                p, q, s, _ = inst[i]
                inst[i] = (p, q, s, (0, 2, 3)[w % 3])
                mats[i] = three[w % 3]
    a.instances = inst
    b = _copy(base, asset_paths=[(cube, three[0]), base.asset_paths[1]], instance_materials=mats)
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--forms", default=",".join(FORMS))
    ap.add_argument("--no-swap", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    names = a.forms.split(",")
    res = {}
    for name in [s for s in a.shapes.split(",") if s]:
        base = SHAPES[name]()
        rs = {k: scenes.make_renderer(dsc) for k, dsc in _forms(base, names).items()}
        res[name] = _timed(rs, a.rounds, a.steps)
        res[name]["entry"] = {k: (r.raster_entry(), r.bvh_launch()["kernel"], r.bvh_launch()["textured"]) for k, r in rs.items()}
        med = res[name]["us_median"]
        for k in med:
            if k != "off" and "off" in med:
                res[name][k.replace("-", "_") + "_over_off"] = med[k] / med["off"] - 1.0
        print(json.dumps({name: res[name]}), flush=True)
        del rs
    if not a.no_swap and set(names) == set(FORMS):
        da, db = _swap_descs()
        rs = {"three-objects": scenes.make_renderer(da), "column": scenes.make_renderer(db)}
        key = "swap 4096x64^2, one of three textures per world"
        res[key] = _timed(rs, a.rounds, a.steps)
        res[key]["entry"] = {k: (r.raster_entry(), r.bvh_launch()["kernel"], r.bvh_launch()["textured"]) for k, r in rs.items()}
        for r in rs.values():
            r.sync()
        x, y = (r.rgb_tensor().to_torch() for r in rs.values())
        res[key]["images_equal"] = bool((x == y).all())
        med = res[key]["us_median"]
        res[key]["column_over_three_objects"] = med["column"] / med["three-objects"] - 1.0
        print(json.dumps({key: res[key]}), flush=True)
        del rs
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
