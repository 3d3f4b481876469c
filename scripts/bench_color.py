#!/usr/bin/env python3
"""Cost of the per-instance colour column, all in one process: for each shape, a renderer without
the column (off), one with the column allocated and no row overridden (the same images: the cost of the read alone),
one with three rows of four overridden, and one with those colours beside mixed lights (the table form) --
time_renders alternated round by round, median of the rounds, and the spread of the rounds beside it.

  python scripts/bench_color.py [--rounds 5] [--steps 200] [--forms off,zero,mixed,mixed-lights] [--out profiles/r10_color.json]

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

FORMS = ("off", "zero", "mixed", "mixed-lights")


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
        from tests import color_oracle as co
        from tests import light_oracle as lo
        colors = co.mixed(len(base.instances))
        if k == "zero":
            out[k] = _copy(base, instance_colors=True)
        elif k == "mixed":
            out[k] = _copy(base, instance_colors=colors)
        else:
            out[k] = _copy(base, instance_colors=colors, world_lights=lo.mixed(base.num_worlds))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--forms", default=",".join(FORMS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}
    for name in a.shapes.split(","):
        base = SHAPES[name]()
        rs = {k: scenes.make_renderer(dsc) for k, dsc in _forms(base, a.forms.split(",")).items()}
        entry = {k: (r.raster_entry(), r.bvh_launch()["kernel"]) for k, r in rs.items()}
        for r in rs.values():
            r.time_renders(20)                    # warm-up of every instantiation the window uses
        us = {k: [] for k in rs}
        for _ in range(a.rounds):
            for k, r in rs.items():
                us[k].append(r.time_renders(a.steps) * 1000.0 / a.steps)
        med = {k: statistics.median(v) for k, v in us.items()}
        spread = {k: (max(v) - min(v)) / statistics.median(v) for k, v in us.items()}
        res[name] = {"us_median": med, "us_rounds": us, "spread": spread, "entry": entry}
        for k in med:
            if k != "off" and "off" in med:
                res[name][k.replace("-", "_") + "_over_off"] = med[k] / med["off"] - 1.0
        print(json.dumps({name: res[name]}), flush=True)
        del rs
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
