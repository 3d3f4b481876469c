#!/usr/bin/env python3
"""Cost of per-world lights, all in one process: for each shape, a renderer of default lights, one
whose worlds share a non-default light (uniform form: the kernel arguments), one whose lights differ by a float ulp
of the ambient term in every other world (table form over the default's images: the cost of the table alone), one of
mixed lights (table form), and one of default lights and mixed projections (the per-view instantiations with the
projection table live and the light table uniform) -- time_renders alternated round by round, median of the rounds,
and the spread of the rounds beside it.

  python scripts/bench_light.py [--rounds 5] [--steps 200] [--out profiles/r09_light.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from madrona_renderer_amd import scenes  # noqa: E402
from scripts.bench_projection import SHAPES  # noqa: E402
from tests import light_oracle as lo  # noqa: E402
from tests import projection_oracle as po  # noqa: E402


def _copy(desc, **kw):
    d = scenes.SceneDesc(**{k: getattr(desc, k) for k in desc.__dataclass_fields__})
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}
    for name in a.shapes.split(","):
        base = SHAPES[name]()
        n = base.num_worlds
        d, amb, dif = lo.DEFAULT
        ulp = float(np.nextafter(np.float32(amb), np.float32(1.0)))
        forms = {
            "default": base,
            "uniform": _copy(base, world_lights=[((0.0, 0.0, -1.0), 0.1, 0.9)] * n),
            "table-same-images": _copy(base, world_lights=[(d, amb if w % 2 == 0 else ulp, dif) for w in range(n)]),
            "table-mixed": _copy(base, world_lights=lo.mixed(n)),
            "pv-projections-only": _copy(base, camera_projections=po.mixed(len(base.cameras))),
        }
        rs = {k: scenes.make_renderer(dsc) for k, dsc in forms.items()}
        entry = {k: (r.raster_entry(), r.bvh_launch()["kernel"]) for k, r in rs.items()}
        for r in rs.values():
            r.time_renders(20)                    # warm-up of every instantiation the window uses
        us = {k: [] for k in rs}
        for _ in range(a.rounds):
            for k, r in rs.items():
                us[k].append(r.time_renders(a.steps) * 1000.0 / a.steps)
        med = {k: statistics.median(v) for k, v in us.items()}
        spread = {k: (max(v) - min(v)) / statistics.median(v) for k, v in us.items()}
        res[name] = {"us_median": med, "us_rounds": us, "spread": spread, "entry": entry,
                     "table_same_images_over_default": med["table-same-images"] / med["default"] - 1.0,
                     "table_mixed_over_default": med["table-mixed"] / med["default"] - 1.0,
                     "uniform_over_default": med["uniform"] / med["default"] - 1.0}
        print(json.dumps({name: res[name]}), flush=True)
        del rs
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
