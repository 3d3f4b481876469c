#!/usr/bin/env python3
"""Cost of per-view projection, all in one process: for each shape, a renderer of default cameras,
one whose cameras share a non-default projection (uniform form: the kernel arguments) and one whose cameras differ
(per-view form: the 32-byte table) -- once with views a float ulp apart, which isolates the cost of the table from
that of different images, once with mixed fovs and near planes -- time_renders alternated round by round, median of
the rounds.

  python scripts/bench_projection.py [--rounds 5] [--steps 200] [--out profiles/r08_projection.json]
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
from tests import meshes  # noqa: E402
from tests import projection_oracle as po  # noqa: E402

SHAPES = {
    "headline 4096x64^2": lambda: scenes.synthetic_scene(4096),
    "configs[2] 1024x128^2+wall": lambda: scenes.synthetic_scene(1024, width=128, height=128, with_wall=True),
    "configs[4] 4096x256^2 rt": lambda: scenes.synthetic_scene(4096, width=256, height=256, render_mode="Raytracer"),
    "bvh 1024x482 tris": lambda: meshes.cube_field(num_worlds=1024, cubes=40),
}


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
        n = len(base.cameras)
        forms = {"default": base}
        uni = scenes.SceneDesc(**{k: getattr(base, k) for k in base.__dataclass_fields__})
        uni.camera_projections = [(60.0, None)] * n
        pv = scenes.SceneDesc(**{k: getattr(base, k) for k in base.__dataclass_fields__})
        pv.camera_projections = po.mixed(n)
        # the per-view form over the uniform one's images: 60 degrees in every view, every other view a float ulp wider
        # (the table differs from view to view, the pixels practically do not)
        pv60 = scenes.SceneDesc(**{k: getattr(base, k) for k in base.__dataclass_fields__})
        wide = float(np.nextafter(np.float32(60.0), np.float32(90.0)))
        pv60.camera_projections = [(60.0 if i % 2 == 0 else wide, None) for i in range(n)]
        forms["uniform60"], forms["per-view60"], forms["per-view"] = uni, pv60, pv
        rs = {k: scenes.make_renderer(d) for k, d in forms.items()}
        entry = {k: (r.raster_entry(), r.bvh_launch()["kernel"]) for k, r in rs.items()}
        for r in rs.values():
            r.time_renders(20)                    # warm-up of every instantiation the window uses
        us = {k: [] for k in rs}
        for _ in range(a.rounds):
            for k, r in rs.items():
                us[k].append(r.time_renders(a.steps) * 1000.0 / a.steps)
        med = {k: statistics.median(v) for k, v in us.items()}
        res[name] = {"us_median": med, "us_rounds": us, "entry": entry,
                     "per_view60_over_uniform60": med["per-view60"] / med["uniform60"] - 1.0,
                     "per_view_over_default": med["per-view"] / med["default"] - 1.0}
        print(json.dumps({name: res[name]}), flush=True)
        del rs
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
