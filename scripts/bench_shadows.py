#!/usr/bin/env python3
"""The shadow stage, timed: cast() -- one any-hit ray per pixel of every world's 64 x 64 view -- against
trace() of the ray-cast sensor with as many rays (the pinhole rays of the same views), on one renderer, in one process,
alternating; and the cost of apply: a step of a normals=True renderer with apply=True minus one with apply=False.
Prints one JSON line per workload; --out FILE also appends the lines there (profiles/shadow_latest.txt is made this
way).

    python scripts/bench_shadows.py [--worlds 1024] [--reps 20] [--brute] [--out FILE]
"""
import argparse
import dataclasses
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--brute", action="store_true", help="the form of the kernel without any cull (MRX_SHADOW_BRUTE=1)")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.brute:
        os.environ["MRX_SHADOW_BRUTE"] = "1"

    import torch
    from madrona_renderer_amd import scenes, shadows
    from oracle import oracle
    from tests import ray_oracle as ro

    def timed(who, fn):
        who.mark(0)
        fn()
        who.mark(1)
        return who.elapsed_ms() * 1000.0

    def alternate(pairs):
        for who, fn in pairs:
            for _ in range(5):
                timed(who, fn)
        out = [[] for _ in pairs]
        for _ in range(args.reps):
            for k, (who, fn) in enumerate(pairs):
                out[k].append(timed(who, fn))
        return [statistics.median(x) for x in out]

    desc = scenes.synthetic_scene(args.worlds)
    fs = oracle.FlatScene(desc)
    W, R = desc.num_worlds, desc.width * desc.height
    lines = []

    # cast() against trace(), one renderer
    rays = np.stack([ro.pinhole(fs, v, tmin=oracle.RASTER_ZNEAR) for v in range(W)])
    r = scenes.make_renderer(dataclasses.replace(desc, rays=R), render_outputs="Depth")
    t = r.ray_tensor().to_torch()
    t.copy_(torch.from_numpy(rays).to(t.device))
    sh = shadows.attach(r, apply=False)
    r.sync()
    cast, trace = alternate([(r, sh.cast), (r, r.trace)])
    lines.append({"workload": "synthetic_scene", "what": "cast vs trace", "worlds": W, "rays_per_world": R,
                  "brute": bool(args.brute), "cast_us": round(cast, 2), "trace_us": round(trace, 2),
                  "ratio": round(cast / trace, 3), "ns_per_shadow_ray": round(cast * 1000.0 / (W * R), 4),
                  "occluded_share": round(float((sh.mask_tensor() == 0).float().mean()), 4),
                  "hit_share": round(float((r.depth_tensor().to_torch() > 0).float().mean()), 4)})
    print(json.dumps(lines[-1]), flush=True)
    del r, sh, t

    # the cost of apply: whole steps of two renderers with normals
    with_normals = dataclasses.replace(desc, normals=True)
    ra, rm, plain = (scenes.make_renderer(with_normals) for _ in range(3))
    shadows.attach(ra, apply=True)
    shadows.attach(rm, apply=False)
    for x in (ra, rm, plain):
        x.sync()
    a, m, p = alternate([(ra, ra.render), (rm, rm.render), (plain, plain.render)])
    lines.append({"workload": "synthetic_scene", "what": "step with normals", "worlds": W, "brute": bool(args.brute),
                  "step_apply_us": round(a, 2), "step_mask_us": round(m, 2), "step_without_us": round(p, 2),
                  "apply_cost_us": round(a - m, 2), "stage_cost_us": round(m - p, 2)})
    print(json.dumps(lines[-1]), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
