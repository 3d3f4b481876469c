#!/usr/bin/env python3
"""The ray-cast sensor's trace stage, timed: the 4096 pinhole rays of every world's 64 x 64 view,
traced alone (trace()), against the depth-only render of the same views by a renderer without the sensor, in one
process -- on synthetic_scene (14 triangles a world, flat objects), cube_field(40) (41 rows a world) and mesh_worlds
(14,152 triangles a world behind three-level BLASes).  Prints one JSON line per workload; --out FILE also appends the
lines there (profiles/rays_latest.txt is made this way).

    python scripts/bench_rays.py [--worlds 1024] [--mesh-worlds 256] [--reps 20] [--brute] [--out FILE]
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
    ap.add_argument("--mesh-worlds", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--brute", action="store_true", help="the form of the kernel without any cull (MRX_RAYS_BRUTE=1)")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.brute:
        os.environ["MRX_RAYS_BRUTE"] = "1"

    import torch
    from madrona_renderer_amd import scenes
    from oracle import oracle
    from tests import meshes
    from tests import ray_oracle as ro

    workloads = [("synthetic_scene", scenes.synthetic_scene(args.worlds)),
                 ("cube_field_40", scenes.cube_field(args.worlds, 40)),
                 ("mesh_worlds", meshes.mesh_worlds(args.mesh_worlds))]
    lines = []
    for name, desc in workloads:
        fs = oracle.FlatScene(desc)
        W, R = desc.num_worlds, desc.width * desc.height
        rays = np.stack([ro.pinhole(fs, v, tmin=oracle.RASTER_ZNEAR) for v in range(W)])
        r = scenes.make_renderer(dataclasses.replace(desc, rays=R), render_outputs="Depth")
        plain = scenes.make_renderer(desc, render_outputs="Depth")
        t = r.ray_tensor().to_torch()
        t.copy_(torch.from_numpy(rays).to(t.device))
        r.sync()
        plain.sync()

        def timed(who, fn):
            who.mark(0)
            fn()
            who.mark(1)
            return who.elapsed_ms() * 1000.0

        for who, fn in ((r, r.trace), (plain, plain.render)):
            for _ in range(5):
                timed(who, fn)
        trace, render = [], []
        for _ in range(args.reps):
            trace.append(timed(r, r.trace))
            render.append(timed(plain, plain.render))
        hit = float((r.ray_id_tensor().to_torch() != -1).float().mean())
        tu, ru = statistics.median(trace), statistics.median(render)
        line = {"workload": name, "worlds": W, "rays_per_world": R, "brute": bool(args.brute),
                "trace_us": round(tu, 2), "ns_per_ray": round(tu * 1000.0 / (W * R), 4),
                "depth_render_us": round(ru, 2), "ratio": round(tu / ru, 3), "hit_share": round(hit, 4),
                "render_path": plain.raster_entry(), "max_world_triangles": int(fs.obj_num_tris[fs.inst_obj0[
                    fs.world_inst_start[0]:fs.world_inst_start[1]]].sum())}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del r, plain
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
