#!/usr/bin/env python3
"""Kernel time of each output selection (RGBD, Depth, RGB: Manager::RenderOutputs) on the shapes
that matter, one JSON line per (configuration, setting):

  python scripts/bench_outputs.py [--rounds 5] [--budget-ms 30] [--only headline,c2,...] [--normals] [--labels]
                                  [--root TREE] [--supersample N[,N...]] [--positions]
                                  [--observations CHANNELS[,DTYPE[,STACK]]]

--normals times RGBD+N, Depth+N and RGB+N (the surface-normal output beside each selection) beside the
three settings, in the same alternation; without it the script does what it always did.
--labels times RGBD+V (the ids tensor holding visibility ids: in Rasterizer mode the renderer that writes the same
12 B/px without labels) and RGBD+L (mixed labels in the label column, DESIGN.md 4.16: the segmask in both modes) beside
them.  --root TREE imports madrona_renderer_amd from another checkout (a build of the parent commit, say); a tree
whose SceneDesc has no instance_labels skips RGBD+L, so the same command line measures both builds.

--supersample N measures the resolve stage instead, RGBD, on the configurations chosen (default:
headline and c2): SS = time_renders of the renderer at supersample=N (render + resolve), PLAIN = time_renders of the
plain renderer of the sample size N*W x N*H, in the same alternation, and RESOLVE = the resolve alone (mark, a batch of
resolve(), mark) with its bytes -- bytes_per_step of SS minus that of PLAIN -- as a fraction of 8 TB/s; `placement`
is what the sample tensors' placement search timed (candidates, kept).

--positions measures the unprojection stage instead, RGBD, world frame, on the configurations chosen
(default: headline and c2): POS = time_renders of the renderer with positions=True (render + unproject), PLAIN =
time_renders of the renderer without, in the same alternation, and UNPROJECT = the stage alone (mark, a batch of
unproject(), mark) with its bytes -- bytes_per_step of POS minus that of PLAIN, 20 per pixel -- as a fraction of 8 TB/s.

--observations CHANNELS[,DTYPE[,STACK]] measures the observation stage instead, on the configurations
chosen (default: headline and c2), depth channels normalised to (0.1, 20): OBS = time_renders of the renderer with the
option (render + observe), PLAIN = time_renders of the renderer without, in the same alternation, and OBSERVE = the
stage alone (mark, a batch of observe(), mark) with its bytes -- bytes_per_step of OBS minus that of PLAIN -- as a
fraction of 8 TB/s.

Every renderer of a configuration is created and warmed first; then the settings alternate within
the process, `rounds` times, each measurement a batch of back-to-back renders between two events
(time_renders) of about `budget-ms`.  Reported: the median and the spread (min / max) of the
kernel us per render, views/s at the median, the algorithmic output bytes per view of the setting
and the fraction of 8 TB/s they make at the median (bytes_per_step of the renderer: the tensors
written plus the pose rows read).  bench.py is untouched: this is a measurement of its own.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0
SETTINGS = ("RGBD", "Depth", "RGB")
NORMAL_SETTINGS = ("RGBD+N", "Depth+N", "RGB+N")
LABEL_SETTINGS = ("RGBD+V", "RGBD+L")


def configs(scenes):
    # (key, label, scene factory, kernel_variant)
    return [
        ("headline", "4096 worlds x 64x64 cube+plane (the headline)", lambda: scenes.synthetic_scene(4096), None),
        ("c2", "1024 worlds x 64x64 cube+plane (BASELINE configs[1])", lambda: scenes.synthetic_scene(1024), None),
        ("configs2", "4096 worlds x 128x128 cube+plane+wall (BASELINE configs[2])",
         lambda: scenes.synthetic_scene(4096, width=128, height=128, with_wall=True), None),
        ("configs4", "4096 worlds x 256x256 Raytracer, textured (BASELINE configs[4], default dispatch)",
         lambda: scenes.synthetic_scene(4096, width=256, height=256, textured=True, render_mode="Raytracer"), None),
        ("bvh482", "1024 worlds x 64x64, 40 cubes + plane = 482 triangles per world (BVH tile kernel)",
         lambda: scenes.cube_field(1024, 40), None),
    ]


def make(scenes, factory, setting, variant):
    if variant is not None:
        os.environ["MADRONA_MI355_KERNEL"] = str(variant)
    try:
        desc = factory()
        if setting.endswith("+N"):
            desc.normals = True
            setting = setting[:-2]
        elif setting.endswith("+V"):
            os.environ["MADRONA_MI355_VISIBILITY"] = "1"
            setting = setting[:-2]
        elif setting.endswith("+L"):
            # labels in [1000, 2000), rows 1::4 at the sentinel (tests/label_oracle.py::mixed)
            import numpy as np
            labels = np.random.default_rng(11).integers(1000, 2000, len(desc.instances)).astype(np.int32)
            labels[1::4] = -2 ** 31
            desc.instance_labels = labels
            setting = setting[:-2]
        return scenes.make_renderer(desc, render_outputs=setting)
    finally:
        os.environ.pop("MADRONA_MI355_KERNEL", None)
        os.environ.pop("MADRONA_MI355_VISIBILITY", None)


def us_per_render(r, steps):
    return r.time_renders(steps) * 1000.0 / steps


def supersample_main(a, scenes):
    import dataclasses
    only = set(filter(None, a.only.split(","))) or {"headline", "c2"}
    for key, label, factory, variant in configs(scenes):
        if key not in only:
            continue
        for n in [int(x) for x in a.supersample.split(",")]:
            base = factory()
            ss = scenes.make_renderer(dataclasses.replace(base, supersample=n))
            plain = scenes.make_renderer(dataclasses.replace(base, width=base.width * n, height=base.height * n))

            def resolve_us(steps, r=ss):
                r.mark(0)
                for _ in range(steps):
                    r.resolve()
                r.mark(1)
                return r.elapsed_ms() * 1000.0 / steps

            fns = {"SS": lambda steps, r=ss: us_per_render(r, steps), "PLAIN": lambda steps, r=plain: us_per_render(r, steps),
                   "RESOLVE": resolve_us}
            steps = {}
            for s, fn in fns.items():
                t0 = time.perf_counter()
                while time.perf_counter() - t0 < 0.2:
                    est = fn(20)
                steps[s] = max(10, min(5000, int(a.budget_ms * 1000.0 / max(est, 1.0))))
            times = {s: [] for s in fns}
            for _ in range(a.rounds):
                for s, fn in fns.items():
                    times[s].append(fn(steps[s]))
            nbytes = {"SS": int(ss.bytes_per_step()), "PLAIN": int(plain.bytes_per_step())}
            nbytes["RESOLVE"] = nbytes["SS"] - nbytes["PLAIN"]
            for s in fns:
                med = statistics.median(times[s])
                print(json.dumps({
                    "config": key, "workload": label, "supersample": n, "setting": s, "views": base.num_views,
                    "native": [base.width, base.height], "steps": steps[s], "rounds": a.rounds,
                    "us_median": round(med, 3), "us_min": round(min(times[s]), 3), "us_max": round(max(times[s]), 3),
                    "us_all": [round(t, 3) for t in times[s]],
                    "ratio_to_plain": round(med / statistics.median(times["PLAIN"]), 4),
                    "bytes": nbytes[s], "frac_8tbps": round(nbytes[s] / (med * 1e-6) / 1e9 / HBM_PEAK_GBPS, 4),
                    "placement": (ss if s != "PLAIN" else plain).placement(),
                }), flush=True)
            del ss, plain


def positions_main(a, scenes):
    import dataclasses
    only = set(filter(None, a.only.split(","))) or {"headline", "c2"}
    for key, label, factory, variant in configs(scenes):
        if key not in only:
            continue
        base = factory()
        pos = scenes.make_renderer(dataclasses.replace(base, positions=True))
        plain = scenes.make_renderer(base)

        def unproject_us(steps, r=pos):
            r.mark(0)
            for _ in range(steps):
                r.unproject()
            r.mark(1)
            return r.elapsed_ms() * 1000.0 / steps

        fns = {"POS": lambda steps, r=pos: us_per_render(r, steps), "PLAIN": lambda steps, r=plain: us_per_render(r, steps),
               "UNPROJECT": unproject_us}
        steps = {}
        for s, fn in fns.items():
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.2:
                est = fn(20)
            steps[s] = max(10, min(5000, int(a.budget_ms * 1000.0 / max(est, 1.0))))
        times = {s: [] for s in fns}
        for _ in range(a.rounds):
            for s, fn in fns.items():
                times[s].append(fn(steps[s]))
        nbytes = {"POS": int(pos.bytes_per_step()), "PLAIN": int(plain.bytes_per_step())}
        nbytes["UNPROJECT"] = nbytes["POS"] - nbytes["PLAIN"]
        for s in fns:
            med = statistics.median(times[s])
            print(json.dumps({
                "config": key, "workload": label, "positions": "world", "setting": s, "views": base.num_views,
                "native": [base.width, base.height], "steps": steps[s], "rounds": a.rounds,
                "us_median": round(med, 3), "us_min": round(min(times[s]), 3), "us_max": round(max(times[s]), 3),
                "us_all": [round(t, 3) for t in times[s]],
                "ratio_to_plain": round(med / statistics.median(times["PLAIN"]), 4),
                "bytes": nbytes[s], "frac_8tbps": round(nbytes[s] / (med * 1e-6) / 1e9 / HBM_PEAK_GBPS, 4),
            }), flush=True)
        del pos, plain


def observations_main(a, scenes):
    import dataclasses
    only = set(filter(None, a.only.split(","))) or {"headline", "c2"}
    f = a.observations.split(",")
    opt = dict(channels=f[0], dtype=f[1] if len(f) > 1 else "float32", stack=int(f[2]) if len(f) > 2 else 1)
    if opt["channels"] in ("rgbd", "d", "yd"):
        opt["depth_range"] = (0.1, 20.0)
    for key, label, factory, variant in configs(scenes):
        if key not in only:
            continue
        base = factory()
        obs = scenes.make_renderer(dataclasses.replace(base, observations=opt))
        plain = scenes.make_renderer(base)

        def observe_us(steps, r=obs):
            r.mark(0)
            for _ in range(steps):
                r.observe()
            r.mark(1)
            return r.elapsed_ms() * 1000.0 / steps

        fns = {"OBS": lambda steps, r=obs: us_per_render(r, steps), "PLAIN": lambda steps, r=plain: us_per_render(r, steps),
               "OBSERVE": observe_us}
        steps = {}
        for s, fn in fns.items():
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.2:
                est = fn(20)
            steps[s] = max(10, min(5000, int(a.budget_ms * 1000.0 / max(est, 1.0))))
        times = {s: [] for s in fns}
        for _ in range(a.rounds):
            for s, fn in fns.items():
                times[s].append(fn(steps[s]))
        nbytes = {"OBS": int(obs.bytes_per_step()), "PLAIN": int(plain.bytes_per_step())}
        nbytes["OBSERVE"] = nbytes["OBS"] - nbytes["PLAIN"]
        for s in fns:
            med = statistics.median(times[s])
            print(json.dumps({
                "config": key, "workload": label, "observations": opt, "setting": s, "views": base.num_views,
                "native": [base.width, base.height], "steps": steps[s], "rounds": a.rounds,
                "us_median": round(med, 3), "us_min": round(min(times[s]), 3), "us_max": round(max(times[s]), 3),
                "us_all": [round(t, 3) for t in times[s]],
                "ratio_to_plain": round(med / statistics.median(times["PLAIN"]), 4),
                "bytes": nbytes[s], "frac_8tbps": round(nbytes[s] / (med * 1e-6) / 1e9 / HBM_PEAK_GBPS, 4),
            }), flush=True)
        del obs, plain


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--budget-ms", type=float, default=30.0, help="device time of one measurement")
    ap.add_argument("--only", default="", help="comma-separated configuration keys")
    ap.add_argument("--normals", action="store_true", help="also time each setting with the surface-normal output")
    ap.add_argument("--labels", action="store_true", help="also time RGBD with visibility ids and with the label column")
    ap.add_argument("--root", default="", help="import madrona_renderer_amd from this checkout instead")
    ap.add_argument("--supersample", default="", help="factors (2,3,4): measure the resolve stage instead (DESIGN.md 4.18)")
    ap.add_argument("--positions", action="store_true", help="measure the unprojection stage instead (DESIGN.md 4.19)")
    ap.add_argument("--observations", default="", help="CHANNELS[,DTYPE[,STACK]]: measure the observation stage instead (DESIGN.md 4.21)")
    a = ap.parse_args(argv)
    if a.rounds < 3:
        ap.error("--rounds must be at least 3")
    if a.root:
        sys.path.insert(0, os.path.abspath(a.root))
    from madrona_renderer_amd import scenes
    if a.supersample:
        return supersample_main(a, scenes)
    if a.positions:
        return positions_main(a, scenes)
    if a.observations:
        return observations_main(a, scenes)
    only = set(filter(None, a.only.split(",")))
    settings = SETTINGS + (NORMAL_SETTINGS if a.normals else ())
    if a.labels:
        has = "instance_labels" in scenes.SceneDesc.__dataclass_fields__
        settings += LABEL_SETTINGS if has else LABEL_SETTINGS[:1]
    for key, label, factory, variant in configs(scenes):
        if only and key not in only:
            continue
        rs = {s: make(scenes, factory, s, variant) for s in settings}
        views = factory().num_views
        # warm every shape: clocks up, first launches (XCC report, cold caches) out of the way
        steps = {}
        for s, r in rs.items():
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.2:
                est = us_per_render(r, 20)
            steps[s] = max(10, min(5000, int(a.budget_ms * 1000.0 / max(est, 1.0))))
        times = {s: [] for s in settings}
        for _ in range(a.rounds):
            for s in settings:
                times[s].append(us_per_render(rs[s], steps[s]))
        base = statistics.median(times["RGBD"])
        for s in settings:
            med = statistics.median(times[s])
            b = int(rs[s].bytes_per_step())
            print(json.dumps({
                "config": key, "workload": label, "setting": s, "render_path": rs[s].render_path(),
                "views": views, "steps": steps[s], "rounds": a.rounds,
                "kernel_us_median": round(med, 3), "kernel_us_min": round(min(times[s]), 3),
                "kernel_us_max": round(max(times[s]), 3), "kernel_us_all": [round(t, 3) for t in times[s]],
                "ratio_to_rgbd": round(med / base, 4),
                "views_per_s": round(views / (med * 1e-6)),
                "bytes_per_view": round(b / views, 1),
                "frac_8tbps": round(b / (med * 1e-6) / 1e9 / HBM_PEAK_GBPS, 4),
            }), flush=True)
        del rs


if __name__ == "__main__":
    main()
