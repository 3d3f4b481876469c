#!/usr/bin/env python3
"""The compaction stage's time beside unproject()'s and beside the torch chain that computes the same [views, N, 4]
from position_tensor().  Needs an MI355X.

  python scripts/bench_cloud.py [--views 1024] [--points 1024] [--reps 20] [--out profiles/cloud_latest.txt]

One renderer with positions="world" and the point-cloud output; compact(), unproject() and the torch chain are timed in
turns on the renderer's stream after a warm-up, and the medians are printed.  The torch chain -- a validity mask, a
cumsum, a searchsorted for every slot's rank, a gather and the padding -- is checked against the stage's points first.
"""
import argparse
import dataclasses
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_chain(position, n):
    """[views, H, W, 4] -> [views, n, 4]: S18's selection with framework ops"""
    import torch
    views = position.shape[0]
    flat = position.reshape(views, -1, 4)
    valid = flat[..., 3] > 0
    cs = valid.to(torch.int64).cumsum(1)
    m = cs[:, -1:]
    k = torch.arange(n, device=position.device, dtype=torch.int64)[None]
    rank = torch.where(m >= n, (k * m) // n, k)
    idx = torch.searchsorted(cs, rank + 1).clamp(max=flat.shape[1] - 1)
    out = torch.gather(flat, 1, idx[..., None].expand(-1, -1, 4))
    return torch.where((k < m)[..., None], out, torch.zeros_like(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=1024)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from madrona_renderer_amd import cloud, scenes
    os.environ["MADRONA_MI355_VISIBILITY"] = "0"
    r = scenes.make_renderer(dataclasses.replace(scenes.synthetic_scene(a.views), positions="world"))
    c = cloud.attach(r, a.points)
    r.step()
    r.sync()
    position = r.position_tensor().to_torch()
    same = torch.equal(torch_chain(position, a.points).view(torch.int32), c.points_tensor().view(torch.int32))
    stream = torch.cuda.current_stream()

    def timed(fn):
        r.mark(0)
        fn()
        r.mark(1)
        return r.elapsed_ms() * 1000.0

    def timed_torch():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        torch_chain(position, a.points)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0

    for fn in (lambda: timed(c.compact), lambda: timed(r.unproject), timed_torch):
        for _ in range(5):
            fn()
    t = {"compact": [], "unproject": [], "torch": []}
    for _ in range(a.reps):
        t["compact"].append(timed(c.compact))
        t["unproject"].append(timed(r.unproject))
        t["torch"].append(timed_torch())
    med = {k: statistics.median(v) for k, v in t.items()}
    count = c.count_tensor().cpu().numpy()
    lines = [
        "## scripts/bench_cloud.py --views %d --points %d --reps %d: medians, one MI355X" % (a.views, a.points, a.reps),
        "views %d of 64 x 64, N = %d, valid pixels per view min %d median %d max %d"
        % (a.views, a.points, count.min(), int(statistics.median(count.tolist())), count.max()),
        "compact()    %8.2f us   (min %.2f, max %.2f)" % (med["compact"], min(t["compact"]), max(t["compact"])),
        "unproject()  %8.2f us   (min %.2f, max %.2f)" % (med["unproject"], min(t["unproject"]), max(t["unproject"])),
        "torch chain  %8.2f us   (min %.2f, max %.2f; its points equal the stage's bit for bit: %s)"
        % (med["torch"], min(t["torch"]), max(t["torch"]), same),
        "compact / unproject %.2f, torch chain / compact %.1f" % (med["compact"] / med["unproject"], med["torch"] / med["compact"]),
    ]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
