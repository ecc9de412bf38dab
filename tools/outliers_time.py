"""Time plade_cloud_filter_outliers_dev on synthetic scenes (not part of bench.py).

The cloud is resident (plade_cloud_upload), so the numbers exclude the upload.  The library records HIP events on its stream
around the four parts (plade_stats_get: outliers_grid_s, outliers_search_s, outliers_reduce_s = mu, sigma and the keep flags,
outliers_compact_s = scan, kept list and row gather).  Median of --iters calls after --warmup calls.  The scenes are those of
tools/normals_time.py (sample_scene(n, sample_seed=1)), whose estimate_normals at the same k is the yardstick.

With --benefit N the normals of an N-point scene are estimated before and after the filter (k = 16): the points that reach
k_normals_ring and the search time of both.

    python tools/outliers_time.py --sizes 1000000 10000000 --ks 16 32 --benefit 1000000 [--out profiles/outliers_time.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import plade_amd  # noqa: E402
from plade_amd.synth import sample_scene  # noqa: E402

PARTS = ("grid", "search", "reduce", "compact")


def normals_row(ctx, xyz, k, warmup, iters):
    grid, search, ring = [], [], 0
    for it in range(warmup + iters):
        c = ctx.upload_xyz(xyz, k=k)
        s = ctx.stats()
        c.free()
        if it >= warmup:
            grid.append(s["normals_grid_s"])
            search.append(s["normals_search_s"])
            ring = int(s["normals_ring_queries"])
    return {"n": len(xyz), "grid_ms": 1e3 * float(np.median(grid)), "search_pca_ms": 1e3 * float(np.median(search)),
            "ring_queries": ring, "ring_fraction": ring / len(xyz)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--ks", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--alpha", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--benefit", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = plade_amd.Context(0)
    rows = []
    for n in args.sizes:
        cloud = ctx.upload(sample_scene(n, sample_seed=1))
        for k in args.ks:
            t = {p: [] for p in PARTS}
            ring = kept = builds = 0
            for it in range(args.warmup + args.iters):
                f = ctx.remove_outliers_dev(cloud, k=k, alpha=args.alpha)
                s = ctx.stats()
                f.free()
                if it >= args.warmup:
                    for p in PARTS:
                        t[p].append(s[f"outliers_{p}_s"])
                    ring, kept, builds = int(s["outliers_ring_queries"]), int(s["outliers_kept"]), int(s["outliers_grid_builds"])
            ms = {p: 1e3 * float(np.median(t[p])) for p in PARTS}
            row = {"what": "filter", "n": n, "k": k, "alpha": args.alpha, **{f"{p}_ms": ms[p] for p in PARTS},
                   "total_ms": sum(ms.values()), "grid_builds": builds, "ring_queries": ring, "ring_fraction": ring / n, "kept": kept,
                   "iters": args.iters}
            print(json.dumps(row), flush=True)
            rows.append(row)
        cloud.free()
    if args.benefit:
        xyz = np.ascontiguousarray(sample_scene(args.benefit, sample_seed=1)[:, :3])
        filtered, _, info = ctx.remove_outliers(xyz, k=16, alpha=args.alpha, per_point=False)
        for what, a in (("normals_raw", xyz), ("normals_filtered", filtered)):
            row = {"what": what, "k": 16, **normals_row(ctx, a, 16, args.warmup, args.iters)}
            print(json.dumps(row), flush=True)
            rows.append(row)
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
