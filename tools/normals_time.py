"""Time plade_cloud_upload_xyz's normal estimation on synthetic scenes (not part of bench.py).

The grid build and the search + PCA are timed separately with the HIP events the library records on its stream around them
(plade_stats_get: normals_grid_s, normals_search_s): the coordinates are already in device memory then, so the numbers
exclude the upload.  Median of --iters calls after --warmup calls.

    python tools/normals_time.py --sizes 1000000 10000000 --ks 16 32 [--out profiles/normals_time.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--ks", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = plade_amd.Context(0)
    rows = []
    for n in args.sizes:
        xyz = np.ascontiguousarray(sample_scene(n, sample_seed=1)[:, :3])
        for k in args.ks:
            grid, search, ring, builds = [], [], 0, 0
            for it in range(args.warmup + args.iters):
                c = ctx.upload_xyz(xyz, k=k)
                s = ctx.stats()
                c.free()
                if it >= args.warmup:
                    grid.append(s["normals_grid_s"])
                    search.append(s["normals_search_s"])
                    ring, builds = int(s["normals_ring_queries"]), int(s["normals_grid_builds"])
            g, q = float(np.median(grid)), float(np.median(search))
            row = {"n": n, "k": k, "grid_ms": 1e3 * g, "search_pca_ms": 1e3 * q, "total_ms": 1e3 * (g + q),
                   "ms_per_1M_points": 1e3 * (g + q) / (n / 1e6), "grid_builds": builds, "ring_queries": ring,
                   "ring_fraction": ring / n, "iters": args.iters}
            print(json.dumps(row), flush=True)
            rows.append(row)
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
