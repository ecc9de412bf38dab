"""Time plade_merge_clouds_dev on synthetic scan pairs (not part of bench.py).

The clouds are resident (plade_cloud_upload), so the merge's numbers exclude the upload.  The library records HIP events on its
stream around the four parts (plade_stats_get: merge_transform_s = transform pass + bounding box, merge_sort_s = keys + radix
sort, merge_runs_s = run heads + six-channel gather, merge_fuse_s); `events_ms` is their sum, `wall_ms` the whole call on the
host's clock (with the allocation and finish of the resident result).  Median of --iters calls after --warmup calls.

The yardstick is plade_voxel_downsample of the same points -- the source transformed on the host, both clouds concatenated -- at
the same leaf: three channels, fp32 sums, no transform; it takes host points, so its `wall_ms` contains the 12 B/point upload and
the read-back of the centroids.  leaf is given as a fraction of the diagonal D of the merged clouds' bounding box; 0 = plain
concatenation (no yardstick).

    python tools/merge_time.py --sizes 1000000 10000000 --leaves 0.005 0.02 0 [--out profiles/merge_time.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import plade_amd  # noqa: E402
from plade_amd.synth import make_pair  # noqa: E402

PARTS = ("transform", "sort", "runs", "fuse")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--leaves", type=float, nargs="+", default=[0.005, 0.02, 0.0])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = plade_amd.Context(0)
    rows = []
    for n in args.sizes:
        tg, sr, T = make_pair(n, seed=0, keep=1.0)
        T = T.astype(np.float32)
        moved = sr[:, :3] @ T[:3, :3].T + T[:3, 3]
        both = np.ascontiguousarray(np.concatenate([tg[:, :3], moved]), np.float32)
        D = float(np.linalg.norm(both.max(0).astype(np.float64) - both.min(0).astype(np.float64)))
        ct, cs = ctx.upload(tg), ctx.upload(sr)
        for frac in args.leaves:
            leaf = frac * D
            t = {p: [] for p in PARTS}
            wall, n_out = [], 0
            for it in range(args.warmup + args.iters):
                plade_amd.device_synchronize(0)
                t0 = time.perf_counter()
                m = ctx.merge_clouds_dev([ct, cs], [None, T], leaf)
                dt = time.perf_counter() - t0
                s = ctx.stats()
                n_out = m.n
                m.free()
                if it >= args.warmup:
                    wall.append(dt)
                    for p in PARTS:
                        t[p].append(s[f"merge_{p}_s"])
            ms = {p: 1e3 * float(np.median(t[p])) for p in PARTS}
            row = {"what": "merge_clouds_dev", "n": [len(tg), len(sr)], "leaf_over_D": frac, "leaf": leaf,
                   **{f"{p}_ms": ms[p] for p in PARTS}, "events_ms": sum(ms.values()), "wall_ms": 1e3 * float(np.median(wall)),
                   "rows": n_out, "iters": args.iters}
            if frac > 0:
                base = []
                for it in range(args.warmup + args.iters):
                    t0 = time.perf_counter()
                    v = ctx.voxel_downsample(both, leaf)
                    if it >= args.warmup:
                        base.append(time.perf_counter() - t0)
                row["voxel_downsample_wall_ms"] = 1e3 * float(np.median(base))
                row["voxel_downsample_rows"] = len(v)
                row["wall_ratio"] = row["wall_ms"] / row["voxel_downsample_wall_ms"]
            print(json.dumps(row), flush=True)
            rows.append(row)
        ct.free()
        cs.free()
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
