"""Time plade_cloud_distances_dev on synthetic pairs (not part of bench.py).

The source is evaluated at its ground-truth transform on resident clouds.  The stages are timed with the HIP events the library
records on its stream (plade_stats_get: distances_grid_s -- the target's row grid, distances_sort_s -- p', cell keys and the radix
sort of the probes, distances_lane_s / distances_ring_s -- the two search passes, distances_summary_s -- the plane term and the
fp64 sums), so the numbers exclude the uploads and the read-back.  Median of --iters calls after --warmup calls, no per-point
outputs (evaluate mode).

Bytes: the compulsory traffic of the search kernels -- per probe its index (4 B) and p' (16 B) read, idx and d2 (8 B) written;
the target's sorted points (16 B each) and row table (4 B per padded cell) read once -- over the lane + ring time, as a share of
the MI355X's 8 TB/s HBM peak.  Candidate re-reads by neighbouring probes are cache hits and are not counted.

    python tools/distances_time.py [--cases 1000000:0.01 1000000:0.05 10000000:0.01] [--out profiles/distances_time.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import plade_amd  # noqa: E402
from plade_amd.synth import make_pair  # noqa: E402

HBM_PEAK = 8.0e12   # bytes / s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["1000000:0.01", "1000000:0.05", "10000000:0.01"],
                    help="n:d, d as a fraction of the target's bounding-box diagonal D")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = plade_amd.Context(0)
    rows = []
    pairs = {}
    for case in args.cases:
        n, frac = case.split(":")
        n, frac = int(n), float(frac)
        if n not in pairs:
            pairs.clear()
            pairs[n] = make_pair(n, seed=args.seed)
        tg, sr, Tgt = pairs[n]
        D = float(np.linalg.norm(tg[:, :3].max(0).astype(np.float64) - tg[:, :3].min(0)))
        ct, cs = ctx.upload(tg), ctx.upload(sr)
        keys = ("grid", "sort", "lane", "ring", "summary")
        t = {k: [] for k in keys}
        for it in range(args.warmup + args.iters):
            s = ctx.cloud_distances_dev(ct, cs, frac * D, T=Tgt, per_point=False)[3]
            st = ctx.stats()
            if it >= args.warmup:
                for k in keys:
                    t[k].append(st[f"distances_{k}_s"])
        ring_queries = int(st["distances_ring_queries"])
        ct.free(); cs.free()
        ms = {k: 1e3 * float(np.median(v)) for k, v in t.items()}
        search = ms["lane"] + ms["ring"]
        ext = tg[:, :3].max(0).astype(np.float64) - tg[:, :3].min(0)
        area = 2 * (ext[0] * ext[1] + ext[1] * ext[2] + ext[0] * ext[2])
        cell = min(1.5 * np.sqrt(8.0 * area / (np.pi * len(tg))), 1.03 * frac * D)   # the library's cell (k_distances.hip)
        padded_cells = float(np.prod(np.floor(ext / (cell * 1.001)) + 5))
        search_bytes = len(sr) * (4 + 16 + 8) + len(tg) * 16 + 4 * min(padded_cells, 48e6)
        row = {"n_t": len(tg), "n_s": len(sr), "seed": args.seed, "d_over_D": frac, "d": frac * D,
               **{f"{k}_ms": v for k, v in ms.items()}, "search_ms": search, "total_ms": sum(ms.values()),
               "ring_queries": ring_queries, "ring_share_of_search": ms["ring"] / search if search > 0 else None,
               "search_bytes": search_bytes, "search_hbm_share": search_bytes / (1e-3 * search) / HBM_PEAK if search > 0 else None,
               "fitness": s["fitness"], "rmse": s["rmse"], "iters": args.iters}
        print(json.dumps(row), flush=True)
        rows.append(row)
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
