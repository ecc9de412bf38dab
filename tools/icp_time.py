"""Time plade_refine_icp_dev on synthetic pairs (not part of bench.py).

Each pair is registered first with the library's defaults (closest_point_mode = 1, oriented normals); the refinement then starts
from that result on resident clouds.  The stages are timed with the HIP events the library records on its stream (plade_stats_get:
icp_sample_s -- the source's voxel grid, icp_grid_s -- one target grid per stage, icp_loop_s -- the queued iterations), so the
numbers exclude the uploads.  Median of --iters calls after --warmup calls.  The share of the coarsest stage is measured by a
second refinement limited to that stage (max_dist = min_dist = 0.025 D) run for the same number of iterations as the coarsest
stage took.

    python tools/icp_time.py --sizes 1000000 10000000 [--out profiles/icp_time.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = plade_amd.Context(0, orient_normals=1)
    rows = []
    for n in args.sizes:
        tg, sr, Tgt = make_pair(n, seed=args.seed)
        ok, T0 = ctx.registration(tg, sr)
        if not ok:
            raise SystemExit(f"registration of the {n}-point pair failed")
        ct, cs = ctx.upload(tg), ctx.upload(sr)
        samp, grid, loop = [], [], []
        for it in range(args.warmup + args.iters):
            T, info = ctx.refine_icp_dev(ct, cs, T0)
            s = ctx.stats()
            if it >= args.warmup:
                samp.append(s["icp_sample_s"]); grid.append(s["icp_grid_s"]); loop.append(s["icp_loop_s"])
        # the coarsest stage alone, for as many iterations as it takes in the full run (the first stage converges at the same
        # iterate: the same distance, the same start)
        lo = np.array([tg[:, :3].min(0), tg[:, :3].max(0)], np.float64)
        D = float(np.linalg.norm(lo[1] - lo[0]))
        _, first = ctx.refine_icp_dev(ct, cs, T0, max_dist=0.025 * D, min_dist=0.025 * D)
        coarse = []
        for it in range(args.warmup + args.iters):
            ctx.refine_icp_dev(ct, cs, T0, max_dist=0.025 * D, min_dist=0.025 * D)
            if it >= args.warmup:
                coarse.append(ctx.stats()["icp_loop_s"])
        ct.free(); cs.free()
        a, g, q, c = (1e3 * float(np.median(v)) for v in (samp, grid, loop, coarse))
        row = {"n": n, "seed": args.seed, "samples": info["samples"], "iterations": info["iterations"], "stages": info["stages"],
               "converged": info["converged"], "sample_ms": a, "grid_ms": g, "loop_ms": q, "total_ms": a + g + q,
               "coarsest_stage_iterations": first["iterations"], "coarsest_stage_loop_ms": c,
               "coarsest_stage_share_of_loop": c / q if q > 0 else None,
               "err_before": float(np.linalg.norm(T0.astype(np.float64) - Tgt)), "err_after": float(np.linalg.norm(T.astype(np.float64) - Tgt)),
               "rmse": info["rmse"], "fitness": info["fitness"], "iters": args.iters}
        print(json.dumps(row), flush=True)
        rows.append(row)
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
