"""Time plade_refine_gicp_dev beside plade_refine_icp_dev on a resident synthetic pair (not part of bench.py).

Both refinements report the library's HIP-event times for their sample, their stage grids and their loop (plade_stats_get:
gicp_sample_s / gicp_grid_s / gicp_loop_s and icp_sample_s / icp_grid_s / icp_loop_s), so the numbers exclude any upload.  The
point-to-plane loop of the same build is the yardstick: the loop time per iteration of the two is set side by side and their ratio
reported.  The start is the generator's transformation under a small perturbation; median of --iters calls after --warmup calls.

    python tools/gicp_time.py [--n 1000000] [--out profiles/gicp_time.json]
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


def perturb(T, rot, trans, seed):
    """[R(axis, rot) | trans * unit] T with a seeded random axis and direction."""
    rng = np.random.default_rng(seed)
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    v = rng.normal(size=3)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    U = np.eye(4)
    U[:3, :3] = np.eye(3) + np.sin(rot) * K + (1.0 - np.cos(rot)) * (K @ K)
    U[:3, 3] = v / np.linalg.norm(v) * trans
    return U @ np.asarray(T, np.float64)


def timed(call, stats, prefix, warmup, iters):
    rows = []
    for it in range(warmup + iters):
        T, info = call()
        s = stats()
        if it >= warmup:
            rows.append((s[prefix + "_sample_s"], s[prefix + "_grid_s"], s[prefix + "_loop_s"]))
    sample, grid, loop = (float(np.median([r[k] for r in rows])) for k in range(3))
    return T, info, {"sample_ms": 1e3 * sample, "grid_ms": 1e3 * grid, "loop_ms": 1e3 * loop,
                     "loop_ms_per_iteration": 1e3 * loop / max(info["iterations"], 1), "iterations": info["iterations"],
                     "stages": info["stages"], "converged": info["converged"], "samples": info["samples"],
                     "correspondences": info["correspondences"], "rmse": info["rmse"], "fitness": info["fitness"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rot", type=float, default=0.02)
    ap.add_argument("--trans", type=float, default=0.02)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gicp_time.json"))
    args = ap.parse_args()
    tg, sr, Tgt = make_pair(args.n, seed=args.seed)
    T0 = perturb(Tgt, args.rot, args.trans, seed=1).astype(np.float32)
    ctx = plade_amd.Context(0)
    ct, cs = ctx.upload(tg), ctx.upload(sr)
    err = lambda T: float(np.linalg.norm(T.astype(np.float64) - Tgt))   # noqa: E731
    Tg, _, gicp = timed(lambda: ctx.refine_gicp_dev(ct, cs, T0), ctx.stats, "gicp", args.warmup, args.iters)
    Ti, _, icp = timed(lambda: ctx.refine_icp_dev(ct, cs, T0), ctx.stats, "icp", args.warmup, args.iters)
    ct.free(); cs.free()
    ctx.close()
    out = {"n_target": len(tg), "n_source": len(sr), "start_error": err(T0), "iters": args.iters, "warmup": args.warmup,
           "gicp": dict(gicp, error=err(Tg)), "icp": dict(icp, error=err(Ti)),
           "loop_per_iteration_ratio_gicp_over_icp": gicp["loop_ms_per_iteration"] / icp["loop_ms_per_iteration"]}
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
