"""Time plade_cloud_m3c2_dev on resident synthetic scenes (not part of bench.py).

Two samplings of one scene of --size points each are resident; the core points are every --every-th point of the first with the
scene's normals, resident too.  The transform + grid builds, the walk and the reduction are timed separately with the HIP events
the library records on its stream around them (plade_stats_get: m3c2_grid_s, m3c2_walk_s, m3c2_reduce_s): nothing is uploaded in
the timed calls, the only host copy is the distance array.  The radius of a row is chosen so that the median count of the
reference cloud in a cylinder is about --counts: from a first guess it is scaled twice by sqrt(target / median) on every
--calibrate-th core point (a surface: the count grows with R^2), at depth 4 R.  Each radius runs at depth 4 R and 20 R.  Median of
--iters calls after --warmup calls.

    python tools/m3c2_time.py [--size 1000000] [--counts 16 64] [--out profiles/m3c2_time.json]
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
    ap.add_argument("--size", type=int, default=1_000_000)
    ap.add_argument("--every", type=int, default=10, help="core points: every n-th point of the reference cloud")
    ap.add_argument("--counts", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--depths", type=float, nargs="+", default=[4.0, 20.0], help="in units of the radius")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--calibrate", type=int, default=50, help="the radius is calibrated on every n-th core point")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "m3c2_time.json"))
    args = ap.parse_args()
    ctx = plade_amd.Context(0)
    A = np.ascontiguousarray(sample_scene(args.size, sample_seed=1))
    B = np.ascontiguousarray(sample_scene(args.size, sample_seed=2))
    core = np.ascontiguousarray(A[::args.every])
    ra, rb, rc, rs = ctx.upload(A), ctx.upload(B), ctx.upload(core), ctx.upload(np.ascontiguousarray(core[::args.calibrate]))
    rows = []
    for target in args.counts:
        r = 0.04 * np.sqrt(1e6 / args.size) * np.sqrt(target / 16.0)      # a first guess only: the two steps below correct it
        for _ in range(2):
            count = ctx.m3c2_dev(rs, ra, rb, r, 4.0 * r)[1]["count"]
            r *= np.sqrt(target / max(float(np.median(count[:, 0])), 1.0))
        for depth in args.depths:
            grid, walk, red = [], [], []
            for it in range(args.warmup + args.iters):
                dist, info = ctx.m3c2_dev(rc, ra, rb, r, depth * r, per_point=it == 0)
                if it == 0:
                    first = info
                s = ctx.stats()
                if it >= args.warmup:
                    grid.append(s["m3c2_grid_s"]); walk.append(s["m3c2_walk_s"]); red.append(s["m3c2_reduce_s"])
            g, w, e = float(np.median(grid)), float(np.median(walk)), float(np.median(red))
            row = {"n": args.size, "core_points": len(core), "radius": float(r), "depth": float(depth * r), "depth_over_radius": depth,
                   "median_count": float(np.median(first["count"][:, 0])), "max_count": int(first["max_count"]), "valid": int(first["valid"]),
                   "significant": int(first["significant"]), "grid_ms": 1e3 * g, "walk_ms": 1e3 * w, "reduce_ms": 1e3 * e,
                   "total_ms": 1e3 * (g + w + e), "walk_ns_per_core_point": 1e9 * w / len(core), "iters": args.iters}
            print(json.dumps(row), flush=True)
            rows.append(row)
    for c in (ra, rb, rc, rs):
        c.free()
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
