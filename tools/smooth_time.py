"""Time plade_cloud_smooth_dev on resident synthetic scenes (not part of bench.py).

The grid build and the fit are timed separately with the HIP events the library records on its stream around them
(plade_stats_get: smooth_grid_s, smooth_fit_s, smooth_reduce_s): the cloud is resident, so the numbers exclude any upload.  The
radius of a row is chosen so that the median neighbourhood holds about --counts points.  It is calibrated on a crop: the slab
between two x quantiles that holds about --crop points, smoothed on its own, counting only the points farther than r from the
slab's faces (their neighbourhoods are complete); from a first guess the radius is scaled twice by sqrt(target / median) (a
surface: the count grows with r^2).  One call on the whole cloud through the C ABI, asking for the counts alone, then records the
median reached there.  Median of --iters calls after --warmup calls.

    python tools/smooth_time.py --sizes 1000000 10000000 --counts 16 64 [--out profiles/smooth_time.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import plade_amd  # noqa: E402
from plade_amd.synth import sample_scene  # noqa: E402


def crop_median(ctx, slab, lo, hi, r):
    """Median count, at radius r, of the slab's points farther than r from its faces x = lo and x = hi."""
    count = ctx.smooth_cloud(slab, r, normals=False)[1]["count"]
    inner = (slab[:, 0] >= lo + r) & (slab[:, 0] <= hi - r)
    return float(np.median(count[inner])) if inner.any() else float(np.median(count))


def full_counts(ctx, xyz, r):
    """(counts, summary) of the whole cloud: plade_smooth_cloud with every optional output but the counts left out."""
    prm = plade_amd.SmoothParams()
    ctx.L.plade_smooth_default_params(ctypes.byref(prm))
    prm.radius = float(r)
    out = np.empty((len(xyz), 3), np.float32)
    count = np.empty(len(xyz), np.uint32)
    summ = plade_amd.SmoothSummary()
    rc = ctx.L.plade_smooth_cloud(ctx.h, xyz.ctypes.data, len(xyz), 3, ctypes.byref(prm), out.ctypes.data, None, None, None,
                                  count.ctypes.data, None, None, ctypes.byref(summ))
    if rc != plade_amd.PLADE_OK:
        raise RuntimeError(ctx.L.plade_last_error(ctx.h).decode())
    return count, summ


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--counts", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--crop", type=int, default=200_000, help="points of the slab the radius is calibrated on")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = plade_amd.Context(0)
    rows = []
    for n in args.sizes:
        cloud = np.ascontiguousarray(sample_scene(n, sample_seed=1))
        xyz = np.ascontiguousarray(cloud[:, :3])
        res = ctx.upload(cloud)
        half = min(0.5, 0.5 * args.crop / n)
        lo, hi = (float(v) for v in np.quantile(xyz[:, 0], [0.5 - half, 0.5 + half]))
        slab = np.ascontiguousarray(xyz[(xyz[:, 0] >= lo) & (xyz[:, 0] <= hi)])
        for target in args.counts:
            r = 0.04 * np.sqrt(1e6 / n) * np.sqrt(target / 16.0)        # a first guess only: the two steps below correct it
            for _ in range(2):
                r *= np.sqrt(target / max(crop_median(ctx, slab, lo, hi, r), 1.0))
            count, summ = full_counts(ctx, xyz, r)
            info = {"count": count, "max_count": summ.max_count, "fitted": summ.fitted}
            grid, fit, red = [], [], []
            for it in range(args.warmup + args.iters):
                c = ctx.smooth_cloud_dev(res, r)
                s = ctx.stats()
                c.free()
                if it >= args.warmup:
                    grid.append(s["smooth_grid_s"]); fit.append(s["smooth_fit_s"]); red.append(s["smooth_reduce_s"])
            g, q, e = float(np.median(grid)), float(np.median(fit)), float(np.median(red))
            row = {"n": n, "radius": float(r), "median_count": float(np.median(info["count"])), "max_count": int(info["max_count"]),
                   "fitted": int(info["fitted"]), "grid_ms": 1e3 * g, "fit_ms": 1e3 * q, "reduce_ms": 1e3 * e, "total_ms": 1e3 * (g + q + e),
                   "ms_per_1M_points": 1e3 * (g + q + e) / (n / 1e6), "iters": args.iters}
            print(json.dumps(row), flush=True)
            rows.append(row)
        res.free()
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
