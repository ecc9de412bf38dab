"""Time plade_cloud_keypoints_iss_dev on a resident synthetic scene and the feature match behind it (not part of bench.py).

One sampling of a scene of --size points is resident.  The grid build, the scatter walk (with the eigenvalues and the salient test) and
the suppression walk (with the list and the summary) are timed separately with the HIP events the library records on its stream
around them (plade_stats_get: iss_grid_s, iss_scatter_s, iss_nms_s): nothing is uploaded in the timed calls and no per-point array is
copied back.  The salient radius of a row is chosen so that the median number of points within it (the point itself included) is
about --counts: from a first guess it is scaled twice by sqrt(target / median) (a surface: the count grows with r^2); the non-max
radius is half of it.  Median of --iters calls after --warmup calls.

The match: two samplings of --match-size points are described with FPFH at the radius calibrated for a median of 64 counted pairs
(the tables of tools/fpfh_time.py); the keypoints of the first (salient radius = that radius, non-max radius half of it) select its
rows, and the selected table is matched against the whole second table (feat_match_s: both searches, the merge, the filter and the
compaction), next to the match of the two full tables in the same process.

    python tools/iss_time.py [--size 1000000] [--counts 16 64] [--out profiles/iss_time.json]
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


def calibrate(ctx, cloud, n, target):
    r = 0.04 * np.sqrt(1e6 / n) * np.sqrt(target / 16.0)            # a first guess only: the two steps below correct it
    for _ in range(2):
        count = ctx.iss_keypoints_dev(cloud, r)[1]["count"]
        r *= np.sqrt(target / max(float(np.median(count)), 1.0))
    return float(r)


def calibrate_fpfh(ctx, cloud, n, target):                         # as tools/fpfh_time.py
    r = 0.04 * np.sqrt(1e6 / n) * np.sqrt(target / 16.0)
    for _ in range(2):
        pairs = ctx.fpfh_dev(cloud, r)[1]["pairs"]
        r *= np.sqrt(target / max(float(np.median(pairs)), 1.0))
    return float(r)


def timed_match(ctx, a, b, warmup, iters):
    t = []
    for it in range(warmup + iters):
        corr, info = ctx.match_features_dev(a, b)
        if it >= warmup:
            t.append(ctx.stats()["feat_match_s"])
    return float(np.median(t)), int(info["n_corr"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1_000_000)
    ap.add_argument("--counts", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--match-size", type=int, default=100_000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iss_time.json"))
    args = ap.parse_args()
    ctx = plade_amd.Context(0)
    rows = []
    ra = ctx.upload(np.ascontiguousarray(sample_scene(args.size, sample_seed=1)))
    for target in args.counts:
        rs = calibrate(ctx, ra, args.size, target)
        grid, scatter, nms = [], [], []
        for it in range(args.warmup + args.iters):
            index, info = ctx.iss_keypoints_dev(ra, rs, rs / 2, per_point=it == 0)
            if it == 0:
                first = info
            s = ctx.stats()
            if it >= args.warmup:
                grid.append(s["iss_grid_s"]); scatter.append(s["iss_scatter_s"]); nms.append(s["iss_nms_s"])
        g, h, w = float(np.median(grid)), float(np.median(scatter)), float(np.median(nms))
        members = int(first["count"].astype(np.int64).sum())
        row = {"what": "iss", "n": args.size, "salient_radius": rs, "non_max_radius": rs / 2, "median_count": float(np.median(first["count"])),
               "max_count": int(first["max_count"]), "salient": int(first["salient"]), "keypoints": int(first["keypoints"]),
               "neighbourhood_members": members, "grid_ms": 1e3 * g, "scatter_ms": 1e3 * h, "nms_ms": 1e3 * w, "total_ms": 1e3 * (g + h + w),
               "scatter_ns_per_member": 1e9 * h / max(members, 1), "iters": args.iters}
        print(json.dumps(row), flush=True)
        rows.append(row)
    ra.free()
    n = args.match_size
    ca = ctx.upload(np.ascontiguousarray(sample_scene(n, sample_seed=1)))
    cb = ctx.upload(np.ascontiguousarray(sample_scene(n, sample_seed=2)))
    r = calibrate_fpfh(ctx, ca, n, 64)
    fa, fb = ctx.fpfh_dev(ca, r, resident=True)[2], ctx.fpfh_dev(cb, r, resident=True)[2]
    index, ki = ctx.iss_keypoints_dev(ca, r, r / 2, per_point=False)
    sel = ctx.select_features(fa, index)
    full_s, full_corr = timed_match(ctx, fa, fb, args.warmup, args.iters)
    key_s, key_corr = timed_match(ctx, sel, fb, args.warmup, args.iters)
    row = {"what": "match", "ns": n, "nt": n, "radius": r, "salient_radius": r, "non_max_radius": r / 2, "keypoints": len(index),
           "keypoint_share": len(index) / n, "full_match_ms": 1e3 * full_s, "full_mutual_correspondences": full_corr,
           "keypoint_match_ms": 1e3 * key_s, "keypoint_mutual_correspondences": key_corr, "iters": args.iters}
    print(json.dumps(row), flush=True)
    rows.append(row)
    for c in (sel, fa, fb, ca, cb):
        c.free()
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
