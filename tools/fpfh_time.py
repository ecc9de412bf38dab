"""Time plade_cloud_fpfh_dev and plade_match_features_dev on resident synthetic scenes (not part of bench.py).

One sampling of a scene of --size points is resident.  The grid build + axes gather, the SPFH walk and the weighting walk are timed
separately with the HIP events the library records on its stream around them (plade_stats_get: fpfh_grid_s, fpfh_spfh_s,
fpfh_weight_s): nothing is uploaded in the timed calls and no per-point array is copied back but the descriptors.  The radius of a
row is chosen so that the median number of counted pairs is about --counts: from a first guess it is scaled twice by
sqrt(target / median) (a surface: the count grows with r^2).  The match is timed (feat_match_s: both searches, the merge, the
filter and the compaction) between the resident descriptors of two samplings of --match-sizes points each, described at the radius
calibrated for the last of --counts.  Median of --iters calls after --warmup calls.  Last, make_pair(--pair-size, seed=0) is
described at a radius calibrated the same way and matched: the number of mutual correspondences and the share of them that the
ground-truth transformation brings within the radius (information for a pose estimator, no threshold).

    python tools/fpfh_time.py [--size 1000000] [--counts 16 64] [--out profiles/fpfh_time.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import plade_amd  # noqa: E402
from plade_amd.synth import make_pair, sample_scene  # noqa: E402


def calibrate(ctx, cloud, n, target):
    r = 0.04 * np.sqrt(1e6 / n) * np.sqrt(target / 16.0)            # a first guess only: the two steps below correct it
    for _ in range(2):
        pairs = ctx.fpfh_dev(cloud, r)[1]["pairs"]
        r *= np.sqrt(target / max(float(np.median(pairs)), 1.0))
    return float(r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1_000_000)
    ap.add_argument("--counts", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--match-sizes", type=int, nargs="+", default=[20_000, 100_000])
    ap.add_argument("--pair-size", type=int, default=20_000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fpfh_time.json"))
    args = ap.parse_args()
    ctx = plade_amd.Context(0)
    rows = []
    A = np.ascontiguousarray(sample_scene(args.size, sample_seed=1))
    ra = ctx.upload(A)
    for target in args.counts:
        r = calibrate(ctx, ra, args.size, target)
        grid, spfh, weight = [], [], []
        for it in range(args.warmup + args.iters):
            desc, info = ctx.fpfh_dev(ra, r, per_point=it == 0)
            if it == 0:
                first = info
            s = ctx.stats()
            if it >= args.warmup:
                grid.append(s["fpfh_grid_s"]); spfh.append(s["fpfh_spfh_s"]); weight.append(s["fpfh_weight_s"])
        g, h, w = float(np.median(grid)), float(np.median(spfh)), float(np.median(weight))
        pairs_total = int(first["pairs"].astype(np.int64).sum())
        row = {"what": "fpfh", "n": args.size, "radius": r, "median_pairs": float(np.median(first["pairs"])), "max_pairs": int(first["max_pairs"]),
               "described": int(first["described"]), "counted_pairs": pairs_total, "grid_ms": 1e3 * g, "spfh_ms": 1e3 * h, "weight_ms": 1e3 * w,
               "total_ms": 1e3 * (g + h + w), "spfh_ns_per_pair": 1e9 * h / max(pairs_total, 1), "iters": args.iters}
        print(json.dumps(row), flush=True)
        rows.append(row)
    ra.free()
    for n in args.match_sizes:
        ca = ctx.upload(np.ascontiguousarray(sample_scene(n, sample_seed=1)))
        cb = ctx.upload(np.ascontiguousarray(sample_scene(n, sample_seed=2)))
        r = calibrate(ctx, ca, n, args.counts[-1])
        fa, fb = ctx.fpfh_dev(ca, r, resident=True)[2], ctx.fpfh_dev(cb, r, resident=True)[2]
        t = []
        for it in range(args.warmup + args.iters):
            corr, info = ctx.match_features_dev(fa, fb)
            if it >= args.warmup:
                t.append(ctx.stats()["feat_match_s"])
        m = float(np.median(t))
        row = {"what": "match", "ns": n, "nt": n, "radius": r, "mutual_correspondences": int(info["n_corr"]), "match_ms": 1e3 * m,
               "ns_per_distance": 1e9 * m / (2.0 * n * n), "iters": args.iters}
        print(json.dumps(row), flush=True)
        rows.append(row)
        for c in (fa, fb, ca, cb):
            c.free()
    tg, sr, T = make_pair(args.pair_size, seed=0)
    ct, cs = ctx.upload(tg), ctx.upload(sr)
    r = calibrate(ctx, ct, len(tg), args.counts[-1])
    (ft, it_, ht), (fs, is_, hs) = ctx.fpfh_dev(ct, r, resident=True), ctx.fpfh_dev(cs, r, resident=True)
    corr = ctx.match_features_dev(hs, ht)[0]
    p = sr[corr[:, 0], :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    true = int((np.linalg.norm(p - tg[corr[:, 1], :3].astype(np.float64), axis=1) < r).sum())
    row = {"what": "pair", "n_target": len(tg), "n_source": len(sr), "radius": r, "described_target": int(it_["described"]),
           "described_source": int(is_["described"]), "mutual_correspondences": len(corr), "true_under_T_gt": true,
           "true_share": true / max(len(corr), 1)}
    print(json.dumps(row), flush=True)
    rows.append(row)
    for c in (ht, hs, ct, cs):
        c.free()
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
