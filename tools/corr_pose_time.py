"""Time plade_estimate_pose_corr on synthetic correspondence sets (not part of bench.py).

A set of --sizes correspondences (tests/corr_cases.py: --share of them true under a random pose with --noise of Gaussian noise, the
rest uniform in a 10-unit box) is estimated with --hypotheses hypotheses at inlier_dist --dist.  The three spans are the HIP events
the library records on its stream (plade_stats_get): corr_pose_build_s (the upload of the list, the gather, the hypotheses, the scan
and the compaction, up to the one host wait that reads the length of the list), corr_pose_score_s (the counts and the best
hypothesis) and corr_pose_refine_s (the refinement loop and the final sums).  The points' upload and its bounding-box pass come before
the first event and are not in them.  Median of --iters calls after --warmup calls.  There is no earlier implementation to compare with.

    python tools/corr_pose_time.py [--sizes 5000 30000] [--hypotheses 65536 1048576] [--out profiles/corr_pose_time.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import plade_amd  # noqa: E402
import corr_cases  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[5_000, 30_000])
    ap.add_argument("--hypotheses", type=int, nargs="+", default=[65_536, 1_048_576])
    ap.add_argument("--share", type=float, default=0.1)
    ap.add_argument("--noise", type=float, default=0.02)
    ap.add_argument("--dist", type=float, default=0.1)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corr_pose_time.json"))
    args = ap.parse_args()
    ctx = plade_amd.Context(0)
    rows = []
    for M in args.sizes:
        S, Q, corr, T, inl = corr_cases.synthetic(M, args.share, M, noise=args.noise, shuffle=True)
        src, tgt = np.ascontiguousarray(S, np.float32), np.ascontiguousarray(Q, np.float32)
        for H in args.hypotheses:
            spans = {"corr_pose_build_s": [], "corr_pose_score_s": [], "corr_pose_refine_s": []}
            for it in range(args.warmup + args.iters):
                Tg, info = ctx.estimate_pose(src, tgt, corr, args.dist, hypotheses=H)
                s = ctx.stats()
                if it >= args.warmup:
                    for k in spans:
                        spans[k].append(s[k])
            b, sc, rf = (float(np.median(spans[k])) for k in ("corr_pose_build_s", "corr_pose_score_s", "corr_pose_refine_s"))
            R = Tg[:3, :3].astype(np.float64) @ T[:3, :3].T
            row = {"what": "corr_pose", "m": M, "hypotheses": H, "true_share": args.share, "inlier_dist": args.dist,
                   "scored": int(info["scored"]), "best_count": int(info["best_count"]), "inliers": int(info["inliers"]),
                   "refinements": int(info["refinements"]), "build_ms": 1e3 * b, "score_ms": 1e3 * sc, "refine_ms": 1e3 * rf,
                   "total_ms": 1e3 * (b + sc + rf), "score_ns_per_pair": 1e9 * sc / max(int(info["scored"]) * M, 1),
                   "rotation_error_deg": float(np.degrees(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)))),
                   "translation_error": float(np.linalg.norm(Tg[:3, 3] - T[:3, 3])), "iters": args.iters}
            print(json.dumps(row), flush=True)
            rows.append(row)
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
