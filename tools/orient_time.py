"""Time plade_cloud_orient_normals_dev on synthetic scenes (not part of bench.py).

The cloud is resident (plade_cloud_upload), so the numbers exclude the upload.  The library records HIP events on its stream
around the three parts (plade_stats_get: orient_grid_s, orient_rounds_s = every launch of the Boruvka rounds with the read-back
of the hook count between them, orient_finish_s = anchors, component ids and the scatter to the original order).  Median of
--iters calls after --warmup calls, in this one fresh process.  The clouds are the targets of make_pair(n) with half of the
normals turned round at random; the radius is a multiple of the cloud's average spacing.

The yardstick for "one 27-cell walk" is the components tool at the same radius on the same cloud (components_link_s of
filter_components_dev with min_size = 1: one pass over the same blocks with the same predicate, plus its unions), from the same
job.  rounds_over_link = orient_rounds_s / components_link_s.

    python tools/orient_time.py [--sizes 1000000] [--factors 2 5] [--out profiles/orient_time.json]

writes the rows to --out (default: profiles/orient_time.json) and prints them, then the table of DESIGN.md section 27.
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

PARTS = ("grid", "rounds", "finish")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000])
    ap.add_argument("--factors", type=float, nargs="+", default=[2.0, 5.0])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orient_time.json"))
    args = ap.parse_args()
    ctx = plade_amd.Context(0)
    rows = []
    for n in args.sizes:
        tg = make_pair(n)[0]
        tg[np.random.default_rng(args.seed).random(n) < 0.5, 3:] *= -1
        spacing = float(ctx.average_spacing(tg))
        cloud = ctx.upload(tg)
        for f in args.factors:
            r = float(np.float32(f * spacing))
            t = {p: [] for p in PARTS}
            info = {}
            for it in range(args.warmup + args.iters):
                out, info = ctx.orient_consistent_dev(cloud, r, info=True)
                s = ctx.stats()
                out.free()
                if it >= args.warmup:
                    for p in PARTS:
                        t[p].append(s[f"orient_{p}_s"])
            link = []
            for it in range(args.warmup + args.iters):
                out = ctx.filter_components_dev(cloud, r, min_size=1)
                s = ctx.stats()
                out.free()
                if it >= args.warmup:
                    link.append(s["components_link_s"])
            ms = {p: 1e3 * float(np.median(t[p])) for p in PARTS}
            link_ms = 1e3 * float(np.median(link))
            row = {"n": n, "factor": f, "radius": r, "average_spacing": spacing, "seed": args.seed,
                   **{f"{p}_ms": ms[p] for p in PARTS}, "total_ms": sum(ms.values()), "components_link_ms": link_ms,
                   "rounds_over_link": ms["rounds"] / link_ms, "rounds": int(info["rounds"]), "components": int(info["components"]),
                   "flipped": int(info["flipped"]), "tree_edges": int(info["tree_edges"]), "iters": args.iters}
            print(json.dumps(row), flush=True)
            rows.append(row)
        cloud.free()
    ctx.close()
    with open(args.out, "w") as f:
        json.dump(rows, f, indent=1)
    print(design_table(rows))


def design_table(rows):
    """the rows as the markdown table of DESIGN.md section 27"""
    out = ["| points | radius / average spacing | components | flipped | rounds | grid | rounds | anchors + ids + scatter | **total** | "
           "components link | rounds / link |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for w in rows:
        n = f"{w['n'] // 1000000}M" if w["n"] % 1000000 == 0 else str(w["n"])
        out.append(f"| {n} | {w['factor']:g} | {w['components']:,} | {w['flipped']:,} | {w['rounds']} | {w['grid_ms']:.2f} ms | "
                   f"{w['rounds_ms']:.2f} ms | {w['finish_ms']:.2f} ms | **{w['total_ms']:.2f} ms** | {w['components_link_ms']:.2f} ms | "
                   f"{w['rounds_over_link']:.1f} |".replace(",", " "))
    return "\n".join(out)


if __name__ == "__main__":
    main()
