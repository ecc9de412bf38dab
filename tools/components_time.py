"""Time plade_cloud_filter_components_dev on synthetic scenes (not part of bench.py).

The cloud is resident (plade_cloud_upload), so the numbers exclude the upload.  The library records HIP events on its stream
around the four parts (plade_stats_get: components_grid_s, components_link_s = the union-find over the edges, components_label_s =
roots, ids, sizes and the selection, components_compact_s = scan, kept list and row gather).  Median of --iters calls after
--warmup calls.  The clouds are the targets of make_pair(n); the radius is a multiple of the cloud's average spacing.

The yardstick is the radius outlier filter at the same radius on the same cloud with per-point counts
(remove_outliers(mode="radius", per_point=True), outliers_search_s): it walks the same 27-cell blocks in full and tests the same
predicate, without the unions.  link_over_search = components_link_s / outliers_search_s.

    python tools/components_time.py [--sizes 1000000 10000000] [--factors 1.5 2.5 5] [--out profiles/components_time.json]

writes the rows to --out (default: profiles/components_time.json) and prints them, then the table of DESIGN.md section 14.
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

PARTS = ("grid", "link", "label", "compact")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--factors", type=float, nargs="+", default=[1.5, 2.5, 5.0])
    ap.add_argument("--min-size", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_time.json"))
    args = ap.parse_args()
    ctx = plade_amd.Context(0)
    rows = []
    for n in args.sizes:
        tg = make_pair(n)[0]
        spacing = float(ctx.average_spacing(tg))
        cloud = ctx.upload(tg)
        for f in args.factors:
            r = float(np.float32(f * spacing))
            t = {p: [] for p in PARTS}
            comps = kept = 0
            for it in range(args.warmup + args.iters):
                out = ctx.filter_components_dev(cloud, r, min_size=args.min_size)
                s = ctx.stats()
                out.free()
                if it >= args.warmup:
                    for p in PARTS:
                        t[p].append(s[f"components_{p}_s"])
                    comps, kept = int(s["components_count"]), int(s["components_kept"])
            search = []
            mean_nb = 0.0
            for it in range(args.warmup + args.iters):
                info = ctx.remove_outliers(tg, mode="radius", radius=r, min_neighbours=1, per_point=True)[2]
                if it >= args.warmup:
                    search.append(ctx.stats()["outliers_search_s"])
                    mean_nb = float(info["count"].mean())
            ms = {p: 1e3 * float(np.median(t[p])) for p in PARTS}
            search_ms = 1e3 * float(np.median(search))
            row = {"n": n, "factor": f, "radius": r, "spacing": spacing, "min_size": args.min_size,
                   **{f"{p}_ms": ms[p] for p in PARTS}, "total_ms": sum(ms.values()), "radius_search_ms": search_ms,
                   "link_over_search": ms["link"] / search_ms, "mean_neighbours": mean_nb, "components": comps, "kept": kept,
                   "iters": args.iters}
            print(json.dumps(row), flush=True)
            rows.append(row)
        cloud.free()
    ctx.close()
    with open(args.out, "w") as f:
        json.dump(rows, f, indent=1)
    print(design_table(rows))


def design_table(rows):
    """the rows as the markdown table of DESIGN.md section 14"""
    out = ["| points | r / spacing | neighbours within r | components | grid | link | label | scan + gather | **total** | radius search "
           "| link / search |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for w in rows:
        n = f"{w['n'] // 1000000}M" if w["n"] % 1000000 == 0 else str(w["n"])
        out.append(f"| {n} | {w['factor']:g} | {w['mean_neighbours']:.1f} | {w['components']:,} | {w['grid_ms']:.2f} ms | "
                   f"{w['link_ms']:.2f} ms | {w['label_ms']:.2f} ms | {w['compact_ms']:.2f} ms | **{w['total_ms']:.2f} ms** | "
                   f"{w['radius_search_ms']:.2f} ms | {w['link_over_search']:.1f} |".replace(",", " "))
    return "\n".join(out)


if __name__ == "__main__":
    main()
