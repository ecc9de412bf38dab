"""Time plade_cloud_cluster_dbscan_dev on synthetic scenes (not part of bench.py).

The cloud is resident (plade_cloud_upload), so the numbers exclude the upload.  The library records HIP events on its stream around
the five parts (plade_stats_get: dbscan_grid_s, dbscan_core_s = the counting walk, dbscan_link_s = the union-find over the core-core
edges and the border rule, dbscan_label_s = roots, ids, sizes and the selection, dbscan_compact_s = scan, kept list and row gather).
Median of --iters calls after --warmup calls, one fresh process per row.  The clouds are the targets of make_pair(n); the radius is
a multiple of the cloud's average spacing.

The yardstick, in the same process, is the closest thing the library offered before: remove_outliers_dev(mode="radius", radius=r,
min_neighbours=min_points - 1) followed by filter_components_dev(r) on its result -- two grids, two walks, two keep tails, the sum
of the two calls' event spans.  It computes something else: it drops the border points, and the components it finds are those of
the thinned cloud.

    python tools/dbscan_time.py [--sizes 100000 1000000] [--factors 2.5 5] [--min-points 4 16] [--out profiles/dbscan_time.json]

writes the rows to --out and prints them, then the table of DESIGN.md section 30.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARTS = ("grid", "core", "link", "label", "compact")
OUTLIER_PARTS = ("grid", "search", "reduce", "compact")
COMPONENT_PARTS = ("grid", "link", "label", "compact")


def one_row(n, factor, min_points, warmup, iters, lib):
    import plade_amd
    from plade_amd.synth import make_pair
    if lib:
        plade_amd.load_library(lib)
    ctx = plade_amd.Context(0)
    tg = make_pair(n)[0]
    spacing = float(ctx.average_spacing(tg))
    r = float(np.float32(factor * spacing))
    cloud = ctx.upload(tg)
    t = {p: [] for p in PARTS}
    chain = []
    info = None
    for it in range(warmup + iters):
        out, _, info = ctx.dbscan_dev(cloud, r, min_points, info=True)
        s = ctx.stats()
        out.free()
        if it >= warmup:
            for p in PARTS:
                t[p].append(s[f"dbscan_{p}_s"])
    chain_kept = 0
    for it in range(warmup + iters):
        dense = ctx.remove_outliers_dev(cloud, mode="radius", radius=r, min_neighbours=min_points - 1)
        a = sum(ctx.stats()[f"outliers_{p}_s"] for p in OUTLIER_PARTS)
        comp = ctx.filter_components_dev(dense, r)
        b = sum(ctx.stats()[f"components_{p}_s"] for p in COMPONENT_PARTS)
        chain_kept = comp.n
        comp.free()
        dense.free()
        if it >= warmup:
            chain.append(a + b)
    cloud.free()
    ctx.close()
    ms = {p: 1e3 * float(np.median(t[p])) for p in PARTS}
    totals = 1e3 * np.sum([t[p] for p in PARTS], axis=0)
    chain_ms = 1e3 * np.asarray(chain)
    return {"n": n, "factor": factor, "radius": r, "spacing": spacing, "min_points": min_points, **{f"{p}_ms": ms[p] for p in PARTS},
            "total_ms": float(np.median(totals)), "total_min_ms": float(totals.min()), "total_max_ms": float(totals.max()),
            "chain_ms": float(np.median(chain_ms)), "chain_min_ms": float(chain_ms.min()), "chain_max_ms": float(chain_ms.max()),
            "dbscan_over_chain": float(np.median(totals) / np.median(chain_ms)), "clusters": int(info["clusters"]),
            "core": int(info["core"]), "border": int(info["border"]), "noise": int(info["noise"]), "chain_kept": int(chain_kept),
            "iters": iters}


def design_table(rows):
    """the rows as the markdown table of DESIGN.md section 30"""
    out = ["| points | r / spacing | min_points | clusters | core / border / noise | grid | core | link | label | scan + gather | **total** "
           "(min .. max) | outlier filter + components (min .. max) | total / chain |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for w in rows:
        n = f"{w['n'] // 1000000}M" if w["n"] % 1000000 == 0 else str(w["n"])
        out.append(f"| {n} | {w['factor']:g} | {w['min_points']} | {w['clusters']} | {w['core']} / {w['border']} / {w['noise']} | "
                   f"{w['grid_ms']:.2f} ms | {w['core_ms']:.2f} ms | {w['link_ms']:.2f} ms | {w['label_ms']:.2f} ms | {w['compact_ms']:.2f} ms | "
                   f"**{w['total_ms']:.2f} ms** ({w['total_min_ms']:.2f} .. {w['total_max_ms']:.2f}) | {w['chain_ms']:.2f} ms "
                   f"({w['chain_min_ms']:.2f} .. {w['chain_max_ms']:.2f}) | {w['dbscan_over_chain']:.2f} |")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--factors", type=float, nargs="+", default=[2.5, 5.0])
    ap.add_argument("--min-points", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dbscan_time.json"))
    ap.add_argument("--lib", default=None, help="another build of libplade_hip.so (a variant of a kernel, for one comparison)")
    ap.add_argument("--row", type=float, nargs=3, metavar=("N", "FACTOR", "MIN_POINTS"), help="one row in this process, as JSON on stdout")
    args = ap.parse_args()
    if args.row:
        print(json.dumps(one_row(int(args.row[0]), args.row[1], int(args.row[2]), args.warmup, args.iters, args.lib)), flush=True)
        return
    rows = []
    for n in args.sizes:
        for f in args.factors:
            for mp in args.min_points:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--row", str(n), str(f), str(mp), "--warmup", str(args.warmup),
                                    "--iters", str(args.iters)] + (["--lib", args.lib] if args.lib else []), capture_output=True, text=True, timeout=600)
                if r.returncode != 0:     # nothing more on the GPU after a row that failed
                    sys.exit(f"row {n} {f} {mp} failed ({r.returncode}):\n{r.stdout}{r.stderr}")
                row = json.loads(r.stdout.strip().split("\n")[-1])
                print(json.dumps(row), flush=True)
                rows.append(row)
    with open(args.out, "w") as f:
        json.dump(rows, f, indent=1)
    print(design_table(rows))


if __name__ == "__main__":
    main()
