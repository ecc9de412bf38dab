"""Time plade_cloud_scale_normals_dev against S single-scale walks on synthetic scenes (not part of bench.py).

The cloud is resident (plade_cloud_upload), so the numbers exclude the upload.  The library records HIP events on its stream around
the three parts (plade_stats_get: scales_grid_s, scales_walk_s = the walk and the fit kernel, scales_reduce_s).  The yardstick is
what a caller had before: S calls of plade_cloud_smooth_dev, one per radius -- the existing single-scale walk with the same
neighbourhoods, one grid and one walk per call (smooth_grid_s + smooth_fit_s + smooth_reduce_s, summed over the S calls;
k_smooth.hip is the parent's, unchanged).  Median of --iters calls after --warmup calls; every (size, S) runs in a fresh process.
The clouds are the targets of make_pair(n); the S radii go from 2 to 6 times the cloud's average spacing in equal steps.

    python tools/scales_time.py [--sizes 100000 1000000] [--scales 2 4 8] [--out profiles/scales_time.json]

writes the rows to --out (default: profiles/scales_time.json) and prints them, then the table of DESIGN.md section 29.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARTS = ("grid", "walk", "reduce")
SMOOTH_PARTS = ("grid", "fit", "reduce")


def one(n, S, warmup, iters):
    import plade_amd
    from plade_amd.synth import make_pair
    ctx = plade_amd.Context(0)
    tg = make_pair(n)[0]
    spacing = float(ctx.average_spacing(tg))
    radii = [float(np.float32((2.0 + 4.0 * s / (S - 1)) * spacing)) for s in range(S)]
    cloud = ctx.upload(tg)
    t = {p: [] for p in PARTS}
    info = None
    for it in range(warmup + iters):
        out, info = ctx.scale_normals_dev(cloud, radii, info=True)
        s = ctx.stats()
        out.free()
        if it >= warmup:
            for p in PARTS:
                t[p].append(s[f"scales_{p}_s"])
    single = []
    for it in range(warmup + iters):
        total = 0.0
        for r in radii:
            out = ctx.smooth_cloud_dev(cloud, r)
            s = ctx.stats()
            out.free()
            total += sum(s[f"smooth_{p}_s"] for p in SMOOTH_PARTS)
        if it >= warmup:
            single.append(total)
    cloud.free()
    ctx.close()
    ms = {p: 1e3 * float(np.median(t[p])) for p in PARTS}
    single_ms = 1e3 * float(np.median(single))
    return {"n": n, "scales": S, "radii": radii, "average_spacing": spacing, **{f"{p}_ms": ms[p] for p in PARTS},
            "total_ms": sum(ms.values()), "single_scale_calls_ms": single_ms, "speedup": single_ms / sum(ms.values()),
            "fitted": info["fitted"], "chosen_hist": list(info["chosen_hist"]), "max_count": info["max_count"], "iters": iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--scales", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scales_time.json"))
    ap.add_argument("--one", type=int, nargs=2, metavar=("N", "S"), help="one (size, scales) in this process: prints its row")
    args = ap.parse_args()
    if args.one:
        print("@row " + json.dumps(one(args.one[0], args.one[1], args.warmup, args.iters)), flush=True)
        return
    rows = []
    for n in args.sizes:
        for S in args.scales:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(n), str(S), "--warmup", str(args.warmup),
                                "--iters", str(args.iters)], capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit(f"scales_time: the run of n = {n}, S = {S} failed ({r.returncode}):\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
            row = json.loads([l for l in r.stdout.split("\n") if l.startswith("@row ")][-1][5:])
            print(json.dumps(row), flush=True)
            rows.append(row)
    with open(args.out, "w") as f:
        json.dump(rows, f, indent=1)
    print(design_table(rows))


def design_table(rows):
    """the rows as the markdown table of DESIGN.md section 29"""
    out = ["| points | scales | largest neighbourhood | grid | walk + fit | reduce | **one call** | S single-scale calls | ratio |",
           "|---|---|---|---|---|---|---|---|---|"]
    for w in rows:
        n = f"{w['n'] // 1000000}M" if w["n"] % 1000000 == 0 else str(w["n"])
        out.append(f"| {n} | {w['scales']} | {w['max_count']} | {w['grid_ms']:.2f} ms | {w['walk_ms']:.2f} ms | {w['reduce_ms']:.2f} ms | "
                   f"**{w['total_ms']:.2f} ms** | {w['single_scale_calls_ms']:.2f} ms | {w['speedup']:.2f} |")
    return "\n".join(out)


if __name__ == "__main__":
    main()
