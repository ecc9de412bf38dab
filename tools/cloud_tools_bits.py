"""Print the cloud tools' bits from one build of the library, to compare two builds (not part of bench.py).

Normals, the outlier filter (both modes), the components (with and without keep_largest), the subsample, the consistent
orientation (both modes), the smoothing, the distances, M3C2, FPFH and its match, the ISS keypoints, the merge (fused and
concatenated), the two ICP linearisations, the resident forms that return a cloud (each downloaded) and the multi-scale normals, each on
tests/golden/g9_room.npz and on a seeded synthetic sheet: one line per call with a sha1 of every returned array and every summary
field (floats in hex).  One process per library:

    python tools/cloud_tools_bits.py path/to/parent/libplade_hip.so > old.txt
    python tools/cloud_tools_bits.py plade_amd/libplade_hip.so      > new.txt
    cmp old.txt new.txt && sha1sum new.txt

A tool that only the newer build has adds lines (the multi-scale normals: `scales_*`, then DBSCAN: `dbscan*`, at the end of each
block); run the older build from its own checkout and compare the lines both print.
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import plade_amd  # noqa: E402


def bits(v):
    """Every array as a sha1 of its bytes, every float in hex, containers in order (dicts by key)."""
    if isinstance(v, np.ndarray):
        return f"{v.dtype}{list(v.shape)}:" + hashlib.sha1(np.ascontiguousarray(v).tobytes()).hexdigest()[:16]
    if isinstance(v, dict):
        return "{" + " ".join(f"{k}={bits(v[k])}" for k in sorted(v)) + "}"
    if isinstance(v, (tuple, list)):
        return "(" + " ".join(bits(x) for x in v) + ")"
    if isinstance(v, (float, np.floating)):
        return float(v).hex()
    return repr(v)


def sheet(n, seed):
    """A wavy sheet over a 4 x 4 square, noisy z, unit normals, a few far outliers: (n, 6) float32."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0.0, 4.0, size=(n, 2))
    z = 0.2 * np.sin(1.5 * xy[:, 0]) + rng.normal(scale=0.01, size=n)
    z[:: 97] += rng.uniform(0.5, 1.0, size=len(z[:: 97]))
    nr = np.stack([-0.3 * np.cos(1.5 * xy[:, 0]), np.zeros(n), np.ones(n)], 1) + rng.normal(scale=0.05, size=(n, 3))
    nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    return np.ascontiguousarray(np.concatenate([xy, z[:, None], nr], 1), dtype=np.float32)


def run(ctx, name, tgt, src, T, r):
    """One line per call; r: a radius at which a point has a dozen neighbours."""
    out = []

    def line(tag, v):
        out.append(f"{name} {tag} {bits(v)}")

    xyz = np.ascontiguousarray(tgt[:, :3])
    line("normals", ctx.estimate_normals(xyz, k=16, curvature=True, neighbours=True))
    line("outliers_stat", ctx.remove_outliers(tgt, mode="statistical", k=16, alpha=1.0))
    line("outliers_radius", ctx.remove_outliers(tgt, mode="radius", radius=r, min_neighbours=6))
    line("components", ctx.connected_components(tgt, 0.5 * r, min_size=3))
    line("components_largest", ctx.connected_components(tgt, 0.5 * r, min_size=3, keep_largest=2))
    line("subsample", ctx.subsample(tgt, 0.7 * r, seed=5))
    line("orient_vote", ctx.orient_consistent(tgt, r, mode=plade_amd.ORIENT_VOTE, viewpoint=(0.0, 0.0, 10.0)))
    line("orient_extreme", ctx.orient_consistent(tgt, r, mode=plade_amd.ORIENT_EXTREME, direction=(0.0, 0.0, 1.0), inward=1))
    line("smooth", ctx.smooth_cloud(tgt, r, moments=True))
    line("distances", ctx.cloud_distances(tgt, src, 2.0 * r, T=T))
    line("m3c2", ctx.m3c2(tgt[::3], tgt, src, r, 4.0 * r, T=T, moments=True))
    dt, it = ctx.fpfh(tgt, 2.0 * r, seams=True)
    ds, is_ = ctx.fpfh(src, 2.0 * r, seams=True)
    line("fpfh_tgt", (dt, it))
    line("fpfh_src", (ds, is_))
    line("match", ctx.match_features(ds, dt, mutual=True, max_ratio=0.9))
    line("match_plain", ctx.match_features(ds, dt, mutual=False))
    line("iss", ctx.iss_keypoints(tgt, 2.0 * r, seams=True))
    line("merge_fused", ctx.merge_clouds([tgt, src], [None, T], leaf=r))
    line("merge_cat", ctx.merge_clouds([tgt, src], [None, T], leaf=0.0))
    for c in (None, (3.0, -2.0, 0.5)):
        line("icp_linearize", ctx.icp_linearize(tgt, np.ascontiguousarray(src[:, :3]), T, 2.0 * r, center=c))
        line("gicp_linearize", ctx.gicp_linearize(tgt, src, T, 2.0 * r, center=c))

    # the resident forms that return a cloud: the call's own outputs, then the cloud's rows
    def resident(tag, res):
        cloud, rest = (res[0], res[1:]) if isinstance(res, tuple) else (res, ())
        line(tag, (rest, cloud.download()))
        cloud.free()

    ct, cs = ctx.upload(tgt), ctx.upload(src)
    resident("outliers_stat_dev", ctx.remove_outliers_dev(ct, mode="statistical", k=16, alpha=1.0, info=True))
    resident("outliers_radius_dev", ctx.remove_outliers_dev(ct, mode="radius", radius=r, min_neighbours=6, info=True))
    resident("components_dev", ctx.filter_components_dev(ct, 0.5 * r, min_size=3, keep_largest=2, info=True))
    resident("subsample_dev", ctx.subsample_dev(ct, 0.7 * r, seed=5, info=True))
    resident("orient_vote_dev", ctx.orient_consistent_dev(ct, r, mode=plade_amd.ORIENT_VOTE, viewpoint=(0.0, 0.0, 10.0), info=True))
    resident("orient_extreme_dev", ctx.orient_consistent_dev(ct, r, mode=plade_amd.ORIENT_EXTREME, inward=1, info=True))
    resident("smooth_dev", ctx.smooth_cloud_dev(ct, r, info=True))
    resident("smooth_keep_normals_dev", ctx.smooth_cloud_dev(ct, r, fit_normals=False, info=True))
    resident("upload_xyz", ctx.upload_xyz(xyz, k=16))
    resident("merge_fused_dev", ctx.merge_clouds_dev([ct, cs], [None, T], leaf=r, info=True))
    resident("merge_cat_dev", ctx.merge_clouds_dev([ct, cs], [None, T], leaf=0.0, info=True))
    # (the multi-scale normals come last: the lines above keep their place and their sha1 from build to build)
    rs = (0.7 * r, r, 1.5 * r)
    line("scales_planarity", ctx.scale_features(tgt, rs, mode=0, moments=True))
    line("scales_variation_own_normals", ctx.scale_features(tgt, rs, mode=1, orient=1, query_index=np.arange(0, len(tgt), 3), moments=True))
    resident("scales_dev", ctx.scale_normals_dev(ct, rs, orient=1, info=True))
    # (DBSCAN, added after them, the same way)
    line("dbscan", ctx.dbscan(tgt, 0.5 * r, min_points=4, min_size=3, keep_largest=2))
    resident("dbscan_dev", ctx.dbscan_dev(ct, 0.5 * r, min_points=4, min_size=3, keep_largest=2, info=True))
    ct.free()
    cs.free()
    return out


def main():
    plade_amd.load_library(sys.argv[1] if len(sys.argv) > 1 else plade_amd.LIB_PATH)
    ctx = plade_amd.Context(0)
    z = np.load(os.path.join(ROOT, "tests", "golden", "g9_room.npz"))
    tgt, src, gt = z["target"], z["source"], z["groundtruth"]
    ext = tgt[:, :3].max(0) - tgt[:, :3].min(0)
    area = 2.0 * (ext[0] * ext[1] + ext[1] * ext[2] + ext[0] * ext[2])
    out = run(ctx, "g9_room", tgt, src, np.asarray(gt, np.float64), float(np.sqrt(12.0 * area / (np.pi * len(tgt)))))
    a, b = sheet(40000, 7), sheet(30011, 8)
    T = np.eye(4)
    T[:3, 3] = (0.01, -0.02, 0.015)
    out += run(ctx, "sheet", a, b, T, float(np.sqrt(12.0 * 16.0 / (np.pi * len(a)))))
    ctx.close()
    print("\n".join(out))


if __name__ == "__main__":
    main()
