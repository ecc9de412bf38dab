"""Print the bits of the two ICP refinements from one build of the library, to compare two builds (not part of bench.py).

On tests/golden/g8_polyhedron.npz and g9_room.npz: plade_icp_linearize and plade_gicp_linearize (epsilon 1e-3 and 1) -- ground
truth and a 0.03 perturbation, d = 0.025 D and 0.0025 D, about the origin and about (3, -2, 0.5) -- one line each with a hash of
the correspondences and the moments in hex; plade_refine_icp and plade_refine_gicp (epsilon 1e-3 and 1) from three starts,
uncapped and capped at 3 iterations, and plade_refine_icp_dev / plade_refine_gicp_dev from the first start, one line each with
T_out in hex, the result and the sorted keys of plade_stats_get (the keys only: the times differ).  One process per library:

    python tools/icp_bits.py path/to/parent/libplade_hip.so > old.txt
    python tools/icp_bits.py plade_amd/libplade_hip.so      > new.txt
    cmp old.txt new.txt && sha1sum new.txt
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import plade_amd  # noqa: E402


def main():
    plade_amd.load_library(sys.argv[1] if len(sys.argv) > 1 else plade_amd.LIB_PATH)
    import icp_restate as R
    ctx = plade_amd.Context(0, orient_normals=1)
    out = []

    def refined(tag, call):
        try:
            T, info = call()
        except plade_amd.PladeError as e:      # a failed refinement: T_in, the result and the message
            T, info = e.T, dict(e.info, error=str(e))
        out.append(tag + " " + T.tobytes().hex() + " " + repr(sorted(info.items())) + " " + " ".join(sorted(ctx.stats())))

    for scene in ("g8_polyhedron.npz", "g9_room.npz"):
        z = np.load(os.path.join(ROOT, "tests", "golden", scene))
        tgt, src, gt = z["target"], np.ascontiguousarray(z["source"]), z["groundtruth"]
        D = R.Target(tgt).diag
        out.append("scene " + scene)
        S = np.ascontiguousarray(src[:, :3])
        for T in (gt, R.perturb(gt, 0.03, 0.03, seed=5)):
            for d in (0.025 * D, 0.0025 * D):
                for c in (None, (3.0, -2.0, 0.5)):
                    corr, mom = ctx.icp_linearize(tgt, S, T, d, center=c)
                    out.append("lin " + hashlib.sha1(corr.tobytes()).hexdigest()[:12] + " " + mom.tobytes().hex())
                    for eps in (1e-3, 1.0):
                        corr, mom = ctx.gicp_linearize(tgt, src, T, d, epsilon=eps, center=c)
                        out.append(f"glin {eps} " + hashlib.sha1(corr.tobytes()).hexdigest()[:12] + " " + mom.tobytes().hex())
        starts = (gt, R.perturb(gt, 0.05, 0.05, seed=1), R.perturb(gt, 0.1, 0.1, seed=2))
        for T0 in starts:
            refined("refine", lambda: ctx.refine_icp(tgt, src, T0))
            refined("refine3", lambda: ctx.refine_icp(tgt, src, T0, max_iterations=3))
            for eps in (1e-3, 1.0):
                refined(f"grefine {eps}", lambda: ctx.refine_gicp(tgt, src, T0, epsilon=eps))
                refined(f"grefine3 {eps}", lambda: ctx.refine_gicp(tgt, src, T0, epsilon=eps, max_iterations=3))
        ct, cs = ctx.upload(tgt), ctx.upload(src)
        refined("refine_dev", lambda: ctx.refine_icp_dev(ct, cs, starts[1]))
        refined("grefine_dev", lambda: ctx.refine_gicp_dev(ct, cs, starts[1]))
        ct.free(); cs.free()
    ctx.close()
    print("\n".join(out))


if __name__ == "__main__":
    main()
