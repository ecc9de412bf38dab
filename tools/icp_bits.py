"""Print the point-to-plane ICP's bits from one build of the library, to compare two builds (not part of bench.py).

plade_icp_linearize on tests/golden/g9_room.npz -- ground truth and a 0.03 perturbation, d = 0.025 D and 0.0025 D, about the origin
and about (3, -2, 0.5): 8 lines with a hash of the correspondences and the 29 moments in hex -- and plade_refine_icp from three
starts, uncapped and capped at 3 iterations: 6 lines with T_out in hex and the result.  One process per library:

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
    z = np.load(os.path.join(ROOT, "tests", "golden", "g9_room.npz"))
    tgt, src, gt = z["target"], z["source"], z["groundtruth"]
    ctx = plade_amd.Context(0, orient_normals=1)
    D = R.Target(tgt).diag
    out = []
    S = np.ascontiguousarray(src[:, :3])
    for T in (gt, R.perturb(gt, 0.03, 0.03, seed=5)):
        for d in (0.025 * D, 0.0025 * D):
            for c in (None, (3.0, -2.0, 0.5)):
                corr, mom = ctx.icp_linearize(tgt, S, T, d, center=c)
                out.append("lin " + hashlib.sha1(corr.tobytes()).hexdigest()[:12] + " " + mom.tobytes().hex())
    for T0 in (gt, R.perturb(gt, 0.05, 0.05, seed=1), R.perturb(gt, 0.1, 0.1, seed=2)):
        T, info = ctx.refine_icp(tgt, src, T0)
        out.append("refine " + T.tobytes().hex() + " " + repr(sorted(info.items())))
        T, info = ctx.refine_icp(tgt, src, T0, max_iterations=3)
        out.append("refine3 " + T.tobytes().hex() + " " + repr(sorted(info.items())))
    ctx.close()
    print("\n".join(out))


if __name__ == "__main__":
    main()
