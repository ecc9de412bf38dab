"""numpy restatement of the plane-to-plane (generalized) ICP refinement (plade_amd/csrc/gicp.h).

numpy only.  The match is the point-to-plane ICP's exact float32 argmin (tests/icp_restate.py), with the extra conditions on the two
normals; every fp64 term of the linearisation follows the written operation order of gicp.h, so numpy float64 gives the kernel's term
bit for bit, and only the summation (math.fsum here) differs.  The sample is the merge restatement (tests/merge_restate.py) of one
cloud under the identity; solve, update (icp_restate.step on the 21 + 6 moments) and schedule are icp_restate's.
"""
import math

import numpy as np

import icp_restate as R
import merge_restate as MR

F32 = np.float32
N_MOMENTS = 30
TOO_FEW, DEGENERATE = R.TOO_FEW, R.DEGENERATE


def metric(nh, ah, eps):
    """The six entries (M00, M01, M02, M11, M12, M22) of M = adj(Sigma) / det, Sigma = 2 I - k nh nh^T - k ah ah^T, k = 1 - eps, for
    arrays of unit vectors nh, ah (each a list of three fp64 arrays), in the written order."""
    k = 1.0 - eps
    S = {}
    for i in range(3):
        for j in range(i, 3):
            dd = 2.0 if i == j else 0.0
            S[i, j] = (dd - k * (nh[i] * nh[j])) - k * (ah[i] * ah[j])
    C00 = S[1, 1] * S[2, 2] - S[1, 2] * S[1, 2]
    C01 = S[0, 2] * S[1, 2] - S[0, 1] * S[2, 2]
    C02 = S[0, 1] * S[1, 2] - S[0, 2] * S[1, 1]
    C11 = S[0, 0] * S[2, 2] - S[0, 2] * S[0, 2]
    C12 = S[0, 1] * S[0, 2] - S[0, 0] * S[1, 2]
    C22 = S[0, 0] * S[1, 1] - S[0, 1] * S[0, 1]
    det = (S[0, 0] * C00 + S[0, 1] * C01) + S[0, 2] * C02
    return C00 / det, C01 / det, C02 / det, C11 / det, C12 / det, C22 / det


def unit(v):
    """v / sqrt((v0 v0 + v1 v1) + v2 v2) for a list of three fp64 arrays."""
    ln = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    return [v[0] / ln, v[1] / ln, v[2] / ln]


def terms(T, c, X, q, n, m, eps):
    """The 30 per-correspondence terms (a list of fp64 arrays): X = double(s), q = double(q_j), n = double(n_j), m = double(m) as
    (K, 3) arrays; T fp64 4 x 4, c the centre."""
    p = [((T[r, 0] * X[:, 0] + T[r, 1] * X[:, 1]) + T[r, 2] * X[:, 2]) + T[r, 3] for r in range(3)]
    e = [p[r] - q[:, r] for r in range(3)]
    u = [p[r] - c[r] for r in range(3)]
    nh = unit([n[:, 0], n[:, 1], n[:, 2]])
    ah = unit([(T[r, 0] * m[:, 0] + T[r, 1] * m[:, 1]) + T[r, 2] * m[:, 2] for r in range(3)])
    M00, M01, M02, M11, M12, M22 = metric(nh, ah, eps)
    M = [[M00, M01, M02], [M01, M11, M12], [M02, M12, M22]]
    w = [(M[r][0] * e[0] + M[r][1] * e[1]) + M[r][2] * e[2] for r in range(3)]
    G = [[M[r][2] * u[1] - M[r][1] * u[2], M[r][0] * u[2] - M[r][2] * u[0], M[r][1] * u[0] - M[r][0] * u[1], M[r][0], M[r][1], M[r][2]]
         for r in range(3)]

    def JT(row, v0, v1, v2):
        return (v2 * u[1] - v1 * u[2], v0 * u[2] - v2 * u[0], v1 * u[0] - v0 * u[1], v0, v1, v2)[row]

    out = [JT(a, G[0][b], G[1][b], G[2][b]) for a in range(6) for b in range(a, 6)]
    out += [JT(a, w[0], w[1], w[2]) for a in range(6)]
    out.append((e[0] * w[0] + e[1] * w[1]) + e[2] * w[2])
    out.append((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    out.append(np.ones(len(X)))
    return out


def _len2(v):
    v = v.astype(np.float64)
    return (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]


def match(target, src6, T, d):
    """corr (int32, -1: none): the ICP's argmin, kept when the distance passes, n_j is finite with non-zero length and the source's
    own normal is finite with non-zero length.  No second choice."""
    src6 = np.asarray(src6, F32)
    nearest = R.Target.__new__(R.Target)
    nearest.__dict__.update(target.__dict__)
    nearest.finite = np.ones(len(target.t), bool)                       # the plain nearest point first
    corr = nearest.match(R.transform_f32(T, src6[:, :3]), d)
    with np.errstate(invalid="ignore", over="ignore"):
        ok_t = np.isfinite(target.t[:, 3:6]).all(1) & (_len2(target.t[:, 3:6]) > 0)
        ok_s = np.isfinite(src6[:, 3:6]).all(1) & (_len2(src6[:, 3:6]) > 0)
    sel = corr >= 0
    bad = sel & ~(ok_t[np.where(sel, corr, 0)] & ok_s)
    corr[bad] = -1
    return corr


def linearize(tgt, src6, T, d, eps, center=None, sums="fsum"):
    """(corr, moments30, abs_moments30) of one match + linearise pass at stage distance d with the fp64 4 x 4 T about `center`
    (default: the origin).  tgt: an (N, 6) array or an icp_restate.Target.  sums: "fsum" (exact), or a seeded permutation of the
    plain left-to-right sum ("perm<seed>": the spread of the summation order, for the tolerances)."""
    target = tgt if isinstance(tgt, R.Target) else R.Target(tgt)
    T = np.asarray(T, np.float64)
    src6 = np.ascontiguousarray(src6, F32)
    c = np.zeros(3) if center is None else np.asarray(center, np.float64)
    eps = float(eps) if eps else 1e-3
    corr = match(target, src6, T, d)
    sel = corr >= 0
    j = corr[sel]
    tt = terms(T, c, src6[sel, :3].astype(np.float64), target.t[j, :3].astype(np.float64), target.t[j, 3:6].astype(np.float64),
               src6[sel, 3:6].astype(np.float64), eps)
    if sums == "fsum":
        mom = np.array([math.fsum(t) for t in tt])
    else:
        order = np.random.default_rng(int(sums[4:])).permutation(int(sel.sum()))
        mom = np.array([np.cumsum(t[order])[-1] if len(t) else 0.0 for t in tt])
    absm = np.array([math.fsum(np.abs(t)) for t in tt])
    return corr, mom, absm


def sample(src6, leaf):
    """S: the source voxel-fused under the merge's rules at `leaf` (fp32), (n, 6) float32 rows in ascending voxel order."""
    return MR.merge([np.ascontiguousarray(src6, F32)], leaf=F32(leaf))[0]


def refine(tgt, src6, T_in, S=None, trace=None, epsilon=0.0, sums="fsum", **params):
    """The whole refinement: (T fp64 4 x 4 -- T_in on failure --, info dict with the plade_gicp_result fields).  S: the sample rows
    (default: sample(src6, resolved leaf))."""
    target = tgt if isinstance(tgt, R.Target) else R.Target(tgt)
    c = R.resolve(target.diag, amax=target.amax, **params)
    if S is None:
        S = sample(src6, c["leaf"])
    S = np.ascontiguousarray(S, F32)
    sbar = R.sample_mean(S)
    T0 = np.asarray(T_in, F32).astype(np.float64)
    T = T0.copy()
    stage, it = 0, 0
    info = dict(iterations=0, stages=1, converged=False, failure=0, correspondences=0, samples=len(S), rmse=0.0, fitness=0.0,
                final_dist=c["dists"][0], cost=0.0)
    while True:
        d = c["dists"][stage]
        ck = R.apply(T, sbar)
        _, m, _ = linearize(target, S, T, d, epsilon, center=ck, sums=sums)
        count = int(m[29])
        info.update(correspondences=count, rmse=float(np.sqrt(m[28] / count)) if count else 0.0, cost=float(m[27] / count) if count else 0.0,
                    fitness=count / len(S) if len(S) else 0.0, final_dist=d, stages=stage + 1)
        if count < c["min_corr"]:
            info.update(failure=TOO_FEW, iterations=it)
            return T0, info
        x, T = R.step(m, T, ck)
        if x is None:
            info.update(failure=DEGENERATE, iterations=it)
            return T0, info
        it += 1
        info["iterations"] = it
        if np.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) < c["eps_rot"] and \
                np.sqrt((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5]) < c["eps_trans"]:
            if stage + 1 < len(c["dists"]):
                stage += 1
            else:
                info["converged"] = True
                if trace is not None:
                    trace.append(dict(info))
                return T, info
        if trace is not None:
            trace.append(dict(info))
        if it >= c["max_iter"]:
            return T, info
