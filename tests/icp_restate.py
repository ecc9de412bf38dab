"""numpy restatement of the point-to-plane ICP refinement (plade_amd/csrc/icp.h).

numpy only.  The correspondences are the exact float32 set the kernels compute: p' = fp32(R) s + fp32(t) row by row as
((r0 x + r1 y) + r2 z) + t, j = argmin over all target points of (flann_d2(p', q_j), j), kept when flann_d2 < (float)d * (float)d
and n_j is finite.  The argmin is taken by chunked brute force over the target points inside the chunk's bounding box grown by
a little more than d (nothing outside it can be closer than d, so the set is exact).  The linearisation and the loop follow the
same fp64 expressions as the kernels; only the summation order of the moments differs.
"""
import numpy as np

F32 = np.float32
N_MOMENTS = 29
TOO_FEW, DEGENERATE = 1, 2


def voxel_downsample(xyz, leaf):
    """VoxelGrid centroids (PCL's keys: floor(p / leaf) - floor(min / leaf), fp32 sums); ordered by voxel key.  The library's
    plade_voxel_downsample is the reference for S in the GPU tests -- this form is for the host-only tests."""
    p = np.asarray(xyz, F32)[:, :3]
    inv = F32(1.0) / F32(leaf)
    mn = np.floor(p.min(0) * inv).astype(np.int64)
    ijk = np.floor(p * inv).astype(np.int64) - mn
    dims = ijk.max(0) + 1
    key = ijk[:, 0] + dims[0] * (ijk[:, 1] + dims[1] * ijk[:, 2])
    order = np.argsort(key, kind="stable")
    k = key[order]
    heads = np.flatnonzero(np.r_[True, k[1:] != k[:-1]])
    sums = np.add.reduceat(p[order].astype(np.float64), heads, axis=0)
    cnt = np.diff(np.r_[heads, len(k)])
    return (sums / cnt[:, None]).astype(F32)


def transform_f32(T, xyz):
    """p' of the match step: fp32(R), fp32(t), ((r0 x + r1 y) + r2 z) + t in float32."""
    Tf = np.asarray(T, np.float64).astype(F32)
    x, y, z = (np.ascontiguousarray(np.asarray(xyz, F32)[:, k]) for k in range(3))
    return np.stack([((Tf[r, 0] * x + Tf[r, 1] * y) + Tf[r, 2] * z) + Tf[r, 3] for r in range(3)], axis=1)


class Target:
    """Target points (x y z nx ny nz) with the index structure of the chunked brute force."""

    def __init__(self, tgt):
        self.t = np.ascontiguousarray(tgt, F32)
        self.xyz = np.ascontiguousarray(self.t[:, :3])
        self.finite = np.isfinite(self.t[:, 3:6]).all(1)
        self.order = np.argsort(self.xyz[:, 0], kind="stable")
        self.xs = self.xyz[self.order, 0]
        mn, mx = self.xyz.min(0).astype(np.float64), self.xyz.max(0).astype(np.float64)
        self.diag = float(np.linalg.norm(mx - mn))
        self.amax = float(max(np.abs(mn).max(), np.abs(mx).max()))

    def match(self, P, d, chunk=256):
        """j (int32, -1: no correspondence) of the float32 points P at stage distance d."""
        P = np.asarray(P, F32)
        n = len(P)
        d2 = F32(d) * F32(d)
        out = np.full(n, -1, np.int32)
        if n == 0:
            return out
        fin = np.isfinite(P).all(1)
        # chunks of spatially close queries: sort by a coarse cell
        c = max(float(d), self.diag / 32.0)
        lo = np.where(fin[:, None], P, 0).min(0)
        cell = np.floor((np.where(fin[:, None], P, lo) - lo) / c).astype(np.int64)
        qorder = np.lexsort((cell[:, 0], cell[:, 1], cell[:, 2]))
        qorder = qorder[fin[qorder]]
        r = 1.01 * float(d) + 1e-5 * self.amax
        for c0 in range(0, len(qorder), chunk):
            idx = qorder[c0:c0 + chunk]
            Q = P[idx]
            qlo, qhi = Q.min(0).astype(np.float64) - r, Q.max(0).astype(np.float64) + r
            a, b = np.searchsorted(self.xs, qlo[0], "left"), np.searchsorted(self.xs, qhi[0], "right")
            cand = self.order[a:b]
            cy, cz = self.xyz[cand, 1], self.xyz[cand, 2]
            cand = np.sort(cand[(cy >= qlo[1]) & (cy <= qhi[1]) & (cz >= qlo[2]) & (cz <= qhi[2])])
            if len(cand) == 0:
                continue
            C = self.xyz[cand]
            ax = Q[:, 0:1] - C[None, :, 0]
            ay = Q[:, 1:2] - C[None, :, 1]
            az = Q[:, 2:3] - C[None, :, 2]
            dd = ax * ax
            dd += ay * ay
            dd += az * az
            k = np.argmin(dd, axis=1)                      # first of equal minima: the smaller index (cand ascending)
            dmin = dd[np.arange(len(idx)), k]
            j = cand[k]
            ok = (dmin < d2) & self.finite[j]
            out[idx[ok]] = j[ok]
        return out

    def linearize(self, src_xyz, T, d, center=None):
        """(corr, moments, abs_moments): one match + linearise pass at distance d with the fp64 4 x 4 T about the fp64 point
        `center` (default: the origin, as the seam's Python binding; the refinement passes c_k = T_k s-bar)."""
        T = np.asarray(T, np.float64)
        S = np.asarray(src_xyz, F32)[:, :3]
        c = np.zeros(3) if center is None else np.asarray(center, np.float64)
        corr = self.match(transform_f32(T, S), d)
        sel = corr >= 0
        X = S[sel].astype(np.float64)
        j = corr[sel]
        q = self.t[j, :3].astype(np.float64)
        nn = self.t[j, 3:6].astype(np.float64)
        p = [((T[r, 0] * X[:, 0] + T[r, 1] * X[:, 1]) + T[r, 2] * X[:, 2]) + T[r, 3] for r in range(3)]
        res = (nn[:, 0] * (p[0] - q[:, 0]) + nn[:, 1] * (p[1] - q[:, 1])) + nn[:, 2] * (p[2] - q[:, 2])
        u = [p[r] - c[r] for r in range(3)]
        J = [u[1] * nn[:, 2] - u[2] * nn[:, 1], u[2] * nn[:, 0] - u[0] * nn[:, 2], u[0] * nn[:, 1] - u[1] * nn[:, 0],
             nn[:, 0], nn[:, 1], nn[:, 2]]
        terms = [J[u] * J[v] for u in range(6) for v in range(u, 6)] + [J[u] * res for u in range(6)] + [res * res,
                                                                                                        np.ones(len(res))]
        mom = np.array([t.sum() for t in terms])
        absm = np.array([np.abs(t).sum() for t in terms])
        return corr, mom, absm


def sample_mean(S):
    """s-bar: the fp64 mean of the sample's x y z."""
    S = np.asarray(S, F32)[:, :3].astype(np.float64)
    return S.sum(0) / len(S) if len(S) else np.zeros(3)


def apply(T, v):
    """T v in fp64 with the kernels' row order ((r0 x + r1 y) + r2 z) + t (the centre c_k = T_k s-bar)."""
    T = np.asarray(T, np.float64)
    return np.array([((T[r, 0] * v[0] + T[r, 1] * v[1]) + T[r, 2] * v[2]) + T[r, 3] for r in range(3)])


def cholesky_solve(m):
    """x of J^T J x = -J^T r from the 29 moments, or None when a pivot is <= 1e-12 times its own diagonal entry A[j][j]
    (degenerate; an exactly zero column counts).  The test is unchanged when a column is rescaled (units, lever arms)."""
    A = np.zeros((6, 6))
    k = 0
    for u in range(6):
        for v in range(u, 6):
            A[u, v] = A[v, u] = m[k]
            k += 1
    L = np.zeros((6, 6))
    for j in range(6):                                   # the kernel's order of operations
        piv = A[j, j]
        for k in range(j):
            piv -= L[j, k] * L[j, k]
        if not piv > 1e-12 * A[j, j]:
            return None
        L[j, j] = np.sqrt(piv)
        for i in range(j + 1, 6):
            v = A[i, j]
            for k in range(j):
                v -= L[i, k] * L[j, k]
            L[i, j] = v / L[j, j]
    y = np.zeros(6)
    for i in range(6):
        v = -m[21 + i]
        for k in range(i):
            v -= L[i, k] * y[k]
        y[i] = v / L[i, i]
    x = np.zeros(6)
    for i in range(5, -1, -1):
        v = y[i]
        for k in range(i + 1, 6):
            v -= L[k, i] * x[k]
        x[i] = v / L[i, i]
    return x


def rodrigues(w):
    th = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    if not th > 0.0:
        return np.eye(3)
    k = np.asarray(w[:3]) / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def resolve(diag, source_leaf=0.0, max_dist=0.0, min_dist=0.0, eps_rotation=1e-6, eps_translation=0.0, max_iterations=60,
            min_correspondences=100, amax=0.0):
    """The resolved parameters.  amax = the target's largest |coordinate|: the tolerances never fall below what fp32
    coordinates of that size resolve, eps_trans >= 4 ulp(1) amax and eps_rot >= 4 ulp(1) amax / diag (0: no floor)."""
    leaf = source_leaf or 0.005 * diag
    dmax = max_dist or 0.025 * diag
    dmin = min_dist or min(0.0025 * diag, dmax)
    dists = [dmax]
    while dists[-1] > dmin:
        dists.append(max(dmin, dists[-1] / 2))
    floor = 4.0 * 2.0 ** -23 * amax
    return dict(leaf=leaf, dists=dists, eps_rot=max(eps_rotation or 1e-6, floor / diag),
                eps_trans=max(eps_translation or 1e-6 * diag, floor), max_iter=max_iterations or 60,
                min_corr=min_correspondences or 100)


def step(m, T, c):
    """(x, T_next) of one solve + update from the moments m linearised about the fp64 centre c, or (None, T) when degenerate:
    T_next = [R | (c - R c) + x3..5] T with R = Rodrigues(x0..2), in fp64 with the kernel's row order."""
    x = cholesky_solve(m)
    if x is None:
        return None, T
    Rm = rodrigues(x[:3])
    t = [(c[r] - ((Rm[r, 0] * c[0] + Rm[r, 1] * c[1]) + Rm[r, 2] * c[2])) + x[3 + r] for r in range(3)]
    Tn = np.eye(4)
    for r in range(3):
        for k in range(3):
            Tn[r, k] = (Rm[r, 0] * T[0, k] + Rm[r, 1] * T[1, k]) + Rm[r, 2] * T[2, k]
        Tn[r, 3] = ((Rm[r, 0] * T[0, 3] + Rm[r, 1] * T[1, 3]) + Rm[r, 2] * T[2, 3]) + t[r]
    return x, Tn


def refine(tgt, src, T_in, S=None, trace=None, **params):
    """The whole refinement: (T fp64 4 x 4 -- T_in on failure --, info dict with the plade_icp_result fields).  S: the sample
    (default: voxel_downsample of src with the resolved leaf).  trace: a list that receives, after update k, a copy of the info
    a run capped at max_iterations = k returns."""
    target = tgt if isinstance(tgt, Target) else Target(tgt)
    c = resolve(target.diag, amax=target.amax, **params)
    if S is None:
        S = voxel_downsample(np.asarray(src, F32)[:, :3], c["leaf"])
    sbar = sample_mean(S)
    T = np.asarray(T_in, F32).astype(np.float64)
    stage, it = 0, 0
    info = dict(iterations=0, stages=1, converged=False, failure=0, correspondences=0, samples=len(S), rmse=0.0, fitness=0.0,
                final_dist=c["dists"][0])
    while True:
        d = c["dists"][stage]
        _, m, _ = target.linearize(S, T, d, center=apply(T, sbar))
        count = int(m[28])
        info.update(correspondences=count, rmse=float(np.sqrt(m[27] / count)) if count else 0.0,
                    fitness=count / len(S) if len(S) else 0.0, final_dist=d, stages=stage + 1)
        if count < c["min_corr"]:
            info.update(failure=TOO_FEW, iterations=it)
            return np.asarray(T_in, F32).astype(np.float64), info
        x, T = step(m, T, apply(T, sbar))
        if x is None:
            info.update(failure=DEGENERATE, iterations=it)
            return np.asarray(T_in, F32).astype(np.float64), info
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


def perturb(T, rot, trans, seed):
    """[R(axis, rot) | trans * unit] T with a seeded random axis and direction."""
    rng = np.random.default_rng(seed)
    a = rng.normal(size=3)
    v = rng.normal(size=3)
    U = np.eye(4)
    U[:3, :3] = rodrigues(a / np.linalg.norm(a) * rot)
    U[:3, 3] = v / np.linalg.norm(v) * trans
    return U @ np.asarray(T, np.float64)


DIRECTION = np.array([1.0, 0.7, 0.3]) / np.linalg.norm([1.0, 0.7, 0.3])


def frame(offset, rot=0.0, seed=11):
    """A rigid change of frame F (fp64 4 x 4): a rotation by `rot` about a seeded axis, then a translation by `offset` along a
    fixed direction (a scene whose centroid sits near the origin ends about `offset` from it)."""
    F = perturb(np.eye(4), rot, 0.0, seed)
    F[:3, 3] = offset * DIRECTION
    return F


def move(cloud, F, scale=1.0):
    """The cloud (N x 3 or N x 6) in the frame F, its coordinates multiplied by `scale` first: fp32 of the fp64 x y z; the normals
    are rotated (bit for bit the same when F does not rotate; NaN stays NaN)."""
    a = np.asarray(cloud, F32)
    out = a.copy()
    X = a[:, :3].astype(np.float64) * scale
    out[:, :3] = (X @ F[:3, :3].T + F[:3, 3]).astype(F32)
    if a.shape[1] >= 6 and not np.array_equal(F[:3, :3], np.eye(3)):
        out[:, 3:6] = (a[:, 3:6].astype(np.float64) @ F[:3, :3].T).astype(F32)
    return np.ascontiguousarray(out)


def conjugate(T, F, scale=1.0):
    """The source -> target transform T in the frame F of `move(.., F, scale)`: F S T S^-1 F^-1 with S = scale I."""
    T = np.array(T, np.float64)
    T[:3, 3] *= scale
    return F @ T @ np.linalg.inv(F)


def back(T, F, scale=1.0):
    """T of the frame F mapped back to the original frame (the inverse of conjugate)."""
    T = np.linalg.inv(F) @ np.asarray(T, np.float64) @ F
    T[:3, 3] /= scale
    return T
