"""numpy restatement of the cloud-to-cloud distances (plade_amd/csrc/distances.h).

numpy only.  p' = fp32(R) s + fp32(t) row by row as ((r0 x + r1 y) + r2 z) + t; j = the argmin over all target points of
(flann_d2(p', q_j), j) in float32; a correspondence when flann_d2 < (float)d * (float)d.  The argmin is taken by chunked brute
force over the target points inside the chunk's bounding box grown by a little more than d: nothing outside it can be closer than
d, so idx and d2 are the exact set.  The plane residual and the summary use the fp64 expressions of the kernels; only the
summation order of the summary differs.
"""
import numpy as np

F32 = np.float32
INF = np.float32(np.inf)


def transform_f32(T, xyz):
    """p' of the match step: fp32(R), fp32(t), ((r0 x + r1 y) + r2 z) + t in float32 (T None: the identity)."""
    Tf = np.eye(4, dtype=F32) if T is None else np.asarray(T).astype(F32).reshape(4, 4)
    x, y, z = (np.ascontiguousarray(np.asarray(xyz, F32)[:, k]) for k in range(3))
    return np.stack([((Tf[r, 0] * x + Tf[r, 1] * y) + Tf[r, 2] * z) + Tf[r, 3] for r in range(3)], axis=1)


def flann_d2(Q, C):
    """(len(Q), len(C)) float32 matrix of ((dx dx + dy dy) + dz dz)."""
    ax = Q[:, 0:1] - C[None, :, 0]
    ay = Q[:, 1:2] - C[None, :, 1]
    az = Q[:, 2:3] - C[None, :, 2]
    dd = ax * ax
    dd += ay * ay
    dd += az * az
    return dd


def nearest(tgt_xyz, P, d, chunk=512, pairs=1 << 23):
    """(idx int32, d2 float32) of the float32 probes P against the target points within d: -1 / +inf without a correspondence."""
    X = np.ascontiguousarray(np.asarray(tgt_xyz, F32)[:, :3])
    P = np.asarray(P, F32)
    n = len(P)
    d2 = F32(d) * F32(d)
    idx = np.full(n, -1, np.int32)
    dist = np.full(n, INF, F32)
    if n == 0 or len(X) == 0:
        return idx, dist
    order_t = np.argsort(X[:, 0], kind="stable")
    xs = X[order_t, 0]
    mn, mx = X.min(0).astype(np.float64), X.max(0).astype(np.float64)
    amax = float(max(np.abs(mn).max(), np.abs(mx).max(), np.abs(P).max()))
    c = max(float(d), float(np.linalg.norm(mx - mn)) / 32.0)
    lo = P.min(0)
    cell = np.floor((P - lo) / c).astype(np.int64)
    qorder = np.lexsort((cell[:, 0], cell[:, 1], cell[:, 2]))
    r = 1.01 * float(d) + 1e-5 * amax
    for c0 in range(0, n, chunk):
        qi = qorder[c0:c0 + chunk]
        Q = P[qi]
        qlo, qhi = Q.min(0).astype(np.float64) - r, Q.max(0).astype(np.float64) + r
        a, b = np.searchsorted(xs, qlo[0], "left"), np.searchsorted(xs, qhi[0], "right")
        cand = order_t[a:b]
        cy, cz = X[cand, 1], X[cand, 2]
        cand = np.sort(cand[(cy >= qlo[1]) & (cy <= qhi[1]) & (cz >= qlo[2]) & (cz <= qhi[2])])
        best_d = np.full(len(qi), INF, F32)
        best_j = np.full(len(qi), -1, np.int64)
        step = max(1, pairs // len(qi))
        for k0 in range(0, len(cand), step):            # ascending candidate blocks: a tie keeps the earlier (smaller) index
            cb = cand[k0:k0 + step]
            dd = flann_d2(Q, X[cb])
            k = np.argmin(dd, axis=1)                    # first of equal minima: the smaller index
            dm = dd[np.arange(len(qi)), k]
            better = dm < best_d
            best_d[better] = dm[better]
            best_j[better] = cb[k[better]]
        ok = best_d < d2
        idx[qi[ok]] = best_j[ok].astype(np.int32)
        dist[qi[ok]] = best_d[ok]
    return idx, dist


def plane_residual(tgt, src_xyz, T, idx):
    """fp64 r_i = (n0 (p0 - q0) + n1 (p1 - q1)) + n2 (p2 - q2), p = double(T) double(s_i); NaN without a correspondence or with
    a non-finite normal."""
    T = np.eye(4) if T is None else np.asarray(T).astype(F32).astype(np.float64).reshape(4, 4)
    S = np.asarray(src_xyz, F32)[:, :3].astype(np.float64)
    t = np.asarray(tgt, F32)
    r = np.full(len(S), np.nan)
    sel = idx >= 0
    j = idx[sel]
    q = t[j, :3].astype(np.float64)
    nn = t[j, 3:6].astype(np.float64)
    X = S[sel]
    p = [((T[k, 0] * X[:, 0] + T[k, 1] * X[:, 1]) + T[k, 2] * X[:, 2]) + T[k, 3] for k in range(3)]
    with np.errstate(invalid="ignore"):
        rr = (nn[:, 0] * (p[0] - q[:, 0]) + nn[:, 1] * (p[1] - q[:, 1])) + nn[:, 2] * (p[2] - q[:, 2])
    rr[~np.isfinite(nn).all(1)] = np.nan
    r[sel] = rr
    return r


def summary(idx, d2, r):
    """The plade_distance_summary fields of the per-point results (r: the fp64 plane residuals)."""
    n = len(idx)
    sel = idx >= 0
    count = int(sel.sum())
    dd = d2[sel].astype(np.float64)
    fin = np.isfinite(r)
    pc = int(fin.sum())
    nan = float("nan")
    return {"n": n, "count": count, "plane_count": pc, "fitness": count / n,
            "rmse": float(np.sqrt(dd.sum() / count)) if count else nan,
            "mean": float(np.sqrt(dd).sum() / count) if count else nan,
            "max": float(np.sqrt(dd).max()) if count else nan,
            "plane_rmse": float(np.sqrt((r[fin] ** 2).sum() / pc)) if pc else nan}


def cloud_distances(tgt, src_xyz, d, T=None):
    """(idx, d2, plane float32, summary) of distances.h."""
    P = transform_f32(T, src_xyz)
    idx, d2 = nearest(np.asarray(tgt, F32)[:, :3], P, d)
    r = plane_residual(tgt, src_xyz, T, idx)
    return idx, d2, r.astype(F32), summary(idx, d2, r)


def diag(tgt):
    t = np.asarray(tgt, np.float64)[:, :3]
    return float(np.linalg.norm(t.max(0) - t.min(0)))


def rot_z(a):
    c, s = np.cos(a), np.sin(a)
    R = np.eye(4)
    R[:2, :2] = [[c, -s], [s, c]]
    return R


def rot_x(a):
    c, s = np.cos(a), np.sin(a)
    R = np.eye(4)
    R[1:3, 1:3] = [[c, -s], [s, c]]
    return R
