"""numpy restatement of the moving-least-squares plane projection (plade_amd/csrc/smooth.h).

numpy only.  d(i, j) = ((dx dx + dy dy) + dz dz) in float32 by brute force over ALL points; N_i = the j with d < float32(r) *
float32(r), the point itself included.  Everything behind the distances is float64: u = d / r2, w = (1 - u)^2, q = p_j - p_i,
W = sum w, S = sum w q, M = sum (w q_a) q_b, each added one term after the other in ascending (d, j) order (np.add.reduceat walks a
segment in order); mu = S / W, C = M / W - mu mu^T; the fit is numpy.linalg.eigh's: n = the eigenvector of the smallest
eigenvalue l0, flipped toward the viewpoint, curvature = max(l0, 0) / trace, delta = n . mu, p' = float32(p + delta n).  A point
with fewer than min_neighbours neighbours or C exactly zero is unfitted: position copied, NaN normal and curvature, delta = 0.
Only the order of the sums and the eigen-solver differ from the kernel.
"""
import numpy as np

from outlier_restate import flann_d2

F32 = np.float32
MOMENTS = ("W", "Sx", "Sy", "Sz", "Mxx", "Mxy", "Mxz", "Myy", "Myz", "Mzz")


def _xyz(points):
    return np.ascontiguousarray(np.asarray(points, F32)[:, :3])


def moments(points, radii, pairs=1 << 25):
    """For every radius: (count (n,) uint32, mom (n, 10) float64 in the order of MOMENTS, mag (n, 10) float64: the sums of the
    absolute values of the terms).  One brute-force pass over the distances serves all radii."""
    X = _xyz(points)
    X64 = X.astype(np.float64)
    n = len(X)
    r2s = [F32(r) * F32(r) for r in radii]
    out = [(np.zeros(n, np.uint32), np.zeros((n, 10)), np.zeros((n, 10))) for _ in radii]
    step = max(1, pairs // max(n, 1))
    for c0 in range(0, n, step):
        qi = np.arange(c0, min(n, c0 + step))
        dd = flann_d2(X[qi], X)
        for r2, (cnt, mom, mag) in zip(r2s, out):
            rr, cc = np.nonzero(dd < r2)
            d = dd[rr, cc]
            order = np.lexsort((cc, d, rr))                        # per query: ascending (d, j)
            rr, cc, d = rr[order], cc[order], d[order]
            per = np.bincount(rr, minlength=len(qi))
            cnt[qi] = per
            has = per > 0
            start = (np.cumsum(per) - per)[has]
            u = d.astype(np.float64) / np.float64(r2)
            w = (1.0 - u) * (1.0 - u)
            q = X64[cc] - X64[qi[rr]]
            wq = w[:, None] * q
            terms = np.stack([w, wq[:, 0], wq[:, 1], wq[:, 2], wq[:, 0] * q[:, 0], wq[:, 0] * q[:, 1], wq[:, 0] * q[:, 2],
                              wq[:, 1] * q[:, 1], wq[:, 1] * q[:, 2], wq[:, 2] * q[:, 2]], axis=1)
            if len(start):
                mom[qi[has]] = np.add.reduceat(terms, start, axis=0)
                mag[qi[has]] = np.add.reduceat(np.abs(terms), start, axis=0)
    return out


def fit(points, count, mom, min_neighbours=6, viewpoint=(0.0, 0.0, 0.0)):
    """The fit and the projection from the moments: dict xyz (n, 3) float32, normal (n, 3) float64 (NaN where unfitted), curvature,
    delta, mu (n, 3), fitted (bools), gap = (l1 - l0) / trace (NaN where unfitted)."""
    X = _xyz(points)
    P = X.astype(np.float64)
    n = len(X)
    W = mom[:, 0]
    ok = count >= np.uint32(min_neighbours)
    Ws = np.where(W > 0, W, 1.0)
    mu = mom[:, 1:4] / Ws[:, None]
    Mm = mom[:, 4:] / Ws[:, None]
    C = np.empty((n, 3, 3))
    for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        C[:, a, b] = C[:, b, a] = Mm[:, k] - mu[:, a] * mu[:, b]
    fitted = ok & (C != 0).any(axis=(1, 2))
    C[~fitted] = np.eye(3)
    lam, vec = np.linalg.eigh(C)
    nrm = vec[:, :, 0].copy()
    v = np.asarray(viewpoint, np.float64)
    flip = ((v[None, :] - P) * nrm).sum(1) < 0
    nrm[flip] = -nrm[flip]
    tr = lam.sum(1)
    curv = np.maximum(lam[:, 0], 0.0) / tr
    gap = (lam[:, 1] - lam[:, 0]) / tr
    delta = (nrm * mu).sum(1)
    delta[~fitted] = 0.0
    nrm[~fitted] = np.nan
    curv[~fitted] = np.nan
    gap[~fitted] = np.nan
    xyz = X.copy()
    xyz[fitted] = (P[fitted] + delta[fitted, None] * nrm[fitted]).astype(F32)
    return {"xyz": xyz, "normal": nrm, "curvature": curv, "delta": delta, "mu": mu, "fitted": fitted, "gap": gap}


def smooth(points, radius, min_neighbours=6, viewpoint=(0.0, 0.0, 0.0)):
    """Everything for one radius: the dict of fit() plus count, moments and mag."""
    count, mom, mag = moments(points, (radius,))[0]
    out = fit(points, count, mom, min_neighbours, viewpoint)
    out.update(count=count, moments=mom, mag=mag)
    return out


def summary(delta, fitted, count):
    """What plade_smooth_summary holds, from per-point arrays."""
    d = np.asarray(delta, np.float64)[np.asarray(fitted, bool)]
    return {"n": len(delta), "fitted": int(len(d)), "rms": float(np.sqrt((d * d).sum() / len(d))) if len(d) else 0.0,
            "max": float(np.abs(d).max()) if len(d) else 0.0, "max_count": int(np.max(count))}
