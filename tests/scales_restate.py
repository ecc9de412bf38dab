"""numpy restatement of the multi-scale normals and dimensionality features (plade_amd/csrc/scales.h).

numpy only, brute force over ALL pairs of points.  d(i, j) is the float32 expression of flann_d2 (r = ax ax; r += ay ay; r += az az);
j is in N(i, s) iff d < r2_s, the float32 square of the radius; the point itself belongs to every scale.  The moments are float64
from the float32 inputs, q = p_j - p_i, the nine sums of q and q_a q_b added term by term in ascending j (the kernel adds in the order
of its grid walk: the two differ by at most the sequential-sum bound, which the sums of |term| give).  mu = S / c and C = M / c - mu
mu^T follow k_scales_fit's expressions; the eigenvalues are pca_eig.h's sym3_eigenvalues expression for expression, clamped at 0,
and take a dtype so that the same expressions can be evaluated in numpy.longdouble.  Features, the fitted test and the choice are
divisions and comparisons: exact functions of their inputs.  The normals are numpy.linalg.eigh's; only the order of the sums and the
eigenvector solver differ from the kernel.
"""
import numpy as np

F32 = np.float32
F64 = np.float64
TWO_PI_3 = 2.0943951023931954923
TIE = 1e-9             # two criterion values of one query closer than this (absolute: both criteria lie in [0, 1]) make it unsure
FLAT = 1e-9            # l2 <= FLAT * l1: a degenerate C (the neighbours are collinear to rounding)
UPPER = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def radii2(radii):
    """the float32 squares (float)r * (float)r"""
    r = np.asarray(radii, F64).astype(F32)
    return (r * r).astype(F32)


def pairs_within(cloud, r2, queries=None, rows=512, window=True):
    """(t, j, d): all pairs of a query slot t and a point j with d = d(query t, j) < r2, ascending in (t, j); queries: the indices
    of the queried points (None: all).  Brute force; with `window` a block of queries (taken in the order of their x) meets only
    the points whose x lies within 1.001 sqrt(r2) + 1e-6 max|x| of the block's -- every other point has ax ax >= r2 in fp32 already,
    and d only grows from there -- which changes no pair (tests/test_scales_host.py compares the two)."""
    X = np.ascontiguousarray(np.asarray(cloud, F32)[:, :3])
    qi = np.arange(len(X)) if queries is None else np.asarray(queries, np.int64)
    order = np.argsort(X[:, 0], kind="stable")
    xs = X[order, 0].astype(F64)
    qorder = np.argsort(X[qi, 0], kind="stable")
    reach = 1.001 * float(np.sqrt(F64(r2))) + 1e-6 * float(np.abs(xs).max() if len(xs) else 0.0)
    T, J, D = [], [], []
    for i0 in range(0, len(qi), rows):
        slots = qorder[i0:i0 + rows]
        Q = X[qi[slots]]
        if window:
            lo = np.searchsorted(xs, float(Q[:, 0].min()) - reach, side="left")
            hi = np.searchsorted(xs, float(Q[:, 0].max()) + reach, side="right")
            cols = order[lo:hi]
        else:
            cols = np.arange(len(X))
        ax = Q[:, 0, None] - X[cols, 0][None, :]
        ay = Q[:, 1, None] - X[cols, 1][None, :]
        az = Q[:, 2, None] - X[cols, 2][None, :]
        d = ax * ax
        d = d + ay * ay
        d = d + az * az
        assert d.dtype == F32
        tt, jj = np.nonzero(d < r2)
        T.append(slots[tt]); J.append(cols[jj]); D.append(d[tt, jj])
    t, j, d = np.concatenate(T), np.concatenate(J), np.concatenate(D)
    o = np.lexsort((j, t))
    return t[o], j[o], d[o]


def moments(cloud, radii, queries=None):
    """(count (k, S) int64, mom (k, S, 9) float64: Sx Sy Sz Mxx Mxy Mxz Myy Myz Mzz, mag (k, S, 9): the sums of |term|)."""
    X = np.ascontiguousarray(np.asarray(cloud, F32)[:, :3])
    P = X.astype(F64)
    qi = np.arange(len(X)) if queries is None else np.asarray(queries, np.int64)
    k, r2 = len(qi), radii2(radii)
    t, j, d = pairs_within(X, r2.max(), None if queries is None else qi)
    q = P[j] - P[qi[t]]
    terms = np.stack([q[:, 0], q[:, 1], q[:, 2]] + [q[:, a] * q[:, b] for a, b in UPPER], axis=1)
    count = np.zeros((k, len(r2)), np.int64)
    mom, mag = np.zeros((k, len(r2), 9)), np.zeros((k, len(r2), 9))
    for s, r2s in enumerate(r2):
        own = d < r2s                                                  # each scale's own test
        ts, te = t[own], terms[own]
        count[:, s] = np.bincount(ts, minlength=k)
        for e in range(9):                                             # (bincount adds in the order of its input: ascending j)
            mom[:, s, e] = np.bincount(ts, weights=te[:, e], minlength=k)
            mag[:, s, e] = np.bincount(ts, weights=np.fabs(te[:, e]), minlength=k)
    return count, mom, mag


def covariance(mom, count, dtype=F64):
    """(..., 6): C = M / c - mu mu^T (xx xy xz yy yz zz) in k_scales_fit's expression order, evaluated in `dtype`."""
    m = np.asarray(mom).astype(dtype)
    W = np.asarray(count).astype(dtype)[..., None]
    mu = m[..., :3] / W
    Mm = m[..., 3:] / W
    return np.stack([Mm[..., e] - mu[..., a] * mu[..., b] for e, (a, b) in enumerate(UPPER)], axis=-1)


def sym3(C, dtype=F64):
    """(..., 3): l1 >= l2 >= l3 of the six entries C by sym3_eigenvalues' expressions in `dtype`, each clamped at 0."""
    T = dtype
    C = np.asarray(C).astype(T)
    c00, c01, c02, c11, c12, c22 = (C[..., e] for e in range(6))
    three, two, six, half, one, zero = T(3.0), T(2.0), T(6.0), T(0.5), T(1.0), T(0.0)
    tr = c00 + c11 + c22
    q = tr / three
    b00, b11, b22 = c00 - q, c11 - q, c22 - q
    p2 = b00 * b00 + b11 * b11 + b22 * b22 + two * (c01 * c01 + c02 * c02 + c12 * c12)
    pos = p2 > 0
    with np.errstate(all="ignore"):
        pp = np.sqrt(np.where(pos, p2, one) / six)
        i00, i11, i22, i01, i02, i12 = b00 / pp, b11 / pp, b22 / pp, c01 / pp, c02 / pp, c12 / pp
        r = half * (i00 * (i11 * i22 - i12 * i12) - i01 * (i01 * i22 - i12 * i02) + i02 * (i01 * i12 - i11 * i02))
        r = np.minimum(one, np.maximum(-one, r))
        phi = np.arccos(r) / three
        lmax = np.where(pos, q + two * pp * np.cos(phi), q)
        lmin = np.where(pos, q + two * pp * np.cos(phi + T(TWO_PI_3)), q)
        lmid = np.where(pos, tr - lmax - lmin, q)
    hi, lo = np.maximum(lmax, lmid), np.minimum(lmax, lmid)
    L = np.stack([np.maximum(hi, lmin), np.maximum(lo, np.minimum(hi, lmin)), np.minimum(lo, lmin)], axis=-1)
    return np.maximum(L, zero)


def eigenvalues(mom, count, dtype=F64):
    return sym3(covariance(mom, count, dtype), dtype)


def features(L):
    """(..., 4) float64: linearity, planarity, sphericity, variation of float64 eigenvalues (NaN / inf where l1 = 0)."""
    L = np.asarray(L, F64)
    l1, l2, l3 = L[..., 0], L[..., 1], L[..., 2]
    with np.errstate(all="ignore"):
        return np.stack([(l1 - l2) / l1, (l2 - l3) / l1, l3 / l1, l3 / ((l1 + l2) + l3)], axis=-1)


def fitted_test(count, C, L, min_neighbours=6):
    """c >= min_neighbours, C not exactly zero (pca_eig's refusal), l1 > 0"""
    return (np.asarray(count) >= min_neighbours) & (np.asarray(C) != 0).any(axis=-1) & (np.asarray(L)[..., 0] > 0)


def criterion(F, mode):
    """the value the choice compares, larger is better: planarity (mode 0) or minus the variation (mode 1)"""
    return F[..., 1] if mode == 0 else -F[..., 3]


def choose(crit, fitted):
    """(k,) int32: over the fitted scales in ascending s, a later one replaces the current one only when strictly better; -1: none."""
    crit, fitted = np.asarray(crit, F64), np.asarray(fitted, bool)
    k, S = fitted.shape
    chosen, best = np.full(k, -1, np.int32), np.zeros(k)
    for s in range(S):
        take = fitted[:, s] & ((chosen < 0) | (crit[:, s] > best))
        chosen[take] = s
        best[take] = crit[take, s]
    return chosen


def pick(per_scale, chosen):
    """the chosen scale's row of a (k, S, m) array as float32, NaN where chosen = -1"""
    per_scale = np.asarray(per_scale)
    out = np.full((len(chosen), per_scale.shape[2]), np.nan, F32)
    has = chosen >= 0
    out[has] = per_scale[np.nonzero(has)[0], chosen[has]].astype(F32)
    return out


def flips(P, N, viewpoint=(0.0, 0.0, 0.0), row_normals=None):
    """(k, S) bools: which of the normals N (k, S, 3) the orientation rule turns round.  P: the queries' positions (k, 3)."""
    P, N = np.asarray(P, F32).astype(F64), np.asarray(N, F64)
    v = np.asarray(viewpoint, F32).astype(F64)
    w = v[None, :] - P
    with np.errstate(all="ignore"):
        flip = w[:, None, 0] * N[..., 0] + w[:, None, 1] * N[..., 1] + w[:, None, 2] * N[..., 2] < 0
        if row_normals is not None:
            g = np.asarray(row_normals, F32).astype(F64)
            t = (g[:, None, 0] * N[..., 0] + g[:, None, 1] * N[..., 1]) + g[:, None, 2] * N[..., 2]
            flip = np.where(t < 0, True, np.where(t > 0, False, flip))
    return flip


def eigh_normals(C):
    """(normals (..., 3) float64: numpy's eigenvector of the smallest eigenvalue, gap (...): (l2 - l3) / trace by eigh)"""
    C = np.asarray(C, F64)
    A = np.empty(C.shape[:-1] + (3, 3))
    for e, (a, b) in enumerate(UPPER):
        A[..., a, b] = A[..., b, a] = C[..., e]
    lam, vec = np.linalg.eigh(A)
    with np.errstate(all="ignore"):
        gap = (lam[..., 1] - lam[..., 0]) / lam.sum(-1)
    return vec[..., :, 0], gap


def unsure(crit, fitted, count, L, min_neighbours=6):
    """(k,) bools: the queries on which last-bit differences of the sums could change the choice -- two fitted scales whose
    criterion values lie within TIE of each other, or a scale with exactly min_neighbours neighbours and a degenerate C."""
    crit, fitted, L = np.asarray(crit, F64), np.asarray(fitted, bool), np.asarray(L, F64)
    k, S = fitted.shape
    out = ((np.asarray(count) == min_neighbours) & (L[..., 1] <= FLAT * L[..., 0])).any(axis=1)
    for a in range(S):
        for b in range(a + 1, S):
            out |= fitted[:, a] & fitted[:, b] & (np.fabs(crit[:, a] - crit[:, b]) <= TIE)
    return out


def scales(cloud, radii, mode=0, min_neighbours=6, viewpoint=(0.0, 0.0, 0.0), orient=0, queries=None):
    """Everything: a dict with count, moments, mag, cov, eigenvalues, fitted, features (per scale), criterion, chosen, unsure,
    normals (k, S, 3 float64 by eigh, oriented, NaN where unfitted), gap, normal and chosen_features (float32, NaN where -1)."""
    A = np.asarray(cloud, F32)
    qi = np.arange(len(A)) if queries is None else np.asarray(queries, np.int64)
    count, mom, mag = moments(A, radii, queries)
    C = covariance(mom, count)
    L = sym3(C)
    fit = fitted_test(count, C, L, min_neighbours)
    F = features(L)
    crit = criterion(F, mode)
    chosen = choose(crit, fit)
    N, gap = eigh_normals(np.where(fit[..., None], C, np.array([1.0, 0.0, 0.0, 2.0, 0.0, 3.0])))
    flip = flips(A[qi, :3], N, viewpoint, A[qi, 3:6] if orient else None)
    N = np.where(flip[..., None], -N, N)
    N[~fit] = np.nan
    return dict(count=count, moments=mom, mag=mag, cov=C, eigenvalues=L, fitted=fit, features=F, criterion=crit, chosen=chosen,
                unsure=unsure(crit, fit, count, L, min_neighbours), normals=N, gap=np.where(fit, gap, np.nan),
                normal=pick(N, chosen), chosen_features=pick(F, chosen))


def summary(chosen, count, scales_asked):
    """What plade_scale_summary holds, from per-query arrays."""
    chosen = np.asarray(chosen)
    return dict(queries=len(chosen), fitted=int((chosen >= 0).sum()),
                chosen_hist=tuple(int((chosen == s).sum()) for s in range(scales_asked)), max_count=int(np.max(count)))
