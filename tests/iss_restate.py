"""numpy restatement of the ISS keypoint detector (plade_amd/csrc/keypoints.h).

numpy only, brute force over ALL pairs of points.  d(i, j) is the float32 expression of flann_d2 (r = ax ax; r += ay ay; r += az az);
j is in N_i iff d < rs2 and in B_i iff d < rn2, the float32 squares of the radii; the point itself belongs to both.  The scatter is
float64 from the float32 inputs, summed term by term in ascending j (the kernel sums in the order of its grid walk: the two differ by
at most the sequential-sum bound c 2^-53 sum |term|, which moment_bound() returns).  The eigenvalues are the closed form of
pca_eig.h's sym3_eigenvalues expression for expression: up to acos everything is + - * / sqrt and so bit-equal to the kernel, given
the same M and c; eigenvalues() takes a dtype so that the same expressions can be evaluated in numpy.longdouble.  The salient test and
the suppression are comparisons: exact functions of their inputs.
"""
import numpy as np

F32 = np.float32
F64 = np.float64
FLAT = 1e-9            # l3 > FLAT * l1
EDGE = 1e-9            # what counts as borderline: a ratio test or a pair of saliencies within this, relative
TWO_PI_3 = 2.0943951023931954923


def radii2(salient_radius, non_max_radius=0.0):
    rs = F32(salient_radius)
    rn = rs if non_max_radius == 0.0 else F32(non_max_radius)
    return F32(rs * rs), F32(rn * rn)


def pairs_within(cloud, r2, rows=512):
    """(i, j): all ordered pairs with d(i, j) < r2, the pairs (i, i) included, ascending in (i, j)."""
    X = np.ascontiguousarray(np.asarray(cloud, F32)[:, :3])
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    I, J = [], []
    for i0 in range(0, len(X), rows):
        i1 = min(len(X), i0 + rows)
        ax = x[i0:i1, None] - x[None, :]
        ay = y[i0:i1, None] - y[None, :]
        az = z[i0:i1, None] - z[None, :]
        d = ax * ax
        d = d + ay * ay
        d = d + az * az
        assert d.dtype == F32
        ii, jj = np.nonzero(d < r2)
        I.append(ii + i0); J.append(jj)
    return np.concatenate(I), np.concatenate(J)


def scatter(cloud, i, j):
    """(M (n, 6) float64: xx xy xz yy yz zz about the query, c (n,) int64, A (n, 6): the sums of |term|)."""
    P = np.asarray(cloud, F32)[:, :3].astype(F64)
    n = len(P)
    q = P[j] - P[i]
    M, A = np.empty((n, 6), F64), np.empty((n, 6), F64)
    for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        t = q[:, a] * q[:, b]
        M[:, k] = np.bincount(i, weights=t, minlength=n)          # (bincount adds in the order of its input: ascending j)
        A[:, k] = np.bincount(i, weights=np.fabs(t), minlength=n)
    return M, np.bincount(i, minlength=n).astype(np.int64), A


def moment_bound(c, A):
    """per entry: the sequential-sum bound c 2^-53 sum |term| of an fp64 sum of c terms"""
    return c[:, None].astype(F64) * 2.0 ** -53 * A


def eigenvalues(M, c, dtype=F64):
    """(n, 3): l1 >= l2 >= l3 of M / c by sym3_eigenvalues' expressions, evaluated in `dtype`."""
    T = dtype
    M = np.asarray(M).astype(T)
    cd = np.asarray(c).astype(T)
    c00, c01, c02, c11, c12, c22 = (M[:, k] / cd for k in range(6))
    three, two, six, half, one = T(3.0), T(2.0), T(6.0), T(0.5), T(1.0)
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
    return np.stack([np.maximum(hi, lmin), np.maximum(lo, np.minimum(hi, lmin)), np.minimum(lo, lmin)], axis=1)


def salient_test(L, c, gamma21=0.975, gamma32=0.975):
    """(salient (n,) bools, saliency (n,) float64) of float64 eigenvalues L (n, 3) and counts c."""
    L = np.asarray(L, F64)
    l1, l2, l3 = L[:, 0], L[:, 1], L[:, 2]
    s = (np.asarray(c) >= 3) & (l1 > 0) & (l2 < gamma21 * l1) & (l3 < gamma32 * l2) & (l3 > FLAT * l1)
    return s, np.where(s, l3, 0.0)


def edge_near(L, c, gamma21=0.975, gamma32=0.975):
    """a ratio test of the point is within EDGE (relative) of its bound"""
    L = np.asarray(L, F64)
    l1, l2, l3 = L[:, 0], L[:, 1], L[:, 2]
    near = lambda a, b: np.fabs(a - b) <= EDGE * np.fabs(b)
    return (np.asarray(c) >= 3) & (l1 > 0) & (near(l2, gamma21 * l1) | near(l3, gamma32 * l2) | near(l3, FLAT * l1))


def suppress(saliency, i, j, n, min_neighbours=5):
    """(keypoint (n,) bools, m (n,) int64) from the saliencies and the pairs (i, j) of the B_i (self pairs included)."""
    s = np.asarray(saliency, F64)
    m = np.bincount(i, minlength=n).astype(np.int64)
    beats = (i != j) & ((s[j] > s[i]) | ((s[j] == s[i]) & (j < i)))
    beaten = np.bincount(i, weights=beats, minlength=n) > 0
    return (s > 0) & (m - 1 >= min_neighbours) & ~beaten, m


def tie_near(saliency, i, j, n):
    """a point with a salient neighbour in B_i whose saliency is within EDGE (relative) of its own"""
    s = np.asarray(saliency, F64)
    close = (i != j) & (s[i] > 0) & (s[j] > 0) & (np.fabs(s[j] - s[i]) <= EDGE * np.maximum(s[i], s[j]))
    return np.bincount(i, weights=close, minlength=n) > 0


def iss(cloud, salient_radius, non_max_radius=0.0, gamma21=0.975, gamma32=0.975, min_neighbours=5):
    """The detector: a dict with scatter, abs_terms, count, eigenvalues, salient, saliency, nms_count, keypoint, index and
    unsure -- the points on which a last-bit difference of the eigenvalues could change the answer: edge_near, tie_near, or a
    B_i that holds an edge_near point."""
    n = len(cloud)
    rs2, rn2 = radii2(salient_radius, non_max_radius)
    i, j = pairs_within(cloud, rs2)
    M, c, A = scatter(cloud, i, j)
    L = eigenvalues(M, c)
    sal, s = salient_test(L, c, gamma21, gamma32)
    bi, bj = (i, j) if rn2 == rs2 else pairs_within(cloud, rn2)
    key, m = suppress(s, bi, bj, n, min_neighbours)
    edge = edge_near(L, c, gamma21, gamma32)
    unsure = edge | tie_near(s, bi, bj, n) | (np.bincount(bi, weights=edge[bj], minlength=n) > 0)
    return dict(scatter=M, abs_terms=A, count=c, eigenvalues=L, salient=sal, saliency=s, nms_count=m, keypoint=key,
                index=np.nonzero(key)[0].astype(np.uint32), unsure=unsure, edge_near=edge, nms_pairs=(bi, bj))


def summary(out):
    return dict(n=len(out["count"]), salient=int(out["salient"].sum()), keypoints=int(out["keypoint"].sum()),
                max_count=int(out["count"].max()))
