"""numpy restatement of the FPFH descriptors and of their feature-space match (plade_amd/csrc/fpfh.h).

numpy only, brute force over ALL pairs of points.  d(i, j) is the float32 expression of flann_d2 (r = ax ax; r += ay ay; r += az az);
j is a neighbour of i iff 0 < d < r2, r2 = float32(r) * float32(r).  Everything behind that is float64 from the float32 inputs with
the expressions of fpfh.h term for term, every dot product (a_x b_x + a_y b_y) + a_z b_z, every cross product
(a_y b_z - a_z b_y, a_z b_x - a_x b_z, a_x b_y - a_y b_x); no np.sum / einsum / linalg.norm where the order matters.  Between the
kernel and this file only atan2 and the order of the weighted sums differ.  The match is float32 throughout and is reproduced bit for
bit.
"""
import numpy as np

F32 = np.float32
F64 = np.float64
BINS, DIM = 11, 33
EDGE = 1e-9


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def axes(cloud):
    """(has_axis (n,) bools, n^ as three (n,) float64 arrays: NaN where there is no axis)."""
    n = np.asarray(cloud, F32)[:, 3:6].astype(F64)
    with np.errstate(all="ignore"):
        len2 = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        has = np.isfinite(len2) & (len2 > 0)
        s = np.sqrt(np.where(has, len2, 1.0))
        nh = [np.where(has, n[:, k] / s, np.nan) for k in range(3)]
    return has, nh


def neighbour_pairs(cloud, radius, rows=512):
    """(i, j, d): all ordered pairs with 0 < d(i, j) < r2, ascending in (i, j); d float32."""
    X = np.ascontiguousarray(np.asarray(cloud, F32)[:, :3])
    r = F32(radius)
    r2 = F32(r * r)
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    I, J, D = [], [], []
    for i0 in range(0, len(X), rows):
        i1 = min(len(X), i0 + rows)
        ax = x[i0:i1, None] - x[None, :]
        ay = y[i0:i1, None] - y[None, :]
        az = z[i0:i1, None] - z[None, :]
        d = ax * ax
        d = d + ay * ay
        d = d + az * az
        assert d.dtype == F32
        ii, jj = np.nonzero((d > 0) & (d < r2))
        I.append(ii + i0); J.append(jj); D.append(d[ii, jj])
    return np.concatenate(I), np.concatenate(J), np.concatenate(D), r2


def _bin(x):
    with np.errstate(invalid="ignore"):
        t = np.floor(11.0 * x)
        return np.where(t >= 0, np.minimum(t, 10.0), 0.0).astype(np.int64)


def pair_features(cloud, i, j):
    """The features of the pairs (i, j) (arrays): counted (bools), b1, b2, b3 (ints), near (bools: 11 (...) of f1, f2 or f3 is
    within EDGE of an integer)."""
    P = np.asarray(cloud, F32)[:, :3].astype(F64)
    has, nh = axes(cloud)
    ni = [nh[k][i] for k in range(3)]
    nj = [nh[k][j] for k in range(3)]
    q = [P[j, k] - P[i, k] for k in range(3)]
    with np.errstate(all="ignore"):
        l = np.sqrt(dot(q, q))
        e = [q[k] / l for k in range(3)]
        ai, aj = dot(ni, e), dot(nj, e)
        swap = np.fabs(ai) < np.fabs(aj)
        n1 = [np.where(swap, nj[k], ni[k]) for k in range(3)]
        n2 = [np.where(swap, ni[k], nj[k]) for k in range(3)]
        dp = [np.where(swap, -e[k], e[k]) for k in range(3)]
        f3 = dot(n1, dp)
        v = cross(dp, n1)
        vl = np.sqrt(dot(v, v))
        counted = has[i] & has[j] & (vl != 0)
        v = [v[k] / vl for k in range(3)]
        w = cross(n1, v)
        f2 = dot(v, n2)
        f1 = np.arctan2(dot(w, n2), dot(n1, n2))
        x1, x2, x3 = 11.0 * ((f1 + np.pi) / (2.0 * np.pi)), 11.0 * ((f2 + 1.0) * 0.5), 11.0 * ((f3 + 1.0) * 0.5)
        near = np.zeros(len(i), bool)
        for x in (x1, x2, x3):
            near |= np.fabs(x - np.rint(x)) < EDGE
    b1, b2, b3 = _bin((f1 + np.pi) / (2.0 * np.pi)), _bin((f2 + 1.0) * 0.5), _bin((f3 + 1.0) * 0.5)
    return counted, b1, b2, b3, near & counted


def fpfh(cloud, radius, min_pairs=5):
    """A dict: spfh (n, 33 uint32), pairs (n uint32), described (n bools), raw (n, 34 float64: W, R; zeros where not described),
    desc (n, 33 float32; NaN rows where not described), edge_near (n bools: some counted pair of the point has 11 (...) of f1, f2
    or f3 within EDGE of an integer), edge_reach (n bools: the point or one of its neighbours is edge_near, so its weighted sums
    may see another histogram), has_axis, counted_pairs (their total)."""
    cloud = np.asarray(cloud, F32)
    n = len(cloud)
    i, j, d, r2 = neighbour_pairs(cloud, radius)
    counted, b1, b2, b3, near = pair_features(cloud, i, j)
    H = np.zeros((n, DIM), np.int64)
    ic = i[counted]
    np.add.at(H, (ic, b1[counted]), 1)
    np.add.at(H, (ic, BINS + b2[counted]), 1)
    np.add.at(H, (ic, 2 * BINS + b3[counted]), 1)
    c = np.bincount(ic, minlength=n)
    has, _ = axes(cloud)
    described = has & (c >= int(min_pairs))
    edge_near = np.bincount(i[near], minlength=n) > 0
    edge_reach = edge_near | (np.bincount(i[edge_near[j]], minlength=n) > 0)
    # the weighting: the described j in N_i of a described i
    use = described[i] & described[j]
    iu, ju = i[use], j[use]
    w = F64(r2) / d[use].astype(F64)
    hn = np.zeros((n, DIM), F64)
    hn[described] = H[described].astype(F64) / c[described].astype(F64)[:, None]
    raw = np.zeros((n, DIM + 1), F64)
    raw[:, 0] = np.bincount(iu, weights=w, minlength=n)
    for b in range(DIM):
        raw[:, 1 + b] = np.bincount(iu, weights=w * hn[ju, b], minlength=n)
    desc = descriptor(H, c, described, raw)
    return {"spfh": H.astype(np.uint32), "pairs": c.astype(np.uint32), "described": described, "raw": raw, "desc": desc,
            "edge_near": edge_near, "edge_reach": edge_reach, "has_axis": has, "counted_pairs": int(counted.sum())}


def descriptor(spfh, pairs, described, raw):
    """F of fpfh.h from H, c, the described flags and (W, R): float32; NaN rows where not described."""
    H, c = np.asarray(spfh).astype(F64), np.asarray(pairs).astype(F64)
    W, R = raw[:, 0], raw[:, 1:]
    out = np.full(H.shape, np.nan, F32)
    with np.errstate(all="ignore"):
        a = 50.0 * (H / c[:, None] + R / W[:, None])
        b = (100.0 * H) / c[:, None]
    F = np.where((W > 0)[:, None], a, b).astype(F32)
    m = np.asarray(described, bool)
    out[m] = F[m]
    return out


def summary(pairs, described):
    m = np.asarray(described, bool)
    c = np.asarray(pairs).astype(np.int64)
    return {"n": len(c), "described": int(m.sum()), "max_pairs": int(c.max()),
            "mean_pairs": float(c[m].sum()) / float(m.sum()) if m.any() else 0.0}


# ---- the match -------------------------------------------------------------------------------------------------------------------
def delta(S, T):
    """(ns, nt) float32: sum over b = 0 .. 32, in that order, of (S_b - T_b) * (S_b - T_b)."""
    S, T = np.asarray(S, F32), np.ascontiguousarray(np.asarray(T, F32).T)
    d = np.zeros((len(S), T.shape[1]), F32)
    x = np.empty_like(d)
    with np.errstate(all="ignore"):
        for b in range(DIM):
            np.subtract(S[:, b, None], T[b][None, :], out=x)
            np.multiply(x, x, out=x)
            np.add(d, x, out=d)
    return d


def nearest2(S, T, rows=128):
    """nn (ns int32, -1: none), d2 (ns, 2 float32, NaN: none): the two smallest (delta, t) over the valid targets, for the valid
    sources; a target whose delta is NaN is passed over."""
    S, T = np.asarray(S, F32), np.asarray(T, F32)
    ns = len(S)
    nn = np.full(ns, -1, np.int32)
    d2 = np.full((ns, 2), np.nan, F32)
    tv = ~np.isnan(T[:, 0])
    for s0 in range(0, ns, rows):
        s1 = min(ns, s0 + rows)
        d = delta(S[s0:s1], T)
        ok = tv[None, :] & ~np.isnan(d) & ~np.isnan(S[s0:s1, 0])[:, None]
        key = np.where(ok, d.view(np.uint32).astype(np.uint64) << np.uint64(32), np.uint64(2 ** 64 - 1))
        key = np.where(ok, key | np.arange(len(T), dtype=np.uint64)[None, :], key)
        rows_ = np.arange(s1 - s0)
        for k in range(2):                                   # the keys are distinct: two minima in turn
            t = np.argmin(key, axis=1)
            good = key[rows_, t] != np.uint64(2 ** 64 - 1)
            if k == 0:
                nn[s0:s1] = np.where(good, t, -1)
            d2[s0:s1, k] = np.where(good, d[rows_, t], np.nan)
            key[rows_, t] = np.uint64(2 ** 64 - 1)
    return nn, d2


def keep(nn, d2, back, mutual=True, max_ratio=0.0):
    """corr ((m, 2) int32 ascending in s) from the two searches."""
    k = nn >= 0
    if mutual:
        k &= back[np.maximum(nn, 0)] == np.arange(len(nn))
    if max_ratio:
        r = F32(max_ratio)
        r2 = F32(r * r)
        with np.errstate(invalid="ignore"):
            k &= np.isnan(d2[:, 1]) | (d2[:, 0] < r2 * d2[:, 1])
    s = np.nonzero(k)[0]
    return np.stack([s, nn[s]], axis=1).astype(np.int32)


def match(S, T, mutual=True, max_ratio=0.0):
    """A dict: nn, d2, back (nt int32), corr."""
    nn, d2 = nearest2(S, T)
    back, _ = nearest2(T, S)
    return {"nn": nn, "d2": d2, "back": back, "corr": keep(nn, d2, back, mutual, max_ratio)}
