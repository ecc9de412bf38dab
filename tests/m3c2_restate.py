"""numpy restatement of the M3C2 distances (plade_amd/csrc/m3c2.h).

numpy only, brute force over ALL points of a cloud for every core point.  B is transformed first, row by row in float32:
((r0 x + r1 y) + r2 z) + t.  Everything behind that is float64 from the float32 inputs, with the expressions of m3c2.h term for
term: len2 = (nx nx + ny ny) + nz nz, n^ = n / sqrt(len2) (no axis when len2 is 0 or not finite); q = p - c;
t = (q_x n^_x + q_y n^_y) + q_z n^_z; e = q - t n^; rho2 = (e_x e_x + e_y e_y) + e_z e_z; p is in the cylinder iff
|t| <= L and rho2 < R R.  c = the count, S1 = sum t, S2 = sum t t; mean = S1 / c, var = max(S2 - S1 mean, 0) / (c - 1),
distance = mean_B - mean_A, lod = 1.96 (sqrt(var_A / c_A + var_B / c_B) + reg_error), significant = |distance| > lod, for the
core points with an axis and c_A, c_B >= min_points; NaN / 0 for the others.  Only the order of the sums differs from the kernel.
"""
import numpy as np

F32 = np.float32
F64 = np.float64


def _xyz(points):
    return np.ascontiguousarray(np.asarray(points, F32)[:, :3])


def transform(points, T):
    """B under T in float32, the row rule of section 11 (None: the identity, through the same arithmetic)."""
    X = _xyz(points)
    M = np.eye(4, dtype=F32) if T is None else np.asarray(T, F32).reshape(4, 4)
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    out = np.empty_like(X)
    for r in range(3):
        out[:, r] = ((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3]
    assert out.dtype == F32
    return out


def axes(core):
    """(has_axis (m,) bools, n^ (m, 3) float64: NaN where there is no axis)."""
    n = np.asarray(core, F32)[:, 3:6].astype(F64)
    with np.errstate(all="ignore"):
        len2 = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        has = np.isfinite(len2) & (len2 > 0)
        nh = n / np.sqrt(np.where(has, len2, 1.0))[:, None]
    nh[~has] = np.nan
    return has, nh


def moments(core, cloud, params, pairs=1 << 22):
    """For every (R, L) of params: dict count (m,) uint32, S1, S2 (m,) float64 and A1, A2: the sums of the absolute values of
    the terms.  One brute-force pass over the geometry serves all pairs (R, L).  cloud: already in the core points' frame."""
    C = _xyz(core).astype(F64)
    P = _xyz(cloud).astype(F64)
    has, nh = axes(core)
    m = len(C)
    out = [{"count": np.zeros(m, np.uint32), "S1": np.zeros(m), "S2": np.zeros(m), "A1": np.zeros(m), "A2": np.zeros(m)} for _ in params]
    step = max(1, pairs // max(len(P), 1))
    for c0 in range(0, m, step):
        s = slice(c0, min(m, c0 + step))
        with np.errstate(invalid="ignore"):
            qx = P[None, :, 0] - C[s, None, 0]
            qy = P[None, :, 1] - C[s, None, 1]
            qz = P[None, :, 2] - C[s, None, 2]
            ax, ay, az = nh[s, None, 0], nh[s, None, 1], nh[s, None, 2]
            t = (qx * ax + qy * ay) + qz * az
            ex, ey, ez = qx - t * ax, qy - t * ay, qz - t * az
            rho2 = (ex * ex + ey * ey) + ez * ez
            at = np.abs(t)
            for (R, L), o in zip(params, out):
                inside = (at <= F64(L)) & (rho2 < F64(R) * F64(R))          # (NaN: False)
                tt = np.where(inside, t, 0.0)
                o["count"][s] = inside.sum(1)
                o["S1"][s] = tt.sum(1)
                o["S2"][s] = (tt * tt).sum(1)
                o["A1"][s] = np.abs(tt).sum(1)
                o["A2"][s] = o["S2"][s]
    return out


def derive(has_axis, count_a, S1a, S2a, count_b, S1b, S2b, min_points=4, reg_error=0.0):
    """The derived values from counts and moments with the fp64 expressions of m3c2.h: dict valid, distance, lod, sigma (m, 2),
    significant."""
    ca, cb = np.asarray(count_a).astype(np.int64), np.asarray(count_b).astype(np.int64)
    valid = np.asarray(has_axis, bool) & (ca >= min_points) & (cb >= min_points)
    na, nb = np.where(valid, ca, 2).astype(F64), np.where(valid, cb, 2).astype(F64)
    S1a, S2a, S1b, S2b = (np.asarray(x, F64) for x in (S1a, S2a, S1b, S2b))
    ma, mb = S1a / na, S1b / nb
    va = np.maximum(S2a - S1a * ma, 0.0) / (na - 1.0)
    vb = np.maximum(S2b - S1b * mb, 0.0) / (nb - 1.0)
    dist = mb - ma
    lod = 1.96 * (np.sqrt(va / na + vb / nb) + F64(reg_error))
    sigma = np.stack([np.sqrt(va), np.sqrt(vb)], axis=1)
    sig = valid & (np.abs(dist) > lod)
    dist[~valid] = np.nan
    lod[~valid] = np.nan
    sigma[~valid] = np.nan
    return {"valid": valid, "distance": dist, "lod": lod, "sigma": sigma, "significant": sig}


def m3c2(core, ref, cmp, params, T=None, min_points=4, reg_error=0.0):
    """Everything for every (R, L) of params: a list of the dicts of derive() plus has_axis, count (m, 2), moments (m, 4:
    S1_A S2_A S1_B S2_B) and mag (m, 4: the sums of the absolute values of the terms)."""
    has, _ = axes(core)
    ma = moments(core, ref, params)
    mb = moments(core, transform(cmp, T), params)
    out = []
    for a, b in zip(ma, mb):
        r = derive(has, a["count"], a["S1"], a["S2"], b["count"], b["S1"], b["S2"], min_points, reg_error)
        r.update(has_axis=has, count=np.stack([a["count"], b["count"]], axis=1),
                 moments=np.stack([a["S1"], a["S2"], b["S1"], b["S2"]], axis=1),
                 mag=np.stack([a["A1"], a["A2"], b["A1"], b["A2"]], axis=1))
        out.append(r)
    return out


def summary(distance, significant, count):
    """What plade_m3c2_summary holds, from per-point arrays (a valid core point is one whose distance is not NaN)."""
    d = np.asarray(distance, F64)
    v = ~np.isnan(d)
    dv = d[v]
    k = len(dv)
    return {"m": len(d), "valid": int(k), "significant": int(np.asarray(significant, bool)[v].sum()),
            "mean": float(dv.sum() / k) if k else float("nan"), "rms": float(np.sqrt((dv * dv).sum() / k)) if k else float("nan"),
            "max": float(np.abs(dv).max()) if k else float("nan"), "max_count": int(np.max(count))}
