"""The semantics of the pose estimator over correspondences (plade_amd/csrc/corr_pose.h), restated in numpy.

Everything up to the least-squares refit is fp64 with + - * / sqrt only, every dot product (a_x b_x + a_y b_y) + a_z b_z, every
cross product (a_y b_z - a_z b_y, a_z b_x - a_x b_z, a_x b_y - a_y b_x): numpy evaluates the same operations in the same order,
so triples, statuses, hypothesis transforms, counts and flags are the library's bit for bit.  The refit here is numpy's SVD (Kabsch)
on plain numpy sums -- another algorithm than the library's Horn quaternion in a fixed summation order -- and agrees with it to
rounding; horn() restates the library's solver itself (same operations, same order) for the host tests."""
import numpy as np

_U = np.uint64
SWEEPS = 12


def mix64(z):
    """splitmix64's finaliser on a python int"""
    m = (1 << 64) - 1
    z = (z + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def _mix64_np(z):
    with np.errstate(over="ignore"):
        z = z + _U(0x9E3779B97F4A7C15)
        z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
        return z ^ (z >> _U(31))


def draws(seed, H, M):
    """(H, 3) int64: the triple of every hypothesis"""
    base = _U(mix64(int(seed)))
    h = np.arange(H, dtype=np.uint64)
    out = np.empty((H, 3), np.int64)
    for k in range(3):
        z = _mix64_np(base ^ (_U(4) * h + _U(k)))
        out[:, k] = (((z >> _U(32)) * _U(M)) >> _U(32)).astype(np.int64)
    return out


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _frame(pa, pb, pc):
    u, v = pb - pa, pc - pa
    e1 = u / np.sqrt(dot(u, u))[..., None]
    w = cross(u, v)
    wl = np.sqrt(dot(w, w))
    e3 = w / wl[..., None]
    e2 = cross(e3, e1)
    return e1, e2, e3, (wl > 0.0) & np.isfinite(wl)


def _edge_fails(si, sj, qi, qj, sim):
    ds, dq = si - sj, qi - qj
    ls, lt = np.sqrt(dot(ds, ds)), np.sqrt(dot(dq, dq))
    return np.fmin(ls, lt) < sim * np.fmax(ls, lt)


def packed(src, tgt, corr):
    """S, Q (M, 3) float64 of a correspondence list into two point arrays (their first three columns)"""
    corr = np.asarray(corr)
    return (np.asarray(src)[corr[:, 0], :3].astype(np.float64), np.asarray(tgt)[corr[:, 1], :3].astype(np.float64))


def hypotheses(S, Q, seed=0, H=65536, sim=0.9, triples=None):
    """triple (H, 3), status (H,) uint8 and T (H, 3, 4) float64 (zeros unless status 0) of every hypothesis"""
    tri = draws(seed, H, len(S)) if triples is None else np.asarray(triples, np.int64)
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    with np.errstate(all="ignore"):
        same = (a == b) | (b == c) | (a == c)
        rej = _edge_fails(S[a], S[b], Q[a], Q[b], sim) | _edge_fails(S[b], S[c], Q[b], Q[c], sim) | _edge_fails(S[c], S[a], Q[c], Q[a], sim)
        s1, s2, s3, oks = _frame(S[a], S[b], S[c])
        t1, t2, t3, okt = _frame(Q[a], Q[b], Q[c])
        R = (t1[:, :, None] * s1[:, None, :] + t2[:, :, None] * s2[:, None, :]) + t3[:, :, None] * s3[:, None, :]
        cs = ((S[a] + S[b]) + S[c]) / 3.0
        ct = ((Q[a] + Q[b]) + Q[c]) / 3.0
        t = ct - ((R[:, :, 0] * cs[:, None, 0] + R[:, :, 1] * cs[:, None, 1]) + R[:, :, 2] * cs[:, None, 2])
    status = np.where(same, 1, np.where(rej, 2, np.where(~(oks & okt), 3, 0))).astype(np.uint8)
    T = np.concatenate([R, t[:, :, None]], axis=2)
    T[status != 0] = 0.0
    return tri, status, T


def d2_under(T, S, Q):
    """T (..., 3, 4), S, Q (M, 3) -> d2 (..., M)"""
    T = np.asarray(T, np.float64)[..., :3, :4]
    x = ((T[..., None, :, 0] * S[:, None, 0] + T[..., None, :, 1] * S[:, None, 1]) + T[..., None, :, 2] * S[:, None, 2]) + T[..., None, :, 3]
    d = x - Q
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def flags_under(T, S, Q, dist):
    return d2_under(T, S, Q) < dist * dist


def counts(T, status, S, Q, dist, block=256):
    """count (H,) uint32: 0 unless status 0"""
    out = np.zeros(len(status), np.uint32)
    idx = np.flatnonzero(status == 0)
    for i in range(0, len(idx), block):
        j = idx[i:i + block]
        out[j] = flags_under(T[j], S, Q, dist).sum(axis=1)
    return out


def best_of(count, status):
    """(h, count) of the scored hypothesis with the largest count, ties to the smallest h; None when nothing is scored"""
    idx = np.flatnonzero(status == 0)
    if len(idx) == 0:
        return None
    k = idx[np.argmax(count[idx])]
    return int(k), int(count[k])


def moment_terms(S, Q, T, dist):
    """flags and the per-correspondence terms of the refinement's sums: ones (M,), S, Q (M, 3), d2 (M,) -- zero where not flagged"""
    d2 = d2_under(T, S, Q)
    f = d2 < dist * dist
    z = np.where(f, 1.0, 0.0)
    return f, z, np.where(f[:, None], S, 0.0), np.where(f[:, None], Q, 0.0), np.where(f, d2, 0.0)


def moments_replayed(S, Q, T, dist):
    """flags and the 17 moments of plade_corr_pose_moments in the library's summation order (tests/fixed_order.py)"""
    import fixed_order
    f, one, s, q, d2 = moment_terms(S, Q, T, dist)
    red = lambda v: fixed_order.reduce(v, np.add)
    n = red(one)
    with np.errstate(all="ignore"):
        sm = np.array([red(s[:, k]) for k in range(3)]) / n
        qm = np.array([red(q[:, k]) for k in range(3)]) / n
    C = np.zeros(9)
    if f.any():
        ds, dq = S - sm, Q - qm
        for a in range(3):
            for b in range(3):
                C[3 * a + b] = red(np.where(f, dq[:, a] * ds[:, b], 0.0))
    return f, np.concatenate([[n], sm, qm, C, [red(d2)]])


def kabsch(C):
    """the rotation R (det +1) that maximises trace(R^T C), C = sum (Q - q)(S - s)^T: numpy's SVD"""
    U, _, Vt = np.linalg.svd(C)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    return U @ D @ Vt


def horn(C):
    """the library's solver: Horn's quaternion by SWEEPS cyclic Jacobi sweeps, operation for operation"""
    C = np.asarray(C, np.float64).reshape(3, 3)
    Sxx, Sxy, Sxz = C[0, 0], C[1, 0], C[2, 0]
    Syx, Syy, Syz = C[0, 1], C[1, 1], C[2, 1]
    Szx, Szy, Szz = C[0, 2], C[1, 2], C[2, 2]
    A = np.array([[(Sxx + Syy) + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
                  [Syz - Szy, (Sxx - Syy) - Szz, Sxy + Syx, Szx + Sxz],
                  [Szx - Sxz, Sxy + Syx, (Syy - Sxx) - Szz, Syz + Szy],
                  [Sxy - Syx, Szx + Sxz, Syz + Szy, (Szz - Sxx) - Syy]])
    V = np.eye(4)
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS):
            for p, q in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
                apq = A[p, q]
                if apq == 0.0:
                    continue
                theta = (A[q, q] - A[p, p]) / (2.0 * apq)
                t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                for M in (A, V):
                    x, y = M[:, p].copy(), M[:, q].copy()
                    M[:, p], M[:, q] = c * x - s * y, s * x + c * y
                    if M is A:
                        x, y = A[p, :].copy(), A[q, :].copy()
                        A[p, :], A[q, :] = c * x - s * y, s * x + c * y
    col = 0
    for k in (1, 2, 3):
        if A[k, k] > A[col, col]:
            col = k
    q0, q1, q2, q3 = V[:, col]
    l = np.sqrt((q0 * q0 + q1 * q1) + (q2 * q2 + q3 * q3))
    w, x, y, z = q0 / l, q1 / l, q2 / l, q3 / l
    return np.array([[((w * w + x * x) - y * y) - z * z, 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                     [2.0 * (x * y + w * z), ((w * w - x * x) + y * y) - z * z, 2.0 * (y * z - w * x)],
                     [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), ((w * w - x * x) - y * y) + z * z]])


def refit(S, Q, f, solver=kabsch):
    """the least-squares T (3, 4) over the flagged correspondences, and the singular values of their cross-covariance"""
    sm, qm = S[f].mean(axis=0), Q[f].mean(axis=0)
    C = (Q[f] - qm).T @ (S[f] - sm)
    R = solver(C)
    return np.concatenate([R, (qm - R @ sm)[:, None]], axis=1), np.linalg.svd(C, compute_uv=False)


def estimate(S, Q, dist, seed=0, H=65536, sim=0.9, min_inliers=3, refine_iterations=5, solver=kabsch):
    """The whole estimator.  Returns a dict: ok, failure (0 .. 3), T (3, 4) float64, flags, best (h, count), refinements, margin (the
    smallest |d2 - dist^2| / dist^2 met in any flag evaluation of the loop) and sv_ratio (the largest singular-value ratio s0 / s2 of
    a cross-covariance the loop refitted -- inf for a planar set)."""
    out = dict(ok=False, failure=0, T=np.eye(4)[:3], flags=np.zeros(len(S), bool), best=None, refinements=0, margin=np.inf,
               sv_ratio=0.0)
    if len(S) < 3:
        out["failure"] = 1
        return out
    tri, status, Th = hypotheses(S, Q, seed, H, sim)
    cnt = counts(Th, status, S, Q, dist)
    out.update(triple=tri, status=status, Th=Th, count=cnt)
    b = best_of(cnt, status)
    if b is None:
        out["failure"] = 2
        return out
    out["best"] = b
    if b[1] < min_inliers:
        out["failure"] = 3
        return out
    thr2 = dist * dist

    def flags(T):
        d2 = d2_under(T, S, Q)
        out["margin"] = min(out["margin"], float(np.abs(d2 - thr2).min() / thr2))
        return d2 < thr2

    T = Th[b[0]]
    f = flags(T)
    for _ in range(refine_iterations):
        Tn, sv = refit(S, Q, f, solver)
        out["sv_ratio"] = max(out["sv_ratio"], float(sv[0] / sv[2]) if sv[2] > 0 else np.inf)
        if not np.isfinite(Tn).all():
            break
        fn = flags(Tn)
        if fn.sum() < f.sum():
            break
        same = np.array_equal(fn, f)
        T, f = Tn, fn
        out["refinements"] += 1
        if same:
            break
    d2 = d2_under(T, S, Q)
    out.update(ok=True, T=T, flags=f, inliers=int(f.sum()), rmse=float(np.sqrt(d2[f].sum() / f.sum())), fitness=f.sum() / len(S))
    return out


def pose_error(T, T_gt):
    """(rotation error in degrees, translation error) of a 3 x 4 / 4 x 4 T against the ground truth"""
    T, T_gt = np.asarray(T, np.float64), np.asarray(T_gt, np.float64)
    R = T[:3, :3] @ T_gt[:3, :3].T
    ang = np.degrees(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)))
    return float(ang), float(np.linalg.norm(T[:3, 3] - T_gt[:3, 3]))
