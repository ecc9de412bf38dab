"""Cases, exact reference and contract for pca_eig (plade_amd/csrc/pca_eig.h), the 3 x 3 eigen-solve behind every normal.

numpy only.  A table is a cloud of blocks: block b is k points centre_b + L_b * H with int64 local coordinates |L| <= 2^15,
H = 2^-20 and centres on a lattice of spacing 2 inside |c| < 8, so every coordinate is exact in fp32, a block is at most 0.11
across and its k points are the k nearest neighbours of each of them.  The far table is the same geometry times 2^7 about
2^10 (1, -1, 1): H = 2^-13, still exact in fp32.  k = 3, 16 and 64, and k = 33 for covariances that are isotropic up to rounding
(33 does not divide exactly: lattice_blocks()).

The reference is the covariance of a block as exact integers, (k sum L_a L_b - S_a S_b) / k^2, decomposed by a cyclic Jacobi
iteration in numpy.longdouble (LD_OK: 64-bit significands; the tests skip otherwise).

The contract (errors(), check()), with s = the trace, g = l1 - l0, v0 / v2 the eigenvectors of the smallest / largest eigenvalue:

    n finite, | |n| - 1 | <= 1e-6
    angle(n, v0)   <= 2^-23 + M 2^-52 s / g            where g > 0         (angle = asin |n x v0|)
    |n . v2|       <= 2^-23 + M 2^-52 s / (l2 - l1)    where l2 > l1
    |curv - l0/s|  <= 2^-23 (l0 / s) + M 2^-52

2^-23 is twice the worst rounding of three fp32 components, sqrt(3) 2^-25.  e = (error - floor) * gap / s / 2^-52, at least 0, is
O(1) for a backward-stable solver: the share of M that a result uses.  (floor = the 2^-23 term for the fp32 outputs of the library,
0 for an fp64 result.)  M is 8 times the worst e of the suite's older reference pipeline (the covariance about the query in fp64,
then numpy.linalg.eigh: pca_ref of test_gpu_normals.py) on these same tables against the long-double reference, never against the
code under test: E_EIGH below, asserted in test_eig_cases_host.py.  The factor 8 covers another summation order, the weighted
moments of the smoothing and another libm.

restate_pca_eig() is pca_eig operation for operation in fp64 (the build uses -ffp-contract=off: up to libm's acos / cos the same
roundings), restate_pca_store() / restate_smooth_fit() what k_normals.hip / k_smooth.hip do around it.
"""
import functools
import math

import numpy as np

F32 = np.float32
F64 = np.float64
LD = np.longdouble
LD_OK = bool(np.finfo(LD).eps < 2e-19)

H = 2.0 ** -20
LMAX = 1 << 15
FAR_SCALE = 2.0 ** 7
FAR_BASE = 2.0 ** 10 * np.array([1.0, -1.0, 1.0])
RADIUS = 0.25                    # the smoothing radius that covers a block and nothing else (times FAR_SCALE on the far table)
FLOOR = 2.0 ** -23
EPS = 2.0 ** -52
# the worst e of pca_ref (fp64 covariance about the query, numpy.linalg.eigh) over every point of MARGIN_TABLES, measured against the
# long-double reference: angle 0.64 (k64 needle), long axis 1.03 (k16 (1, 1.001e-3, 1e-3)), curvature 1.19 (k3 triple).  1.19 is
# rounded up to 1.25, which leaves 5 % for another LAPACK build; M = 8 E_EIGH = 10
E_EIGH = 1.25
M = 8.0 * E_EIGH

SPECTRA = ((1.0, 0.3, 1e-4), (1.0, 1.0, 1e-6), (1.0, 1e-3, 1e-8), (1.0, 2e-3, 1e-3), (1.0, 1.01e-3, 1e-3), (1.0, 1.001e-3, 1e-3),
           (1.0, 1e-7, 1e-8), (1.0, 3e-9, 1e-9), (1.3, 1.1, 1.0), (1.001, 1.0005, 1.0))
SPECTRA_64 = (SPECTRA[0], SPECTRA[2], SPECTRA[5], SPECTRA[7])
A3, B3, C3 = np.array([2, 1, 2]), np.array([-2, 2, 1]), np.array([1, 2, -2])     # mutually orthogonal, each of length 3


class Block:
    def __init__(self, kind, L, axis=None, normal=None):
        self.kind = kind
        self.L = np.asarray(L, np.int64)
        self.axis = axis             # the known long axis (not normalised), or None
        self.normal = normal         # the known normal, or None
        assert self.L.ndim == 2 and self.L.shape[1] == 3 and np.abs(self.L).max() <= LMAX


def spectrum_name(sp):
    return "(%g, %g, %g)" % sp


def generic_block(rng, k, spectrum):
    """k normal draws whitened to unit covariance, scaled by the sqrt of the spectrum, rotated, scaled to max|L| = 2^15, rounded"""
    X = rng.standard_normal((k, 3))
    X -= X.mean(0)
    X = X @ np.linalg.inv(np.linalg.cholesky(X.T @ X / k)).T
    X *= np.sqrt(np.asarray(spectrum, F64))
    Q, R = np.linalg.qr(rng.standard_normal((3, 3)))
    X = X @ (Q * np.sign(np.diag(R))).T
    return Block(spectrum_name(spectrum), np.rint(X * (LMAX / np.abs(X).max())).astype(np.int64))


def exact_blocks():
    ij = [(i, j) for i in range(4) for j in range(4)]
    sc = 1 << 11                                                       # |L| <= 9 * 2^11
    corners = [(sb, sc_) for sb in (-1, 1) for sc_ in (-1, 1)]
    cube = np.array([(x, y, z) for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)])
    return [
        Block("exact plane", sc * np.array([i * A3 + j * B3 for i, j in ij]), normal=C3),
        Block("exact plane, unequal steps", (sc // 4) * np.array([i * A3 + 3 * j * B3 for i, j in ij]), normal=C3),
        Block("exact line", sc * np.array([i * A3 for i in range(16)]) // 2, axis=A3),
        Block("exact prolate", sc * np.array([i * A3 + s * B3 + t * C3 for i in range(4) for s, t in corners]), axis=A3),
        Block("exact isotropic", sc * np.concatenate([cube, cube])),
        Block("coincident", np.zeros((16, 3), np.int64)),
    ]


def triple_blocks(seed=3):
    """k = 3: rank <= 2 always; random, nearly collinear (the third point a few lattice steps off the chord) and collinear"""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(10):
        out.append(Block("triple", rng.integers(-LMAX, LMAX + 1, (3, 3))))
    for t in range(10):
        p = rng.integers(-LMAX // 2, LMAX // 2 + 1, (2, 3))
        mid = (p[0] + p[1]) // 2 + rng.integers(-3, 4, 3) * (1 + 40 * (t % 3))
        out.append(Block("triple, nearly collinear", np.stack([p[0], p[1], mid])))
    for t in range(4):
        d = rng.integers(-2000, 2001, 3)
        out.append(Block("triple, collinear", np.stack([-7 * d, 2 * d, (5 + t) * d]), axis=d))
    return out


def lattice_blocks(steps=(1 << 11, 1 << 13, 3000, 2731, 1500, 777)):
    """k = 33: a lattice point, its 26 neighbours in the 3 x 3 x 3 cube and the 6 at two steps along the axes.  C = 26/33 step^2 I
    exactly, which no fp64 number holds: trace / 3 misses the diagonal by an ulp, and the mean about a query other than the centre
    is rounded, so the solver sees a matrix that is isotropic up to rounding, with r anywhere in [-1, 1]."""
    cube = [(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1)]
    arms = [tuple(2 * sg * (a == t) for a in range(3)) for t in range(3) for sg in (-1, 1)]
    return [Block("exact isotropic", st * np.array(cube + arms)) for st in steps]


class Table:
    """blocks -> the cloud P (n, 3) float32 in a seeded shuffled order, block_of (n,), members: block -> the indices of its points"""
    def __init__(self, name, k, blocks, far=False, seed=0):
        self.name, self.k, self.blocks, self.far = name, k, blocks, far
        assert all(len(b.L) == k for b in blocks)
        lattice = np.array([(x, y, z) for x in range(-6, 7, 2) for y in range(-6, 7, 2) for z in range(-6, 7, 2)], F64)
        rng = np.random.default_rng(seed)
        centres = lattice[rng.permutation(len(lattice))[:len(blocks)]]
        assert len(centres) == len(blocks)
        X = np.concatenate([c + b.L.astype(F64) * H for c, b in zip(centres, blocks)])      # exact in fp64
        self.scale = FAR_SCALE if far else 1.0
        if far:
            X = FAR_BASE + FAR_SCALE * X
        block_of = np.repeat(np.arange(len(blocks)), k)
        perm = rng.permutation(len(X))
        self.X64 = X[perm]
        self.P = np.ascontiguousarray(self.X64.astype(F32))
        assert np.array_equal(self.P.astype(F64), self.X64), "a coordinate is not exact in fp32"
        self.block_of = block_of[perm]
        self.members = [np.nonzero(self.block_of == b)[0] for b in range(len(blocks))]
        self.kinds = [b.kind for b in blocks]
        self.radius = RADIUS * self.scale

    @functools.cached_property
    def ref(self):
        """(lam (B, 3) ascending, V (B, 3, 3) columns v0 v1 v2, zero (B,)) in long double, in units of the lattice step"""
        C, zero = zip(*(exact_covariance(b.L) for b in self.blocks))
        lam, V = jacobi(np.stack(C))
        return lam, V, np.array(zero)


def generic_blocks(k, spectra, repeats, seed):
    rng = np.random.default_rng(seed)
    return [generic_block(rng, k, sp) for sp in spectra for _ in range(repeats)]


@functools.lru_cache(maxsize=None)
def table(name):
    if name == "k16":
        return Table(name, 16, generic_blocks(16, SPECTRA, 6, 16) + exact_blocks(), seed=1)
    if name == "k16_far":
        return Table(name, 16, generic_blocks(16, SPECTRA, 6, 16) + exact_blocks(), far=True, seed=2)
    if name == "k3":
        return Table(name, 3, triple_blocks(), seed=3)
    if name == "k64":
        return Table(name, 64, generic_blocks(64, SPECTRA_64, 3, 64), seed=4)
    if name == "k33":
        return Table(name, 33, generic_blocks(33, SPECTRA_64, 2, 33) + lattice_blocks(), seed=5)
    raise KeyError(name)


TABLES = ("k16", "k16_far", "k3", "k64", "k33")
MARGIN_TABLES = TABLES[:4]       # E_EIGH is measured on these; k33 is held to the same M (on it eigh itself needs 1.58)


def neighbour_sets(P, k):
    """(n, k): each point's k nearest by flann_d2 in fp32, ties by index (knn_ref of test_gpu_normals.py), each row sorted"""
    from outlier_restate import flann_d2
    X = np.ascontiguousarray(np.asarray(P, F32)[:, :3])
    d = flann_d2(X, X)
    assert d.dtype == F32
    order = np.lexsort((np.broadcast_to(np.arange(len(X)), d.shape), d), axis=1)
    return np.sort(order[:, :k], axis=1)


# ---- the reference ------------------------------------------------------------------------------------------------------------
def exact_covariance(L):
    """((3, 3) long double = k^2 C in lattice units from exact Python integers, C is exactly zero)"""
    k = len(L)
    rows = [[int(v) for v in p] for p in L]
    S = [sum(p[a] for p in rows) for a in range(3)]
    C = np.empty((3, 3), LD)
    for a in range(3):
        for b in range(3):
            num = k * sum(p[a] * p[b] for p in rows) - S[a] * S[b]
            assert abs(num) < 1 << 53                                   # exact as a double, so as a long double
            C[a, b] = LD(float(num))
    return C / LD(k * k), not C.any()


def jacobi(A, sweeps=12):
    """Cyclic Jacobi on a batch (B, 3, 3) of symmetric long-double matrices: (lam (B, 3) ascending, V (B, 3, 3), A V = V lam)."""
    A = np.array(A, LD)
    n = len(A)
    V = np.tile(np.eye(3, dtype=LD), (n, 1, 1))
    one = LD(1)
    for _ in range(sweeps):
        if not (A[:, 0, 1].any() or A[:, 0, 2].any() or A[:, 1, 2].any()):
            break
        for p, q in ((0, 1), (0, 2), (1, 2)):
            apq = A[:, p, q]
            live = apq != 0
            with np.errstate(all="ignore"):
                theta = (A[:, q, q] - A[:, p, p]) / (LD(2) * np.where(live, apq, one))
                t = np.where(theta >= 0, one, -one) / (np.fabs(theta) + np.sqrt(theta * theta + one))
            t = np.where(live & np.isfinite(t), t, LD(0))
            c = one / np.sqrt(t * t + one)
            s = t * c
            J = np.tile(np.eye(3, dtype=LD), (n, 1, 1))
            J[:, p, p] = c; J[:, q, q] = c; J[:, p, q] = s; J[:, q, p] = -s
            A = np.matmul(np.matmul(J.transpose(0, 2, 1), A), J)
            A[:, p, q] = A[:, q, p] = 0
            V = np.matmul(V, J)
    lam = np.stack([A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]], 1)
    order = np.argsort(lam, axis=1, kind="stable")
    return np.take_along_axis(lam, order, 1), np.take_along_axis(V, order[:, None, :], 2)


# ---- the contract -------------------------------------------------------------------------------------------------------------
def errors(n, curv, lam, V, margin=M, floor=FLOOR):
    """n (m, 3), curv (m,), lam (m, 3), V (m, 3, 3) -> a dict of float64 arrays: the errors, their bounds and e (angle, axis: the
    component along v2, curv); an absent gap gives error 0, bound inf."""
    n = np.asarray(n, F64).astype(LD)
    lam, V = np.asarray(lam, LD), np.asarray(V, LD)
    s = lam.sum(1)
    g, G = lam[:, 1] - lam[:, 0], lam[:, 2] - lam[:, 1]
    norm = np.sqrt((n * n).sum(1))
    with np.errstate(all="ignore"):
        u = n / norm[:, None]
        sin = np.sqrt((np.cross(u, V[:, :, 0]) ** 2).sum(1))
        ang = np.where(g > 0, np.arcsin(np.minimum(sin, LD(1))), LD(0))
        ang_bound = np.where(g > 0, floor + margin * EPS * s / np.where(g > 0, g, LD(1)), np.inf)
        axis = np.where(G > 0, np.fabs((u * V[:, :, 2]).sum(1)), LD(0))
        axis_bound = np.where(G > 0, floor + margin * EPS * s / np.where(G > 0, G, LD(1)), np.inf)
        c0 = lam[:, 0] / s
        cerr = np.fabs(np.asarray(curv, F64).astype(LD) - c0)
        cbound = floor * np.fabs(c0) + margin * EPS
    f = lambda x: np.asarray(x, F64)
    over = lambda x, fl: np.maximum(x - fl, LD(0))
    return dict(finite=np.isfinite(f(n)).all(1), unit=f(np.fabs(norm - 1)), angle=f(ang), angle_bound=f(ang_bound), axis=f(axis),
                axis_bound=f(axis_bound), curv=f(cerr), curv_bound=f(cbound), e_angle=f(over(ang, floor) * g / s / EPS),
                e_axis=f(over(axis, floor) * G / s / EPS), e_curv=f(over(cerr, floor * np.fabs(c0)) / EPS))


def worst_by_kind(err, kinds):
    """{kind: (worst e_angle, e_axis, e_curv)} over the rows of each kind (kinds: one name per row)"""
    kinds = np.asarray(kinds)
    return {k: tuple(float(np.nanmax(err[e][kinds == k])) for e in ("e_angle", "e_axis", "e_curv")) for k in dict.fromkeys(kinds)}


def report(err, kinds):
    return "\n".join("%-32s e_angle %.3g  e_axis %.3g  e_curv %.3g" % ((k,) + v) for k, v in worst_by_kind(err, kinds).items())


def check(n, curv, lam, V, kinds, margin=M):
    """The contract on rows whose covariance is not exactly zero; the failure message carries the worst e per block kind."""
    err = errors(n, curv, lam, V, margin)
    bad = []
    if not err["finite"].all():
        bad.append("%d normals are not finite" % int((~err["finite"]).sum()))
    else:
        for what, ok in (("| |n| - 1 | <= 1e-6", err["unit"] <= 1e-6), ("angle(n, v0)", err["angle"] <= err["angle_bound"]),
                         ("|n . v2|", err["axis"] <= err["axis_bound"]), ("curvature", err["curv"] <= err["curv_bound"])):
            if not ok.all():
                bad.append("%s fails on %d of %d rows, kinds %s" % (what, int((~ok).sum()), len(ok), sorted(set(np.asarray(kinds)[~ok]))))
    assert not bad, "\n".join(bad) + "\n" + report(err, kinds)
    return err


# ---- the restatement ----------------------------------------------------------------------------------------------------------
TWO_PI_3 = 2.0943951023931954923


def _cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def _dot(u, v):
    return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]


def _largest_cross(r0, r1, r2):
    x01, x02, x12 = _cross(r0, r1), _cross(r0, r2), _cross(r1, r2)
    n01, n02, n12 = _dot(x01, x01), _dot(x02, x02), _dot(x12, x12)
    v, vn = x01, n01
    if n02 > vn:
        v, vn = x02, n02
    if n12 > vn:
        v, vn = x12, n12
    return v, vn


def _across(rr):
    """cross(rr, the unit vector along the axis of rr's smallest component)"""
    ax, ay, az = abs(rr[0]), abs(rr[1]), abs(rr[2])
    e = (1.0, 0.0, 0.0) if ax <= ay and ax <= az else (0.0, 1.0, 0.0) if ay <= az else (0.0, 0.0, 1.0)
    return _cross(rr, e)


def restate_pca_eig(c00, c01, c02, c11, c12, c22):
    """pca_eig in Python floats (IEEE fp64), expression for expression: None when C is exactly zero, else (n, l0, tr)."""
    c00, c01, c02, c11, c12, c22 = (float(x) for x in (c00, c01, c02, c11, c12, c22))
    if c00 == 0.0 and c01 == 0.0 and c02 == 0.0 and c11 == 0.0 and c12 == 0.0 and c22 == 0.0:
        return None
    tr = c00 + c11 + c22
    q = tr / 3.0
    b00, b11, b22 = c00 - q, c11 - q, c22 - q
    p2 = b00 * b00 + b11 * b11 + b22 * b22 + 2.0 * (c01 * c01 + c02 * c02 + c12 * c12)
    l0 = q
    if p2 > 0.0:
        pp = math.sqrt(p2 / 6.0)
        i00, i11, i22, i01, i02, i12 = b00 / pp, b11 / pp, b22 / pp, c01 / pp, c02 / pp, c12 / pp
        r = 0.5 * (i00 * (i11 * i22 - i12 * i12) - i01 * (i01 * i22 - i12 * i02) + i02 * (i01 * i12 - i11 * i02))
        r = min(1.0, max(-1.0, r))
        phi = math.acos(r) / 3.0
        root = q + 2.0 * pp * math.cos(phi if r > 0.0 else phi + TWO_PI_3)
        if r > 0.0:
            # the largest root first, its eigenvector, then the 2 x 2 problem across it
            lmax = root
            v, vn = _largest_cross((c00 - lmax, c01, c02), (c01, c11 - lmax, c12), (c02, c12, c22 - lmax))
            if vn > 0.0:
                s = 1.0 / math.sqrt(vn)
                v2 = (v[0] * s, v[1] * s, v[2] * s)
                u = _across(v2)
                s = 1.0 / math.sqrt(_dot(u, u))
                u = (u[0] * s, u[1] * s, u[2] * s)
                w = _cross(v2, u)
                cu = (c00 * u[0] + c01 * u[1] + c02 * u[2], c01 * u[0] + c11 * u[1] + c12 * u[2], c02 * u[0] + c12 * u[1] + c22 * u[2])
                cw = (c00 * w[0] + c01 * w[1] + c02 * w[2], c01 * w[0] + c11 * w[1] + c12 * w[2], c02 * w[0] + c12 * w[1] + c22 * w[2])
                m00, m01, m11 = _dot(u, cu), _dot(u, cw), _dot(w, cw)
                d = 0.5 * (m00 - m11)
                h = math.sqrt(d * d + m01 * m01)
                x, y = -m01, d + h
                x2, y2 = h - d, -m01
                if x2 * x2 + y2 * y2 > x * x + y * y:
                    x, y = x2, y2
                if not (x * x + y * y > 0.0):
                    x, y = 1.0, 0.0
                nv = (x * u[0] + y * w[0], x * u[1] + y * w[1], x * u[2] + y * w[2])
                s = 1.0 / math.sqrt(_dot(nv, nv))
                return (nv[0] * s, nv[1] * s, nv[2] * s), 0.5 * (m00 + m11) - h, tr
            # C - lmax I vanishes to rounding: C is isotropic to an ulp; l0 = q, a direction from below
        else:
            l0 = root
    r0, r1, r2 = (c00 - l0, c01, c02), (c01, c11 - l0, c12), (c02, c12, c22 - l0)
    v, vn = _largest_cross(r0, r1, r2)
    q0, q1, q2 = _dot(r0, r0), _dot(r1, r1), _dot(r2, r2)
    rr, rmax = r0, q0
    if q1 > rmax:
        rr, rmax = r1, q1
    if q2 > rmax:
        rr, rmax = r2, q2
    if not (vn > 1e-20 * rmax * rmax):
        v = _across(rr) if rmax > 0.0 else (0.0, 0.0, 1.0)
        vn = _dot(v, v)
    s = 1.0 / math.sqrt(vn)
    return (v[0] * s, v[1] * s, v[2] * s), l0, tr


def _outputs(res, dtype):
    if res is None:
        return np.full(3, np.nan, dtype), dtype(np.nan)
    nv, l0, tr = res
    return np.asarray(nv, F64).astype(dtype), dtype(max(l0, 0.0) / tr)


def restate_pca_store(P, i, nbr, dtype=F32):
    """pca_store of k_normals.hip for point i and its neighbour list: (n (3,) up to sign, curvature), rounded to float32 as the
    kernel stores them, or with dtype = float64 as it holds them before"""
    X = np.asarray(P, F32)[:, :3].astype(F64)
    m = len(nbr)
    px, py, pz = (float(v) for v in X[i])
    rows = [tuple(float(v) for v in X[j]) for j in nbr]
    sx = sy = sz = 0.0
    for r in rows:
        sx += r[0] - px; sy += r[1] - py; sz += r[2] - pz
    mx, my, mz = sx / m, sy / m, sz / m
    c00 = c01 = c02 = c11 = c12 = c22 = 0.0
    for r in rows:
        ex, ey, ez = (r[0] - px) - mx, (r[1] - py) - my, (r[2] - pz) - mz
        c00 += ex * ex; c01 += ex * ey; c02 += ex * ez
        c11 += ey * ey; c12 += ey * ez; c22 += ez * ez
    return _outputs(restate_pca_eig(c00 / m, c01 / m, c02 / m, c11 / m, c12 / m, c22 / m), dtype)


def restate_smooth_fit(mom, dtype=F32):
    """the fit of k_smooth.hip from one row of moments (W, S, M): (n (3,) up to sign, curvature, delta float64)"""
    W, sx, sy, sz, m00, m01, m02, m11, m12, m22 = (float(v) for v in mom)
    mx, my, mz = sx / W, sy / W, sz / W
    res = restate_pca_eig(m00 / W - mx * mx, m01 / W - mx * my, m02 / W - mx * mz, m11 / W - my * my, m12 / W - my * mz, m22 / W - mz * mz)
    n, curv = _outputs(res, dtype)
    return n, curv, 0.0 if res is None else _dot(res[0], (mx, my, mz))


def moment_reference(mom):
    """(lam, V, mu) in long double from rows of moments: C = M / W - mu mu^T, then Jacobi"""
    mom = np.asarray(mom, F64).astype(LD)
    W = mom[:, 0]
    mu = mom[:, 1:4] / W[:, None]
    C = np.empty((len(mom), 3, 3), LD)
    for t, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        C[:, a, b] = C[:, b, a] = mom[:, 4 + t] / W - mu[:, a] * mu[:, b]
    lam, V = jacobi(C)
    return lam, V, mu
