"""numpy restatement of the cloud merge (plade_amd/csrc/merge.h).

numpy only.  Every expression is the one the semantics state: the fp32 transform row by row, the fp32 voxel of p', the fp64 sums
taken one point after the other in ascending (cloud, index) order (np.add.at applies its updates in the order of the index array;
reduceat and sum do not promise that order), the fp64 division and square root, the rounding to fp32.  The GPU tests compare
with this bit for bit.
"""
import numpy as np

F32 = np.float32
EINVAL, ELIMIT = -1, -5
MAX_CLOUDS = 16


class MergeError(ValueError):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


def transform_rows(T, rows):
    """(p', n') of the rows x y z nx ny nz under the row-major 4 x 4 T (None: the identity, same arithmetic), in float32."""
    Tf = np.eye(4, dtype=F32) if T is None else np.asarray(T, F32).reshape(4, 4)
    r = np.asarray(rows, F32)
    x, y, z, nx, ny, nz = (np.ascontiguousarray(r[:, k]) for k in range(6))
    out = np.empty((len(r), 6), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(3):
            out[:, k] = ((Tf[k, 0] * x + Tf[k, 1] * y) + Tf[k, 2] * z) + Tf[k, 3]
            out[:, 3 + k] = (Tf[k, 0] * nx + Tf[k, 1] * ny) + Tf[k, 2] * nz
    return out


def voxel_ijk(p, leaf):
    """Voxel coordinates of the float32 points p: floor(p * inv) - floor(min * inv) with inv = 1.f / leaf, all in float32."""
    inv = F32(1.0) / F32(leaf)
    lo = np.floor(p.min(0) * inv).astype(np.int64)
    ijk = np.floor(p * inv).astype(np.int64) - lo
    if (ijk.max(0) >= (1 << 18)).any():
        raise MergeError(ELIMIT, "more than 2^18 leaves along one axis")
    return ijk


def merge(clouds, transforms=None, leaf=0.0):
    """Returns (rows (M, 6) float32, count (M,) uint32, mask (M,) uint32, summary dict)."""
    k = len(clouds)
    if not 1 <= k <= MAX_CLOUDS:
        raise MergeError(EINVAL, "1 to 16 clouds")
    leaf = F32(leaf)
    if not np.isfinite(leaf) or leaf < 0:
        raise MergeError(EINVAL, "leaf must be finite and >= 0")
    if transforms is None:
        transforms = [None] * k
    parts, cloud_of = [], []
    for c, (rows, T) in enumerate(zip(clouds, transforms)):
        if rows is None:
            raise MergeError(EINVAL, "NULL cloud")
        rows = np.asarray(rows, F32)
        if len(rows) == 0:
            raise MergeError(EINVAL, "an empty cloud")
        if not np.isfinite(rows[:, :3]).all() or (T is not None and not np.isfinite(np.asarray(T, F32)).all()):
            raise MergeError(EINVAL, "non-finite coordinate or transform")
        parts.append(transform_rows(T, rows))
        cloud_of.append(np.full(len(rows), c, np.int64))
    cat, cloud_of = np.concatenate(parts), np.concatenate(cloud_of)
    n_in = len(cat)
    if n_in >= 1 << 31:
        raise MergeError(ELIMIT, "2^31 points or more")
    if not np.isfinite(cat[:, :3]).all():
        raise MergeError(EINVAL, "non-finite transformed coordinate")
    bit = (np.uint32(1) << cloud_of.astype(np.uint32)).astype(np.uint32)
    if leaf == 0:
        summary = {"n_in": n_in, "n_out": n_in, "n_shared": 0, "max_count": 1}
        return cat, np.ones(n_in, np.uint32), bit, summary
    ijk = voxel_ijk(cat[:, :3], leaf)
    key = ijk[:, 0] + (ijk[:, 1] << 18) + (ijk[:, 2] << 36)            # ascending (k, j, i)
    order = np.argsort(key, kind="stable")                              # ascending (cloud, index) inside a voxel
    ks = key[order]
    head = np.r_[True, ks[1:] != ks[:-1]]
    seg = np.cumsum(head) - 1
    m = int(seg[-1]) + 1
    s = cat[order]
    count = np.zeros(m, np.int64)
    np.add.at(count, seg, 1)
    psum = np.zeros((m, 3), np.float64)
    np.add.at(psum, seg, s[:, :3].astype(np.float64))                   # sequential: one point after the other
    fin = np.isfinite(s[:, 3:6]).all(1)
    nsum = np.zeros((m, 3), np.float64)
    np.add.at(nsum, seg[fin], s[fin, 3:6].astype(np.float64))
    nfin = np.zeros(m, np.int64)
    np.add.at(nfin, seg[fin], 1)
    mask = np.zeros(m, np.uint32)
    np.bitwise_or.at(mask, seg, bit[order])
    rows = np.empty((m, 6), F32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        rows[:, :3] = (psum / count[:, None].astype(np.float64)).astype(F32)
        q = (nsum[:, 0] * nsum[:, 0] + nsum[:, 1] * nsum[:, 1]) + nsum[:, 2] * nsum[:, 2]
        nrm = (nsum / np.sqrt(q)[:, None]).astype(F32)
    nrm[(nfin == 0) | (q == 0)] = np.nan
    rows[:, 3:] = nrm
    popc = np.array([bin(int(v)).count("1") for v in mask], np.int64)
    summary = {"n_in": n_in, "n_out": m, "n_shared": int((popc >= 2).sum()), "max_count": int(count.max())}
    return rows, count.astype(np.uint32), mask, summary


def same_bits(a, b):
    """Bit-for-bit equality of two float32 arrays, NaNs by position (any NaN payload)."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (a.view(np.uint32)[~na] == b.view(np.uint32)[~nb]).all())
