"""numpy + scipy restatement of the candidate clustering (plade_amd/csrc/k_cluster.hip, cluster_transforms).

Edge: i ~ j when i != j and BOTH
    ((dx dx + dy dy) + dz dz) of the translations in float32  <  float32(float64(float32(r)) ** 2)      (pcl_r2, not float32(r) ** 2)
    ((e0 e0 + e1 e1) + e2 e2) of the Euler angle differences in float32  <  float32(gate).
A NaN in either expression is no edge (both comparisons are false).  The edge set is exact on both paths: brute force over all pairs
(outlier_restate.flann_d2 has this arithmetic order) up to BRUTE_MAX candidates; above that the candidate pairs of
cKDTree.query_pairs(1.001 r) in float64 -- a superset: the float32 expression is off from the true squared distance by a few ulps of
the largest squared coordinate difference, far less than the 0.2 % the candidate radius gives away -- each re-decided with the float32
expressions.  No tolerance, no excluded candidates.  Clusters are the connected components (scipy.sparse.csgraph), numbered in ascending
order of their smallest member: cluster c is the one with the c-th smallest seed, which is what the seam plade_cluster_transforms
returns.
"""
import numpy as np

from components_restate import labels_from_edges, pair_d2
from outlier_restate import flann_d2

F32 = np.float32
BRUTE_MAX = 8192


def r2_of(r):
    """pcl::KdTreeFLANN::radiusSearch: static_cast<float>(radius * radius) with `double radius` = the float threshold."""
    with np.errstate(over="ignore"):
        return F32(np.float64(F32(r)) ** 2)


def _rows(a):
    return np.ascontiguousarray(np.asarray(a, F32).reshape(-1, 3))


def _sorted(e):
    return e[np.lexsort((e[:, 1], e[:, 0]))].astype(np.int64)


def edges_brute(t_xyz, euler, r, gate, pairs=1 << 23):
    """All edges (i < j) by brute force: (k, 2) int64, sorted."""
    T, E = _rows(t_xyz), _rows(euler)
    n = len(T)
    r2, g = r2_of(r), F32(gate)
    out = [np.zeros((0, 2), np.int64)]
    step = max(1, pairs // max(n, 1))
    with np.errstate(invalid="ignore", over="ignore"):
        for c0 in range(0, n, step):
            near = (flann_d2(T[c0:c0 + step], T) < r2) & (flann_d2(E[c0:c0 + step], E) < g)
            ii, jj = np.nonzero(near)
            ii += c0
            m = ii < jj
            out.append(np.stack([ii[m], jj[m]], 1))
    return _sorted(np.concatenate(out))


def edges_kdtree(t_xyz, euler, r, gate):
    """The same edge set from k-d tree candidates (float64, 1.001 r) re-decided in float32.  Finite translations and a finite r only."""
    from scipy.spatial import cKDTree
    T, E = _rows(t_xyz), _rows(euler)
    cand = cKDTree(T.astype(np.float64)).query_pairs(1.001 * float(F32(r)), output_type="ndarray").astype(np.int64)
    if len(cand) == 0:
        return np.zeros((0, 2), np.int64)
    lo, hi = np.minimum(cand[:, 0], cand[:, 1]), np.maximum(cand[:, 0], cand[:, 1])
    with np.errstate(invalid="ignore", over="ignore"):
        m = (pair_d2(T, lo, hi) < r2_of(r)) & (pair_d2(E, lo, hi) < F32(gate))
    return _sorted(np.stack([lo[m], hi[m]], 1))


def edges(t_xyz, euler, r, gate):
    return edges_brute(t_xyz, euler, r, gate) if len(_rows(t_xyz)) <= BRUTE_MAX else edges_kdtree(t_xyz, euler, r, gate)


def cluster(t_xyz, euler, r, gate, edge_list=None):
    """(cluster_of int32, n_clusters): what plade_cluster_transforms returns for these candidates."""
    n = len(_rows(t_xyz))
    if n == 0:
        return np.zeros(0, np.int32), 0
    e = edges(t_xyz, euler, r, gate) if edge_list is None else edge_list
    label, size = labels_from_edges(n, e)
    return label, len(size)
