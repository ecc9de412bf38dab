"""Inputs of the pose estimator's tests: synthetic correspondence sets with a known pose, and a pair of scans of a terrain without
planes (the case the feature registration exists for)."""
import numpy as np

from plade_amd.synth import random_se3

BOX = 10.0


def synthetic(M, share, seed, noise=0.0, box=BOX, shuffle=False):
    """M correspondences between two clouds of M points each, `share` of them true.  Source points uniform in the box; a true
    correspondence's target point is T S + noise * N(0, 1), T = random_se3(seed); the others' are uniform in the box.  Returns
    (src (M, 3), tgt (M, 3), corr (M, 2) int32, T (4, 4), inlier (M,) bool) in float64 -- a test casts the points to float32 for the
    library and hands the restatement the same float32 values.  With shuffle the target points are stored in a random order."""
    rng = np.random.default_rng(seed)
    T = random_se3(seed)
    S = rng.uniform(0.0, box, (M, 3))
    inl = np.zeros(M, bool)
    inl[rng.permutation(M)[:int(round(share * M))]] = True
    Q = rng.uniform(0.0, box, (M, 3))
    Q[inl] = S[inl] @ T[:3, :3].T + T[:3, 3] + noise * rng.normal(size=(int(inl.sum()), 3))
    order = rng.permutation(M) if shuffle else np.arange(M)
    tgt = np.empty_like(Q)
    tgt[order] = Q
    corr = np.stack([np.arange(M), order], axis=1).astype(np.int32)
    return S, tgt, corr, T, inl


def _terrain(scene_seed):
    rng = np.random.default_rng(scene_seed)
    c = rng.uniform((0.0, 0.0), (10.0, 8.0), (40, 2))
    a = rng.uniform(0.5, 1.5, 40) * rng.choice((-1.0, 1.0), 40)
    s = rng.uniform(0.4, 1.0, 40)
    return c, a, s


def _sample_terrain(n, scene, sample_seed, noise=0.005):
    """n points x y z nx ny nz (float64) on z = sum a_k exp(-|p - c_k|^2 / (2 s_k^2)) over the 10 x 8 plate, analytic unit normals,
    Gaussian noise along the normal"""
    c, a, s = scene
    rng = np.random.default_rng(sample_seed)
    p = rng.uniform((0.0, 0.0), (10.0, 8.0), (n, 2))
    d = p[:, None, :] - c[None, :, :]
    g = a * np.exp(-(d * d).sum(axis=2) / (2.0 * s * s))
    z = g.sum(axis=1)
    grad = -(g[:, :, None] * d / (s * s)[None, :, None]).sum(axis=1)
    nrm = np.concatenate([-grad, np.ones((n, 1))], axis=1)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    pts = np.concatenate([p, z[:, None]], axis=1) + noise * rng.normal(size=(n, 1)) * nrm
    return np.concatenate([pts, nrm], axis=1)


def terrain_pair(n, scene_seed=7, keep=0.7, amplitude=1.0):
    """(target (n, 6), source (~n, 6), T_gt) float32 clouds of 40 Gaussian bumps on a 10 x 8 plate: the target is one sampling, the
    source another one cut at the `keep` quantile of x and moved by inv(random_se3(9001)); T_gt maps source -> target."""
    c, a, s = _terrain(scene_seed)
    scene = (c, amplitude * a, s)
    target = _sample_terrain(n, scene, 1)
    full = _sample_terrain(int(n / keep), scene, 2)
    part = full[full[:, 0] <= np.quantile(full[:, 0], keep)]
    T = random_se3(9001)
    Ti = np.linalg.inv(T)
    source = np.concatenate([part[:, :3] @ Ti[:3, :3].T + Ti[:3, 3], part[:, 3:] @ Ti[:3, :3].T], axis=1)
    return np.ascontiguousarray(target, np.float32), np.ascontiguousarray(source, np.float32), T
