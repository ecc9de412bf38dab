"""The summaries of the cloud tools are reduced in ONE fixed order (plade_amd/csrc/fixed_reduce.h): every summary field equals the
numpy replay of that order (tests/fixed_order.py) over the GPU's own per-point outputs -- counts, maxima and quotients of sums bit
for bit, the fields behind a square root within 1 ulp of numpy's sqrt of the replayed sum.  Sizes: 1; the wave's edges 63, 64, 65;
the workgroup's 255, 256, 257; 16384 = 64 x 256 (one partial per lane of the final wavefront), 16385 (lane 0 takes a second
partial) and 16641 = 65 x 256 + 1 (a ragged last workgroup on top)."""
import numpy as np
import pytest

import plade_amd
import distance_restate as DR
import fixed_order as F

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 256, 257, 16384, 16385, 16641)


@pytest.fixture(scope="module")
def fctx():
    c = plade_amd.Context(0)
    yield c
    c.close()


_clouds = {}


def _cloud(n):
    """(rows (n, 6), a second noisy sample of the same sheet, radius): a wavy sheet over the unit square with noisy z and
    unit normals; about a dozen points within the radius of most points."""
    if n not in _clouds:
        rng = np.random.default_rng(1000 + n)

        def sample():
            xy = rng.uniform(0.0, 1.0, size=(n, 2))
            z = 0.05 * np.sin(6.0 * xy[:, 0]) + rng.normal(scale=0.004, size=n)
            nr = np.stack([-0.3 * np.cos(6.0 * xy[:, 0]), np.zeros(n), np.ones(n)], 1) + rng.normal(scale=0.05, size=(n, 3))
            nr /= np.linalg.norm(nr, axis=1, keepdims=True)
            return np.ascontiguousarray(np.concatenate([xy, z[:, None], nr], 1), dtype=np.float32)

        _clouds[n] = (sample(), sample(), float(min(0.4, np.sqrt(12.0 / (np.pi * n)))))
    return _clouds[n]


def _same_bits(a, b, what):
    a, b = np.float64(a), np.float64(b)
    assert a.tobytes() == b.tobytes(), (what, float(a), float(b))


def _within_1ulp(a, b, what):
    a, b = np.float64(a), np.float64(b)
    print(what, "same bits" if a == b else "differs", float(a), float(b))
    assert a == b or a == np.nextafter(b, np.inf) or a == np.nextafter(b, -np.inf), (what, float(a), float(b))


@pytest.mark.parametrize("n", SIZES)
def test_outliers_statistical(fctx, n):
    pts, _, _ = _cloud(n)
    _, kept, info = fctx.remove_outliers(pts, mode="statistical", k=8, alpha=1.0)
    m = info["mean_dist"]
    mu = F.reduce(m, np.add) / np.float64(n)
    e = m - mu
    s2 = F.reduce(e * e, np.add)
    sigma = np.sqrt(s2 / np.float64(n - 1)) if n > 1 else 0.0
    print("outliers", n, info["mu"], mu, info["sigma"], sigma)
    _same_bits(info["mu"], mu, "mu")
    _within_1ulp(info["sigma"], sigma, "sigma")
    _same_bits(info["threshold"], np.float64(info["mu"]) + np.float64(1.0) * np.float64(info["sigma"]), "threshold")
    assert info["kept"] == len(kept) == int((m <= info["threshold"]).sum())


@pytest.mark.parametrize("n", SIZES)
def test_smoothing(fctx, n):
    pts, _, r = _cloud(n)
    _, info = fctx.smooth_cloud(pts, r)
    fit, e, c = info["fitted_mask"], info["displacement"], info["count"]
    f = F.reduce(fit.astype(np.uint32), np.add)
    s2 = F.reduce(np.where(fit, e * e, 0.0), np.add)
    print("smooth", n, info["fitted"], f, info["rms"], info["max"], info["max_count"])
    assert info["fitted"] == f == int(fit.sum()) and (n < 256 or f > n // 2)
    assert info["max_count"] == F.reduce(c, np.maximum) == c.max()
    _same_bits(info["max"], F.reduce(np.where(fit, np.abs(e), 0.0), np.fmax), "max")
    _within_1ulp(info["rms"], np.sqrt(s2 / np.float64(f)) if f else 0.0, "rms")


@pytest.mark.parametrize("n", SIZES)
def test_m3c2(fctx, n):
    a, b, r = _cloud(n)
    dist, info = fctx.m3c2(a, a, b, r, 0.1)
    ok = ~np.isnan(dist)
    f = F.reduce(ok.astype(np.uint32), np.add)
    e = np.where(ok, dist, 0.0)
    print("m3c2", n, info["valid"], f, info["mean"], info["rms"], info["max"], info["max_count"])
    assert info["valid"] == f == int(ok.sum()) and (n < 256 or f > n // 2)
    assert info["significant"] == F.reduce((info["significant_mask"] & ok).astype(np.uint32), np.add)
    assert info["max_count"] == F.reduce(info["count"].max(axis=1), np.maximum)
    if f == 0:
        assert np.isnan(info["mean"]) and np.isnan(info["rms"]) and np.isnan(info["max"])
        return
    _same_bits(info["mean"], F.reduce(e, np.add) / np.float64(f), "mean")
    _same_bits(info["max"], F.reduce(np.abs(e), np.fmax), "max")
    _within_1ulp(info["rms"], np.sqrt(F.reduce(e * e, np.add) / np.float64(f)), "rms")


@pytest.mark.parametrize("n", SIZES)
def test_distances(fctx, n):
    tgt, src, r = _cloud(n)
    idx, d2, plane, s = fctx.cloud_distances(tgt, src, r)
    hit = idx >= 0
    dd = np.where(hit, d2.astype(np.float64), 0.0)
    dist = np.sqrt(dd)
    count = int(F.reduce(hit.astype(np.float64), np.add))
    print("distances", n, s["count"], count, s["mean"], s["rmse"], s["max"], s["plane_rmse"])
    assert s["n"] == n and s["count"] == count == int(hit.sum()) and (n < 256 or count > n // 2)
    assert s["plane_count"] == int(F.reduce((~np.isnan(plane)).astype(np.float64), np.add))
    if count == 0:
        assert np.isnan(s["mean"]) and np.isnan(s["rmse"]) and np.isnan(s["max"])
        return
    _same_bits(s["fitness"], np.float64(count) / np.float64(n), "fitness")
    _same_bits(s["mean"], F.reduce(dist, np.add) / np.float64(count), "mean")
    _same_bits(s["max"], F.reduce(dist, np.fmax), "max")
    _within_1ulp(s["rmse"], np.sqrt(F.reduce(dd, np.add) / np.float64(count)), "rmse")
    # the fp64 plane residuals are not returned: restated from the GPU's correspondences, at test_gpu_distances.py's tolerance
    res = DR.plane_residual(tgt, src, None, idx)
    fin = np.isfinite(res)
    ref = np.sqrt(F.reduce(np.where(fin, res * res, 0.0), np.add) / np.float64(fin.sum()))
    assert s["plane_count"] == int(fin.sum()) and abs(s["plane_rmse"] - ref) <= 1e-12 * abs(ref)


@pytest.mark.parametrize("n", SIZES)
def test_fpfh(fctx, n):
    pts, _, r = _cloud(n)
    _, info = fctx.fpfh(pts, r)
    d, c = info["described_mask"], info["pairs"].astype(np.uint64)
    f = F.reduce(d.astype(np.uint64), np.add)
    sc = F.reduce(np.where(d, c, np.uint64(0)), np.add)
    print("fpfh", n, info["described"], f, info["mean_pairs"], info["max_pairs"])
    assert info["described"] == f == int(d.sum()) and (n < 256 or f > n // 2)
    assert info["max_pairs"] == F.reduce(c, np.maximum) == c.max()
    _same_bits(info["mean_pairs"], np.float64(sc) / np.float64(f) if f else 0.0, "mean_pairs")
