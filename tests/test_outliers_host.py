"""Outlier removal, host side (no GPU): the entry points are declared, exported, bound and listed; the default parameters need
no GPU; the CLI without the switch behaves as the parent revision's; and the numpy restatement of the semantics
(tests/outlier_restate.py) removes the generated outliers of a synthetic scene and hardly any surface point."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import plade_amd
from plade_amd.synth import sample_scene
import outlier_restate as R
from test_normals_host import CLI, PARENT_RESULT, PARENT_STDERR, PARENT_STDOUT, _write, _xyz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("plade_outlier_default_params", "plade_filter_outliers", "plade_cloud_filter_outliers_dev")


def test_new_symbols_are_declared_exported_bound_and_listed():
    hdr = open(os.path.join(ROOT, "include", "plade_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(plade_[a-z_0-9]+)\s*\(", hdr))
    L = plade_amd.load_library()
    for s in NEW:
        assert s in declared, s
        assert hasattr(L, s), s
        assert s in plade_amd.ABI_SYMBOLS
        assert getattr(L, s).argtypes is not None
    for m in ("remove_outliers", "remove_outliers_dev"):
        assert callable(getattr(plade_amd.Context, m))
    for t in ("plade_outlier_params", "plade_outlier_summary"):
        assert re.search(r"\}\s*" + t + r"\s*;", hdr), t


def test_default_params_need_no_gpu():
    p = plade_amd.OutlierParams()
    p.k, p.alpha, p.radius, p.min_neighbours, p.mode = -7, -1.0, -1.0, -7, 9
    plade_amd.load_library().plade_outlier_default_params(ctypes.byref(p))
    assert (p.mode, p.k, p.alpha, p.radius, p.min_neighbours, p.reserved) == (plade_amd.PLADE_OUTLIER_STATISTICAL, 16, 1.0, 0.0, 1, 0)
    assert plade_amd.outlier_default_params() == {"mode": 0, "k": 16, "alpha": 1.0, "radius": 0.0, "min_neighbours": 1}


def test_structs_match_the_header():
    P, S = plade_amd.OutlierParams, plade_amd.OutlierSummary
    assert [f for f, _ in P._fields_] == ["mode", "k", "alpha", "radius", "min_neighbours", "reserved"]
    assert ctypes.sizeof(P) == 32 and P.alpha.offset == 8 and P.radius.offset == 16 and P.min_neighbours.offset == 24
    assert [f for f, _ in S._fields_] == ["n", "kept", "mu", "sigma", "threshold"]
    assert ctypes.sizeof(S) == 40 and S.mu.offset == 16 and S.threshold.offset == 32


def test_the_header_with_the_new_structs_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "plade_hip.h"\nint main(void) { plade_outlier_params p; plade_outlier_summary s; plade_outlier_default_params(&p);\n'
                   '  s.kept = 0; return (int)(sizeof(p) + sizeof(s) + s.kept) & 0; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_cli_without_the_switch_is_the_parents(tmp_path):
    pt, ps = str(tmp_path / "t.ply"), str(tmp_path / "s.ply")
    for p, seed in ((pt, 1), (ps, 2)):
        _write(p, _xyz(100, seed=seed), "binary_little_endian", np.float32)
    env = {k: v for k, v in os.environ.items() if not k.startswith("PLADE_")}
    for extra in ({}, {"PLADE_REMOVE_OUTLIERS": "0"}):
        res = str(tmp_path / "r.txt")
        r = subprocess.run([CLI, pt, ps, res], capture_output=True, text=True, timeout=120, env=dict(env, **extra))
        assert (r.returncode, r.stdout, r.stderr) == (1, PARENT_STDOUT.format(t=pt, s=ps), PARENT_STDERR), extra
        assert open(res).read() == PARENT_RESULT


def test_restatement_breaks_ties_by_index_and_counts_duplicates():
    g = np.stack(np.meshgrid(np.arange(4), np.arange(3), np.arange(3), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    P = np.concatenate([g, g, g])                                  # every lattice point three times
    n = len(g)
    keys, counts = R.neighbours(P, kmax=8, radii=(1.0, np.nextafter(np.float32(1.0), np.float32(2.0))))
    idx, d2 = R.key_index(keys), R.key_d2(keys)
    for i in (0, n + 5, 2 * n + 17):
        twins = sorted(j for j in (i % n, i % n + n, i % n + 2 * n) if j != i)
        assert list(idx[i, :2]) == twins and (d2[i, :2] == 0).all()
        assert (d2[i, 2:] == 1).all() and (np.diff(idx[i, 2:]) > 0).all()   # the six-neighbourhood at distance 1, ascending index
    axis = np.array([((g == p).sum(1) == 2) & (np.abs(g - p).sum(1) == 1) for p in g]).sum(1)   # lattice neighbours at distance 1
    assert np.array_equal(counts[0], np.tile(2, 3 * n))            # r = 1 exactly: only the two twins are closer (`<`)
    assert np.array_equal(counts[1], np.tile(2 + 3 * axis, 3))     # one ulp above: the neighbours at distance 1, three times each
    m = R.mean_dist(keys, 2)
    assert (m == 0).all()


def test_restatement_agrees_with_a_kd_tree_on_a_small_scene():
    pytest.importorskip("scipy.spatial")
    P = sample_scene(3000, scene_seed=3, sample_seed=5)
    a, b = R.statistical(P, 16, 1.0), R.statistical_kdtree(P, 16, 1.0)
    assert np.allclose(a["m"], b["m"], rtol=1e-5, atol=1e-7)
    clear = np.abs(b["m"] - b["threshold"]) > 1e-5 * b["threshold"]
    assert np.array_equal(a["keep"][clear], b["keep"][clear])
    c, keep = R.radius(P, 0.1, 3)
    from scipy.spatial import cKDTree
    X = P[:, :3].astype(np.float64)
    want = np.array([len(v) - 1 for v in cKDTree(X).query_ball_point(X, 0.1)])
    assert np.abs(c.astype(np.int64) - want).max() <= 1 and (c.astype(np.int64) != want).mean() < 1e-3   # fp32 vs fp64 on the boundary


def test_restatement_removes_the_generated_outliers():
    """The semantics do what the filter is for.  200k scene, k = 16, alpha = 1 by a k-d tree: at least 80 % of the generated
    outliers go, at most 0.1 % of the surface points (measured: 86.0 % and 0.002 %).  Without scipy: brute force on a 20k scene
    at alpha = 2, at least 50 % and at most 0.1 % (measured: 58.8 % and 0.03 %)."""
    try:
        import scipy.spatial  # noqa: F401
        cloud, labels = sample_scene(200000, scene_seed=3, sample_seed=4, return_labels=True)
        keep, lo = R.statistical_kdtree(cloud, 16, 1.0)["keep"], 0.80
    except ImportError:
        cloud, labels = sample_scene(20000, scene_seed=3, sample_seed=4, return_labels=True)
        keep, lo = R.statistical(cloud, 16, 2.0)["keep"], 0.50
    out = labels < 0
    removed, lost = float((~keep[out]).mean()), float((~keep[~out]).mean())
    print(f"outliers removed {removed:.4f}, surface points lost {lost:.6f}")
    assert removed >= lo, removed
    assert lost <= 0.001, lost
