"""plade_icp_linearize and plade_gicp_linearize where the last workgroup of the match kernel is one lane, one lane short of a wave,
a wave, one lane more, ..., and two workgroups and a lane: the tail lanes and the write of the correspondences, against the numpy
restatements under the rule and tolerance of test_seam_is_exact_on_the_golden_scenes."""
import numpy as np
import pytest

import plade_amd
from conftest import ORIENTED
import icp_restate as R
import refine_messages as M
from test_gpu_gicp import _check_seam as _check_gicp_seam
from test_gpu_icp import _check_seam as _check_icp_seam

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257, 513]


@pytest.fixture(scope="module")
def rctx():
    c = plade_amd.Context(0, **ORIENTED)
    yield c
    c.close()


@pytest.fixture(scope="module")
def corner():
    """A corner of three planes (nothing is degenerate): 2 000 target points, the source rows a little off them, the restatement's
    target"""
    tgt = M.corner(2000, 11)
    src = M.corner(max(SIZES), 12)
    src[:, :3] += np.random.default_rng(13).normal(scale=0.004, size=(len(src), 3)).astype(np.float32)
    return tgt, src, R.Target(tgt), R.perturb(np.eye(4), 0.01, 0.01, seed=3)


@pytest.mark.parametrize("center", [None, (0.4, -0.3, 0.7)])
@pytest.mark.parametrize("n", SIZES)
def test_seams_at_workgroup_boundaries(rctx, corner, n, center):
    tgt, src, target, T = corner
    rows = np.ascontiguousarray(src[:n])
    corr, mom = _check_icp_seam(rctx, target, tgt, np.ascontiguousarray(rows[:, :3]), T, 0.05, center=center)
    assert len(corr) == n and mom[28] == (corr >= 0).sum()
    for eps in (1e-3, 1.0):
        corr, mom = _check_gicp_seam(rctx, target, tgt, rows, T, 0.05, eps, center=center)
        assert len(corr) == n and mom[29] == (corr >= 0).sum()
