"""pca_eig (plade_amd/csrc/pca_eig.h) on the GPU, through its two callers, against the exact reference and the contract of
tests/eig_cases.py: blocks of exact fp32 points whose neighbourhoods are the blocks themselves, spectra from well separated to
needles with (l1 - l0) / trace of 1e-9, exact planes, lines, a prolate double root, an isotropic block and coincident points.

Normals (estimate_normals, k = 3, 16, 33, 64 and the table far from the origin): the neighbour lists are the blocks, then the contract
against the long-double decomposition of each block's exact integer covariance.  Smoothing (smooth_cloud on the k = 16 tables):
the reference starts from the GPU's own moments, C = M / W - mu mu^T in long double, and the displacement is checked as well.
The viewpoint rule and the bits of the positions are test_gpu_normals.py's and test_gpu_smooth.py's.

Measured on an MI355X (worst e per block kind beyond the fp32 floor): DESIGN.md section 9.
"""
import numpy as np
import pytest

import plade_amd
import eig_cases as E
from conftest import ORIENTED
from test_eig_cases_host import check_displacement

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not E.LD_OK, reason="numpy.longdouble carries fewer than 64 bits here")]
F64 = np.float64


@pytest.fixture(scope="module")
def ectx():
    c = plade_amd.Context(0, **ORIENTED)
    yield c
    c.close()


@pytest.mark.parametrize("name", E.TABLES)
def test_normals_meet_the_contract(ectx, name):
    T = E.table(name)
    out, curv, nbr = ectx.estimate_normals(T.P, k=T.k, curvature=True, neighbours=True)
    want = np.stack([T.members[b] for b in T.block_of])
    assert np.array_equal(np.sort(nbr, axis=1), want)
    lam, V, zero = T.ref
    kinds = np.array([T.kinds[b] for b in T.block_of])
    live = ~zero[T.block_of]
    blk = T.block_of[live]
    n = out[live, 3:]
    err = E.check(n, curv[live], lam[blk], V[blk], kinds[live])
    print(name, "worst e per kind beyond the fp32 floor:\n" + E.report(err, kinds[live]))
    assert np.isnan(out[~live, 3:]).all() and np.isnan(curv[~live]).all()           # coincident points: NaN, as ever
    for b, B in enumerate(T.blocks):
        m = T.members[b]
        if zero[b]:
            continue
        if B.axis is not None:          # the exact line, the exact prolate block, collinear triples: across the known axis
            a = B.axis / np.linalg.norm(B.axis)
            bound = E.FLOOR + E.M * E.EPS * float(lam[b].sum() / (lam[b, 2] - lam[b, 1]))
            assert (np.abs(out[m, 3:].astype(F64) @ a) <= bound).all(), B.kind
        if B.normal is not None:
            c = B.normal / np.linalg.norm(B.normal)
            bound = E.FLOOR + E.M * E.EPS * float(lam[b].sum() / (lam[b, 1] - lam[b, 0]))
            assert (np.linalg.norm(np.cross(out[m, 3:].astype(F64), c), axis=1) <= bound).all(), B.kind
        if B.kind == "exact isotropic":
            assert np.isfinite(out[m, 3:]).all() and (np.abs(np.linalg.norm(out[m, 3:].astype(F64), axis=1) - 1) <= 1e-6).all()
            assert (np.abs(curv[m].astype(F64) - 1 / 3) <= E.FLOOR / 3 + E.M * E.EPS).all()


@pytest.mark.parametrize("name", ["k16", "k16_far"])
def test_smoothing_meets_the_contract(ectx, name):
    T = E.table(name)
    rows, info = ectx.smooth_cloud(T.P, T.radius, min_neighbours=3, moments=True)
    assert (info["count"] == 16).all()
    zero = T.ref[2]
    live = ~zero[T.block_of]
    assert np.array_equal(info["fitted_mask"], live)
    assert np.isnan(rows[~live, 3:]).all() and np.isnan(info["curvature"][~live]).all() and (info["displacement"][~live] == 0).all()
    kinds = np.array([T.kinds[b] for b in T.block_of])
    lam, V, mu = E.moment_reference(info["moments"][live])
    n = rows[live, 3:]
    err = E.check(n, info["curvature"][live], lam, V, kinds[live])
    print(name, "worst e per kind beyond the fp32 floor:\n" + E.report(err, kinds[live]))
    # delta is the fp64 n . mu of the kernel; the normal it returns is that n rounded to fp32, within the floor the bound has
    check_displacement(info["displacement"][live], n, V, mu, err, T.radius)
