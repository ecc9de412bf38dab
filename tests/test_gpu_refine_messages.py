"""The refusals of the two ICP refinements, word for word (tests/refine_messages.py: recorded before the two shared one driver)."""
import numpy as np
import pytest

import plade_amd
from conftest import ORIENTED
import refine_messages as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rctx():
    c = plade_amd.Context(0, **ORIENTED)
    yield c
    c.close()


def test_every_refusal_keeps_its_code_and_its_words(rctx):
    assert {e for e, _, _, _ in M.CASES} == set(M.ENTRIES)
    for entry, case, code, text in M.CASES:
        rc, said, out = M.call(rctx, entry, case)
        assert (rc, said) == (code, text), (entry, case)
        if code == plade_amd.PLADE_EFAIL:                      # a failed refinement hands T_in back
            assert np.array_equal(out, np.eye(4, dtype=np.float32)), (entry, case)
    # the same context still refines
    tgt, src = M.scene("corner")
    for T, info in (rctx.refine_icp(tgt, src, np.eye(4), **M.GOOD), rctx.refine_gicp(tgt, src, np.eye(4), **M.GOOD)):
        assert info["failure"] == 0 and info["converged"] and np.abs(T - np.eye(4)).max() <= 1e-3, (T, info)
