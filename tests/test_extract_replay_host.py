"""The replay of the extraction's acceptance chains (tests/extract_replay.py) has teeth: it passes on what its own
sequential CPU driver produces and names the right step under single mutations of the planes or of the trace.  No GPU."""
import numpy as np
import pytest

import extract_replay as xr
from plade_amd.synth import sample_scene

MIN_SUPPORT = 500


@pytest.fixture(scope="module")
def driven(oracle):
    cloud, labels = sample_scene(50000, scene_seed=11, sample_seed=12, n_boxes=6, return_labels=True)
    rng = np.random.default_rng(5)
    faces = [f for f in np.unique(labels) if f >= 0 and (labels == f).sum() >= 800]
    hyps = []
    # three points of one ground-truth face each.  The last four return to faces that are gone by then: what is left within
    # 3 eps of them stays below min_support, so no refit is kept (final slot 0) and the entry yields no plane
    for q in range(20):
        pts = np.nonzero(labels == faces[q % 16])[0]
        hyps.append(cloud[rng.choice(pts, 3, replace=False), :3].reshape(9))
    trace, planes = xr.drive(cloud, np.array(hyps), oracle, MIN_SUPPORT, 0.005, 0.02, 0.8, orient=1, batch=4)
    return cloud, planes, trace


def _mutable(driven):
    cloud, (coef, off, idx), trace = driven
    return cloud, [coef.copy(), off.copy(), idx.copy()], xr.copy_trace(trace)


def test_audit_passes_on_the_drivers_trace_and_both_refit_branches_occur(driven, oracle):
    cloud, planes, trace = driven
    rep = xr.audit(cloud, planes, trace, oracle)
    print(xr.format_report("driver", rep))
    finals = trace["entry"][:, 2]
    assert rep["entries"] == len(finals) >= 10 and rep["planes"] >= 8
    assert (finals == 0).any() and (finals >= 1).any(), "both branches of the refit rule must be present"
    assert rep["max_batch"] >= 2 and rep["refits"] >= rep["entries"] and rep["below_min_support"] >= 1
    assert rep["worst_pos_ulp"] == 0 and rep["worst_n_fp64"] == 0      # the driver's fit IS the fp64 restatement


def _expect(step, cloud, planes, trace, oracle, *names):
    with pytest.raises(xr.AuditError) as ei:
        xr.audit(cloud, planes, trace, oracle)
    assert ei.value.step == step, str(ei.value)
    for s in names:
        assert s in str(ei.value), str(ei.value)


def test_one_index_removed_from_a_plane(driven, oracle):
    cloud, planes, trace = _mutable(driven)
    p = 2
    planes[2] = np.delete(planes[2], planes[1][p] + 7)
    planes[1][p + 1:] -= 1
    _expect(4, cloud, planes, trace, oracle, f"plane {p})", "1 only on the CPU")


def test_index_of_an_earlier_plane_added_to_a_later_one(driven, oracle):
    cloud, planes, trace = _mutable(driven)
    stolen = planes[2][planes[1][1] + 3]
    p = 4
    planes[2] = np.insert(planes[2], planes[1][p + 1], stolen)
    planes[1][p + 1:] += 1
    _expect(4, cloud, planes, trace, oracle, f"plane {p})", "1 only in the output")


def test_final_slot_changed(driven, oracle):
    cloud, planes, trace = _mutable(driven)
    e = int(np.nonzero(trace["entry"][:, 2] >= 1)[0][0])
    trace["entry"][e, 2] = 0
    _expect(7, cloud, planes, trace, oracle, f"entry {e} ")


def test_two_entries_of_an_iteration_swapped(driven, oracle):
    cloud, planes, trace = _mutable(driven)
    its = trace["entry"][:, 0]
    e = int(np.nonzero(its[1:] == its[:-1])[0][0])
    for k in xr.TRACE_KEYS[2:]:
        trace[k][[e, e + 1]] = trace[k][[e + 1, e]]
    _expect(9, cloud, planes, trace, oracle, f"iteration {its[e]}", "best first")


def test_n_remaining_off_by_one(driven, oracle):
    cloud, planes, trace = _mutable(driven)
    trace["call_u"][4] += 1
    _expect(10, cloud, planes, trace, oracle, "n_remaining")


def test_one_coefficient_changed_by_one_ulp(driven, oracle):
    cloud, planes, trace = _mutable(driven)
    planes[0][3, 1] = np.nextafter(planes[0][3, 1], np.float32(2))
    _expect(8, cloud, planes, trace, oracle, "plane 3)")


def test_a_slots_plane_replaced_by_the_previous_slots(driven, oracle):
    cloud, planes, trace = _mutable(driven)
    e = int(np.nonzero(trace["entry"][:, 2] >= 1)[0][0])
    k = int(trace["entry"][e, 2])
    trace["slot_f"][e, k] = trace["slot_f"][e, k - 1]
    _expect(5, cloud, planes, trace, oracle, f"entry {e} ", f"slot {k}")
