"""Every plane the extraction loop accepts, replayed on the CPU (tests/extract_replay.py).

The building blocks of the loop are pinned one at a time from outside (test_gpu_seams.py, test_gpu_golden.py); here the loop's
own use of them is: with dump = 1 the library hands out the acceptance chains of a detect call -- hypothesis, the four slots,
final slot, stop index -- and `audit` recomputes every score list, connected component, LS refit, weighted score, the refit
rule, the output plane and the bookkeeping from the hypothesis and the points unassigned at that moment.  Integer results
must match exactly, planes within the bounds stated in extract_replay.py.  What stays unpinned is the search: which
hypotheses are drawn, their scores on the subset, the stopping bound.

Measured over the scenes of this file on an MI355X (1472 accepted chains, 4054 slots, 2582 refits, none skipped for a small
eigenvalue gap): refit mean 0 ulp and refit normal at most 5.8e-11 from the plain fp64 fit; against the oracle's fp32 fit the
normal is within 1.2e-6 and the mean within 1.9e-5 (the oracle's own sequential fp32 sums: 395 points around z = 35 m in the
shaft, 1.1e-5 for 4261 points around 5 m in a room -- see ORACLE_SUM_SIGMA in extract_replay.py); wscore within 1.2e-5 relative.
"""
import numpy as np
import pytest

import plade_amd
import extract_replay as xr
from plade_amd.synth import make_pair, sample_scene

pytestmark = pytest.mark.gpu

_ctx = {}
_reports = {}


def _context():
    if "c" not in _ctx:
        _ctx["c"] = plade_amd.Context(0, dump=1, orient_normals=1)
    return _ctx["c"]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for c in _ctx.values():
        c.close()
    _ctx.clear()


def _extract_and_audit(name, cloud, min_support, oracle, orient=1, topup=1):
    ctx = _context()
    ctx.set_params(orient_normals=orient, ransac_topup=topup)
    assert 35000 <= len(cloud) <= 70000
    planes = ctx.extract_planes(cloud, min_support)
    trace = xr.trace_from_dump(ctx.dump())
    assert int(trace["call_u"][1]) == min_support and int(trace["call_u"][2]) == orient
    rep = xr.audit(cloud, planes, trace, oracle, collect_oracle_misses=True)
    assert rep["planes"] == len(planes[0])
    print(xr.format_report(name, rep))
    return rep


def _no_oracle_misses(reps):
    misses = [m for r in reps for m in r["oracle_misses"]]
    assert not misses, "\n".join(misses)


def _room(n=50000):
    return sample_scene(n, scene_seed=11, sample_seed=12, n_boxes=6)


def _shaft():
    rng = np.random.default_rng(4)
    n_wall, h = 12000, 40.0
    walls = []
    for ax, c, sgn in ((0, 0.0, 1), (0, 2.0, -1), (1, 0.0, 1), (1, 2.0, -1)):
        p = np.zeros((n_wall, 6), np.float32)
        p[:, ax] = c + rng.normal(0, 0.002, n_wall)
        p[:, 1 - ax] = rng.random(n_wall) * 2.0
        p[:, 2] = rng.random(n_wall) * h
        p[:, 3 + ax] = sgn
        walls.append(p)
    return np.ascontiguousarray(np.concatenate(walls)[rng.permutation(4 * n_wall)])


def _doubled_room(oracle):
    """The room, the room again shifted by exactly 3 eps along the normal of the walls y = const (every point of those walls
    gets a twin on the boundary of its wall's 3 eps slab), and 4000 exact duplicates."""
    room = _room(28000)
    scale = np.float32(oracle.cloud_scale(room))
    shift = np.float32(np.float32(3) * np.float32(np.float32(0.005) * scale))
    twin = room.copy()
    twin[:, 1] += shift
    cloud = np.ascontiguousarray(np.concatenate([room, twin, room[:4000]]))
    assert np.float32(oracle.cloud_scale(cloud)) == scale      # x is the longer side: eps is what the shift was made of
    return cloud


def _case(name, oracle):
    """One scene, extracted and audited once per session: (list of reports)."""
    if name in _reports:
        return _reports[name]
    if name.startswith("room-"):
        _, ms, orient, topup = name.split("-")
        reps = [_extract_and_audit(name, _room(), int(ms), oracle, int(orient), int(topup))]
    elif name == "tilted":
        cloud = sample_scene(60000, scene_seed=21, sample_seed=22, n_boxes=9, tilted=True)
        reps = [_extract_and_audit(name, cloud, 400, oracle)]
    elif name == "shaft":
        reps = [_extract_and_audit(name, _shaft(), 1000, oracle)]
    elif name == "doubled":
        reps = [_extract_and_audit(name, _doubled_room(oracle), 500, oracle)]
    elif name == "tiles":
        reps = [_extract_and_audit(f"tiles-{n}", _room(n), 500, oracle) for n in (40 * 1024, 40 * 1024 + 1)]
    elif name == "reuse":
        reps = [_extract_and_audit(f"reuse-{n}", sample_scene(n, scene_seed=3, sample_seed=n, n_boxes=5), 500, oracle) for n in (36000, 70000)]
    elif name == "group":
        reps = _group(oracle)
    else:
        raise KeyError(name)
    _reports[name] = reps
    return reps


def _group(oracle):
    """Three pairs = six clouds in one launch sequence; init_min_support low enough for one detect call per cloud (max_planes
    is raised so that no plane set is cut down to the largest 40 and re-ordered)."""
    if "g" not in _ctx:
        _ctx["g"] = plade_amd.Context(0, dump=1, orient_normals=1, init_min_support=300, max_planes=256)
    ctx = _ctx["g"]
    pairs = [tuple(np.ascontiguousarray(a) for a in make_pair(40000, seed=s)[:2]) for s in (3, 4, 5)]
    res = ctx.registration_pairs(pairs, raise_on_error=False)
    reps = []
    for i, (status, _) in enumerate(res):
        assert status in (0, plade_amd.PLADE_EFAIL)
        d, st = ctx.dump(pair=i), ctx.stats(pair=i)
        for side, tag in enumerate(("tgt", "src")):
            assert st[f"extract_planes_trial1_{tag}"] >= 10 and f"extract_planes_trial2_{tag}" not in st, "one detect call per cloud"
            planes = (d[f"{tag}_planes"].reshape(-1, 4), d[f"{tag}_plane_offsets"], d[f"{tag}_plane_idx"])
            rep = xr.audit(pairs[i][side], planes, xr.trace_from_dump(d, f"{tag}_"), oracle, collect_oracle_misses=True)
            print(xr.format_report(f"group pair {i} {tag}", rep))
            reps.append(rep)
    return reps


ROOMS = [f"room-{ms}-{orient}-{topup}" for ms in (500, 2000) for orient in (0, 1) for topup in (0, 1)]
ALL = ROOMS + ["tilted", "shaft", "doubled", "tiles", "group", "reuse"]


@pytest.mark.parametrize("name", ROOMS)
def test_room(oracle, name):
    _no_oracle_misses(_case(name, oracle))


def test_tilted_scene(oracle):
    """Boxes in general position: refits tilt into neighbouring surfaces, chains get deferred."""
    _no_oracle_misses(_case("tilted", oracle))


def test_tall_shaft_labels_in_global_memory(oracle):
    """Walls of 2 m x 40 m at a bitmap cell of 2 % of 2 m: 50 x 1000 pixels, the labelling inside the loop leaves LDS
    (CC_LDS_PIX = 4096).  With 12 000 points on 50 000 pixels a wall falls into hundreds of small components: every accepted
    entry stays below min_support -- points are taken, no plane comes out -- over hundreds of iterations."""
    reps = _case("shaft", oracle)
    assert reps[0]["entries"] >= 4 and reps[0]["max_list"] >= 10000      # whole walls were scored and labelled
    _no_oracle_misses(reps)


def test_duplicates_and_points_on_the_slab_boundary(oracle):
    _no_oracle_misses(_case("doubled", oracle))


def test_whole_tiles_and_one_point_more(oracle):
    _no_oracle_misses(_case("tiles", oracle))


def test_group_of_three_pairs(oracle):
    reps = _case("group", oracle)
    assert len(reps) == 6
    _no_oracle_misses(reps)


def test_context_reused_for_a_smaller_then_a_larger_cloud(oracle):
    """Chain slabs, bitmaps and the trace block are reused from cloud to cloud."""
    _case("room-500-1-1", oracle)
    reps = _case("reuse", oracle)
    assert len(reps) == 2
    _no_oracle_misses(reps)


def test_coverage_of_the_scenes(oracle):
    """What the scenes above must exercise, read from their traces (measured: up to 276 iterations, final slots up to 3,
    1070 entries below min_support, up to 8 chains accepted together, 45 deferred chains)."""
    reps = [(name, r) for name in ALL for r in _case(name, oracle)]
    for name, r in reps:
        print(f"{name}: iterations {r['iterations']} deferred chains {r['deferred']}")
    tot = {k: sum(r[k] for _, r in reps) for k in ("entries", "slots", "refits", "refits_small_gap", "below_min_support", "deferred")}
    worst = {k: max(r[k] for _, r in reps) for k in ("worst_pos_ulp", "worst_n_fp64", "worst_n_oracle", "worst_mean_oracle", "worst_wscore_rel")}
    print("total", tot, "worst", worst)
    assert max(r["iterations"] for _, r in reps) >= 3, "no cloud needed three iterations"
    assert max(r["max_final_slot"] for _, r in reps) >= 1, "no accepted entry kept a refit"
    assert max(r["max_batch"] for _, r in reps) >= 2, "no iteration accepted two chains together"
    if tot["below_min_support"] == 0:
        print("note: no entry was accepted below min_support in these scenes")
    assert tot["refits_small_gap"] <= xr.MAX_SKIPPED * tot["refits"]
