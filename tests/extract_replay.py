"""CPU replay of the plane extraction's acceptance chains (plade_amd/csrc/ransac.hip, k_r_decide).

The search of the extraction loop is random, its acceptance is not: given the hypothesis a chain started from and the points
that were unassigned at that moment, every list, component, refit and score of the chain follows.  With plade_params.dump
the library keeps, for every chain it accepted, the hypothesis and the four slots as k_r_decide saw them (the dump's
`extract_trace_*` arrays); `audit` walks them in order with the CPU oracle (oracle.score_plane, connected_component, ls_fit,
weighted_score -- each pinned to libransac) and a plain fp64 restatement of the LS fit, and raises at the first difference
with a message that names the entry, its plane, the slot and the step:

    step 0   the trace itself is well formed; slot 0 is the hypothesis
    step 1/2 |score list| of slot 0 / of a refit slot = n_list
    step 3   |largest connected component of the list| = n_kept
    step 4   the final slot's component = the plane's index list, as a set
    step 5   a refit slot's plane = LS fit of the previous slot's component
    step 6   wscore = the weighted score of the component
    step 7   final slot and stop index follow from the slots' own n_kept / wscore / err by the reference's refit rule
    step 8   the output plane: coefficients bit for bit, orientation, presence, order
    step 9   the chains of an iteration, accepted together = accepted one by one, best first
    step 10  bookkeeping: n_remaining, every index at most once, the assignment the output implies

`drive` is a small sequential driver with the same acceptance semantics on caller-given hypotheses: it writes a trace and a
plane set in the library's format (the audit's own test, tests/test_extract_replay_host.py, mutates them).
Plain numpy + the oracle; needs no GPU.
"""
import numpy as np

F = np.float32
TRACE_KEYS = ("call_u", "call_f", "entry", "cand", "slot_f", "slot_u", "slot_w")
NORMAL_ORACLE_TOL = 5e-5      # the oracle's (= the reference's) fp32 accumulation noise
MEAN_ORACLE_TOL = 1e-5
MEAN_ORACLE_TOL_LONG = 2e-4   # ... where the list is long (tests/test_gpu_seams.py, plane_component: 35 000 points around 20)
# "Long" is where the ORACLE's own mean cannot be expected inside MEAN_ORACLE_TOL.  It adds the m coordinates one after the other
# in fp32, like the reference: the i-th addition rounds a partial sum of about i * c (c = the mean coordinate) by up to half an ulp,
# i.e. with a standard deviation of about 0.75 * 2^-23 * i * c / sqrt(12); the sum of those, divided by m, has a standard deviation
# of about 1.5e-8 * c * sqrt(m).  A list counts as long once four of these exceed MEAN_ORACLE_TOL (c = 5, m > 1100; c = 20, m > 70).
# The library's own mean is held to one fp32 ulp of the fp64 mean whatever the length.
ORACLE_SUM_SIGMA = 1.5e-8
NORMAL_FP64_TOL = 2.4e-7      # 2 fp32 ulps of 1.0
GAP_REL = 1e-6                # the fp64 normal is compared where the two smallest eigenvalues are >= GAP_REL * scale^2 apart
MAX_SKIPPED = 0.05            # ... and at most this share of the refits may fall below that gap
WSCORE_TOL = 1e-4             # relative (tests/test_gpu_seams.py, plane_component)
ORIENT_TIE = 1e-5             # |sum of normals . n| below this times the point count: the sign is not asserted


class AuditError(AssertionError):
    def __init__(self, step, message):
        super().__init__(f"step {step}: {message}")
        self.step = step


def trace_from_dump(dump, tag=""):
    """The trace of one cloud out of Context.dump(): tag "" after extract_planes, "tgt_" / "src_" after a registration."""
    t = {k: dump[f"{tag}extract_trace_{k}"] for k in TRACE_KEYS}
    return normalise_trace(t)


def normalise_trace(t):
    e = int(t["call_u"][6])
    return {"call_u": np.asarray(t["call_u"], np.uint32).copy(), "call_f": np.asarray(t["call_f"], np.float32).copy(),
            "entry": np.asarray(t["entry"], np.int32).reshape(e, 5).copy(), "cand": np.asarray(t["cand"], np.float32).reshape(e, 8).copy(),
            "slot_f": np.asarray(t["slot_f"], np.float32).reshape(e, 4, 7).copy(),
            "slot_u": np.asarray(t["slot_u"], np.uint32).reshape(e, 4, 4).copy(),
            "slot_w": np.asarray(t["slot_w"], np.float64).reshape(e, 4).copy()}


def copy_trace(t):
    return {k: v.copy() for k, v in t.items()}


def dot3_f32(a, b):
    """a . b in fp32, accumulated left to right without contraction (the library's and the reference's Vec3f::dot)."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    d = F(a[0] * b[0])
    d = F(d + F(a[1] * b[1]))
    return F(d + F(a[2] * b[2]))


def output_plane(n, pos):
    """plane_extraction.cpp:134-149 as k_r_decide restates it: n re-normalised in fp32, d = -n.pos."""
    nn = np.asarray(n, F).copy()
    pos = np.asarray(pos, F)
    l = F(nn[0] * nn[0])
    l = F(l + F(nn[1] * nn[1]))
    l = F(l + F(nn[2] * nn[2]))
    l = F(np.sqrt(l))
    if l > 0:
        nn = (nn / l).astype(F)
    d = F(-F(F(F(nn[0] * pos[0]) + F(nn[1] * pos[1])) + F(nn[2] * pos[2])))
    return np.array([nn[0], nn[1], nn[2], d], F)


def refit_rule(n_kept, wscore, err, min_support):
    """RansacShapeDetector.cpp:633-655 on the four slots' results: (final slot, stop index)."""
    final_slot, stop = 0, 4
    new_score = float(wscore[0])
    for k in (1, 2, 3):
        old_score = new_score
        if n_kept[k - 1] < 3 or err[k]:
            stop = k
            break
        new_score = float(wscore[k])
        if new_score > old_score and n_kept[k] > min_support:
            final_slot = k
        if not new_score > old_score:
            stop = k
            break
    return final_slot, stop


def fit_fp64(cloud, kept):
    """LS plane of the points in plain fp64: (fp64 mean, unit eigenvector of the smallest eigenvalue, gap to the next)."""
    p = cloud[kept, :3].astype(np.float64)
    mean = p.mean(0)
    q = p - mean
    w, v = np.linalg.eigh(q.T @ q / len(p))
    return mean, v[:, 0], float(w[1] - w[0])


def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, F)))


def new_report():
    return {"entries": 0, "planes": 0, "slots": 0, "refits": 0, "refits_small_gap": 0, "worst_pos_ulp": 0.0, "worst_n_fp64": 0.0,
            "worst_n_oracle": 0.0, "worst_mean_oracle": 0.0, "worst_wscore_rel": 0.0, "iterations": 0, "deferred": 0,
            "max_final_slot": 0, "below_min_support": 0, "max_batch": 0, "max_list": 0, "orient_ties": 0, "oracle_misses": []}


def format_report(name, r):
    return (f"{name}: entries {r['entries']} planes {r['planes']} slots {r['slots']} refits {r['refits']} "
            f"(small gap: {r['refits_small_gap']}) worst pos {r['worst_pos_ulp']:.2f} ulp, n vs fp64 {r['worst_n_fp64']:.2e}, "
            f"n vs oracle {r['worst_n_oracle']:.2e}, mean vs oracle {r['worst_mean_oracle']:.2e}, wscore rel {r['worst_wscore_rel']:.2e}; "
            f"iterations {r['iterations']} deferred {r['deferred']} max final slot {r['max_final_slot']} "
            f"below min_support {r['below_min_support']} max batch {r['max_batch']}")


def _chain_lists(cloud, assigned, sf, kmax, errs, eps3, cos_t, oracle):
    return [np.sort(oracle.score_plane(cloud, assigned, np.array([*sf[k, :3], sf[k, 6]], F), eps3, cos_t)) if not errs[k]
            else np.zeros(0, np.int32) for k in range(kmax + 1)]


def audit(cloud, planes, trace, oracle, collect_oracle_misses=False):
    """Replays `trace` (see trace_from_dump) on `cloud` (N x 6 float32) and compares with planes = (coef P x 4, offsets, idx).
    Returns the report (new_report); raises AuditError at the first discrepancy.  collect_oracle_misses: a refit plane that
    agrees with the fp64 restatement but misses the bound against the oracle's fp32 fit by little is written to
    report["oracle_misses"] instead and the walk goes on (the caller asserts that list empty once everything else is checked)."""
    cloud = np.ascontiguousarray(cloud, F)
    coef, offsets, idx = planes
    coef = np.asarray(coef, F).reshape(-1, 4)
    offsets = np.asarray(offsets, np.int64)
    idx = np.asarray(idx, np.int64)
    t = trace
    n, min_support, orient, iterations, n_remaining, n_deferred, E, n_planes = (int(x) for x in t["call_u"])
    eps, eps3, bitmap_eps, cos_t = (F(x) for x in t["call_f"])
    rep = new_report()
    rep["iterations"], rep["deferred"], rep["entries"] = iterations, n_deferred, E
    # ---- step 0: the trace and the call's scalars
    if n != len(cloud):
        raise AuditError(0, f"the call saw {n} points, the cloud has {len(cloud)}")
    if eps3 != F(F(3) * eps):
        raise AuditError(0, f"eps3 {eps3} is not 3 x eps {eps}")
    scale = float(oracle.cloud_scale(cloud))
    if len(t["entry"]) != E:
        raise AuditError(0, "entry count")
    P = len(coef)
    if len(offsets) != P + 1 or offsets[0] != 0 or (len(idx) != offsets[-1]):
        raise AuditError(8, f"plane set is not consistent: {P} planes, offsets {len(offsets)}, {len(idx)} indices")
    if n_planes != P:
        raise AuditError(8, f"the trace reports {n_planes} planes, the output holds {P}")
    its = t["entry"][:, 0]
    if E and (np.any(np.diff(its) < 0) or its.min() < 0 or its.max() >= iterations):
        raise AuditError(0, f"iterations of the entries are not ascending inside 0..{iterations - 1}")
    assigned = np.full(n, -1, np.int32)
    next_plane = 0
    taken_total = 0
    e0 = 0
    while e0 < E:
        e1 = e0
        while e1 < E and its[e1] == its[e0]:
            e1 += 1
        chains = t["entry"][e0:e1, 1]
        # ---- step 9 (order): the chains of a batch are accepted best first = in chain order
        if np.any(np.diff(chains) <= 0) or chains.min() < 0 or chains.max() >= 8:
            raise AuditError(9, f"iteration {its[e0]}: entries {e0}..{e1 - 1} are not in chain order (best first): chains {chains.tolist()}")
        rep["max_batch"] = max(rep["max_batch"], e1 - e0)
        batch = []
        for e in range(e0, e1):
            it, chain, final_slot, stop, out = (int(x) for x in t["entry"][e])
            sf, su, sw = t["slot_f"][e], t["slot_u"][e], t["slot_w"][e]
            who = f"entry {e} (iteration {it}, chain {chain}, plane {out if out >= 0 else 'none'})"
            if not (0 <= stop <= 4 and 0 <= final_slot <= 3 and stop >= 1):
                raise AuditError(0, f"{who}: final slot {final_slot} / stop {stop} out of range")
            kmax = min(stop, 3)
            errs = [int(su[k, 2]) for k in range(kmax + 1)]
            if not np.array_equal(sf[0, :3].view(np.uint32), t["cand"][e, :3].view(np.uint32)) or sf[0, 6] != t["cand"][e, 3] \
                    or not np.array_equal(sf[0, 3:6], t["cand"][e, 4:7]):
                raise AuditError(0, f"{who}: slot 0 is not the hypothesis")
            lists, kepts = [], []
            for k in range(kmax + 1):
                where = f"{who}, slot {k}"
                rep["slots"] += 1
                nk, pk, dk = sf[k, :3], sf[k, 3:6], sf[k, 6]
                if errs[k]:
                    if su[k, 0] or su[k, 1]:
                        raise AuditError(2, f"{where}: a slot without a plane (err {errs[k]}) has a list")
                    lists.append(np.zeros(0, np.int32)); kepts.append(np.zeros(0, np.int32))
                    continue
                # ---- step 5: the plane of a refit slot
                if k >= 1:
                    prev = kepts[k - 1]
                    if len(prev) < 3:
                        raise AuditError(5, f"{where}: refit of {len(prev)} points")
                    if dk != dot3_f32(pk, nk):
                        raise AuditError(5, f"{where}: dist {dk!r} is not pos . n = {dot3_f32(pk, nk)!r}")
                    rep["refits"] += 1
                    rf = oracle.ls_fit(cloud, prev)
                    sgn = F(1) if float(nk @ rf[:3]) >= 0 else F(-1)
                    dn = float(np.abs(sgn * nk - rf[:3]).max())
                    dm = float(np.abs(pk - rf[3:6]).max())
                    mean64, v64, gap = fit_fp64(cloud, prev)
                    pos_ulp = float((np.abs(pk.astype(np.float64) - mean64.astype(F).astype(np.float64)) / _ulp(mean64.astype(F))).max())
                    if pos_ulp > 1.0:
                        raise AuditError(5, f"{where}: pos {pk} is {pos_ulp:.2f} ulp from the fp64 mean {mean64} of slot {k - 1}'s {len(prev)} kept points")
                    long_list = 4 * ORACLE_SUM_SIGMA * float(np.abs(mean64).max()) * np.sqrt(len(prev)) > MEAN_ORACLE_TOL
                    mean_tol = MEAN_ORACLE_TOL_LONG if long_list else MEAN_ORACLE_TOL
                    if dn > NORMAL_ORACLE_TOL or dm > mean_tol:
                        msg = (f"{where}: plane is not the LS fit of slot {k - 1}'s {len(prev)} kept points: normal off by {dn:.3e} "
                               f"(bound {NORMAL_ORACLE_TOL}), mean off by {dm:.3e} (bound {mean_tol}) against the oracle; "
                               f"pos is {pos_ulp:.2f} ulp from the fp64 mean, max |coordinate| {float(np.abs(cloud[prev, :3]).max()):.1f}")
                        # a plane this far from a refit of the kept points is another plane; closer, the walk may go on
                        if collect_oracle_misses and dn <= 10 * NORMAL_ORACLE_TOL and dm <= MEAN_ORACLE_TOL_LONG:
                            rep["oracle_misses"].append(msg)
                        else:
                            raise AuditError(5, msg)
                    rep["worst_pos_ulp"] = max(rep["worst_pos_ulp"], pos_ulp)
                    rep["worst_n_oracle"] = max(rep["worst_n_oracle"], dn)
                    rep["worst_mean_oracle"] = max(rep["worst_mean_oracle"], dm)
                    if gap >= GAP_REL * scale * scale:
                        v32 = v64.astype(F)
                        if float(nk.astype(np.float64) @ v64) < 0:
                            v32 = -v32
                        d64 = float(np.abs(nk - v32).max())
                        if d64 > NORMAL_FP64_TOL:
                            raise AuditError(5, f"{where}: normal {nk} is {d64:.3e} from the fp64 eigenvector {v32} (bound {NORMAL_FP64_TOL}, "
                                                f"eigenvalue gap {gap:.3e})")
                        rep["worst_n_fp64"] = max(rep["worst_n_fp64"], d64)
                    else:
                        rep["refits_small_gap"] += 1
                    if su[k, 3] and not np.array_equal(sf[k].view(np.uint32), sf[k - 1].view(np.uint32)):
                        raise AuditError(5, f"{where}: flagged converged, but its plane is not slot {k - 1}'s")
                # ---- steps 1 / 2: the score list
                lst = np.sort(oracle.score_plane(cloud, assigned, np.array([nk[0], nk[1], nk[2], dk], F), eps3, cos_t))
                if len(lst) != int(su[k, 0]):
                    raise AuditError(1 if k == 0 else 2, f"{where}: score list has {len(lst)} points on the CPU, n_list = {int(su[k, 0])}")
                # ---- step 3: the largest connected component
                kept = np.sort(oracle.connected_component(cloud, nk, pk, lst, bitmap_eps, True)) if len(lst) else lst
                if len(kept) != int(su[k, 1]):
                    raise AuditError(3, f"{where}: connected component keeps {len(kept)} of {len(lst)} points on the CPU, n_kept = {int(su[k, 1])}")
                # ---- step 6: the weighted score
                wref = float(oracle.weighted_score(cloud, nk, pk, kept, eps3)) if len(kept) else 0.0
                wrel = abs(float(sw[k]) - wref) / max(1.0, wref)
                if not wrel <= WSCORE_TOL:
                    raise AuditError(6, f"{where}: wscore {float(sw[k])!r}, the oracle's weighted score of the kept points is {wref!r}")
                rep["worst_wscore_rel"] = max(rep["worst_wscore_rel"], wrel)
                rep["max_list"] = max(rep["max_list"], len(lst))
                lists.append(lst); kepts.append(kept)
            # ---- step 7: final slot and stop index from the GPU's own numbers
            full_kept = [int(su[k, 1]) if k <= kmax else 0 for k in range(4)]
            full_w = [float(sw[k]) if k <= kmax else 0.0 for k in range(4)]
            full_err = [int(su[k, 2]) if k <= kmax else 0 for k in range(4)]
            want_final, want_stop = refit_rule(full_kept, full_w, full_err, min_support)
            if (want_final, want_stop) != (final_slot, stop):
                raise AuditError(7, f"{who}: final slot {final_slot} / stop {stop}, the refit rule on the slots' n_kept {full_kept[:kmax + 1]} and "
                                    f"wscore {full_w[:kmax + 1]} gives {want_final} / {want_stop}")
            rep["max_final_slot"] = max(rep["max_final_slot"], final_slot)
            final_kept = kepts[final_slot]
            # ---- step 8: the output plane
            if len(final_kept) >= min_support and len(final_kept) > 0:
                if out != next_plane:
                    raise AuditError(8, f"{who}: {len(final_kept)} points >= min_support {min_support}: expected as plane {next_plane} of the output")
                want = output_plane(sf[final_slot, :3], sf[final_slot, 3:6])
                if orient:
                    s = float(cloud[final_kept, 3:].astype(np.float64).sum(0) @ want[:3].astype(np.float64))
                    if abs(s) <= ORIENT_TIE * len(final_kept):
                        rep["orient_ties"] += 1
                        if np.array_equal(np.abs(want), np.abs(coef[out])) and not np.array_equal(want, coef[out]):
                            want = -want
                    elif s < 0:
                        want = -want
                if not np.array_equal(want.view(np.uint32), coef[out].view(np.uint32)):
                    raise AuditError(8, f"{who}: coefficients {coef[out].tolist()} are not the final slot {final_slot}'s plane {want.tolist()}")
                # ---- step 4: the plane's points
                got = np.sort(idx[offsets[out]:offsets[out + 1]])
                if not np.array_equal(got, final_kept):
                    only_gpu = np.setdiff1d(got, final_kept)
                    only_cpu = np.setdiff1d(final_kept, got)
                    raise AuditError(4, f"{who}: index list ({len(got)}) is not the final slot {final_slot}'s component ({len(final_kept)}): "
                                        f"{len(only_gpu)} only in the output {only_gpu[:5].tolist()}, {len(only_cpu)} only on the CPU {only_cpu[:5].tolist()}")
                next_plane += 1
                rep["planes"] += 1
            else:
                if out != -1:
                    raise AuditError(8, f"{who}: {len(final_kept)} points < min_support {min_support}, but the trace names plane {out}")
                rep["below_min_support"] += 1
            batch.append((e, who, kmax, errs, lists, final_kept, out))
        # ---- step 9: one by one, best first, against the assignment as it grows
        for e, who, kmax, errs, lists, final_kept, out in batch:
            again = _chain_lists(cloud, assigned, t["slot_f"][e], kmax, errs, eps3, cos_t, oracle)
            for k in range(kmax + 1):
                if not np.array_equal(again[k], lists[k]):
                    raise AuditError(9, f"{who}, slot {k}: accepted one by one its score list has {len(again[k])} points, in the batch {len(lists[k])}: "
                                        f"the chains of iteration {its[e0]} are not disjoint")
            if np.any(assigned[final_kept] != -1):
                raise AuditError(10, f"{who}: takes points that are already assigned")
            assigned[final_kept] = e
            taken_total += len(final_kept)
        e0 = e1
    # ---- step 10: bookkeeping
    if next_plane != P:
        raise AuditError(8, f"the output holds {P} planes, the trace accounts for {next_plane}")
    if n - taken_total != n_remaining:
        raise AuditError(10, f"n - sum of the final slots' n_kept = {n - taken_total}, the call reports n_remaining = {n_remaining}")
    if len(np.unique(idx)) != len(idx):
        raise AuditError(10, "an index appears in more than one plane")
    implied = np.full(n, -1, np.int32)
    outs = t["entry"][:, 4]
    for e in range(E):
        if outs[e] >= 0:
            implied[idx[offsets[outs[e]]:offsets[outs[e] + 1]]] = e
    mask = np.isin(assigned, np.nonzero(outs >= 0)[0]) if E else np.zeros(n, bool)
    if not np.array_equal(np.where(mask, assigned, -1), implied):
        raise AuditError(10, "the assignment at the end of the replay is not the one the output implies")
    if rep["refits"] and rep["refits_small_gap"] > MAX_SKIPPED * rep["refits"]:
        raise AuditError(5, f"{rep['refits_small_gap']} of {rep['refits']} refits have an eigenvalue gap below {GAP_REL} scale^2: too many to skip")
    return rep


# ------------------------------------------------------------------------------------------------------------------
def drive(cloud, hypotheses, oracle, min_support, dist_rel=0.005, bitmap_rel=0.02, cos_t=0.8, orient=0, batch=4):
    """The acceptance semantics of the extraction loop, sequentially and with the oracle, on caller-given hypotheses
    (K x 9: three points each).  Every `batch` hypotheses form an iteration: their chains are computed against the same
    assignment and a chain whose lists touch those of a better chain of its iteration is dropped (the library defers it).
    The LS fit is the plain fp64 one, rounded once.  Returns (trace, (coef, offsets, idx))."""
    cloud = np.ascontiguousarray(cloud, F)
    n = len(cloud)
    scale = F(oracle.cloud_scale(cloud))
    eps, bitmap_eps, cos_t = F(F(dist_rel) * scale), F(F(bitmap_rel) * scale), F(cos_t)
    eps3 = F(F(3) * eps)
    assigned = np.full(n, -1, np.int32)
    ent, cand, slot_f, slot_u, slot_w, coef, offsets, idx = [], [], [], [], [], [], [0], []
    n_deferred = 0
    remaining = n
    hyps = np.asarray(hypotheses, F).reshape(-1, 9)
    it = 0
    for h0 in range(0, len(hyps), batch):
        touched = np.zeros(n, bool)
        accepted = []
        for chain, tri in enumerate(hyps[h0:h0 + batch]):
            ok, pl = oracle.plane_from_points(tri)
            if not ok:
                continue
            sf, su, sw = np.zeros((4, 7), F), np.zeros((4, 4), np.uint32), np.zeros(4, np.float64)
            sf[0, :3], sf[0, 3:6], sf[0, 6] = pl[:3], tri[:3], pl[3]
            kepts, used = [], []
            stop = 4
            for k in range(4):
                if k >= 1:
                    if len(kepts[k - 1]) < 3:
                        su[k, 2] = 2
                        stop = k
                        break
                    mean64, v64, _ = fit_fp64(cloud, kepts[k - 1])
                    sf[k, :3], sf[k, 3:6] = v64.astype(F), mean64.astype(F)
                    sf[k, 6] = dot3_f32(sf[k, 3:6], sf[k, :3])
                lst = oracle.score_plane(cloud, assigned, np.array([*sf[k, :3], sf[k, 6]], F), eps3, cos_t)
                kept = np.sort(oracle.connected_component(cloud, sf[k, :3], sf[k, 3:6], lst, bitmap_eps, True)) if len(lst) else lst
                su[k, 0], su[k, 1] = len(lst), len(kept)
                sw[k] = float(oracle.weighted_score(cloud, sf[k, :3], sf[k, 3:6], kept, eps3)) if len(kept) else 0.0
                kepts.append(kept); used.append(lst)
                if k >= 1 and not sw[k] > sw[k - 1]:
                    stop = k
                    break
            final_slot, stop2 = refit_rule([int(su[k, 1]) for k in range(4)], sw, [int(su[k, 2]) for k in range(4)], min_support)
            assert stop2 == stop
            if any(touched[l].any() for l in used):
                n_deferred += 1
                continue
            for l in used:
                touched[l] = True
            accepted.append((chain, final_slot, stop, tri, sf, su, sw, kepts[final_slot]))
        for chain, final_slot, stop, tri, sf, su, sw, kept in accepted:
            out = -1
            if len(kept) >= min_support and len(kept):
                c = output_plane(sf[final_slot, :3], sf[final_slot, 3:6])
                if orient and float(cloud[kept, 3:].astype(np.float64).sum(0) @ c[:3].astype(np.float64)) < 0:
                    c = -c
                out = len(coef)
                coef.append(c); idx.extend(kept.tolist()); offsets.append(len(idx))
            assigned[kept] = len(ent)
            remaining -= len(kept)
            ent.append([it, chain, final_slot, stop, out])
            cand.append([*sf[0, :3], sf[0, 6], *tri[:3], 0.0])
            slot_f.append(sf); slot_u.append(su); slot_w.append(sw)
        it += 1
    E = len(ent)
    trace = normalise_trace({
        "call_u": np.array([n, min_support, orient, max(it, 1), remaining, n_deferred, E, len(coef)], np.uint32),
        "call_f": np.array([eps, eps3, bitmap_eps, cos_t], F), "entry": np.array(ent, np.int32).reshape(E, 5),
        "cand": np.array(cand, F).reshape(E, 8), "slot_f": np.array(slot_f, F).reshape(E, 4, 7),
        "slot_u": np.array(slot_u, np.uint32).reshape(E, 4, 4), "slot_w": np.array(slot_w, np.float64).reshape(E, 4)})
    return trace, (np.array(coef, F).reshape(-1, 4), np.array(offsets, np.int32), np.array(idx, np.int32))
