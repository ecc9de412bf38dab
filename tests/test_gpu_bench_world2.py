"""bench.py's N > 1 control flow (rendezvous, barriers, max-over-ranks timing, result gather) on a one-GPU box: two
ranks share cuda:0 (PLADE_BENCH_ONE_GPU=1) and exchange over their loopback rendezvous, without torch in the ranks; and
with PLADE_BENCH_TORCH=1 over torch.distributed (gloo here: RCCL refuses two ranks on one device)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("with_torch", [False, True])
def test_bench_two_ranks_on_one_gpu(with_torch, tmp_path):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, PLADE_BENCH_ONE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("PLADE_BENCH_TORCH", None)
    if with_torch:
        env["PLADE_BENCH_TORCH"] = "1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "12", "--warmup", "4",
           "--points", "200000", "--inflight", "2", "--group", "2", "--pairs", "4", "--closed-form-steps", "8",
           "--dump-outputs", str(tmp_path / "dump"), "--full"]       # --full: the pair-alone comparison and the other legs run too
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=540, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1            # rank 0 prints the one JSON line
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["full"] is True
    assert d["torch_in_process"] == with_torch and d["rank_exchange"].startswith("torch") == with_torch
    if not with_torch:
        # RCCL is the default exchange of an N > 1 run and refuses two ranks on ONE device: the ranks agree on the fallback and say why
        assert d["rank_exchange"].startswith("loopback rendezvous") and "rccl not used" in d["rank_exchange"], d["rank_exchange"]
    timed = 12                        # exactly --steps registrations are timed
    assert d["requested_steps"] == timed and d["steps"] == timed and d["pipeline"]["timed_steps"] == timed
    assert d["pipeline"]["groups_in_flight"] == 2 and d["pipeline"]["pairs_per_group"] == 2
    assert d["registrations_timed"] == 2 * timed and d["registrations_ok"] == d["registrations_timed"]
    assert d["results_bit_identical_to_the_pair_alone_rank0"]
    assert d["value"] > 0 and d["cpu_baseline"] is None   # the CPU leg runs at N = 1 only
    # --dump-outputs: rank 0's last timed step, step 11 = pair 11 % 4 = 3 (seed 3), bit for bit what that pair registered alone
    # returns -- so both parametrisations (same arguments) write the same files
    T, ok = np.load(tmp_path / "dump" / "T.npy"), np.load(tmp_path / "dump" / "ok.npy")
    assert T.dtype == np.float32 and T.shape == (4, 4) and ok.dtype == np.float32 and ok.shape == (1,)
    ok_alone, T_alone = _seed3_alone()
    assert np.array_equal(T, np.asarray(T_alone, np.float32)) and ok[0] == (1.0 if ok_alone else 0.0)


def _seed3_alone():
    """(ok, T) of the 200 000-point pair of seed 3 registered alone, with the bench's parameters."""
    import plade_amd
    from plade_amd.synth import make_pair
    tg, sr, _ = make_pair(200000, seed=3)
    c = plade_amd.Context(0, orient_normals=1)              # the bench's parameters (conftest.ORIENTED), a context of its own
    ct, cs = c.upload(tg), c.upload(sr)
    ok_alone, T_alone = c.registration_dev(ct, cs)
    ct.free(); cs.free(); c.close()
    return ok_alone, T_alone


# what a plain run leaves to --full: these objects of the line are null without it
FULL_ONLY = ("results_bit_identical_to_the_pair_alone_rank0", "max_frobenius_vs_ground_truth_rank0", "value_by_seed",
             "parity_vs_reference_solver", "closed_form_mode_rank0", "resident_rank0", "default_mode_rank0",
             "single_registration_latency_ms", "single_registration_latency_by_scene_ms", "roofline", "roofline_sort",
             "dominant_by_gpu_time", "cpu_baseline", "cpu_baseline_batch", "cli_end_to_end")


def test_bench_plain_run_times_the_same_steps_and_leaves_the_other_legs_to_full(tmp_path):
    """Without --full a run sets up, warms up, times exactly --steps registrations, writes --dump-outputs and prints the line:
    the headline fields are there, every other leg's object is null (also where an option sizes that leg), and the dumped
    result of the last timed step (step 11 = pair 3) is bit for bit what that pair registered alone returns -- what the
    --full runs above dump for the same arguments."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "12", "--warmup", "4", "--points", "200000",
           "--inflight", "2", "--group", "2", "--pairs", "4", "--closed-form-steps", "8", "--dump-outputs", str(tmp_path / "dump")]
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ), timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["full"] is False and d["n_gpus"] == 1
    assert d["metric"] == "scan-pair registrations/sec, 1M-pt synthetic pairs" and d["unit"] == "registrations/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["steps"] == d["requested_steps"] == d["pipeline"]["timed_steps"] == 12 and d["warmup"] == 4
    assert d["value"] > 0 and abs(d["value"] * d["ms_per_step"] - 1000.0) < 1e-6 * 1000.0
    assert d["registrations_timed"] == 12 and d["registrations_ok"] == 12
    for k in FULL_ONLY:
        assert k in d and d[k] is None, k
    assert not d["kernels_profiled_step"] and not d["stage_seconds_profiled_step"]
    # every registration of the run is one of the timed pipeline's or of its warm-up: no leg registered a pair alone
    n = [int(l.rsplit(":", 1)[1]) for l in r.stderr.splitlines() if l.startswith("[bench] registrations executed by rank 0:")]
    lead, tail = d["pipeline"]["lead_in_steps"], d["pipeline"]["tail_steps"]
    assert n == [2 * (2 + 2) * 2 + lead + 12 + tail], (n, lead, tail)     # warm-up: 2 contexts x (2 + 2) group compositions x 2 pairs
    T, ok = np.load(tmp_path / "dump" / "T.npy"), np.load(tmp_path / "dump" / "ok.npy")
    assert T.dtype == np.float32 and T.shape == (4, 4) and ok.dtype == np.float32 and ok.shape == (1,)
    ok_alone, T_alone = _seed3_alone()
    assert np.array_equal(T, np.asarray(T_alone, np.float32)) and ok[0] == (1.0 if ok_alone else 0.0)


def test_bench_four_ranks_on_one_gpu():
    """The control flow of an N > 2 run -- four ranks of `torch.distributed.run`, their rendezvous, the barriers around the timed
    region, max-over-ranks timing, the result gather of every rank's pairs in input order, the groups-in-flight choice from the
    CPU quota shared by the ranks -- once, somewhere: all four ranks on the ONE GPU of this box, small clouds.  (Four, not the
    eight of a full node: with this test's own process that keeps at most 5 processes on one GPU.)  --steps 7 with groups of 2
    also times a last group of one pair."""
    import bench
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, PLADE_BENCH_ONE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("PLADE_BENCH_TORCH", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "4", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "7", "--warmup", "2",
           "--points", "60000", "--group", "2", "--pairs", "2", "--closed-form-steps", "0", "--resident-steps", "4", "--full"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 4 and d["scaling"] == "weak" and not d["torch_in_process"] and d["full"] is True
    assert d["rank_exchange"].startswith("loopback rendezvous") and "rccl not used" in d["rank_exchange"], d["rank_exchange"]
    M = d["pipeline"]["groups_in_flight"]
    assert M == bench.inflight_for_budget(bench._cpu_budget(), 4) >= 1 and d["config"]["inflight_chosen_from_cpu_quota"]   # the quota the four ranks share
    timed = 7
    assert d["steps"] == d["requested_steps"] == timed and d["registrations_timed"] == 4 * timed
    assert 0 < d["registrations_ok"] <= d["registrations_timed"]      # (a 60 000-point scene may fail to register: that is a result, not an error)
    assert d["results_bit_identical_to_the_pair_alone_rank0"] and d["value"] > 0
    assert d["config"]["distinct_pairs_total"] == 8 and d["cpu_baseline"] is None
