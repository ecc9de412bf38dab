"""The list-valued switches of the CLI (plade_amd/csrc/cli_switches.h), no GPU: the one parser and its predicates against the table
recorded from the hand-written parsers they replace (tests/switch_cases.py), through a stand-alone program built with the address
and undefined-behaviour sanitizers (tests/cxx/switch_harness.cpp); and the three switches that are read while a file loads, before
any GPU context, through the real CLI."""
import os
import subprocess

import numpy as np
import pytest

from switch_cases import ARITY, CASES
from test_normals_host import CLI, PARENT_RESULT, _write, _xyz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _accepted(case):
    return case[3] == ""


def test_the_table_cannot_pass_vacuously():
    """Every variable has an accepted value of every length it allows, and for every field a rejected value that differs from an
    accepted one in that field alone."""
    assert len(ARITY) == 10 and {c[0] for c in CASES} == set(ARITY)
    assert len({c[:2] for c in CASES}) == len(CASES)
    for var, (required, n) in ARITY.items():
        assert [c for c in CASES if c[:2] == (var, None)] and all(_accepted(c) for c in CASES if c[1] is None), var   # unset: no warning
        mine = [c for c in CASES if c[0] == var and c[1] is not None]
        good = {tuple(c[1].split(",")) for c in mine if _accepted(c)}
        bad = {tuple(c[1].split(",")) for c in mine if not _accepted(c)}
        assert {len(g) for g in good} == set(range(required, n + 1)), var
        for k in range(n):
            assert any(len(b) == len(g) and [i for i in range(len(b)) if b[i] != g[i]] == [k] for b in bad for g in good), (var, k)
        assert any(",," in c[1] for c in mine), var
        for c in mine:
            assert _accepted(c) or (c[3].startswith(f"warning: {var}={c[1]} is not ") and c[3].count("\n") == 1 and c[3][-1] == "\n"), c


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("switches") / "switch_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "plade_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "switch_harness.cpp"), "-o", exe])
    return exe


def test_the_parser_is_the_hand_written_parsers(harness):
    """Bit for bit on the fields, byte for byte on the warnings, all rows in one process (nothing is latched in the header)."""
    feed = "".join(var + ("" if text is None else "\t" + text) + "\n" for var, text, _, _ in CASES)
    r = subprocess.run([harness], input=feed, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    got = r.stdout.split("\n")
    assert got[-1] == "" and len(got) == len(CASES) + 1
    for (var, text, fields, warning), line in zip(CASES, got):
        assert line + "\n" == fields + "\t" + (warning or "\n"), (var, text)


def test_only_the_cli_layer_includes_the_header():
    csrc = os.path.join(ROOT, "plade_amd", "csrc")
    users = [f for f in sorted(os.listdir(csrc)) if '#include "cli_switches.h"' in open(os.path.join(csrc, f), errors="replace").read()]
    assert users == ["plade_host.cpp"]


BAD = {"PLADE_REMOVE_OUTLIERS": "65", "PLADE_KEEP_COMPONENTS": "0.25,0,2", "PLADE_SMOOTH": "0.25,2"}   # rows of the table


@pytest.mark.parametrize("var", sorted(BAD))
def test_cli_with_a_bad_load_time_switch_warns_once_and_is_the_parents(tmp_path, var):
    """A target with normals passes the filters (the switch is read there, and a rejected value is "off": no GPU context), then the
    source without normals fails the load as it did before the header existed."""
    pt, ps, res = str(tmp_path / "t.ply"), str(tmp_path / "s.ply"), str(tmp_path / "r.txt")
    rows = _xyz(100, seed=1)
    rows = np.concatenate([rows, rows / np.linalg.norm(rows, axis=1, keepdims=True)], axis=1).astype(np.float32)
    with open(pt, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex 100\n"
                 + "".join(f"property float {c}\n" for c in ("x", "y", "z", "nx", "ny", "nz")) + "end_header\n").encode())
        f.write(rows.tobytes())
    _write(ps, _xyz(100, seed=2), "binary_little_endian", np.float32)
    env = {k: v for k, v in os.environ.items() if not k.startswith("PLADE_")}
    warning = next(c[3] for c in CASES if c[:2] == (var, BAD[var]))
    parent = "the number of points does not equal to the number of normals in the file\nloading source point cloud failed\n"
    for extra, stderr in (({}, parent), ({var: BAD[var]}, warning + parent)):
        r = subprocess.run([CLI, pt, ps, res], capture_output=True, text=True, timeout=120, env=dict(env, **extra))
        assert (r.returncode, r.stdout, r.stderr) == (1, f"target file: {pt}\nsource file: {ps}\n", stderr), extra
        assert open(res).read() == PARENT_RESULT
