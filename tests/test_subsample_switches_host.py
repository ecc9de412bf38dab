"""The parsers of PLADE_SUBSAMPLE and PLADE_M3C2_CORE (plade_amd/csrc/cli_switches.h), no GPU, through a stand-alone program built
with the address and undefined-behaviour sanitizers (tests/cxx/subsample_switch_harness.cpp): the accepted forms, the defaults, and
the rejected values with the exact warning."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAIL = {"PLADE_SUBSAMPLE": " is not <spacing>[,<seed>] with spacing >= 0 (its square not below FLT_MIN) and seed an integer >= 0; no subsampling",
        "PLADE_M3C2_CORE": " is not <spacing>[,<seed>] with spacing >= 0 (its square not below FLT_MIN) and seed an integer >= 0;"
                           " the whole target as core points"}
OFF = (0.0, 0)
# (text, (spacing, seed) or None when the value is rejected)
VALUES = [(None, OFF), ("0.25", (0.25, 0)), ("0.25,7", (0.25, 7)), (" +5e-1,+12", (0.5, 12)), ("0x1p-2,9223372036854775807", (0.25, (1 << 63) - 1)),
          ("0", OFF), ("0,3", (0.0, 3)), ("-0", OFF), ("1e-18", (1e-18, 0)),
          ("", None), ("wide", None), ("0.25,", None), ("0.25,,1", None), ("0.25,5.0", None), ("0.25,-1", None), ("0.25,7,1", None),
          ("0.25x", None), ("inf", None), ("nan", None), ("-0.25", None), ("1e30", None), ("1e-30", None)]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("subsample_switches") / "subsample_switch_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "plade_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "subsample_switch_harness.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("var", sorted(TAIL))
def test_values(harness, var):
    feed = "".join(var + ("" if text is None else "\t" + text) + "\n" for text, _ in VALUES)
    r = subprocess.run([harness], input=feed, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    got = r.stdout.split("\n")
    assert got[-1] == "" and len(got) == len(VALUES) + 1
    for (text, want), line in zip(VALUES, got):
        fields, warning = line.split("\t")
        spacing, seed = fields.split(" ")
        if want is None:                                           # rejected: the switch's "off" and the one warning
            assert (float.fromhex(spacing), int(seed)) == OFF and warning == f"warning: {var}={text}{TAIL[var]}", (text, line)
        else:
            assert (float.fromhex(spacing), int(seed)) == want and warning == "", (text, line)


def test_the_two_switches_are_documented_at_their_latches():
    host = open(os.path.join(ROOT, "plade_amd", "csrc", "plade_host.cpp")).read()
    for var, parser in (("PLADE_SUBSAMPLE", "parse_subsample"), ("PLADE_M3C2_CORE", "parse_m3c2_core")):
        assert host.count(f'getenv("{var}")') == 1 and host.count(f"cli_switches::{parser}(") == 1 and f"// {var}=<spacing>[,<seed>]" in host
