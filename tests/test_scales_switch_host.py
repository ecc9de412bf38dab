"""The parser of PLADE_M3C2_NORMALS (plade_amd/csrc/cli_switches.h), no GPU, through a stand-alone program built with the address
and undefined-behaviour sanitizers (tests/cxx/scales_switch_harness.cpp): the accepted forms of lengths 2, 3 and 4 with the radii
restated exactly (r_min + (r_max - r_min) * s / (S - 1) is the same fp64 expression here), for every field a rejected value that
differs in that field alone, r_min = r_max, steps too small for fp32, a `,,` value, and the warning byte for byte."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VAR = "PLADE_M3C2_NORMALS"
TAIL = (" is not <r_min>,<r_max>[,<scales>[,<mode>]] with 0 < r_min < r_max (the fp32 squares of the radii strictly ascending), scales in"
        " [2, 8] and mode 0 or 1; the core points keep their normals")
OFF = (0, 4, 0, [0.0] * 4)


def on(r_min, r_max, scales=4, mode=0):
    return (1, scales, mode, [r_min + (r_max - r_min) * s / (scales - 1) for s in range(scales)])


# (text, (on, scales, mode, radii) or None when the value is rejected)
VALUES = [(None, OFF),
          ("0.1,0.4", on(0.1, 0.4)), ("0.1,0.4,3", on(0.1, 0.4, 3)), ("0.1,0.4,3,1", on(0.1, 0.4, 3, 1)),        # lengths 2, 3, 4
          ("0.1,0.4,2", on(0.1, 0.4, 2)), ("0.1,0.4,8,0", on(0.1, 0.4, 8)), (" +1e-1,0x1p-1,5", on(0.1, 0.5, 5)),
          ("0.05,0.07,7,1", on(0.05, 0.07, 7, 1)),
          ("-0.1,0.4,3,1", None), ("0,0.4,3,1", None), ("nan,0.4,3,1", None), ("1e-30,0.4,3,1", None),            # r_min alone
          ("0.1,-0.4,3,1", None), ("0.1,inf,3,1", None), ("0.1,1e30,3,1", None), ("0.1,0.05,3,1", None),          # r_max alone
          ("0.1,0.4,1,1", None), ("0.1,0.4,9,1", None), ("0.1,0.4,3.0,1", None), ("0.1,0.4,x,1", None),           # scales alone
          ("0.1,0.4,3,2", None), ("0.1,0.4,3,-1", None), ("0.1,0.4,3,1.5", None),                                 # mode alone
          ("0.4,0.4", None), ("0.4,0.4,2", None),                                                                 # r_min = r_max
          ("0.4,0.40000001,8", None),                                    # ascending in fp64, the fp32 squares are not
          ("0.1,,3", None), ("0.1,0.4,,1", None), (",,", None),                                                   # `,,`
          ("", None), ("0.1", None), ("wide", None), ("0.1,0.4,", None), ("0.1,0.4,3,1,0", None), ("0.1,0.4x", None)]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("scales_switch") / "scales_switch_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "plade_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "scales_switch_harness.cpp"), "-o", exe])
    return exe


def test_values(harness):
    feed = "".join(VAR + ("" if text is None else "\t" + text) + "\n" for text, _ in VALUES)
    r = subprocess.run([harness], input=feed, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    got = r.stdout.split("\n")
    assert got[-1] == "" and len(got) == len(VALUES) + 1
    for (text, want), line in zip(VALUES, got):
        fields, warning = line.split("\t")
        w = fields.split(" ")
        have = (int(w[0]), int(w[1]), int(w[2]), [float.fromhex(x) for x in w[3:]])
        if want is None:                                           # rejected: the switch's "off" and the one warning
            assert have == OFF and warning == f"warning: {VAR}={text}{TAIL}", (text, line)
        else:
            assert have == want and warning == "", (text, line)    # the radii bit for bit
            if want[0]:
                r32 = np.asarray(have[3], np.float64).astype(np.float32)
                assert (np.diff(r32 * r32) > 0).all()


def test_the_switch_is_documented_at_its_one_latch():
    host = open(os.path.join(ROOT, "plade_amd", "csrc", "plade_host.cpp")).read()
    assert host.count(f'getenv("{VAR}")') == 1 and host.count("cli_switches::parse_m3c2_normals(") == 1
    assert f"// {VAR}=<r_min>,<r_max>[,<scales>[,<mode>]]" in host
    doc = host[host.index(f"// {VAR}="):host.index("const ScaleSwitch &m3c2_normals_switch()")]
    assert all(l.startswith("//") for l in doc.strip().split("\n")) and "PLADE_M3C2" in doc and "no axis" in doc
