"""The owner of a tool's work area in a context (plade::WorkSlot and work_in of plade_amd/csrc/work_slot.h), no GPU, through a
stand-alone program built with the address and undefined-behaviour sanitizers (tests/cxx/work_slot_harness.cpp): a slot creates on
first use only and returns the same object afterwards, deletes exactly once on reset() and not again on destruction, two slots of one
type (the two refinements) are independent, and a slot that was never used destroys cleanly."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKS = ["a new slot holds nothing", "first use creates", "later uses return the same object", "reset deletes once",
          "reset is idempotent", "destruction after reset deletes nothing", "a reset slot creates afresh",
          "destruction deletes what reset did not", "two slots of one type hold two objects", "each slot keeps its own",
          "resetting one leaves the other", "both are gone at the end", "a slot that was never used destroys cleanly",
          "each type is deleted by its own deleter"]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("work_slot") / "work_slot_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "plade_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "work_slot_harness.cpp"), "-o", exe])
    return exe


def test_slot_lifetime(harness):
    r = subprocess.run([harness], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.split("\n") == ["ok " + c for c in CHECKS] + [""]


def test_the_context_holds_slots_and_resets_them_before_its_stream_goes():
    csrc = os.path.join(ROOT, "plade_amd", "csrc")
    ctx, api = open(os.path.join(csrc, "ctx.h")).read(), open(os.path.join(csrc, "api.hip")).read()
    slot = open(os.path.join(csrc, "work_slot.h")).read()
    assert "#include" not in slot                       # stands alone: no HIP, no project header
    assert '#include "work_slot.h"' in ctx
    # every slot the context declares is in the one reset, which runs after the stream's wait and before its destruction
    decl = ctx[ctx.index("plade::WorkSlot normals_work"):]
    names = [n.strip() for n in decl[len("plade::WorkSlot "):decl.index(";")].replace("\n", " ").split(",")]
    assert len(names) == 14 and len(set(names)) == 14
    body = ctx[ctx.index("void reset_tool_work()"):]
    body = body[:body.index("s->reset();")]
    reset = body[body.index("{&") + 1:body.index("})")].replace("\n", " ").replace(" ", "").split(",")
    assert sorted(n[1:] for n in reset) == sorted(names)
    d = api[api.index('extern "C" void plade_ctx_destroy'):]
    assert d.index("hipStreamSynchronize(ctx->stream)") < d.index("ctx->reset_tool_work();") < d.index("hipStreamDestroy(ctx->stream)")
    assert d.index("hipSetDevice(ctx->device)") < d.index("ctx->reset_tool_work();")
