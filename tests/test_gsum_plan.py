"""csrc/gsum_plan.h on its own: tests/cpp/gsum_plan_main.cpp -- a stand-alone program that includes nothing but that header -- built with
host clang++ -fsanitize=address,undefined -fno-sanitize-recover and run directly.  It runs the two passes of the segmented point sums as
a model over integers, with the cut, the destinations and the jobs read through the header's functions as the kernels read them, at
tiny and at the shipped chunk sizes, for nseg in {0, 1, 2, 1000} against segment lengths all 0 / all 1 / chunk - 1 / chunk / chunk + 1,
one segment holding everything, a long segment first / in the middle / last among short ones, and random mixes: every term is added
once, every segment is written once and right, every partial record of a multi-chunk segment is read by exactly one job, the scratch
the plan reserves is never exceeded.  Then one call per refusal of the argument checks, 64-bit extremes of the offsets included.
Nothing here is loaded into Python."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SRC = os.path.join(ROOT, "tests", "cpp", "gsum_plan_main.cpp")
CSRC = os.path.join(ROOT, "bls12_381_amd", "csrc")
HDRS = [os.path.join(CSRC, "gsum_plan.h")]
EXE = os.path.join(ROOT, "build", "gsum_plan_main")


@pytest.fixture(scope="module")
def program():
    if not os.path.exists(CLANG):
        pytest.skip("no host clang++ in this image")
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(f) for f in [SRC] + HDRS):
        tmp = EXE + ".tmp%d" % os.getpid()
        subprocess.check_call([CLANG, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-iquote", CSRC, SRC, "-o", tmp])
        os.replace(tmp, EXE)
    return EXE


def test_plan_program_runs_clean(program):
    """the whole program under the address and undefined-behaviour sanitizers: every check passes and nothing is reported"""
    p = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, "exit status %d\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    lines = p.stdout.split()
    for part in ("plans", "refusals"):
        assert part in lines, "the program did not reach '%s':\n%s" % (part, p.stdout)
    assert p.stdout.strip().endswith("all ok")
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]


def test_the_published_limits_match_the_plan():
    """the limits the public header states are the plan's, and the status bit is one the other sticky flags do not use"""
    plan = open(HDRS[0]).read()
    pub = open(os.path.join(ROOT, "include", "bls12_381_hip.h")).read()
    ctx = open(os.path.join(CSRC, "api_ctx.hip")).read()
    assert "GSUM_MAX_TOTAL = (size_t)1 << 28" in plan and "GSUM_MAX_POINTS = (uint64_t)1 << 32" in plan
    doc = pub[pub.index("Segmented, gathered sums"):pub.index("int blsgpu_g1_sum_segments(")]
    assert "total > 2^28" in doc and "npoints >= 2^32" in doc
    bit = int(re.search(r"GSUM_STATUS_BAD = (\d+)u", plan).group(1))
    assert bit == 16 and "st & GSUM_STATUS_BAD" in ctx
    assert not re.search(r"st & %du\b" % bit, ctx), "another flag already uses that bit"
