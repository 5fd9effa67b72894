"""csrc/fr_lagrange_plan.h on its own: tests/cpp/fr_lagrange_plan_main.cpp -- a stand-alone program that includes nothing but that header
-- built with host clang++ -fsanitize=address,undefined -fno-sanitize-recover and run directly.  It walks the launch of the Lagrange
coefficients as a model, with the teams, the lanes' nodes, the passes and the tiles read through the header's functions as the kernel
reads them, in both shapes at tiny and at the shipped sizes, for nseg in {0, 1, 2, 1000} against segment lengths all 0 / all 1 /
tile - 1 / tile / tile + 1 / 4096 and random mixes: every segment meets one team, every node one lane, every (node, tile) pair is
visited once, the LDS and the scratch the plan reserves are never exceeded, the device form's bad segments are refused by the one
function that reads the offsets.  Then one call per refusal of the argument checks, 64-bit extremes included.
Nothing here is loaded into Python."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SRC = os.path.join(ROOT, "tests", "cpp", "fr_lagrange_plan_main.cpp")
CSRC = os.path.join(ROOT, "bls12_381_amd", "csrc")
HDRS = [os.path.join(CSRC, "fr_lagrange_plan.h")]
EXE = os.path.join(ROOT, "build", "fr_lagrange_plan_main")


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
    """the limits the public header states are the plan's, and the status bit is the next free one: no other sticky flag uses it"""
    plan = open(HDRS[0]).read()
    pub = open(os.path.join(ROOT, "include", "bls12_381_hip.h")).read()
    ctx = open(os.path.join(CSRC, "api_ctx.hip")).read()
    assert "FLG_LEN_MAX = 4096" in plan and "FLG_MAX_TOTAL = (size_t)1 << 27" in plan and "FLG_MAX_SEGS = (size_t)1 << 27" in plan
    assert re.search(r"#define BLSGPU_FR_LAGRANGE_LEN_MAX 4096\b", pub) and re.search(r"#define BLSGPU_SEG_LEN_MAX 4096\b", pub)
    doc = pub[pub.index("Lagrange coefficients at ARBITRARY nodes"):pub.index("int blsgpu_fr_lagrange_segments(")]
    assert "total <= 2^27" in doc and "nseg <= 2^27" in doc and "t_s <= BLSGPU_FR_LAGRANGE_LEN_MAX" in doc
    bit = int(re.search(r"FLG_STATUS_BAD = (\d+)u", plan).group(1))
    assert bit == 32 and "st & FLG_STATUS_BAD" in ctx
    assert not re.search(r"st & %du\b" % bit, ctx), "another flag already uses that bit"
    others = {int(m) for f in os.listdir(CSRC) if f != "fr_lagrange_plan.h" for m in re.findall(r"_STATUS_BAD = (\d+)u", open(os.path.join(CSRC, f)).read())}
    others |= {int(m) for m in re.findall(r"st & (\d+)u", ctx)}
    assert others == {2, 4, 8, 16} and bit == 2 * max(others), others
