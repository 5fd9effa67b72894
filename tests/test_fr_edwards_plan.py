"""csrc/fr_edwards_plan.h on its own: tests/cpp/fr_edwards_plan_main.cpp -- a stand-alone program that includes nothing but that header
(and the plan headers it includes) -- built with host clang++ -fsanitize=address,undefined -fno-sanitize-recover and run directly.  It
sweeps the signed-window recoding over every (bits, window) in [1, 256] x [2, 8] at the edge scalars, the table layout and its byte
limit, the launch shapes with their LDS and scratch bytes, the `complete` test on the two parameter sets of the tests, and makes one
call per refusal of every argument check.  Nothing here is loaded into Python."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SRC = os.path.join(ROOT, "tests", "cpp", "fr_edwards_plan_main.cpp")
CSRC = os.path.join(ROOT, "bls12_381_amd", "csrc")
HDRS = [os.path.join(CSRC, f) for f in ("fr_edwards_plan.h", "fr_poseidon_plan.h", "gsum_plan.h")]
EXE = os.path.join(ROOT, "build", "fr_edwards_plan_main")


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
    words = p.stdout.split()
    for part in ("recoding", "tables", "plans", "complete", "refusals"):
        assert part in words, "the program did not reach '%s':\n%s" % (part, p.stdout)
    assert int(words[words.index("recoding") + 1]) == 256 * 7 * 14, "every (bits, window) with its fourteen scalars"
    assert int(words[words.index("refusals") + 1]) >= 50
    assert p.stdout.strip().endswith("all ok")
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]


def test_the_published_limits_match_the_plan():
    """the limits the public header prints are the plan's, and the status bit is one no other sticky flag uses"""
    plan = open(HDRS[0]).read()
    pub = open(os.path.join(ROOT, "include", "bls12_381_hip.h")).read()
    ctx = open(os.path.join(CSRC, "api_ctx.hip")).read()

    def plan_shift(name):
        return int(re.search(r"%s = \(size_t\)1 << (\d+);" % name, plan).group(1))

    def pub_shift(name):
        return int(re.search(r"#define %s\s+\(\(size_t\)1 << (\d+)\)" % name, pub).group(1))

    assert plan_shift("FRED_MAX_POINTS") == pub_shift("BLSGPU_FR_EDWARDS_MAX_POINTS") == 26
    assert plan_shift("FRED_MAX_TOTAL") == plan_shift("FRED_MAX_SEGS") == pub_shift("BLSGPU_FR_EDWARDS_MAX_TOTAL") == 26
    assert plan_shift("FRED_MAX_BASES") == pub_shift("BLSGPU_FR_EDWARDS_MAX_BASES") == 24
    assert plan_shift("FRED_TABLE_MAX_BYTES") == pub_shift("BLSGPU_FR_EDWARDS_TABLE_MAX_BYTES") == 31
    assert "FRED_WINDOW_MIN = 2, FRED_WINDOW_MAX = 8" in plan
    assert re.search(r"#define BLSGPU_FR_EDWARDS_WINDOW_MIN 2\b", pub) and re.search(r"#define BLSGPU_FR_EDWARDS_WINDOW_MAX 8\b", pub)
    doc = pub[pub.index("TWISTED EDWARDS GROUPS OVER Fr"):pub.index("typedef struct blsgpu_fr_edwards blsgpu_fr_edwards;")]
    for needle in ("total <= 2^26, k <= 2^26", "n <= 2^26 points", "window in [2, 8], n in [1, 2^24]", "at most 2 GiB", "`bits` in [1, 256]", "16-byte aligned", "ODD order"):
        assert needle in doc, needle
    bit = int(re.search(r"FRED_STATUS_BAD = \(uint32_t\)1 << (\d+);", plan).group(1))
    assert bit == 8 and "st & FRED_STATUS_BAD" in ctx
    others = [int(m) for m in re.findall(r"_STATUS_BAD = \(uint32_t\)1 << (\d+)", "".join(open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f != "fr_edwards_plan.h"))]
    assert bit not in others and (1 << bit) not in (2, 4, 8, 16, 32)
