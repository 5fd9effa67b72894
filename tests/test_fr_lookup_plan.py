"""csrc/fr_lookup_plan.h on its own: tests/cpp/fr_lookup_plan_main.cpp -- a stand-alone program that includes nothing but that header --
built with host clang++ -fsanitize=address,undefined -fno-sanitize-recover and run directly.  It sweeps the launch plan over rows
1 .. 2^24 at the powers of two and +-1 (slots a power of two >= 2 rows, LDS within 64 KB, the counting path flipping exactly at
BLSGPU_FR_LOOKUP_LDS_ROWS, the grids covering n exactly for n in {0, 1, block +- 1, 2^28}), hands the argument checks one call per
refusal, and holds the key hash to its property (keys differing in a single word: at most 1 collision in 10^5 pairs).  Nothing here is
loaded into Python."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SRC = os.path.join(ROOT, "tests", "cpp", "fr_lookup_plan_main.cpp")
CSRC = os.path.join(ROOT, "bls12_381_amd", "csrc")
HDRS = [os.path.join(CSRC, "fr_lookup_plan.h")]
EXE = os.path.join(ROOT, "build", "fr_lookup_plan_main")


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
    for part in ("plans", "refusals", "hash"):
        assert part in lines, "the program did not reach '%s':\n%s" % (part, p.stdout)
    assert p.stdout.strip().endswith("all ok")
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]


def test_the_published_constants_match_the_plan():
    """BLSGPU_FR_LOOKUP_LDS_ROWS of the public header, FRL_LDS_ROWS of the plan and the Python mirrors are one number; likewise the sentinel"""
    import fr_lookup_ref as ref
    plan = open(HDRS[0]).read()
    pub = open(os.path.join(ROOT, "include", "bls12_381_hip.h")).read()
    api = open(os.path.join(ROOT, "bls12_381_amd", "api.py")).read()
    lds = int(re.search(r"constexpr size_t FRL_LDS_ROWS = (\d+);", plan).group(1))
    assert int(re.search(r"#define BLSGPU_FR_LOOKUP_LDS_ROWS (\d+)", pub).group(1)) == lds == ref.LDS_ROWS
    assert int(re.search(r"FR_LOOKUP_LDS_ROWS, FR_LOOKUP_MISS = (\d+), 0xFFFFFFFF", api).group(1)) == lds
    assert "#define BLSGPU_FR_LOOKUP_MISS     0xFFFFFFFFu" in pub and "FRL_MISS = 0xffffffffu" in plan and ref.MISS == 0xFFFFFFFF
    assert int(re.search(r"constexpr int FRL_BLOCK = (\d+);", plan).group(1)) == ref.BLOCK
