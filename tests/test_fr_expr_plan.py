"""csrc/fr_expr_plan.h on its own: tests/cpp/fr_expr_plan_main.cpp -- a stand-alone program that includes nothing but that header --
built with host clang++ -fsanitize=address,undefined -fno-sanitize-recover and run directly.  It hands frx_prog_build one program per
rule of the program format (each refused with a text that names the instruction), a few thousand seeded random valid programs at the
limit sizes, each then broken at one instruction, and sweeps the launch plan over log_n 0..28 x n_regs 1..8 (the grid covers N exactly,
LDS within a CU).  Nothing here is loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SRC = os.path.join(ROOT, "tests", "cpp", "fr_expr_plan_main.cpp")
CSRC = os.path.join(ROOT, "bls12_381_amd", "csrc")
HDRS = [os.path.join(CSRC, "fr_expr_plan.h")]
EXE = os.path.join(ROOT, "build", "fr_expr_plan_main")


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
    for part in ("rules", "programs", "plans"):
        assert part in lines, "the program did not reach '%s':\n%s" % (part, p.stdout)
    assert p.stdout.strip().endswith("all ok")
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
