"""csrc/kzg_recover_plan.h on its own: tests/cpp/kzg_recover_plan_main.cpp -- a stand-alone program that includes nothing but that header
(and kzg_plan.h, whose cell map it inverts) -- built with host clang++ -fsanitize=address,undefined -fno-sanitize-recover and run
directly.  For every (log_n <= 8, log_l <= log_n), both orders and count in {0, 1, 3} it checks that the index map is the inverse of
kzg_cell_src and a bijection, walks the scatter's tiles, and checks that every scratch range lies inside what the plan reserves; then
the effective offsets, the host-form checks, and one call per refusal, 64-bit extremes included.  Nothing here is loaded into Python.

The maps the program prints are compared with tests/kzg_ref.py, and the limits the public header states with the plan's."""
import os
import re
import subprocess

import pytest

import kzg_ref as k
import kzg_recover_ref as rr
from oracle import bls12_381_ref as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SRC = os.path.join(ROOT, "tests", "cpp", "kzg_recover_plan_main.cpp")
CSRC = os.path.join(ROOT, "bls12_381_amd", "csrc")
HDRS = [os.path.join(CSRC, "kzg_recover_plan.h"), os.path.join(CSRC, "kzg_plan.h")]
EXE = os.path.join(ROOT, "build", "kzg_recover_plan_main")
R = o.R_ORDER


@pytest.fixture(scope="module")
def output():
    if not os.path.exists(CLANG):
        pytest.skip("no host clang++ in this image")
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(f) for f in [SRC] + HDRS):
        tmp = EXE + ".tmp%d" % os.getpid()
        subprocess.check_call([CLANG, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-iquote", CSRC, SRC, "-o", tmp])
        os.replace(tmp, EXE)
    p = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, "exit status %d\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    return p.stdout


def test_plan_program_runs_clean(output):
    """the whole program under the address and undefined-behaviour sanitizers: every check passes and nothing is reported"""
    words = output.split()
    for part in ("plans", "offsets", "refusals"):
        assert part in words, "the program did not reach '%s':\n%s" % (part, output[-2000:])
    assert int(words[words.index("refusals") + 1]) >= 35
    assert output.strip().endswith("all ok")


def test_the_maps_agree_with_the_reference(output):
    """the residue of cell i is kzg_ref.coset_shift_exponent, its entries sit at kzg_ref.cell_point_exponent, and the Python inverse map
    of tests/kzg_recover_ref.py undoes it"""
    rows = [tuple(int(x) for x in line.split()[1:]) for line in output.splitlines() if line.startswith("map ")]
    assert len(rows) == sum(2 * (2 << (n - l)) for n in range(5) for l in range(n + 1))
    for log_n, log_l, order, i, rho, last in rows:
        assert rho == k.coset_shift_exponent(i, log_n, log_l, order) == rr.residue(i, log_n, log_l, order), (log_n, log_l, order, i)
        assert last == k.cell_point_exponent(i, (1 << log_l) - 1, log_n, log_l, order)
        assert last % (2 << (log_n - log_l)) == rho
    for log_n, log_l in ((0, 0), (3, 0), (3, 3), (4, 2), (6, 1)):
        for order in (k.NATURAL, k.BITREV):
            for i in range(2 << (log_n - log_l)):
                for t in range(1 << log_l):
                    assert rr.cell_of_index(k.cell_point_exponent(i, t, log_n, log_l, order), log_n, log_l, order) == (i, t)


def test_the_published_limits_match_the_plan():
    """the limits the public header states are the plan's, and the generator is the reference's"""
    plan = open(HDRS[0]).read()
    pub = open(os.path.join(ROOT, "include", "bls12_381_hip.h")).read()
    const = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, plan).group(1))
    assert (const("KZGR_MAX_LOG_N"), const("KZGR_MAX_LOG_L"), const("KZGR_MAX_LOG_CELLS"), const("KZGR_MAX_LOG_TOTAL"), const("KZGR_MAX_LOG_M"), const("KZGR_MAX_LOG_SCALARS")) == \
        (27, 12, 12, 28, 24, 28)
    doc = pub[pub.index("KZG cell recovery: a polynomial rebuilt"):pub.index("int blsgpu_kzg_recover(")]
    for text in ("log_n in [0, 27]", "log_l in [0, min(log_n, 12)]", "log_n - log_l + 1 <= 12", "2c <= 4096", "count * 2n <= 2^28", "m <= 2^24", "m * l <= 2^28", "16-byte", "4-byte",
                 "count == 0 is a no-op", "does NOT set the\n *                 context's sticky flag", "blob in evaluation form"):
        assert text in doc, text
    for item in ("recomputing the proofs inside the call", "byte-level cells", "sharing the\n * tables between polynomials with equal patterns", "2c > 4096"):
        assert item in doc, item
    assert "KZGR_ORDER_NATURAL = 0, KZGR_ORDER_BITREV = 1" in plan and "#define BLSGPU_FR_ORDER_NATURAL 0" in pub.replace("  ", " ")
    limbs = [int(x, 16) for x in re.search(r"KZGR_GEN_MONT\[4\] = \{([^}]*)\}", plan).group(1).replace("ull", "").split(",")]
    assert limbs == o.fr_to_mont_limbs(o.FR_GENERATOR) and o.FR_GENERATOR == rr.G == 7
    status = lambda name: int(re.search(r"%s = (\d+)" % name, plan).group(1))
    assert (status("KZGR_ST_OFFSETS"), status("KZGR_ST_COL"), status("KZGR_ST_DUP"), status("KZGR_ST_FEW")) == (rr.ST_OFFSETS, rr.ST_COL, rr.ST_DUP, rr.ST_FEW)
    # the sticky bit is nobody else's
    bits = re.findall(r"_STATUS_BAD = ([^;]+);", "".join(open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith(".h")))
    assert len(bits) == len(set(b.replace(" ", "") for b in bits)), bits


def test_the_recovery_is_exact_in_python_integers():
    """the mathematics the kernels rest on: the polynomial comes back exactly; with more than c cells one changed value makes the upper
    half non-zero; with exactly c cells any values are consistent and give another polynomial"""
    for log_n, log_l in ((3, 0), (3, 3), (4, 2), (5, 2)):
        for order in (k.NATURAL, k.BITREV):
            rng = o.SplitMix64(70 + 16 * log_n + log_l + order)
            n, l, c = 1 << log_n, 1 << log_l, 1 << (log_n - log_l)
            pats = rr.patterns(rng, log_n, log_l)
            polys = rr.special_polys(rng, n, l)
            for name in ("exactly-c-random", "c-plus-1", "all"):
                col, offsets, cells = rr.call_inputs(polys, [pats[name]] * 4, log_n, log_l, order)
                got, ok = rr.recover(col, offsets, cells, log_n, log_l, order)
                assert ok == [1] * 4 and got == polys, (log_n, log_l, order, name)
                cells[offsets[3]][l - 1] = (cells[offsets[3]][l - 1] + 1) % R
                got, ok = rr.recover(col, offsets, cells, log_n, log_l, order)
                if name == "exactly-c-random":
                    assert ok == [1] * 4 and got[:3] == polys[:3] and got[3] != polys[3]
                    assert [k.cells_by_ntt(got[3], log_n, log_l, order)[i] for i in pats[name]] == cells[offsets[3]:offsets[4]]
                else:
                    assert ok == [1, 1, 1, 0] and got[:3] == polys[:3] and not any(got[3])
