"""csrc/kzg_plan.h on its own: tests/cpp/kzg_plan_main.cpp -- a stand-alone program that includes nothing but that header -- built with
host clang++ -fsanitize=address,undefined -fno-sanitize-recover and run directly.  It walks the data movement of the amortised KZG
openings as a model over index arrays for every (log_n <= 8, log_l <= log_n), count in {0, 1, 3}, both forms and both tile shapes: every
S^ / c^ slot is written exactly once, every segment's scalar and base range lies inside its array, the transposition and both
numberings of proofs and cells are bijections, the scratch the plan reserves is never exceeded.  Then one call per refusal of the
argument checks, 64-bit extremes included.  Nothing here is loaded into Python.

The index maps themselves are compared with tests/kzg_ref.py, and the root the numbering rests on with the constant EIP-7594 names."""
import os
import re
import subprocess

import pytest

import kzg_ref as k
from oracle import bls12_381_ref as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SRC = os.path.join(ROOT, "tests", "cpp", "kzg_plan_main.cpp")
CSRC = os.path.join(ROOT, "bls12_381_amd", "csrc")
HDRS = [os.path.join(CSRC, "kzg_plan.h")]
EXE = os.path.join(ROOT, "build", "kzg_plan_main")


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
    """the limits the public header states are the plan's"""
    plan = open(HDRS[0]).read()
    pub = open(os.path.join(ROOT, "include", "bls12_381_hip.h")).read()
    const = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, plan).group(1))
    assert (const("KZG_MAX_LOG_N"), const("KZG_MAX_LOG_L"), const("KZG_MAX_LOG_TERMS"), const("KZG_MAX_LOG_POINTS")) == (23, 12, 27, 24)
    assert (const("KZG_CELLS_MAX_LOG_N"), const("KZG_CELLS_MAX_LOG_TOTAL")) == (27, 28)
    doc = pub[pub.index("Amortised KZG openings"):pub.index("typedef struct blsgpu_kzg_multiproof")]
    for text in ("log_n in [0, 23]", "log_l in [0, min(log_n, 12)]", "count * 2n <= 2^27", "count * 2c <= 2^24", "log_n in [0, 27]", "count * 2n <= 2^28"):
        assert text in doc, text
    assert 1 << const("KZG_MAX_LOG_L") == int(re.search(r"#define BLSGPU_SEG_LEN_MAX (\d+)", pub).group(1))
    assert "#define BLSGPU_KZG_FORM_COEFFS 0" in pub and "#define BLSGPU_KZG_FORM_EVALS  1" in pub
    assert "KZG_FORM_COEFFS = 0, KZG_FORM_EVALS = 1" in plan and "KZG_ORDER_NATURAL = 0, KZG_ORDER_BITREV = 1" in plan
    for item in ("verification of cells", "recovery from half the cells", "G2", "Lagrange-form SRS", "window-table precomputation"):
        assert item in doc, item


def test_the_root_of_the_cell_numbering_is_the_one_blob_formats_use():
    """the root for log 13 is 7^((r - 1) / 8192) and the root for log 12 its square: bitrev(i l + t, 13) over it is EIP-7594's numbering"""
    assert o.fr_omega(13) == pow(7, (o.R_ORDER - 1) // 8192, o.R_ORDER)
    assert o.fr_omega(12) == o.fr_omega(13) ** 2 % o.R_ORDER
    for log_n, log_l in ((4, 2), (3, 0), (3, 3), (6, 1), (12, 6)):
        for i in (0, 1, (2 << (log_n - log_l)) - 1):
            for t in (0, (1 << log_l) - 1):
                assert k.bitrev((i << log_l) + t, log_n + 1) == k.bitrev(t, log_l) * (2 << (log_n - log_l)) + k.bitrev(i, log_n + 1 - log_l)


@pytest.mark.parametrize("log_n,log_l", [(4, 2), (3, 0), (3, 3), (6, 1), (5, 3)])
def test_the_three_forms_of_the_contract_agree(log_n, log_l):
    """the definition by division, the h_d form and the circulant route stage by stage, for an SRS that is no geometric sequence; cells by
    direct evaluation and through the size-2n transform"""
    rng = o.SplitMix64(100 * log_n + log_l)
    p, sigma = k.random_poly(rng, 1 << log_n), k.random_poly(rng, 1 << log_n)
    for order in (k.NATURAL, k.BITREV):
        want = k.proofs_by_division(p, sigma, log_n, log_l, order)
        assert k.proofs_by_h(p, sigma, log_n, log_l, order) == want
        assert k.pipeline(p, sigma, log_n, log_l, order) == want
        assert k.cells_by_ntt(p, log_n, log_l, order) == k.cells(p, log_n, log_l, order)
    low = p[:1 << log_l] + [0] * ((1 << log_n) - (1 << log_l))
    assert not any(k.proofs_by_division(low, sigma, log_n, log_l, k.NATURAL))
