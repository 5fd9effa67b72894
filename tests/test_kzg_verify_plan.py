"""csrc/kzg_verify_plan.h on its own: tests/cpp/kzg_verify_plan_main.cpp -- a stand-alone program that includes nothing but that header --
built with host clang++ -fsanitize=address,undefined -fno-sanitize-recover and run directly.  It walks the fold of batched KZG cell-proof
verification as a model over counters for every (log_n <= 8, log_l <= log_n), m in {0, 1, 5, 300}, batch cuts with empty, one-cell and
one-batch-of-all batches and four chunk sizes: every chunk covers each cell exactly once, the scratch is never exceeded, broken offsets
flag exactly the batches they touch.  Then one call per refusal of the argument checks, 64-bit extremes included.  Nothing here is
loaded into Python.

The exponent maps the program prints are compared with tests/kzg_ref.py, and the identities the kernels rest on (tests/kzg_verify_ref.py)
with Lagrange's formula on the cell's own points, in both orders."""
import os
import re
import subprocess

import pytest

import kzg_ref as k
import kzg_verify_ref as v
from oracle import bls12_381_ref as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SRC = os.path.join(ROOT, "tests", "cpp", "kzg_verify_plan_main.cpp")
CSRC = os.path.join(ROOT, "bls12_381_amd", "csrc")
HDRS = [os.path.join(CSRC, "kzg_verify_plan.h")]
EXE = os.path.join(ROOT, "build", "kzg_verify_plan_main")
SHAPES = [(0, 0), (3, 0), (3, 3), (4, 2), (6, 1), (8, 6)]
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
    for part in ("plans", "refusals", "shapes"):
        assert part in words, "the program did not reach '%s':\n%s" % (part, output[-2000:])
    assert int(words[words.index("refusals") + 1]) >= 40
    assert output.strip().endswith("all ok")


def test_the_exponent_maps_agree_with_the_reference(output):
    """h_col = w^e with e = kzg_ref.coset_shift_exponent, and the table exponent of a = h^l is the negative of e l mod 2n"""
    rows = [tuple(int(x) for x in line.split()[1:]) for line in output.splitlines() if line.startswith("map ")]
    assert len(rows) == sum(2 * (2 << (n - l)) for n in range(9) for l in range(n + 1))
    for log_n, log_l, order, col, e, a in rows:
        assert e == k.coset_shift_exponent(col, log_n, log_l, order), (log_n, log_l, order, col)
        assert a == (-(e << log_l)) % (2 << log_n)
    w = o.fr_omega(5)                                              # (4, 2): winv^a is h^l
    winv = pow(w, R - 2, R)
    for log_n, log_l, order, col, e, a in rows:
        if (log_n, log_l) == (4, 2):
            assert pow(winv, a, R) == pow(v.shift(col, 4, 2, order), 4, R)


def test_the_published_limits_match_the_plan():
    """the limits the public header states are the plan's"""
    plan = open(HDRS[0]).read()
    pub = open(os.path.join(ROOT, "include", "bls12_381_hip.h")).read()
    const = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, plan).group(1))
    assert (const("KZGV_MAX_LOG_N"), const("KZGV_MAX_LOG_L"), const("KZGV_MAX_LOG_CELLS"), const("KZGV_MAX_LOG_SEGS"), const("KZGV_MAX_LOG_SCALARS")) == (23, 12, 24, 24, 27)
    doc = pub[pub.index("Batched verification of KZG cell proofs"):pub.index("typedef struct blsgpu_kzg_cell_verifier")]
    for text in ("log_n outside\n * [0, 23]", "log_l outside [0, min(log_n, 12)]", "m <= 2^24", "nseg <= 2^24", "m * l <= 2^27", "nseg * l <= 2^27", "16-byte", "8-byte", "4-byte"):
        assert text in doc, text
    assert 1 << const("KZGV_MAX_LOG_L") == int(re.search(r"#define BLSGPU_SEG_LEN_MAX (\d+)", pub).group(1))
    assert "KZGV_ORDER_NATURAL = 0, KZGV_ORDER_BITREV = 1" in plan and "#define BLSGPU_FR_ORDER_NATURAL 0" in pub.replace("  ", " ")
    for item in ("byte-level inputs", "big-endian scalars", "Fiat-Shamir derivation of r", "recovery from half the cells", "Pippenger MSM over", "multi-GPU", "unpredictable",
                 "one pairing product per cell"):
        assert item in doc, item
    kzg = open(os.path.join(CSRC, "kzg_plan.h")).read()
    assert re.search(r"KZG_MAX_LOG_N = (\d+)", kzg).group(1) == "23" and re.search(r"KZG_MAX_LOG_L = (\d+)", kzg).group(1) == "12"


@pytest.mark.parametrize("order", [k.NATURAL, k.BITREV], ids=["natural", "bitrev"])
@pytest.mark.parametrize("log_n,log_l", SHAPES)
def test_the_identities_of_the_fold_hold_in_the_scalar_model(log_n, log_l, order):
    """I[u] = h^(-u) INTT_l(v)[u] is the polynomial through the cell's own points, entry t of a BITREV cell is the coset point
    h g^bitrev(t), and honest inputs over powers of tau satisfy the equation while a changed cell does not"""
    rng = o.SplitMix64(900 + 16 * log_n + log_l + order)
    l, cells = 1 << log_l, 2 << (log_n - log_l)
    w = o.fr_omega(log_n + 1)
    g = pow(w, cells, R)
    assert g == (o.fr_omega(log_l) if log_l else 1)
    for col in sorted({0, 1, cells - 1}):
        cell = [rng.scalar() for _ in range(l)]
        if log_l <= 3:
            assert v.interpolate(cell, col, log_n, log_l, order) == v.interpolate_direct(cell, col, log_n, log_l, order)
        coeffs = v.interpolate(cell, col, log_n, log_l, order)
        h = v.shift(col, log_n, log_l, order)
        for t in sorted({0, l - 1, l // 2}):
            x = pow(w, k.cell_point_exponent(col, t, log_n, log_l, order), R)
            assert x == h * pow(g, k.bitrev(t, log_l) if order == k.BITREV else t, R) % R
            assert k.evaluate(coeffs, x) == cell[t]
    row, col = [0, 1, 0, 1, 0], [0, cells - 1, 1 % cells, 0, cells // 2]
    commits, cs, proofs, sigma, T = v.honest(rng, log_n, log_l, order, 2, row, col)
    rr = [rng.scalar(), 0, 1]
    for offsets in ([0, 5], [0, 1, 2, 3, 4, 5], [0, 0, 3, 3, 5]):
        r = [rr[s % 3] for s in range(len(offsets) - 1)]
        assert [x[2] for x in v.batch(commits, row, col, cs, proofs, offsets, r, sigma, T, log_n, log_l, order)] == [1] * (len(offsets) - 1)
    broken = [list(c) for c in cs]
    broken[3][l - 1] = (broken[3][l - 1] + 1) % R
    assert [x[2] for x in v.batch(commits, row, col, broken, proofs, [0, 3, 5], rr[:2], sigma, T, log_n, log_l, order)] == [1, 0]
    offsets = [0, 3, 3, 5]
    r = [rng.scalar() for _ in range(3)]
    commits, row, cs, proofs, sigma, T = v.consistent(rng, log_n, log_l, order, col, offsets, r, zero_sigma=1, zero_proof=1)
    assert [x[2] for x in v.batch(commits, row, col, cs, proofs, offsets, r, sigma, T, log_n, log_l, order)] == [1, 1, 1]
