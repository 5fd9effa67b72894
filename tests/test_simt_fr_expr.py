"""The Fr expression programs (blsgpu_fr_expr_eval), their device code compiled for the HOST (tests/simt/emu_fr_expr.cpp), against a
Python-integer interpreter of the program format (tests/fr_expr_ref.py).

What runs here is the code the GPU runs: the image frx_prog_build makes of a validated program, and `k_frx_eval` launched from the plan of
csrc/fr_expr_plan.h -- the function api_fr.hip launches from -- with its grid, block, LDS size and rows per lane, at the shape
{block 64, chunk 2}: 128 rows are exactly one tile, 512 four workgroups.  Results are compared limb for limb on the raw 256-bit
integers, so a non-canonical output does not compare equal.  Every column has exactly the length its col_log_len states and ends
against an inaccessible page, `out` is pre-filled with a pattern no result has, and everything runs in a child process under a time
limit (tests/simt_fr_expr_child.py).

That the tests bite is itself a test: test_the_suite_catches_a_seeded_fault builds the library with each of the kernel's five
seeded faults (-DFRX_FAULT=n in fr_expr.hip.h) and requires the cases of this file to tell it from the real one."""
import numpy as np
import pytest

import fr_expr_ref as ref
import simt_fr_expr_child as child
import simt_harness
from oracle import bls12_381_ref as o

RR = ref.RR
SHAPE = (64, 2)
SPECIAL = (0, RR - 1, 1)


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    return simt_harness.emu_lib(child.build)


class Case:
    """one evaluation: the program, the columns as integers (an int entry: the very buffer of that earlier column), the job, the expectation"""

    def __init__(self, what, prog, n_cols, n_regs, consts, cols, log_n, log_stride=0, col_log_len=None, shape=SHAPE):
        self.what, self.prog, self.n_cols, self.n_regs, self.consts, self.cols = what, prog, n_cols, n_regs, consts, cols
        self.log_n, self.log_stride, self.ll, self.shape = log_n, log_stride, col_log_len, shape

    def job(self, lib=None):
        cols = [c if c is None or isinstance(c, int) else ref.mont_words(c) for c in self.cols]
        return {"op": "eval", "n_cols": self.n_cols, "n_regs": self.n_regs, "consts": ref.mont_limbs(self.consts) if self.consts else None, "code": ref.words(self.prog),
                "cols": cols, "col_log_len": self.ll, "log_n": self.log_n, "log_stride": self.log_stride, "shape": self.shape, "lib": lib, "label": self.what}

    def expect(self):
        cols = [self.cols[c] if isinstance(c, int) else c for c in self.cols]
        return ref.mont(ref.run(self.prog, self.n_regs, self.consts, cols, self.ll, self.log_n, self.log_stride))

    def differs(self, res):
        got, want = ref.raw_ints(res["out"]), self.expect()
        assert len(got) == len(want) == 1 << self.log_n, self.what
        return [i for i in range(len(got)) if got[i] != want[i]]

    def check(self, res):
        bad = self.differs(res)
        assert not bad, "%s: %d of %d rows differ, first at %d" % (self.what, len(bad), 1 << self.log_n, bad[0])
        if self.shape:
            assert res["grid"] == -(-(1 << self.log_n) // (self.shape[0] * self.shape[1])), self.what


def _column(n, rng, special=True):
    c = [rng.scalar() for _ in range(n)]
    if special:
        for i, v in zip((0, n - 1, n // 2), SPECIAL):
            c[i] = v
    return c


def kind_matrix_cases():
    """the operand-kind matrix at N = 1, 2, 64 (less than one tile), 128 (exactly one tile) and 512 (four tiles); the constants are
    r - 1 and a seeded value, the columns hold 0 and r - 1 at their ends"""
    prog, n_cols, n_regs, _ = ref.kind_matrix_program()
    out = []
    for log_n in (0, 1, 6, 7, 9):
        rng = o.SplitMix64(100 + log_n)
        consts = [RR - 1, rng.scalar()]
        out.append(Case("kind matrix N=%d" % (1 << log_n), prog, n_cols, n_regs, consts, [_column(1 << log_n, rng), _column(1 << log_n, rng)], log_n))
    return out


def rotation_cases():
    """rotations +1, -1, +3, -32768 and +32767 of one column, summed with distinct constant weights so that no two can swap, at
    log_stride 0, 2 and log_n: the wrap is at both ends of the table and, at 512 rows with stride 4 or a rotation of +-2^15, inside a tile"""
    rots = (1, -1, 3, -32768, 32767)
    prog = [("MUL", 0, ("col", 0, 0), ("const", 0))]
    for k, r in enumerate(rots):
        prog.append(("MAD", 0, ("col", 0, r), ("const", 1 + k)))
    out = []
    for log_n in (1, 7, 9):
        for ls in sorted({0, min(2, log_n), log_n}):
            rng = o.SplitMix64(7000 + 16 * log_n + ls)
            consts = [rng.scalar() for _ in range(1 + len(rots))]
            out.append(Case("rotations N=%d stride=2^%d" % (1 << log_n, ls), prog, 1, 1, consts, [_column(1 << log_n, rng, special=False)], log_n, ls))
    return out


def length_cases():
    """columns of length 1, 4 and N in one program, the length-4 column read at rotations +1 and -3 (it wraps on ITS length), at N = 512 and
    at N = 4 (where 4 is the full length); and the same program with every column the same pointer"""
    prog = [("MUL", 0, ("col", 0, 0), ("col", 1, 0)),                 # N x 1
            ("MAD", 0, ("col", 2, 1), ("col", 0, -1)),                # 4 (rotated) x N (rotated)
            ("MAD", 0, ("col", 2, -3), ("col", 1, 5)),                # a rotated read of the length-1 column is that scalar
            ("ADD", 0, ("reg", 0), ("col", 2, 0))]
    out = []
    for log_n, ls in ((9, 0), (9, 2), (2, 0), (2, 2)):
        rng = o.SplitMix64(900 + log_n + ls)
        n = 1 << log_n
        out.append(Case("lengths N, 1, 4 at N=%d stride=2^%d" % (n, ls), prog, 3, 1, [], [_column(n, rng), [rng.scalar()], _column(4, rng, special=False)], log_n, ls, [log_n, 0, 2]))
    rng = o.SplitMix64(77)
    out.append(Case("every column the same pointer", prog, 3, 1, [], [_column(512, rng), 0, 0], 9, 0, None))
    out.append(Case("the same pointer at three lengths", prog, 3, 1, [], [_column(512, rng), 0, 0], 9, 2, [9, 0, 2]))
    return out


def register_cases():
    """n_regs = 1 (everything through one register) and n_regs = 8 (each register written, all of them read back after the others were
    written: a slot that aliased another would show), and a 256-instruction program"""
    rng = o.SplitMix64(5)
    one = [("MOV", 0, ("col", 0, 0), None), ("MUL", 0, ("reg", 0), ("reg", 0)), ("MAD", 0, ("reg", 0), ("col", 1, 0)), ("SUB", 0, ("reg", 0), ("const", 0))]
    eight = [("MUL", k, ("col", 0, 0), ("const", k)) for k in range(8)] + [("MAD", 0, ("reg", k), ("const", 8 - k)) for k in range(1, 8)]
    long = [("MOV", 0, ("col", 0, 0), None), ("MOV", 1, ("col", 1, 0), None)]
    while len(long) < 256:
        k = len(long)
        long.append((("MAD", "ADD", "MUL", "SUB")[k % 4], k % 2, ("reg", (k + 1) % 2), (("col", k % 2, k % 5 - 2), ("const", k % 3), ("reg", k % 2))[k % 3]))
    consts = [rng.scalar() for _ in range(9)]
    cols = [_column(512, rng), _column(512, rng)]
    return [Case("n_regs=1", one, 2, 1, consts[:1], cols, 9), Case("n_regs=8", eight, 2, 8, consts, cols, 9), Case("256 instructions", long, 2, 2, consts[:3], cols, 9)]


def all_cases():
    return kind_matrix_cases() + rotation_cases() + length_cases() + register_cases()


def _run(cases):
    for c, r in zip(cases, child.run([c.job() for c in cases])):
        c.check(r)


def test_every_op_with_every_pair_of_operand_kinds():
    _run(kind_matrix_cases())


def test_rotations_strides_and_the_wrap():
    cases = rotation_cases()
    # where the wraps are: at N = 512 and stride 4, rotation +3 sends the rows from 500 on to rows 0 .. 11, rotation -1 sends rows 0 .. 3 to
    # 508 .. 511, and +32767 lands inside a tile (row 300 reads row 296)
    assert any(x.log_n == 9 and x.log_stride == 2 for x in cases)
    assert (500 + 3 * 4) % 512 == 0 and (0 - 1 * 4) % 512 == 508 and (300 + 32767 * 4) % 512 == 296
    _run(cases)


def test_columns_of_length_1_4_and_n_and_aliases():
    _run(length_cases())


def test_one_and_eight_registers_and_a_full_program():
    cases = register_cases()
    assert len(cases[2].prog) == 256
    _run(cases)


def test_the_shipped_shape():
    """block 256 with one row per lane, as the plan ships it below 2^19 rows: 2^9 rows are two workgroups; the kind matrix once more"""
    prog, n_cols, n_regs, _ = ref.kind_matrix_program()
    rng = o.SplitMix64(31)
    cases = [Case("shipped shape, kind matrix", prog, n_cols, n_regs, [RR - 1, rng.scalar()], [_column(512, rng), _column(512, rng)], 9, shape=None)]
    for c, r in zip(cases, child.run([c.job() for c in cases])):
        c.check(r)
        assert r["grid"] == 2


def test_the_plan_and_its_python_mirror():
    """log_n 0 .. 28 x n_regs 1 .. 8 at the shipped shapes: the grid covers N exactly, LDS is block * n_regs * 32 bytes and two workgroups
    fit a CU; tests/fr_expr_ref.py's shipped_chunk (which the GPU tests place their samples by) is the plan's; the refusals"""
    jobs = [{"op": "plan", "log_n": ln, "n_regs": nr, "label": "plan"} for ln in range(29) for nr in range(1, 9)]
    for j, r in zip(jobs, child.run(jobs)):
        n = 1 << j["log_n"]
        assert r["ok"] == 1 and r["block"] == ref.BLOCK and r["chunk"] == ref.shipped_chunk(j["log_n"]), (j, r)
        assert r["rows"] == n and r["tile"] == r["block"] * r["chunk"] and r["grid"] * r["tile"] >= n > (r["grid"] - 1) * r["tile"], (j, r)
        assert r["lds"] == 256 * j["n_regs"] * 32 and 2 * r["lds"] <= 160 * 1024, (j, r)
    small = child.run([{"op": "plan", "log_n": 9, "n_regs": 3, "shape": SHAPE, "label": "small"}])[0]
    assert (small["grid"], small["block"], small["chunk"], small["lds"]) == (4, 64, 2, 64 * 3 * 32)
    bad = [dict(log_n=-1, n_regs=1), dict(log_n=29, n_regs=1), dict(log_n=5, n_regs=0), dict(log_n=5, n_regs=9), dict(log_n=5, n_regs=1, shape=(96, 1)), dict(log_n=5, n_regs=1, shape=(64, 0))]
    assert [r["ok"] for r in child.run([dict(b, op="plan", label="refusal") for b in bad])] == [0] * len(bad)


def test_validation_names_the_instruction():
    """frx_prog_build through the emulation library (tests/test_fr_expr_plan.py sweeps it under the sanitizers): a program that reads a
    register before writing it is refused with the instruction index, the accessors' figures of a valid one"""
    prog, n_cols, n_regs, n_consts = ref.kind_matrix_program()
    ok = child.run([{"op": "build", "n_cols": n_cols, "n_regs": n_regs, "consts": ref.mont_limbs([1, 2]), "code": ref.words(prog), "label": "valid"},
                    {"op": "build", "n_cols": 1, "n_regs": 2, "consts": None, "code": ref.words([("MOV", 0, ("col", 0, 0), None), ("ADD", 0, ("reg", 0), ("reg", 1))]), "label": "stale"}])
    assert ok[0]["ok"] and ok[0]["cols_read"] == 3 and ok[0]["max_rot"] == 1
    assert ok[0]["products"] == sum(1 for i in prog if i[0] in ("MUL", "MAD"))
    assert not ok[1]["ok"] and "instruction 1" in ok[1]["error"] and "before" in ok[1]["error"]


FAULTS = {1: "rotation sign flipped", 2: "a short column wrapped with log_n instead of its own length", 3: "SUB operands swapped", 4: "MAD dropping the accumulate",
          5: "the lane's second chunk row reading the first row's registers"}


@pytest.mark.parametrize("fault", sorted(FAULTS), ids=["fault%d" % f for f in sorted(FAULTS)])
def test_the_suite_catches_a_seeded_fault(fault):
    """the cases above against a library whose kernel carries ONE seeded fault: some case must differ from the Python integers, or the
    child must die on a guarded page (a short column read with the table's length runs off its end)"""
    lib = child.build_fault(fault)
    cases = all_cases()
    try:
        res = child.run([c.job(lib) for c in cases])
    except pytest.fail.Exception as e:
        assert fault == 2 and "SIGSEGV" in str(e), "fault %d (%s) ended the child: %s" % (fault, FAULTS[fault], e)
        return
    caught = [c.what for c, r in zip(cases, res) if c.differs(r)]
    assert caught, "no case tells fault %d (%s) from the real kernel" % (fault, FAULTS[fault])
