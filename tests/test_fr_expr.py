"""Fr expression programs (`blsgpu_fr_expr_*`; csrc/fr_expr.hip.h + csrc/fr_expr_plan.h) on the GPU.

Three kinds of expectation: a Python-integer interpreter of the program format (tests/fr_expr_ref.py: all rows at small sizes, sampled
rows at 2^20), the composed route on the device (tools/fr_expr_time.py's Composed: one `fr_op_device` call per instruction --
limb-identical), and an identity that needs no reference at all: the quotient of a satisfying vanilla-PLONK instance, evaluated on the
extended coset and transformed back, has degree below 3n -- and no longer once one wire is changed."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import fr_expr_ref as ref
from bls12_381_amd import synthetic
from oracle import bls12_381_ref as o

pytestmark = pytest.mark.gpu

RR = ref.RR
RINV = pow(ref.MONT, -1, RR)
ERR_ARG = -2
FR_MUL = 0                                                         # blsgpu_fr_op
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    import bls12_381_amd as b
    c = b.Context(0)
    yield c
    c.close()


def limbs(vals):
    return ref.mont_limbs(vals)


def raw(n, seed):
    """n canonical scalars as raw limbs (any integer below r is the Montgomery form of some scalar)"""
    s = np.random.RandomState(seed).randint(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= 0x3F
    return s.view(np.uint64).reshape(n, 4).copy()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda")


def host(t):
    return t.cpu().numpy().view(np.uint64)


class RawColumn:
    """raw limbs read as the integers they stand for, one row at a time (the sampled checks touch a few thousand of 2^20 rows)"""

    def __init__(self, a):
        self.a = a

    def __getitem__(self, i):
        return int.from_bytes(self.a[i].tobytes(), "little") * RINV % RR


def both_forms(ctx, e, cols, log_n, log_stride, ll):
    """the host form and the device form on the same columns ((len, 4) u64 arrays or None): equal, and returned once"""
    import torch
    got = e.eval(cols, log_n, log_stride, ll)
    d_cols = [None if c is None else dev(c) for c in cols]
    d_out = torch.zeros((1 << log_n, 4), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    e.eval_device([None if t is None else t.data_ptr() for t in d_cols], log_n, d_out.data_ptr(), log_stride, ll)
    ctx.synchronize()
    assert np.array_equal(host(d_out), got), "the device form differs from the host form"
    for t, c in zip(d_cols, cols):
        assert t is None or np.array_equal(host(t), c), "an input was written to"
    return got


# ---- against Python integers, all rows ----------------------------------------------------------------------------------------------
def test_the_plonk_program_against_python_integers(ctx):
    """the standard program at log_n = 8 with log_stride = 2 (z read four rows on, 1 / Z_H a column of 4, four challenges of length 1),
    seeded columns with 0 and r - 1 among them: every row, both forms"""
    log_n, ls = 8, 2
    n_cols, n_regs, consts, instrs = synthetic.plonk_quotient_program()
    ll = synthetic.plonk_col_log_len(log_n, ls)
    rng = o.SplitMix64(2025)
    cols = [[rng.scalar() for _ in range(1 << l)] for l in ll]
    for j in range(0, n_cols, 3):
        cols[j][0], cols[j][-1] = 0, RR - 1
    e = ctx.fr_expr(n_cols, n_regs, consts, instrs)
    assert (e.cols, e.regs, e.instructions, e.products_per_row, e.cols_read) == (n_cols, n_regs, len(instrs), 21, (1 << n_cols) - 1)
    got = both_forms(ctx, e, [limbs(c) for c in cols], log_n, ls, ll)
    want = ref.mont(ref.run(ref.from_tuples(instrs), n_regs, consts, cols, ll, log_n, ls))
    assert ref.raw_ints(got) == want
    e.close()


@pytest.mark.parametrize("log_n", [0, 8, 12])
def test_the_operand_kind_matrix_against_python_integers(ctx, log_n):
    """every op with every pair of operand kinds, a square, MADs that read their dst as an operand (the emulation's program), at N = 1,
    256 and 2^12 -- one lane, one workgroup, sixteen: every row, both forms; the constants are r - 1 and a seeded value"""
    prog, n_cols, n_regs, _ = ref.kind_matrix_program()
    rng = o.SplitMix64(300 + log_n)
    consts = [RR - 1, rng.scalar()]
    n = 1 << log_n
    cols = [[rng.scalar() for _ in range(n)] for _ in range(2)]
    cols[0][0], cols[1][-1], cols[0][n // 2] = 0, RR - 1, RR - 1
    e = ctx.fr_expr(n_cols, n_regs, consts, ref.to_tuples(prog))
    got = both_forms(ctx, e, [limbs(c) for c in cols], log_n, 0, None)
    assert ref.raw_ints(got) == ref.mont(ref.run(prog, n_regs, consts, cols, None, log_n, 0))
    e.close()


# ---- tile and grid edges at size ------------------------------------------------------------------------------------------------------
EDGE_PROG = [("MUL", 0, ("col", 0, 0), ("col", 1, 1)), ("MAD", 0, ("col", 2, -3), ("col", 3, 1)), ("MAD", 0, ("col", 4, 0), ("col", 0, 2)), ("SUB", 1, ("reg", 0), ("col", 2, 3)),
             ("MAD", 1, ("reg", 0), ("col", 1, -1))]
EDGE_STRIDE = 2


def _edge_sample(log_n, count=4096):
    """the rows the sampled check looks at, with what the sample must contain"""
    n = 1 << log_n
    tile = ref.BLOCK * ref.shipped_chunk(log_n)
    reach = 3 * (1 << EDGE_STRIDE)                                 # the largest |rot| * stride of EDGE_PROG
    must = {0, n - 1, tile - 1, tile, 2 * tile - 1, n - tile} | set(range(reach)) | set(range(n - reach, n))
    rows = set(must)
    rows |= {int(x) for x in np.random.RandomState(log_n).randint(0, n, size=2 * count)[:count - len(rows)]}
    rows = sorted(rows)
    # these conditions are part of the test
    assert 0 in rows and n - 1 in rows
    for first in (0, tile, n - tile):                              # first and last row of the first, second and last workgroup
        assert first in rows and first + tile - 1 in rows
    assert all(i in rows and n - 1 - i in rows for i in range(reach))      # every row within |rot| * stride of the wrap
    assert len(rows) <= count and len(rows) >= count - 64
    return rows


@pytest.mark.parametrize("log_n", [20, 19])
def test_tile_and_grid_edges_at_size(ctx, log_n):
    """N = 2^20 (four rows per lane, 1024 workgroups) and 2^19 (two rows per lane: the largest grid the plan produces below 2^20):
    rotations -3 .. +3 at stride 4, a column of 4 and a column of 1, against Python integers on 4096 sampled rows that include the
    table's ends, the first and last row of the first, second and last workgroup and every row whose rotated reads wrap"""
    import torch
    n = 1 << log_n
    assert n // (ref.BLOCK * ref.shipped_chunk(log_n)) == 1024
    ll = [log_n, log_n, log_n, EDGE_STRIDE, 0]
    arrays = [raw(1 << l, 40 + j) for j, l in enumerate(ll)]
    e = ctx.fr_expr(5, 2, None, ref.to_tuples(EDGE_PROG))
    d_cols = [dev(a) for a in arrays]
    d_out = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    e.eval_device([t.data_ptr() for t in d_cols], log_n, d_out.data_ptr(), EDGE_STRIDE, ll)
    ctx.synchronize()
    got = host(d_out)
    rows = _edge_sample(log_n)
    want = ref.mont(ref.run(EDGE_PROG, 2, [], [RawColumn(a) for a in arrays], ll, log_n, EDGE_STRIDE, rows))
    bad = [i for i, w in zip(rows, want) if int.from_bytes(got[i].tobytes(), "little") != w]
    assert not bad, "%d of %d sampled rows differ, first at %d" % (len(bad), len(rows), bad[0])
    e.close()


# ---- against the composed route ---------------------------------------------------------------------------------------------------------
def test_against_the_composed_route(ctx):
    """the standard PLONK program at N = 2^16 against one fr_op_device call per instruction on full-length temporaries (the periodic
    column, the challenges and the constants expanded for that route, the rotated operand copied with its wrap): limb for limb.  This
    is the baseline tools/fr_expr_time.py times."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fr_expr_time
    log_n, ls = 16, 2
    n_cols, n_regs, consts, instrs = synthetic.plonk_quotient_program()
    ll = synthetic.plonk_col_log_len(log_n, ls)
    cols = [dev(raw(1 << l, 70 + j)) for j, l in enumerate(ll)]
    d_out = torch.zeros((1 << log_n, 4), dtype=torch.int64, device="cuda")
    e = ctx.fr_expr(n_cols, n_regs, consts, instrs)
    stream = torch.cuda.Stream(device=torch.device("cuda", 0))
    comp = fr_expr_time.Composed(ctx, stream, n_regs, [dev(limbs([c]))[0] for c in consts], instrs, log_n, ls, torch.device("cuda", 0))
    comp.prepare(cols, ll)
    torch.cuda.synchronize()
    ctx.set_stream(stream.cuda_stream)
    try:
        e.eval_device([t.data_ptr() for t in cols], log_n, d_out.data_ptr(), ls, ll)
        want = comp.run()
        ctx.synchronize()
    finally:
        ctx.set_stream(None)
    assert comp.calls == len(instrs) + sum(1 for i in instrs if i[0] == "MAD") and comp.copies == 2
    assert torch.equal(d_out, want) and bool(d_out.any())
    e.close()


# ---- the quotient identity, end to end on the device -----------------------------------------------------------------------------------
def _quotient_coefficients(ctx, inst, log_n, e_bits, expr):
    """trace columns -> coefficients -> the coset g = 7 of the extended domain -> the expression -> coefficients of the quotient, every
    step a device call on resident data (the only copies are the uploads of the instance and the read-back of the result)"""
    import torch
    n, log_big = 1 << log_n, log_n + e_bits
    big = 1 << log_big
    names = ["a", "b", "c", "qL", "qR", "qO", "qM", "qC", "s1", "s2", "s3", "z"]
    g = 7
    d_trace = dev(np.stack([limbs(inst[k]) for k in names]))        # (12, n, 4)
    # X: the coefficient vector (0, 1, 0, ...); L_1: (1/n, ..., 1/n, 0, ..., 0) -- the documented recipes
    x_coef = [0, 1] + [0] * (big - 2)
    l1_coef = [pow(n, -1, RR)] * n + [0] * (big - n)
    d_ext = torch.zeros((14, big, 4), dtype=torch.int64, device="cuda")
    d_ext[12], d_ext[13] = dev(limbs(x_coef)), dev(limbs(l1_coef))
    # Z_H on the coset takes 2^e values: g^n w^(n i) - 1 with w the 2^log_big-th root the transform uses
    w = pow(7, (RR - 1) >> log_big, RR)
    d_zh = dev(limbs([(pow(g, n, RR) * pow(w, n * i, RR) - 1) % RR for i in range(1 << e_bits)]))
    alpha = inst["alpha"]
    d_chal = dev(limbs([inst["beta"], inst["gamma"], alpha, alpha * alpha % RR]))
    d_out = torch.zeros((big, 4), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.fr_ntt_many_device(d_trace.data_ptr(), log_n, 12, inverse=True)
    ctx.synchronize()
    d_ext[:12, :n] = d_trace                                       # zero-padded, on the device
    torch.cuda.synchronize()
    ctx.fr_ntt_many_device(d_ext.data_ptr(), log_big, 14, coset=g)
    ctx.fr_batch_invert_device(d_zh.data_ptr(), 1 << e_bits, d_zh.data_ptr())
    C = synthetic.PLONK_COLS
    ptrs = [0] * len(C)
    for j, k in enumerate(names + ["X", "L1"]):
        ptrs[C[k]] = d_ext[j].data_ptr()
    ptrs[C["zh_inv"]] = d_zh.data_ptr()
    for j, k in enumerate(["beta", "gamma", "alpha", "alpha2"]):
        ptrs[C[k]] = d_chal[j].data_ptr()
    expr.eval_device(ptrs, log_big, d_out.data_ptr(), e_bits, synthetic.plonk_col_log_len(log_big, e_bits))
    ctx.fr_ntt_many_device(d_out.data_ptr(), log_big, 1, inverse=True, coset=g)
    ctx.synchronize()
    return host(d_out)


def test_the_quotient_of_a_satisfying_instance_has_degree_below_3n(ctx):
    """n = 2^6 rows with copy constraints and the accumulator's next-row term, N = 2^8: the quotient's coefficients [3n, 4n) are all zero
    and the low ones are not -- and with one witness entry changed the high ones are NOT all zero"""
    log_n, e_bits = 6, 2
    n = 1 << log_n
    inst = synthetic.plonk_instance(log_n, 11)
    assert sum(1 for i in range(n) if inst["s1"][i] != pow(7, (RR - 1) >> log_n, RR) ** i % RR) > n // 2      # sigma is not the identity
    n_cols, n_regs, consts, instrs = synthetic.plonk_quotient_program()
    expr = ctx.fr_expr(n_cols, n_regs, consts, instrs)
    t = _quotient_coefficients(ctx, inst, log_n, e_bits, expr)
    assert not t[3 * n:].any(), "the quotient of a satisfying instance has a coefficient at or above X^(3n)"
    assert t[:3 * n].any() and t[2 * n:3 * n].any()
    broken = dict(inst)
    broken["a"] = list(inst["a"])
    broken["a"][5] = (broken["a"][5] + 1) % RR
    assert _quotient_coefficients(ctx, broken, log_n, e_bits, expr)[3 * n:].any(), "a broken witness still divides by Z_H"
    expr.close()


# ---- streams, transcripts ---------------------------------------------------------------------------------------------------------------
def _small_case(ctx, seed, log_n=12):
    """EDGE_PROG over seeded columns: (handle, arrays, col_log_len, the host form's result)"""
    ll = [log_n, log_n, log_n, EDGE_STRIDE, 0]
    arrays = [raw(1 << l, seed + j) for j, l in enumerate(ll)]
    e = ctx.fr_expr(5, 2, None, ref.to_tuples(EDGE_PROG))
    return e, arrays, ll, e.eval(arrays, log_n, EDGE_STRIDE, ll)


def test_a_challenge_written_by_the_previous_call(ctx):
    """the length-1 column is the output of an fr_op_device mul enqueued just before the evaluation on the same stream, with no
    synchronisation in between: the result equals the host form fed the product read back afterwards"""
    import torch
    log_n = 12
    e, arrays, ll, _ = _small_case(ctx, 500, log_n)
    d_cols = [dev(a) for a in arrays]
    d_xy = dev(raw(2, 9))
    d_out = torch.zeros((1 << log_n, 4), dtype=torch.int64, device="cuda")
    d_cols[4].zero_()
    torch.cuda.synchronize()
    ctx.fr_op_device(FR_MUL, d_xy[0].data_ptr(), d_xy[1].data_ptr(), 1, d_cols[4].data_ptr())
    e.eval_device([t.data_ptr() for t in d_cols], log_n, d_out.data_ptr(), EDGE_STRIDE, ll)
    ctx.synchronize()
    chal = host(d_cols[4])
    assert chal.any() and not np.array_equal(chal, arrays[4])
    assert np.array_equal(host(d_out), e.eval(arrays[:4] + [chal], log_n, EDGE_STRIDE, ll))
    e.close()


def test_on_a_caller_stream_and_between_pipelined_msm_calls(ctx):
    """the device form on a non-default stream set with set_stream, then enqueued between two pipelined msm_device calls"""
    import torch
    log_n = 13
    e, arrays, ll, want = _small_case(ctx, 600, log_n)

    def buffers():
        return [dev(a) for a in arrays], torch.zeros((1 << log_n, 4), dtype=torch.int64, device="cuda")

    def enqueue(d_cols, d_out):
        e.eval_device([t.data_ptr() for t in d_cols], log_n, d_out.data_ptr(), EDGE_STRIDE, ll)

    def check(d_cols, d_out):
        assert np.array_equal(host(d_out), want)
        assert all(np.array_equal(host(t), a) for t, a in zip(d_cols, arrays)), "an input was written to"

    side = torch.cuda.Stream(device=torch.device("cuda", 0))
    bufs = buffers()
    torch.cuda.synchronize()
    ctx.set_stream(side.cuda_stream)
    try:
        enqueue(*bufs)
        ctx.synchronize()
    finally:
        ctx.set_stream(None)
    check(*bufs)
    m = 1 << 14
    S = np.random.RandomState(5).randint(0, 256, size=(2 * m, 32), dtype=np.uint8)
    S[:, 31] &= 0x3F
    bases = ctx.bases_from_scalars(1, S[:m])
    d_sc = torch.from_numpy(S).to("cuda")
    d_msm = torch.zeros((2, 18), dtype=torch.int64, device="cuda")
    bufs = buffers()
    torch.cuda.synchronize()
    ctx.set_pipelining(True)
    try:
        ctx.msm_device(bases, d_sc[0:m].data_ptr(), m, d_msm[0].data_ptr())
        enqueue(*bufs)
        ctx.msm_device(bases, d_sc[m:2 * m].data_ptr(), m, d_msm[1].data_ptr())
        ctx.join()
        ctx.synchronize()
    finally:
        ctx.set_pipelining(False)
    check(*bufs)
    got = ctx.batch_normalize(1, host(d_msm))
    for i in range(2):
        w = ctx.batch_normalize(1, ctx.msm(bases, S[i * m:(i + 1) * m])[None, :])
        assert np.array_equal(got[0][i], w[0][0]) and got[1][i] == w[1][0], i
    bases.free()
    e.close()


# ---- arguments ----------------------------------------------------------------------------------------------------------------------------
def test_create_refuses_a_bad_program(ctx):
    """every rule of the program format at create: BLSGPU_ERR_ARG, *out left NULL, a text naming the instruction and the rule; the
    context works afterwards"""
    lib, h = ctx.lib, ctx.h
    err = lambda: lib.blsgpu_last_error().decode()
    one = limbs([1])
    code_of = lambda prog: np.array(ref.words(prog), dtype=np.uint32)
    good = [("MOV", 0, ("col", 0, 0), None), ("MUL", 1, ("reg", 0), ("const", 0)), ("MAD", 1, ("col", 1, 1), ("reg", 0))]

    def create(n_cols=2, n_regs=2, n_consts=1, consts=one, code=None, n_instr=None):
        code = code_of(good) if code is None else code
        out = ctypes.c_void_p(0xDEAD)
        rc = lib.blsgpu_fr_expr_create(h, n_cols, n_regs, n_consts, None if consts is None else consts.ctypes.data_as(ctypes.c_void_p),
                                       len(code) // 3 if n_instr is None else n_instr, code.ctypes.data_as(ctypes.c_void_p), ctypes.byref(out))
        if rc == 0:
            lib.blsgpu_fr_expr_free(out)
        else:
            assert out.value is None, "*out must stay NULL after a refusal"
        return rc

    def patched(i, word, value=None, flip=None):
        c = code_of(good)
        c[3 * i + word] = value if value is not None else c[3 * i + word] | flip
        return c

    assert create() == 0
    for kw, text in ((dict(n_cols=0), "n_cols"), (dict(n_cols=33), "n_cols"), (dict(n_regs=0), "n_regs"), (dict(n_regs=9), "n_regs"), (dict(n_consts=33), "n_consts"),
                     (dict(n_consts=-1), "n_consts"), (dict(n_instr=0), "n_instr"), (dict(n_instr=257), "n_instr"), (dict(consts=None), "consts"),
                     (dict(consts=np.array([[2 ** 64 - 1] * 4], dtype=np.uint64)), "constant 0"),
                     (dict(consts=np.frombuffer(RR.to_bytes(32, "little"), dtype=np.uint64).copy()), "constant 0")):
        assert create(**kw) == ERR_ARG and text in err(), kw
    for code, at, text in ((patched(1, 0, value=5 | (1 << 8)), 1, "unknown op"), (patched(1, 1, value=0xC0000000), 1, "kind"), (patched(2, 0, value=3 | (2 << 8)), 2, "dst"),
                           (patched(1, 1, value=2), 1, "register 2"), (patched(2, 1, value=0x40000002), 2, "column 2"), (patched(1, 2, value=0x80000001), 1, "constant 1"),
                           (patched(1, 0, flip=1 << 16), 1, "stray"), (patched(1, 1, flip=1 << 8), 1, "stray"), (patched(2, 1, flip=1 << 24), 2, "stray"),
                           (patched(1, 2, flip=1 << 8), 1, "stray"), (patched(0, 2, value=1), 0, "MOV"), (patched(1, 1, value=1), 1, "before"),
                           (patched(1, 0, value=3 | (1 << 8)), 1, "before")):
        assert create(code=code) == ERR_ARG and "instruction %d" % at in err() and text in err(), (at, text, err())
    assert lib.blsgpu_fr_expr_create(h, 2, 2, 1, one.ctypes.data_as(ctypes.c_void_p), 3, code_of(good).ctypes.data_as(ctypes.c_void_p), None) == ERR_ARG
    with pytest.raises(Exception, match="instruction 1"):
        ctx.fr_expr(1, 2, None, [("MOV", 0, ("col", 0)), ("ADD", 0, 0, 1)])
    assert create() == 0


def test_eval_arguments(ctx):
    """every refusal of both evaluation forms is BLSGPU_ERR_ARG with a text naming the cause, before anything is staged or launched:
    out is untouched, and the next valid call succeeds"""
    import torch
    lib, h = ctx.lib, ctx.h
    log_n = 6
    n = 1 << log_n
    e, arrays, ll, want = _small_case(ctx, 700, log_n)
    err = lambda: lib.blsgpu_last_error().decode()
    y = np.zeros((n + 1, 4), dtype=np.uint64)
    d_arrays = [dev(np.concatenate([a, a[:1]])) for a in arrays]  # one scalar of slack behind every column
    h_arrays = [np.concatenate([a, a[:1]]) for a in arrays]
    d_y = torch.zeros((n + 1, 4), dtype=torch.int64, device="cuda")
    lens = np.array(ll, dtype=np.uint8)
    for device in (False, True):
        base = [t.data_ptr() for t in d_arrays] if device else [a.ctypes.data for a in h_arrays]
        out = d_y.data_ptr() if device else y.ctypes.data
        fn = lib.blsgpu_fr_expr_eval_device if device else lib.blsgpu_fr_expr_eval

        def call(handle=e.handle, cols=base, col_log_len=lens, ln=log_n, ls=EDGE_STRIDE, o=out, ctx_h=h, no_cols=False):
            arr = (ctypes.c_void_p * 5)(*cols)
            return fn(ctx_h, handle, None if no_cols else arr, None if col_log_len is None else col_log_len.ctypes.data_as(ctypes.c_void_p), ln, ls, ctypes.c_void_p(o) if o else None)

        swap = lambda j, v: base[:j] + [v] + base[j + 1:]
        assert call(ctx_h=None) == ERR_ARG and "context" in err()
        assert call(handle=None) == ERR_ARG and "handle" in err()
        assert call(no_cols=True) == ERR_ARG and "NULL" in err()
        assert call(o=None) == ERR_ARG and "NULL" in err()
        assert call(cols=swap(2, None)) == ERR_ARG and "NULL" in err()
        assert call(ln=-1) == ERR_ARG and "log_n" in err()
        assert call(ln=29) == ERR_ARG and "log_n" in err()
        assert call(ls=-1) == ERR_ARG and "log_stride" in err()
        assert call(ls=log_n + 1) == ERR_ARG and "log_stride" in err()
        assert call(col_log_len=np.array([log_n, log_n, log_n + 1, 2, 0], dtype=np.uint8)) == ERR_ARG and "col_log_len" in err()
        assert call(col_log_len=np.array([log_n, log_n, log_n, 2, 255], dtype=np.uint8)) == ERR_ARG and "col_log_len" in err()
        assert call(o=base[1]) == ERR_ARG and "overlap" in err()                        # out is a column
        assert call(o=base[0] + (n - 1) * 32) == ERR_ARG and "overlap" in err()         # out starts at a column's last scalar
        assert call(cols=swap(4, out + (n - 1) * 32)) == ERR_ARG and "overlap" in err() # the length-1 column is out's last scalar
        assert call(cols=swap(4, out + n * 32)) == 0                                    # ... right behind out is fine
        if device:
            assert call(o=out + 8) == ERR_ARG and "aligned" in err()
            assert call(cols=swap(1, base[1] + 8)) == ERR_ARG and "aligned" in err()
        ctx.synchronize()
    # nothing was written by a refused call: repeat the refusals on a zeroed out and look
    d_y.zero_()
    y[:] = 0
    torch.cuda.synchronize()
    assert lib.blsgpu_fr_expr_eval_device(h, e.handle, (ctypes.c_void_p * 5)(*[t.data_ptr() for t in d_arrays]), lens.ctypes.data_as(ctypes.c_void_p), log_n, log_n + 1,
                                          ctypes.c_void_p(d_y.data_ptr())) == ERR_ARG
    assert lib.blsgpu_fr_expr_eval(h, e.handle, (ctypes.c_void_p * 5)(*[a.ctypes.data for a in h_arrays]), lens.ctypes.data_as(ctypes.c_void_p), 29, 0,
                                   ctypes.c_void_p(y.ctypes.data)) == ERR_ARG
    ctx.synchronize()
    assert not y.any() and not d_y.cpu().numpy().any()
    # a column that is not read may be NULL with any length; the valid call succeeds
    e2 = ctx.fr_expr(3, 1, None, [("ADD", 0, ("col", 0), ("col", 2))])
    assert e2.cols_read == 5
    got = e2.eval([arrays[0], None, arrays[1]], log_n, 0, [log_n, 99, log_n])
    assert np.array_equal(got, ctx.fr_op(1, arrays[0], arrays[1]))
    assert np.array_equal(e.eval(arrays, log_n, EDGE_STRIDE, ll), want)
    with pytest.raises(ValueError):
        e.eval(arrays[:4], log_n, EDGE_STRIDE, ll)
    e.close()
    e2.close()


def test_cpp_mirror(ctx, tmp_path):
    """include/bls12_381.hpp FrExpr compiled with g++ against libblsgpu.so: a program with every op against host loops over bls::fr_op"""
    import bls12_381_amd as b
    exe = str(tmp_path / "fr_expr_test")
    libdir = os.path.dirname(b.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "fr_expr_test.cpp"),
                           "-L" + libdir, "-lblsgpu", "-Wl,-rpath," + libdir, "-o", exe])
    out = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "fr_expr ok" in out.stdout, out.stdout + out.stderr
