"""Fr fraction scans (`blsgpu_fr_grand_product*`, `blsgpu_fr_frac_sum*`; csrc/fr_frac.hip.h + csrc/fr_frac_plan.h) on the GPU.

Three kinds of expectation: Python integers mod r (tests/fr_frac_ref.py, the defining formulas), the composed route on the device
(constant-filled arrays, `fr_op_device`, `fr_batch_invert_device`, `fr_scan_device` -- limb-identical, flags included), and two
identities that need no reference at all: the grand product of a permutation with copy cycles ends in 1, the logUp sum of a lookup
instance ends in 0, and neither survives a broken wire or multiplicity."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import fr_frac_ref as ref
from bls12_381_amd import synthetic
from oracle import bls12_381_ref as o

pytestmark = pytest.mark.gpu

RR = ref.RR
MONT = ref.MONT
RINV = pow(MONT, -1, RR)
ERR_ARG = -2
GP, FS = 0, 1
MUL, ADD = 0, 1                                                    # blsgpu_fr_op
SUM, PRODUCT = 0, 1                                                # blsgpu_fr_scan_many


def tile(op, c):
    """csrc/fr_frac_plan.h frf_shape: 256 lanes x 4 elements, x 2 for the fraction sum above four columns"""
    return 256 * (2 if op == FS and c > 4 else 4)


@pytest.fixture(scope="module")
def ctx():
    import bls12_381_amd as b
    c = b.Context(0)
    yield c
    c.close()


def limbs(vals):
    return np.ascontiguousarray(ref.mont_words(vals)).view(np.uint64).reshape(-1, 4).copy()


def set_limbs(tables):
    """a column set of integers -> (c, k, len, 4) u64"""
    c, k, n = len(tables), len(tables[0]), len(tables[0][0])
    return limbs([x for t in tables for row in t for x in row]).reshape(c, k, n, 4)


def out_limbs(rows):
    return limbs([x for row in rows for x in row]).reshape(len(rows), len(rows[0]), 4)


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


# ---- against Python integers ---------------------------------------------------------------------------------------------------------
def _int_case(n, k, c, seed):
    """sets with 0, 1 and r - 1 at the row ends and in the middle, and zero denominators in ONE column at the first, a middle and the last
    element of a row"""
    rng = o.SplitMix64(seed)
    beta, gamma = rng.scalar(), rng.scalar()
    mk = lambda: [[[rng.scalar() for _ in range(n)] for _ in range(k)] for _ in range(c)]
    xa, xb, da, db = mk(), mk(), mk(), mk()
    special = (0, 1, RR - 1)
    for s_i, s in enumerate((xa, xb, da, db)):
        for j in range(c):
            for v in range(min(k, 4)):
                s[j][v][0] = special[(s_i + j + v) % 3]
                s[j][v][-1] = special[(s_i + j + v + 1) % 3]
                s[j][v][n // 2] = special[(s_i + j + v + 2) % 3]
    v = 1 if k > 1 else 0
    zeros = sorted({0, n // 2, n - 1}) if n >= 3 else [0]
    for i in zeros:
        da[c - 1][v][i] = -(beta * db[c - 1][v][i] + gamma) % RR
    return beta, gamma, xa, xb, da, db, v, zeros


@pytest.mark.parametrize("n,k,c", [(1, 5, 1), (63, 40, 3), (100, 33, 2), (tile(GP, 3) + 1, 3, 3), (4096, 4, 8)])
def test_against_python_integers(ctx, n, k, c):
    """both operations, both forms, through the HOST entry points: limb equality at every position, exact flags; the product row with the
    zero is zero from there on and the next row is not"""
    beta, gamma, xa, xb, da, db, zv, zeros = _int_case(n, k, c, 11 * n + k + c)
    A, B, DA, DB = set_limbs(xa), set_limbs(xb), set_limbs(da), set_limbs(db)
    for ex in (False, True):
        want, wflags = ref.grand_product(xa, xb, da, db, beta, gamma, ex)
        got, flags = ctx.fr_grand_product(A, B, DA, DB, beta, gamma, exclusive=ex, return_flags=True)
        bad = np.argwhere((got != out_limbs(want)).any(axis=2))
        assert not len(bad), "grand product ex=%s: %d elements differ, first (row, index) %s" % (ex, len(bad), bad[0])
        assert np.array_equal(flags, np.array(wflags, dtype=np.uint8))
        assert not got[zv, zeros[0] + (1 if ex else 0):].any() and (k == 1 or got[(zv + 1) % k].any(axis=1).all())
        want, wflags = ref.frac_sum(xa, da, db, beta, gamma, ex)
        got, flags = ctx.fr_frac_sum(A, DA, DB, beta, gamma, exclusive=ex, return_flags=True)
        bad = np.argwhere((got != out_limbs(want)).any(axis=2))
        assert not len(bad), "fraction sum ex=%s: %d elements differ, first (row, index) %s" % (ex, len(bad), bad[0])
        assert np.array_equal(flags, np.array(wflags, dtype=np.uint8))
        assert int(flags.sum()) == n * k - len(zeros)
    # NULL sets, limb-form challenges, a (c, len, 4) array as k = 1
    want, _ = ref.grand_product(xa, None, da, None, beta, gamma)
    assert np.array_equal(ctx.fr_grand_product(A, None, DA, None, limbs([beta])[0], limbs([gamma])[0]), out_limbs(want))
    want, _ = ref.frac_sum(None, da, None, beta, gamma)
    assert np.array_equal(ctx.fr_frac_sum(None, DA, None, beta, gamma), out_limbs(want))
    assert np.array_equal(ctx.fr_frac_sum(A[:, 0], DA[:, 0], DB[:, 0], beta, gamma), ctx.fr_frac_sum(A[:, :1], DA[:, :1], DB[:, :1], beta, gamma)[0])


# ---- against the composed route on the device ----------------------------------------------------------------------------------------
class Composed:
    """the same columns from the entry points the library had before: constant-filled arrays for beta and gamma, fr_op_device for every
    factor, fr_batch_invert_device, fr_scan_device"""

    def __init__(self, ctx, total, chal_raw):
        import torch
        self.ctx, self.total = ctx, total
        self.beta = dev(np.repeat(chal_raw[0:1], total, axis=0))
        self.gamma = dev(np.repeat(chal_raw[1:2], total, axis=0))
        z = lambda: torch.zeros((total, 4), dtype=torch.int64, device="cuda")
        self.t, self.num, self.den, self.inv = z(), z(), z(), z()
        self.flags = torch.zeros(total, dtype=torch.uint8, device="cuda")
        self.flags_j = torch.zeros(total, dtype=torch.uint8, device="cuda")

    def factor(self, d_a, d_b, j, pitch, dst):
        """dst = a_j + beta b_j + gamma"""
        op, n, off = self.ctx.fr_op_device, self.total, j * pitch * 32
        if d_b is not None:
            op(MUL, self.beta.data_ptr(), d_b.data_ptr() + off, n, dst.data_ptr())
            op(ADD, dst.data_ptr(), d_a.data_ptr() + off, n, dst.data_ptr())
            op(ADD, dst.data_ptr(), self.gamma.data_ptr(), n, dst.data_ptr())
        else:
            op(ADD, d_a.data_ptr() + off, self.gamma.data_ptr(), n, dst.data_ptr())

    def grand_product(self, c, d_na, d_nb, d_da, d_db, pitch, n, k, d_out, exclusive):
        op, tot = self.ctx.fr_op_device, self.total
        for j in range(c):
            for acc, d_a, d_b in ((self.num, d_na, d_nb), (self.den, d_da, d_db)):
                self.factor(d_a, d_b, j, pitch, self.t if j else acc)
                if j:
                    op(MUL, acc.data_ptr(), self.t.data_ptr(), tot, acc.data_ptr())
        self.ctx.fr_batch_invert_device(self.den.data_ptr(), tot, self.inv.data_ptr(), self.flags.data_ptr())
        op(MUL, self.num.data_ptr(), self.inv.data_ptr(), tot, d_out.data_ptr())
        self.ctx.fr_scan_device(PRODUCT, d_out.data_ptr(), n, k, d_out.data_ptr(), exclusive=exclusive)

    def frac_sum(self, c, d_m, d_da, d_db, pitch, n, k, d_out, exclusive):
        """the flags of the columns are combined with torch between the calls (the composed route has no call for it)"""
        import torch
        op, tot = self.ctx.fr_op_device, self.total
        self.ctx.synchronize()
        self.flags.fill_(1)
        torch.cuda.synchronize()
        for j in range(c):
            term = self.inv if j else self.num
            self.factor(d_da, d_db, j, pitch, self.t)
            self.ctx.fr_batch_invert_device(self.t.data_ptr(), tot, term.data_ptr(), self.flags_j.data_ptr())
            if d_m is not None:
                op(MUL, d_m.data_ptr() + j * pitch * 32, term.data_ptr(), tot, term.data_ptr())
            if j:
                op(ADD, self.num.data_ptr(), term.data_ptr(), tot, self.num.data_ptr())
            self.ctx.synchronize()
            self.flags.mul_(self.flags_j)
            torch.cuda.synchronize()
        self.ctx.fr_scan_device(SUM, self.num.data_ptr(), n, k, d_out.data_ptr(), exclusive=exclusive)


def _raw_sets(c, total, pitch, seed, chal, zeros, null_b):
    """four raw column sets of (c - 1) * pitch + total scalars; at the flat positions `zeros` the denominator factor of column c - 1 is zero"""
    reach = (c - 1) * pitch + total
    xa, xb, da, db = (raw(reach, seed + i) for i in range(4))
    beta, gamma = ref.raw_ints(chal.view(np.uint32))
    off = (c - 1) * pitch
    for p in zeros:
        b = 0 if null_b else ref.raw_ints(db[off + p].view(np.uint32))[0]
        v = -(beta * b * RINV + gamma) % RR                        # raw limbs: a Montgomery product is a b / R
        da[off + p] = np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint64)
    return xa, xb, da, db


def _compare_with_composed(ctx, c, n, k, seed, pitch=None, null_b=False):
    import torch
    total = n * k
    pitch = pitch or total
    chal = raw(2, seed + 100)
    zeros = sorted({0, total - 1, total // 2, n - 1, n, 1023, 1024, 1025} & set(range(total)))
    xa, xb, da, db = _raw_sets(c, total, pitch, seed, chal, zeros, null_b)
    d_xa, d_xb, d_da, d_db, d_chal = dev(xa), None if null_b else dev(xb), dev(da), None if null_b else dev(db), dev(chal)
    z = lambda: torch.zeros((total, 4), dtype=torch.int64, device="cuda")
    d_out, d_want = z(), z()
    d_flags = torch.zeros(total, dtype=torch.uint8, device="cuda")
    comp = Composed(ctx, total, chal)
    torch.cuda.synchronize()
    P = lambda t: None if t is None else t.data_ptr()
    for ex in (False, True):
        d_flags.fill_(7)
        torch.cuda.synchronize()
        ctx.fr_grand_product_device(c, P(d_xa), P(d_xb), P(d_da), P(d_db), pitch, P(d_chal), n, k, P(d_out), P(d_flags), exclusive=ex)
        comp.grand_product(c, d_xa, d_xb, d_da, d_db, pitch, n, k, d_want, ex)
        ctx.synchronize()
        assert torch.equal(d_out, d_want), "grand product ex=%s" % ex
        assert torch.equal(d_flags, comp.flags) and int(d_flags.sum()) == total - len(zeros)
        d_flags.fill_(7)
        torch.cuda.synchronize()
        ctx.fr_frac_sum_device(c, P(d_xa), P(d_da), P(d_db), pitch, P(d_chal), n, k, P(d_out), P(d_flags), exclusive=ex)
        comp.frac_sum(c, d_xa, d_da, d_db, pitch, n, k, d_want, ex)
        ctx.synchronize()
        assert torch.equal(d_out, d_want), "fraction sum ex=%s" % ex
        assert torch.equal(d_flags, comp.flags) and int(d_flags.sum()) == total - len(zeros)
    for d, a in ((d_xa, xa), (d_da, da)):
        assert np.array_equal(host(d), a), "an input was written to"


@pytest.mark.parametrize("n,k", [(1 << 20, 1), (1000, 1048)])
def test_against_the_composed_route(ctx, n, k):
    """c = 3 over about 2^20 elements, one long row and 1048 rows of 1000: limb-identical outputs and flags, zero denominators at both
    ends, at row ends and on either side of a tile boundary"""
    _compare_with_composed(ctx, 3, n, k, 5 + k)


def test_the_second_aggregate_level(ctx):
    """c = 1 and one element more than tile^2: more tiles than one workgroup scans, so k_frs_agg runs at both levels over fused output"""
    t = tile(GP, 1)
    _compare_with_composed(ctx, 1, (t * t + 7) // 7, 7, 31)
    _compare_with_composed(ctx, 1, t * t + 1, 1, 32, null_b=True)


def test_pitch_above_the_table_size(ctx):
    """tables 4099 scalars apart over 3 x 1000 elements: what lies between them reaches no result (the composed route reads the same
    addresses, the integer reference knows only the tables)"""
    _compare_with_composed(ctx, 3, 1000, 3, 77, pitch=4099)
    n, k, c, pitch = 50, 3, 2, 200
    beta, gamma, xa, xb, da, db, _, _ = _int_case(n, k, c, 3)
    pk = lambda s: np.ascontiguousarray(ref.pack_set(s, pitch, poison=0xBAD)).view(np.uint64)
    import torch
    d = [dev(pk(s)) for s in (xa, xb, da, db)]
    d_chal, d_out = dev(limbs([beta, gamma])), torch.zeros((k * n, 4), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.fr_grand_product_device(c, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), pitch, d_chal.data_ptr(), n, k, d_out.data_ptr())
    ctx.synchronize()
    assert np.array_equal(host(d_out).reshape(k, n, 4), out_limbs(ref.grand_product(xa, xb, da, db, beta, gamma)[0]))


# ---- identities -----------------------------------------------------------------------------------------------------------------------
def test_a_permutation_with_copy_cycles_multiplies_to_one(ctx):
    """c = 3 wire columns of 2^12 rows, constant on every cycle of sigma, id_j[i] = 7^j w^i: the inclusive grand product ends in the limbs
    of 1 with every flag set -- and no longer once one wire is changed"""
    wires, ids, sigmas = synthetic.permutation_with_copy_cycles(3, 12, 2024)
    assert sum(1 for j in range(3) for i in range(1 << 12) if sigmas[j][i] != ids[j][i]) > 1 << 12
    W, I, S = (set_limbs([[col] for col in s]) for s in (wires, ids, sigmas))
    beta, gamma = 0x1234567890ABCDEF, 0xFEDCBA0987654321
    z, flags = ctx.fr_grand_product(W, I, W, S, beta, gamma, return_flags=True)       # num_a is den_a: the very same array
    assert flags.all() and np.array_equal(z[0, -1], limbs([1])[0])
    assert not np.array_equal(z[0, (1 << 11) - 1], limbs([1])[0])                     # ... and only the full product does
    ze = ctx.fr_grand_product(W, I, W, S, beta, gamma, exclusive=True)
    assert np.array_equal(ze[0, 0], limbs([1])[0]) and np.array_equal(ze[0, 1:], z[0, :-1])
    broken = [list(col) for col in wires]
    broken[1][77] = (broken[1][77] + 1) % RR
    Wb = set_limbs([[col] for col in broken])
    assert not np.array_equal(ctx.fr_grand_product(Wb, I, Wb, S, beta, gamma)[0, -1], limbs([1])[0])


def test_a_lookup_sums_to_zero(ctx):
    """logUp: f drawn from the table t with multiplicities m, two columns (f, t) with mult = (1, -m): the inclusive sum ends in 0 -- and no
    longer once one multiplicity is changed"""
    n = 1 << 12
    f, t, m = synthetic.lookup_instance(n, 7)
    assert max(m) > 1 and min(m) == 0
    gamma = 0x0123456789ABCDEF0123
    den = set_limbs([[f], [t]])
    mult = lambda mm: set_limbs([[[1] * n], [[-x % RR for x in mm]]])
    h, flags = ctx.fr_frac_sum(mult(m), den, None, 0, gamma, return_flags=True)
    assert flags.all() and not h[0, -1].any() and h[0, n // 2].any()
    m2 = list(m)
    m2[m.index(max(m))] += 1
    assert ctx.fr_frac_sum(mult(m2), den, None, 0, gamma)[0, -1].any()


# ---- streams, transcripts --------------------------------------------------------------------------------------------------------------
def test_on_a_caller_stream_and_between_pipelined_msm_calls(ctx):
    """the device forms on a non-default stream set with set_stream, then enqueued between two pipelined msm_device calls"""
    import torch
    k, n, c = 7, 3000, 2
    rng = o.SplitMix64(99)
    beta, gamma = rng.scalar(), rng.scalar()
    sets = [raw(c * k * n, 60 + i).reshape(c, k, n, 4) for i in range(4)]
    want_p = ctx.fr_grand_product(sets[0], sets[1], sets[2], sets[3], beta, gamma, exclusive=True).reshape(-1, 4)      # the host forms: checked above
    want_s = ctx.fr_frac_sum(sets[0], sets[2], sets[3], beta, gamma).reshape(-1, 4)
    d_chal = dev(limbs([beta, gamma]))

    def buffers():
        return [dev(s) for s in sets] + [torch.zeros((k * n, 4), dtype=torch.int64, device="cuda") for _ in range(2)]

    def enqueue(a, b, da, db, d_p, d_s):
        ctx.fr_grand_product_device(c, a.data_ptr(), b.data_ptr(), da.data_ptr(), db.data_ptr(), k * n, d_chal.data_ptr(), n, k, d_p.data_ptr(), exclusive=True)
        ctx.fr_frac_sum_device(c, a.data_ptr(), da.data_ptr(), db.data_ptr(), k * n, d_chal.data_ptr(), n, k, d_s.data_ptr())

    def check(a, b, da, db, d_p, d_s):
        assert np.array_equal(host(d_p), want_p) and np.array_equal(host(d_s), want_s)
        assert np.array_equal(host(a), sets[0]) and np.array_equal(host(da), sets[2]), "an input was written to"

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
        want = ctx.batch_normalize(1, ctx.msm(bases, S[i * m:(i + 1) * m])[None, :])
        assert np.array_equal(got[0][i], want[0][0]) and got[1][i] == want[1][0], i
    bases.free()


def test_challenges_written_by_the_previous_call(ctx):
    """beta and gamma are two Poseidon digests that hash_many_device writes straight into the challenges buffer, the fraction scans are
    enqueued behind it with no synchronisation: the results equal the host forms fed the digests read back afterwards"""
    import torch
    c, k, n = 3, 2, 700
    t, rf, rp = 3, 8, 57
    consts, mds = synthetic.poseidon_test_params(t, rf, rp, 1)
    h = ctx.fr_poseidon(t, rf, rp, consts, mds)
    sets = [raw(c * k * n, 80 + i).reshape(c, k, n, 4) for i in range(4)]
    d = [dev(s) for s in sets]
    d_pre = dev(raw(4, 9))                                         # two preimages of two scalars
    d_chal = torch.zeros((2, 4), dtype=torch.int64, device="cuda")
    d_p, d_s = (torch.zeros((k * n, 4), dtype=torch.int64, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    h.hash_many_device(d_pre.data_ptr(), 2, d_chal.data_ptr(), tag=5)
    ctx.fr_grand_product_device(c, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), k * n, d_chal.data_ptr(), n, k, d_p.data_ptr())
    ctx.fr_frac_sum_device(c, d[0].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), k * n, d_chal.data_ptr(), n, k, d_s.data_ptr())
    ctx.synchronize()
    chal = host(d_chal)
    assert chal.any(axis=1).all() and not np.array_equal(chal[0], chal[1])
    assert np.array_equal(host(d_p).reshape(k, n, 4), ctx.fr_grand_product(sets[0], sets[1], sets[2], sets[3], chal[0], chal[1]))
    assert np.array_equal(host(d_s).reshape(k, n, 4), ctx.fr_frac_sum(sets[0], sets[2], sets[3], chal[0], chal[1]))
    h.close()


# ---- arguments ------------------------------------------------------------------------------------------------------------------------
def test_arguments(ctx):
    """every refusal is BLSGPU_ERR_ARG with a text naming the cause, before anything is staged or launched: nothing is written to out or
    flags, and the context works afterwards; k == 0 and len == 0 are no-ops"""
    import torch
    lib, h = ctx.lib, ctx.h
    n, k, c = 16, 2, 2
    tot = n * k
    sets = [raw(c * tot + 4, 1 + i) for i in range(4)]
    chal = raw(2, 9)
    y = np.zeros((tot, 4), dtype=np.uint64)
    fl = np.zeros(tot, dtype=np.uint8)
    d_sets = [dev(s) for s in sets]
    d_chal = dev(chal)
    d_y = torch.zeros((tot, 4), dtype=torch.int64, device="cuda")
    d_fl = torch.zeros(tot + 64, dtype=torch.uint8, device="cuda")
    cp = lambda a, off=0: ctypes.c_void_p(a.ctypes.data + off)
    dp = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    err = lambda: lib.blsgpu_last_error().decode()
    # one calling convention for the four entry points: (op, device, ex, c, xa, xb, da, db, pitch, chal, len, k, out, flags)
    def call(op, device, ex, cc, xa, xb, da, db, pitch, ch, ln, kk, out, flags):
        if op == GP:
            if device:
                return lib.blsgpu_fr_grand_product_device(h, ex, cc, xa, xb, da, db, pitch, ch, ln, kk, out, flags)
            return lib.blsgpu_fr_grand_product(h, ex, cc, xa, xb, da, db, ch, ln, kk, out, flags)
        if device:
            return lib.blsgpu_fr_frac_sum_device(h, ex, cc, xa, da, db, pitch, ch, ln, kk, out, flags)
        return lib.blsgpu_fr_frac_sum(h, ex, cc, xa, da, db, ch, ln, kk, out, flags)
    for op in (GP, FS):
        for device in (False, True):
            p = [dp(t) for t in d_sets] if device else [cp(s) for s in sets]
            at = (lambda i, off: dp(d_sets[i], off)) if device else (lambda i, off: cp(sets[i], off))
            ch, out, flags = (dp(d_chal), dp(d_y), dp(d_fl)) if device else (cp(chal), cp(y), cp(fl))
            good = lambda **kw: call(op, device, *[kw.get(name, dflt) for name, dflt in (("ex", 0), ("c", c), ("xa", p[0]), ("xb", p[1]), ("da", p[2]), ("db", p[3]), ("pitch", tot),
                                                                                         ("chal", ch), ("len", n), ("k", k), ("out", out), ("flags", flags))])
            assert good(c=0) == ERR_ARG and "[1, 8]" in err()
            assert good(c=9) == ERR_ARG and "[1, 8]" in err()
            assert good(ex=2) == ERR_ARG and "exclusive" in err()
            assert good(ex=-1) == ERR_ARG and "exclusive" in err()
            assert good(da=None) == ERR_ARG and "NULL" in err()
            assert good(chal=None) == ERR_ARG and "NULL" in err()
            assert good(out=None) == ERR_ARG and "NULL" in err()
            if op == GP:
                assert good(xa=None) == ERR_ARG and "NULL" in err()
            assert good(len=(1 << 28) + 1, k=1) == ERR_ARG and "2^28" in err()
            assert good(len=1 << 27, k=2, c=2, pitch=1 << 28) == ERR_ARG and "2^28" in err()           # (c - 1) * pitch + k * len
            assert good(len=(1 << 63) + 5, k=2) == ERR_ARG and "2^28" in err()          # k * len overflows 64 bits
            assert good(len=(1 << 64) - 1, k=(1 << 64) - 1) == ERR_ARG and "2^28" in err()
            assert good(out=at(2, 32)) == ERR_ARG and "overlap" in err()                # out inside den_a
            assert good(out=at(0, (c * tot - 1) * 32)) == ERR_ARG and "overlap" in err()      # out starts at the last scalar of table c - 1
            assert good(flags=at(3, 5)) == ERR_ARG and "overlap" in err()
            assert good(flags=ctypes.c_void_p(out.value + 3)) == ERR_ARG and "overlap" in err()
            assert good(k=0) == 0 and good(len=0) == 0 and good(k=0, len=0, da=None, xa=None, out=None, chal=None) == 0
            if device:
                assert good(pitch=tot - 1) == ERR_ARG and "pitch" in err()
                assert good(pitch=1 << 28) == ERR_ARG and "2^28" in err()
                assert good(pitch=(1 << 64) - 1) == ERR_ARG and "2^28" in err()
                for name, ptr in (("xa", at(0, 8)), ("da", at(2, 8)), ("db", at(3, 8)), ("chal", dp(d_chal, 8)), ("out", dp(d_y, 8))):
                    assert good(**{name: ptr}) == ERR_ARG and "aligned" in err(), name
                if op == GP:
                    assert good(xb=at(1, 8)) == ERR_ARG and "aligned" in err()
    ctx.synchronize()
    assert not y.any() and not fl.any() and not d_y.cpu().numpy().any() and not d_fl.cpu().numpy().any()
    for i in range(4):
        assert np.array_equal(host(d_sets[i]), sets[i])
    # the context is still usable; unaligned flags; empty calls through the Python forms
    A, B, DA, DB = (s[:c * tot].reshape(c, k, n, 4) for s in sets)
    want, wf = ctx.fr_grand_product(A, B, DA, DB, chal[0], chal[1], return_flags=True)
    ctx.fr_grand_product_device(c, d_sets[0].data_ptr(), d_sets[1].data_ptr(), d_sets[2].data_ptr(), d_sets[3].data_ptr(), tot, d_chal.data_ptr(), n, k, d_y.data_ptr(),
                                d_fl.data_ptr() + 3)
    ctx.synchronize()
    assert np.array_equal(host(d_y).reshape(k, n, 4), want) and np.array_equal(d_fl.cpu().numpy()[3:3 + tot].reshape(k, n), wf)
    assert ctx.fr_grand_product(np.zeros((2, 0, 5, 4), dtype=np.uint64), None, np.zeros((2, 0, 5, 4), dtype=np.uint64), None, 1, 2).shape == (0, 5, 4)
    assert ctx.fr_frac_sum(None, np.zeros((1, 3, 0, 4), dtype=np.uint64), None, 1, 2).shape == (3, 0, 4)
    with pytest.raises(ValueError):
        ctx.fr_grand_product(A, B[:1], DA, DB, 1, 2)
    with pytest.raises(ValueError):
        ctx.fr_frac_sum(None, np.zeros((2, 3, 5), dtype=np.uint64), None, 1, 2)


def test_cpp_mirror(ctx, tmp_path):
    """include/bls12_381.hpp fr_grand_product / fr_frac_sum compiled with g++ against libblsgpu.so: both against host loops over
    bls::fr_op and bls::fr_scan"""
    import bls12_381_amd as b
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "fr_frac_test")
    libdir = os.path.dirname(b.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "fr_frac_test.cpp"),
                           "-L" + libdir, "-lblsgpu", "-Wl,-rpath," + libdir, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "fr_frac ok" in out.stdout, out.stdout + out.stderr
