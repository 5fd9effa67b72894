"""Fr scans and batch inversion (`blsgpu_fr_scan_many*`, `blsgpu_fr_batch_invert*`; csrc/fr_scan.hip.h + csrc/fr_scan_plan.h) on the GPU.

Expectations are Python integers mod r (the defining recurrences), compared limb for limb.  The arithmetic runs on the RAW limbs where
that is exact: a `Scalar`'s limbs are a = v R mod r, sums and Horner rows are linear in them (out_raw[i] = a[i] + z out_raw[i+1] with z the
point's VALUE), and a product of Montgomery forms is out_raw[i] = out_raw[i-1] a[i] / R.  The larger calls are checked by their row totals,
by the recurrence on 64 positions of the device output itself, and against the existing element-wise path (`ctx.fr_op`)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import bls12_381_ref as o

pytestmark = pytest.mark.gpu

RR = o.R_ORDER
MONT = o.FR_MONT_R
RINV = pow(MONT, -1, RR)
ERR_ARG = -2
SUM, PRODUCT, HORNER = 0, 1, 2
BLOCK, CHUNK = 256, 8                                              # csrc/fr_scan_plan.h: FRS_BLOCK, FRS_CHUNK
T = BLOCK * CHUNK                                                  # the tile; more than T tiles take the second aggregate level


@pytest.fixture(scope="module")
def ctx():
    import bls12_381_amd as b
    assert (b.FR_SCAN_SUM, b.FR_SCAN_PRODUCT, b.FR_SCAN_HORNER) == (SUM, PRODUCT, HORNER)
    c = b.Context(0)
    yield c
    c.close()


def _limbs(vals):
    """integers mod r -> (len, 4) u64 Montgomery limbs"""
    b = b"".join((int(v) % RR * MONT % RR).to_bytes(32, "little") for v in vals)
    return np.frombuffer(b, dtype=np.uint64).reshape(-1, 4).copy()


def _from_raw(ints):
    """raw limb integers -> (len, 4) u64"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in ints), dtype=np.uint64).reshape(-1, 4).copy()


def _raw(n, seed):
    """n canonical `Scalar`s as raw limbs (any integer below r is the Montgomery form of some scalar)"""
    s = np.random.RandomState(seed).randint(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= 0x3F                                               # < 2^254 < r
    return s.view(np.uint64).reshape(n, 4).copy()


def _raw_ints(a):
    b = np.ascontiguousarray(a).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def _scan_raw(op, rows, zs=None, exclusive=False):
    """the scan of rows of RAW limb integers, as raw limb integers (z: the points' values)"""
    out = []
    for v, row in enumerate(rows):
        n = len(row)
        res = [0] * n
        if op == HORNER:
            acc, z = 0, zs[v]
            for i in range(n - 1, -1, -1):
                acc = (row[i] + z * acc) % RR
                res[i] = acc
        elif op == SUM:
            acc = 0
            for i in range(n):
                res[i] = acc if exclusive else (acc + row[i]) % RR
                acc = (acc + row[i]) % RR
        else:
            acc = MONT % RR                                        # the raw limbs of 1
            for i in range(n):
                nxt = acc * row[i] % RR * RINV % RR
                res[i] = acc if exclusive else nxt
                acc = nxt
        out.append(res)
    return out


def _special(x, k, n):
    """0, 1 and r - 1 among the rows' elements, at both ends of a row"""
    vals = (0, MONT % RR, (RR - 1) * MONT % RR)
    for i in range(min(k, 6)):
        x[i * n + (0 if i % 2 == 0 else n - 1)] = vals[i % 3]
    return x


@pytest.mark.parametrize("n,k", [(1, 5), (63, 1000), (100, 333), (T + 1, 3), (4096, 16), (2 * T * 64 + 7, 1)])
def test_against_python_integers(ctx, n, k):
    """every op, the exclusive forms included, limb equality at every position; a different point per row"""
    raw = _special(_raw_ints(_raw(n * k, 7 * n + k)), k, n)
    x = _from_raw(raw).reshape(k, n, 4)
    rows = [raw[v * n:(v + 1) * n] for v in range(k)]
    r = o.SplitMix64(n + k)
    zs = [(0, 1, RR - 1)[v] if v < 3 and k >= 3 else r.scalar() for v in range(k)]
    for op, ex in ((SUM, False), (SUM, True), (PRODUCT, False), (PRODUCT, True), (HORNER, False)):
        if op == PRODUCT and n > 4096:
            rows_op = [[a or 5 for a in row] for row in rows]      # a zero would hide everything behind it
            x_op = _from_raw([a for row in rows_op for a in row]).reshape(k, n, 4)
        else:
            rows_op, x_op = rows, x
        got = ctx.fr_scan(op, x_op, points=zs if op == HORNER else None, exclusive=ex)
        want = _from_raw([a for row in _scan_raw(op, rows_op, zs, ex) for a in row]).reshape(k, n, 4)
        bad = np.argwhere((got != want).any(axis=2))
        assert not len(bad), "op=%d exclusive=%s len=%d k=%d: %d elements differ, first (row, index) %s" % (op, ex, n, k, len(bad), bad[0])
    # the limb form of the points and the integer form are the same call; a (len, 4) array is k = 1
    assert np.array_equal(ctx.fr_scan(HORNER, x, points=_limbs(zs)), ctx.fr_scan(HORNER, x, points=zs))
    assert np.array_equal(ctx.fr_scan(SUM, x[0]), ctx.fr_scan(SUM, x[:1])[0])


@pytest.mark.parametrize("n", [1, T + 1, 1 << 16])
def test_batch_inversion_against_python_integers(ctx, n):
    raw = _raw_ints(_raw(n, 90 + n))
    for pos in (0, n - 1, n // 3, T - 1, T, 5 * T + 17):
        if pos < n and n > 1:
            raw[pos] = 0
    if n > 10:
        raw[5], raw[6] = MONT % RR, (RR - 1) * MONT % RR
    x = _from_raw(raw)
    got, flags = ctx.fr_batch_invert(x, return_flags=True)
    want = _from_raw([pow(a * RINV % RR, -1, RR) * MONT % RR if a else 0 for a in raw])
    assert np.array_equal(got, want)
    assert np.array_equal(flags, np.array([1 if a else 0 for a in raw], dtype=np.uint8))
    assert np.array_equal(ctx.fr_batch_invert(x), want)


def test_batch_inversion_equals_fr_op(ctx):
    """2^20 elements, one in 1000 of them zero: limb-identical to the exponentiation of fr_op op 4, equal flags"""
    n = 1 << 20
    x = _raw(n, 4)
    x[::1000] = 0
    got, flags = ctx.fr_batch_invert(x, return_flags=True)
    want, wflags = ctx.fr_op(4, x, return_flags=True)
    assert np.array_equal(got, want) and np.array_equal(flags, wflags)
    assert not got[::1000].any() and not flags[::1000].any() and flags.sum() == n - len(x[::1000])


@pytest.fixture(scope="module")
def big():
    """2^22 raw scalars (none of them zero), as an array and as Python integers: shared by the larger tests, never modified"""
    x = _raw(1 << 22, 2024)
    x[:, 0] |= 1
    return x, _raw_ints(x)


def _spots(total, count=64):
    return [int(p) for p in np.random.RandomState(total % 1000).randint(1, total - 1, size=count)]


def test_sum_and_product_at_2_22(ctx, big):
    """k = 4 and k = 1 over the same 2^22 scalars: every row total from ONE pass of Python integers (the k = 1 total is the combination
    of the four), and the defining recurrence at 64 positions of the device output"""
    x, raw = big
    total = len(raw)
    n4 = total // 4
    sums, prods = [], []
    for v in range(4):
        s, p = 0, 1
        for a in raw[v * n4:(v + 1) * n4]:
            s += a
            p = p * a % RR
        sums.append(s % RR)
        prods.append(p)                                            # the plain product of the raw limbs: raw total = p / R^(n - 1)
    for k in (4, 1):
        n = total // k
        got_s = ctx.fr_scan(SUM, x.reshape(k, n, 4))
        got_p = ctx.fr_scan(PRODUCT, x.reshape(k, n, 4))
        for v in range(k):
            ws = sums[v] if k == 4 else sum(sums) % RR
            wp = prods[v] if k == 4 else prods[0] * prods[1] * prods[2] * prods[3] % RR
            assert _raw_ints(got_s[v, n - 1])[0] == ws, (k, v)
            assert _raw_ints(got_p[v, n - 1])[0] == wp * pow(RINV, n - 1, RR) % RR, (k, v)
        fs, fp = got_s.reshape(-1, 4), got_p.reshape(-1, 4)
        for p in _spots(total):
            head = p % n == 0
            prev_s, prev_p = (0, MONT % RR) if head else (_raw_ints(fs[p - 1])[0], _raw_ints(fp[p - 1])[0])
            assert _raw_ints(fs[p])[0] == (prev_s + raw[p]) % RR, (k, p)
            assert _raw_ints(fp[p])[0] == prev_p * raw[p] % RR * RINV % RR, (k, p)


@pytest.mark.parametrize("k", [4, 1])
def test_horner_at_2_22(ctx, big, k):
    """out[v][0] = p_v(z_v) from one Horner pass in Python integers, a different point per row; out[i] == in[i] + z out[i+1] at 64 positions"""
    x, raw = big
    total = len(raw)
    n = total // k
    r = o.SplitMix64(k)
    zs = [r.scalar() for _ in range(k)]
    got = ctx.fr_scan(HORNER, x.reshape(k, n, 4), points=zs)
    for v in range(k):
        acc, z = 0, zs[v]
        for a in reversed(raw[v * n:(v + 1) * n]):
            acc = (a + z * acc) % RR
        assert _raw_ints(got[v, 0])[0] == acc, (k, v)
    flat = got.reshape(-1, 4)
    for p in _spots(total):
        nxt = 0 if p % n == n - 1 else _raw_ints(flat[p + 1])[0]
        assert _raw_ints(flat[p])[0] == (raw[p] + zs[p // n] * nxt) % RR, (k, p)


def test_the_second_aggregate_level(ctx, big):
    """more than T * T = 2^22 elements: more tiles than one workgroup scans, so the plan takes AGG_REDUCE and two AGG_SCANs
    (csrc/fr_scan_plan.h).  SUM (additions are cheap in Python), five rows that straddle the level's boundary: row totals, 64 recurrence
    positions, and the last element of the call"""
    x, raw = big
    k = 5
    n = (T * T + T + 9 + k - 1) // k
    total = k * n
    assert total > T * T and (total + T - 1) // T > T
    tail = _raw(total - len(raw), 99)
    data = np.concatenate([x, tail])
    ints = raw + _raw_ints(tail)
    got = ctx.fr_scan(SUM, data.reshape(k, n, 4))
    for v in range(k):
        assert _raw_ints(got[v, n - 1])[0] == sum(ints[v * n:(v + 1) * n]) % RR, v
    flat = got.reshape(-1, 4)
    for p in _spots(total) + [total - 1, T * T, T * T - 1, T * T + 1]:
        prev = 0 if p % n == 0 else _raw_ints(flat[p - 1])[0]
        assert _raw_ints(flat[p])[0] == (prev + ints[p]) % RR, p


def test_the_opening_chain_on_the_device(ctx):
    """a KZG opening with no host copy: 2^12 coefficients in device memory -> fr_scan_device(HORNER, z) -> msm_mont_device over [tau^i] G
    reading the len - 1 quotient coefficients at d_out + 32 bytes -> [q(tau)] G, and p(tau) - p(z) = q(tau) (tau - z) in integers"""
    import torch
    import bls12_381_amd as b
    n = 1 << 12
    r = o.SplitMix64(0x0BE9)
    coeff = [r.scalar() for _ in range(n)]
    z, tau = r.scalar(), r.scalar()
    ks = [pow(tau, i, RR) for i in range(n - 1)]
    h = _scan_raw(HORNER, [coeff], [z])[0]                         # on VALUES here: the same recurrence
    q, pz = h[1:], h[0]
    q_tau = sum(qi * ki for qi, ki in zip(q, ks)) % RR
    p_tau = sum(c * pow(tau, i, RR) for i, c in enumerate(coeff)) % RR
    assert (p_tau - pz) % RR == q_tau * (tau - z) % RR
    want = o.g1_to_uncompressed(o.g1_to_affine(o.g1_affine_mul(o.G1_GEN, q_tau)))
    dev = torch.device("cuda", 0)
    bases = ctx.bases_from_scalars(1, ks)
    d_c = torch.from_numpy(_limbs(coeff).view(np.int64)).to(dev)
    d_z = torch.from_numpy(_limbs([z]).view(np.int64)).to(dev)
    d_h = torch.zeros((n, 4), dtype=torch.int64, device=dev)
    d_out = torch.zeros(18, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ctx.fr_scan_device(HORNER, d_c.data_ptr(), n, 1, d_h.data_ptr(), d_points=d_z.data_ptr())
    ctx.msm_mont_device(bases, d_h.data_ptr() + 32, n - 1, d_out.data_ptr())
    ctx.synchronize()
    assert np.array_equal(d_h[0].cpu().numpy().view(np.uint64), _limbs([pz])[0])
    xy, inf = ctx.batch_normalize(1, d_out.cpu().numpy().view(np.uint64)[None, :])
    assert b.G1Affine(xy[0], bool(inf[0])).to_uncompressed() == want
    bases.free()


def test_the_grand_product_chain_on_the_device(ctx):
    """fr_batch_invert_device(den) -> fr_op_device(mul, num, .) -> fr_scan_device(PRODUCT, exclusive) over 8 x 1000: the columns
    z_0 = 1, z_{i+1} = z_i num_i / den_i of a permutation argument, from Python integers"""
    import torch
    k, n = 8, 1000
    r = o.SplitMix64(0x6A4D)
    num = [r.scalar() for _ in range(k * n)]
    den = [r.scalar() or 1 for _ in range(k * n)]
    want = []
    for v in range(k):
        acc = 1
        for i in range(n):
            want.append(acc)
            acc = acc * num[v * n + i] % RR * pow(den[v * n + i], -1, RR) % RR
    dev = torch.device("cuda", 0)
    d_num = torch.from_numpy(_limbs(num).view(np.int64)).to(dev)
    d_den = torch.from_numpy(_limbs(den).view(np.int64)).to(dev)
    torch.cuda.synchronize()
    ctx.fr_batch_invert_device(d_den.data_ptr(), k * n, d_den.data_ptr())
    ctx.fr_op_device(0, d_num.data_ptr(), d_den.data_ptr(), k * n, d_den.data_ptr())
    ctx.fr_scan_device(PRODUCT, d_den.data_ptr(), n, k, d_den.data_ptr(), exclusive=True)
    ctx.synchronize()
    assert np.array_equal(d_den.cpu().numpy().view(np.uint64), _limbs(want))


def test_on_a_caller_stream_and_between_pipelined_msm_calls(ctx):
    """the device forms on a non-default stream set with set_stream, then enqueued between two pipelined msm_device calls"""
    import torch
    dev = torch.device("cuda", 0)
    k, n = 7, 3000
    x = _raw(k * n, 77)
    zs = [o.SplitMix64(5 + v).scalar() for v in range(k)]
    want_h = ctx.fr_scan(HORNER, x.reshape(k, n, 4), points=zs).reshape(-1, 4)      # the host form: checked against integers above
    want_i = ctx.fr_op(4, x)
    want_s = ctx.fr_scan(SUM, x.reshape(k, n, 4)).reshape(-1, 4)

    def buffers():
        return (torch.from_numpy(x.view(np.int64)).to(dev), torch.from_numpy(_limbs(zs).view(np.int64)).to(dev),
                torch.zeros((k * n, 4), dtype=torch.int64, device=dev), torch.zeros((k * n, 4), dtype=torch.int64, device=dev),
                torch.zeros((k * n, 4), dtype=torch.int64, device=dev))

    def enqueue(d_x, d_z, d_h, d_i, d_s):
        ctx.fr_scan_device(HORNER, d_x.data_ptr(), n, k, d_h.data_ptr(), d_points=d_z.data_ptr())
        ctx.fr_batch_invert_device(d_x.data_ptr(), k * n, d_i.data_ptr())
        ctx.fr_scan_device(SUM, d_x.data_ptr(), n, k, d_s.data_ptr())

    def check(d_x, d_z, d_h, d_i, d_s):
        for d, want in ((d_h, want_h), (d_i, want_i), (d_s, want_s), (d_x, x)):
            assert np.array_equal(d.cpu().numpy().view(np.uint64), want)

    side = torch.cuda.Stream(device=dev)
    bufs = buffers()
    torch.cuda.synchronize()
    ctx.set_stream(side.cuda_stream)
    try:
        enqueue(*bufs)
        ctx.synchronize()
    finally:
        ctx.set_stream(None)
    check(*bufs)
    # between pipelined MSM calls
    m = 1 << 14
    S = np.random.RandomState(5).randint(0, 256, size=(2 * m, 32), dtype=np.uint8)
    S[:, 31] &= 0x3F
    bases = ctx.bases_from_scalars(1, S[:m])
    d_s = torch.from_numpy(S).to(dev)
    d_msm = torch.zeros((2, 18), dtype=torch.int64, device=dev)
    bufs = buffers()
    torch.cuda.synchronize()
    ctx.set_pipelining(True)
    try:
        ctx.msm_device(bases, d_s[0:m].data_ptr(), m, d_msm[0].data_ptr())
        enqueue(*bufs)
        ctx.msm_device(bases, d_s[m:2 * m].data_ptr(), m, d_msm[1].data_ptr())
        ctx.join()
        ctx.synchronize()
    finally:
        ctx.set_pipelining(False)
    check(*bufs)
    got = ctx.batch_normalize(1, d_msm.cpu().numpy().view(np.uint64))
    for i in range(2):
        ref = ctx.batch_normalize(1, ctx.msm(bases, S[i * m:(i + 1) * m])[None, :])
        assert np.array_equal(got[0][i], ref[0][0]) and got[1][i] == ref[1][0], i
    bases.free()


def test_arguments(ctx):
    """every refusal is BLSGPU_ERR_ARG with a text naming the cause, before anything is staged or launched: nothing is written to input
    or output, and the context works afterwards; k == 0, len == 0 and n == 0 are no-ops"""
    import torch
    lib, h = ctx.lib, ctx.h
    n = 16
    x = _raw(2 * n, 1)
    y = np.zeros_like(x)
    z = _raw(2, 2)
    keep = x.copy()
    dev = torch.device("cuda", 0)
    d_x = torch.from_numpy(x.view(np.int64)).to(dev)
    d_y = torch.zeros((2 * n, 4), dtype=torch.int64, device=dev)
    d_z = torch.from_numpy(z.view(np.int64)).to(dev)
    cp = lambda a: ctypes.c_void_p(a.ctypes.data)
    dp = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    err = lambda: lib.blsgpu_last_error().decode()
    forms = ((lib.blsgpu_fr_scan_many, cp(x), cp(y), cp(z), lambda off: ctypes.c_void_p(x.ctypes.data + off)),
             (lib.blsgpu_fr_scan_many_device, dp(d_x), dp(d_y), dp(d_z), lambda off: dp(d_x, off)))
    for fn, pi, po, pz, at in forms:
        assert fn(h, 3, 0, pi, n, 2, pz, po) == ERR_ARG and "unknown op" in err()
        assert fn(h, -1, 0, pi, n, 2, pz, po) == ERR_ARG and "unknown op" in err()
        assert fn(h, HORNER, 1, pi, n, 2, pz, po) == ERR_ARG and "exclusive" in err()
        assert fn(h, HORNER, 0, pi, n, 2, None, po) == ERR_ARG and "points" in err()
        assert fn(h, SUM, 0, None, n, 2, None, po) == ERR_ARG and "NULL" in err()
        assert fn(h, SUM, 0, pi, n, 2, None, None) == ERR_ARG and "NULL" in err()
        assert fn(h, SUM, 0, pi, (1 << 28) + 1, 1, None, po) == ERR_ARG and "2^28" in err()
        assert fn(h, SUM, 0, pi, 1 << 27, 3, None, po) == ERR_ARG and "2^28" in err()
        assert fn(h, SUM, 0, pi, (1 << 63) + 5, 2, None, po) == ERR_ARG and "2^28" in err()      # k * len overflows 64 bits
        assert fn(h, SUM, 0, pi, (1 << 64) - 1, (1 << 64) - 1, None, po) == ERR_ARG and "2^28" in err()
        assert fn(h, SUM, 0, pi, n, 1, None, at(32)) == ERR_ARG and "overlap" in err()      # out one element inside in
        assert fn(h, PRODUCT, 0, at(n * 32 - 32), n, 1, None, pi) == ERR_ARG and "overlap" in err()
        assert fn(h, SUM, 0, pi, n, 0, None, po) == 0 and fn(h, SUM, 0, pi, 0, 2, None, po) == 0 and fn(h, HORNER, 0, None, 0, 0, None, None) == 0
    assert lib.blsgpu_fr_scan_many_device(h, SUM, 0, dp(d_x, 8), n, 1, None, dp(d_y)) == ERR_ARG and "aligned" in err()
    assert lib.blsgpu_fr_scan_many_device(h, SUM, 0, dp(d_x), n, 1, None, dp(d_y, 8)) == ERR_ARG and "aligned" in err()
    assert lib.blsgpu_fr_scan_many_device(h, HORNER, 0, dp(d_x), n, 1, dp(d_z, 8), dp(d_y)) == ERR_ARG and "aligned" in err()
    fl = np.zeros(2 * n, dtype=np.uint8)
    d_fl = torch.zeros(2 * n, dtype=torch.uint8, device=dev)
    for fn, pi, po, at in ((lib.blsgpu_fr_batch_invert, cp(x), cp(y), lambda off: ctypes.c_void_p(x.ctypes.data + off)),
                           (lib.blsgpu_fr_batch_invert_device, dp(d_x), dp(d_y), lambda off: dp(d_x, off))):
        pf = cp(fl) if fn is lib.blsgpu_fr_batch_invert else dp(d_fl)
        assert fn(h, None, n, po, pf) == ERR_ARG and "NULL" in err()
        assert fn(h, pi, n, None, pf) == ERR_ARG and "NULL" in err()
        assert fn(h, pi, (1 << 28) + 1, po, pf) == ERR_ARG and "2^28" in err()
        assert fn(h, pi, n, at(32), pf) == ERR_ARG and "overlap" in err()
        assert fn(h, pi, 0, po, None) == 0 and fn(h, None, 0, None, None) == 0
    assert lib.blsgpu_fr_batch_invert_device(h, dp(d_x, 8), n, dp(d_y), dp(d_fl)) == ERR_ARG and "aligned" in err()
    assert lib.blsgpu_fr_batch_invert_device(h, dp(d_x), n, dp(d_y, 8), dp(d_fl)) == ERR_ARG and "aligned" in err()
    ctx.synchronize()
    assert np.array_equal(x, keep) and not y.any() and not fl.any()
    assert np.array_equal(d_x.cpu().numpy().view(np.uint64), keep) and not d_y.cpu().numpy().any() and not d_fl.cpu().numpy().any()
    with pytest.raises(ValueError):
        ctx.fr_scan(SUM, np.zeros((2, 3, 5), dtype=np.uint64))
    with pytest.raises(ValueError):
        ctx.fr_scan(HORNER, x.reshape(2, n, 4))
    with pytest.raises(ValueError):
        ctx.fr_scan(HORNER, x.reshape(2, n, 4), points=[1, 2], exclusive=True)
    with pytest.raises(ValueError):
        ctx.fr_scan(HORNER, x.reshape(2, n, 4), points=[1])
    # the context is still usable; in place through the device form; empty calls through the Python forms
    want = ctx.fr_scan(SUM, x.reshape(2, n, 4))
    assert np.array_equal(want[0, 1], _from_raw([sum(_raw_ints(x[:2])) % RR])[0])
    ctx.fr_scan_device(SUM, d_x.data_ptr(), n, 2, d_x.data_ptr())
    ctx.synchronize()
    assert np.array_equal(d_x.cpu().numpy().view(np.uint64).reshape(2, n, 4), want)
    assert ctx.fr_scan(SUM, np.zeros((0, 8, 4), dtype=np.uint64)).shape == (0, 8, 4)
    assert ctx.fr_batch_invert(np.zeros((0, 4), dtype=np.uint64)).shape == (0, 4)


def test_cpp_mirror(ctx, tmp_path):
    """include/bls12_381.hpp fr_scan / fr_batch_invert compiled with g++ against libblsgpu.so: a HORNER row against a host loop over
    bls::fr_op, a batch inversion against bls::fr_op op 4"""
    import bls12_381_amd as b
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "fr_scan_test")
    libdir = os.path.dirname(b.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "fr_scan_test.cpp"),
                           "-L" + libdir, "-lblsgpu", "-Wl,-rpath," + libdir, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "fr_scan ok" in out.stdout, out.stdout + out.stderr
