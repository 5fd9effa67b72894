"""Multilinear folds, eq tables, evaluations and sumcheck rounds (`blsgpu_fr_mle_fold*`, `blsgpu_fr_eq_table*`, `blsgpu_fr_mle_eval*`,
`blsgpu_fr_sumcheck_*`; csrc/fr_mle.hip.h + csrc/fr_mle_plan.h) on the GPU.

Every expectation is Python integers mod r computed here from the definitions of include/bls12_381_hip.h -- fold(f, r)[i] = f[i] + r (f[i+h] - f[i]),
eq(p)[i] = prod_b (bit b of i ? p_b : 1 - p_b), the round polynomial's values at 0 .. D -- and compared limb for limb, so a non-canonical
output does not compare equal.  The sumchecks are also run through the verifier's own checks."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import bls12_381_ref as o

pytestmark = pytest.mark.gpu

RR = o.R_ORDER
MONT = o.FR_MONT_R
ERR_ARG = -2
BLOCK, CHUNK = 256, 4                                              # csrc/fr_mle_plan.h: FRM_BLOCK, FRM_CHUNK
LOG_T = (BLOCK * CHUNK).bit_length() - 1                           # the tile of the round kernel in positions: 2^10
SPARTAN = [(1, [0, 1, 2]), (RR - 1, [0, 3])]                       # eq * (Az * Bz - Cz)


@pytest.fixture(scope="module")
def ctx():
    import bls12_381_amd as b
    c = b.Context(0)
    yield c
    c.close()


# ---- Python integers: the definitions ------------------------------------------------------------------------------------------------
def _fold(f, r):
    h = len(f) // 2
    return [(f[i] + r * (f[i + h] - f[i])) % RR for i in range(h)]


def _eq(p):
    t = [1]
    for pb in p:
        t = [x * (1 - pb) % RR for x in t] + [x * pb % RR for x in t]
    return t


def _eval(f, p):
    for b in range(len(p) - 1, -1, -1):
        f = _fold(f, p[b])
    return f[0]


def _round(tabs, terms):
    h = len(tabs[0]) // 2
    deg = max(len(ix) for _, ix in terms)
    out = []
    for t in range(deg + 1):
        at = [[((1 - t) * f[i] + t * f[i + h]) % RR for i in range(h)] for f in tabs]
        s = 0
        for c, ix in terms:
            cols = [at[e] for e in ix]
            for i in range(h):
                p = c
                for col in cols:
                    p = p * col[i] % RR
                s += p
        out.append(s % RR)
    return out


def _interpolate(evals, x):
    n, s = len(evals), 0
    for t in range(n):
        num = den = 1
        for u in range(n):
            if u != t:
                num = num * (x - u) % RR
                den = den * (t - u) % RR
        s += evals[t] * num * pow(den, -1, RR)
    return s % RR


def _verify(rounds, point, values, terms, claimed_sum=None):
    """the verifier: evals[0] + evals[1] is the running claim, the next claim the interpolation at the challenge, the last one
    sum_t coef_t prod values; point[b] = the challenge of round m - b"""
    m = len(rounds)
    claim = claimed_sum
    for s, ev in enumerate(rounds, 1):
        assert len(ev) == max(len(ix) for _, ix in terms) + 1
        assert claim is None or (ev[0] + ev[1]) % RR == claim, "round %d: evals[0] + evals[1] is not the running claim" % s
        claim = _interpolate(ev, point[m - s])
    final = 0
    for c, ix in terms:
        p = c
        for e in ix:
            p = p * values[e] % RR
        final += p
    assert final % RR == claim, "the final claim is not sum_t coef_t prod values"


def _challenge(s, ev):
    return (sum((i + 3) * v for i, v in enumerate(ev)) * 0x9E3779B97F4A7C15 + s * s + 1) % RR


# ---- limbs ---------------------------------------------------------------------------------------------------------------------------
def _limbs(vals):
    """integers mod r -> (len, 4) u64 Montgomery limbs"""
    b = b"".join((int(v) % RR * MONT % RR).to_bytes(32, "little") for v in vals)
    return np.frombuffer(b, dtype=np.uint64).reshape(-1, 4).copy()


def _same(got, want_ints):
    """limb equality with the Montgomery forms of want_ints (got is NOT reduced first)"""
    return np.array_equal(np.ascontiguousarray(got, dtype=np.uint64).reshape(-1, 4), _limbs(want_ints))


def _ints(limbs):
    import bls12_381_amd as b
    return [b.fr_limbs_to_int(l) for l in np.asarray(limbs, dtype=np.uint64).reshape(-1, 4)]


def _tables(k, m, seed):
    r = o.SplitMix64(seed)
    n, h = 1 << m, (1 << m) >> 1
    tabs = [[r.scalar() for _ in range(n)] for _ in range(k)]
    vals = (0, 1, RR - 1)
    for j, f in enumerate(tabs):
        for q, pos in enumerate((0, n - 1, max(h - 1, 0), h)):
            if n >= 4 or q < 2:
                f[pos % n] = vals[(j + q) % 3]
    return tabs


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(torch.device("cuda", 0))


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _pitched(tabs, pitch):
    """k tables `pitch` scalars apart in one (k * pitch, 4) array, a marker pattern in the gaps"""
    k, n = len(tabs), len(tabs[0])
    a = np.full((k * pitch, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    for j, f in enumerate(tabs):
        a[j * pitch:j * pitch + n] = _limbs(f)
    return a


def _programs(k):
    c = o.SplitMix64(k).scalar()
    return {1: [(c, [0]), (1, [0, 0])],
            4: SPARTAN,
            8: [(1, [0]), (RR - 1, [1, 2]), (c, [3, 4, 5]), (0, [6, 7, 0, 1]), (2, [2, 2, 2, 2, 2]), (c + 1, [7, 6, 5, 4, 3, 2]), (RR - 2, [1]), (3, [5, 5])]}[k]


# ---- parity through the C ABI --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 3, LOG_T, LOG_T + 1, LOG_T + 2])
def test_parity(ctx, m):
    """k = 1, 4, 8 at every m where the schedule changes hands (one pair, below, at, and at 2x the tile for the plain round; the fused
    round is one tile up to LOG_T + 2): the fold out of place (host form) and in place with a pitch (device form), the evaluation, the
    plain round, the fused round with the folded tables it leaves behind, and the eq table"""
    import torch
    rnd = o.SplitMix64(1000 + m)
    n, h = 1 << m, 1 << (m - 1)
    for k in (1, 4, 8):
        tabs = _tables(k, m, 31 * m + k)
        terms = _programs(k)
        deg = max(len(ix) for _, ix in terms)
        r = (0, 1, RR - 1, rnd.scalar())[(m + k) % 4]
        folded = [_fold(f, r) for f in tabs]
        what = "m=%d k=%d" % (m, k)
        # fold, host form (packed, out of place)
        assert _same(ctx.fr_mle_fold(_limbs([x for f in tabs for x in f]).reshape(k, n, 4), r), [x for f in folded for x in f]), what
        # fold, device form, in place, pitch > 2^m
        pitch = n + 6
        src = _pitched(tabs, pitch)
        d_t, d_r = _dev(src), _dev(_limbs([r]))
        torch.cuda.synchronize()
        ctx.fr_mle_fold_device(d_t.data_ptr(), pitch, m, k, d_r.data_ptr(), d_t.data_ptr(), pitch)
        ctx.synchronize()
        want = src.copy()
        for j in range(k):
            want[j * pitch:j * pitch + h] = _limbs(folded[j])
        assert np.array_equal(_host(d_t), want), what + " (fold in place: lower halves folded, everything else untouched)"
        # evaluation
        p = [rnd.scalar() for _ in range(m)]
        assert _same(ctx.fr_mle_eval(_limbs([x for f in tabs for x in f]).reshape(k, n, 4), p), [_eval(f, p) for f in tabs]), what
        # the plain round: nothing is written but the evaluations
        d_t = _dev(src)
        d_ev = torch.zeros((deg + 1, 4), dtype=torch.int64, device=d_t.device)
        torch.cuda.synchronize()
        ctx.fr_sumcheck_round_device(d_t.data_ptr(), pitch, m, k, terms, d_ev.data_ptr())
        ctx.synchronize()
        assert _same(_host(d_ev), _round(tabs, terms)), what + " (plain round)"
        assert np.array_equal(_host(d_t), src), what
        # the fused round
        if m >= 2:
            ctx.fr_sumcheck_round_device(d_t.data_ptr(), pitch, m, k, terms, d_ev.data_ptr(), d_r_prev=d_r.data_ptr())
            ctx.synchronize()
            assert _same(_host(d_ev), _round(folded, terms)), what + " (fused round)"
            assert np.array_equal(_host(d_t), want), what + " (fused round: lower halves folded, everything else untouched)"
    # eq, with 0 and 1 among the coordinates
    p = [rnd.scalar() for _ in range(m)]
    p[0] = 1
    if m > 2:
        p[m // 2] = 0
    assert _same(ctx.fr_eq_table(p), _eq(p))
    assert np.array_equal(ctx.fr_eq_table(_limbs(p)), ctx.fr_eq_table(p))      # the limb form of the point is the same call


def test_parity_at_2_16(ctx):
    """m = 16, k = 1, 4, 8: the fold and the eq table checked fully, the evaluation, and the rounds by their D + 1 values with terms of at
    most three factors (the fused round for every k, with the tables it leaves behind; the plain one for k = 4)"""
    import torch
    m = 16
    n, h = 1 << m, 1 << (m - 1)
    rnd = o.SplitMix64(16)
    p = [rnd.scalar() for _ in range(m)]
    e = _eq(p)
    assert _same(ctx.fr_eq_table(p), e)
    c = rnd.scalar()
    programs = {1: [(c, [0]), (1, [0, 0])], 4: SPARTAN, 8: [(1, [0, 1, 2]), (RR - 1, [3, 4]), (c, [5, 6, 7])]}
    for k in (1, 4, 8):
        tabs = _tables(k, m, 1616 + k)
        terms = programs[k]
        deg = max(len(ix) for _, ix in terms)
        r = rnd.scalar()
        x = _limbs([v for f in tabs for v in f]).reshape(k, n, 4)
        folded = [_fold(f, r) for f in tabs]
        assert _same(ctx.fr_mle_fold(x, r), [v for f in folded for v in f]), k
        if k == 4:
            assert _same(ctx.fr_mle_eval(x, p), [sum(a * b for a, b in zip(f, e)) % RR for f in tabs])
        d_t, d_r = _dev(x), _dev(_limbs([r]))
        d_ev = torch.zeros((deg + 1, 4), dtype=torch.int64, device=d_t.device)
        torch.cuda.synchronize()
        if k == 4:
            ctx.fr_sumcheck_round_device(d_t.data_ptr(), n, m, k, terms, d_ev.data_ptr())
            ctx.synchronize()
            assert _same(_host(d_ev), _round(tabs, terms))
        ctx.fr_sumcheck_round_device(d_t.data_ptr(), n, m, k, terms, d_ev.data_ptr(), d_r_prev=d_r.data_ptr())
        ctx.synchronize()
        assert _same(_host(d_ev), _round(folded, terms)), k
        got = _host(d_t).reshape(k, n, 4)
        assert _same(got[:, :h], [v for f in folded for v in f]) and np.array_equal(got[:, h:], x[:, h:]), k


# ---- the whole sumcheck --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,k,name", [(14, 4, "spartan"), (1, 4, "spartan"), (9, 2, "degree 6")])
def test_sumcheck_prove(ctx, m, k, name):
    """fr_sumcheck_prove with a deterministic challenge function: the claimed sum from Python, the verifier's checks, and the final
    values against a Python fold of the original tables at the point the challenges define"""
    terms = SPARTAN if name == "spartan" else [(RR - 1, [0, 1, 0, 1, 1, 0]), (7, [1])]
    tabs = _tables(k, m, 5 * m + k)
    x = _limbs([v for f in tabs for v in f]).reshape(k, 1 << m, 4)
    rounds, point, values = ctx.fr_sumcheck_prove(x, terms, _challenge)
    assert len(rounds) == m and len(point) == m
    assert point == [_challenge(m - b, rounds[m - b - 1]) for b in range(m)]      # point[b] = the challenge of round m - b
    total = 0
    for c, ix in terms:
        for i in range(1 << m):
            p = c
            for e in ix:
                p = p * tabs[e][i] % RR
            total += p
    vals = _ints(values)
    _verify(rounds, point, vals, terms, claimed_sum=total % RR)
    assert _same(values, [_eval(f, point) for f in tabs])


def _r1cs(n, seed):
    """random A, B (three entries per row) and z, and C with one entry per row such that (A z) o (B z) = C z; as the stacked 3n-row CSR"""
    r = o.SplitMix64(seed)
    z = [r.scalar() or 1 for _ in range(n)]
    rows = []
    for _ in range(2 * n):
        rows.append([(r.next() % n, r.scalar()) for _ in range(3)])
    az = [sum(v * z[c] for c, v in row) % RR for row in rows[:n]]
    bz = [sum(v * z[c] for c, v in row) % RR for row in rows[n:]]
    for i in range(n):
        j = r.next() % n
        rows.append([(j, az[i] * bz[i] % RR * pow(z[j], -1, RR) % RR)])
    cz = [az[i] * bz[i] % RR for i in range(n)]
    row_ptr = np.cumsum([0] + [len(row) for row in rows]).astype(np.uint32)
    col = np.array([c for row in rows for c, _ in row], dtype=np.uint32)
    return row_ptr, col, [v for row in rows for _, v in row], z, (az, bz, cz)


def _outer_sumcheck(ctx, d_tables, m, tau):
    """Spartan's outer sumcheck over (eq(tau), Az, Bz, Cz) resident in d_tables: the rounds through the handle, the checks of the issue"""
    sc = ctx.fr_sumcheck_device(d_tables.data_ptr(), 1 << m, m, 4, SPARTAN)
    assert (sc.vars_left, sc.degree) == (m, 3)
    rounds, chal, r = [], [], None
    for s in range(1, m + 1):
        ev = _ints(sc.round(r))
        rounds.append(ev)
        r = _challenge(s, ev)
        chal.append(r)
        assert sc.vars_left == (m if s == 1 else m - s + 1)
    values = _ints(sc.finish(r))
    assert sc.vars_left == 0
    sc.close()
    point = chal[::-1]
    assert (rounds[0][0] + rounds[0][1]) % RR == 0, "a satisfied R1CS sums to zero"
    _verify(rounds, point, values, SPARTAN, claimed_sum=0)
    want_eq = 1
    for tb, pb in zip(tau, point):
        want_eq = want_eq * (tb * pb + (1 - tb) * (1 - pb)) % RR
    assert values[0] == want_eq, "values[0] is not eq(tau)(point)"
    return point, values


def test_the_device_chain_without_a_host_copy(ctx):
    """an R1CS of 2^6 rows with a satisfying z: Az, Bz, Cz from Python integers next to eq(tau) from fr_eq_table_device in ONE device
    buffer, fr_sumcheck_device through the rounds"""
    import torch
    m, n = 6, 64
    _, _, _, _, (az, bz, cz) = _r1cs(n, 0x51)
    tau = [o.SplitMix64(0x7A).scalar() for _ in range(1)] + [o.SplitMix64(b + 9).scalar() for b in range(m - 1)]
    host = np.zeros((4, n, 4), dtype=np.uint64)
    host[1], host[2], host[3] = _limbs(az), _limbs(bz), _limbs(cz)
    d_t, d_tau = _dev(host.reshape(-1, 4)), _dev(_limbs(tau))
    torch.cuda.synchronize()
    ctx.fr_eq_table_device(d_tau.data_ptr(), m, d_t.data_ptr())
    point, values = _outer_sumcheck(ctx, d_t, m, tau)
    assert values[1:] == [_eval(f, point) for f in (az, bz, cz)]
    got = _host(d_t).reshape(4, n, 4)                               # begin_device copies: the caller's tables stay as they are
    assert _same(got[0], _eq(tau)) and np.array_equal(got[1:], host[1:])


def test_the_device_chain_behind_fr_spmv_device(ctx):
    """the same with Az, Bz, Cz produced by fr_spmv_device on the stacked 3n-row matrix, written straight into rows 1 .. 3 of the buffer"""
    import torch
    m, n = 6, 64
    row_ptr, col, vals, z, (az, bz, cz) = _r1cs(n, 0x52)
    tau = [o.SplitMix64(40 + b).scalar() for b in range(m)]
    mat = ctx.fr_matrix(row_ptr, col, vals, n)
    d_t = torch.zeros((4 * n, 4), dtype=torch.int64, device=torch.device("cuda", 0))
    d_z, d_tau = _dev(_limbs(z)), _dev(_limbs(tau))
    torch.cuda.synchronize()
    ctx.fr_spmv_device(mat, d_z.data_ptr(), 1, d_t.data_ptr() + n * 32)
    ctx.fr_eq_table_device(d_tau.data_ptr(), m, d_t.data_ptr())
    ctx.synchronize()
    assert _same(_host(d_t)[n:], az + bz + cz), "fr_spmv_device differs from Python (not this module's code)"
    point, values = _outer_sumcheck(ctx, d_t, m, tau)
    assert values[1:] == [_eval(f, point) for f in (az, bz, cz)]
    mat.close()


# ---- streams -------------------------------------------------------------------------------------------------------------------------
def test_on_a_caller_stream_and_between_pipelined_msm_calls(ctx):
    """the device forms on a non-default stream set with set_stream, then enqueued between two pipelined msm_device calls"""
    import torch
    dev = torch.device("cuda", 0)
    m, k = LOG_T + 1, 4                                             # two tiles: records in the context's scratch, the finish kernel
    n, h = 1 << m, 1 << (m - 1)
    rnd = o.SplitMix64(0x57)
    tabs = _tables(k, m, 0x58)
    r = rnd.scalar()
    p = [rnd.scalar() for _ in range(m)]
    x = _limbs([v for f in tabs for v in f])
    folded = [_fold(f, r) for f in tabs]
    want = {"eq": _limbs(_eq(p)), "fold": _limbs([v for f in folded for v in f]), "eval": _limbs([_eval(f, p) for f in tabs]),
            "plain": _limbs(_round(tabs, SPARTAN)), "fused": _limbs(_round(folded, SPARTAN))}

    def buffers():
        z = lambda rows: torch.zeros((rows, 4), dtype=torch.int64, device=dev)
        return {"x": _dev(x), "work": _dev(x), "r": _dev(_limbs([r])), "p": _dev(_limbs(p)), "eq": z(n), "fold": z(k * h), "eval": z(k), "plain": z(4), "fused": z(4)}

    def enqueue(b):
        ctx.fr_eq_table_device(b["p"].data_ptr(), m, b["eq"].data_ptr())
        ctx.fr_mle_fold_device(b["x"].data_ptr(), n, m, k, b["r"].data_ptr(), b["fold"].data_ptr(), h)
        ctx.fr_mle_eval_device(b["x"].data_ptr(), n, m, k, b["p"].data_ptr(), b["eval"].data_ptr())
        ctx.fr_sumcheck_round_device(b["work"].data_ptr(), n, m, k, SPARTAN, b["plain"].data_ptr())
        ctx.fr_sumcheck_round_device(b["work"].data_ptr(), n, m, k, SPARTAN, b["fused"].data_ptr(), d_r_prev=b["r"].data_ptr())

    def check(b):
        for name, w in want.items():
            assert np.array_equal(_host(b[name]), w), name
        assert np.array_equal(_host(b["x"]), x)
        got = _host(b["work"]).reshape(k, n, 4)
        assert np.array_equal(got[:, :h].reshape(-1, 4), want["fold"]) and np.array_equal(got[:, h:], x.reshape(k, n, 4)[:, h:])

    side = torch.cuda.Stream(device=dev)
    bufs = buffers()
    torch.cuda.synchronize()
    ctx.set_stream(side.cuda_stream)
    try:
        enqueue(bufs)
        ctx.synchronize()
    finally:
        ctx.set_stream(None)
    check(bufs)
    # between pipelined MSM calls
    cnt = 1 << 14
    S = np.random.RandomState(5).randint(0, 256, size=(2 * cnt, 32), dtype=np.uint8)
    S[:, 31] &= 0x3F
    bases = ctx.bases_from_scalars(1, S[:cnt])
    d_s = torch.from_numpy(S).to(dev)
    d_msm = torch.zeros((2, 18), dtype=torch.int64, device=dev)
    bufs = buffers()
    torch.cuda.synchronize()
    ctx.set_pipelining(True)
    try:
        ctx.msm_device(bases, d_s[0:cnt].data_ptr(), cnt, d_msm[0].data_ptr())
        enqueue(bufs)
        ctx.msm_device(bases, d_s[cnt:2 * cnt].data_ptr(), cnt, d_msm[1].data_ptr())
        ctx.join()
        ctx.synchronize()
    finally:
        ctx.set_pipelining(False)
    check(bufs)
    got = ctx.batch_normalize(1, d_msm.cpu().numpy().view(np.uint64))
    for i in range(2):
        ref = ctx.batch_normalize(1, ctx.msm(bases, S[i * cnt:(i + 1) * cnt])[None, :])
        assert np.array_equal(got[0][i], ref[0][0]) and got[1][i] == ref[1][0], i
    bases.free()


# ---- arguments -----------------------------------------------------------------------------------------------------------------------
def test_arguments(ctx):
    """every refusal is BLSGPU_ERR_ARG with a text naming the cause, before anything is staged or launched: inputs and outputs are
    untouched and the context works afterwards; k == 0 is a no-op for fold and eval and refused by the sumcheck calls"""
    import torch
    lib, h = ctx.lib, ctx.h
    m, k = 4, 2
    n = 1 << m
    tabs = _tables(k, m, 3)
    x = _limbs([v for f in tabs for v in f])
    keep = x.copy()
    y = np.zeros((k * n, 4), dtype=np.uint64)
    rr = _limbs([5])
    pt = _limbs([3, 4, 5, 6])
    d_x, d_y, d_r, d_p = _dev(x), _dev(y), _dev(rr), _dev(pt)
    torch.cuda.synchronize()
    cp = lambda a, off=0: ctypes.c_void_p(a.ctypes.data + off)
    dp = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    err = lambda: lib.blsgpu_last_error().decode()
    big = 1 << 28
    # fold
    F, FD = lib.blsgpu_fr_mle_fold, lib.blsgpu_fr_mle_fold_device
    assert F(h, cp(x), 0, k, cp(rr), cp(y)) == ERR_ARG and "[1, 28]" in err()
    assert F(h, cp(x), 29, k, cp(rr), cp(y)) == ERR_ARG and "[1, 28]" in err()
    assert F(h, None, m, k, cp(rr), cp(y)) == ERR_ARG and "NULL" in err()
    assert F(h, cp(x), m, k, None, cp(y)) == ERR_ARG and "NULL" in err()
    assert F(h, cp(x), m, k, cp(rr), None) == ERR_ARG and "NULL" in err()
    assert F(h, cp(x), 28, 2, cp(rr), cp(y)) == ERR_ARG and "2^28" in err()
    assert F(h, cp(x), m, (1 << 64) - 1, cp(rr), cp(y)) == ERR_ARG and "2^28" in err()
    assert F(h, cp(x), m, 0, cp(rr), cp(y)) == 0 and F(h, None, m, 0, None, None) == 0
    assert FD(h, dp(d_x), n - 1, m, k, dp(d_r), dp(d_y), n // 2) == ERR_ARG and "pitch" in err()
    assert FD(h, dp(d_x), n, m, k, dp(d_r), dp(d_y), n // 2 - 1) == ERR_ARG and "pitch" in err()
    assert FD(h, dp(d_x), big, m, 3, dp(d_r), dp(d_y), n // 2) == ERR_ARG and "2^28" in err()
    assert FD(h, dp(d_x), (1 << 63) + 1, m, 4, dp(d_r), dp(d_y), n // 2) == ERR_ARG and "2^28" in err()      # (k - 1) * pitch overflows 64 bits
    assert FD(h, dp(d_x, 8), n, m, k, dp(d_r), dp(d_y), n // 2) == ERR_ARG and "aligned" in err()
    assert FD(h, dp(d_x), n, m, k, dp(d_r, 8), dp(d_y), n // 2) == ERR_ARG and "aligned" in err()
    assert FD(h, dp(d_x), n, m, k, dp(d_r), dp(d_y, 8), n // 2) == ERR_ARG and "aligned" in err()
    assert FD(h, dp(d_x), n, m, k, dp(d_r), dp(d_x), n // 2) == ERR_ARG and "overlap" in err()       # same base, another pitch: not the in-place form
    assert FD(h, dp(d_x), n, m, k, dp(d_r), dp(d_x, 32), n) == ERR_ARG and "overlap" in err()
    assert FD(h, dp(d_x), n, m, 1, dp(d_r), dp(d_x, (n - 1) * 32), n) == ERR_ARG and "overlap" in err()
    assert FD(h, None, n, m, k, dp(d_r), dp(d_y), n // 2) == ERR_ARG and "NULL" in err()
    assert FD(h, dp(d_x), n, m, 0, dp(d_r), dp(d_y), n // 2) == 0
    # eq
    E, ED = lib.blsgpu_fr_eq_table, lib.blsgpu_fr_eq_table_device
    assert E(h, cp(pt), -1, cp(y)) == ERR_ARG and "[0, 28]" in err()
    assert E(h, cp(pt), 29, cp(y)) == ERR_ARG and "[0, 28]" in err()
    assert E(h, None, m, cp(y)) == ERR_ARG and "NULL" in err()
    assert E(h, cp(pt), m, None) == ERR_ARG and "NULL" in err()
    assert ED(h, dp(d_p, 8), m, dp(d_y)) == ERR_ARG and "aligned" in err()
    assert ED(h, dp(d_p), m, dp(d_y, 8)) == ERR_ARG and "aligned" in err()
    # eval
    V, VD = lib.blsgpu_fr_mle_eval, lib.blsgpu_fr_mle_eval_device
    assert V(h, cp(x), -1, k, cp(pt), cp(y)) == ERR_ARG and "[0, 28]" in err()
    assert V(h, cp(x), 29, k, cp(pt), cp(y)) == ERR_ARG and "[0, 28]" in err()
    assert V(h, None, m, k, cp(pt), cp(y)) == ERR_ARG and "NULL" in err()
    assert V(h, cp(x), m, k, None, cp(y)) == ERR_ARG and "NULL" in err()
    assert V(h, cp(x), m, k, cp(pt), None) == ERR_ARG and "NULL" in err()
    assert V(h, cp(x), 28, 2, cp(pt), cp(y)) == ERR_ARG and "2^28" in err()
    assert V(h, cp(x), m, 0, cp(pt), cp(y)) == 0 and V(h, None, m, 0, None, None) == 0
    assert VD(h, dp(d_x), n - 1, m, k, dp(d_p), dp(d_y)) == ERR_ARG and "pitch" in err()
    assert VD(h, dp(d_x, 8), n, m, k, dp(d_p), dp(d_y)) == ERR_ARG and "aligned" in err()
    assert VD(h, dp(d_x), n, m, k, dp(d_p), dp(d_x, 64)) == ERR_ARG and "overlap" in err()
    # the round and the handle: a program is (n_terms, term_ptr, term_tab, coef)
    ptr = np.array([0, 2, 3], dtype=np.uint32)
    tab = np.array([0, 1, 1], dtype=np.uint8)
    coef = _limbs([1, RR - 1])
    d_ev = torch.zeros((3, 4), dtype=torch.int64, device=d_x.device)
    RD = lib.blsgpu_fr_sumcheck_round_device
    good = lambda **kw: [kw.get("t", dp(d_x)), kw.get("pitch", n), kw.get("m", m), kw.get("k", k), kw.get("nt", 2), kw.get("ptr", cp(ptr)), kw.get("tab", cp(tab)),
                         kw.get("coef", cp(coef)), kw.get("r", None), kw.get("ev", dp(d_ev))]
    bad_ptr0 = np.array([1, 2, 3], dtype=np.uint32)
    bad_flat = np.array([0, 2, 2], dtype=np.uint32)
    bad_long = np.array([0, 7, 8], dtype=np.uint32)
    bad_tab = np.array([0, 2, 1], dtype=np.uint8)
    bad_coef = np.concatenate([_limbs([1]), np.frombuffer(RR.to_bytes(32, "little"), dtype=np.uint64).reshape(1, 4)])
    for kw, text in (({"k": 0}, "k must be"), ({"k": 9}, "k must be"), ({"nt": 0}, "n_terms"), ({"nt": 9}, "n_terms"), ({"ptr": None}, "NULL"), ({"tab": None}, "NULL"),
                     ({"coef": None}, "NULL"), ({"ptr": cp(bad_ptr0)}, "term_ptr[0]"), ({"ptr": cp(bad_flat)}, "strictly"), ({"ptr": cp(bad_long)}, "1 to 6"),
                     ({"tab": cp(bad_tab)}, "below k"), ({"coef": cp(bad_coef)}, "canonical"), ({"m": 0}, "[1, 28]"), ({"m": 29}, "[1, 28]"),
                     ({"m": 1, "r": dp(d_r)}, "[2, 28]"), ({"pitch": n - 1}, "pitch"), ({"pitch": big}, "2^28"), ({"t": None}, "NULL"), ({"ev": None}, "NULL"),
                     ({"t": dp(d_x, 8)}, "aligned"), ({"ev": dp(d_ev, 8)}, "aligned"), ({"r": dp(d_r, 8)}, "aligned"), ({"ev": dp(d_x, 32)}, "overlap"),
                     ({"r": dp(d_x, 64)}, "inside the tables")):
        assert RD(h, *good(**kw)) == ERR_ARG and text in err(), (kw, err())
    out = ctypes.c_void_p()
    B, BD = lib.blsgpu_fr_sumcheck_begin, lib.blsgpu_fr_sumcheck_begin_device
    assert B(h, cp(x), m, 0, 2, cp(ptr), cp(tab), cp(coef), ctypes.byref(out)) == ERR_ARG and "k must be" in err() and not out.value
    assert B(h, cp(x), 0, k, 2, cp(ptr), cp(tab), cp(coef), ctypes.byref(out)) == ERR_ARG and "[1, 28]" in err() and not out.value
    assert B(h, None, m, k, 2, cp(ptr), cp(tab), cp(coef), ctypes.byref(out)) == ERR_ARG and "NULL" in err() and not out.value
    assert B(h, cp(x), m, k, 2, cp(ptr), cp(bad_tab), cp(coef), ctypes.byref(out)) == ERR_ARG and "below k" in err() and not out.value
    assert B(h, cp(x), m, k, 2, cp(ptr), cp(tab), cp(coef), None) == ERR_ARG and "NULL" in err()
    assert BD(h, dp(d_x, 8), n, m, k, 2, cp(ptr), cp(tab), cp(coef), ctypes.byref(out)) == ERR_ARG and "aligned" in err() and not out.value
    assert BD(h, dp(d_x), n - 1, m, k, 2, cp(ptr), cp(tab), cp(coef), ctypes.byref(out)) == ERR_ARG and "pitch" in err() and not out.value
    lib.blsgpu_fr_sumcheck_free(None)
    assert lib.blsgpu_fr_sumcheck_vars_left(None) == 0 and lib.blsgpu_fr_sumcheck_degree(None) == 0
    ctx.synchronize()
    assert np.array_equal(x, keep) and not y.any()
    assert np.array_equal(_host(d_x), keep) and not _host(d_y).any() and not _host(d_ev).any()
    with pytest.raises(ValueError):
        ctx.fr_mle_fold(np.zeros((2, 3, 4), dtype=np.uint64), 1)
    with pytest.raises(ValueError):
        ctx.fr_mle_eval(x.reshape(k, n, 4), [1, 2])
    # the context still works; empty calls through the Python forms
    assert _same(ctx.fr_mle_fold(x.reshape(k, n, 4), 5), [v for f in tabs for v in _fold(f, 5)])
    assert ctx.fr_mle_fold(np.zeros((0, 8, 4), dtype=np.uint64), 1).shape == (0, 4, 4)
    assert ctx.fr_mle_eval(np.zeros((0, 8, 4), dtype=np.uint64), [1, 2, 3]).shape == (0, 4)
    assert _same(ctx.fr_eq_table([]), [1])
    assert _same(ctx.fr_mle_eval(x.reshape(k * n, 1, 4)[:3], []), [tabs[0][0], tabs[0][1], tabs[0][2]])      # m = 0 copies


def test_calls_out_of_order_on_the_handle(ctx):
    """any order but round(NULL), round(r) ..., finish(r) is BLSGPU_ERR_ARG and leaves the handle as it was: the sumcheck then still
    completes with the right numbers"""
    lib, h = ctx.lib, ctx.h
    m, k = 3, 4
    tabs = _tables(k, m, 99)
    x = _limbs([v for f in tabs for v in f]).reshape(k, 1 << m, 4)
    sc = ctx.fr_sumcheck(x, SPARTAN)
    ev = np.zeros((4, 4), dtype=np.uint64)
    vals = np.zeros((k, 4), dtype=np.uint64)
    r1, r2, r3 = 11, 0, RR - 1
    lr = {r: _limbs([r]) for r in (r1, r2, r3)}
    cp = lambda a: ctypes.c_void_p(a.ctypes.data)
    err = lambda: lib.blsgpu_last_error().decode()
    R, Fi = lib.blsgpu_fr_sumcheck_round, lib.blsgpu_fr_sumcheck_finish
    assert R(h, sc.handle, cp(lr[r1]), cp(ev)) == ERR_ARG and "first round" in err()
    assert Fi(h, sc.handle, cp(lr[r1]), cp(vals)) == ERR_ARG and "rounds are left" in err()
    assert R(h, None, None, cp(ev)) == ERR_ARG and R(h, sc.handle, None, None) == ERR_ARG and "NULL" in err()
    assert sc.vars_left == 3 and not ev.any()
    rounds = [_ints(sc.round())]
    assert R(h, sc.handle, None, cp(ev)) == ERR_ARG and "challenge" in err()
    assert Fi(h, sc.handle, cp(lr[r1]), cp(vals)) == ERR_ARG and "rounds are left" in err()
    assert sc.vars_left == 3
    rounds.append(_ints(sc.round(r1)))
    rounds.append(_ints(sc.round(lr[r2][0])))                     # the limb form of a challenge
    assert sc.vars_left == 1
    assert R(h, sc.handle, cp(lr[r3]), cp(ev)) == ERR_ARG and "one variable is left" in err()
    assert Fi(h, sc.handle, None, cp(vals)) == ERR_ARG and "NULL" in err()
    assert sc.vars_left == 1 and not ev.any() and not vals.any()
    values = sc.finish(r3)
    assert sc.vars_left == 0
    assert R(h, sc.handle, cp(lr[r3]), cp(ev)) == ERR_ARG and "finished" in err()
    assert Fi(h, sc.handle, cp(lr[r3]), cp(vals)) == ERR_ARG
    sc.close()
    sc.close()
    point = [r3, r2, r1]
    py = tabs
    for s, r in enumerate((None, r1, r2)):
        if r is not None:
            py = [_fold(f, r) for f in py]
        assert rounds[s] == _round(py, SPARTAN), s
    assert _same(values, [_eval(f, point) for f in tabs])
    _verify(rounds, point, _ints(values), SPARTAN)


def test_cpp_mirror(ctx, tmp_path):
    """include/bls12_381.hpp fr_mle_fold / fr_eq_table / fr_mle_eval / FrSumcheck compiled with g++ against libblsgpu.so: the fold against
    a host loop over bls::fr_op, the evaluation against the eq inner product, and a whole sumcheck through the verifier's checks"""
    import bls12_381_amd as b
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "fr_mle_test")
    libdir = os.path.dirname(b.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "fr_mle_test.cpp"),
                           "-L" + libdir, "-lblsgpu", "-Wl,-rpath," + libdir, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "fr_mle ok" in out.stdout, out.stdout + out.stderr
