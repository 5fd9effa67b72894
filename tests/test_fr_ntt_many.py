"""Batched and coset Fr transforms (`blsgpu_fr_ntt_many*`, csrc/fr.hip.h + csrc/fr_plan.h): k independent transforms in one call.

Small totals are compared limb for limb with the oracle (oracle/bls12_381_ref.py `fr_ntt`; the coset expectation is the transform of
[x_j g^j], the inverse one fr_ntt(y, inverse)[j] g^-j, in Python integers); larger ones with the existing single-vector path
(`ctx.fr_ntt`, `ctx.fr_op`), which has oracle tests of its own, and with Horner evaluations in Python integers."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import bls12_381_ref as o

pytestmark = pytest.mark.gpu

RR = o.R_ORDER
ERR_ARG = -2
G7 = o.FR_GENERATOR
G_RANDOM = o.SplitMix64(0xC05E7).scalar() or 5


@pytest.fixture(scope="module")
def ctx():
    import bls12_381_amd as b
    c = b.Context(0)
    yield c
    c.close()


def _limbs(vals):
    """integers mod r -> (len, 4) u64 Montgomery limbs"""
    b = b"".join((int(v) % RR * o.FR_MONT_R % RR).to_bytes(32, "little") for v in vals)
    return np.frombuffer(b, dtype=np.uint64).reshape(-1, 4).copy()


def _raw(n, seed):
    """n canonical `Scalar`s as raw limbs (any integer below r is the Montgomery form of some scalar)"""
    s = np.random.RandomState(seed).randint(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= 0x3F                                               # < 2^254 < r
    return s.view(np.uint64).reshape(n, 4).copy()


def _raw_ints(a):
    return [int.from_bytes(row.tobytes(), "little") for row in np.ascontiguousarray(a).reshape(-1, 4)]


def _expect(vs, inverse, g):
    out = []
    for v in vs:
        if g is None:
            out.append(o.fr_ntt(v, inverse=inverse))
        elif not inverse:
            out.append(o.fr_ntt([x * pow(g, j, RR) % RR for j, x in enumerate(v)]))
        else:
            gi = pow(g, -1, RR)
            out.append([y * pow(gi, j, RR) % RR for j, y in enumerate(o.fr_ntt(v, inverse=True))])
    return out


def _powers(g, n):
    """(n, 4) Montgomery limbs of g^j, from Python integers"""
    out, cur = [], 1
    for _ in range(n):
        out.append(cur)
        cur = cur * g % RR
    return _limbs(out)


@pytest.mark.parametrize("log_n,k", [(0, 5), (1, 7), (3, 1000), (6, 1024), (9, 3), (10, 64), (11, 5), (12, 16), (13, 3), (16, 1)])
def test_against_the_oracle(ctx, log_n, k):
    """forward / inverse x coset none / 7 / random, limb equality; the vectors hold 0, 1 and r - 1 among random values"""
    n = 1 << log_n
    r = o.SplitMix64(1000 * log_n + k)
    vs = [[r.scalar() for _ in range(n)] for _ in range(k)]
    for i, val in enumerate((0, 1, RR - 1)):
        vs[i % k][(i * 5) % n] = val
    x = _limbs([e for v in vs for e in v]).reshape(k, n, 4)
    for inverse in (False, True):
        for g in (None, G7, G_RANDOM):
            got = ctx.fr_ntt_many(x, inverse=inverse, coset=g)
            want = _limbs([e for v in _expect(vs, inverse, g) for e in v]).reshape(k, n, 4)
            bad = np.argwhere((got != want).any(axis=2))
            assert not len(bad), "log_n=%d k=%d inverse=%s g=%s: %d elements differ, first (vector, index) %s" % (log_n, k, inverse, g, len(bad), bad[0])
    # the limb form of the shift and the integer form are the same call
    assert np.array_equal(ctx.fr_ntt_many(x, coset=_limbs([G7])[0]), ctx.fr_ntt_many(x, coset=G7))


@pytest.mark.parametrize("log_n,k", [(12, 256), (16, 64), (20, 4), (22, 2)])
def test_against_the_single_transform(ctx, log_n, k):
    """larger calls: equal to a loop of ctx.fr_ntt over the vectors; with a coset, to ctx.fr_ntt(ctx.fr_op(0, x, powers)) and, for the
    inverse, to ctx.fr_op(0, ctx.fr_ntt(y, True), inverse powers), the power tables built from Python integers.  At (20, 4), g = 7: three
    positions per vector by Horner evaluation of the input polynomial at 7 w^m"""
    n = 1 << log_n
    x = _raw(k * n, 50 + log_n).reshape(k, n, 4)
    for inverse in (False, True):
        got = ctx.fr_ntt_many(x, inverse=inverse)
        for v in range(k):
            assert np.array_equal(got[v], ctx.fr_ntt(x[v], inverse=inverse)), (v, inverse)
    pw, pwi = _powers(G7, n), _powers(pow(G7, -1, RR), n)
    fwd = ctx.fr_ntt_many(x, coset=G7)
    inv = ctx.fr_ntt_many(x, inverse=True, coset=G7)
    for v in range(k):
        assert np.array_equal(fwd[v], ctx.fr_ntt(ctx.fr_op(0, x[v], pw))), v
        assert np.array_equal(inv[v], ctx.fr_op(0, ctx.fr_ntt(x[v], inverse=True), pwi)), v
    assert np.array_equal(ctx.fr_ntt_many(fwd, inverse=True, coset=G7), x)
    if (log_n, k) == (20, 4):
        w = o.fr_omega(log_n)
        for v in range(k):
            coeff = _raw_ints(x[v])                                # raw limbs: P_raw(z) = sum raw_j z^j = R * P(z), the raw limbs of the value
            for m in (0, 1 + 37 * v, n - 1 - v):
                z = G7 * pow(w, m, RR) % RR
                acc = 0
                for c in reversed(coeff):
                    acc = (acc * z + c) % RR
                assert _raw_ints(fwd[v][m])[0] == acc, (v, m)


def test_inverse_transforms_feed_a_segmented_msm_on_the_device(ctx):
    """the chain the call exists for, no host copy in between: 8 evaluation-form vectors of 2^12 in device memory -> fr_ntt_many_device(inverse)
    -> a Montgomery-form segmented MSM of all 8 over shared bases [k_i] G -> each result is [sum_j c_j k_j] G with c from the oracle"""
    import torch
    import bls12_381_amd as b
    log_n, k = 12, 8
    n = 1 << log_n
    r = o.SplitMix64(0xF3)
    ys = [[r.scalar() for _ in range(n)] for _ in range(k)]
    ks = [r.scalar() for _ in range(n)]
    cs = [o.fr_ntt(y, inverse=True) for y in ys]
    want = [o.g1_to_uncompressed(o.g1_to_affine(o.g1_affine_mul(o.G1_GEN, sum(c * kk for c, kk in zip(cv, ks)) % RR))) for cv in cs]
    dev = torch.device("cuda", 0)
    bases = ctx.bases_from_scalars(1, ks)
    d_y = torch.from_numpy(_limbs([e for y in ys for e in y]).view(np.int64)).to(dev)
    d_off = torch.from_numpy((np.arange(k + 1, dtype=np.uint32) * n).view(np.int32)).to(dev)
    d_bf = torch.zeros(k, dtype=torch.int32, device=dev)
    d_out = torch.zeros((k, 18), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ctx.set_scalar_form(b.api.SCALAR_MONT)
    try:
        ctx.fr_ntt_many_device(d_y.data_ptr(), log_n, k, inverse=True)
        ctx.msm_segments_device(bases, d_y.data_ptr(), d_off.data_ptr(), k, k * n, d_out.data_ptr(), d_base_first=d_bf.data_ptr())
        ctx.synchronize()
    finally:
        ctx.set_scalar_form(b.api.SCALAR_BYTES)
    xy, inf = ctx.batch_normalize(1, d_out.cpu().numpy().view(np.uint64))
    for i in range(k):
        assert b.G1Affine(xy[i], bool(inf[i])).to_uncompressed() == want[i], i
    bases.free()


def test_on_a_caller_stream_and_between_pipelined_msm_calls(ctx):
    """the device form on a non-default stream set with set_stream, then enqueued between two pipelined msm_device calls"""
    import torch
    dev = torch.device("cuda", 0)
    x = _raw(24 << 9, 77).reshape(24, 1 << 9, 4)
    x2 = _raw(3 << 13, 78).reshape(3, 1 << 13, 4)
    pw, pwi = _powers(G7, 1 << 9), _powers(pow(G7, -1, RR), 1 << 13)             # the expectations: the single-vector path
    want = np.stack([ctx.fr_ntt(ctx.fr_op(0, v, pw)) for v in x])
    want2 = np.stack([ctx.fr_op(0, ctx.fr_ntt(v, inverse=True), pwi) for v in x2])
    side = torch.cuda.Stream(device=dev)
    d_x = torch.from_numpy(x.view(np.int64)).to(dev)
    d_x2 = torch.from_numpy(x2.view(np.int64)).to(dev)
    torch.cuda.synchronize()
    ctx.set_stream(side.cuda_stream)
    try:
        ctx.fr_ntt_many_device(d_x.data_ptr(), 9, 24, coset=G7)
        ctx.fr_ntt_many_device(d_x2.data_ptr(), 13, 3, inverse=True, coset=G7)
        ctx.synchronize()
    finally:
        ctx.set_stream(None)
    assert np.array_equal(d_x.cpu().numpy().view(np.uint64).reshape(x.shape), want)
    assert np.array_equal(d_x2.cpu().numpy().view(np.uint64).reshape(x2.shape), want2)
    # between pipelined MSM calls
    n = 1 << 14
    S = np.random.RandomState(5).randint(0, 256, size=(2 * n, 32), dtype=np.uint8)
    S[:, 31] &= 0x3F
    bases = ctx.bases_from_scalars(1, S[:n])
    d_s = torch.from_numpy(S).to(dev)
    d_msm = torch.zeros((2, 18), dtype=torch.int64, device=dev)
    d_x = torch.from_numpy(x.view(np.int64)).to(dev)
    torch.cuda.synchronize()
    ctx.set_pipelining(True)
    try:
        ctx.msm_device(bases, d_s[0:n].data_ptr(), n, d_msm[0].data_ptr())
        ctx.fr_ntt_many_device(d_x.data_ptr(), 9, 24, coset=G7)
        ctx.msm_device(bases, d_s[n:2 * n].data_ptr(), n, d_msm[1].data_ptr())
        ctx.join()
        ctx.synchronize()
    finally:
        ctx.set_pipelining(False)
    assert np.array_equal(d_x.cpu().numpy().view(np.uint64).reshape(x.shape), want)
    got = ctx.batch_normalize(1, d_msm.cpu().numpy().view(np.uint64))
    for i in range(2):
        ref = ctx.batch_normalize(1, ctx.msm(bases, S[i * n:(i + 1) * n])[None, :])
        assert np.array_equal(got[0][i], ref[0][0]) and got[1][i] == ref[1][0], i
    bases.free()


def test_arguments(ctx):
    """every refusal is BLSGPU_ERR_ARG with a text, before anything is staged or launched, and leaves the context usable; k = 0 is a no-op"""
    import torch
    import bls12_381_amd as b
    lib, h = ctx.lib, ctx.h
    x = _raw(8, 1)
    keep = x.copy()
    p = x.ctypes.data_as(ctypes.c_void_p)
    g7 = _limbs([G7])[0]
    zero = np.zeros(4, dtype=np.uint64)
    r_limbs = np.frombuffer(RR.to_bytes(32, "little"), dtype=np.uint64).copy()
    d = torch.zeros(8 * 4, dtype=torch.int64, device=torch.device("cuda", 0))
    cp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    err = lambda: lib.blsgpu_last_error().decode()
    for fn, ptr in ((lib.blsgpu_fr_ntt_many, p), (lib.blsgpu_fr_ntt_many_device, ctypes.c_void_p(d.data_ptr()))):
        assert fn(h, ptr, 29, 1, 0, None) == ERR_ARG and "log_n" in err()
        assert fn(h, ptr, -1, 1, 0, None) == ERR_ARG
        for log_n in (0, 3, 28):
            assert fn(h, ptr, log_n, ((1 << 28) >> log_n) + 1, 0, None) == ERR_ARG and "2^28" in err()
        assert fn(h, ptr, 3, (1 << 64) - 1, 0, None) == ERR_ARG                 # k * 2^log_n overflows 64 bits
        assert fn(h, None, 3, 1, 0, None) == ERR_ARG and "NULL" in err()
        assert fn(h, ptr, 3, 1, 0, cp(zero)) == ERR_ARG and "zero" in err()
        assert fn(h, ptr, 3, 1, 1, cp(r_limbs)) == ERR_ARG and "canonical" in err()
        assert fn(h, ptr, 3, 0, 0, cp(g7)) == 0 and fn(h, None, 3, 0, 0, None) == 0          # k == 0
    ctx.synchronize()
    assert np.array_equal(x, keep) and not d.cpu().numpy().any()
    with pytest.raises(ValueError):
        ctx.fr_ntt_many(x.reshape(1, 8, 4), coset=0)
    with pytest.raises(ValueError):
        ctx.fr_ntt_many(np.zeros((2, 3, 4), dtype=np.uint64))
    assert b.FR_GENERATOR == 7
    # the context is still usable, and k == 0 through the Python form returns an empty array
    assert np.array_equal(ctx.fr_ntt_many(x.reshape(1, 8, 4))[0], ctx.fr_ntt(x))
    assert ctx.fr_ntt_many(np.zeros((0, 8, 4), dtype=np.uint64)).shape == (0, 8, 4)


def test_cpp_mirror(ctx, tmp_path):
    """include/bls12_381.hpp fr_ntt_many compiled with g++ against libblsgpu.so: round trip with a coset, k = 1 equals fr_ntt"""
    import bls12_381_amd as b
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "fr_ntt_many_test")
    libdir = os.path.dirname(b.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "fr_ntt_many_test.cpp"),
                           "-L" + libdir, "-lblsgpu", "-Wl,-rpath," + libdir, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "fr_ntt_many ok" in out.stdout, out.stdout + out.stderr
