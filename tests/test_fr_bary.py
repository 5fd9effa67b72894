"""Evaluation-form openings (`blsgpu_fr_bary_eval_many*`, `blsgpu_fr_bary_open_many*`; csrc/fr_bary.hip.h + csrc/fr_bary_plan.h) on the GPU.

Expectations are Python integers by the definition (tests/fr_bary_ref.py: interpolate with the oracle's fr_ntt, Horner, synthetic division,
transform the quotient back), compared limb for limb; the two large shapes are compared with the coefficient-form route the library already
had (inverse fr_ntt_many, fr_scan HORNER, forward fr_ntt_many), which must agree to the limb since y and q are unique canonical values."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import fr_bary_ref as ref
from oracle import bls12_381_ref as o

pytestmark = pytest.mark.gpu

RR = ref.RR
ERR_ARG = -2
NAT, REV = ref.NATURAL, ref.BITREV
T = 256 * 8                                                        # csrc/fr_bary_plan.h: FRB_BLOCK * FRB_CHUNK, the tile


@pytest.fixture(scope="module")
def ctx():
    import bls12_381_amd as b
    assert (b.FR_ORDER_NATURAL, b.FR_ORDER_BITREV) == (NAT, REV)
    c = b.Context(0)
    yield c
    c.close()


def _limbs(vals):
    return ref.words(vals).view(np.uint64).reshape(-1, 4).copy()


def _raw(n, seed):
    """n canonical `Scalar`s as raw limbs (any integer below r is the Montgomery form of some scalar)"""
    s = np.random.RandomState(seed).randint(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= 0x3F                                               # < 2^254 < r
    return s.view(np.uint64).reshape(n, 4).copy()


def _values(limbs):
    """(m, 4) u64 Montgomery limbs -> the integers they stand for"""
    rinv = pow(ref.MONT, -1, RR)
    return [v * rinv % RR for v in ref.raw_ints(np.ascontiguousarray(limbs).view(np.uint32))]


def _hit_rows(log_n, k):
    """{row: j}: a hit row with j at an end of the row and one with j at a tile boundary where the row has one; row 0 stays random
    whenever k allows it"""
    n = 1 << log_n
    js = [n - 1, 0]
    if n > T:
        js = [n - 1, T, T - 1, 0]
    if k == 1:
        return {}
    if k == 2:
        return {1: js[0]}
    return {1 + 2 * i: j for i, j in enumerate(js) if 1 + 2 * i < k}


@pytest.mark.parametrize("log_n,k", [(0, 5), (1, 3), (6, 1000), (11, 3), (12, 16), (13, 2)])
def test_against_python_integers(ctx, log_n, k):
    """eval and open in both orders, limb equality of every y and every q[i]: random rows, a row whose point is D[j] with j at an end of
    the row, and rows with j on either side of a tile boundary where rows are longer than a tile (with k = 2 the bit-reversed call takes
    the tile boundary, the natural one the end of the row)"""
    n = 1 << log_n
    x = _raw(k * n, 11 * log_n + k).reshape(k, n, 4)
    rows = [_values(x[v]) for v in range(k)]
    for order in (NAT, REV):
        r = o.SplitMix64(log_n + k + order)
        zs = [r.scalar() for _ in range(k)]
        hits = _hit_rows(log_n, k)
        if k == 2 and order == REV and n > T:
            hits = {1: T}
        if k == 3 and log_n == 1:
            hits = {1: 0, 2: 1}
        for v, j in hits.items():
            zs[v] = ref.domain_point(log_n, order, j)
        want = [ref.expect(rows[v], zs[v], order) for v in range(k)]
        want_y = _limbs([w[0] for w in want])
        want_q = _limbs([a for w in want for a in w[1]]).reshape(k, n, 4)
        y, q = ctx.fr_bary_open(x, zs, order=order)
        bad = np.argwhere((y != want_y).any(axis=1))
        assert not len(bad), "open, order=%d: y differs in rows %s" % (order, bad[:8].ravel())
        bad = np.argwhere((q != want_q).any(axis=2))
        assert not len(bad), "open, order=%d: %d quotient values differ, first (row, index) %s" % (order, len(bad), bad[0])
        for v, j in hits.items():
            assert np.array_equal(y[v], x[v, j]), "y of a hit row is f[j]"
        assert np.array_equal(ctx.fr_bary_eval(x, zs, order=order), want_y), "eval, order=%d" % order
        # the limb form of the points and the integer form are the same call; an (n, 4) array is k = 1
        assert np.array_equal(ctx.fr_bary_eval(x, _limbs(zs), order=order), want_y)
        y0, q0 = ctx.fr_bary_open(x[0], zs[:1], order=order)
        assert np.array_equal(y0, want_y[0]) and np.array_equal(q0, want_q[0])


def _bitrev_index(log_n):
    i = np.arange(1 << log_n, dtype=np.uint64)
    out = np.zeros_like(i)
    for b in range(log_n):
        out |= ((i >> np.uint64(b)) & np.uint64(1)) << np.uint64(log_n - 1 - b)
    return out.astype(np.int64)


@pytest.mark.parametrize("log_n,k,order", [(16, 4, NAT), (16, 4, REV), (20, 1, NAT)])
def test_against_the_composed_device_route(ctx, log_n, k, order):
    """limb equality with inverse fr_ntt_many -> fr_scan(HORNER) -> forward fr_ntt_many on the device; the last row's point is D[j] with j
    in the row's last tile"""
    import torch
    dev = torch.device("cuda", 0)
    n = 1 << log_n
    x = _raw(k * n, 5 * log_n + k).reshape(k, n, 4)
    r = o.SplitMix64(log_n)
    zs = [r.scalar() for _ in range(k)]
    j = n - T + 5
    zs[k - 1] = ref.domain_point(log_n, NAT, j)                   # = D[perm[j]] of the bit-reversed order
    perm = torch.from_numpy(_bitrev_index(log_n)).to(dev)
    d_nat = torch.from_numpy(x.view(np.int64)).to(dev)             # the rows in natural order
    d_z = torch.from_numpy(_limbs(zs).view(np.int64)).to(dev)
    # the composed route, on the natural-order rows
    d_c = d_nat.clone()
    d_h = torch.zeros_like(d_c)
    torch.cuda.synchronize()
    ctx.fr_ntt_many_device(d_c.data_ptr(), log_n, k, inverse=True)
    ctx.fr_scan_device(2, d_c.data_ptr(), n, k, d_h.data_ptr(), d_points=d_z.data_ptr())
    ctx.synchronize()
    want_y = d_h[:, 0, :].clone()
    d_qc = torch.cat([d_h[:, 1:, :], torch.zeros((k, 1, 4), dtype=torch.int64, device=dev)], dim=1).contiguous()
    torch.cuda.synchronize()
    ctx.fr_ntt_many_device(d_qc.data_ptr(), log_n, k, inverse=False)
    ctx.synchronize()
    # the fused call, on the rows in the order under test
    d_in = d_nat if order == NAT else d_nat[:, perm, :].contiguous()
    d_y = torch.zeros((k, 4), dtype=torch.int64, device=dev)
    d_q = torch.zeros((k, n, 4), dtype=torch.int64, device=dev)
    d_y2 = torch.zeros((k, 4), dtype=torch.int64, device=dev)
    keep = d_in.clone()
    torch.cuda.synchronize()
    ctx.fr_bary_open_device(d_in.data_ptr(), log_n, k, d_z.data_ptr(), d_y.data_ptr(), d_q.data_ptr(), order=order)
    ctx.fr_bary_eval_device(d_in.data_ptr(), log_n, k, d_z.data_ptr(), d_y2.data_ptr(), order=order)
    ctx.synchronize()
    want_q = d_qc if order == NAT else d_qc[:, perm, :]
    assert torch.equal(d_y, want_y) and torch.equal(d_y2, want_y)
    assert torch.equal(d_y[k - 1], d_nat[k - 1, j]), "y of the hit row is f[j]"
    bad = (d_q != want_q).any(dim=2).nonzero()
    assert not len(bad), "%d quotient values differ, first (row, index) %s" % (len(bad), bad[0].tolist())
    assert torch.equal(d_in, keep), "the input was written to"


def test_device_forms_chained_on_the_stream_equal_the_host_forms(ctx):
    """eval and open of two shapes enqueued back to back on the context's stream, and again on a caller's stream: the limbs of the host
    forms (checked against integers above); the second shape re-uses the scratch of the first"""
    import torch
    dev = torch.device("cuda", 0)
    shapes = [(12, 5, REV), (7, 33, NAT), (12, 5, NAT)]
    data, want = [], []
    for log_n, k, order in shapes:
        n = 1 << log_n
        x = _raw(k * n, log_n + k + order).reshape(k, n, 4)
        zs = [o.SplitMix64(v + log_n).scalar() for v in range(k)]
        zs[k - 1] = ref.domain_point(log_n, order, n // 2 + 1)
        data.append((x, _limbs(zs)))
        want.append(ctx.fr_bary_open(x, zs, order=order))
        assert np.array_equal(ctx.fr_bary_eval(x, zs, order=order), want[-1][0])

    def run():
        bufs = []
        for (log_n, k, order), (x, z) in zip(shapes, data):
            n = 1 << log_n
            bufs.append((torch.from_numpy(x.view(np.int64)).to(dev), torch.from_numpy(z.view(np.int64)).to(dev), torch.zeros((k, 4), dtype=torch.int64, device=dev),
                         torch.zeros((k, n, 4), dtype=torch.int64, device=dev), torch.zeros((k, 4), dtype=torch.int64, device=dev)))
        torch.cuda.synchronize()
        for (log_n, k, order), (d_x, d_z, d_y, d_q, d_y2) in zip(shapes, bufs):
            ctx.fr_bary_open_device(d_x.data_ptr(), log_n, k, d_z.data_ptr(), d_y.data_ptr(), d_q.data_ptr(), order=order)
            ctx.fr_bary_eval_device(d_x.data_ptr(), log_n, k, d_z.data_ptr(), d_y2.data_ptr(), order=order)
        ctx.synchronize()
        for (wy, wq), (x, _), (d_x, d_z, d_y, d_q, d_y2) in zip(want, data, bufs):
            assert np.array_equal(d_y.cpu().numpy().view(np.uint64), wy) and np.array_equal(d_y2.cpu().numpy().view(np.uint64), wy)
            assert np.array_equal(d_q.cpu().numpy().view(np.uint64), wq)
            assert np.array_equal(d_x.cpu().numpy().view(np.uint64), x)

    run()
    side = torch.cuda.Stream(device=dev)
    ctx.set_stream(side.cuda_stream)
    try:
        run()
    finally:
        ctx.set_stream(None)


def test_the_lagrange_opening_chain_on_the_device(ctx):
    """a KZG opening over a Lagrange SRS with no host copy and no transform: 2^12 evaluations in device memory -> fr_bary_open_device ->
    msm_mont_device over [L_i(tau)] G reading all n quotient values at d_q -> [q(tau)] G, and p(tau) - y = q(tau) (tau - z) in integers"""
    import torch
    import bls12_381_amd as b
    log_n = 12
    n = 1 << log_n
    r = o.SplitMix64(0x1A6)
    f = [r.scalar() for _ in range(n)]
    z, tau = r.scalar(), r.scalar()
    w = o.fr_omega(log_n)
    c = (pow(tau, n, RR) - 1) * pow(n, -1, RR) % RR
    lag, wi = [], 1
    for i in range(n):                                             # L_i(tau) = (tau^n - 1) / n * w^i / (tau - w^i)
        lag.append(c * wi % RR * pow(tau - wi, -1, RR) % RR)
        wi = wi * w % RR
    y, q = ref.expect(f, z, NAT)
    p_tau = sum(a * l for a, l in zip(f, lag)) % RR
    q_tau = sum(a * l for a, l in zip(q, lag)) % RR
    assert (p_tau - y) % RR == q_tau * (tau - z) % RR
    want = o.g1_to_uncompressed(o.g1_to_affine(o.g1_affine_mul(o.G1_GEN, q_tau)))
    dev = torch.device("cuda", 0)
    bases = ctx.bases_from_scalars(1, lag)
    d_f = torch.from_numpy(_limbs(f).view(np.int64)).to(dev)
    d_z = torch.from_numpy(_limbs([z]).view(np.int64)).to(dev)
    d_y = torch.zeros((1, 4), dtype=torch.int64, device=dev)
    d_q = torch.zeros((n, 4), dtype=torch.int64, device=dev)
    d_out = torch.zeros(18, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ctx.fr_bary_open_device(d_f.data_ptr(), log_n, 1, d_z.data_ptr(), d_y.data_ptr(), d_q.data_ptr())
    ctx.msm_mont_device(bases, d_q.data_ptr(), n, d_out.data_ptr())
    ctx.synchronize()
    assert np.array_equal(d_y.cpu().numpy().view(np.uint64), _limbs([y]))
    xy, inf = ctx.batch_normalize(1, d_out.cpu().numpy().view(np.uint64)[None, :])
    assert b.G1Affine(xy[0], bool(inf[0])).to_uncompressed() == want
    bases.free()


def test_arguments(ctx):
    """every refusal is BLSGPU_ERR_ARG with a text naming the cause, before anything is staged or launched: nothing is written to an
    input or an output, and the context works afterwards; k == 0 is a no-op"""
    import torch
    lib, h = ctx.lib, ctx.h
    log_n, k = 4, 2
    n = 1 << log_n
    x = _raw(k * n + n, 1)                                         # one spare row behind the data: room for overlapping ranges
    z = _raw(k + 2, 2)
    y = np.zeros((k + 2, 4), dtype=np.uint64)
    q = np.zeros((k * n + n, 4), dtype=np.uint64)
    keep_x, keep_z = x.copy(), z.copy()
    dev = torch.device("cuda", 0)
    d_x = torch.from_numpy(x.view(np.int64)).to(dev)
    d_z = torch.from_numpy(z.view(np.int64)).to(dev)
    d_y = torch.zeros((k + 2, 4), dtype=torch.int64, device=dev)
    d_q = torch.zeros((k * n + n, 4), dtype=torch.int64, device=dev)
    vp = ctypes.c_void_p
    err = lambda: lib.blsgpu_last_error().decode()
    host = (lib.blsgpu_fr_bary_eval_many, lib.blsgpu_fr_bary_open_many, x.ctypes.data, z.ctypes.data, y.ctypes.data, q.ctypes.data)
    devf = (lib.blsgpu_fr_bary_eval_many_device, lib.blsgpu_fr_bary_open_many_device, d_x.data_ptr(), d_z.data_ptr(), d_y.data_ptr(), d_q.data_ptr())
    for ev, op, px, pz, py, pq in (host, devf):
        def both(log_n_, k_, ax, az, order, ay, aq, what):
            c = lambda a: None if a is None else vp(a)
            assert ev(h, c(ax), log_n_, k_, c(az), order, c(ay)) == ERR_ARG and what in err(), (what, err())
            assert op(h, c(ax), log_n_, k_, c(az), order, c(ay), c(aq)) == ERR_ARG and what in err(), (what, err())
        both(log_n, k, None, pz, NAT, py, pq, "NULL")
        both(log_n, k, px, None, NAT, py, pq, "NULL")
        both(log_n, k, px, pz, NAT, None, pq, "NULL")
        assert op(h, vp(px), log_n, k, vp(pz), NAT, vp(py), None) == ERR_ARG and "NULL" in err()
        both(-1, k, px, pz, NAT, py, pq, "log_n")
        both(29, 1, px, pz, NAT, py, pq, "log_n")
        both(log_n, (1 << 24) + 1, px, pz, NAT, py, pq, "2^28")
        both(28, 2, px, pz, NAT, py, pq, "2^28")
        both(log_n, (1 << 64) - 1, px, pz, NAT, py, pq, "2^28")      # k * 2^log_n overflows 64 bits
        both(log_n, (1 << 60) + 1, px, pz, NAT, py, pq, "2^28")
        both(log_n, k, px, pz, 2, py, pq, "order")
        both(log_n, k, px, pz, -1, py, pq, "order")
        both(log_n, k, px, pz, NAT, px + 32, pq, "overlap")        # y inside evals
        both(log_n, k, px, pz, NAT, px + k * n * 32 - 32, pq, "overlap")      # y on the last scalar of evals
        both(log_n, k, px, pz, NAT, pz + 32, pq, "overlap")        # y on points[1]
        for bad_q in (px, px + 32, px + n * 32, px + k * n * 32 - 32):      # q == evals (no in-place form), q inside evals, q on its last scalar
            assert op(h, vp(px), log_n, k, vp(pz), NAT, vp(py), vp(bad_q)) == ERR_ARG and "overlap" in err()
        assert op(h, vp(px), log_n, k, vp(pq + 32), NAT, vp(py), vp(pq)) == ERR_ARG and "overlap" in err()      # points inside q
        assert op(h, vp(px), log_n, k, vp(pz), NAT, vp(pq + 64), vp(pq)) == ERR_ARG and "overlap" in err()      # y inside q
        assert op(h, vp(px), log_n, k, vp(pz), NAT, vp(pq + k * n * 32 - 32), vp(pq)) == ERR_ARG and "overlap" in err()
        assert ev(h, vp(px), log_n, 0, vp(pz), NAT, vp(py)) == 0 and ev(h, None, log_n, 0, None, REV, None) == 0
        assert op(h, vp(px), log_n, 0, vp(pz), NAT, vp(py), vp(pq)) == 0 and op(h, None, 28, 0, None, NAT, None, None) == 0
    ev, op, px, pz, py, pq = devf
    for args in ((px + 8, pz, py, pq), (px, pz + 8, py, pq), (px, pz, py + 8, pq), (px, pz, py, pq + 8)):
        assert op(h, vp(args[0]), log_n, k, vp(args[1]), NAT, vp(args[2]), vp(args[3])) == ERR_ARG and "aligned" in err()
    for args in ((px + 8, pz, py), (px, pz + 8, py), (px, pz, py + 8)):
        assert ev(h, vp(args[0]), log_n, k, vp(args[1]), NAT, vp(args[2])) == ERR_ARG and "aligned" in err()
    ctx.synchronize()
    assert np.array_equal(x, keep_x) and np.array_equal(z, keep_z) and not y.any() and not q.any()
    assert np.array_equal(d_x.cpu().numpy().view(np.uint64), keep_x) and np.array_equal(d_z.cpu().numpy().view(np.uint64), keep_z)
    assert not d_y.cpu().numpy().any() and not d_q.cpu().numpy().any()
    with pytest.raises(ValueError):
        ctx.fr_bary_eval(np.zeros((2, 3, 4), dtype=np.uint64), [1, 2])      # not a power of two
    with pytest.raises(ValueError):
        ctx.fr_bary_open(np.zeros((2, 4, 5), dtype=np.uint64), [1, 2])
    with pytest.raises(ValueError):
        ctx.fr_bary_open(np.zeros((2, 4, 4), dtype=np.uint64), [1])
    # the context is still usable
    rows = x[:k * n].reshape(k, n, 4)
    zs = [5, ref.domain_point(log_n, NAT, 3)]
    yy, qq = ctx.fr_bary_open(rows, zs)
    want = [ref.expect(_values(rows[v]), zs[v], NAT) for v in range(k)]
    assert np.array_equal(yy, _limbs([w[0] for w in want])) and np.array_equal(qq.reshape(-1, 4), _limbs([a for w in want for a in w[1]]))
    assert ctx.fr_bary_eval(np.zeros((0, 8, 4), dtype=np.uint64), []).shape == (0, 4)


def test_cpp_mirror(ctx, tmp_path):
    """include/bls12_381.hpp fr_bary_eval / fr_bary_open compiled with g++ against libblsgpu.so, against the coefficient-form route of the
    same header"""
    import bls12_381_amd as b
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "fr_bary_test")
    libdir = os.path.dirname(b.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "fr_bary_test.cpp"),
                           "-L" + libdir, "-lblsgpu", "-Wl,-rpath," + libdir, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "fr_bary ok" in out.stdout, out.stdout + out.stderr
