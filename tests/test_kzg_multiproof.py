"""Amortised KZG openings on the GPU (`blsgpu_kzg_multiproof_*`, `blsgpu_kzg_cells*`; csrc/kzg.hip.h + csrc/kzg_plan.h), through the C ABI
and the Python mirror.

Every comparison is exact.  Proofs are compared as affine points after `batch_normalize` with [s] G1 from the oracle's `g1_mul`, where s
is the scalar the DEFINITION gives (tests/kzg_ref.py: q_i = floor(p / (X^l - a_i)) by the recurrence, s = sum_u q_i[u] sigma_u).  The SRS
of the exactness cases is S[m] = [sigma_m] G1 with independent random sigma_m -- NOT powers of one tau: the definition is linear in S,
and a geometric SRS hides index slips that an arbitrary one shows.  sigma_1 = 0 puts an identity among the S[m]; the first polynomial
carries 0, 1 and r - 1 among its coefficients.

The EIP-7594 shape (n = 4096, l = 64, evaluation form, bit-reversed) runs once with S[m] = [tau^m] G1: all 256 proofs against
[q_i(tau)] G1.  Its 2 x 8192 cell values are compared with the oracle's transform of the zero-extended coefficients (`fr_ntt`, the
recursive evaluation of the defining sum, pinned against the O(n^2) sums by the oracle's own tests) and 128 seeded positions of them with
Horner evaluation at the point itself: Horner at all 16384 points is 6.7 * 10^7 big-integer products, over 20 s in this interpreter."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import bls12_381_ref as o
import kzg_ref as k
from g_sum_points import _off_subgroup, wire_points

pytestmark = pytest.mark.gpu

ERR_ARG = -2
SCALAR_BYTES, SCALAR_MONT = 0, 1                                  # BLSGPU_SCALAR_*
R = o.R_ORDER
COUNT = 3
SHAPES = [(4, 2), (3, 0), (3, 3), (6, 1), (8, 2), (8, 6)]
# (log_n, log_l, form, order): every shape in coefficient form and natural order, both forms x both orders on (4, 2) and (8, 2)
CASES = [(n, l, k.COEFFS, k.NATURAL) for n, l in SHAPES] + [(n, l, f, r) for n, l in ((4, 2), (8, 2)) for f in (k.COEFFS, k.EVALS) for r in (k.NATURAL, k.BITREV)
                                                             if (f, r) != (k.COEFFS, k.NATURAL)]


@pytest.fixture(scope="module")
def ctx():
    import bls12_381_amd as b
    c = b.Context(0)
    yield c
    c.close()


def _limbs(vals):
    return np.array([o.fr_to_mont_limbs(int(v) % R) for v in vals], dtype=np.uint64).reshape(-1, 4)


def _ints(limbs):
    return [o.fr_from_mont_limbs([int(w) for w in row]) for row in np.asarray(limbs).reshape(-1, 4)]


@functools.lru_cache(maxsize=None)
def _inputs(log_n, log_l):
    """(sigma, polys): seeded; sigma_1 = 0 (an identity in the SRS), polys[0] starts 0, 1, r - 1 where there is room"""
    rng = o.SplitMix64(1000 + 16 * log_n + log_l)
    n = 1 << log_n
    sigma = [rng.scalar() for _ in range(n)]
    sigma[1] = 0
    polys = [k.random_poly(rng, n) for _ in range(COUNT)]
    for j, v in enumerate((0, 1, R - 1)[:n]):
        polys[0][n - 1 - j] = v                                   # the top coefficients: they reach every quotient
    return sigma, polys


@functools.lru_cache(maxsize=None)
def _want(log_n, log_l, order):
    """the proofs of _inputs by the definition, as affine wire points"""
    sigma, polys = _inputs(log_n, log_l)
    scalars = [s for p in polys for s in k.proofs_by_division(p, sigma, log_n, log_l, order)]
    return _points(scalars)


def _points(scalars):
    return wire_points(1, [o.g1_to_affine(o.g1_mul(o.g1_from_affine(o.G1_GEN), s)) for s in scalars])


def _srs(ctx, sigma):
    return ctx.bases_from_scalars(1, [int(s) for s in sigma])


def _same(ctx, out_xyz, want, what):
    xy, inf = ctx.batch_normalize(1, np.ascontiguousarray(out_xyz).reshape(-1, 18))
    wxy, winf = want
    assert np.array_equal(inf != 0, winf != 0), "%s: identities at %s, wanted at %s" % (what, np.nonzero(inf)[0][:8], np.nonzero(winf)[0][:8])
    live = winf == 0
    bad = np.nonzero((xy != wxy).any(axis=1) & live)[0]
    assert bad.size == 0, "%s: %d proofs differ, first %s" % (what, bad.size, bad[:8])


def _form_input(polys, form, order):
    return _limbs([v for p in polys for v in (k.to_evals(p, order) if form == k.EVALS else p)]).reshape(len(polys), -1, 4)


def _device_proofs(ctx, handle, polys_limbs, form, order, sync=True):
    import torch
    dev = torch.device("cuda", 0)
    count = polys_limbs.shape[0]
    d_in = torch.from_numpy(np.ascontiguousarray(polys_limbs).view(np.int64).reshape(-1).copy()).to(dev)
    d_out = torch.full((count * handle.cells * 18,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=dev)
    handle.proofs_device(d_in.data_ptr(), count, d_out.data_ptr(), form, order)
    if sync:
        ctx.synchronize()
    return d_in, d_out


def _host(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("log_n,log_l,form,order", CASES, ids=["%d-%d-%s-%s" % (n, l, "evals" if f else "coeffs", "bitrev" if r else "natural") for n, l, f, r in CASES])
def test_proofs_match_the_definition_over_an_arbitrary_srs(ctx, log_n, log_l, form, order):
    sigma, polys = _inputs(log_n, log_l)
    want = _want(log_n, log_l, order)
    srs = _srs(ctx, sigma)
    h = ctx.kzg_multiproof_create(srs, log_n, log_l)
    srs.free()                                                    # the handle keeps no reference to the SRS
    try:
        assert (h.log_n, h.log_l, h.cells) == (log_n, log_l, 2 << (log_n - log_l))
        x = _form_input(polys, form, order)
        keep = x.copy()
        _same(ctx, h.proofs(x, form, order), want, "host form")
        assert np.array_equal(x, keep)
        d_in, d_out = _device_proofs(ctx, h, x, form, order)
        _same(ctx, _host(d_out), want, "device form")
        assert np.array_equal(_host(d_in).reshape(x.shape), keep), "the device form wrote the caller's polynomials"
    finally:
        h.close()


def test_the_data_availability_shape_with_a_powers_of_tau_srs(ctx):
    """(12, 6), two blobs in evaluation form and bit-reversed order: 128 cells and 128 cell proofs each"""
    log_n, log_l, n = 12, 6, 4096
    rng = o.SplitMix64(7594)
    tau = rng.scalar()
    sigma = [pow(tau, m, R) for m in range(n)]
    polys = [k.random_poly(rng, n) for _ in range(2)]
    x = _form_input(polys, k.EVALS, k.BITREV)
    srs = _srs(ctx, sigma)
    h = ctx.kzg_multiproof_create(srs, log_n, log_l)
    try:
        out = h.proofs(x, k.EVALS, k.BITREV)
        assert out.shape == (2, 128, 18)
        want = [s for p in polys for s in k.proofs_by_division(p, sigma, log_n, log_l, k.BITREV)]      # q_i(tau)
        _same(ctx, out, _points(want), "cell proofs")
        cells = ctx.kzg_cells(x, log_l, k.EVALS, k.BITREV)
        assert cells.shape == (2, 128, 64, 4)
        w = o.fr_omega(log_n + 1)
        pick = np.random.RandomState(4844)
        for v, p in enumerate(polys):
            assert np.array_equal(cells[v].reshape(-1, 4), _limbs([e for row in k.cells_by_ntt(p, log_n, log_l, k.BITREV) for e in row])), "cells of blob %d" % v
            for i, t in zip(pick.randint(0, 128, 64), pick.randint(0, 64, 64)):
                z = pow(w, k.cell_point_exponent(int(i), int(t), log_n, log_l, k.BITREV), R)
                assert _ints(cells[v, i, t]) == [k.evaluate(p, z)], "cell %d entry %d of blob %d" % (i, t, v)
    finally:
        h.close()
        srs.free()


def test_single_point_openings_equal_horner_quotients_through_the_segmented_msm(ctx):
    """(3, 0): l = 1, every proof a single-point opening at w^i -- the route the library already had"""
    import bls12_381_amd as b
    log_n, n = 3, 8
    sigma, polys = _inputs(3, 0)
    srs = _srs(ctx, sigma)
    h = ctx.kzg_multiproof_create(srs, log_n, 0)
    try:
        got = h.proofs(_limbs([v for p in polys for v in p]).reshape(COUNT, n, 4))
        w = o.fr_omega(log_n + 1)
        rows = _limbs([v for p in polys for i in range(2 * n) for v in p]).reshape(COUNT * 2 * n, n, 4)
        pts = [pow(w, i, R) for _ in polys for i in range(2 * n)]
        q = ctx.fr_scan(b.FR_SCAN_HORNER, rows, pts)[:, 1:, :]                       # n - 1 quotient coefficients per opening
        nseg = COUNT * 2 * n
        off = np.arange(nseg + 1, dtype=np.uint32) * (n - 1)
        want = ctx.msm_segments(srs, ctx.fr_to_bytes(np.ascontiguousarray(q).reshape(-1, 4)), off, base_first=np.zeros(nseg, dtype=np.uint32))
        a, b_ = ctx.batch_normalize(1, got.reshape(-1, 18)), ctx.batch_normalize(1, want)
        assert np.array_equal(a[1], b_[1]) and np.array_equal(a[0][a[1] == 0], b_[0][b_[1] == 0])
    finally:
        h.close()
        srs.free()


def test_cells_of_single_points_are_the_transform_of_the_zero_extended_rows(ctx):
    log_n, n = 6, 64
    _, polys = _inputs(6, 1)
    x = _limbs([v for p in polys for v in p]).reshape(COUNT, n, 4)
    ext = np.zeros((COUNT, 2 * n, 4), dtype=np.uint64)
    ext[:, :n] = x
    assert np.array_equal(ctx.kzg_cells(x, 0).reshape(COUNT, 2 * n, 4), ctx.fr_ntt_many(ext))


@pytest.mark.parametrize("log_n,log_l", [(4, 2), (8, 2), (8, 6), (3, 3), (0, 0)])
@pytest.mark.parametrize("form,order", [(k.COEFFS, k.NATURAL), (k.COEFFS, k.BITREV), (k.EVALS, k.NATURAL), (k.EVALS, k.BITREV)])
def test_cells_match_direct_evaluation(ctx, log_n, log_l, form, order):
    rng = o.SplitMix64(50 + log_n)
    polys = [k.random_poly(rng, 1 << log_n) for _ in range(COUNT)]
    x = _form_input(polys, form, order)
    host = ctx.kzg_cells(x, log_l, form, order)
    want = _limbs([e for p in polys for row in k.cells(p, log_n, log_l, order) for e in row]).reshape(host.shape)
    assert np.array_equal(host, want)
    import torch
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(x.view(np.int64).reshape(-1).copy()).to(dev)
    d_out = torch.zeros(host.size, dtype=torch.int64, device=dev)
    ctx.kzg_cells_device(d_in.data_ptr(), log_n, log_l, COUNT, d_out.data_ptr(), form, order)
    ctx.synchronize()
    assert np.array_equal(_host(d_out).reshape(host.shape), want) and np.array_equal(_host(d_in).reshape(x.shape), x)


def test_edges(ctx):
    log_n, log_l, n = 4, 2, 16
    sigma, polys = _inputs(log_n, log_l)
    srs = _srs(ctx, sigma)
    h = ctx.kzg_multiproof_create(srs, log_n, log_l)
    one = ctx.kzg_multiproof_create(srs, 3, 3)                    # c = 1
    try:
        ident = (np.zeros((8, 12), dtype=np.uint64), np.ones(8, dtype=np.uint8))
        # the zero polynomial, and a polynomial of degree < l: 2c identities each
        low = [polys[1][j] if j < 4 else 0 for j in range(n)]
        out = h.proofs(_limbs([0] * n + low).reshape(2, n, 4))
        _same(ctx, out[0], ident, "zero polynomial")
        _same(ctx, out[1], ident, "degree < l")
        # count = 0 is a no-op, through the mirror and with NULL pointers through the ABI
        assert h.proofs(np.zeros((0, n, 4), dtype=np.uint64)).shape == (0, 8, 18)
        assert ctx.lib.blsgpu_kzg_multiproof_proofs_device(ctx.h, h.handle, None, 0, 0, 0, None) == 0
        assert ctx.lib.blsgpu_kzg_cells_device(ctx.h, None, 4, 2, 0, 0, 0, None) == 0
        # c = 1: two identities, no MSM
        out = one.proofs(_limbs(polys[0][:8] + polys[1][:8]).reshape(2, 8, 4), k.COEFFS, k.BITREV)
        _same(ctx, out, (ident[0][:4], ident[1][:4]), "c = 1")
        # the same handle for two calls back to back on one stream, without a synchronisation in between; identical from run to run
        x = _form_input(polys, k.COEFFS, k.NATURAL)
        _, first = _device_proofs(ctx, h, x, k.COEFFS, k.NATURAL, sync=False)
        _, second = _device_proofs(ctx, h, x[::-1].copy(), k.COEFFS, k.NATURAL, sync=False)
        ctx.synchronize()
        want = _want(log_n, log_l, k.NATURAL)
        _same(ctx, _host(first), want, "first of two calls")
        _same(ctx, _host(second).reshape(COUNT, 8, 18)[::-1], want, "second of two calls")
        again = h.proofs(x)
        assert np.array_equal(again, h.proofs(x)) and np.array_equal(again.reshape(-1), _host(first)), "results differ from run to run"
        # the context's scalar form does not reach the internal MSM
        for form in (SCALAR_BYTES, SCALAR_MONT):
            assert ctx.lib.blsgpu_set_scalar_form(ctx.h, form) == 0
            try:
                assert np.array_equal(h.proofs(x), again), "scalar form %d changed the proofs" % form
            finally:
                assert ctx.lib.blsgpu_set_scalar_form(ctx.h, SCALAR_BYTES) == 0
    finally:
        h.close()
        one.close()
        srs.free()


def test_refusals_return_err_arg_and_leave_the_outputs_untouched(ctx):
    import torch
    lib = ctx.lib
    dev = torch.device("cuda", 0)
    err = lambda: lib.blsgpu_last_error().decode()
    sigma, polys = _inputs(4, 2)
    srs = _srs(ctx, sigma)
    g2 = ctx.bases_from_scalars(2, [1, 2, 3, 4])
    off_xy, off_inf = wire_points(1, [_off_subgroup(1)] * 16)
    off = ctx.upload_bases(1, off_xy, off_inf)
    assert off.subgroup_state == 0
    h = ctx.kzg_multiproof_create(srs, 4, 2)
    slot = ctypes.c_void_p()
    try:
        # create
        for args, why in (((None, 4, 2, ctypes.byref(slot)), "NULL"), ((srs.handle, 4, 2, None), "NULL"), ((g2.handle, 2, 1, ctypes.byref(slot)), "G1"),
                          ((srs.handle, 5, 2, ctypes.byref(slot)), "fewer"), ((off.handle, 4, 2, ctypes.byref(slot)), "subgroup"), ((srs.handle, -1, 0, ctypes.byref(slot)), "log_n"),
                          ((srs.handle, 24, 2, ctypes.byref(slot)), "log_n"), ((srs.handle, 4, 5, ctypes.byref(slot)), "log_l"), ((srs.handle, 4, -1, ctypes.byref(slot)), "log_l"),
                          ((srs.handle, 13, 13, ctypes.byref(slot)), "log_l")):
            assert lib.blsgpu_kzg_multiproof_create(ctx.h, *args) == ERR_ARG and why in err(), (args[1:3], err())
            assert not slot.value
        # proofs and cells, host and device forms
        x = _form_input(polys, k.COEFFS, k.NATURAL)
        out = np.full((COUNT, 8, 18), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        cells = np.full((COUNT, 8, 4, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        d_x = torch.from_numpy(x.view(np.int64).reshape(-1).copy()).to(dev)
        d_out = torch.full((COUNT * 8 * 18 + 2,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=dev)
        d_cells = torch.full((COUNT * 32 * 4 + 2,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=dev)
        hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        big = d_x                                                  # a valid pointer for the calls whose count is refused before anything is read
        proofs_calls = [
            (lib.blsgpu_kzg_multiproof_proofs, (None, hp(x), COUNT, 0, 0, hp(out)), "NULL"), (lib.blsgpu_kzg_multiproof_proofs, (h.handle, None, COUNT, 0, 0, hp(out)), "NULL"),
            (lib.blsgpu_kzg_multiproof_proofs, (h.handle, hp(x), COUNT, 0, 0, None), "NULL"), (lib.blsgpu_kzg_multiproof_proofs, (h.handle, hp(x), COUNT, 2, 0, hp(out)), "form"),
            (lib.blsgpu_kzg_multiproof_proofs, (h.handle, hp(x), COUNT, -1, 0, hp(out)), "form"), (lib.blsgpu_kzg_multiproof_proofs, (h.handle, hp(x), COUNT, 0, 2, hp(out)), "order"),
            (lib.blsgpu_kzg_multiproof_proofs, (h.handle, hp(x), (1 << 22) + 1, 0, 0, hp(out)), "2^27"), (lib.blsgpu_kzg_multiproof_proofs, (h.handle, hp(x), 1 << 63, 0, 0, hp(out)), "2^27"),
            (lib.blsgpu_kzg_multiproof_proofs, (h.handle, hp(x), (1 << 64) - 1, 0, 0, hp(out)), "2^27"), (lib.blsgpu_kzg_multiproof_proofs, (h.handle, hp(x), 1, 0, 0, hp(x)), "overlaps"),
            (lib.blsgpu_kzg_multiproof_proofs_device, (h.handle, d_x.data_ptr() + 8, 1, 0, 0, d_out.data_ptr()), "aligned"),
            (lib.blsgpu_kzg_multiproof_proofs_device, (h.handle, d_x.data_ptr(), 1, 0, 0, d_out.data_ptr() + 8), "aligned"),
            (lib.blsgpu_kzg_multiproof_proofs_device, (h.handle, d_x.data_ptr(), COUNT, 0, 0, d_x.data_ptr() + 32), "overlaps"),
            (lib.blsgpu_kzg_multiproof_proofs_device, (h.handle, big.data_ptr(), (1 << 22) + 1, 0, 0, d_out.data_ptr()), "2^27"),
            (lib.blsgpu_kzg_multiproof_proofs_device, (h.handle, None, COUNT, 0, 0, d_out.data_ptr()), "NULL"),
        ]
        cells_calls = [
            (lib.blsgpu_kzg_cells, (None, 4, 2, COUNT, 0, 0, hp(cells)), "NULL"), (lib.blsgpu_kzg_cells, (hp(x), 4, 2, COUNT, 0, 0, None), "NULL"),
            (lib.blsgpu_kzg_cells, (hp(x), 28, 2, 1, 0, 0, hp(cells)), "log_n"), (lib.blsgpu_kzg_cells, (hp(x), -1, 0, 1, 0, 0, hp(cells)), "log_n"),
            (lib.blsgpu_kzg_cells, (hp(x), 4, 5, COUNT, 0, 0, hp(cells)), "log_l"), (lib.blsgpu_kzg_cells, (hp(x), 14, 13, 1, 0, 0, hp(cells)), "log_l"),
            (lib.blsgpu_kzg_cells, (hp(x), 4, 2, COUNT, 2, 0, hp(cells)), "form"), (lib.blsgpu_kzg_cells, (hp(x), 4, 2, COUNT, 0, 2, hp(cells)), "order"),
            (lib.blsgpu_kzg_cells, (hp(x), 4, 2, (1 << 23) + 1, 0, 0, hp(cells)), "2^28"), (lib.blsgpu_kzg_cells, (hp(x), 4, 2, 1 << 63, 0, 0, hp(cells)), "2^28"),
            (lib.blsgpu_kzg_cells, (hp(x), 27, 2, 2, 0, 0, hp(cells)), "2^28"), (lib.blsgpu_kzg_cells, (hp(x), 4, 2, 1, 0, 0, hp(x)), "overlaps"),
            (lib.blsgpu_kzg_cells_device, (d_x.data_ptr() + 8, 4, 2, 1, 0, 0, d_cells.data_ptr()), "aligned"),
            (lib.blsgpu_kzg_cells_device, (d_x.data_ptr(), 4, 2, 1, 0, 0, d_cells.data_ptr() + 8), "aligned"),
            (lib.blsgpu_kzg_cells_device, (d_x.data_ptr(), 4, 2, COUNT, 0, 0, d_x.data_ptr() + 32), "overlaps"),
        ]
        for fn, args, why in proofs_calls + cells_calls:
            assert fn(ctx.h, *args) == ERR_ARG and why in err(), (fn.__name__, args, err())
        ctx.synchronize()
        assert (out == np.uint64(0xA5A5A5A5A5A5A5A5)).all() and (cells == np.uint64(0xA5A5A5A5A5A5A5A5)).all()
        assert (_host(d_out) == np.uint64(0xA5A5A5A5A5A5A5A5)).all() and (_host(d_cells) == np.uint64(0xA5A5A5A5A5A5A5A5)).all()
        assert np.array_equal(_host(d_x).reshape(x.shape), x)
        # ... and the handle still works
        _same(ctx, h.proofs(x), _want(4, 2, k.NATURAL), "after the refusals")
    finally:
        h.close()
        for s in (srs, g2, off):
            s.free()
