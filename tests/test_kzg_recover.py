"""KZG cell recovery on the GPU (`blsgpu_kzg_recover`, `blsgpu_kzg_recover_device`; csrc/kzg_recover.hip.h + csrc/kzg_recover_plan.h),
through the C ABI and the Python mirror.

Every comparison is exact.  The source polynomials are known, so `polys` is compared with them and `out_cells` with `blsgpu_kzg_cells` of
them, limb for limb; where the result is another polynomial (exactly c cells, one changed) it is the reference's
(tests/kzg_recover_ref.py, Python integers).  The chain runs verify -> recover -> proofs -> verify on device pointers alone."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import bls12_381_ref as o
import kzg_ref as k
import kzg_recover_ref as rr
from g_ntt_points import G
from g_sum_points import wire_points

pytestmark = pytest.mark.gpu

ERR_ARG = -2
SCALAR_BYTES, SCALAR_MONT = 0, 1                                  # BLSGPU_SCALAR_*
R = o.R_ORDER
SHAPES = [(3, 0), (3, 3), (4, 2), (6, 1), (8, 2), (12, 6)]
ORDERS = [k.NATURAL, k.BITREV]
FILL = 0xA5A5A5A5A5A5A5A5
PATTERNS = ("exactly-c-random", "c-plus-1", "all", "first-half", "second-half", "every-other", "shuffled")


@pytest.fixture(scope="module")
def ctx():
    import bls12_381_amd as b
    c = b.Context(0)
    yield c
    c.close()


def _limbs(vals):
    return np.array([o.fr_to_mont_limbs(int(x) % R) for x in vals], dtype=np.uint64).reshape(-1, 4)


def _host(t):
    return t.cpu().numpy().view(np.uint64)


class DeviceCall:
    """the arguments of one call in device memory, outputs filled with a pattern and a little longer than the call may write"""

    def __init__(self, col, offsets, cells, log_n, log_l, want_polys=True, want_cells=True, m=None):
        import torch
        dev = torch.device("cuda", 0)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).reshape(-1).copy()).to(dev) if a.size else torch.zeros(4, dtype=torch.int64, device=dev)
        self.log_n, self.log_l, self.count = log_n, log_l, len(offsets) - 1
        self.m = len(col) if m is None else m
        self.host = [np.asarray(col, dtype=np.uint32), np.asarray(offsets, dtype=np.uint32), np.ascontiguousarray(cells, dtype=np.uint64)]
        self.dev = [up(a, dt) for a, dt in zip(self.host, (np.int32, np.int32, np.int64))]
        n = 1 << log_n
        self.polys = torch.full((self.count * n * 4 + 4,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=dev) if want_polys else None
        self.cells = torch.full((self.count * 2 * n * 4 + 4,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=dev) if want_cells else None
        self.ok = torch.full((self.count + 8,), 0xA5, dtype=torch.uint8, device=dev)

    def run(self, ctx, order):
        d = [t.data_ptr() for t in self.dev]
        ctx.kzg_recover_device(d[0], d[1], self.count, self.m, d[2], self.log_n, self.log_l, self.polys.data_ptr() if self.polys is not None else None,
                               self.cells.data_ptr() if self.cells is not None else None, self.ok.data_ptr(), order)

    def results(self):
        n, l = 1 << self.log_n, 1 << self.log_l
        ok = self.ok.cpu().numpy()
        assert (ok[self.count:] == 0xA5).all(), "ok was written past count"
        polys = cells = None
        if self.polys is not None:
            raw = _host(self.polys)
            assert (raw[self.count * n * 4:] == np.uint64(FILL)).all(), "polys was written past count polynomials"
            polys = raw[:self.count * n * 4].reshape(self.count, n, 4)
        if self.cells is not None:
            raw = _host(self.cells)
            assert (raw[self.count * 2 * n * 4:] == np.uint64(FILL)).all(), "out_cells was written past count polynomials"
            cells = raw[:self.count * 2 * n * 4].reshape(self.count, 2 * n // l, l, 4)
        return polys, cells, ok[:self.count]

    def untouched(self):
        return all((_host(t) == np.uint64(FILL)).all() for t in (self.polys, self.cells) if t is not None) and (self.ok.cpu().numpy() == 0xA5).all()

    def inputs_unchanged(self):
        return all(np.array_equal(t.cpu().numpy().view(dt).reshape(-1)[:h.size], h.reshape(-1)) for t, h, dt in zip(self.dev, self.host, (np.uint32, np.uint32, np.uint64)) if h.size)


@functools.lru_cache(maxsize=None)
def _source(log_n, log_l, order):
    """seven polynomials (the special ones among them), one per pattern: (polys ints, patterns)"""
    rng = o.SplitMix64(6100 + 64 * log_n + 4 * log_l + order)
    n, l = 1 << log_n, 1 << log_l
    pats = rr.patterns(rng, log_n, log_l)
    polys = rr.special_polys(rng, n, l) + [k.random_poly(rng, n) for _ in range(len(PATTERNS) - 4)]
    return polys, [pats[name] for name in PATTERNS]


def _call_arrays(full, received):
    """(col, offsets, cells (m, l, 4)) listing cells `received[v]` of full[v] ((2c, l, 4) limbs)"""
    col = [i for rec in received for i in rec]
    offsets = np.cumsum([0] + [len(rec) for rec in received]).tolist()
    cells = np.concatenate([full[v][rec] for v, rec in enumerate(received)]) if col else np.zeros((0,) + full.shape[2:], dtype=np.uint64)
    return col, offsets, np.ascontiguousarray(cells)


# ---- recovery against the definition -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS, ids=["natural", "bitrev"])
@pytest.mark.parametrize("log_n,log_l", SHAPES)
def test_every_pattern_recovers_the_polynomial_and_all_its_cells(ctx, log_n, log_l, order):
    polys, received = _source(log_n, log_l, order)
    count, n = len(polys), 1 << log_n
    x = _limbs([c for p in polys for c in p]).reshape(count, n, 4)
    full = ctx.kzg_cells(x, log_l, k.COEFFS, order)
    col, offsets, cells = _call_arrays(full, received)
    keep = cells.copy()
    for want_polys, want_cells in ((True, False), (False, True), (True, True)):
        what = "polys %s, out_cells %s" % (want_polys, want_cells)
        p, c, ok = ctx.kzg_recover(col, offsets, cells, log_n, log_l, order, want_polys=want_polys, want_cells=want_cells)
        assert ok.tolist() == [1] * count, "host form, " + what
        assert (p is None) == (not want_polys) and (c is None) == (not want_cells)
        assert p is None or np.array_equal(p, x), "host form, %s: the coefficients differ" % what
        assert c is None or np.array_equal(c, full), "host form, %s: the cells differ" % what
        assert np.array_equal(cells, keep), "the host form wrote the caller's cells"
        call = DeviceCall(col, offsets, cells, log_n, log_l, want_polys, want_cells)
        call.run(ctx, order)
        ctx.synchronize()
        p, c, ok = call.results()
        assert ok.tolist() == [1] * count, "device form, " + what
        assert p is None or np.array_equal(p, x), "device form, %s: the coefficients differ" % what
        assert c is None or np.array_equal(c, full), "device form, %s: the cells differ" % what
        assert call.inputs_unchanged(), "the device form wrote the caller's arrays"


def test_one_polynomial_with_no_cell_missing_and_the_smallest_shape(ctx):
    """(0, 0): n = l = c = 1, two cells of one value each; one of them is enough"""
    x = _limbs([5, 0, R - 1]).reshape(3, 1, 4)
    full = ctx.kzg_cells(x, 0, k.COEFFS, k.NATURAL)
    col, offsets, cells = _call_arrays(full, [[1], [0, 1], [0]])
    p, c, ok = ctx.kzg_recover(col, offsets, cells, 0, 0, k.NATURAL, want_cells=True)
    assert ok.tolist() == [1, 1, 1] and np.array_equal(p, x) and np.array_equal(c, full)


# ---- inconsistency -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS, ids=["natural", "bitrev"])
@pytest.mark.parametrize("log_n,log_l", [(4, 2), (6, 1)])
def test_a_changed_entry_is_an_ordinary_outcome(ctx, log_n, log_l, order):
    rng = o.SplitMix64(8800 + 64 * log_n + 4 * log_l + order)
    n, l, c = 1 << log_n, 1 << log_l, 1 << (log_n - log_l)
    pats = rr.patterns(rng, log_n, log_l)
    polys = [k.random_poly(rng, n) for _ in range(4)]
    received = [pats["c-plus-1"], pats["exactly-c-random"], pats["all"], pats["every-other"]]
    col, offsets, cells = rr.call_inputs(polys, received, log_n, log_l, order)
    x = _limbs([a for p in polys for a in p]).reshape(4, n, 4)
    full = ctx.kzg_cells(x, log_l, k.COEFFS, order)
    assert ctx.lib.blsgpu_synchronize(ctx.h) == 0
    for changed, want_ok in ((0, [0, 1, 1, 1]), (2, [1, 1, 0, 1]), (1, [1, 1, 1, 1])):
        wrong = [list(e) for e in cells]
        kk = offsets[changed] + len(received[changed]) // 2
        wrong[kk][l - 1] = (wrong[kk][l - 1] + 1) % R
        lim = _limbs([e for cl in wrong for e in cl]).reshape(len(col), l, 4)
        want_p, want_k = rr.recover(col, offsets, wrong, log_n, log_l, order)
        assert want_k == want_ok, "the reference disagrees with the issue"
        call = DeviceCall(col, offsets, lim, log_n, log_l)
        call.run(ctx, order)
        assert ctx.lib.blsgpu_synchronize(ctx.h) == 0, "inconsistent cells set the sticky flag"
        p, cs, ok = call.results()
        assert ok.tolist() == want_ok, "polynomial %d changed" % changed
        assert np.array_equal(p, _limbs([a for q in want_p for a in q]).reshape(4, n, 4)), "polynomial %d changed: the coefficients are not the reference's" % changed
        for v in range(4):
            if not want_ok[v]:
                assert not p[v].any() and not cs[v].any(), "the rows of a failed polynomial are not zero"
            elif v != changed:
                assert np.array_equal(cs[v], full[v])
        if want_ok[changed]:                                        # exactly c cells: another polynomial, on which every received cell lies
            assert not np.array_equal(p[changed], x[changed])
            assert np.array_equal(cs[changed][received[changed]], lim[offsets[changed]:offsets[changed + 1]])
        hp, hc, hok = ctx.kzg_recover(col, offsets, lim, log_n, log_l, order, want_cells=True)
        assert hok.tolist() == want_ok and np.array_equal(hp, p) and np.array_equal(hc, cs), "the host form differs from the device form"


# ---- malformed input, device form ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS, ids=["natural", "bitrev"])
def test_the_device_form_contains_malformed_polynomials(ctx, order):
    log_n, log_l = 4, 2
    n, l = 1 << log_n, 1 << log_l
    lib = ctx.lib
    polys, cases = rr.malformed_cases(log_n, log_l, order)
    x = _limbs([a for p in polys for a in p]).reshape(len(polys), n, 4)
    full = ctx.kzg_cells(x, log_l, k.COEFFS, order)
    assert lib.blsgpu_synchronize(ctx.h) == 0
    for name, (col, offsets, cells, m, bad) in cases.items():
        lim = _limbs([e for cl in cells for e in cl]).reshape(len(col), l, 4)
        call = DeviceCall(col, offsets, lim, log_n, log_l, m=m)
        call.run(ctx, order)
        assert lib.blsgpu_synchronize(ctx.h) == ERR_ARG and "kzg_recover_device" in lib.blsgpu_last_error().decode(), name
        assert lib.blsgpu_synchronize(ctx.h) == 0, name
        p, cs, ok = call.results()
        count = len(offsets) - 1
        assert ok.tolist() == [0 if v in bad else 1 for v in range(count)], name
        for v in range(count):
            if v in bad:
                assert not p[v].any() and not cs[v].any(), "%s: the rows of polynomial %d are not zero" % (name, v)
            else:
                assert np.array_equal(p[v], x[v]) and np.array_equal(cs[v], full[v]), "%s: neighbour %d is wrong" % (name, v)
        assert call.inputs_unchanged()
        # a following good call on the same context is right
        gcol, goff, gcells = _call_arrays(full, [list(range(4)), list(range(3, 8))])
        good = DeviceCall(gcol, goff, gcells, log_n, log_l)
        good.run(ctx, order)
        assert lib.blsgpu_synchronize(ctx.h) == 0, name
        p, cs, ok = good.results()
        assert ok.tolist() == [1, 1] and np.array_equal(p, x[:2]) and np.array_equal(cs, full[:2]), "the call after '%s' is wrong" % name


# ---- edges ---------------------------------------------------------------------------------------------------------------------------
def test_edges(ctx):
    log_n, log_l, order = 4, 2, k.BITREV
    polys, received = _source(log_n, log_l, order)
    x = _limbs([c for p in polys for c in p]).reshape(len(polys), 16, 4)
    full = ctx.kzg_cells(x, log_l, k.COEFFS, order)
    col, offsets, cells = _call_arrays(full, received)
    # count = 0 is a no-op, through the mirror and with NULL pointers through the ABI
    p, c, ok = ctx.kzg_recover([], [0], [], log_n, log_l, order, want_cells=True)
    assert p.shape == (0, 16, 4) and c.shape == (0, 8, 4, 4) and ok.shape == (0,)
    assert ctx.lib.blsgpu_kzg_recover(ctx.h, None, None, 0, None, log_n, log_l, order, None, None, None) == 0
    assert ctx.lib.blsgpu_kzg_recover_device(ctx.h, None, None, 0, 0, None, log_n, log_l, order, None, None, None) == 0
    # with BITREV the first c cells are the blob in evaluation form
    assert np.array_equal(full[:, :4].reshape(len(polys), 16, 4), _limbs([v for p in polys for v in k.to_evals(p, k.BITREV)]).reshape(len(polys), 16, 4))
    # two calls back to back on one stream without a synchronisation in between; identical from run to run
    first = DeviceCall(col, offsets, cells, log_n, log_l)
    wrong = cells.copy()
    wrong[offsets[2] + 1, 1, 0] ^= np.uint64(4)                     # polynomial 2 has all its cells
    second = DeviceCall(col, offsets, wrong, log_n, log_l)
    first.run(ctx, order)
    second.run(ctx, order)
    ctx.synchronize()
    (p1, c1, ok1), (p2, c2, ok2) = first.results(), second.results()
    assert ok1.tolist() == [1] * 7 and ok2.tolist() == [1, 1, 0, 1, 1, 1, 1]
    assert np.array_equal(p1, x) and np.array_equal(c1, full) and not p2[2].any() and np.array_equal(np.delete(p2, 2, 0), np.delete(x, 2, 0))
    # the context's scalar form does not reach the result
    for form in (SCALAR_BYTES, SCALAR_MONT):
        assert ctx.lib.blsgpu_set_scalar_form(ctx.h, form) == 0
        try:
            p, c, ok = ctx.kzg_recover(col, offsets, cells, log_n, log_l, order, want_cells=True)
            assert ok.tolist() == [1] * 7 and np.array_equal(p, x) and np.array_equal(c, full), "scalar form %d changed the result" % form
        finally:
            assert ctx.lib.blsgpu_set_scalar_form(ctx.h, SCALAR_BYTES) == 0


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_return_err_arg_and_leave_the_outputs_untouched(ctx):
    lib = ctx.lib
    err = lambda: lib.blsgpu_last_error().decode()
    log_n, log_l, order = 4, 2, k.NATURAL
    polys, received = _source(log_n, log_l, order)
    x = _limbs([c for p in polys[:3] for c in p]).reshape(3, 16, 4)
    full = ctx.kzg_cells(x, log_l, k.COEFFS, order)
    col, offsets, cells = _call_arrays(full, [[0, 1, 2, 3], [7, 6, 5, 4, 3], list(range(8))])
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    cl, of = np.array(col, dtype=np.uint32), np.array(offsets, dtype=np.uint32)
    out_p = np.full((3, 16, 4), FILL, dtype=np.uint64)
    out_c = np.full((3, 8, 4, 4), FILL, dtype=np.uint64)
    out_k = np.full(8, 0xA5, dtype=np.uint8)
    names = ("col", "offsets", "count", "cells", "log_n", "log_l", "order", "polys", "out_cells", "ok")
    good = [hp(cl), hp(of), 3, hp(cells), log_n, log_l, order, hp(out_p), hp(out_c), hp(out_k)]

    def host(why, **change):
        args = [change.get(n, a) for n, a in zip(names, good)]
        assert lib.blsgpu_kzg_recover(ctx.h, *args) == ERR_ARG and why in err() and "kzg_recover" in err(), (sorted(change), err())

    for name in ("col", "offsets", "cells", "ok"):
        host("NULL", **{name: None})
    host("both outputs", polys=None, out_cells=None)
    host("order", order=2)
    host("order", order=-1)
    host("log_n", log_n=-1)
    host("log_n", log_n=28)
    host("log_l", log_l=5)
    host("log_l", log_l=-1)
    host("4096", log_n=13, log_l=1)
    host("2^28", count=(1 << 28) + 1)
    host("2^28", count=(1 << 64) - 1)
    host("overlap", polys=hp(cells))
    host("overlap", out_cells=hp(cells))
    host("overlap", ok=hp(cl))
    host("overlap", out_cells=hp(out_p))
    host("overlap", ok=ctypes.c_void_p(out_c.ctypes.data + 40))
    host("offsets[0]", offsets=hp(np.array([1, 4, 9, 17], dtype=np.uint32)))
    host("non-decreasing", offsets=hp(np.array([0, 9, 4, 17], dtype=np.uint32)))
    host("2c", col=hp(np.array([0, 1, 2, 8] + col[4:], dtype=np.uint32)))
    host("twice", col=hp(np.array([0, 1, 2, 0] + col[4:], dtype=np.uint32)))
    host("fewer than c", offsets=hp(np.array([0, 3, 9, 17], dtype=np.uint32)))
    call = DeviceCall(col, offsets, cells, log_n, log_l)
    d = [t.data_ptr() for t in call.dev]
    dnames = ("col", "offsets", "count", "m", "cells", "log_n", "log_l", "order", "polys", "out_cells", "ok")
    dgood = [d[0], d[1], 3, len(col), d[2], log_n, log_l, order, call.polys.data_ptr(), call.cells.data_ptr(), call.ok.data_ptr()]

    def device(why, **change):
        args = [change.get(n, a) for n, a in zip(dnames, dgood)]
        assert lib.blsgpu_kzg_recover_device(ctx.h, *args) == ERR_ARG and why in err() and "kzg_recover" in err(), (sorted(change), err())

    for name in ("col", "offsets", "cells", "ok"):
        device("NULL", **{name: None})
    device("both outputs", polys=None, out_cells=None)
    device("order", order=7)
    device("2^24", m=(1 << 24) + 1)
    device("2^24", m=1 << 63)
    device("m * l", m=1 << 24, log_n=13, log_l=12)
    device("2^28", count=1 << 24)
    device("no polynomial", count=0)
    device("16-byte", cells=d[2] + 8)
    device("16-byte", polys=call.polys.data_ptr() + 8)
    device("16-byte", out_cells=call.cells.data_ptr() + 8)
    device("4-byte", col=d[0] + 2)
    device("4-byte", offsets=d[1] + 1)
    device("overlap", polys=d[2])
    device("overlap", out_cells=d[2] + 32)
    device("overlap", ok=d[0] + 3)
    device("overlap", out_cells=call.polys.data_ptr() + 64)
    device("overlap", ok=call.polys.data_ptr() + 5)
    ctx.synchronize()
    assert (out_p == np.uint64(FILL)).all() and (out_c == np.uint64(FILL)).all() and (out_k == 0xA5).all()
    assert call.untouched() and call.inputs_unchanged()
    # ... and the call still works
    p, c, ok = ctx.kzg_recover(col, offsets, cells, log_n, log_l, order, want_cells=True)
    assert ok.tolist() == [1, 1, 1] and np.array_equal(p, x) and np.array_equal(c, full)


# ---- the chain -----------------------------------------------------------------------------------------------------------------------
def _g1(scalars):
    return wire_points(1, [o.g1_to_affine(o.g1_mul(o.g1_from_affine(o.G1_GEN), int(s) % R)) for s in scalars])


@pytest.mark.parametrize("log_n,log_l", [(6, 2), (12, 6)])
def test_cells_recover_proofs_verify_on_device_pointers_alone(ctx, log_n, log_l):
    """kzg_cells -> drop a random half -> kzg_recover_device -> kzg_multiproof_proofs_device on the recovered coefficients -> batch_normalize
    -> kzg_verify_cells over all 2c recovered cells with those proofs: no host copy of any scalar or point in between"""
    import torch
    dev = torch.device("cuda", 0)
    order = k.BITREV
    rng = o.SplitMix64(2300 + log_n)
    n, l, c2, count = 1 << log_n, 1 << log_l, 2 << (log_n - log_l), 2
    tau = rng.scalar()
    polys = [k.random_poly(rng, n) for _ in range(count)]
    sigma, t = [], 1
    for _ in range(n):
        sigma.append(t)
        t = t * tau % R
    commit = _g1([k.evaluate(p, tau) for p in polys])
    q = wire_points(2, [G[2].to_affine(G[2].base_mul(pow(tau, l, R)))])[0][0]
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).reshape(-1).copy()).to(dev)
    d_polys = up(_limbs([a for p in polys for a in p]), np.int64)
    d_cells = torch.zeros(count * 2 * n * 4, dtype=torch.int64, device=dev)
    received = []
    for _ in range(count):
        perm = list(range(c2))
        for i in range(c2 - 1, 0, -1):
            j = rng.next() % (i + 1)
            perm[i], perm[j] = perm[j], perm[i]
        received.append(perm[:c2 // 2])
    col = [i for rec in received for i in rec]
    offsets = [0, c2 // 2, c2]
    pick = up(np.array([v * c2 + i for v, rec in enumerate(received) for i in rec], dtype=np.int64), np.int64)
    srs = ctx.bases_from_scalars(1, sigma)
    try:
        mp = ctx.kzg_multiproof_create(srs, log_n, log_l)
        ver = ctx.kzg_cell_verifier_create(srs, log_n, log_l, q)
    finally:
        srs.free()
    try:
        ctx.kzg_cells_device(d_polys.data_ptr(), log_n, log_l, count, d_cells.data_ptr(), k.COEFFS, order)
        ctx.synchronize()                                           # torch gathers on its own stream
        d_half = d_cells.view(count * c2, l * 4).index_select(0, pick).contiguous().view(-1)
        torch.cuda.synchronize()
        d_col, d_off = up(np.array(col, dtype=np.uint32), np.int32), up(np.array(offsets, dtype=np.uint32), np.int32)
        d_rec = torch.zeros(count * n * 4, dtype=torch.int64, device=dev)
        d_all = torch.zeros(count * 2 * n * 4, dtype=torch.int64, device=dev)
        d_ok = torch.zeros(count, dtype=torch.uint8, device=dev)
        d_proofs = torch.zeros(count * c2 * 18, dtype=torch.int64, device=dev)
        d_pxy = torch.zeros(count * c2 * 12, dtype=torch.int64, device=dev)
        d_pinf = torch.zeros(count * c2, dtype=torch.uint8, device=dev)
        ctx.kzg_recover_device(d_col.data_ptr(), d_off.data_ptr(), count, len(col), d_half.data_ptr(), log_n, log_l, d_rec.data_ptr(), d_all.data_ptr(), d_ok.data_ptr(), order)
        mp.proofs_device(d_rec.data_ptr(), count, d_proofs.data_ptr(), k.COEFFS, order)
        ctx.batch_normalize_device(1, d_proofs.data_ptr(), count * c2, d_pxy.data_ptr(), d_pinf.data_ptr())
        d_cxy, d_cinf = up(commit[0], np.int64), up(commit[1], np.uint8)
        d_row = up(np.array([v for v in range(count) for _ in range(c2)], dtype=np.uint32), np.int32)
        d_vcol = up(np.array([i for _ in range(count) for i in range(c2)], dtype=np.uint32), np.int32)
        d_voff = up(np.array([0, c2, 2 * c2], dtype=np.uint32), np.int32)
        d_r = up(_limbs([rng.scalar(), rng.scalar()]), np.int64)
        d_verdict = torch.full((2,), 0xA5, dtype=torch.uint8, device=dev)
        verify = lambda: ver.verify_device(d_cxy.data_ptr(), d_cinf.data_ptr(), count, d_row.data_ptr(), d_vcol.data_ptr(), d_all.data_ptr(), d_pxy.data_ptr(), d_pinf.data_ptr(),
                                           d_voff.data_ptr(), 2, count * c2, d_r.data_ptr(), d_verdict.data_ptr(), None, order)
        verify()
        ctx.synchronize()
        assert d_ok.cpu().tolist() == [1, 1]
        assert d_verdict.cpu().tolist() == [1, 1], "the recovered cells do not verify against the proofs of the recovered coefficients"
        assert torch.equal(d_all, d_cells) and torch.equal(d_rec, d_polys)
        d_all[(c2 + 3) * l * 4 + 2] ^= 1                           # one entry of cell 3 of the second polynomial
        torch.cuda.synchronize()
        verify()
        ctx.synchronize()
        assert d_verdict.cpu().tolist() == [1, 0]
    finally:
        mp.close()
        ver.close()
