"""Batched KZG cell-proof verification on the GPU (`blsgpu_kzg_cell_verifier_*`, `blsgpu_kzg_verify_cells*`; csrc/kzg_verify.hip.h +
csrc/kzg_verify_plan.h), through the C ABI and the Python mirror.

Every comparison is exact.  The round trips take cells and proofs from the library's own producer (`kzg_cells`, `kzg_multiproof_proofs`)
over a powers-of-tau SRS.  The exactness cases run the DEFINITION in the group-as-scalars model (tests/kzg_verify_ref.py) and compare
`out_ab` after `batch_normalize` with [A_s] G1, [B_s] G1 from the oracle's `g1_mul` -- for honest inputs and for inputs that are
consistent over an ARBITRARY SRS (independent sigma_u with a zero among them, random T and proofs, the commitment solved from the
equation), where index slips that a geometric SRS hides show up.  Verdicts are the reference's."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import bls12_381_ref as o
import kzg_ref as k
import kzg_verify_ref as v
from g_ntt_points import G
from g_sum_points import _off_subgroup, wire_points

pytestmark = pytest.mark.gpu

ERR_ARG = -2
SCALAR_BYTES, SCALAR_MONT = 0, 1                                  # BLSGPU_SCALAR_*
R = o.R_ORDER
SHAPES = [(0, 0), (3, 0), (3, 3), (4, 2), (6, 1), (8, 6)]
ORDERS = [k.NATURAL, k.BITREV]
CUTS = {"one-batch": [0, 5], "one-cell-each": [0, 1, 2, 3, 4, 5], "empty-between": [0, 0, 3, 3, 5]}
FILL = 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def ctx():
    import bls12_381_amd as b
    c = b.Context(0)
    yield c
    c.close()


def _limbs(vals):
    return np.array([o.fr_to_mont_limbs(int(x) % R) for x in vals], dtype=np.uint64).reshape(-1, 4)


def _g1(scalars):
    """[s] G1 as affine wire points with their infinity bytes"""
    return wire_points(1, [o.g1_to_affine(o.g1_mul(o.g1_from_affine(o.G1_GEN), int(s) % R)) for s in scalars])


def _g2(scalar):
    return wire_points(2, [G[2].to_affine(G[2].base_mul(int(scalar) % R))])[0][0]


def _verifier(ctx, sigma, T, log_n, log_l):
    """the handle over S[u] = [sigma_u] G1 and q = [T] G2; the SRS is freed at once: the handle keeps no reference to it"""
    srs = ctx.bases_from_scalars(1, [int(s) for s in sigma])
    try:
        return ctx.kzg_cell_verifier_create(srs, log_n, log_l, _g2(T))
    finally:
        srs.free()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


class DeviceCall:
    """the arguments of one call in device memory, outputs filled with a pattern"""

    def __init__(self, commit, row, col, cells, proof, offsets, r, want_ab=True):
        import torch
        dev = torch.device("cuda", 0)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).reshape(-1).copy()).to(dev)
        self.nseg, self.m, self.ncommit = len(offsets) - 1, int(offsets[-1]), commit[0].shape[0]
        self.host = [np.ascontiguousarray(a).copy() for a in (commit[0], commit[1], np.asarray(row, dtype=np.uint32), np.asarray(col, dtype=np.uint32), cells, proof[0], proof[1],
                                                              np.asarray(offsets, dtype=np.uint32), r)]
        kinds = (np.int64, np.uint8, np.int32, np.int32, np.int64, np.int64, np.uint8, np.int32, np.int64)
        self.dev = [up(a, dt) if a.size else torch.zeros(2, dtype=torch.int64, device=dev) for a, dt in zip(self.host, kinds)]
        self.verdict = torch.full((self.nseg + 8,), 0xA5, dtype=torch.uint8, device=dev)
        self.ab = torch.full((self.nseg * 36 + 2,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=dev) if want_ab else None

    def run(self, handle, order):
        d = [t.data_ptr() for t in self.dev]
        handle.verify_device(d[0], d[1], self.ncommit, d[2], d[3], d[4], d[5], d[6], d[7], self.nseg, self.m, d[8], self.verdict.data_ptr(),
                             self.ab.data_ptr() if self.ab is not None else None, order)

    def results(self):
        vd = self.verdict.cpu().numpy()
        assert (vd[self.nseg:] == 0xA5).all(), "the verdicts were written past nseg"
        ab = None
        if self.ab is not None:
            raw = _host(self.ab)
            assert (raw[self.nseg * 36:] == np.uint64(FILL)).all(), "out_ab was written past nseg pairs"
            ab = raw[:self.nseg * 36].reshape(self.nseg, 2, 18)
        return vd[:self.nseg], ab

    def inputs_unchanged(self):
        kinds = (np.uint64, np.uint8, np.uint32, np.uint32, np.uint64, np.uint64, np.uint8, np.uint32, np.uint64)
        return all(np.array_equal(t.cpu().numpy().view(dt).reshape(-1), h.reshape(-1)) for t, h, dt in zip(self.dev, self.host, kinds) if h.size)


# ---- round trips over the library's own producer -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tau_inputs(log_n):
    rng = o.SplitMix64(5000 + log_n)
    n = 1 << log_n
    tau = rng.scalar()
    return tau, [pow(tau, u, R) for u in range(n)], [k.random_poly(rng, n) for _ in range(2)]


def _produce(ctx, log_n, log_l, order):
    """(handle, commitments, cells (2, 2c, l, 4), proofs xy (2, 2c, 12), proofs inf (2, 2c)) from kzg_cells / kzg_multiproof_proofs"""
    tau, sigma, polys = _tau_inputs(log_n)
    x = _limbs([c for p in polys for c in p]).reshape(2, 1 << log_n, 4)
    srs = ctx.bases_from_scalars(1, sigma)
    try:
        mp = ctx.kzg_multiproof_create(srs, log_n, log_l)
        try:
            pxy, pinf = ctx.batch_normalize(1, mp.proofs(x, k.COEFFS, order).reshape(-1, 18))
        finally:
            mp.close()
        handle = ctx.kzg_cell_verifier_create(srs, log_n, log_l, _g2(pow(tau, 1 << log_l, R)))
    finally:
        srs.free()
    cells = ctx.kzg_cells(x, log_l, k.COEFFS, order)
    c2 = 2 << (log_n - log_l)
    return handle, _g1([k.evaluate(p, tau) for p in polys]), cells, pxy.reshape(2, c2, 12), pinf.reshape(2, c2)


@pytest.mark.parametrize("order", ORDERS, ids=["natural", "bitrev"])
@pytest.mark.parametrize("log_n,log_l", SHAPES)
def test_cells_and_proofs_of_the_producer_verify(ctx, log_n, log_l, order):
    handle, commit, cells, pxy, pinf = _produce(ctx, log_n, log_l, order)
    try:
        c2 = handle.cells
        assert (handle.log_n, handle.log_l, c2) == (log_n, log_l, 2 << (log_n - log_l))
        row, col = [0, 1, 1, 0, 1], [0, c2 - 1, 1 % c2, c2 // 2, 0]
        cs, px, pi = cells[row, col], pxy[row, col], pinf[row, col]
        rng = o.SplitMix64(77 + log_n)
        for name, off in CUTS.items():
            r = _limbs([rng.scalar() for _ in off[1:]])
            keep = [a.copy() for a in (cs, px, pi, r)]
            assert handle.verify(commit[0], commit[1], row, col, cs, px, pi, off, r, order).tolist() == [1] * (len(off) - 1), "host form, " + name
            assert all(np.array_equal(a, b) for a, b in zip((cs, px, pi, r), keep))
            call = DeviceCall(commit, row, col, cs, (px, pi), off, r)
            call.run(handle, order)
            ctx.synchronize()
            assert call.results()[0].tolist() == [1] * (len(off) - 1), "device form, " + name
            assert call.inputs_unchanged(), "the device form wrote the caller's arrays"
        wrong = cs.copy()
        wrong[2, 0, 0] ^= np.uint64(1)
        assert handle.verify(commit[0], commit[1], row, col, wrong, px, pi, [0, 2, 5], _limbs([3, 5]), order).tolist() == [1, 0]
    finally:
        handle.close()


def test_the_data_availability_shape_as_one_batch_and_as_one_batch_per_cell(ctx):
    """(12, 6), 2 blobs x 128 cells in the bit-reversed numbering of blob formats"""
    handle, commit, cells, pxy, pinf = _produce(ctx, 12, 6, k.BITREV)
    try:
        row = [i for i in range(2) for _ in range(128)]
        col = [j for _ in range(2) for j in range(128)]
        cs, px, pi = cells.reshape(256, 64, 4), pxy.reshape(256, 12), pinf.reshape(256)
        rng = o.SplitMix64(7594)
        assert handle.verify(commit[0], commit[1], row, col, cs, px, pi, [0, 256], _limbs([rng.scalar()]), k.BITREV).tolist() == [1]
        assert handle.verify(commit[0], commit[1], row, col, cs, px, pi, list(range(257)), _limbs([rng.scalar() for _ in range(256)]), k.BITREV).tolist() == [1] * 256
        wrong = cs.copy()
        wrong[200, 63, 1] ^= np.uint64(1 << 40)
        assert handle.verify(commit[0], commit[1], row, col, wrong, px, pi, [0, 256], _limbs([rng.scalar()]), k.BITREV).tolist() == [0]
        got = handle.verify(commit[0], commit[1], row, col, wrong, px, pi, list(range(257)), _limbs([rng.scalar() for _ in range(256)]), k.BITREV)
        assert got.tolist() == [0 if i == 200 else 1 for i in range(256)], "batches of one cell give the per-cell verdict"
    finally:
        handle.close()


# ---- exactness against the definition ------------------------------------------------------------------------------------------------
def _same_points(ctx, ab, want_scalars, what):
    xy, inf = ctx.batch_normalize(1, np.ascontiguousarray(ab).reshape(-1, 18))
    wxy, winf = _g1(want_scalars)
    assert np.array_equal(inf != 0, winf != 0), "%s: identities at %s, wanted at %s" % (what, np.nonzero(inf)[0], np.nonzero(winf)[0])
    bad = np.nonzero((xy != wxy).any(axis=1) & (winf == 0))[0]
    assert bad.size == 0, "%s: points %s differ" % (what, bad)


def _model_inputs(kind, log_n, log_l, order):
    """scalar-model inputs of 5 cells in the cut [0, 3, 3, 5] (+ the challenges): honest over powers of tau, or consistent over an arbitrary
    SRS with sigma_1 = 0 (sigma_0 for l = 1), an identity proof and -- r_2 = -1 makes the third batch's weights sum to 0 -- an identity commitment"""
    rng = o.SplitMix64(3000 + 64 * log_n + 4 * log_l + order + (17 if kind == "honest" else 0))
    c2 = 2 << (log_n - log_l)
    col = [0, c2 - 1, 1 % c2, c2 // 2, 0]
    offsets = [0, 3, 3, 5]
    r = [rng.scalar(), rng.scalar(), R - 1]
    if kind == "honest":
        row = [0, 1, 1, 0, 1]
        commits, cells, proofs, sigma, T = v.honest(rng, log_n, log_l, order, 2, row, col)
    else:
        commits, row, cells, proofs, sigma, T = v.consistent(rng, log_n, log_l, order, col, offsets, r, zero_sigma=1, zero_proof=1)
    return commits, row, col, cells, proofs, offsets, r, sigma, T


@pytest.mark.parametrize("kind", ["honest", "consistent"])
@pytest.mark.parametrize("order", ORDERS, ids=["natural", "bitrev"])
@pytest.mark.parametrize("log_n,log_l", SHAPES)
def test_out_ab_and_the_verdicts_are_the_definition(ctx, log_n, log_l, order, kind):
    commits, row, col, cells, proofs, offsets, r, sigma, T = _model_inputs(kind, log_n, log_l, order)
    want = v.batch(commits, row, col, cells, proofs, offsets, r, sigma, T, log_n, log_l, order)
    if kind == "consistent":
        assert 0 in sigma and 0 in proofs and commits[2] == 0 and [w[2] for w in want[:2]] == [1, 1]
    else:
        assert [w[2] for w in want] == [1, 1, 1]
    handle = _verifier(ctx, sigma, T, log_n, log_l)
    try:
        commit, proof = _g1(commits), _g1(proofs)
        cs = _limbs([e for c in cells for e in c]).reshape(5, 1 << log_l, 4)
        verdict, ab = handle.verify(commit[0], commit[1], row, col, cs, proof[0], proof[1], offsets, _limbs(r), order, return_ab=True)
        _same_points(ctx, ab, [s for w in want for s in w[:2]], "host form")
        assert verdict.tolist() == [w[2] for w in want]
        call = DeviceCall(commit, row, col, cs, proof, offsets, _limbs(r))
        call.run(handle, order)
        ctx.synchronize()
        dv, dab = call.results()
        _same_points(ctx, dab, [s for w in want for s in w[:2]], "device form")
        assert dv.tolist() == [w[2] for w in want]
        # a changed cell over the arbitrary SRS: the verdict and the pair are still the definition's
        cells2 = [list(c) for c in cells]
        cells2[4][(1 << log_l) - 1] = (cells2[4][-1] + 5) % R
        want2 = v.batch(commits, row, col, cells2, proofs, offsets, r, sigma, T, log_n, log_l, order)
        cs2 = _limbs([e for c in cells2 for e in c]).reshape(cs.shape)
        verdict, ab = handle.verify(commit[0], commit[1], row, col, cs2, proof[0], proof[1], offsets, _limbs(r), order, return_ab=True)
        _same_points(ctx, ab, [s for w in want2 for s in w[:2]], "a changed cell")
        assert verdict.tolist() == [w[2] for w in want2] and (sigma[-1] == 0 or verdict[2] == 0)
    finally:
        handle.close()


# ---- every field is checked ----------------------------------------------------------------------------------------------------------
def test_every_field_of_a_batch_of_five_is_checked(ctx):
    log_n, log_l, order = 4, 2, k.BITREV
    rng = o.SplitMix64(424242)
    row, col = [0, 1, 2, 1, 2, 1, 3, 3, 3], [1, 0, 7, 3, 3, 5, 2, 6, 0]
    offsets = [0, 1, 6, 9]                                         # the batch of five in the middle, on rows 1 and 2
    commits, cells, proofs, sigma, T = v.honest(rng, log_n, log_l, order, 4, row, col)
    r = _limbs([rng.scalar() for _ in range(3)])
    commit, proof = _g1(commits), _g1(proofs)
    cs = _limbs([e for c in cells for e in c]).reshape(9, 4, 4)
    other = _g1([rng.scalar()])
    handle = _verifier(ctx, sigma, T, log_n, log_l)
    try:
        run = lambda cm=commit, rw=row, cl=col, c=cs, pf=proof: handle.verify(cm[0], cm[1], rw, cl, c, pf[0], pf[1], offsets, r, order).tolist()
        assert run() == [1, 1, 1]
        for kk in range(1, 6):
            for entry in (0, 3):
                c = cs.copy()
                c[kk, entry, 0] ^= np.uint64(1)
                assert run(c=c) == [1, 0, 1], "entry %d of cell %d" % (entry, kk)
            pf = (proof[0].copy(), proof[1].copy())
            pf[0][kk] = other[0][0]
            assert run(pf=pf) == [1, 0, 1], "proof %d" % kk
            pf = (proof[0].copy(), proof[1].copy())
            pf[1][kk] = 1
            assert run(pf=pf) == [1, 0, 1], "proof %d replaced by the identity" % kk
            rw = list(row)
            rw[kk] = 3 - row[kk]
            assert run(rw=rw) == [1, 0, 1], "row of cell %d" % kk
            cl = list(col)
            cl[kk] = (col[kk] + 1) % 8
            assert run(cl=cl) == [1, 0, 1], "col of cell %d" % kk
        for rw_ in (1, 2):
            cm = (commit[0].copy(), commit[1].copy())
            cm[0][rw_] = other[0][0]
            assert run(cm=cm) == [1, 0, 1], "commitment %d" % rw_
    finally:
        handle.close()
    wrong_q = _verifier(ctx, sigma, (T + 1) % R, log_n, log_l)
    try:
        assert wrong_q.verify(commit[0], commit[1], row, col, cs, proof[0], proof[1], offsets, r, order).tolist() == [0, 0, 0], "q"
    finally:
        wrong_q.close()


def test_the_challenge_is_used(ctx):
    """two cells of one column on two rows get +d / -d on the same entry: the sum of the two interpolation polynomials is unchanged, so the
    batch passes under r = 1 and fails under a random r; r = 0 checks the first cell only.  Every verdict is the reference's."""
    log_n, log_l, order = 4, 2, k.NATURAL
    rng = o.SplitMix64(1717)
    row, col = [0, 1], [5, 5]
    commits, cells, proofs, sigma, T = v.honest(rng, log_n, log_l, order, 2, row, col)
    d = rng.scalar()
    both = [list(cells[0]), list(cells[1])]
    both[0][2] = (both[0][2] + d) % R
    both[1][2] = (both[1][2] - d) % R
    second = [list(cells[0]), both[1]]
    commit, proof = _g1(commits), _g1(proofs)
    handle = _verifier(ctx, sigma, T, log_n, log_l)
    try:
        for what, cl, r, want in (("r = 1", both, 1, 1), ("a random r", both, rng.scalar(), 0), ("r = 0, the first cell is wrong", both, 0, 0),
                                  ("r = 0, only the second cell is wrong", second, 0, 1), ("r = 1, only the second cell is wrong", second, 1, 0)):
            assert v.batch(commits, row, col, cl, proofs, [0, 2], [r], sigma, T, log_n, log_l, order)[0][2] == want, what + " (reference)"
            cs = _limbs([e for c in cl for e in c]).reshape(2, 4, 4)
            assert handle.verify(commit[0], commit[1], row, col, cs, proof[0], proof[1], [0, 2], _limbs([r]), order).tolist() == [want], what
    finally:
        handle.close()


# ---- edges ---------------------------------------------------------------------------------------------------------------------------
def test_edges(ctx):
    log_n, log_l, order = 4, 2, k.BITREV
    commits, row, col, cells, proofs, offsets, r, sigma, T = _model_inputs("honest", log_n, log_l, order)
    commit, proof = _g1(commits), _g1(proofs)
    cs = _limbs([e for c in cells for e in c]).reshape(5, 4, 4)
    handle = _verifier(ctx, sigma, T, log_n, log_l)
    try:
        # nseg = 0 is a no-op, through the mirror and with NULL pointers through the ABI
        assert handle.verify(None, None, [], [], [], None, None, [0], [], order).shape == (0,)
        assert ctx.lib.blsgpu_kzg_verify_cells(ctx.h, handle.handle, None, None, 0, None, None, None, None, None, None, 0, None, 0, None, None) == 0
        assert ctx.lib.blsgpu_kzg_verify_cells_device(ctx.h, handle.handle, None, None, 0, None, None, None, None, None, None, 0, 0, None, 0, None, None) == 0
        # batches without cells hold
        assert handle.verify(commit[0], commit[1], [], [], [], None, None, [0, 0, 0], _limbs([5, 0]), order).tolist() == [1, 1]
        # two calls back to back on one handle and one stream, without a synchronisation in between; identical from run to run
        first = DeviceCall(commit, row, col, cs, proof, offsets, _limbs(r))
        wrong = cs.copy()
        wrong[0, 1, 2] ^= np.uint64(4)
        second = DeviceCall(commit, row, col, wrong, proof, offsets, _limbs(r))
        first.run(handle, order)
        second.run(handle, order)
        ctx.synchronize()
        (v1, ab1), (v2, _) = first.results(), second.results()
        assert v1.tolist() == [1, 1, 1] and v2.tolist() == [0, 1, 1]
        verdict, ab = handle.verify(commit[0], commit[1], row, col, cs, proof[0], proof[1], offsets, _limbs(r), order, return_ab=True)
        again = handle.verify(commit[0], commit[1], row, col, cs, proof[0], proof[1], offsets, _limbs(r), order, return_ab=True)
        assert np.array_equal(ab, again[1]) and np.array_equal(ab, ab1) and verdict.tolist() == again[0].tolist() == [1, 1, 1], "results differ from run to run"
        # the context's scalar form does not reach the result
        for form in (SCALAR_BYTES, SCALAR_MONT):
            assert ctx.lib.blsgpu_set_scalar_form(ctx.h, form) == 0
            try:
                got = handle.verify(commit[0], commit[1], row, col, cs, proof[0], proof[1], offsets, _limbs(r), order, return_ab=True)
                assert np.array_equal(got[1], ab) and got[0].tolist() == [1, 1, 1], "scalar form %d changed the result" % form
            finally:
                assert ctx.lib.blsgpu_set_scalar_form(ctx.h, SCALAR_BYTES) == 0
    finally:
        handle.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_return_err_arg_and_leave_the_outputs_untouched(ctx):
    lib = ctx.lib
    err = lambda: lib.blsgpu_last_error().decode()
    log_n, log_l, order = 4, 2, k.NATURAL
    commits, row, col, cells, proofs, offsets, r, sigma, T = _model_inputs("honest", log_n, log_l, order)
    commit, proof = _g1(commits), _g1(proofs)
    cs = _limbs([e for c in cells for e in c]).reshape(5, 4, 4)
    q = _g2(T)
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    srs = ctx.bases_from_scalars(1, sigma)
    g2 = ctx.bases_from_scalars(2, [1, 2, 3, 4])
    off_xy, off_inf = wire_points(1, [_off_subgroup(1)] * 4)
    off = ctx.upload_bases(1, off_xy, off_inf)
    assert off.subgroup_state == 0
    slot = ctypes.c_void_p()
    handle = ctx.kzg_cell_verifier_create(srs, log_n, log_l, q)
    try:
        for args, why in (((None, 4, 2, hp(q), None, ctypes.byref(slot)), "NULL"), ((srs.handle, 4, 2, None, None, ctypes.byref(slot)), "NULL"), ((srs.handle, 4, 2, hp(q), None, None), "NULL"),
                          ((g2.handle, 4, 2, hp(q), None, ctypes.byref(slot)), "G1"), ((srs.handle, 4, 3, hp(q), None, ctypes.byref(slot)), "fewer"),
                          ((off.handle, 4, 2, hp(q), None, ctypes.byref(slot)), "subgroup"), ((srs.handle, -1, 0, hp(q), None, ctypes.byref(slot)), "log_n"),
                          ((srs.handle, 24, 2, hp(q), None, ctypes.byref(slot)), "log_n"), ((srs.handle, 4, 5, hp(q), None, ctypes.byref(slot)), "log_l"),
                          ((srs.handle, 4, -1, hp(q), None, ctypes.byref(slot)), "log_l"), ((srs.handle, 13, 13, hp(q), None, ctypes.byref(slot)), "log_l")):
            assert lib.blsgpu_kzg_cell_verifier_create(ctx.h, *args) == ERR_ARG and why in err(), (args[1:3], err())
            assert not slot.value
        rw, cl, of = np.array(row, dtype=np.uint32), np.array(col, dtype=np.uint32), np.array(offsets, dtype=np.uint32)
        rr = _limbs(r)
        verdict = np.full(8, 0xA5, dtype=np.uint8)
        ab = np.full((3, 2, 18), FILL, dtype=np.uint64)
        good = [handle.handle, hp(commit[0]), hp(commit[1]), 2, hp(rw), hp(cl), hp(cs), hp(proof[0]), hp(proof[1]), hp(of), 3, hp(rr), order, hp(verdict), hp(ab)]

        def host(why, **change):
            names = ("h", "commit_xy", "commit_inf", "ncommit", "row", "col", "cells", "proof_xy", "proof_inf", "offsets", "nseg", "r", "order", "verdict", "out_ab")
            args = [change.get(n, a) for n, a in zip(names, good)]
            assert lib.blsgpu_kzg_verify_cells(ctx.h, *args) == ERR_ARG and why in err(), (sorted(change), err())

        for name in ("h", "commit_xy", "commit_inf", "row", "col", "cells", "proof_xy", "proof_inf", "offsets", "r", "verdict"):
            host("NULL", **{name: None})
        host("order", order=2)
        host("order", order=-1)
        host("2^24", nseg=(1 << 24) + 1)
        host("2^24", nseg=(1 << 64) - 1)
        host("2^32", ncommit=1 << 32)
        host("overlap", verdict=hp(cs))
        host("overlap", out_ab=hp(proof[0]))
        host("overlap", out_ab=hp(verdict))
        host("offsets[0]", offsets=hp(np.array([1, 3, 3, 5], dtype=np.uint32)))
        host("non-decreasing", offsets=hp(np.array([0, 4, 3, 5], dtype=np.uint32)))
        host("row index", ncommit=1)
        host("row index", row=hp(np.array([0, 1, 2, 0, 1], dtype=np.uint32)))
        host("2c", col=hp(np.array([0, 7, 8, 4, 0], dtype=np.uint32)))
        call = DeviceCall(commit, row, col, cs, proof, offsets, rr)
        d = [t.data_ptr() for t in call.dev]
        dgood = [handle.handle, d[0], d[1], 2, d[2], d[3], d[4], d[5], d[6], d[7], 3, 5, d[8], order, call.verdict.data_ptr(), call.ab.data_ptr()]

        def device(why, **change):
            names = ("h", "commit_xy", "commit_inf", "ncommit", "row", "col", "cells", "proof_xy", "proof_inf", "offsets", "nseg", "m", "r", "order", "verdict", "out_ab")
            args = [change.get(n, a) for n, a in zip(names, dgood)]
            assert lib.blsgpu_kzg_verify_cells_device(ctx.h, *args) == ERR_ARG and why in err(), (sorted(change), err())

        for name in ("h", "commit_xy", "commit_inf", "row", "col", "cells", "proof_xy", "proof_inf", "offsets", "r", "verdict"):
            device("NULL", **{name: None})
        device("order", order=7)
        device("2^24", m=(1 << 24) + 1)
        device("2^24", m=1 << 63)
        device("2^24", nseg=(1 << 24) + 1)
        device("no batch", nseg=0)
        device("16-byte", cells=d[4] + 8)
        device("16-byte", r=d[8] + 8)
        device("8-byte", proof_xy=d[5] + 4)
        device("8-byte", commit_xy=d[0] + 4)
        device("8-byte", out_ab=call.ab.data_ptr() + 4)
        device("4-byte", row=d[2] + 2)
        device("4-byte", col=d[3] + 1)
        device("4-byte", offsets=d[7] + 2)
        device("overlap", verdict=d[4] + 3)
        device("overlap", out_ab=d[5])
        device("overlap", out_ab=call.verdict.data_ptr() - 8)
        ctx.synchronize()
        assert (verdict == 0xA5).all() and (ab == np.uint64(FILL)).all()
        assert (call.verdict.cpu().numpy() == 0xA5).all() and (_host(call.ab) == np.uint64(FILL)).all() and call.inputs_unchanged()
        # ... and the handle still works
        assert handle.verify(commit[0], commit[1], row, col, cs, proof[0], proof[1], offsets, rr, order).tolist() == [1, 1, 1]
    finally:
        handle.close()
        for s in (srs, g2, off):
            s.free()


def test_the_device_form_contains_bad_indices_and_broken_batches(ctx):
    """one col = 2c and one row = ncommit: their batches get 0 and an identity pair, the others their true verdict, the next synchronize
    returns ERR_ARG and the one after that OK; likewise a batch whose offsets decrease"""
    lib = ctx.lib
    log_n, log_l, order = 4, 2, k.NATURAL
    rng = o.SplitMix64(99)
    row, col = [0, 1, 0, 1, 0, 1, 0], [0, 1, 2, 3, 4, 5, 6]
    offsets = [0, 2, 3, 5, 7]
    commits, cells, proofs, sigma, T = v.honest(rng, log_n, log_l, order, 2, row, col)
    r = _limbs([rng.scalar() for _ in range(4)])
    commit, proof = _g1(commits), _g1(proofs)
    cs = _limbs([e for c in cells for e in c]).reshape(7, 4, 4)
    cs[5, 0, 0] ^= np.uint64(1)                                     # the last batch is wrong on its own account
    handle = _verifier(ctx, sigma, T, log_n, log_l)
    try:
        assert lib.blsgpu_synchronize(ctx.h) == 0
        bad_row, bad_col = list(row), list(col)
        bad_col[1] = 8
        bad_row[2] = 2
        call = DeviceCall(commit, bad_row, bad_col, cs, proof, offsets, r)
        call.run(handle, order)
        assert lib.blsgpu_synchronize(ctx.h) == ERR_ARG and "kzg_verify_cells_device" in lib.blsgpu_last_error().decode()
        assert lib.blsgpu_synchronize(ctx.h) == 0
        vd, ab = call.results()
        assert vd.tolist() == [0, 0, 1, 0]
        for s in (0, 1):
            xy, inf = ctx.batch_normalize(1, ab[s])
            assert inf.tolist() == [1, 1], "batch %d: no identity pair" % s
        good = DeviceCall(commit, row, col, cs, proof, offsets, r)
        good.run(handle, order)
        assert lib.blsgpu_synchronize(ctx.h) == 0
        gv, gab = good.results()
        assert gv.tolist() == [1, 1, 1, 0] and np.array_equal(gab[2:], ab[2:])
        broken = DeviceCall(commit, row, col, cs, proof, [0, 2, 1, 5, 7], r)      # the second batch decreases: it and the one behind it are broken
        broken.run(handle, order)
        assert lib.blsgpu_synchronize(ctx.h) == ERR_ARG
        assert lib.blsgpu_synchronize(ctx.h) == 0
        bv, bab = broken.results()
        assert bv.tolist() == [1, 0, 0, 0] and np.array_equal(bab[0], gab[0]) and np.array_equal(bab[3], gab[3])
        assert ctx.batch_normalize(1, bab[1])[1].tolist() == [1, 1] and ctx.batch_normalize(1, bab[2])[1].tolist() == [1, 1]
    finally:
        handle.close()
