"""Interpolation in the exponent on the GPU (blsgpu_g{1,2}_lagrange_combine[_device]).  A polynomial f of degree t - 1 with random
coefficients is shared as f(id) H, H the generator; any t of the ids recover f(0) H, and f(id') H at a non-member id', for
t in {1, 2, 3, 65, 257}, G1 and G2, host and device forms.  Every expectation is a scalar in Python integers (the formula of
tests/fr_lagrange_ref.py) turned into a point by oracle/bls12_381_ref.py and compared limb for limb after batch_normalize.  Also: the
same subsets reordered in another call, an identity share, an empty segment, a repeated id (flag 0, the formula's value), a curve point
outside the subgroup among the shares, the scalar form of the context, the refusals and the sticky bit, and the chain t partial BLS
signatures -> combine -> to_bytes -> blsgpu_bls_verify_batch under the group key."""
import ctypes
import functools
import random

import numpy as np
import pytest

from oracle import bls12_381_ref as o

import fr_lagrange_ref as ref
import g_sum_points as gp
from g_ntt_points import G

pytestmark = pytest.mark.gpu

ERR_ARG = -2
THRESHOLDS = (1, 2, 3, 65, 257)


@pytest.fixture(scope="module")
def ctx():
    import bls12_381_amd as b
    return b.default_context()


def _scalar_bytes(vals):
    return np.stack([np.frombuffer((int(v) % ref.R).to_bytes(32, "little"), dtype=np.uint8) for v in vals])


def _poly(coef, x):
    acc = 0
    for c in reversed(coef):
        acc = (acc * x + c) % ref.R
    return acc


@functools.lru_cache(maxsize=None)
def sharing():
    """[(ids, z, share scalars, name)] and the scalar every segment must give: for every t two subsets at z = 0 and one at a non-member
    id'; then a segment with a zero share (the identity), an empty one, one with a repeated id"""
    rng = random.Random(91)
    segs, want = [], []
    for t in THRESHOLDS:
        coef = [rng.randrange(ref.R) for _ in range(t)]
        ids = rng.sample(range(1, 4 * t + 8), t + 3)
        a, b = ids[:t], rng.sample(ids, t)
        outsider = ids[t]
        assert outsider not in a
        for name, sub, z in (("t=%d A" % t, a, 0), ("t=%d B" % t, b, 0), ("t=%d at id'" % t, a, outsider)):
            segs.append((sub, z, [_poly(coef, i) for i in sub], name)); want.append(_poly(coef, z))
    ids = [3, 8, 1, 12, 5]
    sh = [rng.randrange(ref.R) for _ in ids]
    sh[2] = 0
    segs.append((ids, 0, sh, "identity share")); want.append(ref.interpolate(ref.lagrange(ids, 0)[0], sh))
    segs.append(([], 7, [], "empty")); want.append(0)
    ids = [4, 9, 4, 2, 6]
    sh = [rng.randrange(ref.R) for _ in ids]
    segs.append((ids, 0, sh, "repeated id")); want.append(ref.interpolate(ref.lagrange(ids, 0)[0], sh))
    return segs, want


def _pack(segs):
    off = np.zeros(len(segs) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(s[0]) for s in segs])
    return ref.to_limbs([i for s in segs for i in s[0]]), off, ref.to_limbs([s[1] for s in segs]), [v for s in segs for v in s[2]]


def _shares(ctx, group, scalars):
    """[s] H for every share scalar, as affine wire points (s = 0 gives the identity)"""
    return ctx.bases_from_scalars(group, _scalar_bytes(scalars)).download()


def _same_points(ctx, group, out_xyz, want_affine, what):
    xy, inf = ctx.batch_normalize(group, out_xyz)
    wxy, winf = gp.wire_points(group, want_affine)
    assert np.array_equal(inf, winf), what
    live = winf == 0
    assert np.array_equal(xy[live], wxy[live]), "%s: segments %s" % (what, np.nonzero((xy != wxy).any(axis=1) & live)[0][:10])


def _device_call(ctx, group, xy, inf, nodes, off, points, total=None, sync=True):
    import torch
    dev = torch.device("cuda", 0)
    nseg = off.shape[0] - 1
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    d = [up(a) for a in (xy, inf, nodes, off, points)]
    d_out = torch.full((max(nseg, 1) * 18 * group * 8,), 0xA5, dtype=torch.uint8, device=dev)
    d_fl = torch.full((max(nseg, 16),), 0xA5, dtype=torch.uint8, device=dev)
    ptr = lambda t: 0 if t is None else t.data_ptr()
    ctx.lagrange_combine_device(group, ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), nseg, xy.shape[0] if total is None else total, ptr(d[4]), d_out.data_ptr(), d_fl.data_ptr())
    if sync:
        ctx.synchronize()
    else:
        torch.cuda.synchronize()
    return d_out.cpu().numpy().view(np.uint64).reshape(-1, 18 * group)[:nseg], d_fl.cpu().numpy()[:nseg]


@pytest.mark.parametrize("group", [1, 2])
def test_any_t_of_n_recover_the_secret_and_new_shares(ctx, group):
    segs, want = sharing()
    nodes, off, points, scalars = _pack(segs)
    xy, inf = _shares(ctx, group, scalars)
    assert inf.sum() == 1                                          # the zero share
    grp = G[group]
    want_aff = [grp.to_affine(grp.base_mul(w)) for w in want]
    flags_want = [ref.lagrange(s[0], s[1])[1] for s in segs]
    assert flags_want.count(0) == 1
    out, fl = ctx.lagrange_combine(group, xy, inf, nodes, off, points)
    _same_points(ctx, group, out, want_aff, "G%d host form" % group)
    assert fl.tolist() == flags_want
    out, fl = _device_call(ctx, group, xy, inf, nodes, off, points)
    _same_points(ctx, group, out, want_aff, "G%d device form" % group)
    assert fl.tolist() == flags_want
    # the same segments in another order, every segment's shares in another order: the same group elements
    rng = random.Random(5)
    order = list(range(len(segs))); rng.shuffle(order)
    shuffled = []
    for k in order:
        ids, z, sh, name = segs[k]
        perm = list(range(len(ids))); rng.shuffle(perm)
        shuffled.append(([ids[p] for p in perm], z, [sh[p] for p in perm], name))
    nodes2, off2, points2, scalars2 = _pack(shuffled)
    xy2, inf2 = _shares(ctx, group, scalars2)
    out2, _ = ctx.lagrange_combine(group, xy2, inf2, nodes2, off2, points2)
    a, b = ctx.batch_normalize(group, out), ctx.batch_normalize(group, out2)
    assert np.array_equal(a[1][order], b[1]) and np.array_equal(a[0][order][b[1] == 0], b[0][b[1] == 0])
    # integer ids and points == NULL through the Python front: the z = 0 segments only
    z0 = [s for s in segs if s[1] == 0 and s[0]][:4]
    n0, o0, _, s0 = _pack(z0)
    x0, i0 = _shares(ctx, group, s0)
    out0, _ = ctx.lagrange_combine(group, x0, i0, [i for s in z0 for i in s[0]], o0)
    _same_points(ctx, group, out0, [grp.to_affine(grp.base_mul(ref.interpolate(ref.lagrange(s[0], 0)[0], s[2]))) for s in z0], "G%d integer ids" % group)


@pytest.mark.parametrize("group", [1, 2])
def test_a_point_outside_the_subgroup_and_the_scalar_form(ctx, group):
    """assume_subgroup off (the default): a curve point outside the prime-order subgroup among the shares is multiplied exactly, as
    mul_batch does; and the coefficients are Montgomery limbs whatever blsgpu_set_scalar_form says"""
    rng = random.Random(17 + group)
    grp, pl = G[group], gp.pool(group)
    from_aff = o.g1_from_affine if group == 1 else o.g2_from_affine
    ids = [2, 5, 7, 11]
    sh = [rng.randrange(ref.R) for _ in ids]
    xy, inf = _shares(ctx, group, sh)
    qxy, qinf = gp.wire_points(group, [pl.points[pl.off]])
    xy[1] = qxy[0]
    z = 9
    lam = ref.lagrange(ids, z)[0]
    terms = [grp.mul(from_aff(pl.points[pl.off]), lam[1])] + [grp.base_mul(lam[i] * sh[i]) for i in (0, 2, 3)]
    want = [grp.to_affine(grp.sum(terms))]
    off = np.array([0, 4], dtype=np.uint32)
    out, fl = ctx.lagrange_combine(group, xy, inf, ids, off, [z])
    _same_points(ctx, group, out, want, "G%d off-subgroup share" % group)
    for form in (1, 0):
        ctx.set_scalar_form(form)
        try:
            out, _ = _device_call(ctx, group, xy, inf, ref.to_limbs(ids), off, ref.to_limbs([z]))
        finally:
            ctx.set_scalar_form(0)
        _same_points(ctx, group, out, want, "G%d scalar form %d" % (group, form))


def test_threshold_signature_chain(ctx):
    """t = 5 of n = 8 partial BLS signatures (public keys in G1, signatures in G2) -> lagrange_combine_device -> batch_normalize ->
    to_bytes -> bls_verify_batch says 1 under the group key; t - 1 honest shares and one wrong one say 0"""
    rng = random.Random(123)
    t, n = 5, 8
    dst = b"BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_"
    msg = b"threshold committees sign once"
    coef = [rng.randrange(ref.R) for _ in range(t)]
    ids = list(range(1, n + 1))
    sk = {i: _poly(coef, i) for i in ids}
    pk_xy, pk_inf = _shares(ctx, 1, [coef[0]])
    pk_bytes = ctx.points_to_bytes(1, pk_xy, pk_inf, compressed=True)
    hxy, hinf = ctx.batch_normalize(2, ctx.hash_to_curve(2, [msg], dst))
    honest, other = [7, 2, 5, 8, 3], [1, 4, 6, 8, 2]
    wrong = list(honest)
    parts = [sk[i] for i in honest] + [sk[i] for i in other] + [sk[i] for i in wrong[:-1]] + [sk[wrong[-1]] + 1]
    sxy, sinf = ctx.batch_normalize(2, ctx.mul_batch(2, np.tile(hxy, (15, 1)), np.tile(hinf, 15), _scalar_bytes(parts)))
    off = np.array([0, 5, 10, 15], dtype=np.uint32)
    out, fl = _device_call(ctx, 2, sxy, sinf, ref.to_limbs(honest + other + wrong), off, None)
    assert fl.tolist() == [1, 1, 1]
    gxy, ginf = ctx.batch_normalize(2, out)
    assert np.array_equal(gxy[0], gxy[1]) and not np.array_equal(gxy[0], gxy[2])       # any t shares give the same signature
    sig_bytes = ctx.points_to_bytes(2, gxy, ginf, compressed=True)
    got = ctx.bls_verify_batch(0, np.tile(pk_bytes, (3, 1)), sig_bytes, [msg] * 3, dst)
    assert got.tolist() == [1, 1, 0]


def test_refusals_and_the_sticky_bit(ctx):
    import torch
    import bls12_381_amd as b
    rng = random.Random(8)
    ids = rng.sample(range(1, 100), 12)
    sh = [rng.randrange(ref.R) for _ in ids]
    xy, inf = _shares(ctx, 1, sh)
    nodes, points = ref.to_limbs(ids), ref.to_limbs([0, 3])
    off = np.array([0, 5, 12], dtype=np.uint32)
    out, fl = np.zeros((2, 18), dtype=np.uint64), np.zeros(2, dtype=np.uint8)
    host = ctx.lib.blsgpu_g1_lagrange_combine
    p = lambda a, o_=0: ctypes.c_void_p(a.ctypes.data + o_)
    good = (p(xy), p(inf), p(nodes), p(off), 2, p(points), p(out), p(fl))
    assert host(ctx.h, *good) == 0
    for what, i, arg in (("NULL xy", 0, None), ("NULL infinity", 1, None), ("NULL nodes", 2, None), ("NULL offsets", 3, None), ("NULL out", 6, None),
                         ("nseg > 2^27", 4, (1 << 27) + 1), ("out on the shares", 6, p(xy, 8)), ("flags on the nodes", 7, p(nodes, 3)), ("flags inside out", 7, p(out, 17))):
        args = list(good); args[i] = arg
        assert host(ctx.h, *args) == ERR_ARG, what
    dec = np.array([0, 7, 5], dtype=np.uint32)
    assert host(ctx.h, p(xy), p(inf), p(nodes), p(dec), 2, p(points), p(out), p(fl)) == ERR_ARG, "decreasing offsets"
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    d_xy, d_inf, d_n, d_off, d_p = [up(a) for a in (xy, inf, nodes, off, points)]
    d_out = torch.zeros(2 * 144 + 16, dtype=torch.uint8, device=dev)
    d_fl = torch.zeros(16, dtype=torch.uint8, device=dev)
    fn = ctx.lib.blsgpu_g1_lagrange_combine_device
    v = lambda t, o_=0: ctypes.c_void_p(t.data_ptr() + o_)
    good = (v(d_xy), v(d_inf), v(d_n), v(d_off), 2, 12, v(d_p), v(d_out), v(d_fl))
    assert fn(ctx.h, *good) == 0
    ctx.synchronize()
    for what, i, arg in (("NULL d_xy", 0, None), ("NULL d_inf", 1, None), ("NULL d_nodes", 2, None), ("NULL d_offsets", 3, None), ("NULL d_out", 7, None),
                         ("total > 2^27", 5, (1 << 27) + 1), ("misaligned d_xy", 0, v(d_xy, 4)), ("misaligned d_nodes", 2, v(d_n, 8)), ("misaligned d_offsets", 3, v(d_off, 2)),
                         ("misaligned d_points", 6, v(d_p, 8)), ("misaligned d_out", 7, v(d_out, 4)), ("d_out on d_xy", 7, v(d_xy)), ("d_flags on d_inf", 8, v(d_inf, 2))):
        args = list(good); args[i] = arg
        assert fn(ctx.h, *args) == ERR_ARG, what
    ctx.synchronize()                                               # nothing was launched, nothing is flagged
    assert ctx.lib.blsgpu_g2_lagrange_combine_device(ctx.h, None, None, None, None, 0, 0, None, None, None) == 0
    assert ctx.lib.blsgpu_g1_lagrange_combine(ctx.h, None, None, None, None, 0, None, None, None) == 0
    # the sticky bit: segment 1 ends beyond total, segment 2 decreases; segments 0 and 3 are right, the other two are not written
    bad = np.array([0, 5, 20, 5, 12], dtype=np.uint32)
    out, fl = _device_call(ctx, 1, xy, inf, nodes, bad, ref.to_limbs([0, 3, 3, 0]), sync=False)
    with pytest.raises(b.BlsGpuError, match="lagrange_combine_device"):
        ctx.synchronize()
    ctx.synchronize()
    assert (out[1:3] == np.uint64(0xA5A5A5A5A5A5A5A5)).all() and fl.tolist() == [1, 0xA5, 0xA5, 1]
    grp = G[1]
    want = [grp.to_affine(grp.base_mul(ref.interpolate(ref.lagrange(ids[a:e], 0)[0], sh[a:e]))) for a, e in ((0, 5), (5, 12))]
    _same_points(ctx, 1, out[[0, 3]], want, "the neighbours of a bad segment")
