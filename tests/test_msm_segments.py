"""Segmented MSM (`blsgpu_g{1,2}_msm_segments*`, csrc/msm_seg.hip.h): k independent small MSMs in one call.

Every result is compared as an affine point with the reference definition (the C oracle's double-and-add + Sum per segment) on a
sample of segments, and with the existing MSM path (`ctx.msm` / `point_sum`) where that covers the whole call."""
import ctypes

import numpy as np
import pytest

from oracle import bls12_381_ref as o
from oracle import c_oracle

pytestmark = pytest.mark.gpu

SEG_LEN_MAX = 4096
ERR_ARG = -2


@pytest.fixture(scope="module")
def ctx():
    import bls12_381_amd as b
    c = b.Context(0)
    yield c
    c.close()


def _scalars(n, seed):
    rs = np.random.RandomState(seed)
    s = rs.randint(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= 0x3F                                               # < 2^254 < r
    return s


def _bases(ctx, group, n, seed):
    bases = ctx.bases_from_scalars(group, _scalars(n, seed))
    xy, inf = bases.download()
    return bases, xy, inf


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)


def _aff(ctx, group, xyz):
    xy, inf = ctx.batch_normalize(group, np.asarray(xyz).reshape(-1, 18 if group == 1 else 36))
    return [(None if f else xy[i].tobytes()) for i, f in enumerate(inf)]


def _oracle(group, xy, inf, s):
    """reference-definition sum of s[i] * P_i, as (affine bytes or None for the identity)"""
    if len(s) == 0:
        return None
    msm, toaff = (c_oracle.g1_msm, c_oracle.g1_to_affine) if group == 1 else (c_oracle.g2_msm, c_oracle.g2_to_affine)
    axy, ainf = toaff(msm(xy, inf, s)[0])
    return None if ainf else axy.tobytes()


def _check_sample(ctx, group, out, xy, inf, S, off, bf, idx):
    got = _aff(ctx, group, out)
    for j in idx:
        f = int(off[j]) if bf is None else int(bf[j])
        ln = int(off[j + 1] - off[j])
        assert got[j] == _oracle(group, xy[f:f + ln], inf[f:f + ln], S[off[j]:off[j + 1]]), j


@pytest.mark.parametrize("group", [1, 2])
def test_random_lengths_contiguous(ctx, group):
    """2^12 segments of random length in [0, 64] over contiguous bases: all of them against one MSM over the concatenation (the
    sum of the segments), a sample against the oracle and against `ctx.msm` on the same slice"""
    rs = np.random.RandomState(11 + group)
    k = 1 << 12
    lens = rs.randint(0, 65, size=k)
    lens[:3] = [0, 1, 64]
    off = _offsets(lens)
    total = int(off[-1])
    bases, xy, inf = _bases(ctx, group, total, 21 + group)
    S = _scalars(total, 31 + group)
    out = ctx.msm_segments(bases, S, off)
    assert out.shape == (k, 18 if group == 1 else 36)
    assert _aff(ctx, group, ctx.point_sum(group, out)) == _aff(ctx, group, ctx.msm(bases, S))
    idx = list(range(6)) + list(rs.choice(k, 26 if group == 1 else 10, replace=False))
    _check_sample(ctx, group, out, xy, inf, S, off, None, idx)
    got = _aff(ctx, group, out)
    for j in idx[:8]:
        if lens[j]:
            assert got[j] == _aff(ctx, group, ctx.msm(bases, S[off[j]:off[j + 1]], first=int(off[j])))[0], j
    # k = 0 does nothing
    assert ctx.msm_segments(bases, S[:0], [0]).shape == (0, 18 if group == 1 else 36)


@pytest.mark.parametrize("group", [1, 2])
def test_shared_prefix_srs(ctx, group):
    """base_first all 0 (commitments to many short polynomials under one SRS), lengths up to SEG_LEN_MAX"""
    rs = np.random.RandomState(41 + group)
    k = 24
    lens = rs.randint(0, SEG_LEN_MAX + 1, size=k)
    lens[0], lens[1], lens[2] = SEG_LEN_MAX, 0, 3
    off = _offsets(lens)
    bases, xy, inf = _bases(ctx, group, SEG_LEN_MAX, 51 + group)
    S = _scalars(int(off[-1]), 61 + group)
    out = ctx.msm_segments(bases, S, off, base_first=np.zeros(k, dtype=np.uint32))
    got = _aff(ctx, group, out)
    for j in range(k):
        want = _aff(ctx, group, ctx.msm(bases, S[off[j]:off[j + 1]], first=0))[0]
        assert got[j] == want, j
    _check_sample(ctx, group, out, xy, inf, S, off, np.zeros(k, dtype=np.uint32), [1, 2])


@pytest.mark.parametrize("group", [1, 2])
def test_overlapping_base_first(ctx, group):
    rs = np.random.RandomState(71 + group)
    n, k = 3000, 300
    lens = rs.randint(0, 200, size=k)
    bf = np.array([rs.randint(0, n - ln + 1) for ln in lens], dtype=np.uint32)
    off = _offsets(lens)
    bases, xy, inf = _bases(ctx, group, n, 81 + group)
    S = _scalars(int(off[-1]), 91 + group)
    out = ctx.msm_segments(bases, S, off, base_first=bf)
    _check_sample(ctx, group, out, xy, inf, S, off, bf, list(rs.choice(k, 24 if group == 1 else 10, replace=False)))


def _edge_set(group):
    """points as oracle affine tuples: multiples of the generator, the identity, P and -P, one base repeated"""
    gen, amul, toaff, neg = ((o.G1_GEN, o.g1_affine_mul, o.g1_to_affine, o.g1_neg) if group == 1 else
                             (o.G2_GEN, o.g2_affine_mul, o.g2_to_affine, o.g2_neg))
    r = o.SplitMix64(900 + group)
    P = [toaff(amul(gen, r.scalar())) for _ in range(6)]
    ident = toaff(amul(gen, 0))
    return P + [ident, neg(P[0]), P[1], P[1], P[1]]


def _wire(group, pts):
    fp = lambda x: np.array(o.fp_to_mont_limbs(x), dtype=np.uint64)
    if group == 1:
        xy = np.stack([np.concatenate([fp(p[0]), fp(p[1])]) if not p[2] else np.zeros(12, np.uint64) for p in pts])
    else:
        xy = np.stack([np.concatenate([fp(p[0][0]), fp(p[0][1]), fp(p[1][0]), fp(p[1][1])]) if not p[2] else np.zeros(24, np.uint64) for p in pts])
    return xy, np.array([1 if p[2] else 0 for p in pts], dtype=np.uint8)


def _edge_segments(n):
    """(base_first, scalars) per segment over the edge set of _edge_set (indices: 0..5 random, 6 identity, 7 = -P0, 8..10 = P1)"""
    rr = o.R_ORDER
    r = o.SplitMix64(77)
    segs = [
        (0, []),                                                   # empty
        (2, [r.scalar()]),                                         # one point
        (0, [0] * 6),                                              # all-zero scalars
        (0, [rr - 1] * 6),                                         # r - 1
        (6, [r.scalar()]),                                         # the identity base alone
        (5, [r.scalar(), 12345, 7]),                               # identity among others
        (8, [5, 5, 5]),                                            # the same base thrice in one bucket: doubling case
        (8, [rr - 1, 1, 3]),                                       # -P1 + P1 + 3 P1: opposite digits of one base
        (0, [9] + [0] * 6 + [9]),                                  # P0 and -P0 with one scalar: the identity
        (0, [r.scalar() for _ in range(n)]),                       # everything
    ]
    return segs


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("off_subgroup", [False, True])
def test_edge_segments(ctx, kats, group, off_subgroup):
    """len 0 and 1, zero scalars, r - 1, identity bases, one base repeated in one bucket, P and -P; with an off-subgroup point in the
    set (the reference's own, test_is_torsion_free) the call runs on plain 256-bit windows and must still match the double-and-add"""
    pts = _edge_set(group)
    if off_subgroup:
        F = o.fp_from_mont_limbs
        v = kats["tests"]["g1.test_is_torsion_free" if group == 1 else "g2.test_is_torsion_free"]["fp"]
        A = (F(v[0]), F(v[1]), False) if group == 1 else ((F(v[0]), F(v[1])), (F(v[2]), F(v[3])), False)
        pts = pts + [A, A]
    xy, inf = _wire(group, pts)
    bases = ctx.upload_bases(group, xy, inf)
    assert bases.subgroup_state == (0 if off_subgroup else 1)
    segs = _edge_segments(len(pts))
    if off_subgroup:
        segs.append((len(pts) - 2, [o.R_ORDER - 1, 3]))
    lens = [len(s) for _, s in segs]
    off = _offsets(lens)
    bf = np.array([f for f, _ in segs], dtype=np.uint32)
    flat = [v for _, s in segs for v in s]
    import bls12_381_amd as b
    S = b.api.scalars_to_bytes(flat)
    out = ctx.msm_segments(bases, S, off, base_first=bf)
    # the Python oracle's `multiply` + `Sum` over the oracle's own points (the C oracle's batch MSM is not used here: identity bases)
    msm, toaff = (o.g1_msm, o.g1_to_affine) if group == 1 else (o.g2_msm, o.g2_to_affine)
    F = o.fp_from_mont_limbs
    axy, ainf = ctx.batch_normalize(group, out)
    for j, (f, sv) in enumerate(segs):
        want = toaff(msm(pts[f:f + len(sv)], sv)) if sv else None
        if ainf[j] or want is None or want[2]:
            assert bool(ainf[j]) and (want is None or want[2]), j
            continue
        w = [F(axy[j][6 * i:6 * i + 6]) for i in range(len(axy[j]) // 6)]
        got = (w[0], w[1]) if group == 1 else ((w[0], w[1]), (w[2], w[3]))
        assert got == (want[0], want[1]), j
    assert ainf[0] and ainf[2] and ainf[4] and ainf[8]


@pytest.mark.parametrize("group", [1, 2])
def test_host_form_limits(ctx, group):
    """SEG_LEN_MAX accepted; SEG_LEN_MAX + 1, decreasing offsets, a base range past the set and a scalar >= r: BLSGPU_ERR_ARG"""
    lib = ctx.lib
    fn = lib.blsgpu_g1_msm_segments if group == 1 else lib.blsgpu_g2_msm_segments
    bases, _, _ = _bases(ctx, group, SEG_LEN_MAX + 1, 101 + group)
    S = _scalars(SEG_LEN_MAX + 1, 111 + group)
    out = np.zeros((2, 18 if group == 1 else 36), dtype=np.uint64)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)

    def call(off, bf=None, s=S):
        off = np.asarray(off, dtype=np.uint32)
        bf = None if bf is None else np.asarray(bf, dtype=np.uint32)
        return fn(ctx.h, bases.handle, p(bf), p(off), p(s), len(off) - 1, p(out))

    assert call([0, SEG_LEN_MAX, SEG_LEN_MAX]) == 0
    want = _aff(ctx, group, ctx.msm(bases, S[:SEG_LEN_MAX]))[0]
    assert _aff(ctx, group, out[0])[0] == want
    assert call([0, SEG_LEN_MAX + 1]) == ERR_ARG
    assert call([0, 10, 5]) == ERR_ARG
    assert call([0, 10, 20], bf=[0, SEG_LEN_MAX - 8]) == ERR_ARG
    bad = S.copy()
    bad[3] = np.frombuffer(o.R_ORDER.to_bytes(32, "little"), dtype=np.uint8)
    assert call([0, 4, 8], s=bad) == ERR_ARG
    assert call([0, 4, 8]) == 0                                    # the context is fine afterwards
    ctx.synchronize()


@pytest.mark.parametrize("group", [1, 2])
def test_device_form_violations(ctx, group):
    """the device form cannot read the offsets: its kernel reports a violated contract through blsgpu_synchronize"""
    import torch
    import bls12_381_amd as b
    dev = torch.device("cuda", 0)
    bases, _, _ = _bases(ctx, group, 64, 121 + group)
    S = _scalars(SEG_LEN_MAX + 2, 131 + group)
    d_s = torch.from_numpy(S).to(dev)
    d_out = torch.zeros((2, 18 if group == 1 else 36), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ctx.synchronize()
    cases = [([0, 10, 5], None, 10),                               # decreasing
             ([0, SEG_LEN_MAX + 1, SEG_LEN_MAX + 1], [0, 0], SEG_LEN_MAX + 1),      # too long
             ([0, 10, 20], [0, 60], 20),                           # bases past the set
             ([0, 10, 30], None, 20)]                              # offsets[k] > total
    for offs, bf, total in cases:
        d_off = torch.tensor(np.array(offs, dtype=np.int64), dtype=torch.int32, device=dev)
        d_bf = None if bf is None else torch.tensor(bf, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ctx.msm_segments_device(bases, d_s.data_ptr(), d_off.data_ptr(), 2, total, d_out.data_ptr(),
                                d_base_first=None if d_bf is None else d_bf.data_ptr())
        with pytest.raises(b.BlsGpuError):
            ctx.synchronize()
    # a valid call leaves no flag behind
    d_off = torch.tensor([0, 10, 20], dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.msm_segments_device(bases, d_s.data_ptr(), d_off.data_ptr(), 2, 20, d_out.data_ptr())
    ctx.synchronize()
    got = _aff(ctx, group, d_out.cpu().numpy().view(np.uint64))
    assert got[1] == _aff(ctx, group, ctx.msm(bases, S[10:20], first=10))[0]


@pytest.mark.parametrize("group", [1, 2])
def test_mont_device_chain(ctx, group):
    """fr_from_bytes_device -> msm_segments_device with SCALAR_MONT on the context: no conversion in between"""
    import torch
    import bls12_381_amd as b
    dev = torch.device("cuda", 0)
    rs = np.random.RandomState(141 + group)
    lens = rs.randint(0, 40, size=200)
    off = _offsets(lens)
    total = int(off[-1])
    bases, _, _ = _bases(ctx, group, total, 151 + group)
    S = _scalars(total, 161 + group)
    want = ctx.msm_segments(bases, S, off)
    d_bytes = torch.from_numpy(S).to(dev)
    d_limbs = torch.zeros((total, 4), dtype=torch.int64, device=dev)
    d_off = torch.from_numpy(off.view(np.int32)).to(dev)
    d_out = torch.zeros((len(lens), 18 if group == 1 else 36), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ctx.fr_from_bytes_device(d_bytes.data_ptr(), total, d_limbs.data_ptr())
    ctx.set_scalar_form(b.api.SCALAR_MONT)
    try:
        ctx.msm_segments_device(bases, d_limbs.data_ptr(), d_off.data_ptr(), len(lens), total, d_out.data_ptr())
        ctx.synchronize()
        # the host form reads `to_bytes()` output whatever the context's form
        assert _aff(ctx, group, ctx.msm_segments(bases, S, off)) == _aff(ctx, group, want)
    finally:
        ctx.set_scalar_form(b.api.SCALAR_BYTES)
    assert _aff(ctx, group, d_out.cpu().numpy().view(np.uint64)) == _aff(ctx, group, want)


@pytest.mark.parametrize("group", [1, 2])
def test_between_pipelined_msm_device(ctx, group):
    """a segments call enqueued between pipelined msm_device calls: every result is right after join"""
    import torch
    dev = torch.device("cuda", 0)
    n = 1 << 14
    bases, _, _ = _bases(ctx, group, n, 171 + group)
    lens = np.random.RandomState(191 + group).randint(0, 65, size=500)
    off = _offsets(lens)
    S = _scalars(3 * n + int(off[-1]), 181 + group)
    W = 18 if group == 1 else 36
    d_s = torch.from_numpy(S).to(dev)
    d_msm = torch.zeros((3, W), dtype=torch.int64, device=dev)
    d_off = torch.from_numpy(off.view(np.int32)).to(dev)
    d_seg = torch.zeros((len(lens), W), dtype=torch.int64, device=dev)
    seg_s = d_s[3 * n:]
    torch.cuda.synchronize()
    ctx.set_pipelining(True)
    try:
        ctx.msm_device(bases, d_s[0:n].data_ptr(), n, d_msm[0].data_ptr())
        ctx.msm_device(bases, d_s[n:2 * n].data_ptr(), n, d_msm[1].data_ptr())
        ctx.msm_segments_device(bases, seg_s.data_ptr(), d_off.data_ptr(), len(lens), int(off[-1]), d_seg.data_ptr())
        ctx.msm_device(bases, d_s[2 * n:3 * n].data_ptr(), n, d_msm[2].data_ptr())
        ctx.join()
        ctx.synchronize()
    finally:
        ctx.set_pipelining(False)
    got = _aff(ctx, group, d_msm.cpu().numpy().view(np.uint64))
    for i in range(3):
        assert got[i] == _aff(ctx, group, ctx.msm(bases, S[i * n:(i + 1) * n]))[0], i
    assert _aff(ctx, group, d_seg.cpu().numpy().view(np.uint64)) == _aff(ctx, group, ctx.msm_segments(bases, S[3 * n:3 * n + int(off[-1])], off))
