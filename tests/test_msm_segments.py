"""Segmented MSM (`blsgpu_g{1,2}_msm_segments*`, csrc/msm_seg.hip.h): k independent small MSMs in one call.

Every result is compared as an affine point with the reference definition (the C oracle's double-and-add + Sum per segment) on a
sample of segments, and with the existing MSM path (`ctx.msm` / `point_sum`) where that covers the whole call."""
import ctypes
import os

import numpy as np
import pytest

from oracle import bls12_381_ref as o
from oracle import c_oracle
from msm_edge_values import boundary_values as _boundary_values, carry_values as _carry_values

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


# ---- edges of the kernel's own scalar recoding, chunk loop and batch loop, in all four (group, mode) configurations ----------------
# split: the default context over subgroup bases (G1 GLV halves, G2 psi digits); plain: a context created with BLSGPU_NO_GLV = 1, whose
# 64 windows of 4 bits span 2 (G1) or 4 (G2) workgroups that each recompute the signed digits of the windows below their own.
CONFIGS = [(1, "split"), (1, "plain"), (2, "split"), (2, "plain")]
CONFIG_IDS = ["g1-glv", "g1-plain", "g2-gls", "g2-plain"]
SEG_BATCH_BYTES = 64 << 20                                         # api_msm.hip: window sums of one batch of segments
PROJ_WORDS = {1: 44, 2: 84}                                        # msm.hip.h Store<FpPolicy / Fp2Policy>::PROJ_WORDS
NWIN = {(1, "split"): 32, (1, "plain"): 64, (2, "split"): 16, (2, "plain"): 64}     # msm_seg.hip.h SegCfg::NWIN


@pytest.fixture(scope="module")
def plain_ctx():
    import bls12_381_amd as b
    os.environ["BLSGPU_NO_GLV"] = "1"
    try:
        c = b.Context(0)
    finally:
        os.environ.pop("BLSGPU_NO_GLV")
    yield c
    c.close()


def _pick(ctx, plain_ctx, mode):
    return plain_ctx if mode == "plain" else ctx


def _gen_multiples(group, exps):
    """[e mod r] G for every e by the C oracle's double-and-add, as _aff gives points: affine limb bytes, None for the identity"""
    gen = o.G1_GEN if group == 1 else o.G2_GEN
    g, _ = _wire(group, [gen])
    sb = np.stack([np.frombuffer((int(e) % o.R_ORDER).to_bytes(32, "little"), dtype=np.uint8) for e in exps])
    xy, inf = c_oracle.mul_batch_affine(group, np.tile(g, (len(exps), 1)), None, sb)
    return [None if inf[i] else xy[i].tobytes() for i in range(len(exps))]


def _bytes(vals):
    return np.stack([np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint8) for v in vals]) if len(vals) else np.zeros((0, 32), np.uint8)


def _seg_exps(ks, ss, off, bf=None):
    """the discrete log of every segment over bases [k_i] G: sum_i k[base_first_j + i] s[offsets_j + i] mod r"""
    out = []
    for j in range(len(off) - 1):
        f = int(off[j]) if bf is None else int(bf[j])
        out.append(sum(ks[f + i] * ss[int(off[j]) + i] for i in range(int(off[j + 1] - off[j]))) % o.R_ORDER)
    return out


def _run_vs_oracle(c, group, ks, ss, lens, bf=None, bases=None):
    """segments over bases [k_i] G: every segment against the oracle; returns the (k, 18|36) result"""
    off = _offsets(lens)
    if bases is None:
        bases = c.bases_from_scalars(group, _bytes(ks))
    out = c.msm_segments(bases, _bytes(ss), off, base_first=bf)
    got = _aff(c, group, out)
    want = _gen_multiples(group, _seg_exps(ks, ss, off, bf))
    bad = [j for j in range(len(lens)) if got[j] != want[j]]
    assert not bad, "segments %s differ from the oracle (first scalar %s)" % (bad[:8], hex(ss[int(off[bad[0]])]) if lens[bad[0]] else "-")
    return out


def _rand(n, seed):
    r = o.SplitMix64(seed)
    return [r.scalar() for _ in range(n)]


@pytest.mark.parametrize("group,mode", CONFIGS, ids=CONFIG_IDS)
def test_full_range_scalars(ctx, plain_ctx, group, mode):
    """scalars uniform in [0, r) (almost half of them >= 2^254): every segment against the oracle, all of them through point_sum against
    one MSM over the concatenation"""
    from bls12_381_amd import synthetic
    c = _pick(ctx, plain_ctx, mode)
    rs = np.random.RandomState(201 + group)
    lens = rs.randint(0, 41, size=300 if group == 1 else 150)
    total = int(lens.sum())
    kb, sb = synthetic.scalars(total, 211 + group), synthetic.scalars(total, 221 + group)
    assert (sb[:, 31] >= 0x40).sum() > total // 3
    ks, ss = synthetic.to_ints(kb), synthetic.to_ints(sb)
    bases = c.bases_from_scalars(group, kb)
    out = _run_vs_oracle(c, group, ks, ss, lens, bases=bases)
    assert _aff(c, group, c.point_sum(group, out)) == _aff(c, group, c.msm(bases, sb))
    bases.free()


@pytest.mark.parametrize("group,mode", CONFIGS, ids=CONFIG_IDS)
def test_decomposition_boundaries(ctx, plain_ctx, group, mode):
    """every branch value of the GLV (G1) / psi (G2) split of tests/decomp_model.py as a product of its own, then all in one segment"""
    c = _pick(ctx, plain_ctx, mode)
    vals = _boundary_values(group)
    n = len(vals)
    ks = _rand(n, 231 + group)
    bases = c.bases_from_scalars(group, _bytes(ks))
    _run_vs_oracle(c, group, ks, vals, [1] * n, bases=bases)
    _run_vs_oracle(c, group, ks, vals, [n], bf=np.zeros(1, np.uint32), bases=bases)
    bases.free()


@pytest.mark.parametrize("group,mode", CONFIGS, ids=CONFIG_IDS)
def test_signed_recoding_carries(ctx, plain_ctx, group, mode):
    """2^(4m) - 1, - 8, - 9, + 0, + 1 and the all-8 / all-9 nibble runs for m = 1..63, nibbles 8 / 9 / F straddling bits 64, 128 and 192,
    and [2^254, r) with top nibbles 4..7: each as a product of its own, then all in one segment (several 128-scalar chunks)"""
    c = _pick(ctx, plain_ctx, mode)
    vals = _carry_values()
    n = len(vals)
    ks = _rand(n, 241 + group)
    bases = c.bases_from_scalars(group, _bytes(ks))
    _run_vs_oracle(c, group, ks, vals, [1] * n, bases=bases)
    _run_vs_oracle(c, group, ks, vals, [n], bf=np.zeros(1, np.uint32), bases=bases)
    bases.free()


@pytest.mark.parametrize("group,mode", CONFIGS, ids=CONFIG_IDS)
def test_chunk_and_list_shapes(ctx, plain_ctx, group, mode):
    """lengths at the 128-scalar chunk boundaries up to SEG_LEN_MAX over a shared prefix; one base and one scalar over a whole segment
    (every digit in one bucket per window: the longest lists, mostly doublings); P, -P alternating with equal scalars (accumulators
    back at the identity again and again, within and across chunks; for G2 the complete-addition tail and its return to XYZZ)"""
    c = _pick(ctx, plain_ctx, mode)
    lens = [127, 128, 129, 255, 256, 257, 4095, 4096]
    ks = _rand(SEG_LEN_MAX, 251 + group)
    ss = _rand(sum(lens), 261 + group)
    _run_vs_oracle(c, group, ks, ss, lens, bf=np.zeros(len(lens), np.uint32))
    k, s, t = _rand(3, 271 + group)
    ks = [k] * SEG_LEN_MAX
    _run_vs_oracle(c, group, ks, [s] * SEG_LEN_MAX + [t] * 3000, [SEG_LEN_MAX, 3000], bf=np.zeros(2, np.uint32))
    ks = [k, o.R_ORDER - k] * (SEG_LEN_MAX // 2 + 1)
    lens = [SEG_LEN_MAX, SEG_LEN_MAX - 1, SEG_LEN_MAX, 129, 2000]
    ss = [s] * (3 * SEG_LEN_MAX - 1 + 129) + [t, t, s, s] * 500          # the last: P, -P under t, then P, -P under s
    out = _run_vs_oracle(c, group, ks, ss, lens, bf=np.array([0, 0, 1, 2, 0], np.uint32))
    got = _aff(c, group, out)
    assert got[0] is None and got[2] is None and got[4] is None and got[1] is not None and got[3] is not None


@pytest.mark.parametrize("group,mode", CONFIGS, ids=CONFIG_IDS)
def test_more_than_two_batches(ctx, plain_ctx, group, mode):
    """k >= 2 x batch + 7 short segments, batch = SEG_BATCH_BYTES / (NWIN x PROJ_WORDS x 4): three launches of the batch loop, each with
    its own seg0 and output offset over the same window-sum scratch; the host and the device form"""
    import torch
    c = _pick(ctx, plain_ctx, mode)
    batch = SEG_BATCH_BYTES // (NWIN[(group, mode)] * PROJ_WORDS[group] * 4)
    k = 2 * batch + 7
    rs = np.random.RandomState(281 + group)
    lens = rs.randint(0, 4, size=k)
    check = [0, batch - 1, batch, batch + 1, 2 * batch, k - 1]
    lens[check] = 3
    off = _offsets(lens)
    total = int(off[-1])
    from bls12_381_amd import synthetic
    kb, sb = synthetic.scalars(total, 291 + group), synthetic.scalars(total, 301 + group)
    bases = c.bases_from_scalars(group, kb)
    out = c.msm_segments(bases, sb, off)
    got = _aff(c, group, out)
    whole = _aff(c, group, c.msm(bases, sb))
    assert _aff(c, group, c.point_sum(group, out)) == whole
    assert whole == _gen_multiples(group, [synthetic.dot_mod_r(kb, sb)])
    ks, ss = {}, {}
    for j in check:
        for i in range(int(off[j]), int(off[j + 1])):
            ks[i] = int.from_bytes(kb[i].tobytes(), "little"); ss[i] = int.from_bytes(sb[i].tobytes(), "little")
    want = _gen_multiples(group, [sum(ks[i] * ss[i] for i in range(int(off[j]), int(off[j + 1]))) for j in check])
    assert [got[j] for j in check] == want
    dev = torch.device("cuda", 0)
    d_s = torch.from_numpy(sb).to(dev)
    d_off = torch.from_numpy(off.view(np.int32)).to(dev)
    d_out = torch.zeros((k, 18 if group == 1 else 36), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    c.msm_segments_device(bases, d_s.data_ptr(), d_off.data_ptr(), k, total, d_out.data_ptr())
    c.synchronize()
    dgot = _aff(c, group, d_out.cpu().numpy().view(np.uint64))
    assert [dgot[j] for j in check] == want
    assert dgot == got
    bases.free()


_BAD = [o.R_ORDER, o.R_ORDER + 1, (1 << 255) + 5, (1 << 256) - 1]


@pytest.mark.parametrize("group,mode", CONFIGS, ids=CONFIG_IDS)
def test_mont_device_form_at_the_edges(ctx, plain_ctx, group, mode):
    """the boundary and carry values as `Scalar` limbs (fr_from_bytes_device -> msm_segments_device with SCALAR_MONT): the same points as
    the byte form; bytes >= r and limbs >= r reported by synchronize() in each form, and a valid call afterwards is clean"""
    import torch
    import bls12_381_amd as b
    c = _pick(ctx, plain_ctx, mode)
    dev = torch.device("cuda", 0)
    vals = _boundary_values(group) + _carry_values()
    n = len(vals)
    lens = [1] * n + [n]
    off = _offsets(lens)
    bf = np.array(list(range(n)) + [0], dtype=np.uint32)
    ks = _rand(n, 311 + group)
    bases = c.bases_from_scalars(group, _bytes(ks))
    S = _bytes(vals + vals)
    want = _aff(c, group, c.msm_segments(bases, S, off, base_first=bf))
    assert want == _gen_multiples(group, _seg_exps(ks, vals + vals, off, bf))
    d_bytes = torch.from_numpy(S).to(dev)
    d_limbs = torch.zeros((2 * n, 4), dtype=torch.int64, device=dev)
    d_off = torch.from_numpy(off.view(np.int32)).to(dev)
    d_bf = torch.from_numpy(bf.view(np.int32)).to(dev)
    d_out = torch.zeros((n + 1, 18 if group == 1 else 36), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    c.fr_from_bytes_device(d_bytes.data_ptr(), 2 * n, d_limbs.data_ptr())
    run = lambda d_s: c.msm_segments_device(bases, d_s.data_ptr(), d_off.data_ptr(), n + 1, 2 * n, d_out.data_ptr(), d_base_first=d_bf.data_ptr())
    c.set_scalar_form(b.api.SCALAR_MONT)
    try:
        run(d_limbs)
        c.synchronize()
        assert _aff(c, group, d_out.cpu().numpy().view(np.uint64)) == want
        for v in _BAD:                                             # limbs >= r
            bad = d_limbs.clone()
            bad[n + 3] = torch.from_numpy(np.frombuffer(v.to_bytes(32, "little"), dtype=np.int64).copy()).to(dev)
            torch.cuda.synchronize()
            run(bad)
            with pytest.raises(b.BlsGpuError, match="canonical"):
                c.synchronize()
        run(d_limbs)
        c.synchronize()
    finally:
        c.set_scalar_form(b.api.SCALAR_BYTES)
    for v in _BAD:                                                 # bytes >= r
        bad = d_bytes.clone()
        bad[5] = torch.from_numpy(np.frombuffer(v.to_bytes(32, "little"), dtype=np.uint8).copy()).to(dev)
        torch.cuda.synchronize()
        run(bad)
        with pytest.raises(b.BlsGpuError, match="canonical"):
            c.synchronize()
    d_out.zero_()
    run(d_bytes)
    c.synchronize()
    assert _aff(c, group, d_out.cpu().numpy().view(np.uint64)) == want
    bases.free()
