"""Parity of the HIP path (through the C ABI) against the oracle and the reference's golden vectors.

All tests need a real MI355X (`-m gpu`).  Comparison points: field elements and Gt / raw
Miller values as canonical Montgomery limbs (bit-exact), group elements as uncompressed affine bytes;
point-formula outputs additionally as exact projective triples, because the kernels use the reference's
own complete formulas.
"""
import os

import numpy as np
import pytest

from oracle import bls12_381_ref as o

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import bls12_381_amd as b
    return b.default_context()


# ---- oracle <-> wire helpers ---------------------------------------------------------------------------
def fpw(x):
    return np.array(o.fp_to_mont_limbs(x), dtype=np.uint64)


def fp2w(a):
    return np.concatenate([fpw(a[0]), fpw(a[1])])


def fp12w(f):
    return np.concatenate([fpw(c) for c in o.fp12_flatten(f)])


def wfp(w):
    return o.fp_from_mont_limbs([int(x) for x in w])


def wfp2(w):
    return (wfp(w[0:6]), wfp(w[6:12]))


def wfp12(w):
    return o.fp12_unflatten([wfp(w[6 * i:6 * i + 6]) for i in range(12)])


def g1aff_w(a):
    return np.concatenate([fpw(a[0]), fpw(a[1])]), np.uint8(1 if a[2] else 0)


def g2aff_w(a):
    return np.concatenate([fp2w(a[0]), fp2w(a[1])]), np.uint8(1 if a[2] else 0)


def g1proj_w(p):
    return np.concatenate([fpw(p[0]), fpw(p[1]), fpw(p[2])])


def g2proj_w(p):
    return np.concatenate([fp2w(p[0]), fp2w(p[1]), fp2w(p[2])])


def w_g1proj(w):
    return (wfp(w[0:6]), wfp(w[6:12]), wfp(w[12:18]))


def w_g2proj(w):
    return (wfp2(w[0:12]), wfp2(w[12:24]), wfp2(w[24:36]))


def rng_fp(r):
    v = 0
    for i in range(6):
        v |= r.next() << (64 * i)
    return v % o.P


EDGE_FP = [0, 1, 2, o.P - 1, o.P - 2, (o.P - 1) // 2, (o.P + 1) // 2, (1 << 380), (1 << 381) - 1 - ((1 << 381) - 1) // o.P * 0,
           o.MONT_R, pow(o.MONT_R, -1, o.P), 0xFFFFFFFF, (1 << 364) - 1, (1 << 364), o.P - (1 << 28), (1 << 28) - 1]
EDGE_FP = [v % o.P for v in EDGE_FP]


# ---- field arithmetic ------------------------------------------------------------------------------------
def test_fp_ops(ctx, kats):
    r = o.SplitMix64(0xB1512381)
    a = EDGE_FP + [rng_fp(r) for _ in range(3000)]
    b = list(reversed(EDGE_FP)) + [rng_fp(r) for _ in range(3000)]
    # the reference's own multiplication / squaring KAT operands (src/fp.rs:700-749)
    t = kats["tests"]
    ka, kb, _ = [o.fp_from_mont_limbs(v) for v in t["fp.test_multiplication"]["fp"]]
    a += [ka, o.fp_from_mont_limbs(t["fp.test_squaring"]["fp"][0])]
    b += [kb, o.fp_from_mont_limbs(t["fp.test_squaring"]["fp"][0])]
    A, B = np.stack([fpw(x) for x in a]), np.stack([fpw(x) for x in b])
    for op, fn in [(0, o.fp_mul), (1, o.fp_add), (2, o.fp_sub)]:
        got = ctx.fp_op(op, A, B)
        want = np.stack([fpw(fn(x, y)) for x, y in zip(a, b)])
        assert np.array_equal(got, want), f"fp op {op}"
    assert np.array_equal(ctx.fp_op(3, A), np.stack([fpw(o.fp_sqr(x)) for x in a]))
    assert np.array_equal(ctx.fp_op(5, A), np.stack([fpw(o.fp_neg(x)) for x in a]))
    inv = ctx.fp_op(4, A[:200])
    assert np.array_equal(inv, np.stack([fpw(o.fp_inv(x) or 0) for x in a[:200]]))
    # the safegcd inversion (op 4) against the on-device x^(p-2) (op 6) on every operand, and a * a^-1 = 1
    inv_all = ctx.fp_op(4, A)
    assert np.array_equal(inv_all, ctx.fp_op(6, A))
    nz = [i for i, x in enumerate(a) if x % o.P]
    assert np.array_equal(ctx.fp_op(0, A[nz], inv_all[nz]), np.stack([fpw(1)] * len(nz)))
    # KAT results verbatim
    assert np.array_equal(ctx.fp_op(0, np.array([t["fp.test_multiplication"]["fp"][0]], dtype=np.uint64),
                                    np.array([t["fp.test_multiplication"]["fp"][1]], dtype=np.uint64))[0],
                          np.array(t["fp.test_multiplication"]["fp"][2], dtype=np.uint64))


def test_fp2_ops(ctx, kats):
    r = o.SplitMix64(7)
    a = [(x, y) for x in EDGE_FP[:6] for y in EDGE_FP[:6]] + [(rng_fp(r), rng_fp(r)) for _ in range(1500)]
    b = [(rng_fp(r), rng_fp(r)) for _ in range(len(a))]
    A, B = np.stack([fp2w(x) for x in a]), np.stack([fp2w(x) for x in b])
    for op, fn in [(0, o.fp2_mul), (1, o.fp2_add), (2, o.fp2_sub)]:
        assert np.array_equal(ctx.fp2_op(op, A, B), np.stack([fp2w(fn(x, y)) for x, y in zip(a, b)])), f"fp2 op {op}"
    assert np.array_equal(ctx.fp2_op(3, A), np.stack([fp2w(o.fp2_sqr(x)) for x in a]))
    assert np.array_equal(ctx.fp2_op(5, A), np.stack([fp2w(o.fp2_neg(x)) for x in a]))
    assert np.array_equal(ctx.fp2_op(6, A), np.stack([fp2w(o.fp2_mul_by_nonresidue(x)) for x in a]))
    assert np.array_equal(ctx.fp2_op(4, A[:100]), np.stack([fp2w(o.fp2_inv(x) or (0, 0)) for x in a[:100]]))
    t = kats["tests"]["fp2.test_multiplication"]["fp"]
    got = ctx.fp2_op(0, np.array([t[0] + t[1]], dtype=np.uint64), np.array([t[2] + t[3]], dtype=np.uint64))[0]
    assert np.array_equal(got, np.array(t[4] + t[5], dtype=np.uint64))


def test_fp12_ops(ctx):
    r = o.SplitMix64(99)
    def rnd12(): return o.fp12_unflatten([rng_fp(r) for _ in range(12)])
    a = [rnd12() for _ in range(40)] + [o.FP12_ONE]
    b = [rnd12() for _ in range(41)]
    A, B = np.stack([fp12w(x) for x in a]), np.stack([fp12w(x) for x in b])
    assert np.array_equal(ctx.fp12_op(0, A, B), np.stack([fp12w(o.fp12_mul(x, y)) for x, y in zip(a, b)]))
    assert np.array_equal(ctx.fp12_op(3, A), np.stack([fp12w(o.fp12_sqr(x)) for x in a]))
    assert np.array_equal(ctx.fp12_op(4, A), np.stack([fp12w(o.fp12_inv(x)) for x in a]))
    assert np.array_equal(ctx.fp12_op(7, A), np.stack([fp12w(o.fp12_frobenius(x)) for x in a]))
    assert np.array_equal(ctx.fp12_op(8, A), np.stack([fp12w(o.fp12_conj(x)) for x in a]))
    # cyclotomic_square is only meaningful on the cyclotomic subgroup: x^((p^6-1)(p^2+1))
    def to_cyc(f):
        t = f
        for _ in range(6):
            t = o.fp12_frobenius(t)
        t = o.fp12_mul(t, o.fp12_inv(f))
        return o.fp12_mul(o.fp12_frobenius(o.fp12_frobenius(t)), t)
    cyc = [to_cyc(x) for x in a[:8]]
    C = np.stack([fp12w(x) for x in cyc])
    want = np.stack([fp12w(o.cyclotomic_square(x)) for x in cyc])
    assert np.array_equal(ctx.fp12_op(9, C), want)
    assert np.array_equal(want, np.stack([fp12w(o.fp12_sqr(x)) for x in cyc]))
    # product tree
    assert np.array_equal(ctx.fp12_product(A[:19]), fp12w(__import__("functools").reduce(o.fp12_mul, a[:19])))
    assert np.array_equal(ctx.fp12_product(A[:0]), fp12w(o.FP12_ONE))


# ---- point formulas: exact projective triples --------------------------------------------------------------
def _points(group, n, seed):
    r = o.SplitMix64(seed)
    gen = o.G1_GEN if group == 1 else o.G2_GEN
    mul = o.g1_affine_mul if group == 1 else o.g2_affine_mul
    ident = o.g1_identity() if group == 1 else o.g2_identity()
    pts = [mul(gen, r.scalar()) for _ in range(n)]
    return pts, ident


@pytest.mark.parametrize("group", [1, 2])
def test_point_ops(ctx, group):
    pts, ident = _points(group, 12, 5 + group)
    pw, wp = (g1proj_w, w_g1proj) if group == 1 else (g2proj_w, w_g2proj)
    add, dbl, madd, toaff = (o.g1_add, o.g1_double, o.g1_add_mixed, o.g1_to_affine) if group == 1 else \
        (o.g2_add, o.g2_double, o.g2_add_mixed, o.g2_to_affine)
    affw = g1aff_w if group == 1 else g2aff_w
    neg = o.g1_neg if group == 1 else o.g2_neg
    a = pts[:6] + [ident, pts[0], pts[1], ident, pts[2], pts[3]]
    b = pts[6:] + [pts[3], ident, pts[1], ident, neg(pts[2]), dbl(pts[3])]
    A, B = np.stack([pw(x) for x in a]), np.stack([pw(x) for x in b])
    got = ctx.point_op(group, 0, A, B)
    for i, (x, y) in enumerate(zip(a, b)):
        assert wp(got[i]) == add(x, y), f"add {i}"
    got = ctx.point_op(group, 1, A)
    for i, x in enumerate(a):
        assert toaff(wp(got[i])) == toaff(dbl(x)), f"double {i}"
        if not toaff(x)[2]:
            assert wp(got[i]) == dbl(x)
    baff = [toaff(y) for y in b]
    Bx = np.stack([affw(y)[0] for y in baff])
    Bi = np.array([affw(y)[1] for y in baff], dtype=np.uint8)
    got = ctx.point_op(group, 2, A, Bx, Bi)
    for i, (x, y) in enumerate(zip(a, baff)):
        assert wp(got[i]) == madd(x, y), f"mixed {i}"
    # Sum + batch_normalize (incl. identities)
    s = ctx.point_sum(group, A)
    acc = ident
    for x in a:
        acc = add(acc, x)
    assert toaff(wp(s)) == toaff(acc)
    xy, inf = ctx.batch_normalize(group, A)
    for i, x in enumerate(a):
        ex, ei = affw(toaff(x))
        assert np.array_equal(xy[i], ex) and inf[i] == ei


@pytest.mark.parametrize("group", [1, 2])
def test_fixed_base_multiples_match_golden(ctx, group, golden_dir):
    """k * generator for k = 0..999 computed on the GPU == src/tests/*_uncompressed_valid_test_vectors.dat."""
    import bls12_381_amd as b
    ks = list(range(1000))
    bases = ctx.bases_from_scalars(group, ks)
    xy, inf = bases.download()
    name = "g1" if group == 1 else "g2"
    usz = 96 if group == 1 else 192
    raw = open(os.path.join(golden_dir, f"{name}_uncompressed_valid_test_vectors.dat"), "rb").read()
    craw = open(os.path.join(golden_dir, f"{name}_compressed_valid_test_vectors.dat"), "rb").read()
    cls = b.G1Affine if group == 1 else b.G2Affine
    for k in ks:
        pt = cls(xy[k], bool(inf[k]))
        assert pt.to_uncompressed() == raw[usz * k:usz * (k + 1)], k
        assert pt.to_compressed() == craw[usz // 2 * k:usz // 2 * (k + 1)], k
        if k % 100 == 0:
            assert cls.from_uncompressed_unchecked(raw[usz * k:usz * (k + 1)]) == pt


# ---- MSM ---------------------------------------------------------------------------------------------------
def _msm_case(ctx, group, ks, scalars, window=0):
    """bases = [k_i] G built on the device; expected = [sum k_i s_i] G from the oracle (discrete-log identity),
    compared on uncompressed affine bytes."""
    ctx.set_msm_window(window)
    bases = ctx.bases_from_scalars(group, ks)
    out = ctx.msm(bases, scalars)
    xy, inf = ctx.batch_normalize(group, out[None, :])
    tot = sum(k * s for k, s in zip(ks, scalars)) % o.R_ORDER
    if group == 1:
        want = o.g1_to_uncompressed(o.g1_to_affine(o.g1_affine_mul(o.G1_GEN, tot)))
        import bls12_381_amd as b
        got = b.G1Affine(xy[0], bool(inf[0])).to_uncompressed()
    else:
        want = o.g2_to_uncompressed(o.g2_to_affine(o.g2_affine_mul(o.G2_GEN, tot)))
        import bls12_381_amd as b
        got = b.G2Affine(xy[0], bool(inf[0])).to_uncompressed()
    ctx.set_msm_window(0)
    assert got == want


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("n", [0, 1, 2, 3, 17, 256, 1024])
def test_msm_small_vs_reference_definition(ctx, group, n):
    """sum_i (P_i * s_i) exactly as the reference defines it (double-and-add + Sum), n <= 2^10 (config 1)."""
    r = o.SplitMix64(0xB1512381 + n)
    ks = [r.scalar() for _ in range(n)]
    ss = [r.scalar() for _ in range(n)]
    if n <= 17:
        gen, amul, msm, toaff, enc = (o.G1_GEN, o.g1_affine_mul, o.g1_msm, o.g1_to_affine, o.g1_to_uncompressed) if group == 1 else \
            (o.G2_GEN, o.g2_affine_mul, o.g2_msm, o.g2_to_affine, o.g2_to_uncompressed)
        pts = [toaff(amul(gen, k)) for k in ks]
        want = enc(toaff(msm(pts, ss)))
        import bls12_381_amd as b
        if group == 1:
            got = b.msm_g1([b.G1Affine(*g1aff_w(p)) for p in pts], ss).to_affine().to_uncompressed()
        else:
            got = b.msm_g2([b.G2Affine(*g2aff_w(p)) for p in pts], ss).to_affine().to_uncompressed()
        assert got == want
    _msm_case(ctx, group, ks, ss)


@pytest.mark.parametrize("group", [1, 2])
def test_msm_edge_cases(ctx, group):
    r = o.SplitMix64(4242)
    rr = o.R_ORDER
    # scalars 0, 1, r-1, 2^k boundaries; identity bases (k = 0); duplicates; P and -P with equal digits
    ks = [1, 2, 3, 0, 5, 5, 5, rr - 5, 7, rr - 7, 0, 11] + [r.scalar() for _ in range(20)]
    ss = [0, 1, rr - 1, 12345, 9, 9, rr - 9, 9, (1 << 254), (1 << 254), 0, (1 << 16) - 1] + \
         [(1 << (16 * i)) - 1 for i in range(1, 11)] + [(1 << 15) + (1 << (16 * i + 15)) for i in range(10)]
    for w in (0, 4, 7, 13, 16):
        _msm_case(ctx, group, ks, ss, window=w)
    _msm_case(ctx, group, [3] * 300, [1] * 300)                 # one bucket takes everything
    _msm_case(ctx, group, [r.scalar() for _ in range(64)], [0] * 64)     # all-zero scalars -> identity
    _msm_case(ctx, group, [4, rr - 4], [77, 77])                          # P + (-P) inside one bucket


@pytest.mark.parametrize("group,logn", [(1, 14), (1, 16), (2, 14)])
def test_msm_medium(ctx, group, logn):
    n = 1 << logn
    r = o.SplitMix64(logn * 1000 + group)
    ks = [r.scalar() for _ in range(n)]
    ss = [r.scalar() for _ in range(n)]
    _msm_case(ctx, group, ks, ss)


def test_msm_full_size_2_20(ctx):
    """BASELINE config 2: 2^20-point G1 MSM, checked through the discrete-log identity."""
    from bls12_381_amd import synthetic as sy
    n = 1 << 20
    # the headline distribution: uniform in [0, r) by rejection, all 255 bits in play -- bench.py's own sampler and seed
    kb = sy.scalars(n, sy.SEED + 1)
    sb = sy.scalars(n, sy.SEED)
    assert int(sb[:, 31].max()) >= 0x70 and int(kb[:, 31].max()) >= 0x70          # scalars above 2^254 are present
    ss = sy.to_ints(sb)
    bases = ctx.bases_from_scalars(1, kb)
    out = ctx.msm(bases, sb)
    xy, inf = ctx.batch_normalize(1, out[None, :])
    tot = sy.dot_mod_r(kb, sb)
    import bls12_381_amd as b
    assert b.G1Affine(xy[0], bool(inf[0])).to_uncompressed() == o.g1_to_uncompressed(o.g1_to_affine(o.g1_affine_mul(o.G1_GEN, tot)))
    # linearity (size-independent property): MSM(2s) == 2 * MSM(s)
    s2 = [(2 * s) % o.R_ORDER for s in ss[:4096]]
    a = ctx.msm(bases, ss[:4096]); b2 = ctx.msm(bases, s2)
    d = ctx.point_op(1, 1, a[None, :])
    assert np.array_equal(ctx.batch_normalize(1, d)[0], ctx.batch_normalize(1, b2[None, :])[0])


# ---- pairings --------------------------------------------------------------------------------------------------
def _pair_inputs(n, seed):
    r = o.SplitMix64(seed)
    ps = [o.g1_to_affine(o.g1_affine_mul(o.G1_GEN, r.scalar())) for _ in range(n)]
    qs = [o.g2_to_affine(o.g2_affine_mul(o.G2_GEN, r.scalar())) for _ in range(n)]
    return ps, qs


def test_pairing_generator_kat(ctx, kats):
    """src/tests/mod.rs:78-231: e(G1gen, G2gen) == the RELIC constant, bit for bit."""
    import bls12_381_amd as b
    want = np.array(kats["consts"]["pairings.GT_GENERATOR"], dtype=np.uint64).reshape(72)
    got = b.pairing(b.G1Affine.generator(), b.G2Affine.generator())
    assert np.array_equal(got.f, want)
    ml = b.multi_miller_loop([(b.G1Affine.generator(), b.G2Prepared(b.G2Affine.generator()))])
    assert np.array_equal(ml.final_exponentiation().f, want)
    assert b.Gt.generator() == got and b.Bls12.pairing(b.G1Affine.generator(), b.G2Affine.generator()) == got


def test_pairing_batch_vs_oracle(ctx):
    ps, qs = _pair_inputs(6, 31337)
    ps += [o.G1_IDENTITY_AFF, ps[0]]
    qs += [qs[0], o.G2_IDENTITY_AFF]
    G1 = np.stack([g1aff_w(p)[0] for p in ps]); F1 = np.array([g1aff_w(p)[1] for p in ps], dtype=np.uint8)
    G2 = np.stack([g2aff_w(q)[0] for q in qs]); F2 = np.array([g2aff_w(q)[1] for q in qs], dtype=np.uint8)
    ml = ctx.miller_loop_batch(G1, F1, G2, F2)
    want_ml = [o.miller_loop(p, q) for p, q in zip(ps, qs)]
    for i in range(len(ps)):
        assert np.array_equal(ml[i], fp12w(want_ml[i])), f"miller {i}"
    gt = ctx.pairing_batch(G1, F1, G2, F2)
    for i in range(len(ps)):
        assert np.array_equal(gt[i], fp12w(o.final_exponentiation(want_ml[i]))), f"pairing {i}"
    assert np.array_equal(ctx.final_exponentiation_batch(ml), gt)
    # multi_miller_loop: same Fp12 value as the reference's shared-accumulator loop (identities skipped)
    mm = ctx.multi_miller_loop(G1, F1, G2, F2)
    want_mm = o.multi_miller_loop([(p, o.g2_prepare(q)) for p, q in zip(ps, qs)])
    assert np.array_equal(mm, fp12w(want_mm))
    assert np.array_equal(ctx.multi_miller_loop(G1[:0], F1[:0], G2[:0], F2[:0]), fp12w(o.FP12_ONE))


def test_pairing_bilinearity_and_api(ctx):
    """pairings.rs:835-921 through the mirrored API."""
    import bls12_381_amd as b
    a, c = b.Scalar(0x1234567890ABCDEF), b.Scalar(0xFEDCBA0987654321)
    g = (b.G1Affine.generator() * a).to_affine()
    h = (b.G2Affine.generator() * c).to_affine()
    p = b.pairing(g, h)
    assert p == b.pairing((b.G1Affine.generator() * (a * c)).to_affine(), b.G2Affine.generator())
    assert p == b.Gt.generator() * (a * c)
    assert p != b.Gt.identity()
    assert b.pairing(b.G1Affine.identity(), h) == b.Gt.identity()
    assert -p == b.pairing(g, -h) and (p + (-p)) == b.Gt.identity()
    terms = [(g, b.G2Prepared(h)), (b.G1Affine.identity(), b.G2Prepared(h)), (b.G1Affine.generator(), b.G2Prepared(b.G2Affine.generator()))]
    assert b.multi_miller_loop(terms).final_exponentiation() == p + b.Gt.generator()
    assert b.MillerLoopResult.default().final_exponentiation() == b.Gt.identity()
    # group API: (g*a)*b == g*(a*b), Sum, batch_normalize
    gp = b.G1Projective.generator()
    assert (gp * a) * c == gp * (a * c)
    assert b.G1Projective.sum([gp, gp.double(), b.G1Projective.identity()]) == gp * b.Scalar(3)
    assert b.G1Projective.batch_normalize([gp, b.G1Projective.identity()])[1].is_identity()


def test_pairing_batch_large(ctx):
    """2^10 pairings: e([a_i]G1, [b_i]G2) all equal e(G1,G2)^(a_i b_i); checked via a product identity."""
    n = 1 << 10
    r = o.SplitMix64(777)
    a = [r.scalar() for _ in range(n)]
    bb = [r.scalar() for _ in range(n)]
    b1 = ctx.bases_from_scalars(1, a); b2 = ctx.bases_from_scalars(2, bb)
    g1, f1 = b1.download(); g2, f2 = b2.download()
    gt = ctx.pairing_batch(g1, f1, g2, f2)
    prod = ctx.fp12_product(gt)
    e = sum(x * y for x, y in zip(a, bb)) % o.R_ORDER
    assert np.array_equal(prod, fp12w(o.gt_mul_scalar(o.pairing(o.G1_GEN, o.G2_GEN), e)))
    for i in (0, 1, n - 1):
        assert np.array_equal(gt[i], fp12w(o.gt_mul_scalar(o.pairing(o.G1_GEN, o.G2_GEN), a[i] * bb[i] % o.R_ORDER)))


def test_cpp_host_mirror(ctx, kats, tmp_path):
    """include/bls12_381.hpp (C++ mirror of the reference API) compiled with g++ against libblsgpu.so and run."""
    import subprocess
    import bls12_381_amd as b
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "host_mirror_test")
    libdir = os.path.dirname(b.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "host_mirror_test.cpp"),
                           "-L" + libdir, "-lblsgpu", "-Wl,-rpath," + libdir, "-o", exe])
    kat = tmp_path / "gt.bin"
    kat.write_bytes(np.array(kats["consts"]["pairings.GT_GENERATOR"], dtype=np.uint64).tobytes())
    out = subprocess.run([exe, str(kat)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "host mirror ok" in out.stdout, out.stdout + out.stderr


# ---- batched (de)serialisation + validation ------------------------------------------------
@pytest.mark.parametrize("group", [1, 2])
def test_codec_golden_roundtrip(ctx, group, golden_dir):
    """All 1000 golden records of each file decode (checked and unchecked, both encodings) to k*G and re-encode
    to the same bytes; results equal the oracle's decoders."""
    name = "g1" if group == 1 else "g2"
    usz = 96 if group == 1 else 192
    unc = np.frombuffer(open(os.path.join(golden_dir, f"{name}_uncompressed_valid_test_vectors.dat"), "rb").read(), dtype=np.uint8).reshape(1000, usz)
    cmp_ = np.frombuffer(open(os.path.join(golden_dir, f"{name}_compressed_valid_test_vectors.dat"), "rb").read(), dtype=np.uint8).reshape(1000, usz // 2)
    xy_c, inf_c, ok_c = ctx.points_from_bytes(group, cmp_, compressed=True, checked=True)
    xy_u, inf_u, ok_u = ctx.points_from_bytes(group, unc, compressed=False, checked=True)
    assert ok_c.all() and ok_u.all()
    assert np.array_equal(xy_c, xy_u) and np.array_equal(inf_c, inf_u)
    assert inf_c[0] == 1 and not inf_c[1:].any()
    bases = ctx.bases_from_scalars(group, list(range(1000)))
    bxy, binf = bases.download()
    assert np.array_equal(bxy[1:], xy_c[1:]) and np.array_equal(binf, inf_c)
    assert np.array_equal(ctx.points_to_bytes(group, xy_c, inf_c, compressed=True), cmp_)
    assert np.array_equal(ctx.points_to_bytes(group, xy_c, inf_c, compressed=False), unc)
    xy_x, inf_x, ok_x = ctx.points_from_bytes(group, cmp_, compressed=True, checked=False)
    assert ok_x.all() and np.array_equal(xy_x, xy_c)


@pytest.mark.parametrize("group", [1, 2])
def test_codec_rejections(ctx, group, kats):
    """Every class of invalid encoding the reference rejects (flags, non-canonical coordinates, no square root,
    off-curve, off-subgroup), checked entry by entry against the oracle's decoders."""
    import bls12_381_amd as b
    r = o.SplitMix64(555 + group)
    if group == 1:
        enc_c, enc_u = o.g1_to_compressed, o.g1_to_uncompressed
        dec = {(True, True): o.g1_from_compressed, (True, False): o.g1_from_compressed_unchecked,
               (False, True): o.g1_from_uncompressed, (False, False): o.g1_from_uncompressed_unchecked}
        v = kats["tests"]["g1.test_is_torsion_free"]["fp"]
        off_sub = (o.fp_from_mont_limbs(v[0]), o.fp_from_mont_limbs(v[1]), False)
        pts = [o.g1_to_affine(o.g1_affine_mul(o.G1_GEN, r.scalar())) for _ in range(6)] + [o.G1_IDENTITY_AFF, off_sub]
        affw, csz = g1aff_w, 48
    else:
        enc_c, enc_u = o.g2_to_compressed, o.g2_to_uncompressed
        dec = {(True, True): o.g2_from_compressed, (True, False): o.g2_from_compressed_unchecked,
               (False, True): o.g2_from_uncompressed, (False, False): o.g2_from_uncompressed_unchecked}
        v = kats["tests"]["g2.test_is_torsion_free"]["fp"]
        F = o.fp_from_mont_limbs
        off_sub = ((F(v[0]), F(v[1])), (F(v[2]), F(v[3])), False)
        pts = [o.g2_to_affine(o.g2_affine_mul(o.G2_GEN, r.scalar())) for _ in range(6)] + [o.G2_IDENTITY_AFF, off_sub]
        affw, csz = g2aff_w, 96
    for compressed in (True, False):
        enc = enc_c if compressed else enc_u
        size = csz if compressed else 2 * csz
        cases = [enc(p) for p in pts]
        base = bytearray(cases[0])
        for flip in (0x80, 0x40, 0x20, 0xc0, 0xe0, 0x60):                  # flag combinations
            m = bytearray(base); m[0] ^= flip; cases.append(bytes(m))
        ident = bytearray(enc(pts[6]))
        m = bytearray(ident); m[size - 1] = 1; cases.append(bytes(m))      # infinity flag with non-zero coordinate
        m = bytearray(ident); m[0] |= 0x20; cases.append(bytes(m))         # infinity + sort flag
        pbytes = o.P.to_bytes(48, "big")
        m = bytearray(base); m[0:48] = bytes([pbytes[0] | (base[0] & 0xe0)]) + pbytes[1:]; cases.append(bytes(m))   # x = p (non-canonical)
        m = bytearray(base); m[size - 1] ^= 1; cases.append(bytes(m))      # perturbed: no sqrt / off-curve
        m = bytearray(base); m[size - 2] ^= 0x55; cases.append(bytes(m))
        m = bytearray(base); m[5] ^= 0x10; cases.append(bytes(m))
        for k in range(40):                                                # random x (about half have no root)
            m = bytearray(base)
            for j in range(1, 48):
                m[j] = r.next() & 0xff
            cases.append(bytes(m))
        data = np.frombuffer(b"".join(cases), dtype=np.uint8).reshape(len(cases), size)
        for checked in (True, False):
            xy, inf, ok = ctx.points_from_bytes(group, data, compressed=compressed, checked=checked)
            for i, c in enumerate(cases):
                want = dec[(compressed, checked)](c)
                assert bool(ok[i]) == (want is not None), (compressed, checked, i)
                if want is not None:
                    ex, ei = affw(want)
                    assert np.array_equal(xy[i], ex) and inf[i] == ei, (compressed, checked, i)
    cls = b.G1Affine if group == 1 else b.G2Affine
    assert cls.from_compressed(enc_c(pts[0])) == cls(*affw(pts[0]))
    assert cls.from_compressed(enc_c(off_sub)) is None and cls.from_compressed_unchecked(enc_c(off_sub)) is not None
    assert cls.from_uncompressed(enc_u(pts[1])) == cls(*affw(pts[1]))


@pytest.mark.parametrize("group,window", [(1, 0), (1, 12), (2, 16)])
def test_msm_precomputed_tables(ctx, group, window):
    """Resident window-shifted tables: same group element as the plain path and as the oracle (incl. edge scalars,
    identity bases, sub-ranges)."""
    r = o.SplitMix64(9000 + window)
    n = 3000
    rr = o.R_ORDER
    ks = [0, 1, 5, 5, rr - 5] + [r.scalar() for _ in range(n - 5)]
    ss = [7, rr - 1, 9, rr - 9, 9] + [r.scalar() for _ in range(n - 5)]
    ss[100] = 0; ss[101] = (1 << 254) + 12345; ss[102] = (1 << 20) - 1; ss[103] = 1 << 19
    bases = ctx.bases_from_scalars(group, ks)
    plain = ctx.msm(bases, ss)
    bases.precompute(window)
    pre = ctx.msm(bases, ss)
    a, ia = ctx.batch_normalize(group, plain[None, :]); b2, ib = ctx.batch_normalize(group, pre[None, :])
    assert np.array_equal(a, b2) and np.array_equal(ia, ib)
    tot = sum(k * s for k, s in zip(ks, ss)) % rr
    want = (o.g1_to_affine(o.g1_affine_mul(o.G1_GEN, tot)) if group == 1 else o.g2_to_affine(o.g2_affine_mul(o.G2_GEN, tot)))
    ex, ei = (g1aff_w if group == 1 else g2aff_w)(want)
    assert np.array_equal(b2[0], ex) and ib[0] == ei
    # sub-range of the resident tables
    sub = ctx.msm(bases, ss[500:1500], first=500)
    tot = sum(k * s for k, s in zip(ks[500:1500], ss[500:1500])) % rr
    want = (o.g1_to_affine(o.g1_affine_mul(o.G1_GEN, tot)) if group == 1 else o.g2_to_affine(o.g2_affine_mul(o.G2_GEN, tot)))
    ex, ei = (g1aff_w if group == 1 else g2aff_w)(want)
    sx, si = ctx.batch_normalize(group, sub[None, :])
    assert np.array_equal(sx[0], ex) and si[0] == ei


def test_msm_precomputed_tables_with_cut_buckets(ctx):
    """Resident tables put the entries of ALL windows into one bucket set, so its buckets are routinely cut into many work items: a
    small window with many points (2^17 points, 9-bit window: ~7 items per bucket) and the default window with heavily repeated
    scalars.  The accumulation grid must cover every item (round-4 review: it was sized for one window's entries) -- compared with
    the plain path and the discrete-log identity."""
    n = 1 << 17
    kb, ks = _rand_scalars_np(n, 4401)
    sb, ss = _rand_scalars_np(n, 4402)
    bases = ctx.bases_from_scalars(1, kb)
    plain = ctx.batch_normalize(1, ctx.msm(bases, sb)[None, :])
    tot = sum(k * s for k, s in zip(ks, ss)) % o.R_ORDER
    ex, ei = g1aff_w(o.g1_to_affine(o.g1_affine_mul(o.G1_GEN, tot)))
    assert np.array_equal(plain[0][0], ex) and plain[1][0] == ei
    rep = sb.copy(); rep[:] = sb[7]                                   # one scalar everywhere: 13 buckets hold everything
    rep[::1000] = sb[::1000]
    rs = [int.from_bytes(rep[i].tobytes(), "little") for i in range(n)]
    tot_rep = sum(k * s for k, s in zip(ks, rs)) % o.R_ORDER
    rx, ri = g1aff_w(o.g1_to_affine(o.g1_affine_mul(o.G1_GEN, tot_rep)))
    for window in (9, 12, 0):
        bases.precompute(window)
        got = ctx.batch_normalize(1, ctx.msm(bases, sb)[None, :])
        assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1]), window
        got = ctx.batch_normalize(1, ctx.msm(bases, rep)[None, :])
        assert np.array_equal(got[0][0], rx) and got[1][0] == ri, window


@pytest.mark.parametrize("group", [1, 2])
def test_batch_normalize_large(ctx, group):
    """`batch_normalize` over 10 000 points (the reference's 'batch to affine n=10000' bench point) incl. identities:
    Montgomery's-trick kernel == per-point inversion kernel == oracle on a sample."""
    n = 10000
    r = o.SplitMix64(31 + group)
    ks = [r.scalar() for _ in range(n)]
    for j in (0, 5, 4095, 4096, 9999):
        ks[j] = 0
    bases = ctx.bases_from_scalars(group, ks)
    xy, inf = bases.download()
    w = 6 if group == 1 else 12
    # build non-trivial projective representatives: (x*z : y*z : z) with z = x of another point
    z = np.roll(xy[:, :w], 1, axis=0).copy()
    z[np.roll(inf, 1) == 1] = xy[1, w:2 * w]           # the rolled-in neighbour was an identity (x = 0): use a non-zero z
    X = ctx.fp_op(0, xy[:, :6], z[:, :6]) if group == 1 else ctx.fp2_op(0, xy[:, :12], z)
    Y = ctx.fp_op(0, xy[:, 6:], z[:, :6]) if group == 1 else ctx.fp2_op(0, xy[:, 12:], z)
    z[inf == 1] = 0
    xyz = np.concatenate([X, Y, z], axis=1)
    big_xy, big_inf = ctx.batch_normalize(group, xyz)                       # n >= 4096: Montgomery's trick
    assert np.array_equal(big_inf, inf) and np.array_equal(big_xy[inf == 0], xy[inf == 0])
    small_xy, small_inf = ctx.batch_normalize(group, xyz[:3000])            # per-point inversion kernel
    assert np.array_equal(small_xy, big_xy[:3000]) and np.array_equal(small_inf, big_inf[:3000])
    ident = (np.concatenate([fpw(0), fpw(1)]) if group == 1 else np.concatenate([fp2w((0, 0)), fp2w((1, 0))]))
    assert np.array_equal(big_xy[0], ident)


# ---- multi-GPU logic as logical shards on one device (SURVEY.md 8e caveat) ------------------------------------------
@pytest.mark.parametrize("world", [2, 8])
def test_logical_shards_msm_and_miller(ctx, world):
    """The N-rank path (contiguous shards -> per-rank partial -> gather -> fold) executed as N logical ranks on one
    GPU gives the same element as the unsharded call: G1 MSM, G2 MSM and multi_miller_loop."""
    from bls12_381_amd.distributed import shard_range
    r = o.SplitMix64(1234 + world)
    n = 5000
    ks = [r.scalar() for _ in range(n)]
    ss = [r.scalar() for _ in range(n)]
    sb = np.stack([np.frombuffer(s.to_bytes(32, "little"), dtype=np.uint8) for s in ss])
    for group in (1, 2):
        bases = ctx.bases_from_scalars(group, ks)
        full = ctx.msm(bases, sb)
        parts = []
        for rank in range(world):
            lo, hi = shard_range(n, rank, world)
            parts.append(ctx.msm(bases, sb[lo:hi], first=lo))            # what rank `rank` would compute
        folded = ctx.point_sum(group, np.stack(parts))                     # what every rank does after the all-gather
        assert np.array_equal(ctx.batch_normalize(group, folded[None, :])[0], ctx.batch_normalize(group, full[None, :])[0])
    m = 64
    g1, f1 = ctx.bases_from_scalars(1, ks[:m]).download()
    g2, f2 = ctx.bases_from_scalars(2, ss[:m]).download()
    f1[3] = 1; f2[10] = 1                                                  # identities are skipped (pairings.rs:566-569)
    whole = ctx.multi_miller_loop(g1, f1, g2, f2)
    parts = []
    for rank in range(world):
        lo, hi = shard_range(m, rank, world)
        parts.append(ctx.multi_miller_loop(g1[lo:hi], f1[lo:hi], g2[lo:hi], f2[lo:hi]))
    assert np.array_equal(ctx.fp12_product(np.stack(parts)), whole)
    assert np.array_equal(ctx.final_exponentiation_batch(whole[None, :])[0],
                          ctx.final_exponentiation_batch(ctx.fp12_product(np.stack(parts))[None, :])[0])


# ---- scalar field Fr and its transform (reference src/scalar.rs) --------------------------
def frw(x):
    return np.array(o.fr_to_mont_limbs(x), dtype=np.uint64)


def frs(a):
    return [o.fr_from_mont_limbs(row) for row in a]


EDGE_FR = [0, 1, 2, o.R_ORDER - 1, o.R_ORDER - 2, (o.R_ORDER - 1) // 2, (1 << 254), (1 << 64) - 1, 7, o.FR_ROOT_OF_UNITY]


def test_fr_ops(ctx, kats):
    r = o.SplitMix64(0xF2)
    a = EDGE_FR + [r.scalar() for _ in range(2000)]
    b = list(reversed(EDGE_FR)) + [r.scalar() for _ in range(2000)]
    A, B = np.stack([frw(x) for x in a]), np.stack([frw(x) for x in b])
    for op, fn in [(0, o.fr_mul), (1, o.fr_add), (2, o.fr_sub)]:
        assert np.array_equal(ctx.fr_op(op, A, B), np.stack([frw(fn(x, y)) for x, y in zip(a, b)])), f"fr op {op}"
    assert np.array_equal(ctx.fr_op(3, A), np.stack([frw(o.fr_sqr(x)) for x in a]))
    assert np.array_equal(ctx.fr_op(5, A), np.stack([frw(o.fr_neg(x)) for x in a]))
    assert np.array_equal(ctx.fr_op(6, A), np.stack([frw(o.fr_double(x)) for x in a]))
    inv, some = ctx.fr_op(4, A[:300], return_flags=True)
    assert np.array_equal(inv, np.stack([frw(o.fr_inv(x) or 0) for x in a[:300]]))
    assert list(some) == [0 if x == 0 else 1 for x in a[:300]]          # CtOption::none exactly for zero (scalar.rs:573-628)
    # the reference's stored limb patterns go through unchanged: R2 * R2 = R3 * R ... (R2 limbs = value 2^256)
    c = kats["consts"]
    R2 = np.array([c["scalar.R2"]], dtype=np.uint64)
    assert np.array_equal(ctx.fr_op(0, R2, R2)[0], np.array(c["scalar.R3"], dtype=np.uint64))
    root, root_inv = np.array([c["scalar.ROOT_OF_UNITY"]], dtype=np.uint64), np.array([c["scalar.ROOT_OF_UNITY_INV"]], dtype=np.uint64)
    assert np.array_equal(ctx.fr_op(0, root, root_inv)[0], np.array(c["scalar.R"], dtype=np.uint64))
    assert np.array_equal(ctx.fr_op(4, root)[0], root_inv[0])


# the reference's own byte vectors of scalar.rs:864-1040 (test_to_bytes / test_from_bytes / test_from_bytes_wide_*): data, cited
SCALAR_R2_BYTES = bytes([254, 255, 255, 255, 1, 0, 0, 0, 2, 72, 3, 0, 250, 183, 132, 88, 245, 79, 188, 236, 239, 79, 140, 153, 111, 5, 197, 172, 89, 177, 36, 24])
SCALAR_NEG1_BYTES = bytes([0, 0, 0, 0, 255, 255, 255, 255, 254, 91, 254, 255, 2, 164, 189, 83, 5, 216, 161, 9, 8, 216, 57, 51, 72, 125, 157, 41, 83, 167, 237, 115])


def test_scalar_bytes_conversions_vs_oracle_and_reference_kats(ctx, kats):
    """SURVEY.md 8 row a8 on the device: `Scalar::to_bytes` (scalar.rs:284-296), `from_bytes` (:256-280), `from_bytes_wide` (:300-331)
    over vectors -- the reference's own known answers (scalar.rs:864-1040), the edge values 0, 1, r - 1, `from_bytes_wide(&[0xff; 64])`,
    non-canonical inputs, and 4 000 random elements against the limb-level restatement in the oracle"""
    c = kats["consts"]
    u = lambda name: np.array(c[name], dtype=np.uint64)
    # to_bytes: zero, one (= R limbs), R2, -1
    neg1 = frw(o.R_ORDER - 1)
    got, ok = ctx.fr_to_bytes(np.stack([np.zeros(4, dtype=np.uint64), u("scalar.R"), u("scalar.R2"), neg1]), return_flags=True)
    assert bytes(got[0]) == bytes(32) and bytes(got[1]) == (1).to_bytes(32, "little")
    assert bytes(got[2]) == SCALAR_R2_BYTES and bytes(got[3]) == SCALAR_NEG1_BYTES and list(ok) == [1, 1, 1, 1]
    # from_bytes: the same four back, then the reference's rejections (modulus, modulus + 1, a higher byte bumped twice)
    mod = bytearray(SCALAR_NEG1_BYTES); mod[0] = 1
    bad2 = bytearray(mod); bad2[0] = 2
    bad3 = bytearray(mod); bad3[22] = 58
    bad4 = bytearray(mod); bad4[31] = 116
    rows = [bytes(32), (1).to_bytes(32, "little"), SCALAR_R2_BYTES, SCALAR_NEG1_BYTES, bytes(mod), bytes(bad2), bytes(bad3), bytes(bad4)]
    limbs, some = ctx.fr_from_bytes(np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(-1, 32))
    assert list(some) == [1, 1, 1, 1, 0, 0, 0, 0]
    assert not limbs[0].any() and np.array_equal(limbs[1], u("scalar.R")) and np.array_equal(limbs[2], u("scalar.R2")) and np.array_equal(limbs[3], neg1)
    for i in range(4, 8):                        # the value is computed either way (tmp * R2), exactly as the reference computes it before CtOption masks it
        assert [int(x) for x in limbs[i]] == o.scalar_limbs_from_bytes(rows[i])[0]
    # from_bytes_wide: from_u512 KATs (modulus|0 -> 0, 1 -> R, 2^256 -> R2, max -> R3 - R), R2 / -1 padded, and the stored maximum
    wide = [o.R_ORDER.to_bytes(32, "little") + bytes(32), (1).to_bytes(64, "little"), bytes(32) + (1).to_bytes(32, "little"), b"\xff" * 64,
            SCALAR_R2_BYTES + bytes(32), SCALAR_NEG1_BYTES + bytes(32)]
    w = ctx.fr_from_bytes_wide(np.frombuffer(b"".join(wide), dtype=np.uint8).reshape(-1, 64))
    r3_minus_r = ctx.fr_op(2, u("scalar.R3")[None, :], u("scalar.R")[None, :])[0]
    assert not w[0].any() and np.array_equal(w[1], u("scalar.R")) and np.array_equal(w[2], u("scalar.R2")) and np.array_equal(w[3], r3_minus_r)
    assert np.array_equal(w[3], u("scalar.FROM_BYTES_WIDE_MAXIMUM")) and np.array_equal(w[4], u("scalar.R2")) and np.array_equal(w[5], neg1)
    # random elements and raw 256- / 512-bit strings against the oracle's limb-level restatement
    r = o.SplitMix64(0xA8)
    vals = EDGE_FR + [r.scalar() for _ in range(4000)]
    L = np.stack([frw(v) for v in vals])
    B = ctx.fr_to_bytes(L)
    assert [bytes(row) for row in B] == [o.scalar_limbs_to_bytes([int(x) for x in row]) for row in L] == [v.to_bytes(32, "little") for v in vals]
    back, some = ctx.fr_from_bytes(B)
    assert np.array_equal(back, L) and some.all()
    raw = np.random.RandomState(8).randint(0, 256, size=(2000, 64), dtype=np.uint8)
    raw[0] = 0; raw[1] = 255
    W = ctx.fr_from_bytes_wide(raw)
    assert [[int(x) for x in row] for row in W] == [o.scalar_limbs_from_bytes_wide(bytes(row)) for row in raw]
    lim2, some2 = ctx.fr_from_bytes(raw[:, :32].copy())
    want2 = [o.scalar_limbs_from_bytes(bytes(row[:32])) for row in raw]
    assert [[int(x) for x in row] for row in lim2] == [w_[0] for w_ in want2] and [bool(x) for x in some2] == [w_[1] for w_ in want2]
    # limbs that no `Scalar` holds (>= r): flagged by to_bytes
    _, okb = ctx.fr_to_bytes(np.stack([np.array(o.FR_MODULUS_LIMBS, dtype=np.uint64), np.full(4, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64), neg1]), return_flags=True)
    assert list(okb) == [0, 0, 1]


@pytest.mark.parametrize("group", [1, 2])
def test_msm_and_mul_batch_take_scalar_limbs(ctx, group):
    """`msm(&[G1Affine], &[Scalar])` with the scalars as `&[Scalar]` memory (Montgomery limbs, blsgpu_g{1,2}_msm_mont): the same point as the
    byte-form call and as the oracle's discrete-log identity, on the endomorphism path, on plain windows (BLSGPU_NO_GLV) and through
    mul_batch; scalars 0, 1, r - 1 included; limbs >= r are reported like non-canonical bytes"""
    import ctypes
    import bls12_381_amd as b
    r = o.SplitMix64(0xA80 + group)
    n = 777
    ks = [r.scalar() for _ in range(n)]
    ss = [0, 1, o.R_ORDER - 1, o.R_ORDER - 2] + [r.scalar() for _ in range(n - 4)]
    L = np.stack([frw(v) for v in ss])
    tot = sum(k * s for k, s in zip(ks, ss)) % o.R_ORDER
    if group == 1:
        want = o.g1_to_uncompressed(o.g1_to_affine(o.g1_affine_mul(o.G1_GEN, tot))); Aff = b.G1Affine
    else:
        want = o.g2_to_uncompressed(o.g2_to_affine(o.g2_affine_mul(o.G2_GEN, tot))); Aff = b.G2Affine
    made = [ctx]
    os.environ["BLSGPU_NO_GLV"] = "1"
    try:
        made.append(b.Context(0))
    finally:
        os.environ.pop("BLSGPU_NO_GLV")
    try:
        for cx in made:
            bases = cx.bases_from_scalars(group, ks)
            for w in (0, 9, 16):
                cx.set_msm_window(w)
                xy, inf = cx.batch_normalize(group, cx.msm_mont(bases, L)[None, :])
                assert Aff(xy[0], bool(inf[0])).to_uncompressed() == want, (cx is ctx, w)
            cx.set_msm_window(0)
            # the context-wide setting reaches the plain entry points (here: msm_many through the byte-typed signature)
            cx.set_scalar_form(b.api.SCALAR_MONT)
            try:
                out = cx.msm_many(bases, L.view(np.uint8).reshape(1, n, 32))
            finally:
                cx.set_scalar_form(b.api.SCALAR_BYTES)
            xy, inf = cx.batch_normalize(group, out)
            assert Aff(xy[0], bool(inf[0])).to_uncompressed() == want
            # limbs >= r: reported, and the flag does not stick
            Lb = L.copy(); Lb[5] = np.array(o.FR_MODULUS_LIMBS, dtype=np.uint64)
            with pytest.raises(b.BlsGpuError, match="canonical"):
                cx.msm_mont(bases, Lb)
            cx.msm_mont(bases, L)
            bases.free()
    finally:
        made[1].close()
    # mul_batch: n independent products, bytes vs limbs vs the oracle (first 24 through tier-1 multiply), also on the vouched fast path
    m = 300
    bases = ctx.bases_from_scalars(group, ks[:m])
    xy, inf = bases.download()
    via_bytes = ctx.batch_normalize(group, ctx.mul_batch(group, xy, inf, ss[:m]))
    via_limbs = ctx.batch_normalize(group, ctx.mul_batch_mont(group, xy, inf, L[:m]))
    assert np.array_equal(via_bytes[0], via_limbs[0]) and np.array_equal(via_bytes[1], via_limbs[1])
    fast = b.Context(0)
    try:
        fast.set_assume_subgroup(True)
        via_fast = fast.batch_normalize(group, fast.mul_batch_mont(group, xy, inf, L[:m]))
    finally:
        fast.close()
    assert np.array_equal(via_bytes[0], via_fast[0]) and np.array_equal(via_bytes[1], via_fast[1])
    gen, amul, toaff, enc = (o.G1_GEN, o.g1_affine_mul, o.g1_to_affine, o.g1_to_uncompressed) if group == 1 else (o.G2_GEN, o.g2_affine_mul, o.g2_to_affine, o.g2_to_uncompressed)
    for i in range(24):
        assert Aff(via_limbs[0][i], bool(via_limbs[1][i])).to_uncompressed() == enc(toaff(amul(gen, ks[i] * ss[i] % o.R_ORDER)))
    bases.free()


def test_transform_feeds_msm_on_the_device_without_a_host_copy(ctx):
    """the chain row f3 exists for: blsgpu_fr_ntt_device -> blsgpu_g1_msm_mont_device on the same device buffer (no conversion kernel, no
    host round trip), against the oracle: MSM(NTT(x), [k_i] G) = [sum_j NTT(x)_j k_j] G.  Also blsgpu_fr_to_bytes_device -> the byte-form MSM,
    and `Gt * Scalar` with limbs"""
    import torch
    import bls12_381_amd as b
    log_n = 10
    n = 1 << log_n
    r = o.SplitMix64(0xA8C)
    x = [r.scalar() for _ in range(n)]
    ks = [r.scalar() for _ in range(n)]
    y = o.fr_ntt(x)
    tot = sum(k * s for k, s in zip(ks, y)) % o.R_ORDER
    want = o.g1_to_uncompressed(o.g1_to_affine(o.g1_affine_mul(o.G1_GEN, tot)))
    dev = torch.device("cuda", 0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        bases = ctx.bases_from_scalars(1, ks)
        d_x = torch.from_numpy(np.stack([frw(v) for v in x]).view(np.int64)).to(dev)
        d_out = torch.zeros(18, dtype=torch.int64, device=dev)
        ctx.fr_ntt_device(d_x.data_ptr(), log_n)
        ctx.msm_mont_device(bases, d_x.data_ptr(), n, d_out.data_ptr())
        d_bytes = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
        d_out2 = torch.zeros(18, dtype=torch.int64, device=dev)
        ctx.fr_to_bytes_device(d_x.data_ptr(), n, d_bytes.data_ptr())
        ctx.msm_device(bases, d_bytes.data_ptr(), n, d_out2.data_ptr())
        ctx.synchronize()
        for d in (d_out, d_out2):
            xy, inf = ctx.batch_normalize(1, d.cpu().numpy().view(np.uint64)[None, :])
            assert b.G1Affine(xy[0], bool(inf[0])).to_uncompressed() == want
        assert [bytes(row) for row in d_bytes.cpu().numpy()] == [v.to_bytes(32, "little") for v in y]
        # Gt * Scalar with limbs: e(G1, G2)^s for s as bytes and as limbs
        gt = b.pairing(b.G1Affine.generator(), b.G2Affine.generator()).f
        svals = [1, 2, o.R_ORDER - 1, y[3]]
        G = np.tile(gt, (len(svals), 1))
        by_bytes = ctx.gt_mul_scalar_batch(G, svals)
        d_g = torch.from_numpy(G.view(np.int64)).to(dev); d_s = torch.from_numpy(np.stack([frw(v) for v in svals]).view(np.int64)).to(dev)
        d_o = torch.zeros((len(svals), 72), dtype=torch.int64, device=dev)
        ctx.set_scalar_form(b.api.SCALAR_MONT)
        try:
            ctx.gt_mul_scalar_batch_device(d_g.data_ptr(), d_s.data_ptr(), len(svals), d_o.data_ptr())
            ctx.synchronize()
        finally:
            ctx.set_scalar_form(b.api.SCALAR_BYTES)
        assert np.array_equal(d_o.cpu().numpy().view(np.uint64), by_bytes)
        bases.free()
    finally:
        ctx.set_stream(None)


@pytest.mark.parametrize("log_n", [0, 1, 2, 3, 5, 9, 10, 11, 12, 13])
def test_fr_ntt_vs_oracle(ctx, log_n):
    n = 1 << log_n
    r = o.SplitMix64(1000 + log_n)
    x = [r.scalar() for _ in range(n)]
    if n >= 4:
        x[0], x[1], x[2] = 0, o.R_ORDER - 1, 1
    X = np.stack([frw(v) for v in x])
    Y = ctx.fr_ntt(X)
    assert frs(Y) == o.fr_ntt(x)
    assert np.array_equal(ctx.fr_ntt(Y, inverse=True), X)
    assert frs(ctx.fr_ntt(X, inverse=True)) == o.fr_ntt(x, inverse=True)


@pytest.mark.parametrize("log_n", [11, 13, 14, 17, 20, 21, 22, 23])
def test_fr_ntt_column_tiles_equal_stage_passes(log_n):
    """round 5: from 2^20 elements the top stages run on column tiles in LDS (k_fr_cols: up to seven stages per pass).  A context that
    uses them at EVERY size (BLSGPU_NTT_IMPL=cols) against one that never does (=stage: the passes of rounds 2-4, which the oracle pins
    at 2^0 .. 2^13): canonical outputs limb-identical in both directions, odd and even depths, one to four column passes; the
    2^11 / 2^13 results also against the oracle, sampled outputs of 2^14 against the defining sum; two other tile shapes at 2^20"""
    import bls12_381_amd as bls
    n = 1 << log_n
    rs = np.random.RandomState(50 + log_n)
    raw = rs.randint(0, 256, size=(n, 32), dtype=np.uint8); raw[:, 31] &= 0x3F
    X = raw.view(np.uint64).reshape(n, 4).copy()
    X[0] = 0; X[1] = frw(o.R_ORDER - 1)
    made = []
    for impl in ("cols", "stage"):
        os.environ["BLSGPU_NTT_IMPL"] = impl
        try:
            made.append(bls.Context(0))
        finally:
            os.environ.pop("BLSGPU_NTT_IMPL")
    new, old = made
    try:
        Y, Yo = new.fr_ntt(X), old.fr_ntt(X)
        assert np.array_equal(Y, Yo)
        assert np.array_equal(new.fr_ntt(Y, inverse=True), X)
        assert np.array_equal(new.fr_ntt(X, inverse=True), old.fr_ntt(X, inverse=True))
        if log_n == 20:
            for shape in ("12,10,1024", "10,3,256"):           # (the switches are read when a context is created: csrc/diag.h)
                os.environ["BLSGPU_NTT_COLS"] = shape; os.environ["BLSGPU_NTT_IMPL"] = "cols"
                try:
                    shaped = bls.Context(0)
                finally:
                    os.environ.pop("BLSGPU_NTT_COLS"); os.environ.pop("BLSGPU_NTT_IMPL")
                try:
                    assert np.array_equal(shaped.fr_ntt(X), Yo), shape
                finally:
                    shaped.close()
    finally:
        new.close(); old.close()
    if log_n <= 13:
        assert frs(Y) == o.fr_ntt([o.fr_from_mont_limbs(v) for v in X])
    if log_n == 14:
        w = o.fr_omega(log_n)
        xs = [o.fr_from_mont_limbs(X[j]) for j in range(n)]
        for k in (1, 4097, n - 1):
            wk = pow(w, k, o.R_ORDER)
            acc, t = 0, 1
            for j in range(n):
                acc += xs[j] * t
                t = t * wk % o.R_ORDER
            assert o.fr_from_mont_limbs(Y[k]) == acc % o.R_ORDER


def test_fr_ntt_large_properties(ctx):
    """2^20 scalars (the MSM's scalar vector at the headline size): round trip, linearity, sampled outputs against the
    defining sum, and the convolution theorem on a sparse product."""
    log_n = 20
    n = 1 << log_n
    rs = np.random.RandomState(5)
    raw = rs.randint(0, 256, size=(n, 32), dtype=np.uint8); raw[:, 31] &= 0x3F                  # < 2^254 < r: canonical limbs
    X = raw.view(np.uint64).reshape(n, 4).copy()
    Y = ctx.fr_ntt(X)
    assert np.array_equal(ctx.fr_ntt(Y, inverse=True), X)
    # sampled outputs: y_k = sum_j x_j w^(jk) with x_j = limbs interpreted through the Montgomery map
    w = o.fr_omega(log_n)
    rinv = pow(o.FR_MONT_R, -1, o.R_ORDER)
    xs = [int.from_bytes(raw[j].tobytes(), "little") for j in range(n)]                          # raw limb integers = x_j * R
    for k in (0, 1, n // 2, 777777):
        wk = pow(w, k, o.R_ORDER)
        acc, t = 0, 1
        for j in range(n):
            acc += xs[j] * t
            t = t * wk % o.R_ORDER
        assert o.fr_from_mont_limbs(Y[k]) == acc * rinv % o.R_ORDER
    # linearity: NTT(x + x') = NTT(x) + NTT(x')
    X2 = np.roll(X, 12345, axis=0)
    assert np.array_equal(ctx.fr_ntt(ctx.fr_op(1, X, X2)), ctx.fr_op(1, Y, ctx.fr_ntt(X2)))
    # convolution theorem: multiplying by the monomial z^s in the coefficient domain = pointwise w^(ks)
    s = 3
    mono = np.zeros((n, 4), dtype=np.uint64); mono[s] = frw(1)
    M = ctx.fr_ntt(mono)
    prod = ctx.fr_ntt(ctx.fr_op(0, Y, M), inverse=True)
    assert np.array_equal(prod, np.roll(X, s, axis=0))                                          # cyclic shift by s


# ---- hash-to-curve (reference src/hash_to_curve/) --------------------------------------------------
def _h2c_vectors(golden_dir):
    import json
    return json.load(open(os.path.join(golden_dir, "h2c_vectors.json")))


@pytest.mark.parametrize("group", [1, 2])
def test_hash_to_curve_rfc_vectors(ctx, golden_dir, group):
    """the RFC 9380 (draft-16) vectors of the reference's tests/hash_to_curve_g{1,2}.rs, compared on uncompressed bytes"""
    import bls12_381_amd as b
    vecs = _h2c_vectors(golden_dir)["g1" if group == 1 else "g2"]
    for encode in (False, True):
        sel = [t for t in vecs if t["test"].endswith("_nu") == encode]
        assert len(sel) == 5
        dst = bytes.fromhex(sel[0]["dst"])
        G = b.G1Projective if group == 1 else b.G2Projective                     # the mirror's reference-style entry points
        single = (G.encode_to_curve if encode else G.hash_to_curve)(bytes.fromhex(sel[1]["msg"]), dst)
        assert single.to_affine().to_uncompressed().hex() == sel[1]["out"]
        out = ctx.hash_to_curve(group, [bytes.fromhex(t["msg"]) for t in sel], dst, encode_only=encode)
        xy, inf = ctx.batch_normalize(group, out)
        for k, t in enumerate(sel):
            pt = (b.G1Affine if group == 1 else b.G2Affine)(xy[k], bool(inf[k]))
            assert pt.to_uncompressed().hex() == t["out"], (group, encode, k)


def test_expanders_reference_vectors_and_oracle(ctx, golden_dir):
    """the reference's expander vectors (tests/expand_msg.rs: XMD over SHA-256 with short and long DST and over SHA-512, XOF over SHAKE128 with
    short and long DST and over SHAKE256 -- 60 cases) through blsgpu_expand_message_batch, then random messages / lengths / DSTs against the
    oracle (hashlib digests); `HashToField for Scalar` on the reference's stored answers (map_scalar.rs:27-45) and against the oracle"""
    import bls12_381_amd as b
    from oracle import h2c_ref as h
    A = b.api
    vecs = _h2c_vectors(golden_dir)["expand_msg"]
    assert len(vecs) == 60
    ex_of = lambda name: A.EXPAND_XMD_SHA512 if "sha512" in name else A.EXPAND_XMD_SHA256 if "sha256" in name else A.EXPAND_XOF_SHAKE128 if "shake128" in name else A.EXPAND_XOF_SHAKE256
    by_call = {}
    for t in vecs:
        by_call.setdefault((ex_of(t["test"]), t["dst"], t["len_in_bytes"]), []).append(t)
    for (ex, dst, ln), ts in by_call.items():
        got = ctx.expand_message(ex, [bytes.fromhex(t["msg"]) for t in ts], bytes.fromhex(dst), ln)
        for k, t in enumerate(ts):
            assert bytes(got[k]).hex() == t["out"], (t["test"], k)
    assert {k[0] for k in by_call} == {0, 1, 2, 3}
    r = o.SplitMix64(0xE7)
    msgs = [b"", b"a", bytes(111), bytes(112), bytes(127), bytes(128), bytes(135), bytes(136), bytes(137), bytes(167), bytes(168), bytes(169), bytes(range(256)) * 3] + \
           [bytes((r.next() >> 8) & 0xFF for _ in range(int(r.next() % 400))) for _ in range(20)]
    for ex in (A.EXPAND_XMD_SHA256, A.EXPAND_XMD_SHA512, A.EXPAND_XOF_SHAKE128, A.EXPAND_XOF_SHAKE256):
        for dst in (b"QUUX-V01-CS02", b"", b"x" * 255, b"long-dst-" * 40):
            for ln in (1, 31, 32, 33, 48, 64, 96, 128, 135, 136, 137, 168, 169, 256, 500):
                got = ctx.expand_message(ex, msgs if ln in (48, 128, 500) else msgs[:4], dst, ln)
                for k in range(got.shape[0]):
                    assert bytes(got[k]) == h.expand_message(ex, msgs[k], dst, ln), (ex, len(dst), ln, k)
    # limits the reference enforces by panicking
    with pytest.raises(b.BlsGpuError):
        ctx.expand_message(A.EXPAND_XMD_SHA256, [b"m"], b"d", 255 * 32 + 1)
    with pytest.raises(b.BlsGpuError):
        ctx.expand_message(4, [b"m"], b"d", 32)
    assert bytes(ctx.expand_message(A.EXPAND_XMD_SHA256, [b"m"], b"d", 255 * 32)[0]) == h.expand_message(0, b"m", b"d", 255 * 32)
    assert bytes(ctx.expand_message(A.EXPAND_XOF_SHAKE256, [b"m"], b"d", 65535)[0]) == h.expand_message(3, b"m", b"d", 65535)
    # Scalar::from_okm on the stored answers: hash_to_scalar's second stage (k_hash_to_scalar) is fed directly through expand -> identity check below
    for ex in (0, 1, 2, 3):
        for dst in (b"BLS12381-scalar-suite", b"y" * 300):
            for count in (1, 2, 5):
                got = ctx.hash_to_scalar(ex, msgs[:12], dst, count)
                for k in range(12):
                    want = h.hash_to_field_scalar(msgs[k], dst, count, ex)
                    assert [o.fr_from_mont_limbs(row) for row in got[k]] == want, (ex, count, k)
    for t in _h2c_vectors(golden_dir)["hash_to_scalar"]:
        assert "%064x" % h.scalar_from_okm(bytes.fromhex(t["okm"])) == t["out"]


@pytest.mark.parametrize("group", [1, 2])
def test_hash_to_curve_with_every_expander(ctx, group):
    """`hash_to_curve::<X>` / `encode_to_curve::<X>` for the four expanders the reference tests: XMD:SHA-256 through the uniform-bytes path must give
    the very limbs of the fused kernel (and so the RFC vectors); the others are compared with the oracle on the projective coordinates"""
    import bls12_381_amd as b
    from oracle import h2c_ref as h
    A = b.api
    r = o.SplitMix64(0xE8 + group)
    msgs = [b"", b"abc", bytes(200)] + [bytes((r.next() >> 8) & 0xFF for _ in range(int(r.next() % 150))) for _ in range(9)]
    for dst in (b"QUUX-V01-CS02-with-BLS12381G%d_XOF:SHAKE-256_SSWU_RO_" % group, b"z" * 300):
        for encode in (False, True):
            fused = ctx.hash_to_curve(group, msgs, dst, encode_only=encode)
            assert np.array_equal(ctx.hash_to_curve_expander(group, A.EXPAND_XMD_SHA256, msgs, dst, encode_only=encode), fused)
            for ex in (A.EXPAND_XMD_SHA512, A.EXPAND_XOF_SHAKE128, A.EXPAND_XOF_SHAKE256):
                out = ctx.hash_to_curve_expander(group, ex, msgs, dst, encode_only=encode)
                for k, m in enumerate(msgs[:6] if len(dst) > 255 else msgs):
                    if group == 1:
                        want = np.concatenate([fpw(c) for c in (h.g1_encode_to_curve if encode else h.g1_hash_to_curve)(m, dst, ex)])
                    else:
                        want = np.concatenate([fp2w(c) for c in (h.g2_encode_to_curve if encode else h.g2_hash_to_curve)(m, dst, ex)])
                    assert np.array_equal(out[k], want), (group, ex, encode, k)
    with pytest.raises(b.BlsGpuError):
        ctx.hash_to_curve_expander(group, 7, msgs, b"d")


@pytest.mark.parametrize("group", [1, 2])
def test_hash_to_curve_from_uniform_bytes_and_degenerate_field_elements(ctx, group):
    """the part of hash_to_curve behind the expander (mod.rs:86-108: from_okm, map_to_curve twice, sum, clear_h) on caller-supplied uniform bytes:
    (a) with the bytes of expand_message it gives the limbs of hash_to_curve itself; (b) field elements no hash will ever produce -- 0, 1, u, -1,
    equal pairs -- against the oracle's restatement of the reference's formulas on the projective coordinates.  The bulk G2 form finds the square
    root of the map by another method than the reference (h2c_sswu_g2_dual): (b) is where its degenerate branches (u = 0: gx1_num = 0, y = 0,
    x = x1) are exercised."""
    import bls12_381_amd as b
    from oracle import h2c_ref as h
    A = b.api
    M = 1 if group == 1 else 2
    msgs = [b"", b"abc", bytes(77), b"q" * 130]
    dst = b"QUUX-V01-CS02-with-BLS12381G%d_XMD:SHA-256_SSWU_RO_" % group
    for encode in (False, True):
        per = (1 if encode else 2) * M * 64
        uni = ctx.expand_message(A.EXPAND_XMD_SHA256, msgs, dst, per)
        assert np.array_equal(ctx.hash_to_curve_from_uniform(group, uni, encode_only=encode), ctx.hash_to_curve(group, msgs, dst, encode_only=encode))
    # (b) chosen field elements: okm = db * 2^256 + da (map_g1.rs:513-531), so a value v < p is the 64 bytes of v itself
    okm = lambda v: int(v).to_bytes(64, "big")

    def same(got, want_limbs, want_pt):
        """exact projective limbs -- except for the identity (u1 = -u0 maps to P and -P): the reference's `double` returns the literal (0 : 1 : 0) for an
        identity input (g1.rs:666, g2.rs:737) where the kernels let the formula run, so the Y of an identity result differs; the point does not"""
        z = want_pt[2]
        if z == 0 or z == (0, 0):
            n = len(got) // 3
            return (not got[:n].any()) and got[n:2 * n].any() and (not got[2 * n:].any())
        return np.array_equal(got, want_limbs)
    r = o.SplitMix64(0x51 + group)
    big = lambda: r.scalar() * r.scalar() % o.P
    if group == 1:
        vals = [0, 1, o.P - 1, 2, 5, big(), big()]
        pairs = [(0, 0), (0, 1), (1, 0), (1, 1), (o.P - 1, 1), (2, 5), (vals[5], vals[5]), (vals[5], vals[6]), (0, vals[6])]
        uni = np.frombuffer(b"".join(okm(a) + okm(c) for a, c in pairs), dtype=np.uint8).reshape(len(pairs), 128)
        out = ctx.hash_to_curve_from_uniform(1, uni)
        for k, (a, c) in enumerate(pairs):
            want = h.g1_clear_cofactor(o.g1_add(h.g1_map_to_curve(a), h.g1_map_to_curve(c)))
            assert same(out[k], np.concatenate([fpw(x) for x in want]), want), (k, a, c)
        enc = ctx.hash_to_curve_from_uniform(1, np.frombuffer(b"".join(okm(v) for v in vals), dtype=np.uint8).reshape(len(vals), 64), encode_only=True)
        for k, v in enumerate(vals):
            assert np.array_equal(enc[k], np.concatenate([fpw(x) for x in h.g1_clear_cofactor(h.g1_map_to_curve(v))])), (k, v)
    else:
        vals = [(0, 0), (1, 0), (0, 1), (o.P - 1, 0), (0, o.P - 1), (1, 1), (2, 0), (big(), big()), (big(), 0), (0, big()), (big(), big())]
        pairs = [(vals[0], vals[0]), (vals[0], vals[1]), (vals[1], vals[0]), (vals[2], vals[3]), (vals[4], vals[5]), (vals[7], vals[7]), (vals[7], vals[10]),
                 (vals[8], vals[9]), (vals[6], vals[0]), (vals[10], vals[1])]
        enc2 = lambda u: okm(u[0]) + okm(u[1])
        uni = np.frombuffer(b"".join(enc2(a) + enc2(c) for a, c in pairs), dtype=np.uint8).reshape(len(pairs), 256)
        out = ctx.hash_to_curve_from_uniform(2, uni)
        for k, (a, c) in enumerate(pairs):
            want = h.g2_clear_cofactor(o.g2_add(h.g2_map_to_curve(a), h.g2_map_to_curve(c)))
            assert same(out[k], np.concatenate([fp2w(x) for x in want]), want), (k, a, c)
        enc = ctx.hash_to_curve_from_uniform(2, np.frombuffer(b"".join(enc2(v) for v in vals), dtype=np.uint8).reshape(len(vals), 128), encode_only=True)
        for k, v in enumerate(vals):
            assert np.array_equal(enc[k], np.concatenate([fp2w(x) for x in h.g2_clear_cofactor(h.g2_map_to_curve(v))])), (k, v)
    assert ctx.hash_to_curve_from_uniform(group, np.zeros((0, 128 * M), dtype=np.uint8)).shape[0] == 0
    with pytest.raises(b.BlsGpuError):
        b._lib.check(ctx.lib.blsgpu_hash_to_curve_from_uniform_batch(ctx.h, 3, None, 1, 0, None), "group")


@pytest.mark.parametrize("group", [1, 2])
def test_hash_to_curve_vs_oracle(ctx, group):
    """random and edge-case messages / DSTs against the oracle, on the PROJECTIVE coordinates (the kernels follow the
    reference's formulas step for step), plus subgroup membership of the results"""
    from oracle import h2c_ref as h
    r = o.SplitMix64(31 + group)
    msgs = [b"", b"a", bytes(55), bytes(56), bytes(63), bytes(64), bytes(65), bytes(range(256)) * 3] + \
           [bytes((r.next() >> 8) & 0xFF for _ in range(int(r.next() % 200))) for _ in range(24)]
    for dst in (b"QUUX-V01-CS02-with-BLS12381G%d_XMD:SHA-256_SSWU_RO_" % group, b"", b"x" * 255, b"long-dst-" * 40):
        for encode in (False, True):
            out = ctx.hash_to_curve(group, msgs, dst, encode_only=encode)
            for k, m in enumerate(msgs if dst.startswith(b"QUUX") else msgs[:6]):
                if group == 1:
                    p = (h.g1_encode_to_curve if encode else h.g1_hash_to_curve)(m, dst)
                    want = np.concatenate([fpw(c) for c in p])
                else:
                    p = (h.g2_encode_to_curve if encode else h.g2_hash_to_curve)(m, dst)
                    want = np.concatenate([fp2w(c) for c in p])
                assert np.array_equal(out[k], want), (group, len(dst), encode, k)
    # results are in the prime-order subgroup: the checked decoder accepts their encodings
    out = ctx.hash_to_curve(group, msgs, b"subgroup-check")
    xy, inf = ctx.batch_normalize(group, out)
    enc = ctx.points_to_bytes(group, xy, inf, compressed=True)
    _, _, ok = ctx.points_from_bytes(group, enc, compressed=True, checked=True)
    assert ok.all() and not inf.any()
    assert ctx.hash_to_curve(group, [], b"x").shape[0] == 0


@pytest.mark.parametrize("group", [1, 2])
def test_hash_to_curve_split_and_plain_forms_agree(group):
    """round 5: small batches map u0 and u1 of a message on two lane groups (k_hash_to_curve_split); 1 001 messages of ragged lengths
    through a context that always splits and one that never does give identical PROJECTIVE limbs, and both match the oracle on a
    sample (the default context of the tests above takes the split form for these sizes)"""
    import bls12_381_amd as bls
    from oracle import h2c_ref as h
    r = o.SplitMix64(77 + group)
    msgs = [b""] + [bytes((r.next() >> 8) & 0xFF for _ in range(int(r.next() % 150))) for _ in range(1000)]
    dst = b"BLS_SIG_BLS12381G%d_XMD:SHA-256_SSWU_RO_NUL_" % group
    outs = []
    for split in ("1", "0"):
        os.environ["BLSGPU_H2C_SPLIT"] = split
        try:
            c = bls.Context(0)
        finally:
            os.environ.pop("BLSGPU_H2C_SPLIT")
        try:
            outs.append(c.hash_to_curve(group, msgs, dst))
        finally:
            c.close()
    assert np.array_equal(outs[0], outs[1])
    for k in (0, 1, 500, 1000):
        p = (h.g1_hash_to_curve if group == 1 else h.g2_hash_to_curve)(msgs[k], dst)
        want = np.concatenate([(fpw(c) if group == 1 else fp2w(c)) for c in p])
        assert np.array_equal(outs[0][k], want) and np.array_equal(outs[1][k], want), (group, k)


# ---- BASELINE.json full sizes (configs[2] and the per-GPU share of configs[4]) through size-independent identities --------
def _rand_scalars_np(n, seed):
    rs = np.random.RandomState(seed)
    b = rs.randint(0, 256, size=(n, 32), dtype=np.uint8); b[:, 31] &= 0x3F          # < 2^254 < r
    return b, [int.from_bytes(b[i].tobytes(), "little") for i in range(n)]


def test_msm_g2_full_size_2_20(ctx):
    """2^20-point G2 MSM: MSM(s, [k_i] G2) == [sum s_i k_i] G2, compared on uncompressed bytes"""
    import bls12_381_amd as b
    n = 1 << 20
    kb, ks = _rand_scalars_np(n, 21)
    sb, ss = _rand_scalars_np(n, 22)
    out = ctx.msm(ctx.bases_from_scalars(2, kb), sb)
    xy, inf = ctx.batch_normalize(2, out[None, :])
    tot = sum(k * s for k, s in zip(ks, ss)) % o.R_ORDER
    assert b.G2Affine(xy[0], bool(inf[0])).to_uncompressed() == o.g2_to_uncompressed(o.g2_to_affine(o.g2_affine_mul(o.G2_GEN, tot)))


def test_pairings_full_size_2_16_and_multi_miller_2_18(ctx):
    """2^16 independent pairings (product identity + sampled exact values) and one 2^18-term multi_miller_loop:
    final_exponentiation(prod_i ML(a_i G1, b_i G2)) == e(G1, G2)^(sum a_i b_i)   (pairings.rs:871-921 at scale)"""
    n = 1 << 18
    ab, a = _rand_scalars_np(n, 31)
    bb, bs = _rand_scalars_np(n, 32)
    g1, f1 = ctx.bases_from_scalars(1, ab).download()
    g2, f2 = ctx.bases_from_scalars(2, bb).download()
    gen = o.pairing(o.G1_GEN, o.G2_GEN)
    m = 1 << 16
    gt = ctx.pairing_batch(g1[:m], f1[:m], g2[:m], f2[:m])
    assert np.array_equal(ctx.fp12_product(gt), fp12w(o.gt_mul_scalar(gen, sum(x * y for x, y in zip(a[:m], bs[:m])) % o.R_ORDER)))
    for i in (0, 12345, m - 1):
        assert np.array_equal(gt[i], fp12w(o.gt_mul_scalar(gen, a[i] * bs[i] % o.R_ORDER)))
    ml = ctx.multi_miller_loop(g1, f1, g2, f2)
    fe = ctx.final_exponentiation_batch(ml[None, :] if ml.ndim == 1 else ml)
    assert np.array_equal(np.asarray(fe).reshape(-1), fp12w(o.gt_mul_scalar(gen, sum(x * y for x, y in zip(a, bs)) % o.R_ORDER)))


def test_gt_mul_scalar_batch(ctx):
    """`&Gt * &Scalar` (pairings.rs:297-322) on the device against the oracle, edge scalars included, and its group law"""
    gen = o.pairing(o.G1_GEN, o.G2_GEN)
    r = o.SplitMix64(404)
    ss = [0, 1, 2, o.R_ORDER - 1, (1 << 254) + 12345] + [r.scalar() for _ in range(27)]
    G = np.stack([fp12w(gen)] * len(ss))
    out = ctx.gt_mul_scalar_batch(G, ss)
    for k in (0, 1, 2, 3, 4, 5, 17, 31):
        assert np.array_equal(out[k], fp12w(o.gt_mul_scalar(gen, ss[k]))), k
    # (g * a) * b == g * (a b) and g*a + g*b == g*(a+b), all on the device
    a, b = ss[7], ss[9]
    ga = ctx.gt_mul_scalar_batch(G[:1], [a])
    assert np.array_equal(ctx.gt_mul_scalar_batch(ga, [b])[0], ctx.gt_mul_scalar_batch(G[:1], [a * b % o.R_ORDER])[0])
    gb = ctx.gt_mul_scalar_batch(G[:1], [b])
    assert np.array_equal(ctx.fp12_op(0, ga, gb)[0], ctx.gt_mul_scalar_batch(G[:1], [(a + b) % o.R_ORDER])[0])
    import bls12_381_amd as bl
    assert bl.Gt(fp12w(gen)) * bl.Scalar(5) == bl.Gt(out[1]) + bl.Gt(out[1]) + bl.Gt(out[1]) + bl.Gt(out[1]) + bl.Gt(out[1])


def test_msm_fallback_sort_path(monkeypatch):
    """the global-atomic digit sort that takes over beyond 2^24 points per call (forced here through the library's test hook),
    alternating with the default path on the same sizes and on a skewed input"""
    import bls12_381_amd as b
    monkeypatch.setenv("BLSGPU_FORCE_SLOW_SORT", "1")
    slow = b.Context(0)
    monkeypatch.delenv("BLSGPU_FORCE_SLOW_SORT")
    r = o.SplitMix64(2424)
    for n, w in ((300, 0), (5000, 0), (5000, 13), (20000, 16)):
        ks = [r.scalar() for _ in range(n)]
        ss = [r.scalar() for _ in range(n)]
        _msm_case(slow, 1, ks, ss, window=w)
    _msm_case(slow, 2, [r.scalar() for _ in range(3000)], [r.scalar() for _ in range(3000)])
    _msm_case(slow, 1, [3] * 3000, [7] * 3000)                      # one bucket per window holds everything
    slow.close() if hasattr(slow, "close") else None


def test_abi_error_behaviour(ctx):
    """status codes instead of undefined behaviour: NULL / out-of-range / mismatched arguments are rejected with
    BLSGPU_ERR_ARG and a message, and the context stays usable (INTEGRATION.md "Error behaviour")"""
    import ctypes
    import bls12_381_amd as b
    lib, h = ctx.lib, ctx.h
    ERR_ARG = -2
    r = o.SplitMix64(5)
    ks = [r.scalar() for _ in range(8)]
    b1 = ctx.bases_from_scalars(1, ks)
    b2 = ctx.bases_from_scalars(2, ks)
    sc = np.zeros((8, 32), dtype=np.uint8); sc[:, 0] = 1
    out18 = np.zeros(18, dtype=np.uint64); out36 = np.zeros(36, dtype=np.uint64)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.blsgpu_g1_msm(h, b2.handle, 0, P(sc), 8, P(out18)) == ERR_ARG            # G2 bases handed to the G1 entry point
    assert b"other group" in lib.blsgpu_last_error()
    assert lib.blsgpu_g1_msm(h, b1.handle, 4, P(sc), 8, P(out18)) == ERR_ARG            # range runs past the resident bases
    assert lib.blsgpu_g1_msm(h, b1.handle, 0, None, 8, P(out18)) == ERR_ARG             # NULL scalars with n > 0
    assert lib.blsgpu_g1_msm(h, None, 0, P(sc), 8, P(out18)) == ERR_ARG
    assert lib.blsgpu_fp_op(h, 99, P(out18), P(out18), 1, P(out18)) == ERR_ARG
    assert lib.blsgpu_fr_ntt(h, P(out36), 40, 0) == ERR_ARG                              # log_n out of range
    assert lib.blsgpu_set_msm_window(h, 3) == ERR_ARG
    assert lib.blsgpu_pairing_batch(h, None, None, None, None, 4, P(out36)) == ERR_ARG
    with pytest.raises(b.BlsGpuError):
        ctx.fr_op(0, np.zeros((2, 4), dtype=np.uint64))                                  # binary op without b
    with pytest.raises(ValueError):
        ctx.fr_ntt(np.zeros((3, 4), dtype=np.uint64))
    # n = 0 is a value, not an error: identity / Fp12::one (src/pairings.rs:554-603 with no terms)
    assert lib.blsgpu_g1_msm(h, b1.handle, 0, None, 0, P(out18)) == 0
    xy, inf = ctx.batch_normalize(1, out18[None, :])
    assert bool(inf[0])
    # the context still works
    _msm_case(ctx, 1, ks, [1] * 8)


@pytest.mark.parametrize("n", [(1 << 17) + 5, (1 << 18) + 1, (1 << 19) + 3])
def test_multi_miller_shared_squarings(ctx, n):
    """large multi_miller_loop calls put K = 2 / 4 / 8 terms on one accumulator (one squaring per bit for all of them);
    the raw value must equal the product of the individual Miller values limb for limb, identity terms skipped, ragged n"""
    m = 4096                                                    # distinct points; terms cycle through them
    r = o.SplitMix64(n)
    g1, f1 = ctx.bases_from_scalars(1, [r.scalar() for _ in range(m)]).download()
    g2, f2 = ctx.bases_from_scalars(2, [r.scalar() for _ in range(m)]).download()
    idx = np.arange(n) % m
    G1, G2 = g1[idx], g2[(idx * 7 + 3) % m]
    F1 = np.zeros(n, dtype=np.uint8); F2 = np.zeros(n, dtype=np.uint8)
    F1[[0, 5, n - 1]] = 1; F2[[5, 77, n - 2]] = 1               # identities on either side, including the ragged tail
    got = ctx.multi_miller_loop(G1, F1, G2, F2)
    each = ctx.miller_loop_batch(G1[:m], np.zeros(m, dtype=np.uint8), G2[:m], np.zeros(m, dtype=np.uint8))   # first m terms individually
    # product over all n terms from per-term values: terms repeat with period lcm; evaluate through the batch API in chunks
    acc = None
    for s0 in range(0, n, 1 << 16):
        e0 = min(n, s0 + (1 << 16))
        part = ctx.fp12_product(ctx.miller_loop_batch(G1[s0:e0], F1[s0:e0], G2[s0:e0], F2[s0:e0]))
        acc = part if acc is None else ctx.fp12_op(0, acc[None, :], part[None, :])[0]
    assert np.array_equal(got, acc)
    assert np.array_equal(each[1], ctx.miller_loop_batch(G1[1:2], F1[1:2], G2[1:2], F2[1:2])[0])


def test_msm_pipelined_slots_are_independent(ctx):
    """twelve asynchronous MSMs of different sizes, groups and scalars through the four pipeline slots (three streams
    each), results compared with the synchronous calls: catches any scratch shared between calls in flight"""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    rs = np.random.RandomState(77)
    nmax = 1 << 16
    kb = rs.randint(0, 256, size=(nmax, 32), dtype=np.uint8); kb[:, 31] &= 0x3F
    bases = {1: ctx.bases_from_scalars(1, kb), 2: ctx.bases_from_scalars(2, kb[:1 << 14])}
    jobs = []
    for j in range(12):
        g = 2 if j % 3 == 2 else 1
        n = [1 << 16, 40000, 1 << 12, 1 << 14, 777, 1 << 15][j % 6]
        if g == 2:
            n = min(n, 1 << 14)
        sb = rs.randint(0, 256, size=(n, 32), dtype=np.uint8); sb[:, 31] &= 0x3F
        jobs.append((g, n, sb, torch.from_numpy(sb).to(dev), torch.zeros(18 * g, dtype=torch.int64, device=dev)))
    want = [ctx.msm(bases[g], sb) for g, n, sb, _, _ in jobs]             # synchronous reference results
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_pipelining(True)
    try:
        for rep in range(2):
            for g, n, sb, d_s, d_o in jobs:
                ctx.msm_device(bases[g], d_s.data_ptr(), n, d_o.data_ptr())
            ctx.join(0)
            torch.cuda.synchronize()
            for (g, n, sb, d_s, d_o), w in zip(jobs, want):
                got = d_o.cpu().numpy().view(np.uint64)
                assert np.array_equal(ctx.batch_normalize(g, got[None, :])[0], ctx.batch_normalize(g, w[None, :])[0]), (rep, g, n)
                d_o.zero_()
    finally:
        ctx.set_pipelining(False)
        ctx.set_stream(0)


@pytest.mark.parametrize("group", [1, 2])
def test_msm_on_public_encodings(ctx, golden_dir, group):
    """`blsgpu_g{1,2}_msm_bytes`: the golden k*G records (uncompressed bytes, k = 0..999, identity included) as bases,
    random scalars -> uncompressed bytes of [sum s_k k] G; invalid encodings are refused"""
    import bls12_381_amd as b
    size = 96 if group == 1 else 192
    raw = open(os.path.join(golden_dir, f"g{group}_uncompressed_valid_test_vectors.dat"), "rb").read()
    n = 300
    r = o.SplitMix64(group)
    ss = [r.scalar() for _ in range(n)]
    got = ctx.msm_bytes(group, raw[:n * size], ss)
    tot = sum(k * s for k, s in enumerate(ss)) % o.R_ORDER
    if group == 1:
        want = o.g1_to_uncompressed(o.g1_to_affine(o.g1_affine_mul(o.G1_GEN, tot)))
    else:
        want = o.g2_to_uncompressed(o.g2_to_affine(o.g2_affine_mul(o.G2_GEN, tot)))
    assert got == want
    assert ctx.msm_bytes(group, b"", []) == (o.g1_to_uncompressed(o.G1_IDENTITY_AFF) if group == 1 else o.g2_to_uncompressed(o.G2_IDENTITY_AFF))
    bad = bytearray(raw[size:2 * size]); bad[0] |= 0x80                       # compression flag on an uncompressed encoding
    with pytest.raises(b.BlsGpuError):
        ctx.msm_bytes(group, bytes(bad), [1])


def test_pairing_batch_exact_vs_c_oracle(ctx):
    """2^12 pairings, raw Miller values and final results, limb for limb against the tier-1 C restatement of pairings.rs
    (identities on either side included)"""
    from oracle import c_oracle
    c_oracle.build()
    n = 1 << 12
    ab, _ = _rand_scalars_np(n, 41)
    bb, _ = _rand_scalars_np(n, 42)
    g1, f1 = ctx.bases_from_scalars(1, ab).download()
    g2, f2 = ctx.bases_from_scalars(2, bb).download()
    f1 = f1.copy(); f2 = f2.copy(); f1[[3, 100]] = 1; f2[[100, 4000]] = 1
    want_ml, _ = c_oracle.pairing_batch(1, g1, f1, g2, f2)
    want, _ = c_oracle.pairing_batch(0, g1, f1, g2, f2)
    assert np.array_equal(ctx.miller_loop_batch(g1, f1, g2, f2), want_ml)
    assert np.array_equal(ctx.pairing_batch(g1, f1, g2, f2), want)
    assert np.array_equal(ctx.final_exponentiation_batch(want_ml[:64]), c_oracle.pairing_batch(2, want_ml[:64], None, None, None)[0])


@pytest.mark.parametrize("group", [1, 2])
def test_msm_many_matches_single_calls(ctx, group):
    """`blsgpu_g{1,2}_msm_many`: k MSMs over the same bases through the internal pipeline == k synchronous calls"""
    n, k = (1 << 15, 9) if group == 1 else (1 << 13, 6)
    kb, _ = _rand_scalars_np(n, 50 + group)
    bases = ctx.bases_from_scalars(group, kb)
    rs = np.random.RandomState(60 + group)
    S = rs.randint(0, 256, size=(k, n, 32), dtype=np.uint8); S[:, :, 31] &= 0x3F
    S[2, :, :] = 0                                                 # one all-zero vector: identity in the middle of the batch
    many = ctx.msm_many(bases, S)
    for j in range(k):
        one = ctx.msm(bases, S[j])
        assert np.array_equal(ctx.batch_normalize(group, many[j][None, :])[0], ctx.batch_normalize(group, one[None, :])[0]), j
    assert ctx.batch_normalize(group, many[2][None, :])[1][0] == 1
    assert ctx.msm_many(bases, S[:0]).shape[0] == 0


# ---- round 2: the north-star sizes with the survey's input distribution (uniform in [0, r): top bits and the top-window carry) ----
def _g1_point_bytes(ctx, xyz):
    import bls12_381_amd as b
    xy, inf = ctx.batch_normalize(1, np.asarray(xyz)[None, :])
    return b.G1Affine(xy[0], bool(inf[0])).to_uncompressed()


def _expected_g1(tot):
    """[tot] G1 as uncompressed bytes, by the tier-1 C oracle (one 255-step double-and-add of the generator)"""
    from oracle import c_oracle
    gx = np.concatenate([fpw(o.G1_GEN[0]), fpw(o.G1_GEN[1])])
    xyz = c_oracle.g1_affine_mul(gx, False, np.frombuffer(int(tot).to_bytes(32, "little"), dtype=np.uint8))
    xy, inf = c_oracle.g1_to_affine(xyz)
    import bls12_381_amd as b
    return b.G1Affine(xy, inf).to_uncompressed()


def test_msm_north_star_sizes_2_21_2_24_and_beyond(ctx):
    """2^21 points (the per-GPU share of BASELINE configs[3]), 2^24 points (the whole of it on one GPU) and 2^24 + 3 points (the
    first size on the fallback sort), scalars uniform in [0, r) from the survey's SplitMix64 stream, through the discrete-log
    identity MSM(s, [k_i]G) = [sum s_i k_i]G on uncompressed bytes; the three calls share one resident base set"""
    from bls12_381_amd import synthetic as sy
    n = (1 << 24) + 3
    kb = sy.scalars(n, sy.SEED + 11)
    sb = sy.scalars(n, sy.SEED + 12)
    assert (sb[:, 31] >> 6).max() == 1                       # bit 254 is in play
    bases = ctx.bases_from_scalars(1, kb)
    # spot-check the device-built bases against the reference definition (tier-1 C): first / last / a few in between
    from oracle import c_oracle
    gx = np.concatenate([fpw(o.G1_GEN[0]), fpw(o.G1_GEN[1])])
    for i in (0, 1, 12345, (1 << 21) - 1, 1 << 24, n - 1):
        xy, inf = bases.download(i, 1)
        want = c_oracle.g1_to_affine(c_oracle.g1_affine_mul(gx, False, kb[i]))
        assert np.array_equal(xy[0], want[0]) and bool(inf[0]) == want[1], i
    tot = 0
    prev = 0
    for m in (1 << 21, 1 << 24, n):
        tot = (tot + sy.dot_mod_r(kb[prev:m], sb[prev:m])) % o.R_ORDER
        prev = m
        got = ctx.msm(bases, sb[:m])
        assert _g1_point_bytes(ctx, got) == _expected_g1(tot), m
    bases.free()


def test_msm_2_15_exact_vs_tier1_reference_definition(ctx):
    """2^15 (point, scalar) pairs: the GPU result equals sum(P_i * s_i) evaluated by the tier-1 C restatement of the reference's
    own multiply + Sum (g1.rs:754-774, :161-171), for G1 and (2^12) for G2; uniform scalars incl. the top bits"""
    from bls12_381_amd import synthetic as sy
    from oracle import c_oracle
    for group, m in ((1, 1 << 15), (2, 1 << 12)):
        kb = sy.scalars(m, 900 + group); sb = sy.scalars(m, 950 + group)
        bases = ctx.bases_from_scalars(group, kb)
        xy, inf = bases.download()
        got = ctx.msm(bases, sb)
        if group == 1:
            ref, _ = c_oracle.g1_msm(xy, inf, sb, 0)
            assert np.array_equal(ctx.batch_normalize(1, got[None, :])[0][0], c_oracle.g1_to_affine(ref)[0])
        else:
            ref, _ = c_oracle.g2_msm(xy, inf, sb, 0)
            assert np.array_equal(ctx.batch_normalize(2, got[None, :])[0][0], c_oracle.g2_to_affine(ref)[0])


def test_noncanonical_scalars_are_reported_not_miscomputed(ctx):
    """a raw 32-byte scalar >= r has no `Scalar` value in the reference (from_bytes -> None, scalar.rs:256-280): the library
    reports BLSGPU_ERR_ARG for it -- at every window width -- instead of returning (s - 2^256) P for the widths that divide 256"""
    import ctypes
    import bls12_381_amd as b
    r = o.SplitMix64(77)
    n = 64
    ks = [r.scalar() for _ in range(n)]
    bases = ctx.bases_from_scalars(1, ks)
    sb = np.stack([np.frombuffer(r.scalar().to_bytes(32, "little"), dtype=np.uint8) for _ in range(n)]).copy()
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    out = np.zeros(18, dtype=np.uint64)
    for bad in (o.R_ORDER, (1 << 255) + 5, (1 << 256) - 1):
        s2 = sb.copy(); s2[17] = np.frombuffer(bad.to_bytes(32, "little"), dtype=np.uint8)
        for w in (0, 8, 13, 16):
            ctx.set_msm_window(w)
            assert ctx.lib.blsgpu_g1_msm(ctx.h, bases.handle, 0, P(s2), n, P(out)) == -2, (hex(bad), w)
            assert b"canonical" in ctx.lib.blsgpu_last_error()
            assert ctx.lib.blsgpu_g1_msm(ctx.h, bases.handle, 0, P(sb), n, P(out)) == 0          # the flag does not stick to the next call
        with pytest.raises(ValueError):
            ctx.msm(bases, s2)                                                                      # the Python mirror rejects before the call
    ctx.set_msm_window(0)
    # r - 1 is canonical and exact
    _msm_case(ctx, 1, ks[:3], [o.R_ORDER - 1, o.R_ORDER - 2, 1])
    # attribution: an ASYNCHRONOUS call with a bad scalar is reported by blsgpu_synchronize; a valid synchronous call made in
    # between returns OK (its verdict travels with its own result) and does not clear the asynchronous call's flag
    import torch
    dev = torch.device("cuda", 0)
    d_bad = torch.from_numpy(s2.view(np.int64).copy()).to(dev); d_out = torch.zeros(18, dtype=torch.int64, device=dev)
    assert ctx.lib.blsgpu_g1_msm_device(ctx.h, bases.handle, 0, ctypes.c_void_p(d_bad.data_ptr()), n, ctypes.c_void_p(d_out.data_ptr())) == 0
    assert ctx.lib.blsgpu_g1_msm(ctx.h, bases.handle, 0, P(sb), n, P(out)) == 0
    good = ctx.batch_normalize(1, out[None, :].copy())           # the projective representative depends on the summation order: compare the point
    assert ctx.lib.blsgpu_synchronize(ctx.h) == -2 and b"canonical" in ctx.lib.blsgpu_last_error()
    assert ctx.lib.blsgpu_synchronize(ctx.h) == 0
    assert ctx.lib.blsgpu_g1_msm(ctx.h, bases.handle, 0, P(sb), n, P(out)) == 0
    again = ctx.batch_normalize(1, out[None, :].copy())
    assert np.array_equal(good[0], again[0]) and np.array_equal(good[1], again[1])
    want = o.g1_to_affine(o.g1_affine_mul(o.G1_GEN, sum(k * int.from_bytes(bytes(sb[i]), "little") for i, k in enumerate(ks)) % o.R_ORDER))
    assert b.G1Affine(good[0][0], bool(good[1][0])).to_uncompressed() == o.g1_to_uncompressed(want)


def test_two_contexts_on_two_host_threads(ctx):
    """the ABI is re-entrant per context: two contexts driven from two host threads at the same time (G1 MSMs on one, pairings and
    a G2 MSM on the other) give the same results as the same calls made alone"""
    import threading
    import bls12_381_amd as b
    from bls12_381_amd import synthetic as sy
    n = 1 << 14
    kb, sb = sy.scalars(n, 31), sy.scalars(n, 32)
    ka, kq = sy.scalars(256, 33), sy.scalars(256, 34)
    c1, c2 = b.Context(0), b.Context(0)
    b1 = c1.bases_from_scalars(1, kb); b2 = c2.bases_from_scalars(2, kb[:4096])
    g1, f1 = c2.bases_from_scalars(1, ka).download(); g2, f2 = c2.bases_from_scalars(2, kq).download()
    want1 = c1.msm(b1, sb); want2 = c2.msm(b2, sb[:4096]); wantp = c2.pairing_batch(g1, f1, g2, f2)
    res, errs = {}, []

    def t1():
        try:
            res["a"] = [c1.msm(b1, sb) for _ in range(6)]
        except Exception as ex:      # noqa: BLE001
            errs.append(ex)

    def t2():
        try:
            res["b"] = [(c2.pairing_batch(g1, f1, g2, f2), c2.msm(b2, sb[:4096])) for _ in range(3)]
        except Exception as ex:      # noqa: BLE001
            errs.append(ex)
    th = [threading.Thread(target=t1), threading.Thread(target=t2)]
    [t.start() for t in th]; [t.join() for t in th]
    assert not errs, errs
    n1 = lambda x: c1.batch_normalize(1, x[None, :])[0]
    n2 = lambda x: c2.batch_normalize(2, x[None, :])[0]
    assert all(np.array_equal(n1(x), n1(want1)) for x in res["a"])
    assert all(np.array_equal(p, wantp) and np.array_equal(n2(m), n2(want2)) for p, m in res["b"])
    c1.close(); c2.close()


@pytest.mark.parametrize("world", [2, 8])
def test_logical_ranks_sharded_pairings_and_mixed_workload(ctx, world):
    """BASELINE configs[4] as `world` logical ranks on one GPU (SURVEY.md 8e caveat), reduced sizes: every rank runs its shard of
    the G1 MSM, the G2 MSM and the multi_miller_loop concurrently on three contexts (bench.MixedJobs, the code `bench.py
    --workload mixed` runs), the partials are gathered and folded as the RCCL path does, and the folded results satisfy the
    discrete-log identities; plus N independent pairings sharded by index slices with no exchange (pairings.rs:607-653)"""
    import torch
    import bench
    import bls12_381_amd as b
    from bls12_381_amd.distributed import LogicalRanks, sharded_pairings, shard_range
    sizes = (12, 11, 9)
    lr = LogicalRanks(world)
    exp = [0, 0, 0]
    for rank in range(world):
        jobs = bench.MixedJobs(b, torch, 0, sizes, rank, world, seed_base=4242)
        jobs.launch()                                   # three jobs in flight at once on this logical rank
        p1, p2, pm = jobs.partials()
        for k, v in enumerate((p1, p2, pm)):
            lr.contribute(("part", k), rank, v)
        e = jobs.expected_scalars()
        exp = [(a + c) % o.R_ORDER for a, c in zip(exp, e)]
        for c in jobs.ctx:
            c.close()
    g1sum = ctx.point_sum(1, lr.collect(("part", 0)))
    g2sum = ctx.point_sum(2, lr.collect(("part", 1)))
    fsum = ctx.fp12_product(lr.collect(("part", 2)))
    assert _g1_point_bytes(ctx, g1sum) == _expected_g1(exp[0])
    xy, inf = ctx.batch_normalize(2, g2sum[None, :])
    assert b.G2Affine(xy[0], bool(inf[0])).to_uncompressed() == o.g2_to_uncompressed(o.g2_to_affine(o.g2_affine_mul(o.G2_GEN, exp[1])))
    gt = ctx.final_exponentiation_batch(fsum[None, :])[0]
    assert np.array_equal(gt, fp12w(o.gt_mul_scalar(o.pairing(o.G1_GEN, o.G2_GEN), exp[2])))
    # independent pairings: rank r computes only its slice; concatenating the slices gives the unsharded batch
    r = o.SplitMix64(99 + world)
    n = 37
    a = [r.scalar() for _ in range(n)]; q = [r.scalar() for _ in range(n)]
    g1, f1 = ctx.bases_from_scalars(1, a).download(); g2, f2 = ctx.bases_from_scalars(2, q).download()
    f1[5] = 1
    whole = ctx.pairing_batch(g1, f1, g2, f2)
    seen = np.zeros((n, 72), dtype=np.uint64)
    for rank in range(world):
        (lo, hi), mine = sharded_pairings(lambda lo, hi: ctx.pairing_batch(g1[lo:hi], f1[lo:hi], g2[lo:hi], f2[lo:hi]) if hi > lo else np.zeros((0, 72), dtype=np.uint64),
                                          n, world, rank)
        assert (lo, hi) == shard_range(n, rank, world)
        seen[lo:hi] = mine
    assert np.array_equal(seen, whole)
    gen = o.pairing(o.G1_GEN, o.G2_GEN)
    assert np.array_equal(whole[7], fp12w(o.gt_mul_scalar(gen, a[7] * q[7] % o.R_ORDER))) and np.array_equal(whole[5], fp12w(o.FP12_ONE))


def test_device_variants_of_miller_final_exp_product(ctx):
    """the device-pointer entry points a sharded multi_miller_loop is built from agree with their host-pointer twins"""
    import torch
    r = o.SplitMix64(555)
    n = 33
    a = [r.scalar() for _ in range(n)]; q = [r.scalar() for _ in range(n)]
    g1, f1 = ctx.bases_from_scalars(1, a).download(); g2, f2 = ctx.bases_from_scalars(2, q).download()
    dev = torch.device("cuda", 0)
    d1 = torch.from_numpy(g1.view(np.int64)).to(dev); d2 = torch.from_numpy(g2.view(np.int64)).to(dev)
    dml = torch.zeros((n, 72), dtype=torch.int64, device=dev); dgt = torch.zeros((n, 72), dtype=torch.int64, device=dev)
    dpr = torch.zeros(72, dtype=torch.int64, device=dev)
    ctx.miller_loop_batch_device(d1.data_ptr(), d2.data_ptr(), n, dml.data_ptr())
    ctx.final_exponentiation_device(dml.data_ptr(), n, dgt.data_ptr())
    ctx.fp12_product_device(dml.data_ptr(), n, dpr.data_ptr())
    ctx.synchronize()
    ml = ctx.miller_loop_batch(g1, None, g2, None)
    assert np.array_equal(dml.cpu().numpy().view(np.uint64), ml)
    assert np.array_equal(dgt.cpu().numpy().view(np.uint64), ctx.pairing_batch(g1, None, g2, None))
    assert np.array_equal(dpr.cpu().numpy().view(np.uint64), ctx.multi_miller_loop(g1, None, g2, None))


@pytest.mark.parametrize("workload", ["msm", "mixed"])
def test_bench_distributed_branch_over_rccl_with_one_rank(workload, tmp_path):
    """bench.py's N > 1 code path -- process group on backend "nccl" (= RCCL) bound to the device, the (world, words) int64
    all-gather of the partial sums on the GPU, the device-side fold, the max / min all-reduces of the timing and agreement
    checks -- executed for real with a single rank (`--dist-single`): a one-GPU box cannot run two RCCL ranks, but every
    call of the branch goes through RCCL exactly as it does with eight."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--dist-single", "--steps", "3", "--warmup", "1",
           "--full", "--no-cpu-baseline", "--no-extras", "--dump-outputs", str(tmp_path)]
    if workload == "msm":
        cmd += ["--log-total", "18"]
    else:
        cmd += ["--workload", "mixed", "--mixed-log", "14", "12", "10"]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", BENCH_FORCE_GROUP_PATH="1")
    env.pop("MASTER_PORT", None)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 1 and line["value"] > 0
    if workload == "msm":
        assert line["scaling"] == "strong" and line["config"]["total_points"] == 1 << 18
        assert "RCCL all-gather" in line["config"]["workload"]
        # the one-process device-group measurement a multi-rank run appends (rank 0 drives every GPU while the others wait at a CPU-side barrier)
        gp = line["group_path"]
        assert "error" not in gp and gp["result_matches"] is True and gp["total_points"] == 1 << 18 and gp["value"] > 0
        sizes = {"g1_msm_result": 96}
    else:
        assert line["ranks_agree"] is True
        sizes = {"g1_msm_result": 96, "g2_msm_result": 192, "multi_miller_loop_final_exp_result": 576}
    # --dump-outputs: the folded results of the last step, as float64 bytes
    assert sorted(os.listdir(str(tmp_path))) == sorted(k + ".npy" for k in sizes)
    for k, sz in sizes.items():
        a = np.load(str(tmp_path / (k + ".npy")))
        assert a.dtype == np.float64 and a.shape == (sz,) and np.array_equal(a, np.round(a)) and 0 <= a.min() and a.max() <= 255 and a.any()


def test_msm_g2_psi_decomposition_boundaries(ctx, monkeypatch):
    """G2 MSMs split every scalar into four signed base-|x| digits (psi acts as [x] on the subgroup, g2.rs:475-482 / :847-890).
    Scalars at the digit boundaries -- multiples of X, X^2, X^3 and their neighbours, the balancing threshold X/2, the carry
    out of the top digit (folded back with x^4 = x^2 - 1 mod r), 0, 1, r - 1 -- against the oracle, on the default path and
    with the decomposition switched off."""
    import bls12_381_amd as b
    X = 0xd201000000010000
    H = X // 2
    rr = o.R_ORDER
    cand = [0, 1, 2, rr - 1, rr - 2, H, H + 1, H - 1, X - 1, X, X + 1]
    for pw in (2, 3):
        for m in (1, 2, H, H + 1, X - 1):
            for dlt in (-1, 0, 1):
                cand.append(m * X ** pw + dlt)
                cand.append(m * X ** pw + H + dlt)
    cand += [X ** 3 * (X - 1) + X ** 2 * (X - 1), (H + 1) * (1 + X + X ** 2 + X ** 3), H * (1 + X + X ** 2 + X ** 3)]
    ss = sorted({c % rr for c in cand if c >= 0})
    r = o.SplitMix64(4040)
    ks = [r.scalar() for _ in ss]
    _msm_case(ctx, 2, ks, ss)
    _msm_case(ctx, 2, ks, ss, window=13)
    _msm_case(ctx, 2, [5] * len(ss), ss)                      # one base, every term lands on the same four images
    monkeypatch.setenv("BLSGPU_NO_GLV", "1")
    plain = b.Context(0)
    monkeypatch.delenv("BLSGPU_NO_GLV")
    _msm_case(plain, 2, ks, ss)
    n = 1 << 12
    ks2 = [r.scalar() for _ in range(n)]; ss2 = [r.scalar() for _ in range(n)]
    _msm_case(plain, 2, ks2, ss2)
    _msm_case(ctx, 2, ks2, ss2)


def test_msm_decomposition_size_limits(ctx):
    """the endomorphism decompositions multiply the number of sort entries (G1: 2n, G2: 4n) and the packed sort index has 24
    bits: the largest calls that still take them -- 2^23 G1 points, 2^22 G2 points, where the index reaches 2^24 - 1 -- and the
    first sizes past the limit (plain windows: cutting larger calls into passes that keep the split was measured slower,
    DESIGN.md 9) must all agree with the discrete-log identity; uniform scalars in [0, r)"""
    import bls12_381_amd as b
    from bls12_381_amd import synthetic as sy
    # G1: 2^23 (2n = 2^24, GLV) and 2^23 + 5 (plain 16 windows), one resident base set
    n = (1 << 23) + 5
    kb = sy.scalars(n, sy.SEED + 31); sb = sy.scalars(n, sy.SEED + 32)
    bases = ctx.bases_from_scalars(1, kb)
    tot = sy.dot_mod_r(kb[:1 << 23], sb[:1 << 23])
    assert _g1_point_bytes(ctx, ctx.msm(bases, sb[:1 << 23])) == _expected_g1(tot)
    tot = (tot + sy.dot_mod_r(kb[1 << 23:], sb[1 << 23:])) % o.R_ORDER
    assert _g1_point_bytes(ctx, ctx.msm(bases, sb)) == _expected_g1(tot)
    bases.free()
    # G2: 2^22 points (4n = 2^24, psi decomposition; the images take 4 GB); a base set of 2^22 + 1 points keeps no images
    m = 1 << 22
    kb = sy.scalars(m + 1, sy.SEED + 41); sb = sy.scalars(m + 1, sy.SEED + 42)

    def g2_bytes(out):
        xy, inf = ctx.batch_normalize(2, out[None, :])
        return b.G2Affine(xy[0], bool(inf[0])).to_uncompressed()

    def want(t):
        return o.g2_to_uncompressed(o.g2_to_affine(o.g2_affine_mul(o.G2_GEN, t)))
    bases = ctx.bases_from_scalars(2, kb[:m])
    tot = sy.dot_mod_r(kb[:m], sb[:m])
    assert g2_bytes(ctx.msm(bases, sb[:m])) == want(tot)
    bases.free()
    bases = ctx.bases_from_scalars(2, kb)
    tot = (tot + sy.dot_mod_r(kb[m:], sb[m:])) % o.R_ORDER
    assert g2_bytes(ctx.msm(bases, sb)) == want(tot)
    bases.free()


@pytest.mark.parametrize("hook,value", [("BLSGPU_ITEM_CAP", "16"), ("BLSGPU_NO_GLV", "1")])
def test_msm_alternative_paths_behind_ab_hooks(monkeypatch, hook, value):
    """two settings stay switchable at context creation because product paths depend on them: short work items (every bucket cut,
    partial sums folded -- the path heavy buckets take) and plain windows without the endomorphism decompositions (the path of
    off-subgroup base sets and of sets beyond the sort's index width): each must produce the same group elements as the default
    path on the edge cases and on a medium random case, for both groups.  (The slower experimental kernels of round 2 now live
    in tools/experiments/, outside the product.)"""
    import bls12_381_amd as b
    monkeypatch.setenv(hook, value)
    c = b.Context(0)
    monkeypatch.delenv(hook)
    r = o.SplitMix64(1234)
    rr = o.R_ORDER
    ks = [1, 2, 3, 0, 5, 5, 5, rr - 5, 7, rr - 7, 0, 11] + [r.scalar() for _ in range(20)]
    ss = [0, 1, rr - 1, 12345, 9, 9, rr - 9, 9, (1 << 254), (1 << 254), 0, (1 << 16) - 1] + \
         [(1 << (16 * i)) - 1 for i in range(1, 11)] + [(1 << 15) + (1 << (16 * i + 15)) for i in range(10)]
    for group in (1, 2):
        for w in (0, 7, 16):
            _msm_case(c, group, ks, ss, window=w)
        _msm_case(c, group, [3] * 300, [1] * 300)
        _msm_case(c, group, [4, rr - 4, 4, 4], [77, 77, 77, 5])
        n = 1 << (14 if group == 1 else 12)
        _msm_case(c, group, [r.scalar() for _ in range(n)], [r.scalar() for _ in range(n)])


# ---- round 3: the MSM is total over curve points; decomposition boundaries ------------------------------------------
def _off_subgroup_points(kats, group):
    """the reference's own on-curve, off-subgroup points (src/g1.rs:1598-1640, src/g2.rs:1862-1906; test_is_torsion_free)"""
    F = o.fp_from_mont_limbs
    if group == 1:
        v = kats["tests"]["g1.test_is_torsion_free"]["fp"]
        return (F(v[0]), F(v[1]), False)
    v = kats["tests"]["g2.test_is_torsion_free"]["fp"]
    return ((F(v[0]), F(v[1])), (F(v[2]), F(v[3])), False)


@pytest.mark.parametrize("group", [1, 2])
def test_msm_with_off_subgroup_points_equals_reference_double_and_add(ctx, kats, group):
    """`multiply` (g1.rs:754-774, g2.rs:825-845) is plain double-and-add over the 255 scalar bits and therefore defined for
    every curve point -- including what from_uncompressed_unchecked hands out.  The endomorphism split is only valid on the
    subgroup, so an uploaded set with such a point must fall back to plain windows and still give the reference's sum; a
    clean set keeps the fast path.  Checked through upload_bases, the one-shot host call, the public-encoding entry point
    and the mirror's `Mul`; scalars include 0, 1, r - 1 and GLV / psi digit boundaries."""
    import bls12_381_amd as b
    gen, amul, msm, toaff, enc, affw, add, aff_to_proj = (
        (o.G1_GEN, o.g1_affine_mul, o.g1_msm, o.g1_to_affine, o.g1_to_uncompressed, g1aff_w, o.g1_add, o.g1_from_affine) if group == 1 else
        (o.G2_GEN, o.g2_affine_mul, o.g2_msm, o.g2_to_affine, o.g2_to_uncompressed, g2aff_w, o.g2_add, o.g2_from_affine))
    on_curve, torsion_free = (o.g1_is_on_curve, o.g1_is_torsion_free) if group == 1 else (o.g2_is_on_curve, o.g2_is_torsion_free)
    A = _off_subgroup_points(kats, group)
    assert on_curve(A) and not torsion_free(A)
    r = o.SplitMix64(7300 + group)
    rr = o.R_ORDER
    L = 0xd201000000010000 ** 2
    # a second off-subgroup point: A + [k]G (still on the curve, still outside the subgroup)
    A2 = toaff(add(aff_to_proj(A), amul(gen, 12345)))
    assert on_curve(A2) and not torsion_free(A2)
    good = [toaff(amul(gen, r.scalar())) for _ in range(9)]
    pts = good[:4] + [A] + good[4:7] + [A2] + good[7:] + [A]
    ss = [r.scalar(), 0, 1, rr - 1, r.scalar(), L, L + 1, L // 2 + 1, rr - 1, 3 * L - 1, r.scalar(), 1]
    assert len(pts) == len(ss)
    want = enc(toaff(msm(pts, ss)))                                    # the oracle's double-and-add + Sum (reference definition)
    AffT = b.G1Affine if group == 1 else b.G2Affine
    xy = np.stack([affw(p)[0] for p in pts]); inf = np.array([affw(p)[1] for p in pts], dtype=np.uint8)

    def aff_bytes(proj):
        axy, ainf = ctx.batch_normalize(group, proj[None, :])
        return AffT(axy[0], bool(ainf[0])).to_uncompressed()

    # resident upload: the set is detected as off-subgroup and keeps no images
    bases = ctx.upload_bases(group, xy, inf)
    assert bases.subgroup_state == 0
    for w in (0, 5, 16):
        ctx.set_msm_window(w)
        assert aff_bytes(ctx.msm(bases, ss)) == want
    ctx.set_msm_window(0)
    # clean set: fast path stays on, result is the reference's
    clean = ctx.upload_bases(group, np.stack([affw(p)[0] for p in good]), None)
    assert clean.subgroup_state == 1
    want_clean = enc(toaff(msm(good, ss[:9])))
    assert aff_bytes(ctx.msm(clean, ss[:9])) == want_clean
    # one-shot host call and the mirror's msm / Mul
    mir = [AffT(*affw(p)) for p in pts]
    got = (b.msm_g1 if group == 1 else b.msm_g2)(mir, ss).to_affine().to_uncompressed()
    assert got == want
    for s in (0, 1, 2, rr - 1, L, r.scalar()):
        single = (AffT(*affw(A)) * b.Scalar(s)).to_affine().to_uncompressed()
        assert single == enc(toaff(amul(A, s)))
    # public encodings (from_uncompressed_unchecked semantics)
    raw = b"".join(enc(p) for p in pts)
    sb = b"".join(int(s).to_bytes(32, "little") for s in ss)
    out = (ctypes_msm_bytes(ctx, group, raw, sb, len(pts)))
    assert out == want
    # the caller may vouch for a set: the test is skipped (state 2); for a genuinely clean set the result is unchanged
    ctx.set_assume_subgroup(True)
    try:
        vouched = ctx.upload_bases(group, np.stack([affw(p)[0] for p in good]), None)
        assert vouched.subgroup_state == 2
        assert aff_bytes(ctx.msm(vouched, ss[:9])) == want_clean
    finally:
        ctx.set_assume_subgroup(False)


def ctypes_msm_bytes(ctx, group, raw, sb, n):
    import ctypes
    from bls12_381_amd import _lib
    lib = _lib.load()
    out = (ctypes.c_uint8 * (96 if group == 1 else 192))()
    fn = lib.blsgpu_g1_msm_bytes if group == 1 else lib.blsgpu_g2_msm_bytes
    _lib.check(fn(ctx.h, ctypes.cast(ctypes.c_char_p(raw), ctypes.c_void_p), ctypes.cast(ctypes.c_char_p(sb), ctypes.c_void_p), n,
                  ctypes.cast(out, ctypes.c_void_p)), "msm_bytes")
    return bytes(out)


def test_msm_g1_glv_decomposition_boundaries(ctx, monkeypatch):
    """G1 MSMs split k = k1 + k2 L (L = z^2, phi(P) = -[L]P on the subgroup, g1.rs:396-437) into balanced halves.  Scalars at
    every branch of k_glv_decompose -- multiples of L and their neighbours, the balancing threshold L/2 for either half (with
    the k1 = 0 corner), scalars on which the Barrett quotient estimate is one short, 0, 1, r - 1 -- against the oracle, on the
    default path, with another window and with the decomposition switched off (mirrors the G2 test)."""
    import bls12_381_amd as b
    from tests.decomp_model import glv_candidates
    rr = o.R_ORDER
    ss = glv_candidates()
    assert all(0 <= s < rr for s in ss)
    r = o.SplitMix64(5050)
    ks = [r.scalar() for _ in ss]
    _msm_case(ctx, 1, ks, ss)
    _msm_case(ctx, 1, ks, ss, window=13)
    _msm_case(ctx, 1, ks, ss, window=7)
    _msm_case(ctx, 1, [5] * len(ss), ss)                      # one base: every term lands on P or phi(P)
    monkeypatch.setenv("BLSGPU_NO_GLV", "1")
    plain = b.Context(0)
    monkeypatch.delenv("BLSGPU_NO_GLV")
    _msm_case(plain, 1, ks, ss)


# ---- round 3: the quad-lane pairing kernels (quad.hip.h) ----------------------------------------------------------------
@pytest.fixture(scope="module")
def layout_contexts():
    """one context per pairing layout (lane pair / quad); the layout is fixed when a context is created"""
    import bls12_381_amd as b
    ctxs = {}
    for name in ("pair", "quad"):
        os.environ["BLSGPU_PAIRING_LAYOUT"] = name
        try:
            ctxs[name] = b.Context(0)
        finally:
            os.environ.pop("BLSGPU_PAIRING_LAYOUT")
    return ctxs


def test_quad_layout_miller_and_pairing_match_pair_layout_and_oracle(layout_contexts):
    """the quad kernels against (i) the oracle on a few pairs incl. identities on either side, raw Miller values and full
    pairings, (ii) the lane-pair kernels limb for limb on 4099 pairs (odd size: a partially filled last block)"""
    r = o.SplitMix64(3303)
    n = 6
    P = [o.g1_to_affine(o.g1_affine_mul(o.G1_GEN, r.scalar())) for _ in range(n)]
    Q = [o.g2_to_affine(o.g2_affine_mul(o.G2_GEN, r.scalar())) for _ in range(n)]
    P[2] = o.G1_IDENTITY_AFF; Q[4] = o.G2_IDENTITY_AFF
    g1 = np.stack([g1aff_w(p)[0] for p in P]); g1f = np.array([g1aff_w(p)[1] for p in P], dtype=np.uint8)
    g2 = np.stack([g2aff_w(q)[0] for q in Q]); g2f = np.array([g2aff_w(q)[1] for q in Q], dtype=np.uint8)
    q = layout_contexts["quad"]
    ml = q.miller_loop_batch(g1, g1f, g2, g2f)
    gt = q.pairing_batch(g1, g1f, g2, g2f)
    for i in range(n):
        ident = P[i][2] or Q[i][2]
        want_ml = o.FP12_ONE if ident else o.miller_loop(P[i], Q[i])
        assert np.array_equal(ml[i], fp12w(want_ml)), i
        assert np.array_equal(gt[i], fp12w(o.pairing(P[i], Q[i]))), i
    assert np.array_equal(q.final_exponentiation_batch(ml), gt)
    # bulk: both layouts, same inputs
    nb = 4099
    ka = [r.scalar() for _ in range(nb)]; kq = [r.scalar() for _ in range(nb)]
    p = layout_contexts["pair"]
    bxy, _ = p.bases_from_scalars(1, ka).download(); qxy, _ = p.bases_from_scalars(2, kq).download()
    assert np.array_equal(q.miller_loop_batch(bxy, None, qxy, None), p.miller_loop_batch(bxy, None, qxy, None))
    assert np.array_equal(q.pairing_batch(bxy, None, qxy, None), p.pairing_batch(bxy, None, qxy, None))


# ---- round 3: batched variable-base scalar multiplication (N in -> N out) --------------------------------------------------
def _golden_points(golden_dir, group):
    size = 96 if group == 1 else 192
    name = "g1_uncompressed_valid_test_vectors.dat" if group == 1 else "g2_uncompressed_valid_test_vectors.dat"
    raw = open(os.path.join(golden_dir, name), "rb").read()
    return [raw[i * size:(i + 1) * size] for i in range(len(raw) // size)]


@pytest.mark.parametrize("group", [1, 2])
def test_mul_batch_golden_multiples_of_the_generator(ctx, golden_dir, group):
    """the reference's golden files hold k * G for k = 0..999 (src/tests/mod.rs:3-76): mul_batch with P = G and s = k for every
    record, compared on uncompressed bytes"""
    import bls12_381_amd as b
    recs = _golden_points(golden_dir, group)
    n = len(recs)
    AffT = b.G1Affine if group == 1 else b.G2Affine
    g = AffT.generator()
    xy = np.repeat(g.xy[None, :], n, axis=0)
    out = ctx.mul_batch(group, xy, None, list(range(n)))
    axy, ainf = ctx.batch_normalize(group, out)
    for k in range(n):
        assert AffT(axy[k], bool(ainf[k])).to_uncompressed() == recs[k], k


@pytest.mark.parametrize("group,logn", [(1, 15), (2, 12)])
def test_mul_batch_random_pairs_vs_tier1_multiply(ctx, group, logn):
    """2^15 (G1) / 2^12 (G2) random (point, scalar) pairs, every output against the tier-1 C restatement of `multiply`
    (g1.rs:754-774 / g2.rs:825-845) after affine conversion; identities, s in {0, 1, r - 1} and an off-subgroup point mixed in"""
    from oracle import c_oracle
    from bls12_381_amd import synthetic as sy
    n = 1 << logn
    kb = sy.scalars(n, sy.SEED + 71 + group); sb = np.array(sy.scalars(n, sy.SEED + 73 + group), dtype=np.uint8).reshape(n, 32).copy()
    xy, inf = ctx.bases_from_scalars(group, kb).download()
    xy = xy.copy(); inf = inf.copy()
    rr = o.R_ORDER
    for j, s in enumerate((0, 1, rr - 1, 2, 1 << 254)):
        sb[j] = np.frombuffer(int(s).to_bytes(32, "little"), dtype=np.uint8)
    inf[7] = 1; xy[7] = g1aff_w(o.G1_IDENTITY_AFF)[0] if group == 1 else g2aff_w(o.G2_IDENTITY_AFF)[0]
    out = ctx.mul_batch(group, xy, inf, sb)
    axy, ainf = ctx.batch_normalize(group, out)
    want_xy, want_inf = c_oracle.mul_batch_affine(group, xy, inf, sb)
    assert np.array_equal(ainf, want_inf)
    assert np.array_equal(axy[ainf == 0], want_xy[want_inf == 0])
    assert ainf[0] == 1 and ainf[7] == 1 and ainf.sum() == 2          # s = 0 and the identity base: exactly these give the identity


@pytest.mark.parametrize("group", [1, 2])
def test_mul_batch_off_subgroup_points_and_mirror(ctx, kats, group):
    """no subgroup precondition: the reference's off-subgroup curve points times boundary scalars equal the oracle's
    double-and-add; the Python mirror's `Mul` and slice form go through the same kernel"""
    import bls12_381_amd as b
    A = _off_subgroup_points(kats, group)
    amul, toaff, enc, affw = ((o.g1_affine_mul, o.g1_to_affine, o.g1_to_uncompressed, g1aff_w) if group == 1 else
                              (o.g2_affine_mul, o.g2_to_affine, o.g2_to_uncompressed, g2aff_w))
    AffT = b.G1Affine if group == 1 else b.G2Affine
    r = o.SplitMix64(9100 + group)
    L = 0xd201000000010000 ** 2
    ss = [0, 1, 2, o.R_ORDER - 1, L, L + 1, (1 << 255) % o.R_ORDER, r.scalar(), r.scalar()]
    pts = [AffT(*affw(A))] * len(ss)
    got = AffT.mul_batch(pts, ss)
    for s, gp in zip(ss, got):
        assert gp.to_affine().to_uncompressed() == enc(toaff(amul(A, s))), s
    assert (AffT(*affw(A)) * b.Scalar(ss[-1])).to_affine().to_uncompressed() == enc(toaff(amul(A, ss[-1])))
    assert AffT.mul_batch([], []) == []


def test_fp6_ops(ctx):
    """the Fp6 layer directly: mul (fp6.rs:200-274), square (:277-291), invert (:294-312),
    mul_by_nonresidue (:139-150), frobenius_map (:154-188), the sparse mul_by_1 / mul_by_01 (:113-136); random operands plus
    0, 1 and elements with zero coefficients"""
    r = o.SplitMix64(606)

    def rnd2():
        return (rng_fp(r), rng_fp(r))

    def rnd6():
        return (rnd2(), rnd2(), rnd2())

    def w6(a):
        return np.concatenate([fp2w(c) for c in a])

    z2 = (0, 0)
    a = [rnd6() for _ in range(30)] + [o.FP6_ONE, (rnd2(), z2, z2), (z2, rnd2(), z2), (z2, z2, rnd2())]
    b = [rnd6() for _ in range(len(a))]
    A, B = np.stack([w6(x) for x in a]), np.stack([w6(x) for x in b])
    assert np.array_equal(ctx.fp6_op(0, A, B), np.stack([w6(o.fp6_mul(x, y)) for x, y in zip(a, b)]))
    assert np.array_equal(ctx.fp6_op(3, A), np.stack([w6(o.fp6_sqr(x)) for x in a]))
    assert np.array_equal(ctx.fp6_op(4, A), np.stack([w6(o.fp6_inv(x)) for x in a]))
    assert np.array_equal(ctx.fp6_op(5, A), np.stack([w6(o.fp6_mul_by_nonresidue(x)) for x in a]))
    assert np.array_equal(ctx.fp6_op(7, A), np.stack([w6(o.fp6_frobenius(x)) for x in a]))
    assert np.array_equal(ctx.fp6_op(11, A, B), np.stack([w6(o.fp6_mul_by_1(x, y[1])) for x, y in zip(a, b)]))
    assert np.array_equal(ctx.fp6_op(12, A, B), np.stack([w6(o.fp6_mul_by_01(x, y[0], y[1])) for x, y in zip(a, b)]))
    # the sparse forms agree with the dense product (fp6.rs:376-561 checks the same identities)
    assert np.array_equal(ctx.fp6_op(12, A, B), ctx.fp6_op(0, A, np.stack([w6((y[0], y[1], z2)) for y in b])))


# ---- round 3: small batches -- one pairing per workgroup (wide.hip.h) ------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 33, 1000])
def test_small_batches_take_the_wide_path_and_match_every_other_layout(ctx, layout_contexts, n):
    """pairing / Miller loop / final exponentiation batches of n <= 1024 run one item per workgroup by default; results must be
    limb-identical to the quad and lane-pair kernels (n = 1000: a batch larger than the chip holds at once) and, for the first
    items, to the oracle; identities on either side give Fp12::one()"""
    import bls12_381_amd as b
    from bls12_381_amd import synthetic as sy
    os.environ["BLSGPU_PAIRING_LAYOUT"] = "wide"
    try:
        w = b.Context(0)
    finally:
        os.environ.pop("BLSGPU_PAIRING_LAYOUT")
    assert w.pairing_layout(n) == 256 and ctx.pairing_layout(n) == 256 and ctx.pairing_layout(1 << 16) == 4      # the program file is there and taken
    ka = sy.scalars(n, sy.SEED + 900 + n); kq = sy.scalars(n, sy.SEED + 901 + n)
    g1, f1 = ctx.bases_from_scalars(1, ka).download(); g2, f2 = ctx.bases_from_scalars(2, kq).download()
    g1 = g1.copy(); g2 = g2.copy(); f1 = f1.copy(); f2 = f2.copy()
    if n >= 3:
        f1[1] = 1; f2[2] = 1
    q = layout_contexts["quad"]
    ml_w, gt_w = w.miller_loop_batch(g1, f1, g2, f2), w.pairing_batch(g1, f1, g2, f2)
    assert np.array_equal(ml_w, q.miller_loop_batch(g1, f1, g2, f2))
    assert np.array_equal(gt_w, q.pairing_batch(g1, f1, g2, f2))
    assert np.array_equal(w.final_exponentiation_batch(ml_w), gt_w)
    # the default context picks the same path by itself and agrees
    assert np.array_equal(ctx.pairing_batch(g1, f1, g2, f2), gt_w)
    assert np.array_equal(ctx.final_exponentiation_batch(ml_w), gt_w)
    if n <= 3:
        for i in range(n):
            Pi = o.G1_IDENTITY_AFF if f1[i] else (wfp(g1[i][0:6]), wfp(g1[i][6:12]), False)
            Qi = o.G2_IDENTITY_AFF if f2[i] else (wfp2(g2[i][0:12]), wfp2(g2[i][12:24]), False)
            assert np.array_equal(gt_w[i], fp12w(o.pairing(Pi, Qi)))
            assert np.array_equal(ml_w[i], fp12w(o.miller_loop(Pi, Qi)))


def test_layout_switches_at_256_and_1536_items(ctx, layout_contexts):
    """the library hands batches of up to 256 items to 1024-lane workgroups (one per CU), up to 1536 items to 512-lane workgroups
    (two per CU) and larger ones to the quad kernels: same limbs on every side of the switches (against the quad-only context)"""
    from bls12_381_amd import synthetic as sy
    assert ctx.pairing_layout(256) == 256 and ctx.pairing_layout(1536) == 256 and ctx.pairing_layout(1537) == 4
    n = 1537
    ka = sy.scalars(n, sy.SEED + 950); kq = sy.scalars(n, sy.SEED + 951)
    g1, f1 = ctx.bases_from_scalars(1, ka).download(); g2, f2 = ctx.bases_from_scalars(2, kq).download()
    q = layout_contexts["quad"]
    want = q.pairing_batch(g1, f1, g2, f2)
    assert np.array_equal(ctx.pairing_batch(g1, f1, g2, f2), want)
    for m in (256, 257, 1536):
        assert np.array_equal(ctx.pairing_batch(g1[:m], f1[:m], g2[:m], f2[:m]), want[:m]), m
    wantm = q.miller_loop_batch(g1[:300], f1[:300], g2[:300], f2[:300])
    assert np.array_equal(ctx.miller_loop_batch(g1[:300], f1[:300], g2[:300], f2[:300]), wantm)
    assert np.array_equal(ctx.final_exponentiation_batch(wantm), want[:300])
    # multi_miller_loop over a handful of terms (wide Miller values, quad product tree) + final exponentiation = product of pairings
    ml = ctx.multi_miller_loop(g1[:3], f1[:3], g2[:3], f2[:3])
    gt = ctx.final_exponentiation_batch(ml[None, :])[0]
    acc = o.FP12_ONE
    for i in range(3):
        acc = o.fp12_mul(acc, o.pairing((wfp(g1[i][0:6]), wfp(g1[i][6:12]), False), (wfp2(g2[i][0:12]), wfp2(g2[i][12:24]), False)))
    assert np.array_equal(gt, fp12w(acc))


def test_one_context_from_two_host_threads_is_refused_not_corrupted(ctx):
    """include/bls12_381_hip.h: one context per host thread.  A second thread that enters the same context while a call is in
    progress gets BLSGPU_ERR_ARG and the first call's result is what it would have been alone"""
    import threading
    import time
    import bls12_381_amd as b
    from bls12_381_amd import synthetic as sy
    c = b.Context(0)
    n = 1 << 15
    ka = sy.scalars(n, sy.SEED + 970); kq = sy.scalars(n, sy.SEED + 971)
    g1, f1 = c.bases_from_scalars(1, ka).download(); g2, f2 = c.bases_from_scalars(2, kq).download()
    want = c.pairing_batch(g1[:64], f1[:64], g2[:64], f2[:64])
    res = {}

    def long_call():
        res["gt"] = c.pairing_batch(g1, f1, g2, f2)              # ~15 ms of kernels plus the copies: the GIL is released inside

    seen = []
    t = threading.Thread(target=long_call)
    t.start()
    deadline = time.time() + 5.0
    while t.is_alive() and time.time() < deadline:
        r = int(c.lib.blsgpu_pairing_layout(c.h, 1))
        if r < 0:
            seen.append(c.lib.blsgpu_last_error())
        time.sleep(0.0005)
    t.join()
    assert seen and all(b"another host thread" in m for m in seen), "the second thread was never refused"
    assert np.array_equal(res["gt"][:64], want)
    assert c.pairing_layout(1) == 256                           # and the context works as before afterwards


# ---- round 4: segmented multi_miller_loop, device groups, diagnostics ---------------------------------------------------------
def _terms_w(ps, qs):
    G1 = np.stack([g1aff_w(p)[0] for p in ps]); F1 = np.array([g1aff_w(p)[1] for p in ps], dtype=np.uint8)
    G2 = np.stack([g2aff_w(q)[0] for q in qs]); F2 = np.array([g2aff_w(q)[1] for q in qs], dtype=np.uint8)
    return G1, F1, G2, F2


def test_multi_miller_loop_many_segments_vs_oracle(ctx):
    """N independent multi_miller_loops in one call: every segment against the oracle's `multi_miller_loop(terms)` (raw value)
    and `.final_exponentiation()`, for k in {0, 1, 2, 3, 8} terms, identities on either side, an empty first / last segment --
    pairings.rs:554-603 once per segment, `MillerLoopResult::default()` for no terms (:28-32)"""
    import bls12_381_amd as b
    ps, qs = _pair_inputs(15, 4242)
    ps[4] = o.G1_IDENTITY_AFF; qs[9] = o.G2_IDENTITY_AFF
    lens = [0, 1, 2, 3, 0, 8, 1, 0]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    assert int(off[-1]) == 15
    G1, F1, G2, F2 = _terms_w(ps, qs)
    raw = ctx.multi_miller_loop_many(G1, F1, G2, F2, off, final_exp=False)
    gt = ctx.multi_miller_loop_many(G1, F1, G2, F2, off, final_exp=True)
    for s, k in enumerate(lens):
        lo = int(off[s])
        want = o.multi_miller_loop([(p, o.g2_prepare(q)) for p, q in zip(ps[lo:lo + k], qs[lo:lo + k])])
        assert np.array_equal(raw[s], fp12w(want)), f"segment {s} (k = {k}): raw Miller value"
        assert np.array_equal(gt[s], fp12w(o.final_exponentiation(want))), f"segment {s} (k = {k}): Gt"
    assert np.array_equal(gt[0], fp12w(o.FP12_ONE))                      # Gt::identity for an empty equation
    # the mirrored API: one equation e(aG, bH) e(-abG, H) = 1 next to one that does not hold
    a, c = b.Scalar(77), b.Scalar(1234567)
    g, h = b.G1Affine.generator(), b.G2Affine.generator()
    eq_ok = [((g * a).to_affine(), b.G2Prepared((h * c).to_affine())), (-(g * (a * c)).to_affine(), b.G2Prepared(h))]
    eq_bad = [((g * a).to_affine(), b.G2Prepared((h * c).to_affine())), (-(g * a).to_affine(), b.G2Prepared(h))]
    res = b.multi_miller_loop_many([eq_ok, eq_bad, []])
    assert res[0] == b.Gt.identity() and res[1] != b.Gt.identity() and res[2] == b.Gt.identity()
    assert res[1] == b.multi_miller_loop(eq_bad).final_exponentiation()
    # nothing to do / malformed offsets
    assert ctx.multi_miller_loop_many(G1[:0], F1[:0], G2[:0], F2[:0], np.zeros(1, dtype=np.uint64)).shape == (0, 72)
    with pytest.raises(b.BlsGpuError):
        ctx.multi_miller_loop_many(G1[:3], F1[:3], G2[:3], F2[:3], np.array([0, 2, 1, 3], dtype=np.uint64))


def test_multi_miller_loop_many_2_12_equations_of_three_vs_c_oracle(ctx):
    """2^12 signature-verification-shaped equations (k = 3) on the throughput kernels, limb for limb: the C oracle's raw Miller
    values multiplied per segment by the Python oracle's Fp12 product, final exponentiation by the C oracle; plus long segments
    (the 32-run form of the segmented product) against the single-product entry point and the oracle"""
    from oracle import c_oracle
    c_oracle.build()
    nseg, k = 1 << 12, 3
    n = nseg * k
    ab, _ = _rand_scalars_np(n, 141)
    bb, _ = _rand_scalars_np(n, 142)
    g1, f1 = ctx.bases_from_scalars(1, ab).download()
    g2, f2 = ctx.bases_from_scalars(2, bb).download()
    f1 = f1.copy(); f2 = f2.copy(); f1[[5, 300]] = 1; f2[[301, 9000]] = 1
    off = (np.arange(nseg + 1) * k).astype(np.uint64)
    assert ctx.pairing_layout(n) == 4 and ctx.pairing_layout(nseg) == 4
    ml, _ = c_oracle.pairing_batch(1, g1, f1, g2, f2)
    prods = np.zeros((nseg, 72), dtype=np.uint64)
    for s in range(nseg):
        acc = wfp12(ml[3 * s])
        acc = o.fp12_mul(o.fp12_mul(acc, wfp12(ml[3 * s + 1])), wfp12(ml[3 * s + 2]))
        prods[s] = fp12w(acc)
    assert np.array_equal(ctx.multi_miller_loop_many(g1, f1, g2, f2, off, final_exp=False), prods)
    want = c_oracle.pairing_batch(2, prods, None, None, None)[0]
    assert np.array_equal(ctx.multi_miller_loop_many(g1, f1, g2, f2, off, final_exp=True), want)
    # ragged and long segments: lengths 1100 (beyond 32 x 32), 40, 0, 7 -- against blsgpu_multi_miller_loop per segment
    lens = [1100, 40, 0, 7]
    off2 = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    m = int(off2[-1])
    got = ctx.multi_miller_loop_many(g1[:m], f1[:m], g2[:m], f2[:m], off2, final_exp=False)
    for s, ln in enumerate(lens):
        lo = int(off2[s])
        assert np.array_equal(got[s], ctx.multi_miller_loop(g1[lo:lo + ln], f1[lo:lo + ln], g2[lo:lo + ln], f2[lo:lo + ln])), s
    acc = o.FP12_ONE
    for i in range(1100, 1140):
        acc = o.fp12_mul(acc, wfp12(ml[i]))
    assert np.array_equal(got[1], fp12w(acc))


@pytest.mark.parametrize("members", [2, 8])
def test_device_group_matches_single_context(ctx, members):
    """blsgpu_group: the sharded entry points of the C library (one context + one host thread per member; here `members` logical
    members on device 0, the code path of an 8-GPU node) against the single-context results -- MSMs as affine points, everything
    in Fp12 limb for limb (a product of partial products is the same field element)"""
    import bls12_381_amd as b
    from bls12_381_amd import synthetic as sy
    grp = b.Group([0] * members)
    assert len(grp) == members
    nrm = lambda g, x: ctx.batch_normalize(g, x[None, :])
    for gid, n in ((1, 5003), (2, 1001)):
        kb, sb = sy.scalars(n, 700 + gid), sy.scalars(n, 710 + gid)
        gb = grp.bases_from_scalars(gid, kb)
        assert len(gb) == n
        rb = ctx.bases_from_scalars(gid, kb)
        want = nrm(gid, ctx.msm(rb, sb))
        got = nrm(gid, grp.msm(gb, sb))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        # fewer scalars than resident bases (some members get nothing), one scalar, none
        for m in (n // 2 + 1, 1, 0):
            w2 = nrm(gid, ctx.msm(rb, sb[:m])); g2_ = nrm(gid, grp.msm(gb, sb[:m]))
            assert np.array_equal(g2_[0], w2[0]) and np.array_equal(g2_[1], w2[1]), (gid, m)
        # uploaded (not generated) bases incl. an identity: subgroup test per member
        xy, inf = rb.download(0, 300)
        inf = inf.copy(); inf[7] = 1
        ub = grp.upload_bases(gid, xy, inf)
        w3 = nrm(gid, ctx.msm(ctx.upload_bases(gid, xy, inf), sb[:300])); g3 = nrm(gid, grp.msm(ub, sb[:300]))
        assert np.array_equal(g3[0], w3[0]) and np.array_equal(g3[1], w3[1])
        gb.free(); ub.free()
    n = 37
    g1, f1 = ctx.bases_from_scalars(1, sy.scalars(n, 721)).download(); g2, f2 = ctx.bases_from_scalars(2, sy.scalars(n, 722)).download()
    f1 = f1.copy(); f1[3] = 1
    assert np.array_equal(grp.pairing_batch(g1, f1, g2, f2), ctx.pairing_batch(g1, f1, g2, f2))
    assert np.array_equal(grp.miller_loop_batch(g1, f1, g2, f2), ctx.miller_loop_batch(g1, f1, g2, f2))
    raw = ctx.multi_miller_loop(g1, f1, g2, f2)
    assert np.array_equal(grp.multi_miller_loop(g1, f1, g2, f2), raw)
    assert np.array_equal(grp.multi_miller_loop(g1, f1, g2, f2, final_exp=True), ctx.final_exponentiation_batch(raw[None, :])[0])
    for m in (3, 0):                          # fewer terms than members; no terms: MillerLoopResult::default / Gt::identity
        assert np.array_equal(grp.multi_miller_loop(g1[:m], f1[:m], g2[:m], f2[:m]), ctx.multi_miller_loop(g1[:m], f1[:m], g2[:m], f2[:m]))
    assert np.array_equal(grp.multi_miller_loop(g1[:0], f1[:0], g2[:0], f2[:0], final_exp=True), fp12w(o.FP12_ONE))
    off = np.array([0, 3, 3, 10, 11, 20, 37], dtype=np.uint64)
    assert np.array_equal(grp.multi_miller_loop_many(g1, f1, g2, f2, off), ctx.multi_miller_loop_many(g1, f1, g2, f2, off))
    # errors of a member surface with its index; the group stays usable
    bad = sy.scalars(8, 730).copy(); bad[5] = 0xFF
    gb = grp.bases_from_scalars(1, sy.scalars(8, 731))
    import ctypes
    out18 = np.zeros(18, dtype=np.uint64)
    rc = grp.lib.blsgpu_g1_msm_sharded(grp.h, gb.handle, bad.ctypes.data_as(ctypes.c_void_p), 8, out18.ctypes.data_as(ctypes.c_void_p))
    assert rc == -2 and b"group member" in grp.lib.blsgpu_last_error() and b"canonical" in grp.lib.blsgpu_last_error()
    ok = sy.scalars(8, 732)
    assert np.array_equal(nrm(1, grp.msm(gb, ok))[0], nrm(1, ctx.msm(ctx.bases_from_scalars(1, sy.scalars(8, 731)), ok))[0])
    grp.close()


def test_layout_variable_and_wide_program_diagnostics(monkeypatch, tmp_path):
    """BLSGPU_PAIRING_LAYOUT takes exact names only (a typo fails blsgpu_create instead of selecting the slowest kernels); a missing /
    stale wide program is reported by blsgpu_wide_status, and with the default layout small batches then run on the quad kernels"""
    import bls12_381_amd as b
    for bad in ("Quad", "WIDE", "wyde", "3"):
        monkeypatch.setenv("BLSGPU_PAIRING_LAYOUT", bad)
        with pytest.raises(b.BlsGpuError, match="BLSGPU_PAIRING_LAYOUT"):
            b.Context(0)
    for good, want in (("quad", 4), ("4", 4), ("pair", 2), ("auto", 256), ("wide", 256)):
        monkeypatch.setenv("BLSGPU_PAIRING_LAYOUT", good)
        c = b.Context(0)
        assert c.pairing_layout(1) == want, good
        c.close()
    monkeypatch.delenv("BLSGPU_PAIRING_LAYOUT")
    c = b.Context(0)
    assert c.wide_status() == "" and c.pairing_layout(1) == 256
    c.close()
    # a stale file: the shipped blob with another format version
    blob = bytearray(open(os.path.join(os.path.dirname(b.LIB_PATH), "wide_prog.bin"), "rb").read())
    blob[60:64] = (99).to_bytes(4, "little")
    stale = tmp_path / "stale.bin"
    stale.write_bytes(bytes(blob))
    for path, word in ((str(stale), "format version"), (str(tmp_path / "absent.bin"), "cannot be opened")):
        monkeypatch.setenv("BLSGPU_WIDE_PROG", path)
        c = b.Context(0)
        assert word in c.wide_status(), c.wide_status()
        assert c.pairing_layout(1) == 4
        g = b.G1Affine.generator(); h = b.G2Affine.generator()
        out = c.pairing_batch(g.xy[None, :], None, h.xy[None, :], None)
        assert np.array_equal(out[0], b.Gt.generator().f)           # still the right value, on the quad kernels
        c.close()
        monkeypatch.setenv("BLSGPU_PAIRING_LAYOUT", "wide")
        c = b.Context(0)
        with pytest.raises(b.BlsGpuError, match=word):
            c.pairing_layout(1)
        c.close()
        monkeypatch.delenv("BLSGPU_PAIRING_LAYOUT")


@pytest.mark.parametrize("group", [1, 2])
def test_mul_batch_endomorphism_fast_path_for_vouched_points(group):
    """blsgpu_set_assume_subgroup(1): mul_batch splits the scalars with the endomorphisms (G1: k_mul_batch_glv, 32 windows of two
    additions; G2: k_mul_batch_gls, 16 windows of four over psi) -- every output against the tier-1 C restatement of `multiply`
    (g1.rs:754-774, g2.rs:825-845) after affine conversion, on random pairs, on every branch boundary of the decomposition
    (tests/decomp_model), identities and s in {0, 1, r - 1}; and equal to the complete-formula kernel a context without the flag runs"""
    import bls12_381_amd as b
    from oracle import c_oracle
    from bls12_381_amd import synthetic as sy
    from tests import decomp_model as dm
    c_oracle.build()
    cands = dm.glv_candidates() if group == 1 else dm.gls_candidates()
    n = (1 << (13 if group == 1 else 11)) + len(cands)
    kb = sy.scalars(n, sy.SEED + 81 + group)
    sb = np.array(sy.scalars(n, sy.SEED + 83 + group), dtype=np.uint8).reshape(n, 32).copy()
    for j, s in enumerate(cands):
        sb[j] = np.frombuffer(int(s).to_bytes(32, "little"), dtype=np.uint8)
    fast = b.Context(0); fast.set_assume_subgroup(True)
    plain = b.Context(0)
    xy, inf = plain.bases_from_scalars(group, kb).download()
    xy = xy.copy(); inf = inf.copy()
    inf[len(cands) + 3] = 1; xy[len(cands) + 3] = g1aff_w(o.G1_IDENTITY_AFF)[0] if group == 1 else g2aff_w(o.G2_IDENTITY_AFF)[0]
    want_xy, want_inf = c_oracle.mul_batch_affine(group, xy, inf, sb)
    got = fast.mul_batch(group, xy, inf, sb)
    axy, ainf = fast.batch_normalize(group, got)
    assert np.array_equal(ainf, want_inf)
    assert np.array_equal(axy[ainf == 0], want_xy[want_inf == 0])
    pxy, pinf = plain.batch_normalize(group, plain.mul_batch(group, xy, inf, sb))
    assert np.array_equal(pinf, ainf) and np.array_equal(pxy[pinf == 0], axy[ainf == 0])
    # a non-canonical scalar is reported by the fast path too
    import ctypes
    bad = sb[:4].copy(); bad[2] = 0xFF
    o18 = np.zeros((4, 18 * group), dtype=np.uint64)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    fn = fast.lib.blsgpu_g1_mul_batch if group == 1 else fast.lib.blsgpu_g2_mul_batch
    assert fn(fast.h, P(np.ascontiguousarray(xy[:4])), None, P(bad), 4, P(o18)) == -2
    fast.close(); plain.close()


@pytest.mark.parametrize("group", [1, 2])
def test_fixed_base_comb_table_matches_double_and_add_and_golden(group, golden_dir):
    """blsgpu_bases_from_scalars on >= 4096 scalars takes the fixed-base comb (k_fixed_base: 32 table lookups + complete mixed
    additions): the same canonical records as the double-and-add kernel small calls run, the golden k*G files for k = 0..999, and
    plain 256-bit integers beyond r (no reduction: [k]G for the integer k, as before)"""
    import bls12_381_amd as b
    n = 4096 + 64
    ks = list(range(1000)) + [o.R_ORDER - 1, o.R_ORDER, o.R_ORDER + 5, (1 << 255) - 19, (1 << 256) - 1, 1 << 248, 255 << 248, 0x0100010001000100]
    r = o.SplitMix64(77 + group)
    while len(ks) < n:
        ks.append(r.next() | (r.next() << 64) | (r.next() << 128) | (r.next() << 192))
    kb = np.zeros((n, 32), dtype=np.uint8)
    for i, k in enumerate(ks):
        kb[i] = np.frombuffer(int(k).to_bytes(32, "little"), dtype=np.uint8)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    import ctypes
    big, small = b.Context(0), b.Context(0)

    def from_raw(c, rows):
        h = ctypes.c_void_p()
        rows = np.ascontiguousarray(rows)
        assert c.lib.blsgpu_bases_from_scalars(c.h, group, rows.ctypes.data_as(ctypes.c_void_p), rows.shape[0], ctypes.byref(h)) == 0
        return b.ResidentBases(c, h, group)
    xy, inf = from_raw(big, kb).download()                       # one call of 4160: the comb
    want_xy = np.zeros_like(xy); want_inf = np.zeros_like(inf)
    for lo in range(0, n, 1024):                                 # five calls of <= 1024: double-and-add (no table in this context)
        wx, wi = from_raw(small, kb[lo:lo + 1024]).download()
        want_xy[lo:lo + 1024] = wx; want_inf[lo:lo + 1024] = wi
    assert np.array_equal(inf, want_inf) and np.array_equal(xy, want_xy)
    assert inf[0] == 1 and inf[1001] == 1 and inf.sum() == 2     # k = 0 and k = r
    usz = 96 if group == 1 else 192
    unc = open(os.path.join(golden_dir, f"g{group}_uncompressed_valid_test_vectors.dat"), "rb").read()
    cls = b.G1Affine if group == 1 else b.G2Affine
    for k in list(range(0, 1000, 53)) + [1, 2, 999]:
        assert cls(xy[k], bool(inf[k])).to_uncompressed() == unc[usz * k:usz * (k + 1)], k
    # once the table exists, small calls use it too
    x2, i2 = from_raw(big, kb[:7]).download()
    assert np.array_equal(x2, want_xy[:7]) and np.array_equal(i2, want_inf[:7])
    big.close(); small.close()


def test_multi_miller_loop_many_shared_squarings_for_many_short_segments(ctx):
    """from 49 152 segments of at most 8 terms blsgpu_multi_miller_loop_many runs one lane pair per segment with a shared accumulator
    (k_multi_miller_seg, the reference's own schedule): the same Miller values, limb for limb, as the per-term path (forced by
    max_seg_terms = 0) -- ragged lengths 0..4 and identities included -- and as the oracle on sampled segments"""
    import torch
    from bls12_381_amd import synthetic as sy
    nseg = 49152 + 7
    rs = np.random.RandomState(5)
    lens = rs.randint(0, 5, size=nseg)
    lens[:4] = [0, 1, 4, 3]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    total = int(off[-1])
    m = 1 << 12                                                    # 2^12 distinct pairs, tiled
    g1, f1 = ctx.bases_from_scalars(1, sy.scalars(m, 801)).download(); g2, f2 = ctx.bases_from_scalars(2, sy.scalars(m, 802)).download()
    f1 = f1.copy(); f2 = f2.copy(); f1[5] = 1; f2[9] = 1
    reps = -(-total // m)
    G1 = np.tile(g1, (reps, 1))[:total]; F1 = np.tile(f1, reps)[:total]; G2 = np.tile(g2, (reps, 1))[:total]; F2 = np.tile(f2, reps)[:total]
    dev = torch.device("cuda", 0)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else np.uint8)).to(dev)
    dG1, dG2, dF1, dF2, dOff = d(G1), d(G2), d(F1), d(F2), torch.from_numpy(off).to(dev)
    outs = []
    for max_k in (4, 0):                                           # shared accumulator / per-term quads + segmented product
        o_ = torch.zeros((nseg, 72), dtype=torch.int64, device=dev)
        ctx.multi_miller_loop_many_device(dG1.data_ptr(), dG2.data_ptr(), dOff.data_ptr(), nseg, total, o_.data_ptr(), max_seg_terms=max_k, final_exp=False,
                                          d_g1_inf=dF1.data_ptr(), d_g2_inf=dF2.data_ptr())
        ctx.synchronize()
        outs.append(o_.cpu().numpy().view(np.uint64))
    assert np.array_equal(outs[0], outs[1])
    pt1 = lambda i: (wfp(G1[i][0:6]), wfp(G1[i][6:12]), bool(F1[i]))
    pt2 = lambda i: (wfp2(G2[i][0:12]), wfp2(G2[i][12:24]), bool(F2[i]))
    for s in (0, 1, 2, 3, nseg - 1):
        terms = [(pt1(i), o.g2_prepare(pt2(i))) for i in range(int(off[s]), int(off[s + 1]))]
        assert np.array_equal(outs[0][s], fp12w(o.multi_miller_loop(terms))), s
    # a bound that does not hold (a 9-term segment behind max_seg_terms = 8) is reported by the next synchronize, not computed wrong in silence
    import bls12_381_amd as b
    lens9 = np.full(nseg, 1, dtype=np.int64); lens9[100] = 9
    off9 = torch.from_numpy(np.concatenate([[0], np.cumsum(lens9)]).astype(np.int64)).to(dev)
    o9 = torch.zeros((nseg, 72), dtype=torch.int64, device=dev)
    ctx.multi_miller_loop_many_device(dG1.data_ptr(), dG2.data_ptr(), off9.data_ptr(), nseg, int(lens9.sum()), o9.data_ptr(), max_seg_terms=8, final_exp=False)
    with pytest.raises(b.BlsGpuError, match="max_seg_terms"):
        ctx.synchronize()
    ctx.synchronize()                                              # the flag is cleared by the report
    # the host entry point takes the same route (its bound is exact) and finishes with the batched final exponentiation
    gt = ctx.multi_miller_loop_many(G1, F1, G2, F2, off.astype(np.uint64), final_exp=True)
    assert np.array_equal(gt[:64], ctx.final_exponentiation_batch(outs[0][:64]))


def test_round4_entry_points_edge_cases_and_argument_errors(ctx):
    """new entry points: degenerate sizes are values (a group of one member, fewer points than members, segments that are all empty,
    no segments), bad arguments are status codes with a message, and the objects stay usable"""
    import ctypes
    import bls12_381_amd as b
    from bls12_381_amd import synthetic as sy
    lib = ctx.lib
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    ERR_ARG = -2
    # multi_miller_loop_many: all-empty segments, zero segments, NULL / malformed arguments
    z12, z24 = np.zeros((0, 12), dtype=np.uint64), np.zeros((0, 24), dtype=np.uint64)
    out = ctx.multi_miller_loop_many(z12, None, z24, None, np.zeros(4, dtype=np.uint64), final_exp=True)
    assert out.shape == (3, 72) and all(np.array_equal(v, fp12w(o.FP12_ONE)) for v in out)
    assert np.array_equal(ctx.multi_miller_loop_many(z12, None, z24, None, np.zeros(4, dtype=np.uint64), final_exp=False)[1], fp12w(o.FP12_ONE))
    off = np.array([0, 1], dtype=np.uint64); o72 = np.zeros(72, dtype=np.uint64)
    g1 = np.zeros(12, dtype=np.uint64); g2 = np.zeros(24, dtype=np.uint64)
    assert lib.blsgpu_multi_miller_loop_many(ctx.h, P(g1), None, P(g2), None, None, 1, 1, P(o72)) == ERR_ARG          # no offsets
    assert lib.blsgpu_multi_miller_loop_many(ctx.h, None, None, P(g2), None, P(off), 1, 1, P(o72)) == ERR_ARG         # terms but no points
    assert lib.blsgpu_multi_miller_loop_many(ctx.h, P(g1), None, P(g2), None, P(np.array([1, 1], dtype=np.uint64)), 1, 1, P(o72)) == ERR_ARG   # offsets[0] != 0
    assert b"offsets" in lib.blsgpu_last_error()
    assert lib.blsgpu_multi_miller_loop_many(ctx.h, None, None, None, None, None, 0, 1, None) == 0                    # nothing to do
    # groups: creation errors, one member, fewer points than members
    h = ctypes.c_void_p()
    assert lib.blsgpu_group_create(None, 2, ctypes.byref(h)) == ERR_ARG
    assert lib.blsgpu_group_create((ctypes.c_int * 1)(0), 0, ctypes.byref(h)) == ERR_ARG
    assert lib.blsgpu_group_create((ctypes.c_int * 2)(0, 4096), 2, ctypes.byref(h)) != 0 and b"member 1" in lib.blsgpu_last_error()
    assert lib.blsgpu_group_size(None) == 0 and lib.blsgpu_group_ctx(None, 0) is None
    one = b.Group([0])
    kb, sb = sy.scalars(3, 950), sy.scalars(3, 951)
    nrm = lambda x: ctx.batch_normalize(1, x[None, :])[0][0]
    want = nrm(ctx.msm(ctx.bases_from_scalars(1, kb), sb))
    assert np.array_equal(nrm(one.msm(one.bases_from_scalars(1, kb), sb)), want)
    eight = b.Group([0] * 8)
    gb = eight.bases_from_scalars(1, kb)                              # three points over eight members: five members hold nothing
    assert np.array_equal(nrm(eight.msm(gb, sb)), want)
    assert lib.blsgpu_group_ctx(eight.h, 7) is not None and lib.blsgpu_group_ctx(eight.h, 8) is None
    o18 = np.zeros(18, dtype=np.uint64)
    assert lib.blsgpu_g2_msm_sharded(eight.h, gb.handle, P(sb), 3, P(o18)) == ERR_ARG and b"other group" in lib.blsgpu_last_error()
    assert lib.blsgpu_g1_msm_sharded(eight.h, gb.handle, P(sb), 4, P(o18)) == ERR_ARG                                 # more scalars than bases
    assert lib.blsgpu_g1_msm_sharded(one.h, gb.handle, P(sb), 3, P(o18)) == ERR_ARG and b"another group" in lib.blsgpu_last_error()
    assert lib.blsgpu_pairing_batch_sharded(eight.h, None, None, None, None, 2, P(o72)) == ERR_ARG
    assert np.array_equal(nrm(eight.msm(gb, sb)), want)               # still usable
    one.close(); eight.close()


# ---- round 5: G2Prepared resident on the device ----------------------------------------------------------------------------------
def _coeffs_w(prep):
    """oracle `G2Prepared` -> (68, 3, 12) u64 in the reference's value format"""
    return np.array([[np.concatenate([fpw(c[0]), fpw(c[1])]) for c in tri] for tri in prep[1]], dtype=np.uint64)


def test_g2_prepared_table_holds_the_reference_coefficients(ctx):
    """`From<G2Affine> for G2Prepared` (pairings.rs:504-546): the device table of 1, 3 and 2^10 points holds the oracle's 68 coefficient
    triples limb for limb (sampled for the large table), the identity keeps its flag and the generator's coefficients (:506-509)"""
    ps, qs = _pair_inputs(3, 515)
    for pts in ([qs[0]], [qs[0], o.G2_IDENTITY_AFF, qs[2]]):
        G2 = np.stack([g2aff_w(q)[0] for q in pts]); F2 = np.array([g2aff_w(q)[1] for q in pts], dtype=np.uint8)
        t = ctx.g2_prepare(G2, F2)
        assert len(t) == len(pts)
        for i, q in enumerate(pts):
            inf, co = t.coeffs(i)
            want = o.g2_prepare(q)
            assert inf == bool(want[0]) and np.array_equal(co, _coeffs_w(want)), i
        t.free()
    kb, ks = _rand_scalars_np(1 << 10, 516)
    g2, f2 = ctx.bases_from_scalars(2, kb).download()
    t = ctx.g2_prepare(g2, None)
    assert len(t) == 1 << 10
    for i in (0, 1, 511, 1023):
        q = o.g2_to_affine(o.g2_affine_mul(o.G2_GEN, ks[i]))
        inf, co = t.coeffs(i)
        assert not inf and np.array_equal(co, _coeffs_w(o.g2_prepare(q))), i
    import bls12_381_amd as b
    with pytest.raises(b.BlsGpuError):
        t.coeffs(1 << 10)
    assert len(ctx.g2_prepare(g2[:0], None)) == 0


def test_multi_miller_loop_prepared_matches_unprepared_and_oracle(ctx):
    """`multi_miller_loop(&[(&G1Affine, &G2Prepared)])` (pairings.rs:554-603) with prepared, unprepared and identity terms mixed: raw
    Miller values limb-identical to the oracle's multi_miller_loop over `g2_prepare`d points and to the unprepared entry points, for one
    product and for segments of 0, 1, 2, 3, 8 and 11 terms (more than one pass); argument errors; the mirrored `G2Prepared.resident`"""
    import bls12_381_amd as b
    ps, qs = _pair_inputs(25, 5151)
    ps[4] = o.G1_IDENTITY_AFF; qs[9] = o.G2_IDENTITY_AFF
    fixed = [qs[20], o.G2_IDENTITY_AFF, qs[21], qs[22]]                       # the "verification key": table entries 0..3 (1 = identity)
    TG = np.stack([g2aff_w(q)[0] for q in fixed]); TF = np.array([g2aff_w(q)[1] for q in fixed], dtype=np.uint8)
    table = ctx.g2_prepare(TG, TF)
    n = 15
    qi = np.full(n, b.UNPREPARED, dtype=np.uint32)
    qi[[1, 2, 5, 6, 7, 10, 14]] = [0, 2, 3, 1, 0, 2, 3]
    eff_q = [fixed[int(k)] if k != b.UNPREPARED else qs[i] for i, k in enumerate(qi)]
    G1, F1, G2, F2 = _terms_w(ps[:n], qs[:n])
    # one product
    want = o.multi_miller_loop([(p, o.g2_prepare(q)) for p, q in zip(ps[:n], eff_q)])
    got = ctx.multi_miller_loop_prepared(G1, F1, table, qi, G2, F2)
    assert np.array_equal(got, fp12w(want))
    EG2, EF2 = np.stack([g2aff_w(q)[0] for q in eff_q]), np.array([g2aff_w(q)[1] for q in eff_q], dtype=np.uint8)
    assert np.array_equal(got, ctx.multi_miller_loop(G1, F1, EG2, EF2))
    # all prepared, no g2 array at all; all unprepared through the same kernel (q_index = None)
    allp = np.array([0, 2, 3, 0, 2], dtype=np.uint32)
    w2 = o.multi_miller_loop([(p, o.g2_prepare(fixed[int(k)])) for p, k in zip(ps[:5], allp)])
    assert np.array_equal(ctx.multi_miller_loop_prepared(G1[:5], F1[:5], table, allp), fp12w(w2))
    assert np.array_equal(ctx.multi_miller_loop_prepared(G1, F1, None, None, G2, F2), ctx.multi_miller_loop(G1, F1, G2, F2))
    assert np.array_equal(ctx.multi_miller_loop_prepared(G1[:0], F1[:0], table, qi[:0]), fp12w(o.FP12_ONE))
    # segments
    lens = [0, 1, 2, 3, 0, 8, 1, 0]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    raw = ctx.multi_miller_loop_prepared_many(G1, F1, table, qi, off, G2, F2, final_exp=False)
    gt = ctx.multi_miller_loop_prepared_many(G1, F1, table, qi, off, G2, F2, final_exp=True)
    assert np.array_equal(raw, ctx.multi_miller_loop_many(G1, F1, EG2, EF2, off, final_exp=False))
    for s, k in enumerate(lens):
        lo = int(off[s])
        w = o.multi_miller_loop([(p, o.g2_prepare(q)) for p, q in zip(ps[lo:lo + k], eff_q[lo:lo + k])])
        assert np.array_equal(raw[s], fp12w(w)), s
        assert np.array_equal(gt[s], fp12w(o.final_exponentiation(w))), s
    off11 = np.array([0, 11, 15], dtype=np.uint64)                           # 11 terms: two passes of the shared loop, multiplied in the kernel
    raw11 = ctx.multi_miller_loop_prepared_many(G1, F1, table, qi, off11, G2, F2, final_exp=False)
    assert np.array_equal(raw11, ctx.multi_miller_loop_many(G1, F1, EG2, EF2, off11, final_exp=False))
    # the same over a device group (the table on every member, terms / segments in contiguous slices, ONE final exponentiation)
    for members in (2, 3):
        grp = b.Group([0] * members)
        gtab = grp.g2_prepare(TG, TF)
        assert len(gtab) == 4
        assert np.array_equal(grp.multi_miller_loop_prepared(G1, F1, gtab, qi, G2, F2), got)
        assert np.array_equal(grp.multi_miller_loop_prepared(G1, F1, gtab, qi, G2, F2, final_exp=True), fp12w(o.final_exponentiation(want)))
        assert np.array_equal(grp.multi_miller_loop_prepared_many(G1, F1, gtab, qi, off, G2, F2, final_exp=True), gt)
        assert np.array_equal(grp.multi_miller_loop_prepared_many(G1, F1, gtab, qi, off, G2, F2, final_exp=False), raw)
        gtab.free(); grp.close()
    # argument errors: index outside the table, an unprepared term without g2, indices without a table
    bad = qi.copy(); bad[3] = 4
    for args in ((G1, F1, table, bad, G2, F2), (G1, F1, table, qi, None, None), (G1, F1, None, qi, G2, F2)):
        with pytest.raises(b.BlsGpuError):
            ctx.multi_miller_loop_prepared(*args)
    # the mirror: e(aG, bH) e(-abG, H) = 1 with H resident
    a, c = b.Scalar(77), b.Scalar(1234567)
    g, h = b.G1Affine.generator(), b.G2Affine.generator()
    hp, hcp = b.G2Prepared.resident_many([h, (h * c).to_affine()])
    assert np.array_equal(hp.coeffs()[1], _coeffs_w(o.g2_prepare(o.G2_GEN)))
    eq_ok = [((g * a).to_affine(), hcp), (-(g * (a * c)).to_affine(), hp)]
    eq_mixed = [((g * a).to_affine(), b.G2Prepared((h * c).to_affine())), (-(g * a).to_affine(), hp)]
    assert b.multi_miller_loop(eq_ok).final_exponentiation() == b.Gt.identity()
    res = b.multi_miller_loop_many([eq_ok, eq_mixed, []])
    assert res[0] == b.Gt.identity() and res[1] != b.Gt.identity() and res[2] == b.Gt.identity()
    plain = [(p, b.G2Prepared(pr.q)) for p, pr in eq_mixed]
    assert res[1] == b.multi_miller_loop(plain).final_exponentiation()
    table.free()


def test_prepared_equations_2_12_vs_c_oracle_and_device_pointers(ctx):
    """2^12 verification-shaped equations e(A_i, B_i) e(C_i, K0) e(D_i, K1) with K0, K1 prepared, on the throughput kernel through the
    device-pointer entry point: equal to the unprepared path limb for limb and to the C oracle's Miller values multiplied per segment;
    2^15 terms of one long product (K > 1 runs + product tree) against the unprepared product; a bad index is reported by synchronize"""
    import torch
    import bls12_381_amd as b
    from oracle import c_oracle
    c_oracle.build()
    dev = torch.device("cuda", 0)
    nseg, k = 1 << 12, 3
    n = nseg * k
    ab, _ = _rand_scalars_np(n, 551)
    bb, _ = _rand_scalars_np(n, 552)
    g1, f1 = ctx.bases_from_scalars(1, ab).download()
    g2, f2 = ctx.bases_from_scalars(2, bb).download()
    kk, _ = _rand_scalars_np(2, 553)
    key, _ = ctx.bases_from_scalars(2, kk).download()
    qi = np.full(n, b.UNPREPARED, dtype=np.uint32); qi[1::3] = 0; qi[2::3] = 1
    eff = g2.copy(); eff[1::3] = key[0]; eff[2::3] = key[1]
    off = (np.arange(nseg + 1) * k).astype(np.uint64)
    table = ctx.g2_prepare(key, None)
    t = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)
    d_g1, d_g2, d_qi, d_off = t(g1), t(g2), t(qi.view(np.int32)), t(off)
    d_out = torch.zeros((nseg, 72), dtype=torch.int64, device=dev)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        ctx.multi_miller_loop_prepared_many_device(d_g1.data_ptr(), table, d_qi.data_ptr(), d_off.data_ptr(), nseg, n, d_out.data_ptr(), max_seg_terms=k, final_exp=False,
                                                   d_g2=d_g2.data_ptr())
        ctx.synchronize()
        raw = d_out.cpu().numpy().view(np.uint64)
        ml, _ = c_oracle.pairing_batch(1, g1, np.zeros(n, dtype=np.uint8), eff, np.zeros(n, dtype=np.uint8))
        for s in (0, 1, 777, nseg - 1):
            acc = o.fp12_mul(o.fp12_mul(wfp12(ml[3 * s]), wfp12(ml[3 * s + 1])), wfp12(ml[3 * s + 2]))
            assert np.array_equal(raw[s], fp12w(acc)), s
        assert np.array_equal(raw, ctx.multi_miller_loop_many(g1, None, eff, None, off, final_exp=False))
        ctx.multi_miller_loop_prepared_many_device(d_g1.data_ptr(), table, d_qi.data_ptr(), d_off.data_ptr(), nseg, n, d_out.data_ptr(), max_seg_terms=k, final_exp=True,
                                                   d_g2=d_g2.data_ptr())
        ctx.synchronize()
        want = c_oracle.pairing_batch(2, raw, None, None, None)[0]
        assert np.array_equal(d_out.cpu().numpy().view(np.uint64), want)
        # one long product: 2^15 terms (12 288 of ours tiled) -> K = 1 quads ... force K > 1 with 2^17 terms
        reps = 11
        big1, big2, bigq = np.tile(g1, (reps, 1)), np.tile(g2, (reps, 1)), np.tile(qi, reps)
        bige = np.tile(eff, (reps, 1))
        got = ctx.multi_miller_loop_prepared(big1, None, table, bigq, big2, None)
        assert np.array_equal(got, ctx.multi_miller_loop(big1, None, bige, None))
        # a bad index on the device-pointer path: skipped term, sticky flag
        badq = qi.copy(); badq[4] = 7
        d_bq = t(badq.view(np.int32))
        ctx.multi_miller_loop_prepared_many_device(d_g1.data_ptr(), table, d_bq.data_ptr(), d_off.data_ptr(), nseg, n, d_out.data_ptr(), max_seg_terms=k, final_exp=False,
                                                   d_g2=d_g2.data_ptr())
        with pytest.raises(b.BlsGpuError):
            ctx.synchronize()
        ctx.synchronize()                                                    # cleared
    finally:
        ctx.set_stream(None)
        table.free()



# ---- round 5: the widened rows with device pointers, bulk verification from bytes -------------------------------------------------
def test_device_twins_of_the_widened_rows_match_their_host_forms_on_canonical_scalars(ctx):
    """blsgpu_g{1,2}_batch_normalize_device, *_from_bytes_batch_device, *_to_bytes_batch_device, blsgpu_gt_mul_scalar_batch_device and
    blsgpu_gt_is_identity_device against their (oracle-checked) host-pointer twins: hash-to-curve -> normalise -> encode -> decode ->
    Miller loop -> identity test without leaving the device.  The Gt scalars are canonical; a scalar >= r is rejected by both twins
    (tests/test_scalar_contract.py)"""
    import torch
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        for group in (1, 2):
            n = 5000 if group == 1 else 300                                  # both normalisation kernels (Montgomery's trick from 4 096 points on)
            kb, _ = _rand_scalars_np(n, 700 + group)
            kb[3] = 0                                                        # an identity
            xy, inf = ctx.bases_from_scalars(group, kb).download()
            w = 6 if group == 1 else 12                                      # u64 per coordinate
            xyz = np.zeros((n, 3 * w), dtype=np.uint64)                      # (x z : y z : z) with z = another point's y (never zero)
            z = np.roll(xy[:, w:], 1, axis=0).copy()
            mul = ctx.fp_op if group == 1 else ctx.fp2_op
            xyz[:, :w] = mul(0, xy[:, :w].copy(), z); xyz[:, w:2 * w] = mul(0, xy[:, w:].copy(), z); xyz[:, 2 * w:] = z
            xyz[inf != 0, 2 * w:] = 0
            hx, hi = ctx.batch_normalize(group, xyz)
            d_xy = torch.zeros((n, 2 * w), dtype=torch.int64, device=dev); d_inf = torch.zeros(n, dtype=torch.uint8, device=dev)
            d_xyz = t(xyz)
            ctx.batch_normalize_device(group, d_xyz.data_ptr(), n, d_xy.data_ptr(), d_inf.data_ptr())
            ctx.synchronize()
            assert np.array_equal(d_xy.cpu().numpy().view(np.uint64), hx) and np.array_equal(d_inf.cpu().numpy(), hi)
            assert np.array_equal(hx, xy) and np.array_equal(hi, inf)
            for compressed in (True, False):
                cb = (48 if group == 1 else 96) * (1 if compressed else 2)
                enc = ctx.points_to_bytes(group, xy, inf, compressed=compressed)
                d_enc = torch.zeros((n, cb), dtype=torch.uint8, device=dev)
                ctx.points_to_bytes_device(group, d_xy.data_ptr(), d_inf.data_ptr(), n, d_enc.data_ptr(), compressed=compressed)
                ctx.synchronize()
                assert np.array_equal(d_enc.cpu().numpy(), enc)
                bad = enc.copy(); bad[7, 5] ^= 0x55                            # a corrupted record (rejected or another point: the twins must agree)
                d_bad = t(bad)
                d_x2 = torch.zeros((n, 2 * w), dtype=torch.int64, device=dev); d_i2 = torch.zeros(n, dtype=torch.uint8, device=dev); d_ok = torch.zeros(n, dtype=torch.uint8, device=dev)
                ctx.points_from_bytes_device(group, d_bad.data_ptr(), n, d_x2.data_ptr(), d_i2.data_ptr(), d_ok.data_ptr(), compressed=compressed, checked=True)
                ctx.synchronize()
                hx2, hi2, hok = ctx.points_from_bytes(group, bad, compressed=compressed, checked=True)
                ok = d_ok.cpu().numpy()
                assert np.array_equal(ok, hok) and np.array_equal(d_i2.cpu().numpy()[ok != 0], hi2[hok != 0])
                assert np.array_equal(d_x2.cpu().numpy().view(np.uint64)[ok != 0], hx2[hok != 0])
        # Gt: scalar multiples and the identity test on the device
        gen = fp12w(o.pairing(o.G1_GEN, o.G2_GEN))
        ss = [0, 1, o.R_ORDER - 1, 12345, 0]                                 # g^0 = identity
        sb = np.stack([np.frombuffer((s % (1 << 256)).to_bytes(32, "little"), dtype=np.uint8) for s in ss])
        G = np.stack([gen] * len(ss))
        d_o = torch.zeros((len(ss), 72), dtype=torch.int64, device=dev); d_f = torch.zeros(len(ss), dtype=torch.uint8, device=dev)
        d_G, d_sb = t(G), t(sb)
        ctx.gt_mul_scalar_batch_device(d_G.data_ptr(), d_sb.data_ptr(), len(ss), d_o.data_ptr())
        ctx.gt_is_identity_device(d_o.data_ptr(), len(ss), d_f.data_ptr())
        ctx.synchronize()
        assert np.array_equal(d_o.cpu().numpy().view(np.uint64)[:4], ctx.gt_mul_scalar_batch(G[:4], ss[:4]))
        assert d_f.cpu().numpy().tolist() == [1, 0, 0, 0, 1]
    finally:
        ctx.set_stream(None)


@pytest.mark.parametrize("mode", [0, 1])
def test_bls_verify_batch_from_bytes_vs_oracle(ctx, mode):
    """Bulk verification, bytes in -> verdict bytes out (blsgpu_bls_verify_batch): 257 signatures (mode 0: public keys in G1, mode 1: in
    G2), a few tampered in every way the chain distinguishes -- wrong message, wrong key, a signature that is not a curve point, a key
    outside the subgroup, identity key and signature -- against (i) verdicts computed by the ORACLE on a sample (hash_to_curve, decoders
    and `pairing` of oracle/), (ii) the C oracle's pairings of the decoded points for every entry"""
    from oracle import h2c_ref as h
    from oracle import c_oracle
    c_oracle.build()
    n = 257
    dst = b"BLS_SIG_BLS12381G%d_XMD:SHA-256_SSWU_RO_NUL_" % (2 if mode == 0 else 1)
    rs = np.random.RandomState(900 + mode)
    msgs = [bytes(rs.randint(0, 256, size=int(rs.randint(0, 80)), dtype=np.uint8)) for _ in range(n)]
    skb, sks = _rand_scalars_np(n, 910 + mode)
    gk, gs = (1, 2) if mode == 0 else (2, 1)                                 # group of the keys / of the signatures
    pk_xy, pk_inf = ctx.bases_from_scalars(gk, skb).download()
    hm = ctx.hash_to_curve(gs, msgs, dst)                                    # (oracle-checked in test_hash_to_curve_vs_oracle)
    hxy, hinf = ctx.batch_normalize(gs, hm)
    sig_xyz = ctx.mul_batch(gs, hxy, hinf, skb)                              # sig_i = sk_i * H(m_i)
    sig_xy, sig_inf = ctx.batch_normalize(gs, sig_xyz)
    pk_b = ctx.points_to_bytes(gk, pk_xy, pk_inf, compressed=True).copy()
    sig_b = ctx.points_to_bytes(gs, sig_xy, sig_inf, compressed=True).copy()
    msgs = list(msgs)
    expect = np.ones(n, dtype=np.uint8)
    msgs[5] = msgs[5] + b"!"; expect[5] = 0                                  # wrong message
    pk_b[9] = pk_b[10]; expect[9] = 0                                        # someone else's key
    sig_b[20] = sig_b[21]; expect[20] = 0                                    # someone else's signature
    ident = lambda size: np.array([0xC0] + [0] * (size - 1), dtype=np.uint8)
    pk_b[30] = ident(pk_b.shape[1]); expect[30] = 0                          # identity key with an honest signature: e(O, H) e(-G, sig) != 1
    pk_b[31] = ident(pk_b.shape[1]); sig_b[31] = ident(sig_b.shape[1]); expect[31] = 1      # both identities: the equation holds (the caller's KeyValidate rejects it)
    # a signature / key that is not a valid encoding: flip bits until the checked decoder of the HOST twin rejects it
    for idx, arr, code, grp in ((40, sig_b, 3, gs), (41, pk_b, 2, gk)):
        for bit in range(8, 64):
            cand = arr[idx].copy(); cand[bit // 8 + 1] ^= 1 << (bit % 8)
            if not ctx.points_from_bytes(grp, cand[None, :], compressed=True, checked=True)[2][0]:
                arr[idx] = cand; expect[idx] = code
                break
        assert expect[idx] == code
    got = ctx.bls_verify_batch(mode, pk_b, sig_b, msgs, dst)
    assert got.tolist() == expect.tolist()
    # (i) the oracle on a sample: decode, hash, pair
    dec_g1 = o.g1_from_compressed; dec_g2 = o.g2_from_compressed
    for i in (0, 5, 9, 30, 31, 40, 41, 256):
        if mode == 0:
            pk, sg = dec_g1(pk_b[i].tobytes()), dec_g2(sig_b[i].tobytes())
        else:
            pk, sg = dec_g2(pk_b[i].tobytes()), dec_g1(sig_b[i].tobytes())
        if pk is None:
            want = 2
        elif sg is None:
            want = 3
        elif mode == 0:
            want = int(o.pairing(pk, o.g2_to_affine(h.g2_hash_to_curve(msgs[i], dst))) == o.pairing(o.G1_GEN, sg))
        else:
            want = int(o.pairing(sg, o.G2_GEN) == o.pairing(o.g1_to_affine(h.g1_hash_to_curve(msgs[i], dst)), pk))
        assert got[i] == want, (i, want)
    # (ii) every entry with valid encodings: e(pk, H(m)) == e(G, sig) by the C oracle on the host twins' decoded points
    pxy, pinf, pok = ctx.points_from_bytes(gk, pk_b, compressed=True, checked=True)
    sxy, sinf, sok = ctx.points_from_bytes(gs, sig_b, compressed=True, checked=True)
    hm2 = ctx.batch_normalize(gs, ctx.hash_to_curve(gs, msgs, dst))
    gen1 = np.tile(g1aff_w(o.G1_GEN)[0], (n, 1)); gen2 = np.tile(g2aff_w(o.G2_GEN)[0], (n, 1)); z = np.zeros(n, dtype=np.uint8)
    if mode == 0:
        lhs = c_oracle.pairing_batch(0, pxy, pinf, hm2[0], hm2[1])[0]; rhs = c_oracle.pairing_batch(0, gen1, z, sxy, sinf)[0]
    else:
        lhs = c_oracle.pairing_batch(0, sxy, sinf, gen2, z)[0]; rhs = c_oracle.pairing_batch(0, hm2[0], hm2[1], pxy, pinf)[0]
    valid = (pok != 0) & (sok != 0)
    want_all = np.where(pok == 0, 2, np.where(sok == 0, 3, (lhs == rhs).all(axis=1).astype(np.uint8)))
    assert np.array_equal(got, want_all.astype(np.uint8)) and valid.sum() == n - 2
    assert ctx.bls_verify_batch(mode, pk_b[:0], sig_b[:0], [], dst).shape == (0,)


@pytest.mark.parametrize("members", [1, 3, 8])
def test_device_group_pipelined_device_pointer_msms(ctx, members):
    """the asynchronous group path (blsgpu_g{1,2}_msm_sharded_device + blsgpu_g{1,2}_partials_fold, persistent worker threads, pipelining
    on): six MSMs with different scalars in flight over logical members on device 0, every folded result against the single-context MSM
    and the discrete-log identity; group_synchronize reports a non-canonical scalar of an asynchronous call"""
    import torch
    import bls12_381_amd as b
    from bls12_381_amd import synthetic as sy
    dev = torch.device("cuda", 0)
    grp = b.Group([0] * members)
    grp.set_pipelining(True)
    for gid, n in ((1, 20011), (2, 3001)):
        sizes = grp.shard_sizes(n)
        kb = sy.scalars(n, 800 + gid)
        gb = grp.bases_from_scalars(gid, kb)
        single = ctx.bases_from_scalars(gid, kb)
        sets = [sy.scalars(n, 810 + gid + 10 * j) for j in range(6)]
        lo = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
        d_s = [[torch.from_numpy(sets[j][lo[k]:lo[k + 1]].copy()).to(dev) for k in range(members)] for j in range(6)]
        w = 18 if gid == 1 else 36
        d_o = [[torch.zeros(w, dtype=torch.int64, device=dev) for _ in range(members)] for _ in range(4)]
        torch.cuda.synchronize()
        got = []
        for j in range(6):
            grp.msm_sharded_device(gb, [t.data_ptr() for t in d_s[j]], [t.data_ptr() for t in d_o[j & 3]])
            if j >= 2:
                got.append(grp.partials_fold(gid, [t.data_ptr() for t in d_o[(j - 2) & 3]], lag=2))
        got.append(grp.partials_fold(gid, [t.data_ptr() for t in d_o[4 & 3]], lag=1))
        got.append(grp.partials_fold(gid, [t.data_ptr() for t in d_o[5 & 3]], lag=0))
        grp.synchronize()
        for j in range(6):
            a = ctx.batch_normalize(gid, got[j][None, :]); want = ctx.batch_normalize(gid, ctx.msm(single, sets[j])[None, :])
            assert np.array_equal(a[0], want[0]) and np.array_equal(a[1], want[1]), (gid, j)
        tot = sy.dot_mod_r(kb, sets[3])
        ref = ctx.bases_from_scalars(gid, [tot]).download()
        a = ctx.batch_normalize(gid, got[3][None, :])
        assert np.array_equal(a[0][0], ref[0][0]) and a[1][0] == ref[1][0]
        # the same with the fold queued on the device (no host round trip): nine MSMs, every fold lagging two calls behind
        d_f = [torch.zeros(w, dtype=torch.int64, device=dev) for _ in range(9)]
        for j in range(9):
            grp.msm_sharded_device(gb, [t.data_ptr() for t in d_s[j % 6]], [t.data_ptr() for t in d_o[j & 3]])
            if j >= 2:
                grp.partials_fold_device(gid, [t.data_ptr() for t in d_o[(j - 2) & 3]], d_f[j - 2].data_ptr(), lag=2)
        grp.partials_fold_device(gid, [t.data_ptr() for t in d_o[7 & 3]], d_f[7].data_ptr(), lag=1)
        grp.partials_fold_device(gid, [t.data_ptr() for t in d_o[8 & 3]], d_f[8].data_ptr(), lag=0)
        grp.synchronize()
        for j in range(9):
            a = ctx.batch_normalize(gid, d_f[j].cpu().numpy().view(np.uint64)[None, :]); want = ctx.batch_normalize(gid, got[j % 6][None, :])
            assert np.array_equal(a[0], want[0]) and np.array_equal(a[1], want[1]), (gid, j)
        if gid == 1:
            bad = sets[0].copy(); bad[lo[members - 1]] = 0xFF                    # >= r, in the last member's slice
            d_bad = [torch.from_numpy(bad[lo[k]:lo[k + 1]].copy()).to(dev) for k in range(members)]
            grp.msm_sharded_device(gb, [t.data_ptr() for t in d_bad], [t.data_ptr() for t in d_o[0]])
            with pytest.raises(b.BlsGpuError, match="group member %d" % (members - 1)):
                grp.synchronize()
            grp.synchronize()
        gb.free()
    grp.close()


def test_bases_cache_for_repeated_one_shot_msms(kats):
    """blsgpu_set_bases_cache: the same base array passed to the one-shot entry point again -- first sight one-shot (untested, plain
    windows), second sight resident (tested, endomorphism images), later calls reuse it -- always the reference's group element, also for
    a set with a point outside the subgroup (resident state 0: plain windows), another array of the same length, eviction, switching off"""
    import bls12_381_amd as b
    c = b.Context(0)
    c.set_bases_cache(2)
    n = 3000
    kb, ks = _rand_scalars_np(n, 1201)
    xy, inf = c.bases_from_scalars(1, kb).download()
    want_for = lambda ss: g1aff_w(o.g1_to_affine(o.g1_affine_mul(o.G1_GEN, sum(k * s for k, s in zip(ks, ss)) % o.R_ORDER)))
    for call in range(4):
        sb, ss = _rand_scalars_np(n, 1210 + call)
        got = c.batch_normalize(1, c.msm_host(1, xy, inf, sb)[None, :])
        ex, ei = want_for(ss)
        assert np.array_equal(got[0][0], ex) and got[1][0] == ei, call
    # another array of the same length (different fingerprint), then the first again; a third array evicts the least recently used
    kb2, ks2 = _rand_scalars_np(n, 1202)
    xy2, inf2 = c.bases_from_scalars(1, kb2).download()
    sb, ss = _rand_scalars_np(n, 1220)
    for arr, keys in ((xy2, ks2), (xy2, ks2), (xy, ks), (xy2, ks2)):
        got = c.batch_normalize(1, c.msm_host(1, arr, None, sb)[None, :])
        tot = sum(k * s for k, s in zip(keys, ss)) % o.R_ORDER
        ex, ei = g1aff_w(o.g1_to_affine(o.g1_affine_mul(o.G1_GEN, tot)))
        assert np.array_equal(got[0][0], ex) and got[1][0] == ei
    # a set with an off-subgroup point: the resident form falls back to plain windows and stays exact (reference `multiply` + Sum)
    off = _off_subgroup_points(kats, 1)
    xy3 = xy.copy(); xy3[7] = g1aff_w(off)[0]
    small = 1100
    sb3, ss3 = _rand_scalars_np(small, 1230)
    want = o.g1_to_affine(o.g1_msm([off if i == 7 else o.g1_to_affine(o.g1_affine_mul(o.G1_GEN, ks[i])) for i in range(16)], ss3[:16]))
    for _ in range(3):
        got = c.batch_normalize(1, c.msm_host(1, np.concatenate([xy3[:16], np.tile(xy3[:1], (small - 16, 1))]), None,
                                              np.concatenate([sb3[:16], np.zeros((small - 16, 32), dtype=np.uint8)]))[None, :])
        assert np.array_equal(got[0][0], g1aff_w(want)[0])
    c.set_bases_cache(0)
    got = c.batch_normalize(1, c.msm_host(1, xy, inf, sb)[None, :])
    tot = sum(k * s for k, s in zip(ks, ss)) % o.R_ORDER
    assert np.array_equal(got[0][0], g1aff_w(o.g1_to_affine(o.g1_affine_mul(o.G1_GEN, tot)))[0])
    c.close()


def test_bases_cache_verify_mode_sees_a_mutated_buffer():
    """blsgpu_set_bases_cache_verify: an array is recognised by a hash of EVERY word, so a caller that reuses a buffer and changes a point
    the 65-point fingerprint does not sample gets the MSM over the NEW contents (the default mode would silently serve the stale resident set --
    the documented hazard, shown here too so that the documentation stays honest)"""
    import bls12_381_amd as b
    n = 4096
    kb, ks = _rand_scalars_np(n, 1301)
    sb, ss = _rand_scalars_np(n, 1302)
    want = lambda keys: g1aff_w(o.g1_to_affine(o.g1_affine_mul(o.G1_GEN, sum(k * s for k, s in zip(keys, ss)) % o.R_ORDER)))[0]
    for verify in (True, False):
        c = b.Context(0)
        c.set_bases_cache(2)
        c.set_bases_cache_verify(verify)
        xy, inf = c.bases_from_scalars(1, kb).download()
        for _ in range(3):                                   # first sight, resident upload, cached
            assert np.array_equal(c.batch_normalize(1, c.msm_host(1, xy, inf, sb)[None, :])[0][0], want(ks))
        # position 5 lies between the sampled positions (step n / 64 = 64): replace it by another multiple of the generator
        ks2 = list(ks); ks2[5] = 0xABCDEF
        xy[5] = g1aff_w(o.g1_to_affine(o.g1_affine_mul(o.G1_GEN, ks2[5])))[0]
        got = c.batch_normalize(1, c.msm_host(1, xy, inf, sb)[None, :])[0][0]
        if verify:
            assert np.array_equal(got, want(ks2))
        else:
            assert np.array_equal(got, want(ks))             # stale: the hazard include/bls12_381_hip.h warns about
        c.close()


def test_prepared_equations_full_size_2_16_bilinearity(ctx):
    """2^16 verification-shaped equations at the bench's size through the prepared path, checked by a size-independent property:
    e(a_i G1, [k1] G2) e(b_i G1, [k2] G2) e(-(a_i k1 + b_i k2) G1, G2) = 1 for every i (bilinearity), with [k1] G2 and [k2] G2 prepared and
    the generator unprepared; one tampered equation must fail.  Everything stays on the device (blsgpu_gt_is_identity_device)."""
    import torch
    import bls12_381_amd as b
    from bls12_381_amd import synthetic as sy
    dev = torch.device("cuda", 0)
    ne = 1 << 16
    k1, k2 = 0x1234567890ABCDEF1234567, 0x0FEDCBA987654321FEDCBA9
    ab = sy.scalars(ne, 5501); bb = sy.scalars(ne, 5502)
    ai = np.array(sy.to_ints(ab), dtype=object); bi = np.array(sy.to_ints(bb), dtype=object)
    ci = (-(ai * k1 + bi * k2)) % o.R_ORDER
    cb = np.frombuffer(b"".join(int(c).to_bytes(32, "little") for c in ci), dtype=np.uint8).reshape(ne, 32)
    pa, _ = ctx.bases_from_scalars(1, ab).download(); pb, _ = ctx.bases_from_scalars(1, bb).download(); pc, _ = ctx.bases_from_scalars(1, cb).download()
    g1 = np.empty((3 * ne, 12), dtype=np.uint64); g1[0::3] = pa; g1[1::3] = pb; g1[2::3] = pc
    key, _ = ctx.bases_from_scalars(2, [k1, k2]).download()
    gen2 = g2aff_w(o.G2_GEN)[0]
    g2 = np.zeros((3 * ne, 24), dtype=np.uint64); g2[2::3] = gen2
    qi = np.zeros(3 * ne, dtype=np.uint32); qi[1::3] = 1; qi[2::3] = b.UNPREPARED
    g1[3 * 777] = pa[778]                                            # one tampered equation
    table = ctx.g2_prepare(key, None)
    t = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)
    d_g1, d_g2, d_qi = t(g1), t(g2), t(qi.view(np.int32))
    d_off = torch.arange(0, 3 * (ne + 1), 3, dtype=torch.int64, device=dev)
    d_gt = torch.zeros((ne, 72), dtype=torch.int64, device=dev); d_fl = torch.zeros(ne, dtype=torch.uint8, device=dev)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        ctx.multi_miller_loop_prepared_many_device(d_g1.data_ptr(), table, d_qi.data_ptr(), d_off.data_ptr(), ne, 3 * ne, d_gt.data_ptr(), max_seg_terms=3, final_exp=True,
                                                   d_g2=d_g2.data_ptr())
        ctx.gt_is_identity_device(d_gt.data_ptr(), ne, d_fl.data_ptr())
        ctx.synchronize()
    finally:
        ctx.set_stream(None)
    fl = d_fl.cpu().numpy()
    assert fl[777] == 0 and fl.sum() == ne - 1
    table.free()


def test_device_group_on_distinct_physical_devices(ctx):
    """the group paths with members on DIFFERENT GPUs (peer copies and events across devices in the asynchronous fold): skipped on a
    one-GPU box -- the build box and the driver's GPU test box have one GPU, so this runs only where a multi-GPU node executes the suite"""
    import torch
    import bls12_381_amd as b
    from bls12_381_amd import synthetic as sy
    nd = torch.cuda.device_count()
    if nd < 2:
        pytest.skip("needs at least two GPUs")
    devs = list(range(min(nd, 8)))
    grp = b.Group(devs)
    grp.set_pipelining(True)
    n = 40001
    kb = sy.scalars(n, 8801)
    gb = grp.bases_from_scalars(1, kb)
    single = ctx.bases_from_scalars(1, kb)
    sizes = grp.shard_sizes(n)
    lo = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    sets = [sy.scalars(n, 8810 + j) for j in range(5)]
    d_s = [[torch.from_numpy(sets[j][lo[k]:lo[k + 1]].copy()).to(torch.device("cuda", devs[k])) for k in range(len(devs))] for j in range(5)]
    d_o = [[torch.zeros(18, dtype=torch.int64, device=torch.device("cuda", devs[k])) for k in range(len(devs))] for _ in range(8)]
    d_f = [torch.zeros(18, dtype=torch.int64, device=torch.device("cuda", devs[0])) for _ in range(5)]
    for d in devs:
        torch.cuda.synchronize(d)
    host = []
    for j in range(5):
        grp.msm_sharded_device(gb, [t.data_ptr() for t in d_s[j]], [t.data_ptr() for t in d_o[j]])
        grp.partials_fold_device(1, [t.data_ptr() for t in d_o[j]], d_f[j].data_ptr(), lag=0)
        host.append(grp.partials_fold(1, [t.data_ptr() for t in d_o[j]], lag=0))
    grp.synchronize()
    for j in range(5):
        want = ctx.batch_normalize(1, ctx.msm(single, sets[j])[None, :])
        for got in (d_f[j].cpu().numpy().view(np.uint64), host[j]):
            a = ctx.batch_normalize(1, got[None, :])
            assert np.array_equal(a[0], want[0]) and np.array_equal(a[1], want[1]), j
    # and the synchronous sharded entry points over real devices
    ps, qs = _pair_inputs(9, 8820)
    G1, F1, G2, F2 = _terms_w(ps, qs)
    assert np.array_equal(grp.multi_miller_loop(G1, F1, G2, F2), ctx.multi_miller_loop(G1, F1, G2, F2))
    assert np.array_equal(grp.pairing_batch(G1, F1, G2, F2), ctx.pairing_batch(G1, F1, G2, F2))
    gb.free(); grp.close()


@pytest.mark.parametrize("members", [1, 3])
def test_device_group_asynchronous_pairings_and_fp12_fold(ctx, members):
    """blsgpu_pairings_sharded_device (pairings / raw Miller values stay sharded; member-local multi_miller_loop products) and
    blsgpu_fp12_partials_fold_device (product on member 0, optional ONE final exponentiation) against the single-context entry points"""
    import torch
    import bls12_381_amd as b
    dev = torch.device("cuda", 0)
    grp = b.Group([0] * members)
    n = 23
    ps, qs = _pair_inputs(n, 9100 + members)
    ps[5] = o.G1_IDENTITY_AFF
    G1, F1, G2, F2 = _terms_w(ps, qs)
    sizes = grp.shard_sizes(n)
    lo = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    t = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)
    d1 = [t(G1[lo[k]:lo[k + 1]].copy()) for k in range(members)]; d2 = [t(G2[lo[k]:lo[k + 1]].copy()) for k in range(members)]
    f1 = [t(F1[lo[k]:lo[k + 1]].copy()) for k in range(members)]; f2 = [t(F2[lo[k]:lo[k + 1]].copy()) for k in range(members)]
    ptr = lambda ts: [x.data_ptr() for x in ts]
    for mode, want in ((0, ctx.pairing_batch(G1, F1, G2, F2)), (1, ctx.miller_loop_batch(G1, F1, G2, F2))):
        outs = [torch.zeros((max(1, sizes[k]), 72), dtype=torch.int64, device=dev) for k in range(members)]
        grp.pairings_sharded_device(mode, ptr(d1), ptr(d2), sizes, ptr(outs), d_g1_inf=ptr(f1), d_g2_inf=ptr(f2))
        grp.synchronize()
        got = np.concatenate([outs[k][:sizes[k]].cpu().numpy().view(np.uint64) for k in range(members)])
        assert np.array_equal(got, want), mode
    parts = [torch.zeros(72, dtype=torch.int64, device=dev) for _ in range(members)]
    res = torch.zeros(72, dtype=torch.int64, device=dev)
    ml = ctx.multi_miller_loop(G1, F1, G2, F2)
    for fe, want in ((False, ml), (True, ctx.final_exponentiation_batch(ml[None, :])[0])):
        grp.pairings_sharded_device(2, ptr(d1), ptr(d2), sizes, ptr(parts), d_g1_inf=ptr(f1), d_g2_inf=ptr(f2))
        grp.fp12_partials_fold_device(ptr(parts), res.data_ptr(), final_exp=fe)
        grp.synchronize()
        assert np.array_equal(res.cpu().numpy().view(np.uint64), want), fe
    grp.close()


def test_bench_two_ranks_on_one_gpu_runs_the_exchange_with_real_kernels():
    """The multi-rank path of bench.py with REAL kernels on both ranks (the build box has one GPU): two processes, gloo
    collectives, both on GPU 0, ONE 2^18-point MSM sharded two ways -- partial sums all-gathered, folded on every rank, ranks compared, and
    the folded point checked against the discrete-log identity [sum s_i k_i] G (`result_matches_identity`)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", GLOO_SOCKET_IFNAME="lo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    import socket
    sk = socket.socket(); sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]; sk.close()          # a free port, not a fixed one
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(root, "bench.py"), "--gpus", "2", "--backend", "gloo", "--same-device", "--log-total", "18", "--steps", "4", "--warmup", "2",
           "--full", "--no-cpu-baseline", "--no-extras"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert res.returncode == 0, res.stderr[-3000:]
    line = json.loads([l for l in res.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["scaling"] == "strong" and line["config"]["total_points"] == 1 << 18
    assert line["result_matches_identity"] is True
    assert line["ranks"]["world"] == 2 and line["ranks"]["world_from_process_group"] == 2 and line["ranks"]["backend"] == "gloo" and line["ranks"]["same_device"] is True
    assert line["value"] > 0


def test_bench_plain_run_dumps_the_last_step_reproducibly(tmp_path):
    """A plain `bench.py` run (no --full) prints the contract's keys and nothing it does not time; --dump-outputs writes the last step's MSM
    result, which is [sum s_i k_i] G by the oracle, and two runs with the same arguments write the same arrays."""
    import json
    import subprocess
    import sys
    from bls12_381_amd import synthetic
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = []
    for k in (0, 1):
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--log-n", "14", "--steps", "5", "--warmup", "2", "--dump-outputs", str(tmp_path / str(k))]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
        assert r.returncode == 0, r.stderr[-2000:]
        lines.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    line = lines[0]
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert line.get(key) is not None, key
    assert line["steps"] == 5 and line["warmup"] == 2 and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx((1 << 14) / (line["ms_per_step"] * 1e-3), rel=1e-3)
    assert "roofline" not in line and "cpu_baseline" not in line and "extras" not in line and "single_call_ms" not in line
    got = [np.load(str(tmp_path / str(k) / "g1_msm_result.npy")) for k in (0, 1)]
    assert got[0].dtype == np.float64 and got[0].shape == (96,) and np.array_equal(got[0], got[1])
    n = 1 << 14
    t = synthetic.dot_mod_r(synthetic.scalars(n, synthetic.SEED), synthetic.scalars(n, synthetic.SEED + 1))
    want = o.g1_to_uncompressed(o.g1_to_affine(o.g1_affine_mul(o.G1_GEN, t)))
    assert bytes(got[0].astype(np.uint8)) == want


def test_round6_entry_points_edge_cases_and_argument_errors(ctx, golden_dir):
    """round-6 entry points: empty inputs are values (the identity, nothing written), NULL / out-of-range arguments are status codes with a
    message, the scalar form of a context is restored by the *_mont entry points, and the kernel-timing facility reports what was launched"""
    import ctypes
    import bls12_381_amd as b
    from bls12_381_amd import synthetic as sy
    lib = ctx.lib
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    ERR_ARG = -2
    A = b.api
    # scalar form: bad value, n = 0 MSM over limbs = identity, form unchanged after a *_mont call
    assert lib.blsgpu_set_scalar_form(ctx.h, 2) == ERR_ARG and lib.blsgpu_set_scalar_form(None, 0) == ERR_ARG
    kb = sy.scalars(4, 960)
    bases = ctx.bases_from_scalars(1, kb)
    ident = ctx.msm_mont(bases, np.zeros((0, 4), dtype=np.uint64))
    assert ctx.batch_normalize(1, ident[None, :])[1][0] == 1
    sb = sy.scalars(4, 961)
    limbs, ok = ctx.fr_from_bytes(sb)
    assert ok.all()
    nrm = lambda x: ctx.batch_normalize(1, x[None, :])[0][0]
    assert np.array_equal(nrm(ctx.msm_mont(bases, limbs)), nrm(ctx.msm(bases, sb)))
    assert np.array_equal(nrm(ctx.msm(bases, sb)), nrm(ctx.msm_mont(bases, limbs)))          # bytes again right after limbs: the form was restored
    o18 = np.zeros(18, dtype=np.uint64)
    assert lib.blsgpu_g1_msm_mont(ctx.h, bases.handle, 0, None, 4, P(o18)) == ERR_ARG
    assert lib.blsgpu_g2_msm_mont(ctx.h, bases.handle, 0, P(limbs), 4, P(o18)) == ERR_ARG and b"other group" in lib.blsgpu_last_error()
    # Fr conversions: n = 0, NULLs
    assert ctx.fr_to_bytes(np.zeros((0, 4), dtype=np.uint64)).shape == (0, 32)
    assert lib.blsgpu_fr_to_bytes(ctx.h, None, 3, P(o18), None) == ERR_ARG
    assert lib.blsgpu_fr_from_bytes_wide(ctx.h, None, 0, None) == 0
    # expanders: empty batch, empty message, len 0, unknown expander, too many blocks, NULL
    assert ctx.expand_message(A.EXPAND_XOF_SHAKE128, [], b"d", 32).shape == (0, 32)
    assert ctx.expand_message(A.EXPAND_XMD_SHA512, [b""], b"", 0).shape == (1, 0)
    assert ctx.hash_to_scalar(A.EXPAND_XMD_SHA256, [], b"d", 3).shape == (0, 3, 4)
    assert ctx.hash_to_scalar(A.EXPAND_XMD_SHA256, [b"m"], b"d", 0).shape == (1, 0, 4)
    off = np.array([0, 1], dtype=np.uint64); m = np.zeros(8, dtype=np.uint8); out = np.zeros(64, dtype=np.uint8)
    assert lib.blsgpu_expand_message_batch(ctx.h, -1, P(m), P(off), 1, P(m), 1, 32, P(out)) == ERR_ARG and b"expander" in lib.blsgpu_last_error()
    assert lib.blsgpu_expand_message_batch(ctx.h, A.EXPAND_XMD_SHA512, P(m), P(off), 1, P(m), 1, 255 * 64 + 1, P(out)) == ERR_ARG
    assert lib.blsgpu_expand_message_batch(ctx.h, 0, P(m), None, 1, P(m), 1, 32, P(out)) == ERR_ARG
    assert lib.blsgpu_expand_message_batch(ctx.h, 0, P(m), P(np.array([1, 0], dtype=np.uint64)), 1, P(m), 1, 32, P(out)) == ERR_ARG and b"offsets" in lib.blsgpu_last_error()
    assert lib.blsgpu_hash_to_scalar_batch(ctx.h, 0, P(m), P(off), 1, P(m), 1, 2000, P(out)) == ERR_ARG                 # 2000 * 48 > 65535
    assert lib.blsgpu_hash_to_curve_expander_batch(ctx.h, 3, 1, P(m), P(off), 1, P(m), 1, 0, P(out)) == ERR_ARG        # group 3
    # oversized lengths are argument errors, found before anything is reserved or staged, and the context stays usable
    assert lib.blsgpu_expand_message_batch(ctx.h, 0, P(m), P(off), 1, P(m), 1, 1 << 40, P(out)) == ERR_ARG and b"65535" in lib.blsgpu_last_error()
    assert lib.blsgpu_hash_to_scalar_batch(ctx.h, 0, P(m), P(off), 1, P(m), 1, 1 << 40, P(out)) == ERR_ARG
    t = next(t for t in _h2c_vectors(golden_dir)["expand_msg"] if "sha256" in t["test"])
    assert bytes(ctx.expand_message(A.EXPAND_XMD_SHA256, [bytes.fromhex(t["msg"])], bytes.fromhex(t["dst"]), t["len_in_bytes"])[0]).hex() == t["out"]
    # kernel timing: off by default (empty report), on: one line per kernel of the calls made, cleared by the report
    assert ctx.kernel_timing_report() == {}
    ctx.kernel_timing(True)
    ctx.msm(bases, sb)
    rep = ctx.kernel_timing_report()
    ctx.kernel_timing(False)
    assert any("k_msm_accumulate" in k for k in rep) and all(v["launches"] >= 1 and v["total_ms"] > 0 and v["min_ms"] <= v["max_ms"] for v in rep.values())
    assert ctx.kernel_timing_report() == {}
    ctx.msm(bases, sb)
    assert ctx.kernel_timing_report() == {}
    need = ctypes.c_size_t(0)
    assert lib.blsgpu_kernel_timing_report(ctx.h, None, 16, ctypes.byref(need)) == ERR_ARG
    assert lib.blsgpu_kernel_timing_report(ctx.h, None, 0, ctypes.byref(need)) == 0 and need.value == 0
    # bases cache verify: NULL context
    assert lib.blsgpu_set_bases_cache_verify(None, 1) == ERR_ARG
    bases.free()
