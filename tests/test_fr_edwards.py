"""Twisted Edwards groups over Fr (`blsgpu_fr_edwards_*`; csrc/fr_edwards.hip.h + csrc/fr_edwards_plan.h) on the GPU, on Jubjub (complete)
and Bandersnatch (not complete: every input point has odd order).

Expectations are Python integers by the affine addition law (tests/fr_edwards_ref.py through the shared cases of
tests/fr_edwards_cases.py, computed once per process).  Projective results are normalised ON THE DEVICE and the affine limbs are compared
limb for limb with the reference's: there is no tolerance anywhere."""
import random

import numpy as np
import pytest

import fr_edwards_cases as cases
import fr_edwards_ref as ref

pytestmark = pytest.mark.gpu

CURVES = ["jubjub", "bandersnatch"]
CHUNK = 256                                                        # csrc/fr_edwards_plan.h: FRED_MSM_BLOCK * FRED_MSM_TERMS
R_LIMBS = np.frombuffer(ref.RR.to_bytes(32, "little"), dtype=np.uint64)


@pytest.fixture(scope="module")
def ctx():
    import bls12_381_amd as b
    c = b.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def curves(ctx):
    hs = {name: ctx.fr_edwards(ref.CURVES[name].a, ref.CURVES[name].d) for name in CURVES}
    yield hs
    for h in hs.values():
        h.close()


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.uint8): np.uint8}[a.dtype]
    return torch.from_numpy(a.view(view)).to(torch.device("cuda", 0))


def host(d, dtype=np.uint64):
    return d.cpu().numpy().view(dtype)


def same_points(e, out_xyz, want, what):
    """the projective results, normalised on the device, are the reference's points limb for limb"""
    xy, ok = e.normalize(out_xyz)
    assert ok.all(), what
    assert ref.raw(xy) == ref.raw(ref.points_limbs(want)), what
    return xy


def test_create(ctx, curves):
    """`complete` for both curves, and every refusal with the argument named"""
    from bls12_381_amd._lib import BlsGpuError
    assert curves["jubjub"].complete and not curves["bandersnatch"].complete
    cv = ref.JUBJUB
    for a, d, needle in ((0, cv.d, "a must not be 0"), (cv.a, 0, "d must not be 0"), (cv.d, cv.d, "a and d must differ"),
                         (R_LIMBS.copy(), cv.d, "a is not a canonical"), (cv.a, R_LIMBS.copy(), "d is not a canonical")):
        with pytest.raises(BlsGpuError) as err:
            ctx.fr_edwards(a, d)
        assert needle in str(err.value)
    sq = ctx.fr_edwards(4, 9)                                       # a square, d square: a curve, not a complete one
    assert not sq.complete
    sq.close()


@pytest.mark.parametrize("name", CURVES)
def test_check_and_normalize(ctx, curves, name):
    """n in {1, 63, 257}; points on and off the curve and limbs >= r; Z random, 1 and 0; host and device forms; out == in is refused"""
    import torch
    from bls12_381_amd._lib import BlsGpuError
    e = curves[name]
    pts = cases.mul_cases(name)["points"]
    xy = ref.points_limbs(pts)
    bad = {5: 0, 40: 1, 200: None}
    for i, coord in bad.items():
        if coord is None:
            xy[i, 0] = R_LIMBS
        else:
            xy[i, coord] = ref.limbs([(pts[i][coord] + 1) % ref.RR])[0]
    rng = random.Random(9)
    zs = [1 if i % 7 == 0 else rng.randrange(1, ref.RR) for i in range(len(pts))]
    zero = {0, 33, 62, 256}
    xyz = ref.limbs([c for i, (p, z) in enumerate(zip(pts, zs)) for c in (p[0] * z % ref.RR, p[1] * z % ref.RR, 0 if i in zero else z)]).reshape(-1, 3, 4)
    for n in (1, 63, 257):
        want_ok = [0 if i in bad else 1 for i in range(n)]
        want_z = [0 if i in zero else 1 for i in range(n)]
        want_xy = ref.raw(ref.points_limbs([(0, 1) if i in zero else pts[i] for i in range(n)]))
        assert list(e.check(xy[:n])) == want_ok, n
        got, ok = e.normalize(xyz[:n])
        assert list(ok) == want_z and ref.raw(got) == want_xy, n
        d_xy, d_xyz = dev(xy[:n]), dev(xyz[:n])
        d_ok, d_ok2, d_out = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros((n, 2, 4), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        e.check_device(d_xy.data_ptr(), n, d_ok.data_ptr())
        e.normalize_device(d_xyz.data_ptr(), n, d_out.data_ptr(), d_ok2.data_ptr())
        ctx.synchronize()
        assert list(host(d_ok, np.uint8)) == want_ok and list(host(d_ok2, np.uint8)) == want_z and ref.raw(host(d_out)) == want_xy, n
        with pytest.raises(BlsGpuError) as err:
            e.normalize_device(d_xyz.data_ptr(), n, d_xyz.data_ptr())
        assert "no in-place form" in str(err.value)
    assert list(e.check(np.zeros((0, 2, 4), dtype=np.uint64))) == []


@pytest.mark.parametrize("name", CURVES)
@pytest.mark.parametrize("bits", cases.MUL_BITS)
def test_mul_batch(ctx, curves, name, bits):
    """n in {1, 63, 257}: the special points (the identity, (0, -1), both points of order 4 and a prime-order point plus a small-order one
    on Jubjub) against 0, 1, 2^bits - 1, s, h s, the carry patterns and 2^256 - 1, then random pairs; host and device forms"""
    import torch
    e = curves[name]
    c = cases.mul_cases(name)
    for n in (1, 63, 257):
        pts, ks, want = ref.points_limbs(c["points"][:n]), ref.scalar_bytes(c["scalars"][bits][:n]), c["want"][bits][:n]
        same_points(e, e.mul_batch(pts, ks, bits), want, (name, bits, n, "host"))
        d_p, d_k, d_out = dev(pts), dev(ks), torch.zeros((n, 3, 4), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        e.mul_batch_device(d_p.data_ptr(), d_k.data_ptr(), bits, n, d_out.data_ptr())
        ctx.synchronize()
        same_points(e, host(d_out), want, (name, bits, n, "device"))
    assert e.mul_batch(c["points"][:2], c["scalars"][bits][:2], bits).shape == (2, 3, 4)      # Python ints in


@pytest.mark.parametrize("name", CURVES)
def test_mul_batch_flags_a_scalar_above_bits(ctx, curves, name):
    """a scalar with a bit at `bits`: BLSGPU_ERR_ARG from the host form, the sticky word and the next synchronise for the device form, and
    every other output stays right"""
    import torch
    from bls12_381_amd._lib import BlsGpuError
    e = curves[name]
    c = cases.mul_cases(name)
    n = 63
    for bits in (3, 64, 253):
        ks = list(c["scalars"][bits][:n])
        ks[17] |= 1 << bits
        pts, kb = ref.points_limbs(c["points"][:n]), ref.scalar_bytes(ks)
        with pytest.raises(BlsGpuError) as err:
            e.mul_batch(pts, kb, bits)
        assert "at or above `bits`" in str(err.value)
        d_p, d_k, d_out = dev(pts), dev(kb), torch.zeros((n, 3, 4), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        e.mul_batch_device(d_p.data_ptr(), d_k.data_ptr(), bits, n, d_out.data_ptr())
        with pytest.raises(BlsGpuError):
            ctx.synchronize()
        ctx.synchronize()                                           # the flag was reported once and cleared
        out = host(d_out).reshape(n, 3, 4)
        keep = [i for i in range(n) if i != 17]
        same_points(e, out[keep], [c["want"][bits][i] for i in keep], (name, bits))
    same_points(e, e.mul_batch(pts[:5], ref.scalar_bytes(c["scalars"][253][:5]), 253), c["want"][253][:5], "a clean call after a flagged one")


def run_msm(ctx, e, name, table, c, what):
    """host form and device form of one case; both agree with the reference limb for limb, and a second device run with the first"""
    import torch
    k = len(c["offsets"]) - 1
    want = c["want"]
    xy_host = same_points(e, table.msm_segments(c["offsets"], ref.scalar_bytes(c["scalars"]), c["base_first"]), want, (what, "host"))
    d_off = dev(np.asarray(c["offsets"], dtype=np.uint32))
    d_bf = None if c["base_first"] is None else dev(np.asarray(c["base_first"], dtype=np.uint32))
    d_k = dev(ref.scalar_bytes(c["scalars"])) if c["scalars"] else torch.zeros(32, dtype=torch.uint8, device="cuda")
    outs = [torch.zeros((k, 3, 4), dtype=torch.int64, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    for o in outs:
        table.msm_segments_device(d_off.data_ptr(), d_k.data_ptr(), k, c["offsets"][-1], o.data_ptr(), None if d_bf is None else d_bf.data_ptr())
    ctx.synchronize()
    xy_dev = [same_points(e, host(o), want, (what, "device")) for o in outs]
    assert np.array_equal(xy_dev[0], xy_dev[1]) and np.array_equal(xy_dev[0], xy_host), (what, "two runs differ after normalize")


@pytest.mark.parametrize("name", CURVES)
@pytest.mark.parametrize("bits", [3, 253])
def test_tables_and_shared_slices(ctx, curves, name, bits):
    """bases n in {1, 8, 64} x window in {2, 4, 8}: 300 segments of 0 .. n terms over ONE shared slice (base_first all 0); from 8 bases on the
    set holds a repeated base and, on Jubjub, the identity and a point with a component of order 4"""
    e = curves[name]
    for n in (1, 8, 64):
        c = cases.msm_case(name, "shared", n, bits, CHUNK)
        xy = ref.points_limbs(cases.base_set(name, n)["points"])
        for window in (2, 4, 8):
            t = e.bases(xy, bits, window)
            assert len(t) == n
            run_msm(ctx, e, name, t, c, (name, "shared", n, bits, window))
            t.close()


@pytest.mark.parametrize("name", CURVES)
def test_segments_around_the_chunk(ctx, curves, name):
    """empty, length 1, exactly a chunk of the shipped shape, one less, one more, three chunks and five, 300 short segments around a long
    one, over random OVERLAPPING slices of 1024 bases; then base_first == NULL, and terms that cancel within a segment"""
    import torch
    e = curves[name]
    big = ref.points_limbs(cases.base_set(name, 1024)["points"])
    d_big = dev(big)
    torch.cuda.synchronize()
    for bits, window in ((253, 4), (3, 2)):
        t = e.bases_from_device(d_big.data_ptr(), 1024, bits, window)
        assert len(t) == 1024
        run_msm(ctx, e, name, t, cases.msm_case(name, "long", 1024, bits, CHUNK), (name, "long", bits, window))
        t.close()
    t = e.bases(ref.points_limbs(cases.base_set(name, 64)["points"]), 253, 4)
    run_msm(ctx, e, name, t, cases.msm_case(name, "natural", 64, 253, CHUNK), (name, "natural"))
    empty = t.msm_segments([0, 0, 0], [])
    assert ref.points_of(e.normalize(empty)[0]) == [(0, 1), (0, 1)] and ref.ints(empty) == [0, 1, 1] * 2      # (0 : 1 : 1) itself
    assert t.msm_segments([0], []).shape == (0, 3, 4)
    t.close()
    t = e.bases(ref.points_limbs(cases.base_set(name, 8)["points"]), 256, 8)
    c = cases.msm_case(name, "cancel", 8, 256, CHUNK)
    assert c["want"][:3] == [(0, 1)] * 3
    run_msm(ctx, e, name, t, c, (name, "cancel"))
    t.close()


@pytest.mark.parametrize("name", CURVES)
def test_msm_agrees_with_mul_batch_and_reference_sums(ctx, curves, name):
    """the fixed-base route against the variable-base one: every term through mul_batch, normalised, summed by the reference's addition"""
    e = curves[name]
    cv = ref.CURVES[name]
    bs = cases.base_set(name, 64)
    c = cases.msm_case(name, "long", 64, 253, 8)                    # the same segment shapes around a chunk of 8: 200 terms or so
    off, bf, ks = c["offsets"], c["base_first"], c["scalars"]
    term_base = [bf[j] + i for j in range(len(bf)) for i in range(off[j + 1] - off[j])]
    prods, ok = e.normalize(e.mul_batch([bs["points"][b] for b in term_base], ks, 253))
    assert ok.all()
    prods = ref.points_of(prods)
    sums = [cv.sum(prods[off[j]:off[j + 1]]) for j in range(len(bf))]
    assert sums == c["want"]
    t = e.bases(ref.points_limbs(bs["points"]), 253, 4)
    same_points(e, t.msm_segments(off, ks, bf), sums, name)
    t.close()


@pytest.mark.parametrize("name", CURVES)
def test_refusals(ctx, curves, name):
    """every refusal of the tables and the MSM: BLSGPU_ERR_ARG with nothing launched, and the sticky flag for a segment the device form
    cannot refuse"""
    import torch
    from bls12_381_amd._lib import BlsGpuError
    e = curves[name]
    pts = cases.base_set(name, 8)["points"]
    xy = ref.points_limbs(pts)

    def refused(fn, needle):
        with pytest.raises(BlsGpuError) as err:
            fn()
        assert needle in str(err.value), (needle, str(err.value))

    refused(lambda: e.bases(xy, 0, 4), "bits must be in [1, 256]")
    refused(lambda: e.bases(xy, 257, 4), "bits must be in [1, 256]")
    refused(lambda: e.bases(xy, 253, 1), "window must be in [2, 8]")
    refused(lambda: e.bases(xy, 253, 9), "window must be in [2, 8]")
    refused(lambda: e.bases(np.zeros((0, 2, 4), dtype=np.uint64), 253, 4), "fr_edwards_bases: ")
    off_curve = xy.copy()
    off_curve[5, 1] = ref.limbs([(pts[5][1] + 1) % ref.RR])[0]
    refused(lambda: e.bases(off_curve, 253, 4), "base 5 is not a point of the curve")
    d_bad = dev(off_curve)
    torch.cuda.synchronize()
    refused(lambda: e.bases_from_device(d_bad.data_ptr(), 8, 253, 4), "a base is not a point of the curve")
    refused(lambda: e.bases_from_device(d_bad.data_ptr() + 8, 7, 253, 4), "16-byte aligned")
    refused(lambda: e.bases_from_device(d_bad.data_ptr(), 1 << 20, 253, 8), "exceed 2 GiB")
    refused(lambda: e.mul_batch(xy, ref.scalar_bytes([1] * 8), 0), "bits must be in [1, 256]")
    refused(lambda: e.mul_batch(xy, ref.scalar_bytes([1] * 8), 257), "bits must be in [1, 256]")
    t = e.bases(xy, 253, 4)
    ks = ref.scalar_bytes([3] * 8)
    refused(lambda: t.msm_segments([1, 4, 8], ks, None), "offsets[0] must be 0")
    refused(lambda: t.msm_segments([0, 5, 4, 8], ks, None), "non-decreasing")
    refused(lambda: t.msm_segments([0, 4, 8], ks, [0, 5]), "outside the table")
    refused(lambda: t.msm_segments([0, 4, 8], ks, [0xFFFFFFFF, 0]), "outside the table")
    bad_k = ref.scalar_bytes([3, 1 << 253] + [3] * 6)
    refused(lambda: t.msm_segments([0, 4, 8], bad_k, None), "at or above `bits`")
    # device form: what it can refuse ...
    d_off, d_k, d_out = dev(np.array([0, 4, 8], dtype=np.uint32)), dev(ks), torch.zeros((2, 3, 4), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    refused(lambda: t.msm_segments_device(d_off.data_ptr() + 2, d_k.data_ptr(), 2, 8, d_out.data_ptr()), "4-byte aligned")
    refused(lambda: t.msm_segments_device(d_off.data_ptr(), d_k.data_ptr() + 8, 2, 8, d_out.data_ptr()), "16-byte aligned")
    refused(lambda: t.msm_segments_device(d_off.data_ptr(), d_k.data_ptr(), 2, (1 << 26) + 1, d_out.data_ptr()), "total must not exceed 2^26")
    refused(lambda: t.msm_segments_device(d_off.data_ptr(), d_k.data_ptr(), 0, 8, d_out.data_ptr()), "terms but no segment")
    refused(lambda: t.msm_segments_device(None, d_k.data_ptr(), 2, 8, d_out.data_ptr()), "NULL offsets")
    refused(lambda: t.msm_segments_device(d_off.data_ptr(), d_k.data_ptr(), 2, 8, d_k.data_ptr()), "overlaps an input")
    # ... and what only the next synchronise can report: decreasing offsets, offsets[k] != total, bases outside the table
    for off, bf, total in (([0, 6, 4, 8], None, 8), ([0, 4, 8], None, 7), ([0, 4, 8], [0, 6], 8)):
        d_o = dev(np.array(off, dtype=np.uint32))
        d_b = None if bf is None else dev(np.array(bf, dtype=np.uint32))
        d_res = torch.zeros((len(off) - 1, 3, 4), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        t.msm_segments_device(d_o.data_ptr(), d_k.data_ptr(), len(off) - 1, total, d_res.data_ptr(), None if d_b is None else d_b.data_ptr())
        with pytest.raises(BlsGpuError) as err:
            ctx.synchronize()
        assert "fr_edwards_msm_segments_device" in str(err.value), (off, bf, total)
        ctx.synchronize()
    same_points(e, t.msm_segments([0, 4, 8], ks, None), [ref.CURVES[name].sum([ref.CURVES[name].mul(3, p) for p in pts[i:i + 4]]) for i in (0, 4)], "a clean call after the flagged ones")
    t.close()
