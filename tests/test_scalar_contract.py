"""The scalar contract across the Python API and `Gt * Scalar`.

A context's scalar form (`set_scalar_form`: canonical bytes or `Scalar` Montgomery limbs) says how the library reads raw scalar
memory.  Ints and `Scalar`s handed to a Python wrapper are converted to canonical bytes by the wrapper itself, so every wrapper must
give the oracle's answer in either form.  `blsgpu_gt_mul_scalar_batch*` must report scalars >= r, as bytes or as limbs, as the header
says for every scalar consumer.  Points are compared as affine limbs, Gt elements as canonical Montgomery limbs."""
import ctypes

import numpy as np
import pytest

from oracle import bls12_381_ref as o

pytestmark = pytest.mark.gpu

ERR_ARG = -2
RR = o.R_ORDER
# 0, 1, r - 1, 2^254, two values in [2^254, r) (top nibbles 4 and 7) and random ones
SCALARS = [0, 1, RR - 1, 1 << 254, (1 << 254) + 0x9F8E7D6C5B4A39281706F5E4D3C2B1A0, RR - 0x1234567] + \
    [o.SplitMix64(0x5CA1).scalar() for _ in range(4)]
BAD = [RR, RR + 1, (1 << 255) + 5, (1 << 256) - 1]
FORMS = ["bytes", "mont"]


@pytest.fixture(scope="module")
def ctx():
    import bls12_381_amd as b
    c = b.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gt_gen():
    return o.pairing(o.G1_GEN, o.G2_GEN)


def _form(name):
    import bls12_381_amd as b
    return b.api.SCALAR_MONT if name == "mont" else b.api.SCALAR_BYTES


def _words(v, dtype):
    """the 32 little-endian bytes of the integer v (< 2^256) as a row of `dtype`"""
    return np.frombuffer(int(v).to_bytes(32, "little"), dtype=dtype).copy()


def fp12w(f):
    return np.concatenate([np.array(o.fp_to_mont_limbs(c), dtype=np.uint64) for c in o.fp12_flatten(f)])


def _gen_aff(group, e):
    """[e] G by the oracle, as affine wire limbs (None for the identity)"""
    gen, amul, toaff = (o.G1_GEN, o.g1_affine_mul, o.g1_to_affine) if group == 1 else (o.G2_GEN, o.g2_affine_mul, o.g2_to_affine)
    a = toaff(amul(gen, e % RR))
    if a[2]:
        return None
    fp = lambda x: np.array(o.fp_to_mont_limbs(x), dtype=np.uint64)
    return np.concatenate([fp(a[0]), fp(a[1])] if group == 1 else [fp(a[0][0]), fp(a[0][1]), fp(a[1][0]), fp(a[1][1])]).tobytes()


def _aff(ctx, group, xyz):
    xy, inf = ctx.batch_normalize(group, np.asarray(xyz, dtype=np.uint64).reshape(-1, 18 if group == 1 else 36))
    return [None if f else xy[i].tobytes() for i, f in enumerate(inf)]


def _dot(ks, ss):
    return sum(k * s for k, s in zip(ks, ss)) % RR


class _FormScope:
    """the context (or device group) in `form` for the body; SCALAR_BYTES again afterwards"""

    def __init__(self, target, form):
        self.t, self.form = target, form

    def __enter__(self):
        self.t.set_scalar_form(self.form)

    def __exit__(self, *exc):
        import bls12_381_amd as b
        self.t.set_scalar_form(b.api.SCALAR_BYTES)


def _run_wrapper(ctx, name, group, form):
    """call one wrapper with the int scalars of SCALARS while the context (or the default context / the group) is in `form`;
    returns (got, want) as lists of affine limb bytes"""
    import bls12_381_amd as b
    n = len(SCALARS)
    r = o.SplitMix64(0xC0 + group)
    ks = [r.scalar() for _ in range(n)]
    ss = list(SCALARS)
    whole = _gen_aff(group, _dot(ks, ss))
    if name == "bases_from_scalars":
        with _FormScope(ctx, form):
            bases = ctx.bases_from_scalars(group, ss)
        xy, inf = bases.download()
        bases.free()
        return [None if inf[i] else xy[i].tobytes() for i in range(n)], [_gen_aff(group, s) for s in ss]
    if name == "Group.msm":
        grp = b.Group([0, 0])
        try:
            gb = grp.bases_from_scalars(group, ks)
            with _FormScope(grp, form):
                out = grp.msm(gb, ss)
            gb.free()
        finally:
            grp.close()
        return _aff(ctx, group, out), [whole]
    if name in ("msm_g", "Affine * Scalar"):
        d = b.default_context()
        Aff = b.G1Affine if group == 1 else b.G2Affine
        pts = [(Aff.generator() * b.Scalar(k)).to_affine() for k in ks[:3]]
        resident = d.bases_from_scalars(group, ks)
        with _FormScope(d, form):
            if name == "msm_g":
                fn = b.msm_g1 if group == 1 else b.msm_g2
                res = [fn(pts, ss[:3]).to_affine(), fn(resident, ss).to_affine()]
                want = [_gen_aff(group, _dot(ks[:3], ss[:3])), whole]
            else:
                res = [(Aff.generator() * b.Scalar(s)).to_affine() for s in ss]
                want = [_gen_aff(group, s) for s in ss]
        resident.free()
        return [None if p.infinity else p.xy.tobytes() for p in res], want
    bases = ctx.bases_from_scalars(group, ks)
    xy, inf = bases.download()
    with _FormScope(ctx, form):
        if name == "msm":
            got, want = _aff(ctx, group, ctx.msm(bases, ss)), [whole]
        elif name == "msm_many":
            got = _aff(ctx, group, ctx.msm_many(bases, [ss, ss[::-1]]))
            want = [whole, _gen_aff(group, _dot(ks, ss[::-1]))]
        elif name == "msm_host":
            got, want = _aff(ctx, group, ctx.msm_host(group, xy, inf, ss)), [whole]
        elif name == "msm_bytes":
            enc = ctx.points_to_bytes(group, xy, inf, compressed=False)
            res = ctx.msm_bytes(group, enc.tobytes(), ss)
            pxy, pinf, ok = ctx.points_from_bytes(group, np.frombuffer(res, dtype=np.uint8), compressed=False)
            assert ok[0]
            got, want = [None if pinf[0] else pxy[0].tobytes()], [whole]
        elif name == "msm_segments":
            off = [0, 1, 4, n]
            got = _aff(ctx, group, ctx.msm_segments(bases, ss, off))
            want = [_gen_aff(group, _dot(ks[a:z], ss[a:z])) for a, z in zip(off[:-1], off[1:])]
        elif name == "mul_batch":
            got, want = _aff(ctx, group, ctx.mul_batch(group, xy, inf, ss)), [_gen_aff(group, k * s) for k, s in zip(ks, ss)]
        else:
            raise AssertionError(name)
    bases.free()
    return got, want


WRAPPERS = ["msm", "msm_many", "msm_host", "msm_bytes", "msm_segments", "mul_batch", "bases_from_scalars", "Group.msm", "msm_g",
            "Affine * Scalar"]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("wrapper", WRAPPERS)
@pytest.mark.parametrize("group", [1, 2])
def test_int_scalars_in_either_form(ctx, group, wrapper, form):
    """every wrapper that takes ints converts them to canonical bytes and must be read as such, whatever the context's form"""
    got, want = _run_wrapper(ctx, wrapper, group, _form(form))
    assert got == want


@pytest.mark.parametrize("form", FORMS)
def test_gt_int_scalars_in_either_form(ctx, gt_gen, form):
    """`Context.gt_mul_scalar_batch` and `Gt * Scalar` with ints / Scalars: the oracle's powers in either form"""
    import bls12_381_amd as b
    want = [fp12w(o.gt_mul_scalar(gt_gen, s)) for s in SCALARS]
    G = np.stack([fp12w(gt_gen)] * len(SCALARS))
    with _FormScope(ctx, _form(form)):
        out = ctx.gt_mul_scalar_batch(G, SCALARS)
    assert all(np.array_equal(out[i], want[i]) for i in range(len(SCALARS)))
    d = b.default_context()
    with _FormScope(d, _form(form)):
        got = [b.Gt(fp12w(gt_gen)) * b.Scalar(s) for s in SCALARS[:4]]
    assert all(np.array_equal(got[i].f, want[i]) for i in range(4))


@pytest.mark.parametrize("group", [1, 2])
def test_raw_arrays_follow_the_context_form(ctx, group):
    """a uint8 array is passed through as it is: after a pinned call in SCALAR_MONT, msm_many still reads raw rows as limbs"""
    n = len(SCALARS)
    r = o.SplitMix64(0xD0 + group)
    ks = [r.scalar() for _ in range(n)]
    bases = ctx.bases_from_scalars(group, ks)
    limbs = np.stack([np.array(o.fr_to_mont_limbs(s), dtype=np.uint64) for s in SCALARS])
    with _FormScope(ctx, _form("mont")):
        pinned = ctx.msm(bases, SCALARS)
        raw = ctx.msm_many(bases, limbs.view(np.uint8).reshape(1, n, 32))
    want = [_gen_aff(group, _dot(ks, SCALARS))]
    assert _aff(ctx, group, pinned) == want and _aff(ctx, group, raw) == want
    bases.free()


# ---- `Gt * Scalar` range: blsgpu_gt_mul_scalar_batch(_device) ---------------------------------------------------------------------
def _scalar_rows(vals, form):
    """the memory of vals in one form: canonical LE bytes, or four u64 limbs (Montgomery form of v < r; v itself for v >= r)"""
    if form == "bytes":
        return np.stack([_words(v, np.uint8) for v in vals])
    rows = [np.array(o.fr_to_mont_limbs(v), dtype=np.uint64) if v < RR else _words(v, np.uint64) for v in vals]
    return np.ascontiguousarray(np.stack(rows)).view(np.uint8).reshape(len(vals), 32)


def _gt_call(ctx, G, rows):
    out = np.zeros_like(G)
    rc = ctx.lib.blsgpu_gt_mul_scalar_batch(ctx.h, G.ctypes.data_as(ctypes.c_void_p), rows.ctypes.data_as(ctypes.c_void_p), G.shape[0],
                                            out.ctypes.data_as(ctypes.c_void_p))
    return rc, out


@pytest.mark.parametrize("form", FORMS)
def test_gt_mul_scalar_rejects_scalars_at_or_above_r(ctx, gt_gen, form):
    """r, r + 1, 2^255 + 5 and 2^256 - 1 (bytes, or limbs in SCALAR_MONT): BLSGPU_ERR_ARG from the host form and an error from the next
    synchronize() after the device form; the next valid call of either form is clean and right"""
    import torch
    import bls12_381_amd as b
    good = [5, RR - 1, 1 << 254]
    want = [fp12w(o.gt_mul_scalar(gt_gen, s)) for s in good]
    G = np.stack([fp12w(gt_gen)] * 3)
    dev = torch.device("cuda", 0)
    d_G = torch.from_numpy(G.view(np.int64)).to(dev)
    d_out = torch.zeros((3, 72), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    with _FormScope(ctx, _form(form)):
        for v in BAD:
            rows = _scalar_rows([good[0], v, good[2]], form)
            rc, _ = _gt_call(ctx, G, rows)
            assert rc == ERR_ARG, hex(v)
            assert b"canonical" in ctx.lib.blsgpu_last_error(), hex(v)
            rc, out = _gt_call(ctx, G, _scalar_rows(good, form))
            assert rc == 0 and all(np.array_equal(out[i], want[i]) for i in range(3)), hex(v)
            d_rows = torch.from_numpy(rows).to(dev)
            torch.cuda.synchronize()
            ctx.gt_mul_scalar_batch_device(d_G.data_ptr(), d_rows.data_ptr(), 3, d_out.data_ptr())
            with pytest.raises(b.BlsGpuError, match="canonical"):
                ctx.synchronize()
        d_rows = torch.from_numpy(_scalar_rows(good, form)).to(dev)
        torch.cuda.synchronize()
        ctx.gt_mul_scalar_batch_device(d_G.data_ptr(), d_rows.data_ptr(), 3, d_out.data_ptr())
        ctx.synchronize()
    got = d_out.cpu().numpy().view(np.uint64)
    assert all(np.array_equal(got[i], want[i]) for i in range(3))


@pytest.mark.parametrize("form", FORMS)
def test_gt_mul_scalar_canonical_edges(ctx, gt_gen, form):
    """canonical scalars at the edges of the 255-bit double-and-add, [2^254, r) included, through the raw entry point in both forms"""
    vals = [0, 1, 2, RR - 1, RR - 2, (RR - 1) // 2, (1 << 254) - 1, 1 << 254, (1 << 254) + 1, RR - 0x1234567, (1 << 253) + (1 << 254),
            (7 << 252) + 0x12345, (1 << 128) - 1, 1 << 128, (1 << 64) - 1]
    G = np.stack([fp12w(gt_gen)] * len(vals))
    with _FormScope(ctx, _form(form)):
        rc, out = _gt_call(ctx, G, _scalar_rows(vals, form))
    assert rc == 0
    bad = [hex(v) for i, v in enumerate(vals) if not np.array_equal(out[i], fp12w(o.gt_mul_scalar(gt_gen, v)))]
    assert not bad
