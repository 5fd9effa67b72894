"""Poseidon over Fr (`blsgpu_fr_poseidon_*`; csrc/fr_poseidon.hip.h + csrc/fr_poseidon_plan.h) on the GPU.

Expectations are Python integers by the textbook definition (tests/fr_poseidon_ref.py), compared limb for limb: there is no tolerance
anywhere.  The one large shape compares the sparse handle with the dense one (two routes to the same unique values) and samples Python."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import fr_poseidon_ref as ref
from bls12_381_amd import synthetic

pytestmark = pytest.mark.gpu

RR = ref.RR
ERR_ARG = -2
WIDTHS = [2, 3, 4, 5, 9, 12]
_params = {}


def params(t, rf, rp):
    if (t, rf, rp) not in _params:
        c, m = synthetic.poseidon_test_params(t, rf, rp, 1)
        _params[(t, rf, rp)] = (t, rf, rp, c, m)
    return _params[(t, rf, rp)]


@pytest.fixture(scope="module")
def ctx():
    import bls12_381_amd as b
    c = b.Context(0)
    yield c
    c.close()


def rand(n, seed):
    return synthetic.to_ints(synthetic.scalars(n, seed))


def handle(ctx, p, form=0):
    return ctx.fr_poseidon(p[0], p[1], p[2], p[3], p[4], form=form)


def ints(limbs):
    return ref.raw_ints(np.ascontiguousarray(limbs).view(np.uint32).reshape(-1, 8))


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(torch.device("cuda", 0))


def host(d):
    return d.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("t", WIDTHS)
@pytest.mark.parametrize("rounds", [(2, 1), (8, 57)], ids=["2-1", "8-57"])
def test_permute_and_hash(ctx, t, rounds):
    """every width, both forms, n in {1, 65, 257, 1000}: a partial wavefront, a partial block, several blocks; host and device forms, in
    place and out of place; states of all 0 and all r - 1 among them; hash_many under two tags"""
    import torch
    import bls12_381_amd as b
    p = params(t, *rounds)
    big = 1000
    st = rand(big * t, 11 * t + rounds[1])
    states = [st[i * t:(i + 1) * t] for i in range(big)]
    states[0], states[1 % big] = [0] * t, [RR - 1] * t
    want = ref.mont([x for s in states for x in ref.permute(s, *p)])
    want_h = {tag: ref.mont([ref.hash_one(tag, s[1:], *p) for s in states[:257]]) for tag in (0, 5)}
    for form, expect in ((b.FR_POSEIDON_AUTO, b.FR_POSEIDON_SPARSE), (b.FR_POSEIDON_DENSE, b.FR_POSEIDON_DENSE)):
        h = handle(ctx, p, form)
        assert (h.width, h.rounds_full, h.rounds_partial, h.form) == (t, rounds[0], rounds[1], expect)
        T = t
        assert h.products_per_permutation == (rounds[0] * (3 * T + T * T) + rounds[1] * (2 * T + 2) + (T - 1) ** 2 if expect == b.FR_POSEIDON_SPARSE
                                              else rounds[0] * (3 * T + T * T) + rounds[1] * (3 + T * T))
        for n in (1, 65, 257, big):
            x = ref.limbs([v for s in states[:n] for v in s]).reshape(n, t, 4)
            assert ints(h.permute(x)) == want[:n * t], (t, rounds, form, n)
            d_x, d_out = dev(x), torch.zeros((n, t, 4), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            h.permute_device(d_x.data_ptr(), n, d_out.data_ptr())
            h.permute_device(d_x.data_ptr(), n, d_x.data_ptr())      # in place, after the out-of-place call on the same stream
            ctx.synchronize()
            assert ints(host(d_out)) == want[:n * t] and torch.equal(d_x, d_out), (t, rounds, form, n, "device")
        assert ints(h.permute(states[:3])) == want[:3 * t]           # Python ints in
        n = 257
        pre = ref.limbs([v for s in states[:n] for v in s[1:]]).reshape(n, t - 1, 4)
        d_pre, d_dig = dev(pre), torch.zeros((n, 4), dtype=torch.int64, device="cuda")
        for tag in (0, 5):
            assert ints(h.hash_many(pre, tag=tag)) == want_h[tag], (t, rounds, form, tag)
            torch.cuda.synchronize()
            h.hash_many_device(d_pre.data_ptr(), n, d_dig.data_ptr(), tag=tag)
            ctx.synchronize()
            assert ints(host(d_dig)) == want_h[tag] and np.array_equal(host(d_pre).reshape(pre.shape), pre)
        h.close()


def test_edge_instances(ctx):
    """zero round constants, M = identity, both at once and constants of r - 1, at t = 3 and t = 5 in both forms, on states of all 0, all
    r - 1, a mix and a random one; host and device forms"""
    import torch
    import bls12_381_amd as b
    rf, rp = 8, 5
    for t in (3, 5):
        _, _, _, c, m = params(t, rf, rp)
        ident = [[1 if i == j else 0 for j in range(t)] for i in range(t)]
        zero_c, top_c = [[0] * t for _ in range(rf + rp)], [[RR - 1] * t for _ in range(rf + rp)]
        states = [[0] * t, [RR - 1] * t, ([0, RR - 1] * t)[:t], rand(t, t)]
        x = ref.limbs([v for s in states for v in s]).reshape(len(states), t, 4)
        for cc, mm in ((zero_c, m), (c, ident), (zero_c, ident), (top_c, m)):
            p = (t, rf, rp, cc, mm)
            want = ref.mont([v for s in states for v in ref.permute(s, *p)])
            for form, expect in ((b.FR_POSEIDON_AUTO, b.FR_POSEIDON_SPARSE), (b.FR_POSEIDON_DENSE, b.FR_POSEIDON_DENSE)):
                h = handle(ctx, p, form)
                assert h.form == expect                              # the identity's lower-right block is regular
                assert ints(h.permute(x)) == want, (t, form)
                d_x = dev(x)
                torch.cuda.synchronize()
                h.permute_device(d_x.data_ptr(), len(states), d_x.data_ptr())
                ctx.synchronize()
                assert ints(host(d_x)) == want, (t, form, "device")
                h.close()


MERKLE = [(3, 10, 3), (3, 0, 2), (3, 1, 2), (5, 4, 1), (9, 3, 1), (12, 2, 2), (2, 3, 5)]


@pytest.mark.parametrize("t,height,k", MERKLE, ids=["a%d-h%d-k%d" % (t - 1, h, k) for t, h, k in MERKLE])
def test_merkle(ctx, t, height, k):
    """arity 2 with height 10 and k = 3 (levels of several workgroups down to levels of three nodes); heights 0 and 1; arities 4, 8, 11 (and 1); `nodes`
    given and NULL, host and device forms; every node against the Python recursion; a second run is limb-identical"""
    import torch
    p = params(t, 2, 1) if height > 3 else params(t, 8, 57 if t <= 5 else 5)
    a = t - 1
    leaves = rand(k * a ** height, 7 * t + height)
    levels, roots = ref.merkle(9, leaves, height, k, *p)
    want_nodes, want_roots = ref.mont([x for lv in levels for x in lv]), ref.mont(roots)
    h = handle(ctx, p)
    x = ref.limbs(leaves)
    r1, n1 = h.merkle(x, height, k, tag=9)
    r2, n2 = h.merkle(leaves, height, k, tag=9, with_nodes=False)
    assert ints(r1) == want_roots and ints(r2) == want_roots and n2 is None
    assert ints(n1) == want_nodes
    d_x, d_roots, d_nodes = dev(x), torch.zeros((k, 4), dtype=torch.int64, device="cuda"), torch.zeros((max(len(want_nodes), 1), 4), dtype=torch.int64, device="cuda")
    d_roots2 = torch.zeros_like(d_roots)
    torch.cuda.synchronize()
    h.merkle_device(d_x.data_ptr(), height, k, d_roots.data_ptr(), d_nodes.data_ptr(), tag=9)
    h.merkle_device(d_x.data_ptr(), height, k, d_roots2.data_ptr(), None, tag=9)
    ctx.synchronize()
    assert ints(host(d_roots)) == want_roots and torch.equal(d_roots, d_roots2)
    assert ints(host(d_nodes))[:len(want_nodes)] == want_nodes
    assert np.array_equal(host(d_x).reshape(x.shape), x), "the leaves were written"
    keep = d_nodes.clone()
    h.merkle_device(d_x.data_ptr(), height, k, d_roots2.data_ptr(), d_nodes.data_ptr(), tag=9)
    ctx.synchronize()
    assert torch.equal(keep, d_nodes) and torch.equal(d_roots, d_roots2), "a second run differs"
    h.close()


def test_hash_many_large(ctx):
    """hash_many_device at n = 2^20, t = 3, (8, 57): the sparse handle against the DENSE handle limb for limb, 256 sampled digests against
    Python"""
    import torch
    import bls12_381_amd as b
    p = params(3, 8, 57)
    n = 1 << 20
    raw = np.random.RandomState(5).randint(0, 256, size=(2 * n, 32), dtype=np.uint8)
    raw[:, 31] &= 0x3F                                               # < 2^254 < r: canonical limbs of some scalar
    x = raw.view(np.uint64).reshape(n, 2, 4)
    hs, hd = handle(ctx, p), handle(ctx, p, b.FR_POSEIDON_DENSE)
    assert (hs.form, hd.form) == (b.FR_POSEIDON_SPARSE, b.FR_POSEIDON_DENSE)
    d_x, d_a, d_b = dev(x), torch.zeros((n, 4), dtype=torch.int64, device="cuda"), torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    hs.hash_many_device(d_x.data_ptr(), n, d_a.data_ptr(), tag=3)
    hd.hash_many_device(d_x.data_ptr(), n, d_b.data_ptr(), tag=3)
    ctx.synchronize()
    assert torch.equal(d_a, d_b)
    idx = [0, 1, 63, 64, 255, 256, n - 1] + [int(v) for v in np.random.RandomState(6).randint(0, n, size=249)]
    got = ints(host(d_a[torch.tensor(idx, device="cuda")]))
    vals = [[v * ref.R_INV % RR for v in ref.raw_ints(x[i].view(np.uint32).reshape(2, 8))] for i in idx]
    assert got == ref.mont([ref.hash_one(3, v, *p) for v in vals])
    hs.close()
    hd.close()


def test_device_transcript(ctx):
    """a Spartan-shaped sumcheck (k = 4 tables, m = 6, eq (Az Bz - Cz), D = 3) whose challenges never leave the device:
    fr_sumcheck_round_device writes its 4 evaluations, fr_poseidon hash_many_device (t = 5, n = 1, tag = the round number) writes the
    scalar the next round reads as d_r_prev -- no synchronisation until the end.  Round evaluations and final table values equal those of
    the host-driven FrSumcheck fed the same challenges computed in Python."""
    import torch
    import bls12_381_amd as b
    k, m, n = 4, 6, 64
    terms = [(1, [0, 1, 2]), (RR - 1, [0, 3])]
    p = params(5, 8, 57)
    h = handle(ctx, p)
    tables = ref.limbs(rand(k * n, 77)).reshape(k, n, 4)
    d_t = dev(tables)
    d_ev = torch.zeros((m, 4, 4), dtype=torch.int64, device="cuda")
    d_r = torch.zeros((m, 4), dtype=torch.int64, device="cuda")
    d_fin = torch.zeros((k, 4), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    mm = m
    for s in range(m):
        ctx.fr_sumcheck_round_device(d_t.data_ptr(), n, mm, k, terms, d_ev[s].data_ptr(), None if s == 0 else d_r[s - 1].data_ptr())
        if s > 0:
            mm -= 1
        h.hash_many_device(d_ev[s].data_ptr(), 1, d_r[s].data_ptr(), tag=s + 1)
    ctx.fr_mle_fold_device(d_t.data_ptr(), n, 1, k, d_r[m - 1].data_ptr(), d_fin.data_ptr(), 1)
    ctx.synchronize()
    sc = ctx.fr_sumcheck(tables, terms)
    r_prev = None
    for s in range(m):
        ev = sc.round(r_prev)
        assert np.array_equal(ev, host(d_ev[s])), "round %d" % (s + 1)
        r_prev = ref.hash_one(s + 1, [b.fr_limbs_to_int(e) for e in ev], *p)
        assert ints(host(d_r[s])) == ref.mont([r_prev]), "challenge %d" % (s + 1)
    assert np.array_equal(sc.finish(r_prev), host(d_fin))
    sc.close()
    h.close()


def test_ntt_then_merkle_on_the_device(ctx):
    """fr_ntt_many_device -> fr_poseidon merkle_device without a host copy: the roots equal Python's over the oracle's transform"""
    import torch
    from oracle import bls12_381_ref as o
    p = params(3, 8, 57)
    h = handle(ctx, p)
    k, log_n = 2, 6
    cols = [rand(1 << log_n, 40 + v) for v in range(k)]
    d_x, d_roots = dev(ref.limbs([x for c in cols for x in c])), torch.zeros((k, 4), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.fr_ntt_many_device(d_x.data_ptr(), log_n, k)
    h.merkle_device(d_x.data_ptr(), log_n, k, d_roots.data_ptr(), None, tag=1)
    ctx.synchronize()
    evals = [y for c in cols for y in o.fr_ntt(c)]
    assert ints(host(d_roots)) == ref.mont(ref.merkle(1, evals, log_n, k, *p)[1])
    h.close()


def test_refusals(ctx):
    """every BLSGPU_ERR_ARG of the header text, each with a text naming the cause and nothing launched: a following valid call works and
    no output was touched"""
    import torch
    import bls12_381_amd as b
    lib, hctx = ctx.lib, ctx.h
    err = lambda: lib.blsgpu_last_error().decode()
    vp = ctypes.c_void_p
    t, rf, rp, c, m = params(3, 4, 3)
    rc, mm = ref.limbs([x for row in c for x in row]), ref.limbs([x for row in m for x in row])
    out = vp()

    def create(tt, f, pp, a_rc, a_mm, form):
        out.value = 0xdead
        rcode = lib.blsgpu_fr_poseidon_create(hctx, tt, f, pp, vp(a_rc) if a_rc else None, vp(a_mm) if a_mm else None, form, ctypes.byref(out))
        return rcode, out.value
    big_rc, big_mm = np.zeros((145 * 13, 4), dtype=np.uint64), np.zeros((169, 4), dtype=np.uint64)
    for tt in (0, 1, 6, 7, 13):
        assert create(tt, rf, rp, big_rc.ctypes.data, big_mm.ctypes.data, 0) == (ERR_ARG, None) and "t must be one of" in err()
    for f in (0, 3, 18):
        assert create(t, f, rp, big_rc.ctypes.data, mm.ctypes.data, 0) == (ERR_ARG, None) and "r_full" in err()
    assert create(t, rf, 129, big_rc.ctypes.data, mm.ctypes.data, 0) == (ERR_ARG, None) and "r_partial" in err()
    assert create(t, rf, rp, rc.ctypes.data, mm.ctypes.data, 2) == (ERR_ARG, None) and "form" in err()
    assert create(t, rf, rp, None, mm.ctypes.data, 0) == (ERR_ARG, None) and "NULL" in err()
    assert create(t, rf, rp, rc.ctypes.data, None, 0) == (ERR_ARG, None) and "NULL" in err()
    bad = rc.copy()
    bad[10] = np.array([0xffffffff00000001, 0x53bda402fffe5bfe, 0x3339d80809a1d805, 0x73eda753299d7d48], dtype=np.uint64)
    assert create(t, rf, rp, bad.ctypes.data, mm.ctypes.data, 0) == (ERR_ARG, None) and "round_constants[10]" in err()
    bad = mm.copy()
    bad[4, 3] = 0xffffffffffffffff
    assert create(t, rf, rp, rc.ctypes.data, bad.ctypes.data, 0) == (ERR_ARG, None) and "mds[4]" in err()
    assert lib.blsgpu_fr_poseidon_create(hctx, t, rf, rp, vp(rc.ctypes.data), vp(mm.ctypes.data), 0, None) == ERR_ARG

    p = params(3, 4, 3)
    h = handle(ctx, p)
    hh = h.handle
    n = 8
    x = ref.limbs(rand(n * 3, 1)).reshape(n, 3, 4)
    d_x = dev(x)
    d_out = torch.zeros((2 * n * 3, 4), dtype=torch.int64, device="cuda")
    tag = ref.limbs([1])
    bad_tag = np.array([0xffffffffffffffff] * 4, dtype=np.uint64)
    px, po, ptag = d_x.data_ptr(), d_out.data_ptr(), tag.ctypes.data
    d_ok = torch.zeros((n, 3, 4), dtype=torch.int64, device="cuda")
    vals = [[v * ref.R_INV % RR for v in ref.raw_ints(x[i].view(np.uint32).reshape(3, 8))] for i in range(n)]
    want = ref.mont([v for s in vals for v in ref.permute(s, *p)])
    torch.cuda.synchronize()
    P, H, M = lib.blsgpu_fr_poseidon_permute_device, lib.blsgpu_fr_poseidon_hash_many_device, lib.blsgpu_fr_poseidon_merkle_device

    def still_works(after):
        """a valid call after the refusals: nothing was launched or left behind, and the refused calls wrote nothing"""
        d_ok.zero_()
        torch.cuda.synchronize()
        assert P(hctx, hh, vp(px), n, vp(d_ok.data_ptr())) == 0, (after, err())
        ctx.synchronize()
        assert ints(host(d_ok)) == want, after
        assert not d_out.any().item() and np.array_equal(host(d_x).reshape(x.shape), x), "a refused call wrote something (%s)" % after
    still_works("create")
    # NULLs
    assert P(hctx, hh, None, n, vp(po)) == ERR_ARG and "NULL" in err()
    assert P(hctx, hh, vp(px), n, None) == ERR_ARG and "NULL" in err()
    assert P(hctx, None, vp(px), n, vp(po)) == ERR_ARG and "NULL handle" in err()
    assert P(None, hh, vp(px), n, vp(po)) == ERR_ARG
    assert H(hctx, hh, None, vp(px), n, vp(po)) == ERR_ARG and "tag" in err()
    assert H(hctx, hh, vp(bad_tag.ctypes.data), vp(px), n, vp(po)) == ERR_ARG and "tag" in err()
    assert H(hctx, hh, vp(ptag), None, n, vp(po)) == ERR_ARG and "NULL" in err()
    assert M(hctx, hh, vp(ptag), None, 3, 1, None, vp(po)) == ERR_ARG and "NULL" in err()
    assert M(hctx, hh, vp(ptag), vp(px), 3, 1, None, None) == ERR_ARG and "NULL" in err()
    still_works("NULLs and a bad tag")
    # misalignment
    assert P(hctx, hh, vp(px + 8), n - 1, vp(po)) == ERR_ARG and "aligned" in err()
    assert P(hctx, hh, vp(px), n, vp(po + 8)) == ERR_ARG and "aligned" in err()
    assert H(hctx, hh, vp(ptag), vp(px + 8), n, vp(po)) == ERR_ARG and "aligned" in err()
    assert M(hctx, hh, vp(ptag), vp(px), 3, 1, vp(po + 8), vp(po + 1024)) == ERR_ARG and "aligned" in err()
    assert M(hctx, hh, vp(ptag), vp(px), 3, 1, None, vp(po + 4)) == ERR_ARG and "aligned" in err()
    still_works("misalignment")
    # overlaps: permute allows out == in only
    assert P(hctx, hh, vp(po), n, vp(po + 32)) == ERR_ARG and "overlap" in err()
    assert P(hctx, hh, vp(po + 32), n, vp(po)) == ERR_ARG and "overlap" in err()
    assert P(hctx, hh, vp(po), n, vp(po + n * 96 - 32)) == ERR_ARG and "overlap" in err()
    assert H(hctx, hh, vp(ptag), vp(po), n, vp(po)) == ERR_ARG and "overlap" in err()
    assert H(hctx, hh, vp(ptag), vp(po), n, vp(po + n * 64 - 32)) == ERR_ARG and "overlap" in err()
    still_works("permute / hash overlaps")
    # merkle, 8 leaves, height 3: 7 nodes, 1 root
    assert M(hctx, hh, vp(ptag), vp(po), 3, 1, None, vp(po + 7 * 32)) == ERR_ARG and "overlap" in err()           # roots inside the leaves
    assert M(hctx, hh, vp(ptag), vp(po), 3, 1, vp(po + 7 * 32), vp(po + 1024)) == ERR_ARG and "overlap" in err()  # nodes on the last leaf
    assert M(hctx, hh, vp(ptag), vp(po), 3, 1, vp(po + 512), vp(po + 512 + 6 * 32)) == ERR_ARG and "overlap" in err()      # roots on the last node
    still_works("merkle overlaps")
    # sizes: 2^28 and 64-bit overflow
    assert P(hctx, hh, vp(px), (1 << 28) // 3 + 1, vp(po)) == ERR_ARG and "2^28" in err()
    assert P(hctx, hh, vp(px), (1 << 63), vp(po)) == ERR_ARG and "2^28" in err()
    assert H(hctx, hh, vp(ptag), vp(px), (1 << 64) - 1, vp(po)) == ERR_ARG and "2^28" in err()
    assert M(hctx, hh, vp(ptag), vp(px), 29, 1, None, vp(po)) == ERR_ARG and "height" in err()
    assert M(hctx, hh, vp(ptag), vp(px), -1, 1, None, vp(po)) == ERR_ARG and "height" in err()
    assert M(hctx, hh, vp(ptag), vp(px), 28, 2, None, vp(po)) == ERR_ARG and "2^28" in err()
    assert M(hctx, hh, vp(ptag), vp(px), 10, (1 << 64) - 1, None, vp(po)) == ERR_ARG and "2^28" in err()
    still_works("sizes")
    # no-ops
    assert P(hctx, hh, None, 0, None) == 0 and H(hctx, hh, vp(ptag), None, 0, None) == 0 and M(hctx, hh, vp(ptag), None, 5, 0, None, None) == 0
    still_works("no-ops")
    # host forms share the checks
    y = np.zeros((n, 3, 4), dtype=np.uint64)
    assert lib.blsgpu_fr_poseidon_permute(hctx, hh, None, n, vp(y.ctypes.data)) == ERR_ARG and "NULL" in err()
    assert lib.blsgpu_fr_poseidon_permute(hctx, hh, vp(x.ctypes.data), n, vp(x.ctypes.data + 32)) == ERR_ARG and "overlap" in err()
    assert lib.blsgpu_fr_poseidon_hash_many(hctx, hh, vp(ptag), vp(x.ctypes.data), n, vp(x.ctypes.data)) == ERR_ARG and "overlap" in err()
    still_works("host forms")
    assert not y.any()
    assert ints(h.permute(x)) == want
    inplace = x.copy()
    assert lib.blsgpu_fr_poseidon_permute(hctx, hh, vp(inplace.ctypes.data), n, vp(inplace.ctypes.data)) == 0      # out == in: the in-place form
    assert ints(inplace) == want
    h.close()


def test_cpp_mirror(ctx, tmp_path):
    """include/bls12_381.hpp bls::FrPoseidon compiled with g++ against libblsgpu.so: permute, hash_many and merkle agree with one another
    and with a Merkle tree rebuilt from hash_many calls"""
    import bls12_381_amd as b
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "fr_poseidon_test")
    libdir = os.path.dirname(b.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "fr_poseidon_test.cpp"),
                           "-L" + libdir, "-lblsgpu", "-Wl,-rpath," + libdir, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "fr_poseidon ok" in out.stdout, out.stdout + out.stderr
