"""The field products and the mixed addition of the G1 bucket accumulation, run on the HOST (tests/simt) against Python integers.

`k_msm_accumulate<FpPolicy>` calls `xyzz_add_mixed_inl<true>` (curve.hip.h): every column sum of its nine inlined products is one
multiply-add chain in source order that starts from the previous column's carry (`mac()` in fe.hip.h).  The arithmetic is that of the
free order, so the two forms must agree limb for limb and both with the integers -- at the extremes the operand types allow, where a
column sum comes closest to 2^64:

  * every limb at A * (2^28 - 1) for the (A1, A2) pairs the formula instantiates (the VALUE bound is deliberately ignored there: the
    result is only required to be the right residue with normalised low limbs);
  * values 0, 1, p - 1 and V * p - 1, in normalised limbs and with limbs spread up to the type's limb bound;
  * 10^4 seeded random operand sets per product.

The point cases run the accumulation kernel itself on hand-built items (tests/simt_msm_child.py): the projective record it stores is
compared LIMB FOR LIMB with a Python model of the same formulas (madd-2008-s with its exact exceptional cases, then X ZZZ : Y ZZ :
ZZ ZZZ), not only as a group element.  The host build has no asm statement (fe.hip.h), so this checks arithmetic and bounds; that the
GPU build computes the same is tests/test_msm_acc_gpu.py."""
import ctypes

import numpy as np
import pytest

import simt_harness
import simt_msm_child as msm_child
from oracle import bls12_381_ref as o
from oracle import c_oracle

P = o.P
NL, LW = 14, 28
LMASK = (1 << LW) - 1
RP_INV = pow(1 << (NL * LW), -1, P)                                # the internal Montgomery factor R' = 2^392
# kind -> the (A, V) operand types of tests/simt/emu_fe_acc.cpp; every result is Fe<1, 2>
KINDS = {0: [(1, 1), (1, 12)], 1: [(2, 2), (1, 12)], 2: [(3, 15), (1, 2)], 3: [(1, 12), (1, 2)], 4: [(3, 15)], 5: [(3, 15), (3, 12), (2, 13), (1, 2)]}
KIND_IDS = ["U2", "S2", "PPP", "Q", "sqr", "sop2"]


@pytest.fixture(scope="module")
def lib():
    path = simt_harness.emu_lib(lambda: simt_harness.build("emu_fe_acc_test", "emu_fe_acc.cpp", sanitize=False))
    l = ctypes.CDLL(path)
    l.emu_fe_acc_products.restype = ctypes.c_int
    return l


def _limbs(v):
    """normalised limbs of v: 13 of 28 bits and the rest in the top limb"""
    out = [(v >> (LW * i)) & LMASK for i in range(NL - 1)] + [v >> (LW * (NL - 1))]
    assert out[-1] < 1 << 32
    return out


def _value(l):
    return sum(int(x) << (LW * i) for i, x in enumerate(l))


def _spread(l, a, rng):
    """the same value with limbs borrowed downwards, none above a * (2^28 - 1)"""
    l = list(l)
    for i in range(NL - 2, -1, -1):
        room = (a * LMASK - l[i]) >> LW
        take = min(room, l[i + 1], int(rng.randint(0, a)))
        l[i] += take << LW
        l[i + 1] -= take
    return l


def _expected(kind, vals):
    if kind == 4:
        return vals[0] * vals[0] * RP_INV % P
    if kind == 5:
        return (vals[0] * vals[1] + vals[2] * vals[3]) * RP_INV % P
    return vals[0] * vals[1] * RP_INV % P


def _run(lib, kind, ops, seq):
    n = len(ops)
    a = np.zeros((n, 4, NL), dtype=np.uint32)
    for i, row in enumerate(ops):
        for j, l in enumerate(row):
            a[i, j] = l
    out = np.zeros((n, NL), dtype=np.uint32)
    rc = lib.emu_fe_acc_products(kind, seq, a.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(n))
    assert rc == 0
    return out


def _check(lib, kind, ops, in_bound):
    got = _run(lib, kind, ops, 1)
    assert np.array_equal(got, _run(lib, kind, ops, 0)), "the two orders of the column sums differ"
    for row, g in zip(ops, got):
        assert all(int(x) <= LMASK for x in g[:NL - 1]), "low limbs of a product are normalised"
        v = _value(g)
        assert v % P == _expected(kind, [_value(l) for l in row])
        if in_bound:
            assert v < 2 * P


@pytest.mark.parametrize("kind", sorted(KINDS), ids=KIND_IDS)
def test_products_at_the_limb_bound(lib, kind):
    """every limb (the top one too) at A * (2^28 - 1): the largest column sums the static_asserts admit"""
    types = KINDS[kind]
    full = [[a * LMASK] * NL for a, _ in types]
    ops = [full]
    # each operand in turn at its bound with the others at 1 and at p - 1
    for j in range(len(types)):
        for other in (1, P - 1):
            ops.append([full[i] if i == j else _limbs(other) for i in range(len(types))])
    _check(lib, kind, ops, in_bound=False)


@pytest.mark.parametrize("kind", sorted(KINDS), ids=KIND_IDS)
def test_products_at_the_value_bound(lib, kind):
    """0, 1, p - 1 and V * p - 1 in every combination, normalised and spread to the limb bound: result < 2p"""
    import itertools
    types = KINDS[kind]
    rng = np.random.RandomState(kind)
    ops = []
    for combo in itertools.product(range(4), repeat=len(types)):
        vals = [(0, 1, P - 1, v * P - 1)[c] for c, (_, v) in zip(combo, types)]
        ops.append([_limbs(x) for x in vals])
        ops.append([_spread(_limbs(x), a, rng) for x, (a, _) in zip(vals, types)])
    for row in ops:
        for l, (a, _) in zip(row, types):
            assert all(x <= a * LMASK for x in l[:NL - 1])
    _check(lib, kind, ops, in_bound=True)


@pytest.mark.parametrize("kind", sorted(KINDS), ids=KIND_IDS)
def test_products_random(lib, kind):
    """10^4 seeded random operand sets below V * p, limbs spread at random up to the limb bound"""
    types = KINDS[kind]
    rng = np.random.RandomState(1000 + kind)
    r = o.SplitMix64(77 + kind)
    ops = []
    for _ in range(10000):
        row = []
        for a, v in types:
            x = ((r.scalar() << 256) | r.scalar()) % (v * P)
            row.append(_spread(_limbs(x), a, rng))
        ops.append(row)
    _check(lib, kind, ops, in_bound=True)


# ---- the mixed addition through the accumulation kernel -----------------------------------------------------------------------------
NEG = 1 << 31


def _model_chain(points, entries):
    """madd-2008-s with the kernel's exceptional cases on integers mod p, then xyzz_to_proj: (X, Y, Z)"""
    inf, x, y, zz, zzz = True, 0, 0, 0, 0
    for e in entries:
        q = points[e & (NEG - 1)]
        if q is None:                                                # identity base: contributes nothing
            continue
        qx, qy = q[0], (P - q[1]) % P if e & NEG else q[1]
        if inf:
            inf, x, y, zz, zzz = False, qx, qy, 1, 1
            continue
        pp_ = (qx * zz - x) % P
        rr_ = (qy * zzz - y) % P
        if pp_ == 0:
            if rr_ == 0:                                             # mdbl-2008-s-1 of the affine operand
                u = 2 * qy % P; v = u * u % P; w = u * v % P; s = qx * v % P; m = 3 * qx * qx % P
                x3 = (m * m - 2 * s) % P
                x, y, zz, zzz = x3, (m * (s - x3) - w * qy) % P, v, w
            else:
                inf = True                                           # the accumulator keeps its coordinates, the flag decides
            continue
        pp = pp_ * pp_ % P; ppp = pp_ * pp % P; q_ = x * pp % P
        x3 = (rr_ * rr_ - ppp - 2 * q_) % P
        x, y, zz, zzz = x3, (rr_ * (q_ - x3) - y * ppp) % P, zz * pp % P, zzz * ppp % P
    if inf:
        return (0, 1, 0)
    return (x * zzz % P, y * zz % P, zz * zzz % P)


def _wire(coords):
    return np.concatenate([np.array(o.fp_to_mont_limbs(c), dtype=np.uint64) for c in coords])


def test_mixed_addition_chains_limb_for_limb():
    c_oracle.build()
    simt_harness.emu_lib(msm_child.build)
    ks = [3, 5, 5, o.R_ORDER - 5, 0, 11, 0x1234567, o.R_ORDER - 1, 2, 7]
    ID = 4
    aff = [o.g1_to_affine(o.g1_affine_mul(o.G1_GEN, k)) if k else None for k in ks]
    points = [None if a is None else (a[0], a[1]) for a in aff]
    xy = np.stack([_wire(p) if p is not None else _wire((0, 1)) for p in points])
    inf = np.array([p is None for p in points], dtype=np.uint8)
    n = len(ks)
    lists = [[0],                                                    # accumulator at infinity: one entry
             [0, 5],                                                 # chains of 2, 3
             [0, 5, 6],
             [1, 2],                                                 # P + P: the doubling branch
             [1, 2, 6],
             [1, 3],                                                 # P + (-P): two records
             [1, 1 | NEG],                                           # P + (-P) through the sign bit
             [1, 3, 0],                                              # ... and a further point after the cancellation
             [ID],                                                   # identity base alone
             [ID, 0, ID, 5, ID],
             [0 | NEG],                                              # a negative-digit entry first
             [6, 7 | NEG, 8],
             [[0, 5, 6, 7, 8, 9][i % 6] | (NEG if i % 4 == 3 else 0) for i in range(65)]]
    sorted_, items = [], []
    for d, l in enumerate(lists):
        items.append((len(sorted_), len(l), d))
        sorted_ += l
    jobs = [{"op": "bases", "label": "bases", "group": 1, "xy": xy, "inf": inf},
            {"op": "accumulate", "label": "chains", "bases": 0, "nsplit": 0xFFFFFFFF, "sorted": np.array(sorted_, dtype=np.uint32),
             "items": np.array(items, dtype=np.uint32), "ctrl": np.array([0, 0, len(items), 0], dtype=np.uint32), "max_items": len(items), "ndest": len(items)}]
    rec = msm_child.run(jobs)[1]["records"]
    for d, l in enumerate(lists):
        want = _model_chain(points, l)
        assert np.array_equal(rec[d], _wire(want)), "chain %d %s" % (d, [hex(e) for e in l[:6]])
        # and the model itself against the oracle's group law
        dlog = sum((-1 if e & NEG else 1) * ks[e & (NEG - 1)] for e in l) % o.R_ORDER
        if dlog == 0:
            assert want[2] == 0
        else:
            zi = pow(want[2], -1, P)
            a = o.g1_to_affine(o.g1_affine_mul(o.G1_GEN, dlog))
            assert (want[0] * zi % P, want[1] * zi % P) == (a[0], a[1])
