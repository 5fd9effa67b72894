"""tests/fr_edwards_ref.py pinned against itself: the Python-integer reference the twisted Edwards tests compare with has to be a group
law before anything is compared with it.  No GPU, no library."""
import random

import pytest

import fr_edwards_ref as ref
import fr_edwards_cases as cases

CURVES = [ref.JUBJUB, ref.BANDERSNATCH]


@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_parameters(cv):
    """the constants the issue states: d as the quotient it is defined by, the expected `complete` verdicts, prime s"""
    if cv is ref.JUBJUB:
        assert cv.a == ref.RR - 1 and cv.d == (-10240 * ref.inv(10241)) % ref.RR
        assert ref.is_square(cv.a) and cv.complete
    else:
        assert cv.a == ref.RR - 5 and cv.d == 138827208126141220649022263972958607803 * ref.inv(171449701953573178309673572579671231137) % ref.RR
        assert not ref.is_square(cv.a) and not cv.complete
    assert not ref.is_square(cv.d)
    assert pow(2, cv.s - 1, cv.s) == 1 and pow(3, cv.s - 1, cv.s) == 1          # s passes two Fermat tests


@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_group_law(cv):
    """associativity and commutativity on random triples, the identity, inverses, closure"""
    rng = random.Random(11)
    for _ in range(8):
        p, q, t = (cv.odd_order_point(rng) for _ in range(3))
        assert cv.on_curve(p) and cv.on_curve(cv.add(p, q))
        assert cv.add(p, q) == cv.add(q, p)
        assert cv.add(cv.add(p, q), t) == cv.add(p, cv.add(q, t))
        assert cv.add(p, (0, 1)) == p and cv.add(p, cv.neg(p)) == (0, 1)


@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_order(cv):
    """[h s] P = O for sampled points, [s] P != O for a point with a small-order part, [s] P = O in the prime-order subgroup"""
    rng = random.Random(5)
    saw_cofactor = False
    for _ in range(6):
        p = cv.sample(rng)
        assert cv.on_curve(p)
        if cv.complete:                                             # any curve point may be multiplied on a complete curve
            assert cv.mul(cv.h * cv.s, p) == (0, 1)
            saw_cofactor |= cv.mul(cv.s, p) != (0, 1)
        q = cv.mul(cv.h, p) if cv.complete else cv.odd_order_point(rng)
        assert cv.mul(cv.s, q) == (0, 1)
    assert saw_cofactor or not cv.complete


@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_double_and_add_is_repeated_addition(cv):
    rng = random.Random(3)
    p = cv.odd_order_point(rng)
    acc = (0, 1)
    for n in range(40):
        assert cv.mul(n, p) == acc
        acc = cv.add(acc, p)
    ks = [0, 1, 2, cv.s - 1, cv.s, rng.getrandbits(253)]
    assert cv.mul_many(ks, [p] * len(ks)) == [cv.mul(k, p) for k in ks]      # the lock-step form the shared cases use


def test_jubjub_small_order_points():
    cv = ref.JUBJUB
    two, four_a, four_b = ref.jubjub_small_points()
    assert cv.on_curve(two) and cv.add(two, two) == (0, 1)
    for f in (four_a, four_b):
        assert cv.on_curve(f) and cv.add(f, f) == two and cv.mul(4, f) == (0, 1)
    assert cv.add(four_a, four_b) == (0, 1)


def test_the_law_raises_on_a_zero_denominator():
    """an exceptional pair is refused, not given a value: with d = 4 any coordinates whose product is 1 / d make 1 - d x1 x2 y1 y2 vanish
    (the law is applied to the coordinates as they are; they need not lie on a curve for this)"""
    cv = ref.Curve("toy", 1, 4, 1, 1)
    with pytest.raises(ref.ZeroDenominator):
        cv.add((1, 1), (ref.inv(4), 1))
    with pytest.raises(ref.ZeroDenominator):
        cv.add((1, 1), (ref.RR - ref.inv(4), 1))                     # and 1 + d x1 x2 y1 y2


def test_digits_restate_the_scalar():
    """the recoding as the reference restates it: the digits sum back to the scalar and stay in the table's range"""
    rng = random.Random(2)
    for bits in (1, 2, 3, 64, 253, 256):
        for window in range(2, 9):
            for k in [0, 1, (1 << bits) - 1] + [rng.getrandbits(bits) for _ in range(20)]:
                dg = ref.digits(k, bits, window)
                assert len(dg) == ref.windows(bits, window)
                assert sum(v << (window * w) for w, v in enumerate(dg)) == k
                assert all(abs(v) <= 1 << (window - 1) for v in dg)


@pytest.mark.parametrize("name", ["jubjub", "bandersnatch"])
def test_no_denominator_vanishes_in_the_shared_cases(name):
    """every input set the emulation and GPU tests use goes through the affine law without an exceptional case (on Bandersnatch every
    point has odd order), and the expectations are curve points"""
    c = cases.mul_cases(name)
    assert len(c["points"]) == len(c["scalars"][64]) and all(ref.CURVES[name].on_curve(p) for p in c["points"])
    for bits, want in c["want"].items():
        assert all(ref.CURVES[name].on_curve(p) for p in want), bits
    for n in (1, 8, 64):
        assert all(ref.CURVES[name].on_curve(p) for p in cases.base_set(name, n)["points"])
    for kind, n, bits, chunk in (("long", 64, 253, 8), ("shared", 8, 3, 256), ("natural", 64, 253, 256), ("cancel", 8, 256, 256)):
        c = cases.msm_case(name, kind, n, bits, chunk)
        assert len(c["want"]) == len(c["offsets"]) - 1 and all(ref.CURVES[name].on_curve(p) for p in c["want"])
