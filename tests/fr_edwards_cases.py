"""The inputs and expectations the twisted Edwards tests share (tests/test_fr_edwards.py on the GPU, tests/test_simt_fr_edwards.py on the
host emulation, tests/test_fr_edwards_ref.py for the exceptional cases): built once per process from tests/fr_edwards_ref.py, never
changed afterwards.  Test infrastructure only.

Points.  Seven special points come first: on Jubjub the identity, a prime-order point G, (0, -1), both points of order 4 and G plus a
small-order point (twice); on Bandersnatch the identity and six points of odd order (the curve is not complete: nothing else is a valid
input).  Each meets the nine special scalars of its `bits`, so the first 63 pairs hold every special case; random pairs follow.
Bases have known logarithms to G (and, on Jubjub, a known multiple of a point T of order 4), so the expectation of a segment is ONE
product whatever its length."""
import functools
import random

import fr_edwards_ref as ref

MUL_BITS = (1, 3, 64, 253, 256)
MUL_N = 257
N_SPECIAL_POINTS, N_SPECIAL_SCALARS = 7, 9


def carry_pattern(window):
    """every window of `window` bits at exactly 2^(window-1): 0x88...8 for window 4"""
    return sum((1 << (window - 1)) << (window * w) for w in range(256 // window + 1)) & ((1 << 256) - 1)


def special_scalars(cv, bits, rng):
    m = (1 << bits) - 1
    fit = lambda v: v if v <= m else rng.getrandbits(bits)
    out = [0, 1, m, fit(cv.s), fit(cv.h * cv.s), carry_pattern(3) & m, carry_pattern(4) & m, carry_pattern(8) & m, fit((1 << 256) - 1)]
    assert len(out) == N_SPECIAL_SCALARS
    return out


@functools.lru_cache(None)
def special_points(name):
    cv = ref.CURVES[name]
    rng = random.Random(101 if cv.complete else 202)
    g = cv.odd_order_point(rng)
    if cv.complete:
        two, f1, f2 = ref.jubjub_small_points()
        pts = [(0, 1), g, two, f1, f2, cv.add(g, f1), cv.add(g, two)]
    else:
        pts = [(0, 1), g] + [cv.odd_order_point(rng) for _ in range(5)]
    assert len(pts) == N_SPECIAL_POINTS
    return pts


@functools.lru_cache(None)
def mul_cases(name):
    """points[i], scalars[bits][i], want[bits][i] = scalars[bits][i] * points[i] (affine) for i < MUL_N and every bits of MUL_BITS"""
    cv = ref.CURVES[name]
    rng = random.Random(303 if cv.complete else 404)
    sp = special_points(name)
    points = [sp[i // N_SPECIAL_SCALARS] for i in range(N_SPECIAL_POINTS * N_SPECIAL_SCALARS)]
    while len(points) < MUL_N:
        # a complete curve takes ANY curve point; the other one points of odd order only
        points.append(cv.sample(rng) if cv.complete and len(points) % 2 else cv.odd_order_point(rng))
    scalars, want = {}, {}
    for bits in MUL_BITS:
        ks = [special_scalars(cv, bits, rng)[i % N_SPECIAL_SCALARS] for i in range(N_SPECIAL_POINTS * N_SPECIAL_SCALARS)]
        ks += [rng.getrandbits(bits) for _ in range(MUL_N - len(ks))]
        scalars[bits] = ks
        want[bits] = cv.mul_many(ks, points)
    return {"points": points, "scalars": scalars, "want": want}


@functools.lru_cache(None)
def base_set(name, n):
    """n bases B_i = dl[i] G + tors[i] T.  From 8 bases on: base 1 repeats base 0 (terms that cancel), and on Jubjub base 2 is the identity
    and base 3 has a component of order 4"""
    cv = ref.CURVES[name]
    rng = random.Random(1000 + n + (0 if cv.complete else 7))
    g = special_points(name)[1]
    t4 = ref.jubjub_small_points()[1] if cv.complete else None
    dl = [rng.randrange(1, 1 << 20) for _ in range(n)]
    tors = [0] * n
    if n >= 8:
        dl[1] = dl[0]
        if cv.complete:
            dl[2], tors[3] = 0, 1
    pts = [cv.add(p, t4) if t else p for p, t in zip(cv.mul_many(dl, [g] * n), tors)]
    return {"g": g, "t4": t4, "points": pts, "dl": dl, "tors": tors}


def _scalars(rng, bits, count):
    m = (1 << bits) - 1
    pool = [0, 1, m, carry_pattern(2) & m, carry_pattern(4) & m, carry_pattern(8) & m]
    return [pool[rng.randrange(len(pool))] if rng.randrange(8) == 0 else rng.getrandbits(bits) for _ in range(count)]


def _finish(name, bs, lens, firsts, bits, rng, scalars=None):
    offsets = [0]
    for l in lens:
        offsets.append(offsets[-1] + l)
    ks = scalars if scalars is not None else _scalars(rng, bits, offsets[-1])
    nat = firsts is None
    fl = [offsets[j] for j in range(len(lens))] if nat else firsts
    cv = ref.CURVES[name]
    es = [sum(k * bs["dl"][fl[j] + i] for i, k in enumerate(ks[offsets[j]:offsets[j + 1]])) % cv.s for j in range(len(lens))]
    want = cv.mul_many(es, [bs["g"]] * len(es))
    for j in range(len(lens)):                                       # the small-order parts (Jubjub's base 3), segment by segment
        t = sum(k * bs["tors"][fl[j] + i] for i, k in enumerate(ks[offsets[j]:offsets[j + 1]])) % 4
        if t:
            want[j] = cv.add(want[j], cv.mul(t, bs["t4"]))
    return {"n": len(bs["points"]), "bits": bits, "offsets": offsets, "base_first": None if nat else list(firsts), "scalars": ks, "want": want}


@functools.lru_cache(None)
def msm_case(name, kind, n, bits, chunk):
    """kind "long": segments around the chunk size over random (overlapping) slices of n >= 3 chunk + 5 bases: empty, length 1, exactly a
    chunk, one less, one more, three chunks and five, 300 short ones around a long one.  "shared": 300 segments over one slice
    (base_first all 0).  "natural": base_first == NULL, the segments tile the first bases.  "cancel": terms that cancel within a segment
    (s B; (h s - 1) B + B; the identity base; the base with a small-order part), bits must hold h s."""
    cv = ref.CURVES[name]
    bs = base_set(name, n)
    rng = random.Random(sum(ord(ch) for ch in kind) * 1000003 + n * 131 + bits * 17 + chunk)
    if kind == "long":
        shorts = lambda: [rng.randrange(4) for _ in range(150)]
        lens = [0, 1, chunk, chunk - 1, chunk + 1, 0, 3 * chunk + 5] + shorts() + [2 * chunk + 3] + shorts() + [0]
        firsts = [rng.randrange(n - l + 1) for l in lens]
        return _finish(name, bs, lens, firsts, bits, rng)
    if kind == "shared":
        lens = [n, 0, 1] + [rng.randrange(n + 1) for _ in range(297)]
        return _finish(name, bs, lens, [0] * len(lens), bits, rng)
    if kind == "natural":
        lens, left = [0], n
        while left:
            l = min(left, rng.randrange(1, 9))
            lens += [l, 0] if rng.randrange(3) == 0 else [l]
            left -= l
        return _finish(name, bs, lens, None, bits, rng)
    assert kind == "cancel" and n >= 8 and (cv.h * cv.s) >> bits == 0
    hs = cv.h * cv.s
    lens = [1, 2, 2, 3, 2]
    firsts = [0, 0, 0, 1, 3]
    ks = [cv.s, hs - 1, 1, cv.s - 1, 1, 5, 7, 9, hs - 1, 1]
    out = _finish(name, bs, lens, firsts, bits, rng, scalars=ks)
    assert out["want"][0] == (0, 1) and out["want"][1] == (0, 1) and out["want"][2] == (0, 1)
    return out
