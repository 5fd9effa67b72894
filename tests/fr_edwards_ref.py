"""Twisted Edwards curves a x^2 + y^2 = 1 + d x^2 y^2 over Fr in Python integers, written from the curve equation: what the tests of
`blsgpu_fr_edwards_*` compare with (tests/test_fr_edwards_ref.py pins this file against itself first).

The addition is the AFFINE law with modular inverses and RAISES on a zero denominator: a test whose inputs would meet an exceptional
case of an incomplete curve fails here instead of comparing two unspecified values.  The two parameter sets are TEST DATA (the library
ships none): Jubjub (a = -1, a square: complete) and Bandersnatch (a = -5, a non-square: not complete; its test points are 4 times a
sampled point, so they have odd order).  Test infrastructure only."""
import numpy as np

RR = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001      # r, the order of Fr
MONT = 1 << 256


class ZeroDenominator(ArithmeticError):
    pass


def inv(x):
    x %= RR
    if x == 0:
        raise ZeroDenominator("a denominator of the addition law vanished")
    return pow(x, -1, RR)


def is_square(x):
    return pow(x % RR, (RR - 1) // 2, RR) == 1


def sqrt(x):
    """Tonelli-Shanks in Fr (r - 1 = 2^32 q); None for a non-square"""
    x %= RR
    if x == 0:
        return 0
    if not is_square(x):
        return None
    q, s = RR - 1, 0
    while q % 2 == 0:
        q //= 2
        s += 1
    z = 2
    while is_square(z):
        z += 1
    m, c, t, res = s, pow(z, q, RR), pow(x, q, RR), pow(x, (q + 1) // 2, RR)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1:
            t2 = t2 * t2 % RR
            i += 1
        b = pow(c, 1 << (m - i - 1), RR)
        m, c = i, b * b % RR
        t, res = t * c % RR, res * b % RR
    return res


class Curve:
    def __init__(self, name, a, d, h, s):
        self.name, self.a, self.d, self.h, self.s = name, a % RR, d % RR, h, s

    @property
    def complete(self):
        return is_square(self.a) and not is_square(self.d)

    def on_curve(self, p):
        x, y = p
        return (self.a * x * x + y * y - 1 - self.d * x * x * y * y) % RR == 0

    def add(self, p, q):
        (x1, y1), (x2, y2) = p, q
        t = self.d * x1 * x2 * y1 * y2 % RR
        return ((x1 * y2 + y1 * x2) * inv(1 + t) % RR, (y1 * y2 - self.a * x1 * x2) * inv(1 - t) % RR)

    def neg(self, p):
        return ((-p[0]) % RR, p[1])

    def mul(self, k, p):
        """double-and-add from the top bit, every step the affine law above"""
        acc = (0, 1)
        for i in range(k.bit_length() - 1, -1, -1):
            acc = self.add(acc, acc)
            if (k >> i) & 1:
                acc = self.add(acc, p)
        return acc

    def add_many(self, ps, qs):
        """ps[i] + qs[i] by the same affine law, the 2 n denominators inverted together (Montgomery's trick); raises like add"""
        ts = [self.d * p[0] * q[0] * p[1] * q[1] % RR for p, q in zip(ps, qs)]
        dens = [v for t in ts for v in ((1 + t) % RR, (1 - t) % RR)]
        pre, acc = [], 1
        for v in dens:
            if v == 0:
                raise ZeroDenominator("a denominator of the addition law vanished")
            pre.append(acc)
            acc = acc * v % RR
        run, invs = inv(acc), [0] * len(dens)
        for i in range(len(dens) - 1, -1, -1):
            invs[i] = run * pre[i] % RR
            run = run * dens[i] % RR
        return [((p[0] * q[1] + p[1] * q[0]) * invs[2 * i] % RR, (p[1] * q[1] - self.a * p[0] * q[0]) * invs[2 * i + 1] % RR) for i, (p, q) in enumerate(zip(ps, qs))]

    def mul_many(self, ks, ps):
        """[ks[i] * ps[i]]: double-and-add in lock step over add_many"""
        accs = [(0, 1)] * len(ps)
        for i in range(max([k.bit_length() for k in ks] + [0]) - 1, -1, -1):
            accs = self.add_many(accs, accs)
            idx = [j for j, k in enumerate(ks) if (k >> i) & 1]
            for j, v in zip(idx, self.add_many([accs[j] for j in idx], [ps[j] for j in idx])):
                accs[j] = v
        return accs

    def sum(self, points):
        acc = (0, 1)
        for p in points:
            acc = self.add(acc, p)
        return acc

    def sample(self, rng):
        """a curve point from a random y: x^2 = (1 - y^2) / (a - d y^2)"""
        while True:
            y = rng.randrange(RR)
            den = (self.a - self.d * y * y) % RR
            if den == 0:
                continue
            x = sqrt((1 - y * y) * inv(den))
            if x is None:
                continue
            if rng.randrange(2):
                x = (-x) % RR
            return (x, y)

    def odd_order_point(self, rng):
        """h times a sampled point: a point of the prime-order subgroup (never the identity for the seeds the tests use)"""
        while True:
            p = self.mul(self.h, self.sample(rng))
            if p != (0, 1):
                return p

    def affine(self, xyz):
        """(X : Y : Z) -> (X / Z, Y / Z)"""
        zi = inv(xyz[2])
        return (xyz[0] * zi % RR, xyz[1] * zi % RR)


JUBJUB = Curve("jubjub", -1, 0x2a9318e74bfa2b48f5fd9207e6bd7fd4292d7f6d37579d2601065fd6d6343eb1, 8,
               6554484396890773809930967563523245729705921265872317281365359162392183254199)
BANDERSNATCH = Curve("bandersnatch", -5, 0x6389c12633c267cbc66e3bf86be3b6d8cb66677177e54f92b369f2f5188d58e7, 4,
                     13108968793781547619861935127046491459309155893440570251786403306729687672801)
CURVES = {"jubjub": JUBJUB, "bandersnatch": BANDERSNATCH}


def jubjub_small_points():
    """the points of order 2 and 4 of Jubjub: (0, -1) and (+-1 / sqrt(a), 0)"""
    i = inv(sqrt(JUBJUB.a))
    return [(0, RR - 1), (i, 0), (RR - i, 0)]


# ---- the signed-window recoding of csrc/fr_edwards_plan.h, restated ------------------------------------------------------------------------
def windows(bits, window):
    return (bits + window) // window


def digits(k, bits, window):
    """digit_w = window w of k + the bit below it - 2^window * the window's top bit, over the low `bits` bits of k"""
    k &= (1 << bits) - 1
    out = []
    for w in range(windows(bits, window)):
        raw = (k >> (w * window)) & ((1 << window) - 1)
        prev = (k >> (w * window - 1)) & 1 if w else 0
        out.append(raw + prev - ((raw >> (window - 1)) << window))
    return out


# ---- wire formats -----------------------------------------------------------------------------------------------------------------------------
def limbs(values):
    """ints in [0, r) -> (n, 4) u64 Montgomery limbs"""
    out = np.zeros((len(values), 4), dtype=np.uint64)
    for i, v in enumerate(values):
        m = (v % RR) * MONT % RR
        out[i] = [(m >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)]
    return out


_MONT_INV = pow(MONT, RR - 2, RR)


def ints(arr):
    """u64 Montgomery limbs (any shape ending in 4) -> the flat list of integers they stand for; limbs >= r are reduced"""
    a = np.ascontiguousarray(arr, dtype=np.uint64).reshape(-1, 4)
    return [(int(r[0]) | int(r[1]) << 64 | int(r[2]) << 128 | int(r[3]) << 192) * _MONT_INV % RR for r in a]


def raw(arr):
    """u64 limbs -> the integers the limbs spell, unreduced (to compare limb for limb)"""
    a = np.ascontiguousarray(arr, dtype=np.uint64).reshape(-1, 4)
    return [int(r[0]) | int(r[1]) << 64 | int(r[2]) << 128 | int(r[3]) << 192 for r in a]


def points_limbs(points):
    """[(x, y)] -> (n, 2, 4) u64"""
    return limbs([c for p in points for c in p]).reshape(len(points), 2, 4)


def points_of(arr):
    v = ints(arr)
    return [(v[2 * i], v[2 * i + 1]) for i in range(len(v) // 2)]


def scalar_bytes(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint8).reshape(-1, 32).copy()
