"""Points and expectations shared by the group transform tests (tests/test_simt_gntt.py on the host emulation, tests/test_g_ntt.py on the GPU):
oracle points <-> projective wire records, and the two statements of the transform in oracle terms.  Every expectation is computed by
oracle/bls12_381_ref.py in Python integers; nothing here touches the library."""
import numpy as np

from oracle import bls12_381_ref as o

RR = o.R_ORDER


class Group:
    def __init__(self, g):
        self.id = g
        self.words = 18 * g                                    # u64 per projective wire point
        self.mul, self.add, self.sum = (o.g1_mul, o.g1_add, o.g1_sum) if g == 1 else (o.g2_mul, o.g2_add, o.g2_sum)
        self.to_affine = o.g1_to_affine if g == 1 else o.g2_to_affine
        self.identity = o.g1_identity() if g == 1 else o.g2_identity()
        self.gen = o.g1_from_affine(o.G1_GEN) if g == 1 else o.g2_from_affine(o.G2_GEN)
        self._cache = {}

    def base_mul(self, s):
        """[s] G as a projective oracle point (Z != 1 in general: the oracle's own addition chain), cached"""
        s = int(s) % RR
        if s not in self._cache:
            self._cache[s] = self.mul(self.gen, s)
        return self._cache[s]

    def mul_cached(self, p, s):
        key = (p, int(s) % RR)
        if key not in self._cache:
            self._cache[key] = self.mul(p, s)
        return self._cache[key]

    def _coord(self, c):
        if self.id == 1:
            return o.fp_to_mont_limbs(c)
        return o.fp_to_mont_limbs(c[0]) + o.fp_to_mont_limbs(c[1])

    def _uncoord(self, limbs):
        limbs = [int(v) for v in limbs]
        if self.id == 1:
            return o.fp_from_mont_limbs(limbs)
        return (o.fp_from_mont_limbs(limbs[:6]), o.fp_from_mont_limbs(limbs[6:]))

    def wire(self, points):
        """projective oracle points -> (len, 18 | 36) u64"""
        rows = [self._coord(p[0]) + self._coord(p[1]) + self._coord(p[2]) for p in points]
        return np.array(rows, dtype=np.uint64).reshape(len(points), self.words)

    def affine(self, wire):
        """(…, 18 | 36) u64 (or the same bytes as u32) -> the oracle's affine triples (x, y, infinity)"""
        w = np.ascontiguousarray(wire).view(np.uint64).reshape(-1, self.words)
        c = self.words // 3
        return [self.to_affine((self._uncoord(r[:c]), self._uncoord(r[c:2 * c]), self._uncoord(r[2 * c:]))) for r in w]

    def affine_of(self, points):
        return [self.to_affine(p) for p in points]


G = {1: Group(1), 2: Group(2)}


def naive(grp, pts, inverse=False):
    """the definition, term by term: Y[m] = sum_j [w^(jm)] P[j]; inverse P[j] = [n^-1] sum_m [w^(-jm)] Y[m].  The n^2 terms of a vector
    are oracle products [w^e] P, e = +-jm mod n, kept in a cache per (point, scalar): vectors that share points share the products."""
    n = len(pts)
    log_n = n.bit_length() - 1
    w = o.fr_omega(log_n)
    sign = -1 if inverse else 1
    ident = grp.to_affine(grp.identity)
    live = [j for j in range(n) if grp.to_affine(pts[j]) != ident]       # [s] identity = identity: not worth an oracle product
    out = [grp.sum(grp.mul_cached(pts[j], pow(w, sign * j * m % n, RR)) for j in live) for m in range(n)]
    if inverse:
        ninv = pow(n, -1, RR)
        out = [grp.mul(p, ninv) for p in out]
    return out


def dlog_expect(grp, scalars, inverse=False):
    """the transform of [s_j] G is [fr_ntt(s)_m] G"""
    return [grp.base_mul(v) for v in o.fr_ntt(list(scalars), inverse=inverse)]


def scalars(n, seed, special=False):
    r = o.SplitMix64(seed)
    s = [r.scalar() for _ in range(n)]
    if special and n >= 4:                                                 # 0, 1 and r - 1 among the s_j
        s[0], s[n // 2], s[n - 1] = 0, 1, RR - 1
    return s
