"""Inputs and expectations shared by the segmented point-sum tests (tests/test_simt_gsum.py on the host emulation, tests/test_g_sum_segments.py
and tests/test_bls_aggregate.py on the GPU): a pool of affine oracle points with the awkward ones in it, the edge-case segment lists in
CSR form, the wire arrays, and every segment's sum computed by oracle/bls12_381_ref.py (`g1_sum` / `g2_sum` over `from_affine`) in Python
integers.  Nothing here touches the library."""
import functools

import numpy as np

from oracle import bls12_381_ref as o

from g_ntt_points import G


def _off_subgroup(group):
    """a curve point outside the prime-order subgroup: the first small x with a square right-hand side whose point is not torsion free"""
    for x in range(1, 200):
        if group == 1:
            b = bytearray(x.to_bytes(48, "big"))
            b[0] |= 0x80
            a = o.g1_from_compressed_unchecked(bytes(b))
            if a is not None and not o.g1_is_torsion_free(a):
                return a
        else:
            b = bytearray((0).to_bytes(48, "big") + x.to_bytes(48, "big"))      # c1 first, then c0 = x
            b[0] |= 0x80
            a = o.g2_from_compressed_unchecked(bytes(b))
            if a is not None and not o.g2_is_torsion_free(a):
                return a
    raise AssertionError("no off-subgroup point found")


class Pool:
    """ident: the identity; p, np_: a point and its negative; off: a curve point outside the subgroup; rest: plain subgroup points"""
    def __init__(self, group, n_plain=20, seed=77):
        self.group = group
        grp = G[group]
        r = o.SplitMix64(seed + group)
        self.points = [grp.to_affine(grp.base_mul(r.scalar())) for _ in range(n_plain)]
        self.ident = len(self.points)
        self.points.append(o.G1_IDENTITY_AFF if group == 1 else o.G2_IDENTITY_AFF)
        self.p = 0
        self.np_ = len(self.points)
        x, y, _ = self.points[0]
        self.points.append((x, (-y) % o.P, False) if group == 1 else (x, o.fp2_neg(y), False))
        self.off = len(self.points)
        self.points.append(_off_subgroup(group))
        self.plain = list(range(1, n_plain))


@functools.lru_cache(maxsize=None)
def pool(group):
    return Pool(group)


def wire_points(group, pts):
    """affine oracle triples -> ((n, 12 | 24) u64, (n,) u8)"""
    w = 12 * group
    xy = np.zeros((len(pts), w), dtype=np.uint64)
    inf = np.zeros(len(pts), dtype=np.uint8)
    for i, (x, y, f) in enumerate(pts):
        if group == 1:
            xy[i] = o.fp_to_mont_limbs(x) + o.fp_to_mont_limbs(y)
        else:
            xy[i] = o.fp_to_mont_limbs(x[0]) + o.fp_to_mont_limbs(x[1]) + o.fp_to_mont_limbs(y[0]) + o.fp_to_mont_limbs(y[1])
        inf[i] = 1 if f else 0
    return xy, inf


def edge_segments(group, chunk, seed, long_chunks=3):
    """the edge-case segments as lists of pool indices: lengths 0, 1, 2, chunk - 1, chunk, chunk + 1, long_chunks chunks + 1; identities at the
    start, in the middle and at the end of a segment; one point five times; P, -P, Q; identities only; a point outside the subgroup;
    an empty segment first and last."""
    pl = pool(group)
    r = np.random.RandomState(seed)
    some = lambda n: [int(pl.plain[k]) for k in r.randint(0, len(pl.plain), n)]
    q = pl.plain[3]
    segs = [[], some(1), some(2), some(chunk - 1), [pl.ident] + some(2) + [pl.ident] + some(1) + [pl.ident], [pl.p] * 5, [pl.p, pl.np_, q], some(chunk + 1),
            [pl.ident] * 3, [], [], [pl.off] + some(1), some(long_chunks * chunk + 1), [pl.p, pl.np_], some(chunk), some(1), []]
    return segs


def skewed_segments(group, short, longest, seed):
    """`short` segments of at most 8 terms and one of `longest` in their middle"""
    pl = pool(group)
    r = np.random.RandomState(seed)
    some = lambda n: [int(pl.plain[k]) for k in r.randint(0, len(pl.plain), n)]
    segs = [some(int(r.randint(0, 9))) for _ in range(short)]
    segs.insert(short // 2, some(longest))
    return segs


def csr(segs):
    off = np.zeros(len(segs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in segs])
    return off


def expected(group, segs, skip=()):
    """the affine oracle sum of every segment (pool indices); None for the segments in `skip`"""
    grp, pl = G[group], pool(group)
    from_aff = o.g1_from_affine if group == 1 else o.g2_from_affine
    proj = [from_aff(a) for a in pl.points]
    return [None if i in skip else grp.to_affine(grp.sum(proj[k] for k in s)) for i, s in enumerate(segs)]


def gathered(group, segs):
    """the call WITH idx: (xy, inf) of the pool, idx, offsets"""
    xy, inf = wire_points(group, pool(group).points)
    idx = np.array([k for s in segs for k in s], dtype=np.uint32)
    return xy, inf, idx, csr(segs)


def contiguous(group, segs, extra=2):
    """the call WITHOUT idx: term t is point t; `extra` points behind the last term are never named"""
    pl = pool(group)
    pts = [pl.points[k] for s in segs for k in s] + [pl.points[pl.off]] * extra
    xy, inf = wire_points(group, pts)
    return xy, inf, None, csr(segs)


def check(group, out_wire, want, what):
    """out_wire: (nseg, 18 | 36) u64 projective -> compared as affine oracle points with `want` (None entries are skipped)"""
    got = G[group].affine(out_wire)
    assert len(got) == len(want), what
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if w is not None and g != w]
    assert not bad, "%s: segments %s differ from the oracle's sums" % (what, bad[:10])
