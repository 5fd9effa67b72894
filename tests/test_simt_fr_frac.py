"""The Fr fraction scans (blsgpu_fr_grand_product / blsgpu_fr_frac_sum), their device code compiled for the HOST
(tests/simt/emu_fr_frac.cpp), against Python integers mod r (tests/fr_frac_ref.py).

What runs here is the code the GPU runs: `k_frf_front<GRAND_PRODUCT | FRAC_SUM>` in both modes, then `k_frs_agg` and `k_frs_tile` in SCAN
mode on the fused output, launched step by step from the plan of csrc/fr_frac_plan.h -- the function api_fr.hip launches from -- with
its grids, blocks, LDS sizes and buffer roles.  The plan is driven at the shipped shape and at small ones (128 x 2, 64 x 3, 64 x 2),
where 129 elements already take the multi-tile path and 64 * 2 * 128 + 1 the second aggregate level.  Every expectation is computed in
Python integers with pow(x, -1, r) (0 for 0); results are compared limb for limb on the raw 256-bit integers, so a non-canonical output
does not compare equal.

Every launch runs its block on one host thread per lane.  The library is built with trapping bounds / shift checks, every buffer
(column sets, scratch records, flags) has exactly the size the plan reserves and ends against an inaccessible page, `out` and `flags`
are pre-filled with a pattern no result has, and everything runs in a child process under a time limit (tests/simt_fr_frac_child.py).

That the tests bite was checked by seeding faults into fr_frac.hip.h one at a time (each was confirmed to fail, then removed):
  * the gamma term dropped on the denominator side (`t[e] = fr_sub(t[e], gamma)` in front of the grand product's zero check): every
    grand-product case differs (seven of the eight tests fail; test_the_plan runs no kernel);
  * the zero replacement forgotten in the tile inversion (`t[e] = fr_one()` removed from the fraction sum): test_zero_denominators
    differs -- the tile's total is zero, so every element of the tile comes out wrong -- and so does the gamma = 0 case of
    test_null_sets_alias_pitch_and_special_challenges, where the zeros among the special values of den_a and den_b meet;
  * the lane prefix record off by one lane (`lane_rec + 12` handed to frs_tile_body): the children of all multi-tile tests end outside
    a guarded buffer (the last lane's record lies behind the plan's LANE buffer);
  * the tile guard removed (`cnt = tile`): likewise, the first partial tile reads behind its column set;
  * the table pitch ignored (`off = j * total * 8`): test_null_sets_alias_pitch_and_special_challenges differs in its pitch cases (the
    kernel reads the poison between the tables); every packed case still passes.

Run time on an 8-core machine: about a minute, 10 s of it the build of the library."""

import numpy as np
import pytest

import fr_frac_ref as ref
import simt_fr_frac_child as child
import simt_harness
from oracle import bls12_381_ref as o

RR = ref.RR
GP, FS = child.GRAND_PRODUCT, child.FRAC_SUM
SHAPES = [(128, 2), (64, 3)]
SPECIAL = (0, 1, RR - 1)


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    return simt_harness.emu_lib(child.build)


def _set(c, k, n, rng, special=True):
    """c tables of k rows of n scalars; 0, 1 and r - 1 at both ends of a row and in its middle"""
    t = [[[rng.scalar() for _ in range(n)] for _ in range(k)] for _ in range(c)]
    if special and n >= 3:
        for j in range(c):
            for v in range(k):
                t[j][v][0] = SPECIAL[(j + v) % 3]
                t[j][v][-1] = SPECIAL[(j + v + 1) % 3]
                t[j][v][n // 2] = SPECIAL[(j + v + 2) % 3]
    return t


class Case:
    """one call: the sets as integers, the job for the child, the expectation"""

    def __init__(self, op, c, k, n, seed, shape, exclusive=False, beta=None, gamma=None, xb=True, db=True, mult=True, alias=False, pitch=None, flags=True, edit=None):
        rng = o.SplitMix64(seed)
        self.op, self.c, self.k, self.n, self.exclusive, self.shape, self.flags = op, c, k, n, exclusive, shape, flags
        self.beta = rng.scalar() if beta is None else beta
        self.gamma = rng.scalar() if gamma is None else gamma
        self.xa = _set(c, k, n, rng) if (op == GP or mult) else None
        self.xb = _set(c, k, n, rng) if (op == GP and xb) else None
        self.da = self.xa if alias else _set(c, k, n, rng)
        self.db = _set(c, k, n, rng) if db else None
        self.alias, self.pitch = alias, pitch
        if edit:
            edit(self)
        self.what = "op=%d c=%d k=%d len=%d ex=%s shape=%s seed=%d" % (op, c, k, n, exclusive, shape, seed)

    def zero_den(self, j, v, i):
        """make denominator factor j of element (v, i) zero by choosing den_a"""
        self.da[j][v][i] = -((self.beta * self.db[j][v][i] if self.db is not None else 0) + self.gamma) % RR

    def job(self):
        pk = lambda s: None if s is None else ref.pack_set(s, self.pitch, poison=0x1234567 if self.pitch else None)
        j = {"op": "frac", "frac_op": self.op, "c": self.c, "len": self.n, "k": self.k, "chal": ref.mont_words([self.beta, self.gamma]),
             "xa": pk(self.xa), "xb": pk(self.xb), "da": None if self.alias else pk(self.da), "db": pk(self.db), "alias": self.alias,
             "exclusive": self.exclusive, "shape": self.shape, "flags": self.flags, "label": self.what}
        if self.pitch:
            j["pitch"] = self.pitch
        return j

    def expect(self):
        if self.op == GP:
            return ref.grand_product(self.xa, self.xb, self.da, self.db, self.beta, self.gamma, self.exclusive)
        return ref.frac_sum(self.xa, self.da, self.db, self.beta, self.gamma, self.exclusive)

    def check(self, res):
        want, wflags = self.expect()
        got = ref.raw_ints(res["out"])
        flat = ref.mont([x for row in want for x in row])
        assert len(got) == len(flat), self.what
        bad = [i for i in range(len(got)) if got[i] != flat[i]]
        assert not bad, "%s: %d of %d elements differ, first at %d" % (self.what, len(bad), len(got), bad[0])
        if self.flags:
            assert list(res["flags"]) == [x for row in wflags for x in row], "flags: " + self.what
        else:
            assert res["flags"] is None
        return want, wflags


def _run(cases):
    res = child.run([c.job() for c in cases])
    return [c.check(r) for c, r in zip(cases, res)]


def _boundary_lengths(block, chunk):
    e, w, t = chunk, 64 * chunk, block * chunk
    return sorted({n for n in (1, 2, e - 1, e, e + 1, w - 1, w, w + 1, t - 1, t, t + 1, 2 * t + 3) if n >= 1})


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_lengths_at_every_boundary(shape):
    """one row of every length at which the schedule changes hands: lane chunk, wavefront, tile, three tiles; both operations, both forms,
    c rotating through 1, 2, 3 (every c meets every kind of boundary over the two shapes), and c = 8 once"""
    cases = []
    for idx, n in enumerate(_boundary_lengths(*shape)):
        for op in (GP, FS):
            for ex in (False, True):
                cases.append(Case(op, 1 + (idx + op + ex) % 3, 1, n, 1000 + n, shape, exclusive=ex))
    t = shape[0] * shape[1]
    cases += [Case(GP, 8, 1, t + 1, 8, shape), Case(FS, 8, 1, t + 1, 9, shape, exclusive=True)]
    _run(cases)


def test_shipped_shapes():
    """the plan's own shapes (256 lanes; four elements per lane, two for the fraction sum above four columns) at c = 3 and, for the
    narrower tile, c = 5: rows that straddle tiles, the barriers of every table hand-over, the inversion's scans across four wavefronts"""
    cases = [Case(GP, 3, 7, 1000, 4242, None), Case(FS, 3, 7, 1000, 4243, None, exclusive=True), Case(FS, 5, 3, 700, 4244, None)]
    res = child.run([c.job() for c in cases])
    for c, r in zip(cases, res):
        assert r["kernels"] == [child.K_FRONT, child.K_AGG_SCAN, child.K_SCAN]
        c.check(r)


def test_rows():
    """k rows whose length does not divide the tile: rows shorter than a lane's chunk, heads in mid-chunk, mid-wavefront and mid-tile, rows
    longer than a tile; 0, 1 and r - 1 at both row ends and in the middle of every table"""
    shape = (128, 2)
    cases = []
    for k in (1, 3, 17):
        for n in (1, 3, 5, 63, 100, 256, 384):
            if k == 17 and n > 100:
                continue
            for op in (GP, FS):
                cases.append(Case(op, 1 + (k + n) % 3, k, n, 77 * k + n, shape, exclusive=(k + n + op) % 2 == 1))
    _run(cases)


def test_zero_denominators():
    """a zero denominator in ONE column at the first, a middle and the last element of a row: exact flags, the product row zero from there on
    and the next row untouched, the sum short of that one term and nothing else -- with the row boundary in mid-chunk and at a tile
    boundary (128 x 2: rows of 256), with and without the beta term"""
    shape = (128, 2)
    cases = []
    for k, n in ((3, 5), (3, 100), (3, 256)):
        for pos in (0, n // 2, n - 1):
            for op in (GP, FS):
                for db in (True, False):
                    def edit(cs, pos=pos):
                        cs.zero_den(1, 1, pos)
                    cases.append((Case(op, 3, k, n, 31 * n + pos, shape, exclusive=(pos == 0), db=db, edit=edit), pos))
    res = child.run([c.job() for c, _ in cases])
    for (c, pos), r in zip(cases, res):
        want, wflags = c.check(r)
        assert [x for row in wflags for x in row].count(0) == 1 and wflags[1][pos] == 0
        if c.op == GP:
            first = pos + 1 if c.exclusive else pos
            assert all(x == 0 for x in want[1][first:]) and all(x != 0 for x in want[1][:first]) and all(x != 0 for x in want[2]), c.what
        else:
            # element `pos` adds the other two columns' terms and nothing else
            beta, gamma = c.beta, c.gamma
            terms = [c.xa[j][1][pos] * ref.inv0(c.da[j][1][pos] + (beta * c.db[j][1][pos] if c.db is not None else 0) + gamma) for j in (0, 2)]
            incl = ref.frac_sum(c.xa, c.da, c.db, beta, gamma, False)[0][1]
            before = incl[pos - 1] if pos else 0
            assert (incl[pos] - before) % RR == sum(terms) % RR, c.what
    # two zeros in one element (two columns), a zero next to a tile boundary on either side, every denominator of a tile zero
    def many(cs):
        cs.zero_den(0, 0, 255); cs.zero_den(2, 0, 255); cs.zero_den(1, 0, 256); cs.zero_den(0, 0, 0)
    def whole_tile(cs):
        for i in range(256, 512):
            cs.zero_den(i % 2, 0, i)
    _run([Case(op, 3, 1, 700, 5 + op, shape, edit=e) for op in (GP, FS) for e in (many, whole_tile)])


def test_null_sets_alias_pitch_and_special_challenges():
    """a zero numerator factor (ordinary data), beta = 0, gamma = 0, num_b / den_b NULL (each and both), mult NULL, num_a == den_a as ONE
    buffer, and pitch > k * len with poison between the tables that must not reach any result; flags NULL too"""
    shape = (128, 2)
    k, n = 3, 100
    def zero_num(cs):                                              # the grand product's factor n_1 / the sum's multiplicity m_1 of element (1, 7)
        cs.xa[1][1][7] = -(cs.beta * cs.xb[1][1][7] + cs.gamma) % RR if cs.op == GP else 0
    cases = []
    for op in (GP, FS):
        cases += [Case(op, 3, k, n, 1, shape, edit=zero_num),
                  Case(op, 2, k, n, 2, shape, beta=0), Case(op, 2, k, n, 3, shape, gamma=0), Case(op, 2, k, n, 4, shape, beta=0, gamma=0, exclusive=True),
                  Case(op, 3, k, n, 5, shape, db=False), Case(op, 3, k, n, 6, shape, flags=False),
                  Case(op, 3, k, n, 7, shape, pitch=k * n + 13), Case(op, 2, 1, 300, 8, shape, pitch=1000, exclusive=True)]
    cases += [Case(GP, 3, k, n, 9, shape, xb=False), Case(GP, 3, k, n, 10, shape, xb=False, db=False), Case(GP, 1, k, n, 11, shape, xb=False, db=False, gamma=0),
              Case(FS, 3, k, n, 12, shape, mult=False), Case(FS, 1, k, n, 13, shape, mult=False, db=False),
              Case(GP, 3, k, n, 14, shape, alias=True), Case(GP, 2, 1, 300, 15, shape, alias=True, pitch=512), Case(FS, 2, k, n, 16, shape, alias=True)]
    wants = _run(cases)
    # aliased with num_b == NULL and den_b == NULL: every f is 1
    al = Case(GP, 2, k, n, 17, shape, alias=True, xb=False, db=False)
    (want, _), = _run([al])
    assert all(x == 1 for row in want for x in row)
    assert len(wants) == len(cases)


def test_many_tiles_and_the_second_aggregate_level():
    """enough tiles to reach the aggregate scan with more than a wavefront of records, and a total above tile^2 at the smallest shape, so
    that both aggregate levels run over fused output; rows that do not divide anything"""
    shape = (64, 2)
    t = 128
    seqs = {1: [child.K_FRONT], 3: [child.K_FRONT, child.K_AGG_SCAN, child.K_SCAN],
            5: [child.K_FRONT, child.K_AGG_REDUCE, child.K_AGG_SCAN, child.K_AGG_SCAN, child.K_SCAN]}
    cases = [(Case(GP, 1, 1, t, 1, shape), 1), (Case(FS, 2, 2, t // 2, 2, shape), 1), (Case(GP, 2, 1, 100 * t + 5, 3, shape), 3), (Case(FS, 1, 97, 100, 4, shape, exclusive=True), 3),
             (Case(GP, 1, 1, t * t + 1, 5, shape, xb=False, db=False), 5), (Case(FS, 1, 165, 100, 6, shape, mult=False, db=False), 5)]
    res = child.run([c.job() for c, _ in cases])
    for (c, steps), r in zip(cases, res):
        assert r["kernels"] == seqs[steps], c.what
        c.check(r)


def test_the_plan():
    """the expected step lists at one-tile, multi-tile and two-level totals, nothing for k == 0 or len == 0, the refusals, and at the shipped
    shapes: LDS of every (op, c) at most 80 KiB, fewer elements per lane for the wide fraction sums"""
    FS1, FR, AR, AS, SC = child.K_FRONT_SINGLE, child.K_FRONT_REDUCE, child.K_AGG_REDUCE, child.K_AGG_SCAN, child.K_SCAN
    shape = (64, 2)
    t = 128
    want = [((1, 1), [FS1], [1]), ((1, t), [FS1], [1]), ((2, t // 2), [FS1], [1]), ((1, t + 1), [FR, AS, SC], [2, 1, 2]), ((3, t), [FR, AS, SC], [3, 1, 3]),
            ((1, t * t), [FR, AS, SC], [t, 1, t]), ((1, t * t + 1), [FR, AR, AS, AS, SC], [t + 1, 2, 1, 2, t + 1]), ((165, 100), [FR, AR, AS, AS, SC], [129, 2, 1, 2, 129]),
            ((0, 5), [], []), ((5, 0), [], [])]
    jobs = [{"op": "plan", "frac_op": op, "c": 3, "len": n, "k": k, "shape": shape, "label": "plan"} for (k, n), _, _ in want for op in (GP, FS)]
    res = child.run(jobs)
    for i, ((k, n), kinds, grids) in enumerate(want):
        for r in res[2 * i:2 * i + 2]:
            assert r["steps"] == len(kinds) and r["kinds"] == kinds and r["grids"] == grids, (k, n, r)
            tiles = -(-k * n // t)
            assert r["recs"][0] == r["recs"][2] == (tiles if tiles > 1 else 0) and r["recs"][4] == (tiles * 64 if tiles > 1 else 0)
            assert r["reach"] == (2 * k * n + k * n if k * n else 0)
    # the shipped shapes
    jobs = [{"op": "plan", "frac_op": op, "c": c, "len": 1 << 16, "k": 3, "label": "shipped"} for op in (GP, FS) for c in range(1, 9)]
    res = child.run(jobs)
    for j, r in zip(jobs, res):
        assert r["steps"] == 3 and r["block"] == 256 and 0 < r["lds"] <= 80 * 1024, (j, r)
        assert r["chunk"] == (2 if j["frac_op"] == FS and j["c"] > 4 else 4)
        assert r["grids"][0] == -(-(3 << 16) // (256 * r["chunk"]))
    one = child.run([{"op": "plan", "frac_op": op, "c": 3, "len": 1024, "k": 1, "label": "one tile"} for op in (GP, FS)])
    assert [r["kinds"] for r in one] == [[FS1], [FS1]]
    # refusals: c out of range, an unknown operation, k * len and the tables' reach above 2^28, a 64-bit overflow, a pitch below k * len
    bad = [dict(frac_op=GP, c=0, len=5, k=5), dict(frac_op=GP, c=9, len=5, k=5), dict(frac_op=2, c=1, len=5, k=5), dict(frac_op=FS, c=1, len=(1 << 28) + 1, k=1),
           dict(frac_op=FS, c=2, len=1 << 27, k=1, pitch=(1 << 27) + 1), dict(frac_op=GP, c=1, len=1 << 33, k=1 << 33), dict(frac_op=GP, c=1, len=(1 << 63) + 1, k=2),
           dict(frac_op=GP, c=2, len=10, k=10, pitch=99), dict(frac_op=GP, c=1, len=5, k=5, shape=(64, 5)), dict(frac_op=GP, c=1, len=5, k=5, shape=(96, 2))]
    res = child.run([dict(b, op="plan", label="refusal %d" % i) for i, b in enumerate(bad)])
    assert [r["steps"] for r in res] == [-1] * len(bad)
    ok = child.run([dict(op="plan", label="limit", frac_op=FS, c=2, len=1 << 27, k=1), dict(op="plan", label="limit", frac_op=GP, c=8, len=1 << 25, k=1)])
    assert [r["steps"] for r in ok] == [5, 5]
