"""The evaluation-form openings (blsgpu_fr_bary_eval_many / blsgpu_fr_bary_open_many), their device code compiled for the HOST
(tests/simt/emu_fr_bary.cpp), against Python integers mod r.

What runs here is the code the GPU runs: `k_frb_tile<eval | open>` in its two modes, `k_frb_row<...>` and `k_frb_quot`, launched step by
step from the plan of csrc/fr_bary_plan.h -- the function api_fr.hip launches from -- with its grids, blocks, LDS sizes and buffer roles,
on a twiddle table built by the transform's own kernels.  The plan is driven at the shipped shape (256 lanes x 8 elements) and at small
ones (64 x 2, 128 x 2), where rows of 256 / 512 elements already lie over several tiles.  Every expectation is computed by the definition
in Python integers (tests/fr_bary_ref.py: interpolate, Horner, synthetic division, transform back -- not the barycentric formula);
results are compared limb for limb, so a non-canonical output does not compare equal.  Every job also checks that `evals` and `points`
were not written.

The kernels add across lanes with shuffles, so EVERY launch runs its block on one host thread per lane.  The library is built with
trapping bounds / shift checks, every buffer (the twiddle table and the records included) has exactly the size the entry point reserves
and ends against an inaccessible page, and it runs in a child process under a time limit (tests/simt_fr_bary_child.py).

That the tests bite was checked by seeding faults into fr_bary.hip.h one at a time (each was confirmed to fail, then removed):
  * the hit ignored (`hitmask` never set in k_frb_tile, so a zero d is inverted as it stands): test_point_in_the_domain and every test
    with z = 1 or z = r - 1 differ;
  * the -w^j half taken as +w^j (`return t` in frb_dom32): test_every_size differs from log_n = 1 on;
  * the tile guard dropped (`cnt = tile` in k_frb_tile): the child of test_partial_last_tile ends outside a guarded buffer;
  * the bit reversal applied to the wrong width (`64 - log_n - 1` in frb_exp): every BITREV case of test_every_size differs;
  * the hit element's slot not skipped by the quotient pass (`hit` compared without the + 1 in k_frb_quot): test_point_in_the_domain
    differs in the row-over-tiles shape."""

import numpy as np
import pytest

import simt_fr_bary_child as child
import simt_harness
import fr_bary_ref as ref
from oracle import bls12_381_ref as o

RR = ref.RR
NAT, REV = ref.NATURAL, ref.BITREV
SMALL = [(64, 2), (128, 2)]


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    return simt_harness.emu_lib(child.build)


def _rand_rows(k, n, seed):
    r = o.SplitMix64(seed)
    return [[r.scalar() for _ in range(n)] for _ in range(k)]


def _job(rows, pts, order=NAT, is_open=True, shape=None, **kw):
    k, n = len(rows), len(rows[0])
    j = {"evals": np.stack([ref.words(v) for v in rows]).reshape(k, n, 8), "points": ref.words(pts), "order": order, "open": is_open, "shape": shape,
         "label": "k=%d n=%d order=%d open=%s shape=%s %s" % (k, n, order, is_open, shape, kw.get("note", ""))}
    return j


def _run_and_check(cases):
    """cases: (rows, points, order, open, shape[, note]) -> the results, each compared with the definition"""
    jobs = [_job(c[0], c[1], c[2], c[3], c[4], note=c[5] if len(c) > 5 else "") for c in cases]
    res = child.run(jobs)
    for c, j, r in zip(cases, jobs, res):
        rows, pts, order, is_open = c[0], c[1], c[2], c[3]
        want = [ref.expect(row, z, order) for row, z in zip(rows, pts)]
        got_y = ref.raw_ints(r["y"])
        bad = [v for v in range(len(rows)) if got_y[v] != ref.mont([want[v][0]])[0]]
        assert not bad, "%s: y differs in rows %s" % (j["label"], bad[:8])
        if is_open:
            n = len(rows[0])
            got_q = ref.raw_ints(r["q"])
            flat = ref.mont([x for w in want for x in w[1]])
            bad = [(i // n, i % n) for i in range(len(flat)) if got_q[i] != flat[i]]
            assert not bad, "%s: q differs at %d places, first (row, i) = %s" % (j["label"], len(bad), bad[:6])
        else:
            assert r["q"] is None
        assert np.array_equal(r["evals_after"], j["evals"]), "%s: evals were written" % j["label"]
        assert np.array_equal(r["points_after"], j["points"]), "%s: points were written" % j["label"]
    return res


def _log2(x):
    return x.bit_length() - 1


@pytest.mark.parametrize("shape", SMALL, ids=["%dx%d" % s for s in SMALL])
def test_every_size(shape):
    """log_n from 0 to log2(tile) + 2: rows inside a lane, over lanes of one wavefront, over wavefronts, exactly one per tile, two and four
    tiles per row; both orders, eval and open; a random point, a point of the domain and z with z^n = -1 in every call"""
    t = shape[0] * shape[1]
    cases = []
    for log_n in range(0, _log2(t) + 3):
        n = 1 << log_n
        for order in (NAT, REV):
            rows = _rand_rows(3, n, 100 * log_n + order)
            r = o.SplitMix64(7 * log_n + order)
            pts = [r.scalar(), ref.domain_point(log_n, order, (3 * n) // 4), pow(o.fr_omega(log_n + 1), 2 * (n // 3) + 1, RR)]
            cases.append((rows, pts, order, True, shape))
            cases.append((rows[:2], pts[:2], order, False, shape))
    _run_and_check(cases)


def test_partial_last_tile():
    """k in {1, 2, 3, 17} rows that do not fill the last tile; points 0, 1 (= D[0]) and r - 1 (= D[n / 2] in natural order) among them"""
    shape = (64, 2)
    cases = []
    for k in (1, 2, 3, 17):
        for n in (1, 2, 4, 8, 32):
            for order in (NAT, REV):
                rows = _rand_rows(k, n, 31 * k + n)
                r = o.SplitMix64(k + n)
                fixed = [0, 1, RR - 1]
                pts = [fixed[v % 5] if v % 5 < 3 else r.scalar() for v in range(k)] if k > 1 else [r.scalar()]
                assert (k * n) % 128 or k * n < 128
                cases.append((rows, pts, order, True, shape))
                if order == NAT:
                    cases.append((rows, pts, order, False, shape))
    _run_and_check(cases)


@pytest.mark.parametrize("shape", SMALL, ids=["%dx%d" % s for s in SMALL])
def test_point_in_the_domain(shape):
    """z = D[j] with j at both ends of the row, at the last index of a lane's chunk and the first of the next, at the last index of a tile
    and the first of the next: several hit rows in one call at different j, un-hit rows between them, a hit row and an un-hit row inside
    one workgroup (rows of half a tile and less), in both shapes and both orders"""
    block, chunk = shape
    t = block * chunk
    cases = []
    for n in (2, chunk, 4 * chunk, t // 2, t, 2 * t, 4 * t):
        log_n = _log2(n)
        js = sorted({j for j in (0, n - 1, chunk - 1, chunk, 64 * chunk - 1, 64 * chunk, t - 1, t, 2 * t - 1, 2 * t, 3 * t) if 0 <= j < n})
        for order in (NAT, REV):
            r = o.SplitMix64(n + order)
            pts = []
            for j in js:
                pts += [ref.domain_point(log_n, order, j), r.scalar()]
            pts = [r.scalar()] + pts                               # an un-hit row first: hit rows at odd positions
            rows = _rand_rows(len(pts), n, 5 * n + order)
            cases.append((rows, pts, order, True, shape, "hits at %s" % js))
            if order == REV:
                cases.append((rows, pts, order, False, shape, "hits at %s" % js))
    _run_and_check(cases)


def test_special_points_and_rows():
    """z in {0, 1, r - 1} and an odd power of the 2n-th root (z^n = -1, not in the domain); rows that are all zero, constant (q is all
    zero) or hold 0 and r - 1 at both ends -- rows in a tile and rows over tiles"""
    shape = (64, 2)
    cases = []
    for n in (1, 2, 16, 128, 256):
        log_n = _log2(n)
        r = o.SplitMix64(n)
        zs = [0, 1, RR - 1, pow(o.fr_omega(log_n + 1), 1, RR), pow(o.fr_omega(log_n + 1), 2 * n - 1, RR), r.scalar()]
        const = r.scalar()
        ends = _rand_rows(1, n, n + 1)[0]
        ends[0], ends[-1] = 0, RR - 1
        ends2 = list(reversed(ends))
        for order in (NAT, REV):
            rows, pts = [], []
            for z in zs:
                for row in ([0] * n, [const] * n, ends, ends2, _rand_rows(1, n, z % 1000)[0]):
                    rows.append(row)
                    pts.append(z)
            res = _run_and_check([(rows, pts, order, True, shape)])[0]
            q = res["q"]
            for v in range(len(rows)):
                if v % 5 in (0, 1):
                    assert not q[v].any(), "the quotient of a constant row is zero"
    # log_n = 0: y = f[0] and q[0] = 0 for every z
    r = _run_and_check([([[5], [0], [RR - 1]], [0, 1, 12345], NAT, True, shape)])[0]
    assert not r["q"].any() and ref.raw_ints(r["y"]) == ref.mont([5, 0, RR - 1])


def test_rows_are_independent():
    """changing row v changes the outputs of row v and no other"""
    shape = (64, 2)
    jobs, meta = [], []
    for k, n, v in ((17, 4, 9), (5, 32, 1), (3, 128, 0), (3, 256, 2)):
        log_n = _log2(n)
        a = _rand_rows(k, n, 3 * k + n)
        b = [list(x) for x in a]
        b[v] = _rand_rows(1, n, 999)[0]
        r = o.SplitMix64(n)
        pts = [r.scalar() for _ in range(k)]
        pts[v] = ref.domain_point(log_n, NAT, n - 1)               # the changed row is a hit row: its neighbours must not notice
        jobs += [_job(a, pts, NAT, True, shape), _job(b, pts, NAT, True, shape)]
        meta.append((k, n, v))
    res = child.run(jobs)
    for i, (k, n, v) in enumerate(meta):
        ra, rb = res[2 * i], res[2 * i + 1]
        for row in range(k):
            assert np.array_equal(ra["y"][row], rb["y"][row]) == (row != v), (k, n, row)
            assert np.array_equal(ra["q"][row], rb["q"][row]) == (row != v), (k, n, row)


def test_the_plan_takes_the_launches_it_should():
    """one launch while a row fits a tile; tile pass and row pass above it, and the quotient pass for open; nothing for k == 0 -- from the
    plan's own kernel ids"""
    R, T, W, Q = child.K_ROWS, child.K_TILE, child.K_ROW, child.K_QUOT
    shape = (64, 2)
    want = [((1, 1), [R], [R]), ((3, 1), [R], [R]), ((1, 128), [R], [R]), ((5, 64), [R], [R]), ((1, 256), [T, W], [T, W, Q]), ((3, 512), [T, W], [T, W, Q])]
    cases = []
    for (k, n), ev, op in want:
        rows = _rand_rows(k, n, k + n)
        pts = [o.SplitMix64(n + v).scalar() for v in range(k)]
        cases += [(rows, pts, NAT, False, shape), (rows, pts, NAT, True, shape)]
    res = _run_and_check(cases)
    for i, ((k, n), ev, op) in enumerate(want):
        assert res[2 * i]["kernels"] == ev and res[2 * i + 1]["kernels"] == op, (k, n)
    empty = [{"evals": np.zeros((0, 16, 8), dtype=np.uint32), "points": np.zeros((0, 8), dtype=np.uint32), "open": op, "shape": shape, "label": "k=0"} for op in (False, True)]
    empty += [{"evals": np.zeros((0, 512, 8), dtype=np.uint32), "points": np.zeros((0, 8), dtype=np.uint32), "open": True, "shape": shape, "label": "k=0, rows over tiles"}]
    for r in child.run(empty):
        assert r["kernels"] == []
    # the shipped shape: a row of 2048 is one launch, a row of 4096 three
    res = _run_and_check([(_rand_rows(1, 2048, 1), [5], NAT, True, None), (_rand_rows(1, 4096, 2), [5], NAT, True, None)])
    assert [r["kernels"] for r in res] == [[R], [T, W, Q]]


def test_shipped_shape():
    """the plan's real block (256 lanes, four wavefronts, chunks of eight): rows inside a lane and over lanes with a partial last tile,
    a row over four wavefronts, rows over two tiles; hits at chunk, wavefront and tile boundaries; bit-reversed order"""
    cases = []
    for n, k, js in ((4, 700, (0, 3)), (64, 33, (7, 8, 63)), (1024, 7, (511, 512, 1023)), (4096, 2, (2047, 2048))):
        log_n = _log2(n)
        r = o.SplitMix64(n)
        pts = [r.scalar() for _ in range(k)]
        for idx, j in enumerate(js):
            pts[(2 * idx + 1) % k] = ref.domain_point(log_n, REV, j)
        cases.append((_rand_rows(k, n, n + k), pts, REV, True, None, "hits at %s" % (js,)))
    cases.append((_rand_rows(2, 4096, 77), [3, ref.domain_point(12, NAT, 4095)], NAT, False, None))
    _run_and_check(cases)
