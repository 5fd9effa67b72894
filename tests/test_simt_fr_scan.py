"""The Fr scans and the batch inversion (blsgpu_fr_scan_many / blsgpu_fr_batch_invert), their device code compiled for the HOST
(tests/simt/emu_fr_scan.cpp), against Python integers mod r.

What runs here is the code the GPU runs: `k_frs_tile<SUM | PRODUCT | HORNER>` in its three modes, `k_frs_agg<...>` in its two and
`k_frs_invert`, launched step by step from the plan of csrc/fr_scan_plan.h -- the function api_fr.hip launches from -- with its grids,
blocks, LDS sizes and buffer roles.  The plan is driven at the shipped shape (256 lanes x 8 elements) and at small ones (128 x 2,
64 x 3, 64 x 2), where 129 elements already take the multi-tile path and 64 * 2 * 128 + 1 the second aggregate level.  Every
expectation is computed here in Python integers (the defining recurrences); results are compared limb for limb, so a non-canonical
output does not compare equal.

The kernels scan across lanes with shuffles, so EVERY launch runs its block on one host thread per lane (there is no one-lane shortcut
as in test_simt_fr.py); `test_shipped_block_size` is the one with the plan's real 256 lanes.  The library is built with trapping bounds /
shift checks, every buffer (scratch records included) has exactly the size the plan reserves and ends against an inaccessible page,
and it runs in a child process under a time limit (tests/simt_fr_scan_child.py).

That the tests bite was checked by seeding faults into fr_scan.hip.h one at a time (each was confirmed to fail, then removed):
  * the head flag dropped in the combine (`o.f = 0` instead of `o.f = l.f` in frs_combine): test_rows fails (a row longer than a lane's
    reach picks up the previous row);
  * the cross-wavefront step taking one record too many (`i <= w` instead of `i < w` in frs_block_scan): test_lengths_at_every_boundary
    differs;
  * the carry-in applied across a row head (`frs_apply` instead of `frs_carry` in k_frs_tile's SCAN mode): test_rows fails;
  * the tile guard removed (`cnt = tile` in k_frs_tile): the child of test_lengths_at_every_boundary ends outside a guarded buffer.

Run time on an 8-core machine: about 55 s, 10 s of them the build of the library."""

import numpy as np
import pytest

import simt_fr_scan_child as child
import simt_harness
from oracle import bls12_381_ref as o

RR = o.R_ORDER
MONT = o.FR_MONT_R
SUM, PRODUCT, HORNER = 0, 1, 2
SHAPES = [(128, 2), (64, 3), child.SHIPPED]


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    return simt_harness.emu_lib(child.build)


def _words(vals):
    """integers mod r -> (len, 8) u32 Montgomery words"""
    b = b"".join((int(v) % RR * MONT % RR).to_bytes(32, "little") for v in vals)
    return np.frombuffer(b, dtype=np.uint32).reshape(-1, 8)


def _ints(words):
    """(…, 8) u32 words -> the raw 256-bit integers (NOT reduced: a non-canonical output must not compare equal)"""
    w = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, 8)
    return [int.from_bytes(row.tobytes(), "little") for row in w]


def _mont(vals):
    return [int(v) % RR * MONT % RR for v in vals]


def _rows(k, n, seed, special=True):
    r = o.SplitMix64(seed)
    vs = [[r.scalar() for _ in range(n)] for _ in range(k)]
    if special and n >= 3:                                         # 0, 1 and r - 1 among the elements, at both ends of a row
        for i, v in enumerate(vs):
            vals = (0, 1, RR - 1)
            v[0] = vals[i % 3]
            v[-1] = vals[(i + 1) % 3]
            v[n // 2] = vals[(i + 2) % 3]
    return vs


def _expect(op, rows, points=None, exclusive=False):
    out = []
    for v, row in enumerate(rows):
        n = len(row)
        res = [0] * n
        if op == HORNER:
            z = points[v]
            acc = 0
            for i in range(n - 1, -1, -1):
                acc = (row[i] + z * acc) % RR
                res[i] = acc
        else:
            acc = 0 if op == SUM else 1
            for i in range(n):
                nxt = (acc + row[i]) % RR if op == SUM else acc * row[i] % RR
                res[i] = acc if exclusive else nxt
                acc = nxt
        out.append(res)
    return out


def _job(op, rows, points=None, **kw):
    k, n = len(rows), len(rows[0])
    j = {"op": "scan", "scan_op": op, "data": np.stack([_words(v) for v in rows]).reshape(k, n, 8),
         "label": "op=%d k=%d len=%d %s" % (op, k, n, kw)}
    if points is not None:
        j["points"] = _words(points)
    j.update(kw)
    return j


def _assert_equal(res, want, what):
    got = _ints(res["out"])
    flat = _mont([x for v in want for x in v])
    assert len(got) == len(flat)
    bad = [i for i in range(len(got)) if got[i] != flat[i]]
    assert not bad, "%s: %d of %d elements differ, first at %d" % (what, len(bad), len(got), bad[0])


def _points(k, seed):
    r = o.SplitMix64(seed)
    fixed = [0, 1, RR - 1]
    return [fixed[v] if v < 3 and k > 1 else r.scalar() for v in range(k)]


def _boundary_lengths(block, chunk):
    e, w, t = chunk, 64 * chunk, block * chunk
    return sorted({n for n in (1, 2, e - 1, e, e + 1, w - 1, w, w + 1, t - 1, t, t + 1, 2 * t + 3) if n >= 1})


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_lengths_at_every_boundary(shape):
    """one row of every length at which the schedule changes hands: lane chunk, wavefront, tile, three tiles; every op, both forms"""
    cases = []
    for n in _boundary_lengths(*shape):
        rows = _rows(1, n, 1000 + n)
        for z in ([5] if shape == child.SHIPPED else [0, 1, RR - 1, o.SplitMix64(n).scalar()]):
            cases.append((HORNER, rows, [z], False))
        for op in (SUM, PRODUCT):
            nz = [[x or 3 for x in rows[0]]] if op == PRODUCT else rows      # a product of non-zero elements: every position is checked
            cases.append((op, nz, None, False))
            cases.append((op, nz, None, True))
    res = child.run([_job(op, rows, pts, exclusive=ex, shape=shape) for op, rows, pts, ex in cases])
    for (op, rows, pts, ex), r in zip(cases, res):
        _assert_equal(r, _expect(op, rows, pts, ex), "shape=%s op=%d len=%d exclusive=%s z=%s" % (shape, op, len(rows[0]), ex, pts))


@pytest.mark.parametrize("shape", SHAPES[:2], ids=["%dx%d" % s for s in SHAPES[:2]])
def test_rows(shape):
    """k rows whose length does not divide the tile: heads in mid-chunk, mid-wavefront and mid-tile, rows that straddle two and three
    tiles, rows that start exactly at a tile boundary; a different point per row, 0, 1 and r - 1 among them; in place too"""
    t = shape[0] * shape[1]
    cases = []
    for k in (1, 2, 3, 17):
        for n in (3, 5, 63, 65, 100, t, t + t // 2):
            if k == 17 and n > 100:
                continue
            rows = _rows(k, n, 77 * k + n)
            pts = _points(k, k + n)
            for op, ex in ((SUM, False), (SUM, True), (PRODUCT, False), (PRODUCT, True), (HORNER, False)):
                cases.append((op, rows, pts if op == HORNER else None, ex, (k * n) % 2 == 1))
    res = child.run([_job(op, rows, pts, exclusive=ex, shape=shape, inplace=inp) for op, rows, pts, ex, inp in cases])
    for (op, rows, pts, ex, inp), r in zip(cases, res):
        _assert_equal(r, _expect(op, rows, pts, ex), "shape=%s op=%d k=%d len=%d exclusive=%s inplace=%s" % (shape, op, len(rows), len(rows[0]), ex, inp))
        if not inp:
            assert np.array_equal(r["in_after"], np.stack([_words(v) for v in rows])), "the input was written to"


def test_product_zero_ends_with_its_row():
    """a zero as the LAST element of row v: the rest of row v is zero from there, row v + 1 is untouched -- with the row boundary in
    mid-chunk, at a tile boundary (128 x 2: rows of 256) and a zero in the first position"""
    shape = (128, 2)
    cases = []
    for k, n in ((3, 5), (3, 256), (4, 100), (2, 384)):
        rows = [[x or 1 for x in row] for row in _rows(k, n, 5 * n + k, special=False)]
        rows[0][-1] = 0
        rows[k - 1][0] = 0
        cases.append(rows)
    res = child.run([_job(PRODUCT, rows, exclusive=ex, shape=shape) for rows in cases for ex in (False, True)])
    i = 0
    for rows in cases:
        for ex in (False, True):
            want = _expect(PRODUCT, rows, None, ex)
            assert all(x != 0 for x in want[1][1:]) or len(rows) == 2
            _assert_equal(res[i], want, "k=%d len=%d exclusive=%s" % (len(rows), len(rows[0]), ex))
            i += 1


def test_the_plan_takes_the_launches_it_should():
    """one launch for a single tile, reduce / aggregate scan / scan above it, the second aggregate level beyond tile^2 elements, nothing
    for k == 0 or len == 0 -- from the plan's own kernel ids -- and the results of the deepest branch against Python integers"""
    S, R, AR, AS, SC = child.K_SINGLE, child.K_REDUCE, child.K_AGG_REDUCE, child.K_AGG_SCAN, child.K_SCAN
    shape = (64, 2)
    t = 128
    want = [((1, 1), [S]), ((1, t), [S]), ((2, t // 2), [S]), ((1, t + 1), [R, AS, SC]), ((3, t), [R, AS, SC]), ((1, t * t), [R, AS, SC]),
            ((1, t * t + 1), [R, AR, AS, AS, SC]), ((165, 100), [R, AR, AS, AS, SC])]
    cases = []
    for (k, n), seq in want:
        for op in ((SUM, PRODUCT, HORNER) if k > 100 else (SUM,)):
            rows = _rows(k, n, k + n)
            if op == PRODUCT:
                rows = [[x or 2 for x in row] for row in rows]
            cases.append((op, rows, _points(k, 3 * k) if op == HORNER else None, seq))
    empty = [{"op": "scan", "scan_op": SUM, "data": np.zeros((0, 5, 8), dtype=np.uint32), "shape": shape, "label": "k=0"},
             {"op": "scan", "scan_op": SUM, "data": np.zeros((3, 0, 8), dtype=np.uint32), "shape": shape, "label": "len=0"}]
    res = child.run([_job(op, rows, pts, shape=shape) for op, rows, pts, _ in cases] + empty)
    for (op, rows, pts, seq), r in zip(cases, res):
        assert r["kernels"] == seq, (op, len(rows), len(rows[0]))
        _assert_equal(r, _expect(op, rows, pts), "op=%d k=%d len=%d" % (op, len(rows), len(rows[0])))
    for r in res[len(cases):]:
        assert r["kernels"] == []
    # the shipped shape: 2048 elements are one launch, 2049 three
    res = child.run([_job(SUM, _rows(1, n, n)) for n in (2048, 2049)])
    assert [r["kernels"] for r in res] == [[S], [R, AS, SC]]


def test_vectors_are_independent():
    """changing row v changes output row v and no other"""
    shape = (128, 2)
    jobs, meta = [], []
    for k, n, v in ((17, 5, 9), (3, 100, 1), (3, 300, 0), (4, 256, 2)):
        a = [[x or 1 for x in row] for row in _rows(k, n, 3 * k + n, special=False)]
        b = [list(x) for x in a]
        b[v] = [x or 1 for x in _rows(1, n, 999, special=False)[0]]
        pts = _points(k, n)
        for op in (SUM, PRODUCT, HORNER):
            jobs += [_job(op, a, pts if op == HORNER else None, shape=shape), _job(op, b, pts if op == HORNER else None, shape=shape)]
            meta.append((op, k, n, v, b, pts))
    res = child.run(jobs)
    for i, (op, k, n, v, b, pts) in enumerate(meta):
        ra, rb = res[2 * i], res[2 * i + 1]
        for row in range(k):
            assert np.array_equal(ra["out"][row], rb["out"][row]) == (row != v), (op, k, n, row)
        _assert_equal(rb, _expect(op, b, pts), "changed row")


def _inv_expect(vals):
    return [pow(x, -1, RR) if x else 0 for x in vals]


def _inv_job(vals, **kw):
    j = {"op": "invert", "data": _words(vals), "label": "n=%d %s" % (len(vals), kw)}
    j.update(kw)
    return j


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_batch_inversion(shape):
    """equality with pow(x, -1, r): zeros at element 0, at the last element and on either side of a tile boundary, a tile of nothing but
    zeros between non-zero tiles, an all-zero vector, n = 1, flags NULL and non-NULL, in place; 1 and r - 1 among the values"""
    t = shape[0] * shape[1]
    r = o.SplitMix64(31 + t)
    cases = []
    for n in (1, 2, shape[1] + 1, 64 * shape[1] + 1, t - 1, t, t + 1, 3 * t + 5):
        v = [r.scalar() or 1 for _ in range(n)]
        v[n // 2] = RR - 1
        v[n // 3] = 1
        cases.append(v)
        z = list(v)
        for pos in (0, n - 1, t - 1, t, 2 * t - 1):
            if pos < n:
                z[pos] = 0
        cases.append(z)
    block = [r.scalar() or 1 for _ in range(3 * t)]
    block[t:2 * t] = [0] * t
    cases += [block, [0] * (t + 3), [0], [1], [RR - 1]]
    jobs = [_inv_job(v, flags=(i % 2 == 0), inplace=(i % 3 == 0), shape=shape) for i, v in enumerate(cases)]
    res = child.run(jobs)
    for i, (v, rr) in enumerate(zip(cases, res)):
        assert rr["kernels"] == [child.K_INVERT]
        got = _ints(rr["out"])
        want = _mont(_inv_expect(v))
        bad = [p for p in range(len(v)) if got[p] != want[p]]
        assert not bad, "shape=%s case %d n=%d: %d inverses differ, first at %d" % (shape, i, len(v), len(bad), bad[0])
        if i % 2 == 0:
            assert list(rr["flags"]) == [1 if x else 0 for x in v], "flags of case %d" % i
        else:
            assert rr["flags"] is None
    assert child.run([{"op": "invert", "data": np.zeros((0, 8), dtype=np.uint32), "label": "n=0"}])[0]["kernels"] == []


def test_shipped_block_size():
    """the plan's real block (256 lanes, four wavefronts, chunks of eight) on one host thread per lane: the barriers, the wavefront scans
    and the cross-wavefront step of every kernel, rows that straddle tiles, and the inversion's forward and backward scans"""
    shape = child.SHIPPED
    rows = _rows(7, 1000, 4242)
    nz = [[x or 7 for x in row] for row in rows]
    pts = _points(7, 11)
    cases = [(SUM, rows, None, True), (PRODUCT, nz, None, False), (HORNER, rows, pts, False)]
    res = child.run([_job(op, rw, p, exclusive=ex, shape=shape, inplace=True) for op, rw, p, ex in cases])
    for (op, rw, p, ex), r in zip(cases, res):
        assert r["kernels"] == [child.K_REDUCE, child.K_AGG_SCAN, child.K_SCAN]
        _assert_equal(r, _expect(op, rw, p, ex), "shipped shape op=%d" % op)
