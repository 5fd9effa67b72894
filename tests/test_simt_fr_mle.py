"""The multilinear operations over Fr (blsgpu_fr_mle_fold / blsgpu_fr_eq_table / blsgpu_fr_mle_eval / blsgpu_fr_sumcheck_round_device), their
device code compiled for the HOST (tests/simt/emu_fr_mle.cpp), against Python integers mod r.

What runs here is the code the GPU runs: `k_frm_fold`, `k_frm_eq`, `k_frm_round<plain | fused>` and `k_frm_round_finish`, launched step by
step from the plans of csrc/fr_mle_plan.h -- the functions api_fr.hip launches from -- with their grids, blocks, LDS sizes, buffer roles
and pitches, and the term program through the same validation (frm_prog_build), which folds the 2^5 bookkeeping into the coefficients.
The plans are driven at the shipped shape (256 lanes x 4 positions) and at small ones (64 x 1, 64 x 3: a ragged last tile), where a few
hundred elements already take several workgroups and the finish kernel.  Every expectation is computed here in Python integers from the
definitions (fold, eq, the round polynomial); results are compared limb for limb, so a non-canonical output does not compare equal.

The kernels add across lanes with shuffles, so EVERY launch runs its block on one host thread per lane.  The library is built with
trapping bounds / shift checks, every buffer (tables with their pitch, records, scratch) has exactly the size the plan reserves, ends
against an inaccessible page and holds a sentinel pattern wherever nothing may be written, and it runs in a child process under a time
limit (tests/simt_fr_mle_child.py).

That the tests bite was checked by seeding faults one at a time (each was confirmed to fail test_round, then removed):
  * the 2^5 correction dropped from one term length (`5 * n` -> `5 * (n - (n == 2))` in frm_prog_build): the evaluations differ wherever
    a term has two factors;
  * `i + h` read as `i + h - 1` (`row + npos * 8 - 8` in the plain branch of k_frm_round): the evaluations differ;
  * the fused fold writing its upper result at `i + 2q` instead of `i + q`: the check of the folded tables fails (the lower half differs
    from the Python fold and the upper half is no longer untouched);
  * the last tile's guard removed (`if (i >= npos) break` in k_frm_round): the child ends outside a guarded buffer, already at m = 1,
    where one lane has a pair and the others would read past it;
  * the finish kernel reading one record too few (`i + 1 < n_rec`): the evaluations differ wherever there is more than one tile.

Run time on an 8-core machine: about 30 s, 10 s of it the build of the library."""

import numpy as np
import pytest

import simt_fr_mle_child as child
import simt_harness
from oracle import bls12_381_ref as o

RR = o.R_ORDER
MONT = o.FR_MONT_R
SHAPES = [(64, 1), (64, 3), child.SHIPPED]
IDS = ["%dx%d" % s for s in SHAPES]
SENT = child.SENTINEL


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    return simt_harness.emu_lib(child.build)


# ---- Python integers: the definitions ------------------------------------------------------------------------------------------------
def _fold(f, r):
    h = len(f) // 2
    return [(f[i] + r * (f[i + h] - f[i])) % RR for i in range(h)]


def _eq(p):
    t = [1]
    for pb in p:                                                   # bit b of the index selects p_b
        t = [x * (1 - pb) % RR for x in t] + [x * pb % RR for x in t]
    return t


def _eval_folds(f, p):
    for b in range(len(p) - 1, -1, -1):
        f = _fold(f, p[b])
    return f[0]


def _round(tabs, terms):
    """evals[t], t = 0 .. D, of sum_t' coef prod_e ((1 - t) f_e[i] + t f_e[i + h]) over i < h"""
    h = len(tabs[0]) // 2
    deg = max(len(ix) for _, ix in terms)
    out = []
    for t in range(deg + 1):
        at = [[((1 - t) * f[i] + t * f[i + h]) % RR for i in range(h)] for f in tabs]
        s = 0
        for c, ix in terms:
            for i in range(h):
                p = c
                for e in ix:
                    p = p * at[e][i] % RR
                s += p
        out.append(s % RR)
    return out


def _interpolate(evals, x):
    """the polynomial of degree len(evals) - 1 through (t, evals[t]) at x"""
    n, s = len(evals), 0
    for t in range(n):
        num = den = 1
        for u in range(n):
            if u != t:
                num = num * (x - u) % RR
                den = den * (t - u) % RR
        s += evals[t] * num * pow(den, -1, RR)
    return s % RR


# ---- words ---------------------------------------------------------------------------------------------------------------------------
def _mont(v):
    return int(v) % RR * MONT % RR


def _words(vals):
    """integers mod r -> (len, 8) u32 Montgomery words"""
    b = b"".join(_mont(v).to_bytes(32, "little") for v in vals)
    return np.frombuffer(b, dtype=np.uint32).reshape(-1, 8).copy()


def _raw(words):
    """(…, 8) u32 words -> the raw 256-bit integers (NOT reduced: a non-canonical output must not compare equal)"""
    w = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, 8)
    return [int.from_bytes(row.tobytes(), "little") for row in w]


SENT_SCALAR = int.from_bytes(np.full(8, SENT, dtype=np.uint32).tobytes(), "little")


def _tables(k, m, seed):
    """k tables of 2^m random scalars with 0, 1 and r - 1 at both ends and on either side of the h boundary"""
    r = o.SplitMix64(seed)
    n, h = 1 << m, 1 << m >> 1
    tabs = [[r.scalar() for _ in range(n)] for _ in range(k)]
    vals = (0, 1, RR - 1)
    for j, f in enumerate(tabs):
        for q, pos in enumerate((0, n - 1, h - 1 if h else 0, h)):
            if n >= 4 or q < 2:
                f[pos % n] = vals[(j + q) % 3]
    return tabs


def _stack(tabs):
    return np.stack([_words(f) for f in tabs])


def _terms_job(terms):
    ptr, tab = [0], []
    for _, ix in terms:
        tab += ix
        ptr.append(len(tab))
    coef = np.array([[(_mont(c) >> (64 * w)) & (2 ** 64 - 1) for w in range(4)] for c, _ in terms], dtype=np.uint64)
    return {"term_ptr": ptr, "term_tab": tab, "coef": coef}


def _check_rows(buf, pitch, rows, what):
    """the whole buffer: row j at j * pitch holds rows[j] (integers -> Montgomery), every other scalar the sentinel"""
    got = _raw(buf)
    assert len(got) == (len(rows) - 1) * pitch + len(rows[0])
    want = [SENT_SCALAR] * len(got)
    for j, row in enumerate(rows):
        want[j * pitch:j * pitch + len(row)] = [_mont(v) for v in row]
    bad = [i for i in range(len(got)) if got[i] != want[i]]
    assert not bad, "%s: %d of %d scalars differ, first at %d" % (what, len(bad), len(got), bad[0])


def _top_m(shape):
    return (shape[0] * shape[1]).bit_length() - 1 + 3


# term programs: (k, terms); coefficients 0, 1 and r - 1 among them
def _programs(seed):
    r = o.SplitMix64(seed)
    c = r.scalar()
    return {
        "spartan": (4, [(1, [0, 1, 2]), (RR - 1, [0, 3])]),
        "one": (1, [(c, [0])]),
        "deg6": (2, [(1, [0, 1, 0, 1, 1, 0])]),
        "square": (4, [(5, [2, 2]), (0, [0, 1]), (RR - 1, [1])]),                     # a repeated index, a zero coefficient, table 3 unused
        "eight": (8, [(1, [0]), (RR - 1, [1, 2]), (c, [3, 4, 5]), (0, [6, 7, 0, 1]), (2, [2, 2, 2, 2, 2]), (r.scalar(), [7, 6, 5, 4, 3, 2]), (RR - 2, [1]),
                      (3, [5, 5])]),
    }


CHALLENGES = [0, 1, RR - 1]


# ---- fold ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_fold(shape):
    """every m from one pair to eight tiles, k = 1, 2, 4, 8, out of place and in place, packed and with a pitch; challenges 0, 1 and r - 1
    return the lower half, the upper half and 2 lo - hi; the input of the out-of-place form and every word between the rows survive"""
    cases = []
    rnd = o.SplitMix64(5)
    for m in range(1, _top_m(shape) + 1):
        k = (1, 2, 4, 8)[m % 4] if m < 12 else 2
        n = 1 << m
        tabs = _tables(k, m, 100 + m)
        for q, r in enumerate(CHALLENGES + [rnd.scalar()] if m <= 4 else [CHALLENGES[m % 3], rnd.scalar()]):
            inplace = (m + q) % 2 == 0
            pin = n + (3 if q % 2 else 0)
            pout = pin if inplace else n // 2 + (5 if q % 2 == 0 else 0)
            cases.append((tabs, r, inplace, pin, pout))
    jobs = [{"op": "fold", "tables": _stack(t), "r": _words([r])[0], "inplace": ip, "pitch_in": pin, "pitch_out": pout, "shape": shape,
             "label": "m=%d k=%d r=%d inplace=%s" % (len(t[0]).bit_length() - 1, len(t), CHALLENGES.index(r) if r in CHALLENGES else -1, ip)} for t, r, ip, pin, pout in cases]
    res = child.run(jobs)
    for (tabs, r, ip, pin, pout), got in zip(cases, res):
        assert got["kernels"] == [child.K_FOLD]
        h = len(tabs[0]) // 2
        want = [_fold(f, r) for f in tabs]
        if r == 0:
            assert want == [f[:h] for f in tabs]
        if r == 1:
            assert want == [f[h:] for f in tabs]
        if r == RR - 1:
            assert want == [[(2 * f[i] - f[i + h]) % RR for i in range(h)] for f in tabs]
        what = "shape=%s m=%d k=%d inplace=%s" % (shape, h.bit_length(), len(tabs), ip)
        if ip:
            _check_rows(got["out"], pin, [w + f[h:] for w, f in zip(want, tabs)], what)
        else:
            _check_rows(got["out"], pout, want, what)
            _check_rows(got["in_after"], pin, tabs, what + " (the input)")
    assert child.run([{"op": "fold", "tables": np.zeros((0, 8, 8), dtype=np.uint32), "r": _words([3])[0], "shape": shape, "label": "k=0"}])[0]["kernels"] == []


# ---- eq ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_eq_table(shape):
    """m = 0 (the Scalar one) through four tiles; random points, points with 0 and 1 among the coordinates, and points of nothing but 0
    and 1, where the table is the indicator of one index"""
    rnd = o.SplitMix64(17)
    cases = []
    for m in range(0, _top_m(shape)):
        cases.append([rnd.scalar() for _ in range(m)])
        if m:
            mixed = [rnd.scalar() for _ in range(m)]
            mixed[0] = 1
            mixed[m - 1] = 0 if m > 1 else 1
            mixed[m // 2] = (0, 1, RR - 1)[m % 3]
            cases.append(mixed)
            cases.append([(0x5a5a5a5a5 >> b) & 1 for b in range(m)])
    res = child.run([{"op": "eq", "point": _words(p).reshape(-1, 8), "shape": shape, "label": "m=%d" % len(p)} for p in cases])
    for p, got in zip(cases, res):
        assert got["kernels"] == [child.K_EQ]
        want = _eq(p)
        if p and all(x in (0, 1) for x in p):
            idx = sum(x << b for b, x in enumerate(p))
            assert want == [1 if i == idx else 0 for i in range(1 << len(p))]
        assert _raw(got["out"]) == [_mont(v) for v in want], "shape=%s m=%d" % (shape, len(p))


# ---- eval ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES[:2], ids=IDS[:2])
def test_mle_eval(shape):
    """f_j(point) by both definitions -- the folds from the top variable down, and the inner product with eq(point) -- for m = 0 (a copy)
    upward, packed and with a pitch; the tables are not written"""
    rnd = o.SplitMix64(23)
    cases = []
    for m in range(0, _top_m(shape) - 1):
        k = (1, 2, 4, 8)[m % 4]
        tabs = _tables(k, m, 300 + m)
        p = [rnd.scalar() for _ in range(m)]
        if m >= 3:
            p[1] = (0, 1, RR - 1)[m % 3]
        cases.append((tabs, p, (1 << m) + (m % 2) * 7))
    jobs = [{"op": "eval", "tables": _stack(t), "point": _words(p).reshape(-1, 8), "pitch": pitch, "shape": shape, "label": "m=%d k=%d" % (len(p), len(t))} for t, p, pitch in cases]
    res = child.run(jobs)
    for (tabs, p, pitch), got in zip(cases, res):
        m = len(p)
        assert got["kernels"] == ([child.K_COPY] if m == 0 else [child.K_FOLD] * m)
        e = _eq(p)
        want = [sum(a * b for a, b in zip(f, e)) % RR for f in tabs]
        assert want == [_eval_folds(f, p) for f in tabs]
        assert _raw(got["out"]) == [_mont(v) for v in want], "shape=%s m=%d" % (shape, m)
        _check_rows(got["in_after"], pitch, tabs, "m=%d (the tables)" % m)


# ---- rounds --------------------------------------------------------------------------------------------------------------------------
def _round_cases(shape):
    progs = _programs(41)
    names = list(progs)
    rnd = o.SplitMix64(43)
    cases = []
    for m in range(1, _top_m(shape) + 1):
        pick = names if m <= 3 else [names[m % len(names)], names[(m + 2) % len(names)]]
        if m >= 12:
            pick = ["spartan"]
        for q, name in enumerate(pick):
            k, terms = progs[name]
            tabs = _tables(k, m, 500 + 7 * m + q)
            pitch = (1 << m) + (6 if (m + q) % 2 else 0)
            cases.append((name, tabs, terms, None, pitch))
            if m >= 2:
                r = CHALLENGES[(m + q) % 3] if q % 2 == 0 else rnd.scalar()
                cases.append((name, tabs, terms, r, pitch))
    return cases


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_round(shape):
    """the plain and the fused round for every m from a single pair (one lane works, the rest idle) to eight tiles: k = 1, 2, 4, 8, terms of
    one and of six factors, a repeated index, a table no term uses, one and eight terms, coefficients 0, 1 and r - 1, challenges 0, 1 and
    r - 1, a pitch with a sentinel pattern between the rows.  The plain round writes nothing but its evaluations; the fused round leaves
    the Python fold in the lower half of every row and the upper half untouched."""
    cases = _round_cases(shape)
    jobs = []
    for name, tabs, terms, r, pitch in cases:
        j = {"op": "round", "tables": _stack(tabs), "pitch": pitch, "shape": shape, "label": "%s m=%d fused=%s" % (name, len(tabs[0]).bit_length() - 1, r is not None)}
        j.update(_terms_job(terms))
        if r is not None:
            j["r_prev"] = _words([r])[0]
        jobs.append(j)
    res = child.run(jobs, timeout=600)
    tile = shape[0] * shape[1]
    for (name, tabs, terms, r, pitch), got in zip(cases, res):
        m = len(tabs[0]).bit_length() - 1
        what = "shape=%s %s m=%d fused=%s" % (shape, name, m, r is not None)
        npos = 1 << (m - (2 if r is not None else 1))
        first = child.K_ROUND if r is None else child.K_ROUND_FUSED
        assert got["kernels"] == ([first] if npos <= tile else [first, child.K_FINISH]), what
        assert got["degree"] == max(len(ix) for _, ix in terms)
        h = len(tabs[0]) // 2
        if r is None:
            now = tabs
            _check_rows(got["after"], pitch, tabs, what + " (the tables)")
        else:
            now = [_fold(f, r) for f in tabs]
            _check_rows(got["after"], pitch, [w + f[h:] for w, f in zip(now, tabs)], what + " (the folded tables)")
        assert _raw(got["evals"]) == [_mont(v) for v in _round(now, terms)], what


def test_the_plans_take_the_launches_they_should():
    """one launch for a single tile, the round and its finish above it (plain: h positions, fused: h / 2) at a small shape and at the
    shipped shape's own boundary, and nothing at all for k == 0 (an evaluation's m folds and its copy for m = 0 are in test_mle_eval)"""
    k, terms = _programs(1)["spartan"]
    R, RF, F = child.K_ROUND, child.K_ROUND_FUSED, child.K_FINISH
    jobs, want = [], []
    for shape, m, r, seq in (((64, 1), 7, None, [R]), ((64, 1), 8, None, [R, F]), ((64, 1), 8, 7, [RF]), ((64, 1), 9, 7, [RF, F]),
                             (child.SHIPPED, 11, None, [R]), (child.SHIPPED, 12, None, [R, F]), (child.SHIPPED, 12, 9, [RF])):
        tabs = _tables(k, m, 900 + m)
        j = {"op": "round", "tables": _stack(tabs), "shape": shape, "label": "plan m=%d" % m}
        j.update(_terms_job(terms))
        if r is not None:
            j["r_prev"] = _words([r])[0]
        jobs.append(j)
        want.append((seq, _round(tabs if r is None else [_fold(f, r) for f in tabs], terms)))
    empty = [{"op": "fold", "tables": np.zeros((0, 8, 8), dtype=np.uint32), "r": _words([3])[0], "label": "fold k=0"},
             {"op": "eval", "tables": np.zeros((0, 8, 8), dtype=np.uint32), "point": _words([1, 2, 3]), "label": "eval k=0"}]
    res = child.run(jobs + empty)
    for (seq, ev), got in zip(want, res):
        assert got["kernels"] == seq
        assert _raw(got["evals"]) == [_mont(v) for v in ev]
    for got in res[len(jobs):]:
        assert got["kernels"] == []                                # k == 0: nothing is launched


def test_full_sumcheck():
    """m = 9, k = 4, the Spartan shape (D = 3) on 64 x 3: round 1 plain, rounds 2 .. 9 fused, the last challenge by a fold.  Every round's
    evaluations against Python, and the verifier's own checks: evals[0] + evals[1] equals the running claim, the next claim is the
    interpolation at the challenge, the final claim equals sum_t coef_t prod values, and the values are f_j at p_b = r_(m-b)."""
    shape = (64, 3)
    m = 9
    k, terms = _programs(3)["spartan"]
    tabs = _tables(k, m, 77)
    rnd = o.SplitMix64(78)
    chal = [rnd.scalar() for _ in range(m)]
    chal[3], chal[5] = 0, 1
    prog = _terms_job(terms)
    cur = _stack(tabs)                     # the device tables, as the previous round left them (pitch 2^m kept)
    py = tabs
    claim = None
    for s in range(1, m + 1):
        j = {"op": "round", "tables": cur[:, :1 << (m - s + 1 + (1 if s > 1 else 0))], "pitch": 1 << m, "shape": shape, "label": "sumcheck round %d" % s}
        j.update(prog)
        if s > 1:
            j["r_prev"] = _words([chal[s - 2]])[0]
            py = [_fold(f, chal[s - 2]) for f in py]
        got = child.run([j])[0]
        want = _round(py, terms)
        assert _raw(got["evals"]) == [_mont(v) for v in want], "round %d" % s
        assert claim is None or (want[0] + want[1]) % RR == claim, "round %d: evals[0] + evals[1] is not the running claim" % s
        claim = _interpolate(want, chal[s - 1])
        after = got["after"]               # rows `2^m` apart, the last one cut at its length
        rows = 1 << (m - s + 1 + (1 if s > 1 else 0))
        cur = np.stack([after[jj * (1 << m):jj * (1 << m) + rows] for jj in range(k)])
    last = child.run([{"op": "fold", "tables": cur[:, :2], "r": _words([chal[m - 1]])[0], "inplace": True, "pitch_in": 1 << m, "shape": shape, "label": "last fold"}])[0]
    values = [_raw(last["out"][jj * (1 << m)])[0] for jj in range(k)]
    point = [chal[m - 1 - b] for b in range(m)]
    want_values = [_eval_folds(f, point) for f in tabs]
    assert values == [_mont(v) for v in want_values]
    assert sum(c * _prod(want_values[e] for e in ix) for c, ix in terms) % RR == claim
    e = _eq(point)
    assert want_values == [sum(a * b for a, b in zip(f, e)) % RR for f in tabs]


def _prod(it):
    p = 1
    for v in it:
        p = p * v % RR
    return p
