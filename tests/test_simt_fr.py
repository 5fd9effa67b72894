"""The batched / coset Fr transform (blsgpu_fr_ntt_many), its device code compiled for the HOST (tests/simt/emu_fr.cpp), against the oracle.

What runs here is the code the GPU runs: `k_fr_twiddles`, `k_fr_tw_levels`, `k_fr_ninv`, `k_fr_coset_table`, `k_fr_stage1`, `k_fr_stage2`,
`k_fr_cols` (each with and without the coset load) and `k_fr_tile<true>`, launched step by step from the plan of csrc/fr_plan.h -- the
function api_fr.hip launches from -- with its grids, blocks and arguments; `k_fr_tile<false>`, the single transform's twin, once.
Every expectation comes from oracle/bls12_381_ref.py (`fr_ntt`, `FR_GENERATOR`, Montgomery conversion): the coset expectation is
`fr_ntt([x_j g^j])` and, for the inverse, `fr_ntt(y, inverse=True)[j] g^-j`, in Python integers.  Results are compared limb for limb.

The library is built with trapping bounds / shift checks, every buffer has exactly the size the host reserves for it and ends against an
inaccessible page (the data buffer too: a tile that reads past the last vector faults), and it runs in a child process under a time
limit (tests/simt_fr_child.py).  The breadth of the cases runs the LDS kernels with one lane per workgroup (they stride by blockDim.x:
any block size computes the same); `test_real_block_sizes` runs each of them with the plan's block on one host thread per lane, which
is what exercises the barriers.

That the tests bite was checked by seeding faults into fr.hip.h / fr_plan.h one at a time (each was confirmed to fail, then removed):
  * bit reversal over the whole array instead of per vector (`r = brev(p) >> (64 - log_n)` in k_fr_tile<true>): test_plain_transform
    fails at the first k > 1 (elements differ);
  * coset index `p` instead of `p & (n-1)`, in frl_load_shifted (the global passes) and, separately, in the load of k_fr_tile<true>:
    the child of test_the_plan_takes_the_kernels_it_should (the first test with a coset and k = 2) ends reading past the coset table;
  * the tile guard removed (`base + e >= total` on the load): the child of test_plain_transform ends reading past the data buffer;
  * the inverse table without n^-1 (k_fr_coset_table): the inverse coset cases of test_the_plan_takes_the_kernels_it_should differ
    (test_coset_inverse and test_coset_round_trip cover the same).

Run time on an 8-core machine: 29 s, about 10 s of them the build of the library (tests/test_simt_msm.py: about 200 s)."""

import numpy as np
import pytest

import simt_fr_child as child
import simt_harness
from oracle import bls12_381_ref as o

RR = o.R_ORDER
RINV = pow(o.FR_MONT_R, -1, RR)
G7 = o.FR_GENERATOR
SMALL = [0, 1, 2, 3, 6, 9, 10]                                     # whole vectors per tile, one launch, in place
LARGE = [11, 12, 13]                                               # global passes, then the tile kernel
K_SMALL = [1, 2, 3, 5, 17]
K_LARGE = [1, 2, 3]


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    return simt_harness.emu_lib(child.build)


def _words(vals):
    """integers mod r -> (len, 8) u32 Montgomery words"""
    b = b"".join((int(v) % RR * o.FR_MONT_R % RR).to_bytes(32, "little") for v in vals)
    return np.frombuffer(b, dtype=np.uint32).reshape(-1, 8)


def _ints(words):
    """(…, 8) u32 words -> the raw 256-bit integers (NOT reduced: a non-canonical output must not compare equal)"""
    w = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, 8)
    return [int.from_bytes(row.tobytes(), "little") for row in w]


def _mont(vals):
    return [int(v) % RR * o.FR_MONT_R % RR for v in vals]


def _vectors(k, n, seed, special=False):
    r = o.SplitMix64(seed)
    vs = [[r.scalar() for _ in range(n)] for _ in range(k)]
    if special:                                                    # 0, 1 and r - 1 among the elements, at both ends of a vector
        for v in vs:
            for pos, val in zip((0, n // 2, n - 1), (0, 1, RR - 1)):
                v[pos] = val
    return vs


def _job(vs, **kw):
    k, n = len(vs), len(vs[0])
    j = {"op": "many", "data": np.stack([_words(v) for v in vs]).reshape(k, n, 8), "label": "log_n=%d k=%d %s" % (n.bit_length() - 1, k, kw)}
    if kw.get("coset") is not None:
        kw["coset"] = _words([kw["coset"]])[0]
    j.update(kw)
    return j


def _expect(vs, inverse=False, g=None):
    out = []
    for v in vs:
        n = len(v)
        if g is None:
            out.append(o.fr_ntt(v, inverse=inverse))
        elif not inverse:
            out.append(o.fr_ntt([x * pow(g, j, RR) % RR for j, x in enumerate(v)]))
        else:
            gi = pow(g, -1, RR)
            out.append([y * pow(gi, j, RR) % RR for j, y in enumerate(o.fr_ntt(v, inverse=True))])
    return out


def _assert_equal(res, want, what):
    got = _ints(res["out"])
    flat = _mont([x for v in want for x in v])
    assert len(got) == len(flat)
    bad = [i for i in range(len(got)) if got[i] != flat[i]]
    assert not bad, "%s: %d of %d elements differ, first at %d" % (what, len(bad), len(got), bad[0])


def _shapes():
    return [(ln, k) for ln in SMALL for k in K_SMALL] + [(ln, k) for ln in LARGE for k in K_LARGE]


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
def test_plain_transform(inverse):
    """coset == NULL at every (log_n, k): k different vectors containing 0, 1 and r - 1; (6, 17), (3, 5), (9, 3) ... end inside a tile"""
    cases = [(_vectors(k, 1 << ln, 100 * ln + k, special=ln >= 2), ln, k) for ln, k in _shapes()]
    res = child.run([_job(vs, inverse=inverse) for vs, _, _ in cases])
    for (vs, ln, k), r in zip(cases, res):
        _assert_equal(r, _expect(vs, inverse), "log_n=%d k=%d" % (ln, k))


def test_the_plan_takes_the_kernels_it_should():
    """13 = stage2 + stage1 + tile, 12 = stage2 + tile, 11 = stage1 + tile, <= 10 the tile kernel alone, 0 nothing at all; the column-tile
    plan forced at small sizes (as BLSGPU_NTT_COLS allows): one pass of two stages at 2^12, passes of two and one stage at 2^13"""
    S2, S1, T, C = child.K_STAGE2, child.K_STAGE1, child.K_TILE, child.K_COLS
    want = {13: [S2, S1, T], 12: [S2, T], 11: [S1, T], 10: [T], 3: [T], 1: [T], 0: []}
    jobs = [_job(_vectors(2, 1 << ln, 7 + ln), coset=G7) for ln in want]
    cols = [(12, (8, 2, 64), [C, T]), (13, (8, 2, 64), [C, C, T]), (12, (7, 1, 64), [C, C, T])]
    data = {ln: _vectors(2, 1 << ln, 900 + ln, special=True) for ln in (12, 13)}
    variants = [dict(), dict(inverse=True), dict(coset=G7), dict(coset=G7, inverse=True)]
    cjobs = [(ln, shape, seq, kw) for ln, shape, seq in cols for kw in variants]
    res = child.run(jobs + [_job(data[ln], cols=shape, **kw) for ln, shape, seq, kw in cjobs])
    for ln, r in zip(want, res):
        assert r["kernels"] == want[ln], ln
        _assert_equal(r, _expect(_vectors(2, 1 << ln, 7 + ln), False, G7), "log_n=%d" % ln)
    for (ln, shape, seq, kw), r in zip(cjobs, res[len(jobs):]):
        assert r["kernels"] == seq, (ln, shape)
        _assert_equal(r, _expect(data[ln], kw.get("inverse", False), kw.get("coset")), "cols log_n=%d %s %s" % (ln, shape, kw))


def _cosets():
    return [("one", 1), ("seven", G7), ("r-1", RR - 1), ("random", o.SplitMix64(4242).scalar() or 5)]


@pytest.mark.parametrize("name,g", _cosets(), ids=[c[0] for c in _cosets()])
def test_coset_forward(name, g):
    """y[m] = sum_j x[j] g^j w^(jm): the oracle's transform of the shifted coefficients; g = 1 must equal the plain transform"""
    shapes = [(1, 3), (2, 5), (3, 17), (6, 17), (9, 3), (10, 2), (11, 2), (12, 3), (13, 2)] if name in ("seven", "random") else [(3, 5), (6, 17), (10, 2), (11, 2), (13, 2)]
    cases = [(_vectors(k, 1 << ln, 31 * ln + k, special=ln >= 2), ln, k) for ln, k in shapes]
    res = child.run([_job(vs, coset=g) for vs, _, _ in cases] + ([_job(vs) for vs, _, _ in cases] if g == 1 else []))
    for i, (vs, ln, k) in enumerate(cases):
        _assert_equal(res[i], _expect(vs, False, g), "g=%s log_n=%d k=%d" % (name, ln, k))
        if g == 1:
            assert np.array_equal(res[i]["out"], res[len(cases) + i]["out"])


@pytest.mark.parametrize("name,g", _cosets(), ids=[c[0] for c in _cosets()])
def test_coset_inverse(name, g):
    """x[j] = g^-j n^-1 sum_m y[m] w^(-jm): the table entry 2^5 n^-1 g^-j takes the place of the n^-1 scale"""
    shapes = [(1, 3), (2, 5), (3, 17), (6, 17), (9, 3), (10, 2), (11, 2), (12, 3), (13, 2)] if name in ("seven", "random") else [(3, 5), (6, 17), (10, 2), (11, 2), (13, 2)]
    cases = [(_vectors(k, 1 << ln, 57 * ln + k, special=ln >= 2), ln, k) for ln, k in shapes]
    res = child.run([_job(vs, coset=g, inverse=True) for vs, _, _ in cases])
    for (vs, ln, k), r in zip(cases, res):
        _assert_equal(r, _expect(vs, True, g), "g=%s log_n=%d k=%d" % (name, ln, k))


def test_coset_round_trip():
    """inverse(g) after forward(g) is the identity, limb for limb, through both launch shapes"""
    cases = [(_vectors(k, 1 << ln, 11 * ln + k, special=ln >= 2), g) for ln, k in [(0, 3), (1, 7), (3, 129), (6, 17), (10, 3), (12, 2)] for g in (None, G7, RR - 1)]
    fwd = child.run([_job(vs, coset=g) for vs, g in cases])
    back = child.run([{"op": "many", "data": f["out"], "inverse": True, "coset": None if g is None else _words([g])[0], "label": "back"} for f, (vs, g) in zip(fwd, cases)])
    for (vs, g), b in zip(cases, back):
        _assert_equal(b, vs, "round trip g=%s log_n=%d" % (g, len(vs[0]).bit_length() - 1))


def test_vectors_are_independent():
    """changing vector v changes output v and no other (tile ownership, per-vector bit reversal and coset index)"""
    for ln, k, v in [(3, 17, 9), (6, 17, 16), (10, 3, 1), (12, 3, 2)]:
        a = _vectors(k, 1 << ln, 5 * ln + k)
        b = [list(x) for x in a]
        b[v] = _vectors(1, 1 << ln, 999)[0]
        ra, rb = child.run([_job(a, coset=G7), _job(b, coset=G7)])
        for i in range(k):
            assert np.array_equal(ra["out"][i], rb["out"][i]) == (i != v), (ln, k, i)
        _assert_equal(rb, _expect(b, False, G7), "changed vector")


def test_real_block_sizes():
    """the LDS kernels with the plan's block size, one host thread per lane: the barriers between load, stages and store (k_fr_tile<true>
    on whole vectors and behind global passes, k_fr_cols with and without the coset load, k_fr_tile<false>)"""
    cases = [((6, 17), dict(coset=G7)), ((6, 17), dict(coset=G7, inverse=True)), ((3, 129), dict()), ((10, 2), dict(inverse=True)),
             ((11, 2), dict(coset=G7)), ((12, 2), dict(coset=G7, cols=(8, 2, 64))), ((12, 1), dict(inverse=True, cols=(9, 2, 512)))]
    data = [_vectors(k, 1 << ln, 77 * ln + k, special=True) for (ln, k), _ in cases]
    single = [(_vectors(1, 1 << ln, 3 + ln)[0], inv) for ln in (4, 7, 10) for inv in (False, True)]
    res = child.run([_job(vs, threads=1, **kw) for vs, (_, kw) in zip(data, cases)] +
                    [{"op": "single", "data": _words(v), "inverse": inv, "threads": 1, "label": "single n=%d" % len(v)} for v, inv in single])
    for vs, (shape, kw), r in zip(data, cases, res):
        _assert_equal(r, _expect(vs, kw.get("inverse", False), kw.get("coset")), "threads %s %s" % (shape, kw))
    for (v, inv), r in zip(single, res[len(cases):]):
        _assert_equal(r, [o.fr_ntt(v, inverse=inv)], "k_fr_tile<false> n=%d" % len(v))
