"""The group transforms (blsgpu_g1_ntt_many / blsgpu_g2_ntt_many), their device code compiled for the HOST (tests/simt/emu_gntt.cpp), against
the oracle.

What runs here is the code the GPU runs: `k_gntt_permute` and `k_gntt_stage` in its four shapes (G1 / G2, a butterfly per lane or lane
pair / per team of eight lanes) with the shared ladders `mb_ladder_glv` / `mb_ladder_gls` of csrc/mulbatch.hip.h, launched step by step
from the plan of csrc/gntt_plan.h -- the function api_msm.hip launches from -- with its grids, blocks and stage indices, over twiddle
tables built by the Fr transform's own kernels.  Every expectation comes from oracle/bls12_381_ref.py (`g1_mul`, `g1_sum`, `fr_omega`,
`fr_ntt` and the G2 twins) in Python integers (tests/g_ntt_points.py); results are compared as affine points, coordinate for coordinate.

The library is built with trapping bounds / shift checks, every buffer has exactly the size the host reserves for it and ends against an
inaccessible page, and it runs in a child process under a time limit (tests/simt_gntt_child.py).  The lane shape of G1 runs its lanes
one after the other; the lane-pair shape of G2 and both team shapes run with the plan's block size on one host thread per lane, which
is what exercises the pair exchanges and the mailbox barriers.  The shape is forced through BLSGPU_GNTT_TEAM_MAX, the override the
library reads.

That the tests bite was checked by seeding faults into gntt.hip.h one at a time (each was confirmed to fail, then removed):
  * a twiddle exponent without the per-stage stride -- the table level of another stage, `gn_tw_off(stage - 1) + (j >> 1)`:
    test_naive_definition fails at n = 4 (2 of 4 points differ), test_round_trip_and_both_shapes and test_vectors_are_independent
    likewise; with `gn_tw_off(stage + 1) + j` the child ends reading past the twiddle table at n = 4 (SIGSEGV at the guard page);
  * bit reversal over the whole array instead of per vector (`j = p` in k_gntt_permute): test_naive_definition fails at the first
    k = 3 with n >= 4 (points of the later vectors differ), test_vectors_are_independent and the round trip likewise;
  * the missing n^-1 (stage 0 never takes `ninv`): the inverse cases of test_naive_definition and the round trip fail from n = 2 on,
    the forward cases pass;
  * `a - t` written as `t - a` (`op.add(pt_neg(x), y)`): test_naive_definition fails at n = 2, k = 3 in both directions.

Run time on an 8-core machine: 5 to 8 minutes.  A minute is the build of the library and about a minute and a half the oracle's side of
the naive case list (its n^2 products per vector are cached per point); the rest is the emulation itself, most of it the G2 sizes
of the discrete-log identity, whose lane-pair and team shapes run one host thread per lane."""

import numpy as np
import pytest

import simt_gntt_child as child
import simt_harness
from g_ntt_points import G, RR, dlog_expect, naive, scalars

LANE_MAX, TEAM_MAX = 0, 1 << 40                                    # BLSGPU_GNTT_TEAM_MAX values that force a shape


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    return simt_harness.emu_lib(child.build)


def _job(g, vecs, inverse=False, team_max=LANE_MAX, label=""):
    """vecs: k lists of n projective oracle points"""
    grp = G[g]
    data = np.stack([grp.wire(v) for v in vecs])
    return {"op": "many", "group": g, "data": data, "inverse": inverse, "team_max": team_max,
            "label": "G%d n=%d k=%d inverse=%s team_max=%s %s" % (g, len(vecs[0]), len(vecs), inverse, team_max, label)}


def _assert_points(g, res, want_vecs, what):
    got = G[g].affine(res["out"])
    want = [a for v in want_vecs for a in G[g].affine_of(v)]
    assert len(got) == len(want)
    bad = [i for i in range(len(got)) if got[i] != want[i]]
    assert not bad, "%s: %d of %d points differ, first at %d" % (what, len(bad), len(got), bad[0])


def _random_vectors(g, k, n, seed):
    """k vectors of n random subgroup points as projective triples with Z != 1; the identity at the first, a middle and the last
    position of some vector, and (k > 1) one vector that is all identity"""
    grp = G[g]
    vecs = [[grp.base_mul(s) for s in scalars(n, seed + 17 * v)] for v in range(k)]
    assert all(p[2] not in (1, (1, 0)) for v in vecs for p in v)
    ident = grp.identity
    for pos in sorted({0, n // 2, n - 1}):
        vecs[0][pos] = ident
    if k > 1:
        vecs[1] = [ident] * n
    return vecs


NAIVE_SIZES = [(n, k) for n in (1, 2, 4, 8, 16) for k in (1, 3)]


@pytest.mark.parametrize("g", [1, 2], ids=["G1", "G2"])
@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
def test_naive_definition(g, inverse):
    """Y[m] = sum_j [w^(jm)] P[j] and its inverse, term by term in the oracle, n in {1, 2, 4, 8, 16}, k in {1, 3}"""
    cases = [(_random_vectors(g, k, n, 1000 * g + 10 * n + k), n, k) for n, k in NAIVE_SIZES]
    res = child.run([_job(g, vs, inverse) for vs, _, _ in cases])
    for (vs, n, k), r in zip(cases, res):
        _assert_points(g, r, [naive(G[g], v, inverse) for v in vs], "G%d n=%d k=%d" % (g, n, k))


DLOG_SIZES = {1: [(n, k) for n in (32, 64, 256) for k in (1, 2, 5)], 2: [(n, k) for n in (32, 64) for k in (1, 2, 5)]}


@pytest.mark.parametrize("g", [1, 2], ids=["G1", "G2"])
def test_discrete_log_identity(g):
    """P[j] = [s_j] G  ->  [fr_ntt(s)_m] G, with 0, 1 and r - 1 among the s_j; the last size of each group also inverse"""
    cases = [([scalars(n, 7 * n + k + v, special=True) for v in range(k)], n, k, False) for n, k in DLOG_SIZES[g]]
    n, k = DLOG_SIZES[g][-1]
    cases.append(([scalars(n, 9 * n + k + v, special=True) for v in range(k)], n, k, True))
    res = child.run([_job(g, [[G[g].base_mul(s) for s in v] for v in ss], inv) for ss, _, _, inv in cases])
    for (ss, n, k, inv), r in zip(cases, res):
        _assert_points(g, r, [dlog_expect(G[g], s, inv) for s in ss], "G%d n=%d k=%d inverse=%s" % (g, n, k, inv))


@pytest.mark.parametrize("g", [1, 2], ids=["G1", "G2"])
def test_round_trip_and_both_shapes(g):
    """inverse after forward gives the input as affine points, through the lane shape and through the team shape, and the two shapes
    give the same affine points on the same input in both directions"""
    cases = [_random_vectors(g, k, n, 50 * n + k) for n, k in ((2, 3), (8, 2), (16, 3), (32, 1))]
    fwd = child.run([_job(g, vs, False, tm) for vs in cases for tm in (LANE_MAX, TEAM_MAX)])
    back = child.run([{"op": "many", "group": g, "data": f["out"], "inverse": True, "team_max": tm, "label": "back %d" % i}
                      for i, (f, tm) in enumerate(zip(fwd, [tm for _ in cases for tm in (LANE_MAX, TEAM_MAX)]))])
    for i, vs in enumerate(cases):
        lane, team = fwd[2 * i], fwd[2 * i + 1]
        assert (lane["shape"], team["shape"]) == (child.LANE, child.TEAM)
        assert G[g].affine(lane["out"]) == G[g].affine(team["out"]), "forward: the shapes differ, case %d" % i
        assert G[g].affine(back[2 * i]["out"]) == G[g].affine(back[2 * i + 1]["out"]), "inverse: the shapes differ, case %d" % i
        for b, name in ((back[2 * i], "lane"), (back[2 * i + 1], "team")):
            _assert_points(g, b, vs, "round trip through the %s shape, case %d" % (name, i))
    # the team shape against the oracle's definition directly as well (not only against the other shape), in both directions:
    # the inverse one is the path with the two n^-1 products of stage 0 on a team
    inv = child.run([_job(g, vs, True, TEAM_MAX) for vs in cases[1:3]])
    _assert_points(g, fwd[5], [naive(G[g], v) for v in cases[2]], "team shape, n=16 k=3")
    for vs, r in zip(cases[1:3], inv):
        assert r["shape"] == child.TEAM
        _assert_points(g, r, [naive(G[g], v, True) for v in vs], "team shape, inverse, n=%d k=%d" % (len(vs[0]), len(vs)))


def test_plan():
    """the kernel sequence, shape, grid and block for log_n in {0, 1, 2, 5, 12} with B on either side of the crossover"""
    P, F, S = child.K_PERMUTE, child.K_FIRST, child.K_STAGE
    jobs, want = [], []
    for g in (1, 2):
        for log_n in (0, 1, 2, 5, 12):
            for k in (0, 1, 3):
                B = (k << log_n) // 2
                for tm in (None, max(B * g - 1, 0), B * g, LANE_MAX, TEAM_MAX):
                    jobs.append({"op": "plan", "group": g, "log_n": log_n, "k": k, "team_max": tm, "label": "plan G%d %d %d %s" % (g, log_n, k, tm)})
                    want.append((g, log_n, k, B, child.TEAM_MAX_B if tm is None else tm))
    res = child.run(jobs)
    for (g, log_n, k, B, tm), r in zip(want, res):
        steps = r["steps"]
        if log_n == 0 or k == 0:
            assert steps == [], (g, log_n, k)
            continue
        assert len(steps) == log_n + 1                              # the permutation + one step per stage
        shape = child.TEAM if B * g <= tm else child.LANE              # the crossover counts lane-shape lanes: a lane pair per G2 butterfly
        assert [s[0] for s in steps] == [P, F] + [S] * (log_n - 1)
        assert [s[5] for s in steps] == [0] + list(range(log_n))
        assert steps[0][1:5] == (child.LANE, ((k << log_n) + 255) // 256, 256, 0)
        for s in steps[1:]:
            assert s[1] == shape
            if shape == child.TEAM:
                assert s[3] == 64 and s[2] == (B * 8 + 63) // 64 and s[4] == 8 * 6 * 14 * g * 4
            else:
                assert s[3] == 256 and s[2] == (B * g + 255) // 256 and s[4] == 0


@pytest.mark.parametrize("g", [1, 2], ids=["G1", "G2"])
def test_vectors_are_independent(g):
    """changing vector v changes output v and no other (per-vector bit reversal, butterfly blocks that never span vectors)"""
    for n, k, v in [(8, 3, 1), (16, 5, 4)]:
        a = [[G[g].base_mul(s) for s in scalars(n, 300 + 11 * i)] for i in range(k)]
        b = [list(x) for x in a]
        b[v] = [G[g].base_mul(s) for s in scalars(n, 999)]
        ra, rb = child.run([_job(g, a), _job(g, b)])
        pa, pb = G[g].affine(ra["out"]), G[g].affine(rb["out"])
        for i in range(k):
            assert (pa[i * n:(i + 1) * n] == pb[i * n:(i + 1) * n]) == (i != v), (n, k, i)
        _assert_points(g, rb, [dlog_expect(G[g], scalars(n, 999 if i == v else 300 + 11 * i)) for i in range(k)], "changed vector")
