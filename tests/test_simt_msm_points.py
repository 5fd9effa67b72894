"""The point kernels behind the sort of the large MSM -- `k_msm_accumulate_g2pair`, `k_msm_heavy<F>`, the level forms
`k_wsum_level_team2` / `_team` / `_pair` / `_g2pair`, `k_tree_sum<F>`, `k_tree_sum_team_multi<F>`, `k_shift_add_team<F>` and
`k_msm_combine_team<F>` -- compiled for the HOST (tests/simt/emu_msm.cpp) and run ONE STAGE AT A TIME on hand-built records, with the
grid and block shapes of api_msm.hip, and the whole bucket reduction by the schedule of csrc/msm_plan.h (`test_whole_reduction`: the
driver logic of api_msm.hip msm_reduce -- levels, tree steps, Horner -- on the host).  Every record is [e] G for a known exponent e, so every expectation is the oracle's
[f(e ...)] G by exponent arithmetic (`_gen_multiples`, the C oracle's double-and-add) with the level sums of tests/msm_pipe_model.py;
results are compared as affine points.  Every record buffer holds exactly the records the stage may touch and ends against an
inaccessible page: a read or write past the last record, which DevBuf's slack swallows on the GPU, ends the child process.

Known limits: `emu_update_dpp` ignores row mask, bank mask and bound control, so the lane exchanges of the pair forms are vouched for
by the dense GPU runs of tests/test_msm_pipeline_gpu.py; the emulated dynamic LDS is a fixed array, so a launch that asks for too
few LDS bytes is not caught here.  Cases are sized in teams, G2 with fewer shapes than G1, no class of cases cut.

Seeded faults (msm.hip.h on a scratch copy, one at a time) and the test that fails:
  `|| off` dropped in k_wsum_level_team2         test_level_forms (the off = 1 shapes: T misses the weight-1 record of every chunk)
  `if (j < n)` removed in msm_heavy_big          test_heavy_fold (partial counts 17, 65, 72: the read past the last record hits the
                                                 guard page, or a neighbour's partials are added)
  `k < M &&` removed in k_tree_sum_team_multi    test_tree_sums, the trees (9, 3) / (10, 2) next to M = 8 (a group adds the next group's
                                                 records).  Under tree_step's own rule M = min(8, n) a job with M < maxM has n = M, so
                                                 `i < n` implies `k < M` and the fault cannot show: the first version of the test, which
                                                 restated that rule only, let it pass.
  `off = 0` at the bottom level of the schedule  test_whole_reduction (seeded through the entry point's `fault` argument: every window
                                                 sum misses sum_b e_b)

Cost: about 25 s (one run on one machine, the library already built) where tests/test_simt_msm.py takes 170 s.
"""
import numpy as np
import pytest

import msm_pipe_model as mm
import simt_msm_child as child
from oracle import bls12_381_ref as o
from test_simt_msm import _affine, _as_points, _bases, _gen_multiples, emu_lib  # noqa: F401  (emu_lib: the module's autouse fixture)

RR = o.R_ORDER
ONE = np.array(o.fp_to_mont_limbs(1), dtype=np.uint64)
ZERO = np.zeros(6, dtype=np.uint64)
GROUPS = [1, 2]


def _proj(group, exps):
    """[e] G as projective wire limbs (x, y, 1); e = 0 mod r: the identity (0, 1, 0)"""
    xy, inf = _gen_multiples(group, exps)
    one = ONE if group == 1 else np.concatenate([ONE, ZERO])
    zero = np.zeros_like(one)
    return np.stack([np.concatenate([zero, one, zero]) if inf[i] else np.concatenate([xy[i], one]) for i in range(len(exps))])


def _want(group, exps):
    return _as_points(*_gen_multiples(group, exps))


def _exps(n, seed, special=True):
    """exponents with identities sprinkled in, equal neighbours (the running sum doubles) and a record followed by its negative (the
    running sum passes through the identity)"""
    r = o.SplitMix64(seed)
    e = [r.next() % 1000 + 1 for _ in range(n)]
    if special:
        for i in range(0, n, 5):
            e[i] = 0
        if n >= 4:
            e[n - 1] = r.next() % 1000 + 1
            e[n - 2] = e[n - 1]                                      # the chain runs from the high index down: R doubles at once
        if n >= 8:
            e[n - 5] = RR - e[n - 4] - e[n - 3] - 2 * e[n - 1]       # ... and passes through the identity
    return e


# ---- A4 --------------------------------------------------------------------------------------------------------------------------
def test_g2_bucket_accumulation_items():
    """the item lists of the G1 test on lane pairs: lengths 0, 1, 2 and 70, negated entries, identity records first / middle / last, the
    last item ending at the last word of `sorted`; and lists that make the pair leave the fast loop: P then P, P then -P then a
    further point, the same after 20 generic additions, identity and negated entries after the switch"""
    r = o.SplitMix64(77)
    ks = [r.scalar() for _ in range(10)]
    ID = 8
    ks[ID] = 0
    ks[4] = ks[3]
    ks[5] = (RR - ks[3]) % RR
    n, NEG = len(ks), 1 << 31
    lists = [[], [2], [0, 1 | NEG], [3, 4, 6], [3, 5, 7], [3, 3 | NEG], [ID, 1, ID, 2, ID], [3, 3],
             [i % n | (NEG if i % 2 else 0) for i in range(70)],
             [0, 1, 2] * 7 + [3, 4, 6],                              # the switch after 21 generic additions: a doubling
             [0, 1, 2] * 7 + [3, 5, 7, ID, 1 | NEG, ID, 2],          # ... a cancellation, then identities and negated entries
             [3, 4, ID, 6 | NEG, 3 | NEG, ID],
             [5, n - 1]]                                             # the last word of `sorted` names the last record
    sorted_, items = [], []
    for d, l in enumerate(lists):
        items.append((len(sorted_), len(l), len(lists) - 1 - d))
        sorted_ += l
    dlog = lambda e: -ks[e & (NEG - 1)] if e & NEG else ks[e & (NEG - 1)]
    want = _want(2, [sum(dlog(e) for e in l) for l in lists])
    xy, inf = _bases(2, ks)
    jobs = [{"op": "bases", "label": "bases", "group": 2, "xy": xy, "inf": inf},
            {"op": "accumulate_g2", "label": "items", "bases": 0, "sorted": np.array(sorted_, dtype=np.uint32), "items": np.array(items, dtype=np.uint32),
             "ctrl": np.array([0, 0, len(items), 0], dtype=np.uint32), "max_items": len(items), "ndest": len(items)},
            {"op": "accumulate_g2", "label": "more lanes than items", "bases": 0, "sorted": np.array([1, 2 | NEG, n - 1], dtype=np.uint32),
             "items": np.array([(0, 3, 0)], dtype=np.uint32), "ctrl": np.array([0, 0, 1, 0], dtype=np.uint32), "max_items": 200, "ndest": 1}]
    res = child.run(jobs)
    got = _affine(2, res[1]["records"])
    for d, l in enumerate(lists):
        assert got[len(lists) - 1 - d] == want[d], "item %d %s" % (d, [hex(e) for e in l[:6]])
    assert want[0] is None and want[5] is None
    assert _affine(2, res[2]["records"]) == _want(2, [ks[1] - ks[2] + ks[n - 1]])


# ---- A5 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUPS)
def test_heavy_fold(group):
    """partial counts 2, 16 (one lane), 17, 64, 65, 72 (a block; the in-place tree runs strides 1, 8, 64) in one launch of the product's
    grid; among the partials identities, a repeated point, a point and its negative.  The bucket record = the oracle's sum, every
    other record unchanged; ctrl[1] = 0 leaves everything unchanged."""
    counts = [2, 16, 17, 64, 65, 72]
    nb = 8
    buckets = [0, 2, 3, 5, 6, 7]                                    # buckets 1 and 4 are not cut
    exps = _exps(nb, 11, special=False)
    heavy, big, dest = [], [], nb
    for h, (b, k) in enumerate(zip(buckets, counts)):
        part = _exps(k, 100 + k)
        if k == 2:
            part = [7, RR - 7]
        exps += part
        heavy.append((b, dest, k, 0))
        if k > mm.HEAVY_SMALL:
            big.append(h)
        dest += k
    want = list(exps)
    for (b, d0, k, _) in heavy:
        want[b] = sum(exps[d0:d0 + k])
    rec = _proj(group, exps)
    jobs = [{"op": "heavy", "label": "six cut buckets", "group": group, "records": rec, "heavy": heavy, "big": big[::-1], "ctrl": [dest - nb, len(heavy), 0, len(big)], "nb": nb},
            {"op": "heavy", "label": "no cut bucket", "group": group, "records": rec, "heavy": [], "big": [], "ctrl": [0, 0, 0, 0], "nb": nb}]
    res = child.run(jobs)
    got = _affine(group, res[0]["records"])
    wantp = _want(group, want)
    inp = _want(group, exps)
    part_of = {d: h for h, (b, d0, k, _) in enumerate(heavy) for d in range(d0, d0 + k)}
    for i in range(len(exps)):
        if i < nb:
            assert got[i] == wantp[i], "bucket %d" % i
        elif heavy[part_of[i]][2] <= mm.HEAVY_SMALL:
            assert got[i] == inp[i], "partial record %d of a lane-folded bucket changed" % i      # the block fold works in place
    assert _affine(group, res[1]["records"]) == inp


# ---- A6 --------------------------------------------------------------------------------------------------------------------------
LEVEL_SHAPES = [(1, 8, 8, 1), (3, 16, 8, 1), (2, 64, 8, 0), (3, 4, 4, 0), (2, 2, 2, 1), (1, 8, 8, 0), (1, 8 * 33, 8, 1)]
#               (nseg, n, M, off); the last: 33 chains, so that most of the last block is not live in every form


@pytest.mark.parametrize("shape", LEVEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("group", GROUPS)
def test_level_forms(group, shape):
    """R_g = sum E_j and T_g = sum (j - g M + off) E_j over every chunk, by every form the group has, on the same records"""
    nseg, n, M, off = shape
    if group == 2 and shape in ((2, 64, 8, 0), (1, 8 * 33, 8, 1)):
        nseg, n = (1, 24) if shape[3] == 0 else (1, 8 * 17)          # G2: fewer chains, the same classes (17 teams: two blocks in the team form)
    exps = _exps(nseg * n, 7 * n + M + off)
    E = _proj(group, exps)
    jobs = [{"op": "level", "label": "form %d %r" % (f, shape), "group": group, "form": f, "E": E, "nseg": nseg, "n": n, "M": M, "off": off} for f in (0, 1, 2)]
    R, T = [], []
    for s in range(nseg):
        r, t = mm.level_sums(exps[s * n:(s + 1) * n], M, off)
        R += r; T += t
    wr, wt = _want(group, R), _want(group, T)
    for f, res in zip("team2 team pair".split(), child.run(jobs)):
        assert _affine(group, res["R"]) == wr, f
        assert _affine(group, res["T"]) == wt, f


# ---- A7 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUPS)
def test_tree_sums(group):
    """`k_tree_sum_team_multi` with 1, 3 and 8 trees per launch, fan-ins that differ inside a launch (maxM = 8 next to M = 1, 2, 3), n no
    multiple of M (n = 9, M = 8), nseg 1..3; `k_tree_sum` on the same trees.

    Reachability of the one-lane `k_tree_sum`, by reading msm_plan.h msm_reduction (MsmTreePass::multi): a tree joins the multi-job launch when
    nseg * TG * TEAM <= TEAM_LANES_MAX and fewer than TREE_JOBS_MAX trees are in it.  TG <= 2^(c-1) / 64 (the first pass of the bottom
    level's T records) and nseg <= ceil(256 / c), so nseg * TG * 8 <= 16 * 512 * 8 = 65536 at c = 16 unmerged and 1 * 16384 * 8 = 131072
    at c = 21 merged: never above the limit.  A level adds a tree only while G > 1, which takes levels 0 .. 5 at most (2^20 buckets,
    fan 8), so there are never 8 trees.  The `k_tree_sum` launch of api_msm.hip msm_tree_step is therefore unreachable with the windows
    the product accepts (tests/cpp/msm_plan_main.cpp holds the schedule of every accepted shape to that); the kernel is kept and tested
    here."""
    # (n, M) per tree and nseg per launch; M = min(8, n) is tree_step's rule, the (9, 3) and (10, 2) trees use the kernel's wider contract
    sets = {1: (2, [(9, 8)]), 3: (1, [(9, 8), (2, 2), (64, 8)]), 8: (3, [(8, 8), (3, 3), (9, 8), (2, 2), (16, 8), (1, 1), (9, 3), (17, 8)])}
    if group == 2:
        sets[8] = (2, [(8, 8), (3, 3), (9, 8), (2, 2), (4, 4), (1, 1), (10, 2), (5, 5)])
    jobs, wants = [], []
    for k, (nseg, trees) in sets.items():
        es = [_exps(nseg * n, 31 * k + n + i) for i, (n, _) in enumerate(trees)]
        jobs.append({"op": "tree_multi", "label": "%d trees" % k, "group": group, "nseg": nseg, "trees": [(_proj(group, e), n, M) for e, (n, M) in zip(es, trees)]})
        w = [[sum(e[s * n + g * M:min(s * n + (g + 1) * M, (s + 1) * n)]) for s in range(nseg) for g in range((n + M - 1) // M)] for e, (n, M) in zip(es, trees)]
        wants.append(w)
        if k == 3:
            for e, (n, M), wi in zip(es, trees, w):
                jobs.append({"op": "tree", "label": "one lane n=%d" % n, "group": group, "E": _proj(group, e), "nseg": nseg, "n": n, "M": M})
                wants.append(wi)
    for j, res, w in zip(jobs, child.run(jobs), wants):
        if j["op"] == "tree":
            assert _affine(group, res["out"]) == _want(group, w), j["label"]
        else:
            for i, (out, wi) in enumerate(zip(res["outs"], w)):
                assert _affine(group, out) == _want(group, wi), "%s, tree %d" % (j["label"], i)


# ---- A8 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUPS)
def test_shift_add_and_combine(group):
    """out = 2^k x + y for k = 1, 2, 3 with an identity on either side and 2^k x = -y; the Horner pass over the windows for
    (nwin, c) = (1, 4), (2, 16), (16, 4) with identity window sums"""
    jobs, wants = [], []
    for k in (1, 2, 3):
        x = [5, 0, 9, 11, 0, 123456789]
        y = [3, 7, 0, RR - (11 << k), 0, RR - 1]
        jobs.append({"op": "shift_add", "label": "k=%d" % k, "group": group, "x": _proj(group, x), "y": _proj(group, y), "k": k})
        wants.append([(a << k) + b for a, b in zip(x, y)])
    for nwin, c in ((1, 4), (2, 16), (16, 4)):
        w = _exps(nwin, 5 * nwin + c) if nwin > 2 else [17, 0][:nwin]
        if nwin == 2:
            w = [0, 17]
        jobs.append({"op": "combine", "label": "nwin=%d c=%d" % (nwin, c), "group": group, "wsums": _proj(group, w), "c": c})
        wants.append([sum(e << (c * i) for i, e in enumerate(w))])
    for j, res, w in zip(jobs, child.run(jobs), wants):
        assert _affine(group, res["out"]) == _want(group, w), j["label"]


# ---- A9 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbw", [1 << 3, 1 << 7, 1 << 10])
@pytest.mark.parametrize("group", GROUPS)
def test_whole_reduction(group, nbw):
    """the driver logic of api_msm.hip msm_reduce on the host: the schedule of msm_plan.h walked over records [e_b] G of nseg = 2 windows
    -- every level in the form the plan picks, the tree passes of every step, the Horner shifts -- gives [sum_b (b + 1) e_b] G per
    window.  nbw = 2^3: one level, no tree; 2^7: three levels, the bottom one with a tree; 2^10: four levels, trees of two passes.
    Once more with the seeded fault (the bottom level runs with off = 0): the result must differ."""
    nseg = 2
    r = o.SplitMix64(0xA9 + nbw + group)
    exps = [r.next() % 1000 + 1 for _ in range(nseg * nbw)]
    for i in range(0, nseg * nbw, 7):
        exps[i] = 0                                                  # empty buckets
    want = [sum((b + 1) * e for b, e in enumerate(exps[s * nbw:(s + 1) * nbw])) for s in range(nseg)]
    for s in range(nseg):
        assert mm.window_sum(exps[s * nbw:(s + 1) * nbw]) == (want[s], want[s])
    rec = _proj(group, exps)
    jobs = [{"op": "reduce", "label": "nbw=%d" % nbw, "group": group, "records": rec, "nseg": nseg, "nbw": nbw}]
    if nbw == 1 << 7:
        jobs.append({"op": "reduce", "label": "nbw=%d, off = 0 at the bottom level" % nbw, "group": group, "records": rec, "nseg": nseg, "nbw": nbw, "fault": 1})
    res = child.run(jobs)
    assert res[0]["levels"] == len(mm.reduction_schedule(nseg, nbw)["levels"]) == {8: 1, 128: 3, 1024: 4}[nbw]
    assert _affine(group, res[0]["wsums"]) == _want(group, want)
    if len(jobs) > 1:
        assert _affine(group, res[1]["wsums"]) != _want(group, want), "the seeded fault was not caught"
        assert _affine(group, res[1]["wsums"]) == _want(group, [w - sum(exps[s * nbw:(s + 1) * nbw]) for s, w in enumerate(want)])
