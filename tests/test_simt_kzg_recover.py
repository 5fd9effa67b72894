"""The kernels of KZG cell recovery (bls12_381_amd/csrc/kzg_recover.hip.h) on the host: compiled for the CPU through
tests/simt_harness.py / tests/simt/emu_harness.h and launched from the plan of csrc/kzg_recover_plan.h exactly as api_fr.hip launches
them, at the shipped tiles and at tiny ones (a scatter tile of 4, three roots per LDS tile).  The transforms and the batch inversion
between the kernels run in Python integers (tests/simt_kzg_recover_child.py), so every stage is compared with the reference on its own
(tests/kzg_recover_ref.py): the effective offsets, the slot table and the status words, the roots, Zd, Zc, EZ, the scaled vector, and
the finish (polys and ok).  Every comparison is exact.

Three seeded faults (-DKZG_REC_FAULT=n) must each be told from the real kernels by these cases."""
import functools

import pytest

import kzg_ref as k
import kzg_recover_ref as rr
import simt_kzg_recover_child as child
import simt_harness
from oracle import bls12_381_ref as o

R = k.R
SHAPES = [(0, 0), (3, 0), (3, 3), (4, 2), (6, 1), (8, 2), (8, 6)]
TILES = {"shipped": (0, 0), "tiny": (4, 3)}                       # (scatter tile, roots per LDS tile)
GROUPS = (("exactly-c-random", "all", "first-half"), ("c-plus-1", "second-half", "every-other"), ("shuffled", "exactly-c-random", "c-plus-1"))
STAGES = ("eff", "mis", "slot", "status", "rootd", "rootc", "zd", "zc", "ez", "scaled", "upper", "polys", "ok")


@pytest.fixture(scope="module")
def emu_lib():
    return simt_harness.emu_lib(child.build)


@functools.lru_cache(maxsize=None)
def _good(log_n, log_l, order, group):
    """three polynomials, each with its own pattern; the polynomials rotate through the special ones"""
    rng = o.SplitMix64(9100 + 64 * log_n + 4 * log_l + order + 1000 * group)
    pats = rr.patterns(rng, log_n, log_l)
    polys = rr.special_polys(rng, 1 << log_n, 1 << log_l)
    polys = [polys[(group + i) % 4] for i in range(3)]
    col, offsets, cells = rr.call_inputs(polys, [pats[name] for name in GROUPS[group]], log_n, log_l, order)
    return {"log_n": log_n, "log_l": log_l, "order": order, "col": col, "offsets": offsets, "cells": cells, "polys": polys}


@functools.lru_cache(maxsize=None)
def _want(log_n, log_l, order, group):
    j = _good(log_n, log_l, order, group)
    return rr.stages(j["col"], j["offsets"], j["cells"], log_n, log_l, order)


def _expected(j, want):
    m = j.get("m", len(j["col"]))
    eff, mis = rr.effective(j["offsets"], m)
    rd, rc = rr.roots(j["log_n"], j["log_l"])
    c2, n = 2 << (j["log_n"] - j["log_l"]), 1 << j["log_n"]
    bad = [s != 0 for s in want["status"]]
    return dict(want, eff=eff, mis=mis, rootd=rd, rootc=rc, upper=[1 if not b and any(q[n:]) else 0 for b, q in zip(bad, want["q"])])


def _compare(j, r, want):
    exp = _expected(j, want)
    for stage in STAGES:
        assert r[stage] == exp[stage], "%s: %s" % (j["label"], stage)
    assert (r["sticky"] != 0) == any(exp["status"]), j["label"] + ": the sticky word"
    assert r["sticky"] in (0, 1 << 7), j["label"] + ": the sticky word holds another bit"


def _good_jobs(tiles, fault=0, shapes=SHAPES):
    tile, root_tile = TILES[tiles]
    return [dict(_good(log_n, log_l, order, g), op="recover", tile=tile, root_tile=root_tile, fault=fault, group=g,
                 label="(%d, %d) order %d, patterns %s, %s tiles" % (log_n, log_l, order, "/".join(GROUPS[g]), tiles))
            for log_n, log_l in shapes for order in (k.NATURAL, k.BITREV) for g in range(len(GROUPS))]


@pytest.mark.parametrize("tiles", list(TILES))
def test_every_stage_is_the_reference(emu_lib, tiles):
    jobs = _good_jobs(tiles)
    for j, r in zip(jobs, child.run(jobs, timeout=900)):
        want = _want(j["log_n"], j["log_l"], j["order"], j["group"])
        _compare(j, r, want)
        assert r["ok"] == [1, 1, 1] and r["polys"] == j["polys"], j["label"] + ": the polynomials do not come back"


@pytest.mark.parametrize("log_n,log_l", [(3, 0), (4, 2), (6, 1)])
def test_malformed_polynomials_are_contained(emu_lib, log_n, log_l):
    jobs, wants = [], []
    for order in (k.NATURAL, k.BITREV):
        polys, cases = rr.malformed_cases(log_n, log_l, order)
        for name, (col, off, cells, m, bad) in cases.items():
            jobs.append({"op": "recover", "log_n": log_n, "log_l": log_l, "order": order, "col": col, "offsets": off, "cells": cells, "m": m, "tile": 4, "root_tile": 3,
                         "label": "(%d, %d) order %d, %s" % (log_n, log_l, order, name)})
            wants.append((polys, bad))
    for j, r, (polys, bad) in zip(jobs, child.run(jobs, timeout=900), wants):
        want = rr.stages(j["col"], j["offsets"], j["cells"], log_n, log_l, j["order"])
        _compare(j, r, want)
        count = len(j["offsets"]) - 1
        assert [v for v in range(count) if r["status"][v]] == bad, j["label"] + ": the wrong polynomials are flagged"
        for v in range(count):
            if v in bad:
                assert r["ok"][v] == 0 and not any(r["polys"][v]) and all(s == -1 for s in r["slot"][v]), j["label"] + ": polynomial %d is not zeroed" % v
            else:
                assert r["ok"][v] == 1 and r["polys"][v] == polys[v], j["label"] + ": neighbour %d is wrong" % v


def _crafted_q(log_n):
    """Q with one non-zero coefficient, the LAST of the upper half; one that is consistent; one non-zero at the first of the upper half"""
    n = 1 << log_n
    rng = o.SplitMix64(31 + log_n)
    rows = [[rng.scalar() for _ in range(n)] + [0] * n for _ in range(3)]
    rows[0][2 * n - 1] = 1
    rows[2][n] = R - 1
    return rows


@pytest.mark.parametrize("log_n,log_l", [(0, 0), (3, 1), (9, 3)])
def test_the_finish_reads_the_whole_upper_half(emu_lib, log_n, log_l):
    q = _crafted_q(log_n)
    n = 1 << log_n
    jobs = [{"op": "finish", "log_n": log_n, "log_l": log_l, "q": q, "status": st, "label": "finish (%d, %d) status %s" % (log_n, log_l, st)} for st in ([0, 0, 0], [0, 8, 0])]
    for j, r in zip(jobs, child.run(jobs)):
        ok = [0, 0 if j["status"][1] else 1, 0]
        assert r["ok"] == ok and r["upper"] == [1, 0, 1], j["label"]
        assert r["polys"] == [row[:n] if g else [0] * n for row, g in zip(q, ok)], j["label"]


def test_inconsistent_cells_are_told_from_consistent_ones(emu_lib):
    """with c + 1 and with 2c cells one changed entry gives ok = 0 and zero rows for that polynomial alone; with exactly c cells the same
    change gives ok = 1 and the reference's other polynomial"""
    jobs = []
    for log_n, log_l in ((4, 2), (6, 1)):
        for order in (k.NATURAL, k.BITREV):
            for group, changed, ok in ((0, (0, 1), [1, 0, 1]), (1, (0,), [0, 1, 1])):      # exactly c / all / first half;  c + 1 / second half / every other
                j = dict(_good(log_n, log_l, order, group))
                cells = [list(c) for c in j["cells"]]
                for v in changed:
                    kk = j["offsets"][v] + v
                    cells[kk][(1 << log_l) - 1] = (cells[kk][-1] + 1 + v) % R
                jobs.append(dict(j, cells=cells, op="recover", tile=4, root_tile=3, want_ok=ok, changed=changed,
                                 label="(%d, %d) order %d, group %d, changed entries" % (log_n, log_l, order, group)))
    for j, r in zip(jobs, child.run(jobs, timeout=900)):
        want = rr.stages(j["col"], j["offsets"], j["cells"], j["log_n"], j["log_l"], j["order"])
        _compare(j, r, want)
        assert r["ok"] == j["want_ok"] and r["sticky"] == 0, j["label"]
        for v in range(3):
            if v not in j["changed"]:
                assert r["polys"][v] == j["polys"][v], j["label"]
            elif j["want_ok"][v]:
                assert r["polys"][v] != j["polys"][v] and any(r["polys"][v]), j["label"] + ": exactly c cells give another polynomial"
            else:
                assert not any(r["polys"][v]), j["label"] + ": an inconsistent polynomial is not zeroed"


# ---- the seeded faults ---------------------------------------------------------------------------------------------------------------
def _differs(jobs, results, wants):
    for j, r, want in zip(jobs, results, wants):
        exp = _expected(j, want)
        if any(r[s] != exp[s] for s in STAGES):
            return True
    return False


@pytest.mark.parametrize("fault", child.FAULTS)
def test_a_seeded_fault_is_told_from_the_real_kernels(emu_lib, fault):
    simt_harness.emu_lib(functools.partial(child.build_fault, fault))
    if fault == 3:
        q = _crafted_q(3)
        jobs = [{"op": "finish", "log_n": 3, "log_l": 1, "q": q, "status": [0, 0, 0], "fault": fault, "label": "fault 3: finish"}]
        r = child.run(jobs)[0]
        assert r["ok"] != [0, 1, 0], "the check that reads half of the upper half passes the finish test"
        return
    shapes = [(4, 2), (6, 1)]
    jobs = _good_jobs("shipped", fault, shapes) + _good_jobs("tiny", fault, shapes)
    wants = [_want(j["log_n"], j["log_l"], j["order"], j["group"]) for j in jobs]
    assert _differs(jobs, child.run(jobs, timeout=900), wants), "seeded fault %d passes every stage comparison" % fault
