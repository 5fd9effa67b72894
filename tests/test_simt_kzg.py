"""The data movement of the amortised KZG openings (bls12_381_amd/csrc/kzg.hip.h) on the host: the kernels compiled for the CPU through
tests/simt_harness.py / tests/simt/emu_harness.h and launched from the plan of csrc/kzg_plan.h exactly as api_msm.hip launches them, at
a transposition tile of 4 and at the shipped one.  The transforms and the MSM between the kernels run in Python integers in the
group-as-scalars model of tests/kzg_ref.py (tests/simt_kzg_child.py), so every stage is compared with the contract on its own -- the rows
c^_t, the segment order, S^ and X^, the segments, the identities over the upper half -- and the end of the chain with the DEFINITION of
the proofs by division, over an SRS that is no geometric sequence and holds an identity.  Cells are compared with direct evaluation.

Three seeded faults (-DKZG_FAULT=n) must each be told from the real kernels by these cases."""
import functools

import pytest

import kzg_ref as k
import simt_kzg_child as child
import simt_harness
from oracle import bls12_381_ref as o

SHAPES = [(0, 0), (3, 0), (3, 3), (4, 2), (6, 1), (8, 2), (8, 6)]
COUNT = 3
TILES = {"tiny": 4, "shipped": 0}
ALL = [(f, r) for f in (k.COEFFS, k.EVALS) for r in (k.NATURAL, k.BITREV)]


@pytest.fixture(scope="module")
def emu_lib():
    return simt_harness.emu_lib(child.build)


@functools.lru_cache(maxsize=None)
def _inputs(log_n, log_l):
    rng = o.SplitMix64(300 + 16 * log_n + log_l)
    n = 1 << log_n
    sigma = [rng.scalar() for _ in range(n)]
    if n > 2:
        sigma[2] = None                                            # an identity among the S[m]
    polys = [k.random_poly(rng, n) for _ in range(COUNT)]
    for j, v in enumerate((0, 1, k.R - 1)[:n]):
        polys[0][n - 1 - j] = v
    return sigma, polys


def _form(polys, form, order):
    return [k.to_evals(p, order) if form == k.EVALS else list(p) for p in polys]


def _proof_jobs(tile, fault=0, shapes=SHAPES, combos=ALL):
    jobs = []
    for log_n, log_l in shapes:
        sigma, polys = _inputs(log_n, log_l)
        for form, order in combos:
            jobs.append({"op": "proofs", "label": "(%d, %d) form %d order %d tile %d" % (log_n, log_l, form, order, tile), "log_n": log_n, "log_l": log_l, "sigma": sigma,
                         "polys": _form(polys, form, order), "form": form, "order": order, "tile": tile, "fault": fault})
    return jobs


def _check_proofs(j, r):
    log_n, log_l = j["log_n"], j["log_l"]
    sigma, polys = _inputs(log_n, log_l)
    sig = [0 if s is None else s for s in sigma]
    l, c = 1 << log_l, 1 << (log_n - log_l)
    what = j["label"]
    if c > 1:
        assert r["srs_rows"] == [[None if (s is None or sigma[s] is None) else sigma[s] for s in row] for row in k.srs_rows(sig, log_n, log_l)], what + ": S^"
        assert r["xhat"] == k.xhat(sig, log_n, log_l), what + ": X^"
        assert r["rows"] == [[[0 if s is None else p[s] for s in row] for row in k.coeff_rows(log_n, log_l)] for p in polys], what + ": the rows"
        assert r["seg"] == [k.segment_scalars(p, log_n, log_l) for p in polys], what + ": the segment order"
        assert r["offsets"] == [s * l for s in range(COUNT * 2 * c + 1)] and r["base_first"] == [(s % (2 * c)) * l for s in range(COUNT * 2 * c)], what + ": the segments"
        assert r["filled"], what + ": the upper half"
    want = [k.proofs_by_division(p, sig, log_n, log_l, j["order"]) for p in polys]
    assert [[0 if s is None else s for s in row] for row in r["proofs"]] == want, what + ": the proofs"


@pytest.mark.parametrize("tile_name", sorted(TILES))
def test_every_stage_and_the_proofs_vs_the_contract(emu_lib, tile_name):
    jobs = _proof_jobs(TILES[tile_name])
    for j, r in zip(jobs, child.run(jobs)):
        _check_proofs(j, r)


def _cell_jobs(tile, fault=0, shapes=SHAPES, combos=ALL):
    jobs = []
    for log_n, log_l in shapes:
        _, polys = _inputs(log_n, log_l)
        for form, order in combos:
            jobs.append({"op": "cells", "label": "cells (%d, %d) form %d order %d tile %d" % (log_n, log_l, form, order, tile), "log_n": log_n, "log_l": log_l,
                         "polys": _form(polys, form, order), "form": form, "order": order, "tile": tile, "fault": fault})
    return jobs


@functools.lru_cache(maxsize=None)
def _cells_want(log_n, log_l, order):
    _, polys = _inputs(log_n, log_l)
    return [k.cells(p, log_n, log_l, order) for p in polys]


@pytest.mark.parametrize("tile_name", sorted(TILES))
def test_cells_vs_direct_evaluation(emu_lib, tile_name):
    jobs = _cell_jobs(TILES[tile_name])
    for j, r in zip(jobs, child.run(jobs)):
        assert r["cells"] == _cells_want(j["log_n"], j["log_l"], j["order"]), j["label"]


def test_the_plan_the_emulation_walks_is_the_shipped_one(emu_lib):
    r = child.run([{"op": "plan", "label": "blob", "log_n": 12, "log_l": 6, "count": 2, "form": 1}, {"op": "plan", "label": "tiny", "log_n": 4, "log_l": 2, "count": 3, "tile": 4},
                   {"op": "plan", "label": "c = 1", "log_n": 3, "log_l": 3, "count": 3}])
    assert (r[0]["ok"], r[0]["msm"], r[0]["scalars"], r[0]["points"], r[0]["vectors"]) == (1, 1, 2 * 8192, 2 * 128, 2 * 64)
    assert (r[0]["coeff_bytes"], r[0]["rows_bytes"], r[0]["point_bytes"], r[0]["offset_bytes"]) == (2 * 4096 * 32, 2 * 8192 * 32, 256 * 144, 257 * 4)
    assert (r[0]["transpose_block"], r[0]["transpose_grid"]) == (256, 2 * 4 * 8)
    assert (r[1]["transpose_block"], r[1]["transpose_grid"], r[1]["coeff_bytes"]) == (16, 3 * 1 * 2, 0)
    assert (r[2]["ok"], r[2]["msm"], r[2]["rows_bytes"]) == (1, 0, 0)


FAULTS = {1: "the transposition writing element (t, m) where (m, t) belongs", 2: "the zero padding of the rows one slot short",
          3: "natural numbering where the bit-reversed one is asked"}
FAULT_SHAPES = [(4, 2), (6, 1)]


@pytest.mark.parametrize("tile_name", sorted(TILES))
@pytest.mark.parametrize("fault", sorted(FAULTS), ids=["fault%d" % f for f in sorted(FAULTS)])
def test_seeded_faults_are_caught(emu_lib, fault, tile_name):
    """the same cases must tell a kernel with ONE seeded fault from the real one, at either tile: a suite that passes a broken kernel
    checks nothing"""
    simt_harness.emu_lib(lambda: child.build_fault(fault))
    tile = TILES[tile_name]
    pj, cj = _proof_jobs(tile, fault, FAULT_SHAPES), _cell_jobs(tile, fault, FAULT_SHAPES)
    res = child.run(pj + cj)
    caught = False
    for j, r in zip(pj, res[:len(pj)]):
        try:
            _check_proofs(j, r)
        except AssertionError:
            caught = True
    for j, r in zip(cj, res[len(pj):]):
        caught = caught or r["cells"] != _cells_want(j["log_n"], j["log_l"], j["order"])
    assert caught, "no case tells fault %d (%s) from the real kernels (%s tile)" % (fault, FAULTS[fault], tile_name)
