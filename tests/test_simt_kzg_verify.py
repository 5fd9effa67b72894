"""The kernels of batched KZG cell-proof verification (bls12_381_amd/csrc/kzg_verify.hip.h) on the host: compiled for the CPU through
tests/simt_harness.py / tests/simt/emu_harness.h and launched from the plan of csrc/kzg_verify_plan.h exactly as api_msm.hip launches
them, at the automatic cut of the fold and at chunks of a few cells.  The inverse transforms, the point products, their sums and the MSM
between the kernels run in Python integers in the group-as-scalars model (tests/simt_kzg_verify_child.py), so every stage is compared
with the reference on its own (tests/kzg_verify_ref.py): the effective offsets, the weights rho and rho a with the gathered points, the
cells in natural coset order, agg -- and (A, B) from the finish, whose point arithmetic is real, with [A_s] G1, [B_s] G1 of the oracle.

Three seeded faults (-DKZGV_FAULT=n) must each be told from the real kernels by these cases."""
import functools

import pytest

import kzg_ref as k
import kzg_verify_ref as v
import simt_kzg_verify_child as child
import simt_harness
from oracle import bls12_381_ref as o

R = k.R
SHAPES = [(0, 0), (3, 0), (3, 3), (4, 2), (6, 1), (8, 6)]
CUTS = {"one batch": [0, 5], "one cell each": [0, 1, 2, 3, 4, 5], "empty between": [0, 0, 3, 3, 5]}
CHUNKS = {"automatic": 0, "three cells": 3}


@pytest.fixture(scope="module")
def emu_lib():
    return simt_harness.emu_lib(child.build)


@functools.lru_cache(maxsize=None)
def _inputs(log_n, log_l, order, cut):
    """consistent inputs over an arbitrary SRS (sigma_1 = 0, an identity proof) for 5 cells in the cut, or 300 cells in one batch"""
    rng = o.SplitMix64(7000 + 64 * log_n + 4 * log_l + order)
    c2 = 2 << (log_n - log_l)
    offsets = [0, 300] if cut == "long" else CUTS[cut]
    m = offsets[-1]
    col = [0, c2 - 1, 1 % c2, c2 // 2, 0] if m == 5 else [rng.scalar() % c2 for _ in range(m)]
    r = [rng.scalar() for _ in offsets[1:]]
    commits, row, cells, proofs, sigma, T = v.consistent(rng, log_n, log_l, order, col, offsets, r, zero_sigma=1, zero_proof=1)
    return {"log_n": log_n, "log_l": log_l, "order": order, "commits": commits, "row": row, "col": col, "cells": cells, "proofs": proofs, "offsets": offsets, "r": r, "sigma": sigma, "T": T}


def _jobs(chunk, fault=0, shapes=SHAPES, finish=True, long=True):
    jobs = []
    for log_n, log_l in shapes:
        for order in (k.NATURAL, k.BITREV):
            for cut in CUTS:
                jobs.append(dict(_inputs(log_n, log_l, order, cut), op="verify", label="(%d, %d) order %d, %s, chunk %d" % (log_n, log_l, order, cut, chunk), chunk=chunk, fault=fault,
                                 finish=finish and (log_n, log_l) in ((4, 2), (0, 0), (8, 6)), cut=cut))
    if long:
        for order in (k.NATURAL, k.BITREV):
            for ch in (chunk, 64):
                jobs.append(dict(_inputs(4, 2, order, "long"), op="verify", label="(4, 2) order %d, one batch of 300, chunk %d" % (order, ch), chunk=ch, fault=fault, finish=False, cut="long"))
    return jobs


@functools.lru_cache(maxsize=None)
def _want(log_n, log_l, order, cut):
    j = _inputs(log_n, log_l, order, cut)
    rho, rhoa = v.weights(j["col"], j["offsets"], j["r"], log_n, log_l, order)
    agg = v.aggregate(j["col"], j["cells"], j["offsets"], j["r"], log_n, log_l, order)
    ab = v.batch(j["commits"], j["row"], j["col"], j["cells"], j["proofs"], j["offsets"], j["r"], j["sigma"], j["T"], log_n, log_l, order)
    return rho, rhoa, agg, ab


def _point(s):
    return o.g1_to_affine(o.g1_mul(o.g1_from_affine(o.G1_GEN), s % R))


def _check(j, r):
    what = j["label"]
    log_n, log_l, order, offsets = j["log_n"], j["log_l"], j["order"], j["offsets"]
    nseg, l = len(offsets) - 1, 1 << log_l
    rho, rhoa, agg, ab = _want(log_n, log_l, order, j["cut"])
    assert r["eff"] == offsets and not any(r["mis"]) and r["status"] == 0 and not any(r["badidx"]), what + ": the offsets"
    assert r["off64"] == [t * offsets[-1] + x for t in range(3) for x in offsets[:-1]] + [3 * offsets[-1]] and r["msm_off"] == [s * l for s in range(nseg + 1)] and \
        r["base_first"] == [0] * nseg, what + ": the offsets of the sums and of the MSM"
    assert r["rho"] == rho, what + ": rho"
    assert r["rhoa"] == rhoa, what + ": rho a"
    assert r["gathered"], what + ": the gathered points"
    assert r["natural"] == [v.natural_cell(c, log_l, order) for c in j["cells"]], what + ": the cells in natural coset order"
    assert r["agg"] == agg, what + ": agg"
    if j["finish"]:
        assert r["bad"] == [0] * nseg and r["verdict"] == [w[2] for w in ab], what + ": the verdicts"
        assert r["ab"] == [_point(s) for w in ab for s in w[:2]], what + ": (A, B)"
        assert r["qidx"] == [0, 1] * nseg and r["poff"] == [2 * s for s in range(nseg + 1)], what + ": the pairing terms"


@pytest.mark.parametrize("chunk_name", sorted(CHUNKS))
def test_every_stage_vs_the_reference(emu_lib, chunk_name):
    jobs = _jobs(CHUNKS[chunk_name])
    for j, r in zip(jobs, child.run(jobs)):
        _check(j, r)


def test_the_table_of_roots_is_the_inverse_root_of_order_2n(emu_lib):
    res = child.run([{"op": "roots", "label": "log_n %d" % log_n, "log_n": log_n} for log_n in (0, 4, 12, 23)])
    for log_n, r in zip((0, 4, 12, 23), res):
        winv = pow(o.fr_omega(log_n + 1), R - 2, R)
        assert r["tab"] == [pow(winv, 1 << b, R) for b in range(log_n + 1)], log_n


def test_bad_indices_and_broken_offsets_stay_inside_and_are_flagged(emu_lib):
    """every buffer is guarded: an index used as an address ends the child.  The batch with a bad index, the broken batch and the one behind
    it are flagged and get an identity pair and verdict 0; the others are the reference's."""
    base = _inputs(4, 2, k.NATURAL, "one cell each")
    row, col = list(base["row"]), list(base["col"])
    row[1], col[3] = 0xFFFFFFFF, 8
    idx = dict(base, op="verify", label="row = 2^32 - 1, col = 2c", row=row, col=col, finish=True, chunk=3)
    off = dict(base, op="verify", label="offsets 0 1 5 3 9 5", offsets=[0, 1, 5, 3, 9, 5], finish=True, chunk=3)
    ri, ro = child.run([idx, off])
    _, _, _, ab = _want(4, 2, k.NATURAL, "one cell each")
    ident = o.G1_IDENTITY_AFF
    assert ri["status"] == child.STATUS_BAD and ri["badidx"] == [0, 1, 0, 1, 0] and ri["bad"] == [0, 1, 0, 1, 0] and ri["gathered"]
    assert ri["rho"][1] == 0 and ri["rho"][3] == 0 and ri["rhoa"][1] == 0
    assert ri["verdict"] == [w[2] if s not in (1, 3) else 0 for s, w in enumerate(ab)]
    assert ri["ab"] == [ident if s // 2 in (1, 3) else _point(ab[s // 2][s % 2]) for s in range(10)]
    assert ro["eff"] == [0, 1, 5, 5, 5, 5] and ro["mis"] == [0, 0, 0, 1, 1, 0] and ro["status"] == child.STATUS_BAD
    assert ro["bad"] == [0, 0, 1, 1, 1] and ro["verdict"][2:] == [0, 0, 0] and ro["ab"][4:] == [ident] * 6
    assert ro["ab"][:2] == [_point(ab[0][0]), _point(ab[0][1])]


def test_the_plan_the_emulation_walks_is_the_shipped_one(emu_lib):
    r = child.run([{"op": "plan", "label": "blobs", "log_n": 12, "log_l": 6, "m": 8192, "nseg": 1}, {"op": "plan", "label": "tiny", "log_n": 4, "log_l": 2, "m": 300, "nseg": 1, "chunk": 3},
                   {"op": "plan", "label": "refused", "log_n": 4, "log_l": 2, "m": 1, "nseg": 0}])
    assert (r[0]["ok"], r[0]["chunk"], r[0]["nchunks"]) == (1, 8, 1024) and r[0]["part"] == 2 * 1024 * 64 * 32 and r[0]["scal"] == 3 * 8192 * 32
    assert (r[1]["ok"], r[1]["chunk"], r[1]["nchunks"]) == (1, 3, 100)
    assert r[2]["ok"] == 0


FAULTS = {1: "rho's exponent taken from k instead of k - offsets[s]", 2: "h^(+u) in place of h^(-u)", 3: "the fold dropping the last cell of a chunk"}


@pytest.mark.parametrize("chunk_name", sorted(CHUNKS))
@pytest.mark.parametrize("fault", sorted(FAULTS), ids=["fault%d" % f for f in sorted(FAULTS)])
def test_seeded_faults_are_caught(emu_lib, fault, chunk_name):
    """the same cases must tell a kernel with ONE seeded fault from the real one, at either cut: a suite that passes a broken kernel checks
    nothing"""
    simt_harness.emu_lib(lambda: child.build_fault(fault))
    jobs = _jobs(CHUNKS[chunk_name], fault, [(4, 2), (6, 1)], finish=False)
    caught = False
    for j, r in zip(jobs, child.run(jobs)):
        try:
            _check(j, r)
        except AssertionError:
            caught = True
    assert caught, "no case tells fault %d (%s) from the real kernels (%s chunk)" % (fault, FAULTS[fault], chunk_name)
