"""The segmented point sums (bls12_381_amd/csrc/gsum.hip.h) on the host: the two kernels compiled for the CPU through tests/simt_harness.py /
tests/simt/emu_harness.h, one thread per lane, launched from the plan of csrc/gsum_plan.h exactly as api_msm.hip launches them, at a tiny
shape (4 lanes x 2 terms: a chunk of 8 terms) and at the shipped ones, for G1 and G2.  Every expectation is a sum computed by
oracle/bls12_381_ref.py (tests/g_sum_points.py); results are compared as affine points.

The inputs hold segments of 0, 1, 2, chunk - 1, chunk, chunk + 1 and 3 chunks + 1 terms, identities at the start, in the middle and at
the end of a segment, a segment of identities only, one point five times (P + P must double), P, -P, Q (the identity in the middle of a
sum), a curve point outside the subgroup, empty segments first and last, with idx (a pool of 23 points gathered with repeats across
segments) and without.  Offsets beyond `total` are clamped.  An index >= npoints raises the status bit, is never read (the point array
ends against an inaccessible page) and leaves every other segment right.  Four seeded faults (-DGSUM_FAULT=n) must each be told from
the real kernels by these cases, for G1 and G2 at the tiny shape and for G1 at the shipped one.  At the shipped shapes the longest
segment is 2 chunks + 1."""
import functools

import numpy as np
import pytest

import g_sum_points as gp
import simt_gsum_child as child
import simt_harness

TINY = (4, 2)
SHAPES = {"tiny": TINY, "shipped": None}
CHUNK = {("tiny", 1): 8, ("tiny", 2): 8, ("shipped", 1): 256 * 8, ("shipped", 2): 128 * 8}


@pytest.fixture(scope="module")
def emu_lib():
    return simt_harness.emu_lib(child.build)


LONG_CHUNKS = {"tiny": 3, "shipped": 2}                            # the longest segment: that many chunks + 1 term


@functools.lru_cache(maxsize=None)
def _edge_inputs(group, shape_name):
    """the edge list at this shape's chunk, both forms of the call, and the oracle's sums (computed once per shape and group).  At the
    shipped shapes the longest segment is 2 chunks + 1 instead of 3 chunks + 1 -- still a HEAD record in the middle of a combine job,
    a third fewer terms for the one-thread-per-lane emulation."""
    chunk = CHUNK[(shape_name, group)]
    segs = gp.edge_segments(group, chunk, seed=5 + group, long_chunks=LONG_CHUNKS[shape_name])
    return segs, [make(group, segs) for make in (gp.gathered, gp.contiguous)], gp.expected(group, segs)


def _edge_jobs(group, shape_name, fault=0):
    segs, calls, want = _edge_inputs(group, shape_name)
    jobs, wants = [], []
    for form, (xy, inf, idx, off) in zip(("idx", "no idx"), calls):
        jobs.append({"op": "sum", "label": "G%d %s %s" % (group, shape_name, form), "group": group, "xy": xy, "inf": inf, "idx": idx, "offsets": off,
                     "shape": SHAPES[shape_name], "fault": fault})
        wants.append(want)
    return segs, jobs, wants


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("shape_name", ["tiny", "shipped"])
def test_edge_inputs_vs_oracle(emu_lib, group, shape_name):
    _, jobs, wants = _edge_jobs(group, shape_name)
    for j, r, want in zip(jobs, child.run(jobs), wants):
        assert r["rc"] == 0 and r["status"] == 0, j["label"]
        gp.check(group, r["out"], want, j["label"])


def test_the_plan_the_emulation_walks_is_the_shipped_one(emu_lib):
    r = child.run([{"op": "plan", "label": "G1", "group": 1, "nseg": 10, "total": 5000}, {"op": "plan", "label": "G2", "group": 2, "nseg": 10, "total": 5000},
                   {"op": "plan", "label": "tiny", "group": 1, "nseg": 10, "total": 50, "shape": TINY}])
    assert (r[0]["block"], r[0]["terms"], r[0]["chunk"], r[0]["nchunks"]) == (256, 8, 2048, 3) and r[0]["lds"] == 256 * 46 * 4 and r[0]["part_bytes"] == 6 * 176
    assert (r[1]["block"], r[1]["terms"], r[1]["chunk"], r[1]["nchunks"]) == (128, 8, 1024, 5) and r[1]["lds"] == 128 * 86 * 4 and r[1]["part_bytes"] == 10 * 336
    assert (r[2]["chunk"], r[2]["nchunks"], r[2]["chunks_grid"], r[2]["combine_grid"], r[2]["meta_bytes"]) == (8, 7, 7, 14, 56)


@pytest.mark.parametrize("group", [1, 2])
def test_offsets_beyond_total_are_clamped(emu_lib, group):
    """the device form with `total` smaller than the offsets say: the segment across the cut is truncated, those behind it are empty"""
    segs = gp.edge_segments(group, 8, seed=9)
    xy, inf, idx, off = gp.gathered(group, segs)
    cut = int(off[13]) - 11                                        # inside the segment of 3 chunks + 1
    flat = [k for s in segs for k in s]
    cut_segs = [flat[min(int(off[i]), cut):min(int(off[i + 1]), cut)] for i in range(len(segs))]
    assert len(cut_segs[12]) == 25 - 11 and not any(cut_segs[13:])
    huge = off.copy()
    huge[-1] = np.uint64(0xFFFFFFFFFFFFFFFF)
    huge[-2] = np.uint64(1 << 63)
    jobs = [{"op": "sum", "label": "G%d total cut" % group, "group": group, "xy": xy, "inf": inf, "idx": idx[:cut], "offsets": huge, "total": cut, "shape": TINY}]
    r = child.run(jobs)[0]
    assert r["rc"] == 0 and r["status"] == 0
    gp.check(group, r["out"], gp.expected(group, cut_segs), jobs[0]["label"])


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("shape_name", ["tiny", "shipped"])
def test_an_index_outside_the_set_is_flagged_and_never_read(emu_lib, group, shape_name):
    segs, jobs, wants = _edge_jobs(group, shape_name)
    j, want = jobs[0], list(wants[0])
    off = j["offsets"]
    idx = j["idx"].copy()
    npoints = j["xy"].shape[0]
    idx[int(off[7]) + 3] = npoints                                  # the first index past the array: a read of it faults
    idx[int(off[12]) + CHUNK[(shape_name, group)] + 1] = 0xFFFFFFFF
    want[7] = want[12] = None                                       # unspecified
    j = dict(j, idx=idx, label=j["label"] + " bad index")
    r = child.run([j])[0]
    assert r["rc"] == 0 and r["status"] == child.STATUS_BAD
    gp.check(group, r["out"], want, j["label"])


def test_refusals_launch_nothing(emu_lib):
    segs = gp.edge_segments(1, 8, seed=1)
    xy, inf, idx, off = gp.contiguous(1, segs, extra=0)
    short = {"op": "sum", "label": "no idx, total > npoints", "group": 1, "xy": xy[:-1], "inf": inf[:-1], "idx": None, "offsets": off, "shape": TINY}
    none = {"op": "sum", "label": "nseg == 0", "group": 1, "xy": xy, "inf": inf, "idx": None, "offsets": np.zeros(1, dtype=np.uint64), "shape": TINY}
    r = child.run([short, none])
    assert r[0]["rc"] == -1 and (r[0]["out"] == np.uint64(0xA5A5A5A5A5A5A5A5)).all()
    assert r[1]["rc"] == 0 and r[1]["out"].shape[0] == 0


FAULTS = {1: "the last term of a chunk dropped", 2: "the combine pass skipping a segment's first partial", 3: "the identity flag ignored",
          4: "the head of a lane's slice never added to the lane before it"}


# every fault against G1 and G2 at the tiny shape and against the shipped G1 shape (256 lanes x 8 terms)
FAULT_CASES = [(1, "tiny"), (2, "tiny"), (1, "shipped")]


@pytest.mark.parametrize("group,shape_name", FAULT_CASES, ids=["G%d-%s" % c for c in FAULT_CASES])
@pytest.mark.parametrize("fault", sorted(FAULTS), ids=["fault%d" % f for f in sorted(FAULTS)])
def test_seeded_faults_are_caught(emu_lib, fault, group, shape_name):
    """the same cases must tell a kernel with ONE seeded fault from the real one, in either instantiation and at the shipped shape: a
    suite that passes a broken kernel checks nothing"""
    simt_harness.emu_lib(lambda: child.build_fault(fault))
    _, jobs, wants = _edge_jobs(group, shape_name, fault=fault)
    caught = False
    for j, r, want in zip(jobs, child.run(jobs), wants):
        try:
            assert r["rc"] == 0 and r["status"] == 0
            gp.check(group, r["out"], want, j["label"])
        except AssertionError:
            caught = True
    assert caught, "no case tells fault %d (%s) from the real kernels (G%d, %s)" % (fault, FAULTS[fault], group, shape_name)
