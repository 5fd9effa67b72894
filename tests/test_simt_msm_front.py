"""The integer front end of the large MSM -- the two-level counting sort (`k_sort_hist`, `k_sort_scan`, `k_sort_scatter`, `k_sort_fine`),
the fallback sort (`k_msm_digits`, `k_scan_block_sums`, `k_scan_top`, `k_scan_apply`, `k_msm_scatter`) and the work-item kernels
(`k_item_count`, `k_item_scan`, `k_item_fill`) -- compiled for the HOST (tests/simt/emu_msm_front.cpp) and checked ONE STAGE AT A TIME
against the plain-Python models of tests/msm_pipe_model.py.  The stages are not chained: each gets inputs built for it, at sizes of
a few workgroups; the driver logic of api_msm.hip is left to the GPU suite (tests/test_msm_pipeline_gpu.py, tests/test_gpu_parity.py).

Why on the host: DevBuf::reserve (host.h) allocates `bytes + bytes / 8 + 256`, so on the GPU a kernel that writes a few entries past
`total * 4`, past `max_items` or past the heavy list lands in slack and changes nothing, and an index past an LDS histogram bumps a
neighbouring counter nobody may look at.  Here every buffer has exactly the size api_msm.hip computes for it and ends against an
inaccessible page, and the library is built with trapping bounds / shift checks (tests/simt_msm_front_child.py).

Known limits: the emulated dynamic LDS is a fixed array, so a launch that asks for too few LDS bytes is not caught here.  The lanes of
a workgroup run as fibers of one thread in ascending lane order (tests/simt/emu_msm_front.cpp), so a MISSING barrier whose producer is
the lower-numbered lane cannot show here.  The point kernels behind the sort have a module of their own: tests/test_simt_msm_points.py.

That the tests bite was checked by seeding faults into msm.hip.h on a scratch copy, one at a time:
  `(mag - 1) >> fine_bits` -> `mag >> fine_bits` in k_sort_scatter only   every test_fast_sort_* case (an LDS index past the table
                                                                          traps, or a bucket holds its neighbour's entries)
  `rem[k] || !full[k]` -> `rem[k]` in k_item_fill                         test_items (an empty bucket loses its item: ctrl[2] and the
                                                                          tiling differ)
  `nitems > HEAVY_SMALL` -> `>=` in k_item_fill                           test_items (the load 16 * cap is listed as block-folded)
  coarse_out written at `lbase[ci] + r + 1`                               every test_fast_sort_* case (the write past `total * 4`
                                                                          hits the guard page, or a region's first slot stays unset)
The three seeded faults of the point kernels are listed in tests/test_simt_msm_points.py.

Cost: this file about 30 s where tests/test_simt_msm.py takes 170 s (one run on one machine), 4 s of them the build of the library; the
lanes run as fibers of one thread, not as threads (emu_msm_front.cpp says why).
"""
import numpy as np
import pytest

import msm_pipe_model as mm
import simt_harness
import simt_msm_front_child as child
from msm_edge_values import carry_values
from oracle import bls12_381_ref as o

RR = o.R_ORDER
TILE = mm.SORT_TILE


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    return simt_harness.emu_lib(child.build)


def test_model_restates_the_product_constants():
    k = child.run([{"op": "consts", "label": "constants"}])[0]
    assert (k["SORT_TILE"], k["SORT_MAX_COUNTERS"], k["ITEM_CAP_MAX"], k["ITEM_BLOCK_BUCKETS"], k["HEAVY_SMALL"], k["HEAVY_BIG_BLOCKS"]) == \
           (mm.SORT_TILE, mm.SORT_MAX_COUNTERS, mm.ITEM_CAP_MAX, mm.ITEM_BLOCK_BUCKETS, mm.HEAVY_SMALL, mm.HEAVY_BIG_BLOCKS)
    assert k["ITEM_BINS"] == mm.ITEM_CAP_MAX + 1


def test_no_accepted_window_exceeds_the_counter_table():
    """msm_plan.h msm_shape refuses nc > SORT_MAX_COUNTERS, but no window blsgpu_set_msm_window (4..16) or blsgpu_bases_precompute
    (9..21) accepts gets there: the largest unmerged table is 29 x 256 = 7424 counters (plain scalars, c = 9), the largest merged one
    8192 (c = 21).  A later change of the window limits trips this."""
    t = mm.counter_tables()
    assert max(t.values()) <= mm.SORT_MAX_COUNTERS
    assert t[(8, 9, False)] == 7424 == max(v for (w, c, m), v in t.items() if not m)
    assert t[(8, 21, True)] == 8192 == max(v for (w, c, m), v in t.items() if m)


def test_level_sums_model_is_the_window_sum():
    for n in (1, 2, 4, 8, 16, 64, 2048, 32768):
        want, got = mm.window_sum([(7 * b + 3) % 11 for b in range(n)])
        assert want == got


# ---- scalars ---------------------------------------------------------------------------------------------------------------------
def _rand(words, ns, seed):
    """uniform stored sort scalars: canonical scalars (8 words), 127-bit halves / 63-bit digits with a random sign bit"""
    r = o.SplitMix64(seed)
    if words == 8:
        return [r.scalar() for _ in range(ns)]
    bits = 32 * words
    return [((r.next() | (r.next() << 64)) & ((1 << (bits - 1)) - 1)) | ((r.next() & 1) << (bits - 1)) for _ in range(ns)]


def _families(words, c, seed):
    """name -> stored sort scalars: all zero, all equal, the recoding's carry chains, raw digits of exactly 2^(c-1) and 2^(c-1) + 1 in
    every window, uniform; 8 words only: values in [r, 2^256)"""
    bits = 32 * words
    mag_bits = 254 if words == 8 else bits - 1
    clip = lambda v, i: (v & ((1 << mag_bits) - 1)) | (0 if words == 8 else (i & 1) << (bits - 1))
    nbw = 1 << (c - 1)
    rep = lambda d: sum(d << (c * w) for w in range(mag_bits // c + 1))
    fam = {"zero": [0] * 70, "equal": [clip(_rand(words, 1, seed)[0], 1)] * 300,
           "carry": [clip(v, i) for i, v in enumerate(carry_values())],
           "nbw": [clip(rep(nbw), 0), clip(rep(nbw), 1), clip(rep(nbw + 1), 0), clip(rep(nbw + 1), 1), clip(rep(nbw) + 1, 0), clip(rep(nbw - 1), 1)] * 3,
           "uniform": _rand(words, 333, seed + 1)}
    if words == 8:
        r = o.SplitMix64(seed + 2)
        fam["noncanonical"] = [RR, RR + 1, (1 << 256) - 1, 1 << 255, (1 << 256) - (1 << 200), 5, RR - 1] + \
                              [RR + (r.next() | (r.next() << 64) | (r.next() << 128) | (r.next() << 192)) % ((1 << 256) - RR) for _ in range(40)]
    return fam


# ---- A1 / A2: the sorts ------------------------------------------------------------------------------------------------------------
def _sort_job(op, values, c, words=8, merged=0, stride=0, label=""):
    return {"op": op, "label": "%s %s words=%d c=%d ns=%d merged=%d" % (op, label, words, c, len(values), merged), "words": words, "values": values, "c": c,
            "nwin": mm.nwin_of(c, words), "merged": merged, "stride": stride}


def _check_sort(j, res):
    """offs = the exclusive prefix of the model's bucket loads, every bucket's slice of `sorted` = the model's entries as a multiset (the
    order inside a bucket is unspecified), nothing written behind the last entry; the status bit exactly for values >= r"""
    what = j["label"]
    buckets = mm.bucket_entries(j["values"], j["c"], j["nwin"], j["words"], bool(j["merged"]), j["stride"])
    offs = mm.offsets(buckets)
    assert res["offs"].tolist() == offs, what
    srt = res["sorted"]
    got = srt[:offs[-1]].tolist()
    for b, want in enumerate(buckets):
        if sorted(got[offs[b]:offs[b + 1]]) != sorted(want):
            pytest.fail("%s: bucket %d holds %r, the model %r" % (what, b, sorted(got[offs[b]:offs[b + 1]])[:8], sorted(want)[:8]))
    assert (srt[offs[-1]:] == 0xffffffff).all(), what
    assert res["status"] == (1 if j["words"] == 8 and any(v >= RR for v in j["values"]) else 0), what
    if j["op"] == "fast":
        assert res["hist_zero"], what + ": the sort left counters behind for the next call"
        assert res["ctrl_zero"], what + ": the item-control words are not cleared"


def _run_sorts(jobs):
    for j, res in zip(jobs, child.run(jobs)):
        _check_sort(j, res)


FAST_WORDS = {2: 4, 4: 2, 8: 4, 9: 8, 10: 2, 13: 4, 16: 8}        # c -> words per sort scalar: c = 9 on plain scalars is the largest unmerged counter table


@pytest.mark.parametrize("c", sorted(FAST_WORDS))
def test_fast_sort_tile_edges(c):
    """ns around the tile of k_sort_hist / k_sort_scatter, at the windows where the key split changes: c = 2, 4 (no fine bits), 8, 9
    (coarse key of 7 and 8 bits), 10, 13, 16 (7 fine bits).  The jobs of one child share the sort state, as the calls of one slot do."""
    words = FAST_WORDS[c]
    _run_sorts([_sort_job("fast", _rand(words, ns, 100 * c + i), c, words, label="tile") for i, ns in enumerate((1, TILE - 1, TILE, TILE + 1, 2 * TILE + 37))])


@pytest.mark.parametrize("words,c", [(8, 4), (8, 9), (8, 16), (4, 13), (4, 5), (2, 8), (2, 16)])
def test_fast_sort_scalar_families(words, c):
    _run_sorts([_sort_job("fast", v, c, words, label=name) for name, v in _families(words, c, 7 * c + words).items()])


@pytest.mark.parametrize("c", [9, 12, 20, 21])
def test_fast_sort_merged_windows(c):
    """resident window-shifted tables: ONE bucket set, the entry index = w * stride + i; c = 21 fills the counter table
    (ncoarse = 8192 = SORT_MAX_COUNTERS)"""
    fam = _families(8, c, 50 + c)
    jobs = [_sort_job("fast", fam["uniform"], c, 8, 1, 333, "merged"), _sort_job("fast", fam["nbw"], c, 8, 1, 4099, "merged nbw"),
            _sort_job("fast", fam["carry"][::3], c, 8, 1, 1 << 19, "merged carry"), _sort_job("fast", fam["noncanonical"], c, 8, 1, 47, "merged noncanonical"),
            _sort_job("fast", fam["zero"], c, 8, 1, 70, "merged zero"), _sort_job("fast", fam["equal"], c, 8, 1, 300, "merged equal")]
    if c == 12:
        jobs.append(_sort_job("fast", _rand(8, TILE + 1, 12), c, 8, 1, TILE + 1, "merged tile edge"))
    _run_sorts(jobs)


def test_fast_sort_state_between_calls():
    """two different sorts on the same ghist / gbase / gcur / ctrl, the second with the smaller counter table (29 x 256, then 16 x 8),
    then an all-zero input and the first again: the counters are zero and ctrl is clear after each (asserted in _check_sort)"""
    a, b = _rand(8, 700, 1), _rand(2, 900, 2)
    _run_sorts([_sort_job("fast", a, 9, 8, label="first"), _sort_job("fast", b, 4, 2, label="second"), _sort_job("fast", [0] * 5, 13, 4, label="zeros"),
            _sort_job("fast", a, 9, 8, label="first again")])


@pytest.mark.parametrize("c", [4, 7, 11])
def test_fallback_sort(c):
    """nb below, not a multiple of and a multiple of the 1024 buckets of a scan block: 512, 37 x 64 = 2368, 24 x 1024"""
    jobs = [_sort_job("fallback", v, c, label=name) for name, v in _families(8, c, 900 + c).items()]
    jobs += [_sort_job("fallback", _rand(8, n, 31 * c + n), c, label="n") for n in (1, 255, 256, 257, 1100)]
    _run_sorts(jobs)


# ---- A3: work items ---------------------------------------------------------------------------------------------------------------
def _special_loads(cap):
    return [0, 1, cap - 1, cap, cap + 1, 2 * cap, 2 * cap + 1, 16 * cap, 16 * cap + 1, 17 * cap]


def _check_items(offs, cap, res):
    nb = len(offs) - 1
    parts = mm.item_partition(offs, cap)
    ctrl, items, heavy, big = res["ctrl"], res["items"].tolist(), res["heavy"].tolist(), res["big"].tolist()
    assert ctrl[2] == sum(len(p) for p in parts) == len(items)
    assert res["rest_untouched"]
    lens = [it[1] for it in items]
    assert all(x >= y for x, y in zip(lens, lens[1:])), "item lengths must not increase"
    by_dest = {it[2]: (it[0], it[1]) for it in items}
    assert len(by_dest) == len(items), "two items share a record"
    cut = {b: p for b, p in enumerate(parts) if len(p) > 1}
    assert ctrl[1] == len(cut) == len(heavy) and ctrl[0] == sum(len(p) for p in cut.values())
    assert sorted(h[0] for h in heavy) == sorted(cut), "every cut bucket once in the heavy list"
    used = []
    for b, dest0, nitems, _ in heavy:
        assert nitems == len(cut[b]) and nb <= dest0 and dest0 + nitems <= nb + ctrl[0]
        assert sorted(by_dest[dest0 + j] for j in range(nitems)) == sorted(cut[b]), "the items of bucket %d do not tile it" % b
        used += range(dest0, dest0 + nitems)
    assert len(set(used)) == len(used), "partial records overlap"
    for b, p in enumerate(parts):
        if len(p) == 1:
            assert by_dest.get(b) == p[0], "bucket %d" % b          # an empty bucket keeps one item of length 0
    assert sorted(big) == sorted(h for h, e in enumerate(heavy) if e[2] > mm.HEAVY_SMALL) and ctrl[3] == len(big)


@pytest.mark.parametrize("cap", [16, 128, 4096])
def test_items(cap):
    """hand-built offsets with the loads at the edges of the cut (cap - 1, cap, cap + 1, 2 cap, 2 cap + 1) and of the fold (16 and 17
    partials), in a single bucket, and first, last and across the edge of a 2048-bucket block for nb = 2047, 2048, 2049"""
    special = _special_loads(cap)
    cases = [[L] for L in special]
    r = o.SplitMix64(cap)
    for nb in (2047, 2048, 2049):
        loads = [r.next() % 4 for _ in range(nb)]
        loads[:10] = special[::-1]
        loads[nb - 10:] = special                                   # nb = 2049: 16 cap + 1 ends block 0, 17 cap is alone in block 1
        loads[1019:1029] = special[::-1]                            # thread 251 .. 255 of round 3, 0 .. 4 of round 4
        cases.append(loads)
    cases.append([0] * 300)
    cases.append([cap] * 40 + [16 * cap] * 3 + [17 * cap] * 3)
    offs = [np.concatenate([[0], np.cumsum(l)]).astype(np.int64).tolist() for l in cases]
    jobs = [{"op": "items", "label": "cap=%d nb=%d" % (cap, len(f) - 1), "offs": f, "cap": cap} for f in offs]
    for f, res in zip(offs, child.run(jobs)):
        _check_items(f, cap, res)
