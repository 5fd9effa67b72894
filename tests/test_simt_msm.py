"""The MSM device code, compiled for the HOST and run one thread per lane (tests/simt/emu_msm.cpp), against the oracle.

What runs here is the code the GPU runs: `k_msm_seg_accumulate` / `k_msm_seg_combine` in their four instantiations (G1 GLV, G1 plain,
G2 psi split on lane pairs, G2 plain), `k_glv_decompose` / `k_gls_decompose`, `k_bases_import` / `k_bases_endo` / `k_bases_endo_g2` /
`k_bases_subgroup_check`, `k_msm_accumulate<FpPolicy>` and `k_proj_export`, launched with the grid and block shapes of api_msm.hip.
Every expectation comes from the oracle (oracle/bls12_381_ref.py, oracle/c_oracle.py) and from the big-integer models of
tests/decomp_model.py, never from the library under test; points are compared as affine wire limbs, decompositions word for word.

The library is built with trapping bounds / shift checks and reads every input from a buffer that ends against inaccessible pages,
and it runs in a child process under a time limit (tests/simt_msm_child.py): an LDS index out of range, a read past a buffer or a
lane that waits for a partner for ever fails the test that caused it.

The rest of the large MSM runs on the host stage by stage, each stage on inputs of its own and against the models of
tests/msm_pipe_model.py: the integer front end -- `k_sort_*`, the fallback sort (`k_msm_digits`, `k_scan_*`, `k_msm_scatter`) and
`k_item_*` -- in tests/test_simt_msm_front.py (tests/simt/emu_msm_front.cpp); the point kernels behind it -- `k_msm_accumulate_g2pair`,
`k_msm_heavy`, the four `k_wsum_level_*` forms, `k_tree_sum*`, `k_shift_add_team`, `k_msm_combine_team` -- in
tests/test_simt_msm_points.py (this library), which also walks the whole bucket reduction by the schedule of csrc/msm_plan.h as
api_msm.hip `msm_reduce` does.  The launch decisions of `msm_device` are plain host code (csrc/msm_plan.h, tests/test_msm_plan.py).
NOT covered on the host: the streams, events and slot hand-over of `msm_device` and the DPP modifiers the emulation ignores;
tests/test_msm_pipeline_gpu.py covers both on the GPU with every bucket of every window filled.

That the tests bite was checked by seeding faults into the device headers one at a time: no carry in DigitIter::next
(test_signed_recoding_carries, test_window_sums), sub2 flipped in glv_split / a sign flipped in gls_split
(test_decompose_kernels_match_the_models, test_window_sums, test_fullest_lists), no `mz && pm` exit in the G2 walk
(test_exceptional_additions_in_one_bucket, G2), the G1 prefetch index unclamped (test_fullest_lists: bounds trap on `ent`), a list walk
from beg[a] + 1 (nearly all).  In the reduction tree `(b & d) == 0` for `(b & (2 * d - 1)) == 0` only changes lanes whose value never
reaches lane b = 0, the one that stores: no output can differ; `(b & (4 * d - 1)) == 0`, which does reach it, fails test_window_sums.

Cost on an 8-core machine, emulation libraries built from scratch in both runs: `pytest tests -q -m "not gpu"` took 206 s before this
file existed and 408 s with it (this file alone about 200 s, 21 s of them the build of the library; three quarters of the rest are the
two G2 configurations).  The counts below are sized for that: cut counts, G2 plain first, never a class of cases."""

import numpy as np
import pytest

import decomp_model
import simt_msm_child as child
import simt_harness
from msm_edge_values import boundary_values, carry_values
from oracle import bls12_381_ref as o
from oracle import c_oracle

SEG_CHUNK = 128                                                    # msm_seg.hip.h
SEG_LEN_MAX = 4096                                                 # limits.h
SEG_STATUS_BAD = 8
BYTES, MONT = 0, 1                                                 # scalar.hip.h SCALAR_BYTES / SCALAR_MONT
CONFIGS = [(1, 1), (1, 0), (2, 1), (2, 0)]                         # (group, split)
CONFIG_IDS = ["g1-glv", "g1-plain", "g2-gls", "g2-plain"]
RR = o.R_ORDER
X_ABS = decomp_model.X_ABS
LAMBDA = decomp_model.L


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    lib = simt_harness.emu_lib(child.build)
    c_oracle.build()
    return lib


# ---- points and scalars ------------------------------------------------------------------------------------------------------------
def _fpw(x):
    return np.array(o.fp_to_mont_limbs(x), dtype=np.uint64)


def _aff_wire(group, p):
    """oracle affine tuple -> wire limbs; the identity is (0, 1) with its flag set, as the reference stores it"""
    if group == 1:
        return np.concatenate([_fpw(p[0]), _fpw(p[1])])
    return np.concatenate([_fpw(p[0][0]), _fpw(p[0][1]), _fpw(p[1][0]), _fpw(p[1][1])])


def _ident_wire(group):
    return _aff_wire(group, o.G1_IDENTITY_AFF if group == 1 else o.G2_IDENTITY_AFF)


def _bytes(vals):
    return np.stack([np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint8) for v in vals]) if len(vals) else np.zeros((0, 32), np.uint8)


def _gen_multiples(group, exps):
    """[e mod r] G for every e by the C oracle's double-and-add: ((n, 12|24) affine wire limbs, (n,) identity flags)"""
    g = _aff_wire(group, o.G1_GEN if group == 1 else o.G2_GEN)
    if not len(exps):
        return np.zeros((0, len(g)), np.uint64), np.zeros(0, np.uint8)
    xy, inf = c_oracle.mul_batch_affine(group, np.tile(g, (len(exps), 1)), None, _bytes([int(e) % RR for e in exps]))
    return xy, inf


def _as_points(xy, inf):
    return [None if inf[i] else xy[i].tobytes() for i in range(len(inf))]


def _bases(group, ks):
    """the bases [k_i] G in wire form (k_i = 0: the identity with its flag)"""
    xy, inf = _gen_multiples(group, ks)
    xy = xy.copy()
    xy[inf != 0] = _ident_wire(group)
    return xy, inf


def _words(vals, form):
    """scalars as the kernels read them: 32 little-endian bytes, or the four Montgomery limbs of a `Scalar`"""
    if form == MONT:
        vals = [v * o.FR_MONT_R % RR for v in vals]
    return np.frombuffer(_bytes(vals).tobytes(), dtype=np.uint32).reshape(-1, 8)


def _affine(group, xyz):
    """projective wire limbs -> the oracle's affine limbs (None: the identity)"""
    out = []
    for row in np.asarray(xyz).reshape(-1, 18 if group == 1 else 36):
        xy, inf = (c_oracle.g1_to_affine if group == 1 else c_oracle.g2_to_affine)(row)
        out.append(None if inf else xy.tobytes())
    return out


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)


def _rand(n, seed):
    r = o.SplitMix64(seed)
    return [r.scalar() for _ in range(n)]


def _seg_exps(ks, ss, off, bf=None):
    out = []
    for j in range(len(off) - 1):
        f = int(off[j]) if bf is None else int(bf[j])
        out.append(sum(ks[f + i] * ss[int(off[j]) + i] for i in range(int(off[j + 1]) - int(off[j]))) % RR)
    return out


class Call:
    """the jobs of one child process: bases sets and segmented MSMs over them, each with what the oracle says it must give"""

    def __init__(self):
        self.jobs, self.checks = [], []

    def bases(self, group, ks, split):
        xy, inf = _bases(group, ks)
        return self.bases_wire(group, xy, inf, split)

    def bases_wire(self, group, xy, inf, split, check=False):
        self.jobs.append({"op": "bases", "label": "group %d, %d points" % (group, len(inf)), "group": group, "xy": xy, "inf": inf, "endo": bool(split), "check": check})
        return len(self.jobs) - 1

    def segments(self, label, group, split, bases, ks, ss, lens, bf=None, form=BYTES, batch=None, want=None, status=0):
        """segments over bases [k_i] G; `want` overrides the expected points (list of affine bytes / None)"""
        off = _offsets(lens)
        bf = None if bf is None else np.asarray(bf, dtype=np.uint32)
        self.jobs.append({"op": "segments", "label": label, "bases": bases, "split": split, "offsets": off, "scalars": _words(ss, form), "form": form,
                          "k": len(lens), "base_first": bf, "batch": batch})
        if want is None:
            want = _as_points(*_gen_multiples(group, _seg_exps(ks, ss, off, bf)))
        self.checks.append((len(self.jobs) - 1, label, group, want, status))
        return len(self.jobs) - 1

    def run(self, timeout=300):
        res = child.run(self.jobs, timeout)
        for i, label, group, want, status in self.checks:
            got = _affine(group, res[i]["out"])
            bad = [j for j in range(len(want)) if got[j] != want[j]]
            assert not bad, "%s: segments %s of %d differ from the oracle" % (label, bad[:8], len(want))
            assert res[i]["status"] == status, "%s: status word %d, expected %d" % (label, res[i]["status"], status)
        return res


# ---- segmented MSM: scalar edges -----------------------------------------------------------------------------------------------------
# Counts are emulation-sized: a segment of one scalar costs 1 (split), 2 (G1 plain) or 4 (G2 plain) workgroups of 256 host threads, and a
# G2 workgroup is several times dearer than a G1 one (every Fp2 product is lane-pair exchanges).  ALL values of a list always run in the
# one-segment form; as products of their own every OWN_STRIDE-th of them does.
CARRY_OWN_STRIDE = {(1, 1): 4, (1, 0): 8, (2, 1): 16, (2, 0): 32}
BOUNDARY_OWN_STRIDE = {(1, 1): 1, (1, 0): 2, (2, 1): 3, (2, 0): 8}


def _all_and_some(label, group, split, vals, stride, seed):
    """all values in one segment of several chunks, and every stride-th as a product of its own, over the same bases"""
    c = Call()
    n = len(vals)
    own = vals[::stride]
    ks = _rand(n, seed)
    b = c.bases(group, ks, split)
    c.segments(label + ", all in one segment", group, split, b, ks, vals, [n], bf=[0])
    c.segments(label + ", one per segment", group, split, b, ks[:len(own)], own, [1] * len(own))
    c.run()


@pytest.mark.parametrize("group,split", CONFIGS, ids=CONFIG_IDS)
def test_signed_recoding_carries(group, split):
    """2^(4m) - 1, - 8, - 9, + 0, + 1 and the all-8 / all-9 nibble runs for m = 1..63, nibbles 8 / 9 / F straddling bits 64, 128 and 192
    (where the workgroups of plain mode recompute the digits below their own), and [2^254, r) with top nibbles 4..7"""
    _all_and_some("carries", group, split, carry_values(), CARRY_OWN_STRIDE[(group, split)], 241 + group)


@pytest.mark.parametrize("group,split", CONFIGS, ids=CONFIG_IDS)
def test_decomposition_boundaries(group, split):
    """the branch values of the GLV (G1) / psi (G2) split of tests/decomp_model.py: all in one segment, and as products of their own"""
    _all_and_some("split boundaries", group, split, boundary_values(group), BOUNDARY_OWN_STRIDE[(group, split)], 231 + group)


# ---- segmented MSM: segment shapes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group,split", CONFIGS, ids=CONFIG_IDS)
def test_segment_lengths_and_batches(group, split):
    """lengths 0, 1, 2, SEG_CHUNK - 1, SEG_CHUNK, SEG_CHUNK + 1 and three chunks; an empty first and last segment; overlapping base_first;
    a batch smaller than k (seg0 > 0 in the later launches, the window-sum scratch reused)"""
    lens = [0, 1, 2, SEG_CHUNK - 1, SEG_CHUNK, SEG_CHUNK + 1, 2 * SEG_CHUNK + 5, 0]
    nb = 2 * SEG_CHUNK + 5
    ks = _rand(nb + 3, 401 + group)
    ss = _rand(sum(lens), 411 + group)
    c = Call()
    b = c.bases(group, ks, split)
    bf = [0, 0, 1, 2, 1, 0, 3, nb + 3]                              # overlapping ranges over one set; the last (empty) starts at its end
    c.segments("lengths, overlapping base_first, batch 3 of 8", group, split, b, ks, ss, lens, bf=bf, batch=3)
    # contiguous (base_first absent: bases follow the offsets) on the short ones
    lens2 = [0, 2, 1, 0]
    c.segments("contiguous, batch 3 of 4", group, split, b, ks, ss[:3], lens2, batch=3)
    c.run()


def _full_digit_scalars(group, split, n, seed):
    """n scalars whose every signed window digit is non-zero in every sub-scalar (all MAXENT entries of a chunk in play)"""
    r = o.SplitMix64(seed)

    def nibbles(count, top_max):
        v = 0
        for i in range(count):
            hi = top_max if i == count - 1 else 7
            v |= (1 + r.next() % hi) << (4 * i)
        return v

    out = []
    for _ in range(n):
        if not split:
            k = nibbles(64, 6)
            subs = [k]
        elif group == 1:
            k1, k2 = nibbles(32, 4), nibbles(32, 4)
            k = k1 + k2 * LAMBDA
            m = decomp_model.glv_model(k)
            assert (m[0], m[2]) == (k1, k2)
            subs = [k1, k2]
        else:
            d = [nibbles(16, 5) for _ in range(4)]
            k = sum(dj * X_ABS ** j for j, dj in enumerate(d))
            assert [t[0] for t in decomp_model.gls_model(k)] == d
            subs = d
        assert k < RR
        for s in subs:
            assert all(dg != 0 for dg in _recode(s, {1: 64, 2: 32, 4: 16}[len(subs)]))
        out.append(k)
    return out


def _recode(mag, nwin):
    """signed 4-bit digits in [-7, 8] of a magnitude, lowest window first (plain integers)"""
    d, carry = [], 0
    for w in range(nwin):
        raw = ((mag >> (4 * w)) & 15) + carry
        carry = 1 if raw > 8 else 0
        d.append(raw - 16 if raw > 8 else raw)
    assert carry == 0 and (mag >> (4 * nwin)) == 0
    return d


@pytest.mark.parametrize("group,split", CONFIGS, ids=CONFIG_IDS)
def test_fullest_lists(group, split):
    """(i) all scalars of a whole chunk equal: one (window, digit) list per window holds the whole chunk; (ii) every digit of every
    sub-scalar non-zero over a whole chunk: all MAXENT entries of `ent` in play, the last list ends at the array's end (where the
    G1 walk's prefetch of the next entry must stay inside); then a second, short chunk over the stale entries of the first"""
    c = Call()
    n = SEG_CHUNK + 3
    ks = _rand(n, 421 + group)
    b = c.bases(group, ks, split)
    s = _full_digit_scalars(group, split, 1, 431 + group)[0]
    c.segments("one list per window takes the whole chunk", group, split, b, ks, [s] * SEG_CHUNK, [SEG_CHUNK])
    ss = _full_digit_scalars(group, split, n, 441 + group)
    c.segments("every digit non-zero, chunk + 3", group, split, b, ks, ss, [n])
    c.run()


# ---- segmented MSM: exceptional additions inside one bucket ----------------------------------------------------------------------------
@pytest.mark.parametrize("group,split", CONFIGS, ids=CONFIG_IDS)
def test_exceptional_additions_in_one_bucket(group, split):
    """small scalars d put a base into bucket (window 0, d) alone, so the lists are chosen here: the same point twice and four times
    (doubling), P then -P and a further point, identity bases first / middle / last, lists of different length for the two accumulators
    of a quad's lane pairs (digits 1 and 2), and -- over three chunks, which fixes the order -- an accumulator that holds A + B when
    [a + b] G arrives (G2: the pair leaves the XYZZ loop for the complete addition and converts back), with a further point in the next
    chunk; likewise A + B followed by -(A + B) (back to the identity) and a further point"""
    a, bb, d, e = _rand(4, 451 + group)
    c = Call()
    # within one chunk (list order is the sort's)
    ks = [a, a, bb, 0, a, (RR - a) % RR, d, 0, e, a, a, a, a, 0]
    cases = [("same point twice", 0, [3, 3]),
             ("P, P, Q", 0, [3, 3, 3]),
             ("P, -P", 4, [5, 5]),
             ("P, -P, Q", 4, [5, 5, 5]),
             ("identity first", 3, [2, 2, 2]),
             ("identity in the middle", 6, [2, 2, 2]),
             ("identity last", 11, [4, 4, 4]),
             ("identity alone", 3, [6]),
             ("four times the same point", 9, [7, 7, 7, 7]),
             ("lists of 5 and 2 for digits 1 and 2", 4, [1, 2, 1, 1, 2, 1, 1]),
             ("P under 8 and -P under 8 + carry digits", 4, [8, 8 + 16 * 9]),
             ("everything, digits 1..8", 0, [1 + i % 8 for i in range(len(ks))])]
    b = c.bases(group, ks, split)
    ss = [v for _, _, s in cases for v in s]
    c.segments("one bucket, one chunk", group, split, b, ks, ss, [len(s) for _, _, s in cases], bf=[f for _, f, _ in cases])
    # over three chunks: chunk 0 holds A and B, chunk 1 the point that repeats / cancels their sum, chunk 2 a further point
    z = [0] * (SEG_CHUNK - 2)
    for label, third in (("A + B then [a + b] G", (a + bb) % RR), ("A + B then -[a + b] G", (-(a + bb)) % RR)):
        ks3 = [a, bb] + z + [third] + [0] * (SEG_CHUNK - 1) + [d, e]
        ss3 = [3, 3] + z + [3] + [0] * (SEG_CHUNK - 1) + [3, 2]
        b3 = c.bases(group, ks3, split)
        c.segments(label + ", then D", group, split, b3, ks3, ss3, [len(ks3)])
    res = c.run()
    got = _affine(group, res[1]["out"])
    assert got[2] is None and got[7] is None and got[0] is not None          # P - P and the identity alone: the identity


# ---- segmented MSM: plain mode over points outside the subgroup ------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 2])
def test_off_subgroup_points_plain_mode(kats, group):
    """the reference's own curve points outside the subgroup (test_is_torsion_free) among subgroup points: plain 256-bit windows are
    exact for every curve point -- against the C oracle's double-and-add + Sum"""
    F = o.fp_from_mont_limbs
    v = kats["tests"]["g1.test_is_torsion_free" if group == 1 else "g2.test_is_torsion_free"]["fp"]
    A = (F(v[0]), F(v[1]), False) if group == 1 else ((F(v[0]), F(v[1])), (F(v[2]), F(v[3])), False)
    ks = _rand(4, 461 + group)
    xy, inf = _bases(group, ks)
    xy = np.concatenate([xy[:2], _aff_wire(group, A)[None, :], xy[2:], _aff_wire(group, A)[None, :]])
    inf = np.zeros(6, dtype=np.uint8)
    ss = _rand(4, 471 + group) + [RR - 1, 3, 5, 5, 1 << 254]
    lens = [4, 2, 3]
    bf = [0, 4, 1]
    off = _offsets(lens)
    msm, toaff = (c_oracle.g1_msm, c_oracle.g1_to_affine) if group == 1 else (c_oracle.g2_msm, c_oracle.g2_to_affine)
    want = []
    for j in range(3):
        axy, ainf = toaff(msm(xy[bf[j]:bf[j] + lens[j]], inf[bf[j]:bf[j] + lens[j]], _bytes(ss[off[j]:off[j + 1]]))[0])
        want.append(None if ainf else axy.tobytes())
    c = Call()
    b = c.bases_wire(group, xy, inf, split=False)
    c.segments("off-subgroup points", group, 0, b, None, ss, lens, bf=bf, want=want)
    c.run()


# ---- segmented MSM: scalar forms and the contract ------------------------------------------------------------------------------------
@pytest.mark.parametrize("group,split", CONFIGS, ids=CONFIG_IDS)
def test_scalar_forms_and_contract(group, split):
    """Montgomery limbs give the points the bytes give; bytes / limbs >= r set status bit 0; offsets that decrease, a length above
    SEG_LEN_MAX, o1 > total and bases out of range each set SEG_STATUS_BAD, give the identity for that segment and leave the
    neighbours right"""
    n = 12
    ks = _rand(n, 481 + group)
    vals = boundary_values(group)[::9][:6] + carry_values()[::97][:6]
    c = Call()
    b = c.bases(group, ks, split)
    c.segments("bytes", group, split, b, ks, vals, [5, 7])
    c.segments("Montgomery limbs", group, split, b, ks, vals, [5, 7], form=MONT)
    good = _as_points(*_gen_multiples(group, _seg_exps(ks, vals, _offsets([4, 4, 4]))))
    # a scalar >= r: status bit 0 (the points are then unspecified); in each form
    for form, bads in ((BYTES, (RR, (1 << 256) - 1)), (MONT, (RR,))):
        for bad in bads:
            w = _words(vals, form).copy()
            w[5] = np.frombuffer(int(bad).to_bytes(32, "little"), dtype=np.uint32)
            c.jobs.append({"op": "segments", "label": "scalar >= r, form %d" % form, "bases": b, "split": split, "offsets": _offsets([4, 4, 4]), "scalars": w,
                           "form": form, "k": 3})
    first_bad = len(c.jobs) - 3
    # contract violations: the middle segment breaks it
    viol = [("offsets decrease", [0, 8, 4, 8], None, None, None),
            ("o1 > total", [0, 4, 13, 13], None, 12, None),
            ("bases out of range", [0, 4, 8, 12], [0, 9, 8], None, None),
            ("bases out of range (nbases short)", [0, 4, 8, 12], [0, 4, 0], None, 7)]
    vjobs = []
    for label, off, bf, total, nbases in viol:
        c.jobs.append({"op": "segments", "label": label, "bases": b, "split": split, "offsets": np.array(off, np.uint32), "scalars": _words(vals, BYTES), "form": BYTES,
                       "k": 3, "base_first": None if bf is None else np.array(bf, np.uint32), "total": total, "nbases": nbases})
        vjobs.append((len(c.jobs) - 1, label, off, bf))
    # a length above SEG_LEN_MAX: the scalars exist, so only the length is wrong
    long_s = np.zeros((SEG_LEN_MAX + 1 + 8, 8), dtype=np.uint32)
    long_s[:4] = _words(vals[:4], BYTES)
    long_s[-4:] = _words(vals[8:12], BYTES)
    c.jobs.append({"op": "segments", "label": "length above SEG_LEN_MAX", "bases": b, "split": split,
                   "offsets": np.array([0, 4, SEG_LEN_MAX + 5, SEG_LEN_MAX + 9], np.uint32), "scalars": long_s, "form": BYTES, "k": 3,
                   "base_first": np.array([0, 0, 8], np.uint32), "nbases": SEG_LEN_MAX + 1})
    vjobs.append((len(c.jobs) - 1, "length above SEG_LEN_MAX", None, None))
    res = c.run()
    for i in range(first_bad, first_bad + 3):
        assert res[i]["status"] & 1, c.jobs[i]["label"]
        got = _affine(group, res[i]["out"])
        assert got[0] == good[0] and got[2] == good[2], c.jobs[i]["label"]
    for i, label, off, bf in vjobs:
        assert res[i]["status"] == SEG_STATUS_BAD, label
        got = _affine(group, res[i]["out"])
        assert got[1] is None, label
        if label == "offsets decrease":
            want = _as_points(*_gen_multiples(group, [sum(ks[j] * vals[j] for j in range(8)), 0, sum(ks[4 + j] * vals[4 + j] for j in range(4))]))
        elif label == "o1 > total":
            want = [good[0], None, None]                             # the third segment is [13, 13): empty
        elif label == "bases out of range":
            want = [good[0], None, good[2]]
        elif label.startswith("bases out of range"):
            want = [good[0], None, _as_points(*_gen_multiples(group, [sum(ks[j] * vals[8 + j] for j in range(4))]))[0]]
        else:
            want = [good[0], None, good[2]]
        assert got == want, label


# ---- white box: the window sums ----------------------------------------------------------------------------------------------------------
def _sub_scalars(group, split, k):
    """[(magnitude, subtracted, multiplier of the base's discrete log)] of one scalar, from the models of decomp_model"""
    if not split:
        return [(k, 0, 1)]
    if group == 1:
        k1, neg1, k2, sub2, _ = decomp_model.glv_model(k)
        return [(k1, neg1, 1), (k2, sub2, (-LAMBDA) % RR)]          # phi(P) = -[L] P
    return [(m, s, pow(-X_ABS, j, RR)) for j, (m, s) in enumerate(decomp_model.gls_model(k))]     # psi^j(P) = [x^j] P


@pytest.mark.parametrize("group,split", CONFIGS, ids=CONFIG_IDS)
def test_window_sums(group, split):
    """every window sum of one segment equals sum_b b B_b recomputed from the digits of the models (so a wrong reduction tree cannot hide
    behind a Horner that happens to cancel it), over scalars that fill all eight buckets of the windows"""
    n = 40
    ks = _rand(n, 491 + group)
    ss = _rand(n - 8, 501 + group) + boundary_values(group)[-4:] + carry_values()[-4:]
    c = Call()
    b = c.bases(group, ks, split)
    j = c.segments("window sums", group, split, b, ks, ss, [n])
    res = c.run()
    nwin_sub = {(1, 1): 32, (1, 0): 64, (2, 1): 16, (2, 0): 64}[(group, split)]
    exps = [0] * nwin_sub
    for k, s in zip(ks, ss):
        for mag, sub, mult in _sub_scalars(group, split, s):
            for w, dg in enumerate(_recode(mag, nwin_sub)):
                exps[w] += (-dg if sub else dg) * mult * k
    want = _as_points(*_gen_multiples(group, exps))
    got = _affine(group, res[j]["wsums"][0])
    bad = [w for w in range(nwin_sub) if got[w] != want[w]]
    assert not bad, "window sums %s differ" % bad
    assert len({g for g in got}) > nwin_sub // 2


# ---- decomposition kernels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 2])
def test_decompose_kernels_match_the_models(group):
    """k_glv_decompose / k_gls_decompose word for word against decomp_model (itself pinned to big integers by
    test_scalar_decompositions_against_big_integers) on the candidate lists, the carry values and seeded uniform scalars, bytes and limbs"""
    vals = boundary_values(group) + carry_values() + _rand(300, 511 + group)
    n = len(vals)
    want = np.zeros(n * 8, dtype=np.uint32)
    for i, k in enumerate(vals):
        if group == 1:
            k1, neg1, k2, sub2, _ = decomp_model.glv_model(k)
            a, bq = k1 | (neg1 << 127), k2 | (sub2 << 127)
            want[4 * i:4 * i + 4] = np.frombuffer(a.to_bytes(16, "little"), dtype=np.uint32)
            want[4 * n + 4 * i:4 * n + 4 * i + 4] = np.frombuffer(bq.to_bytes(16, "little"), dtype=np.uint32)
        else:
            for j, (m, s) in enumerate(decomp_model.gls_model(k)):
                want[8 * i + 2 * j:8 * i + 2 * j + 2] = np.frombuffer((m | (s << 63)).to_bytes(8, "little"), dtype=np.uint32)
    jobs = [{"op": "decompose", "label": "form %d" % f, "group": group, "scalars": _words(vals, f), "form": f} for f in (BYTES, MONT)]
    bad = _words(vals[:3], BYTES).copy()
    bad[1] = np.frombuffer(int(RR).to_bytes(32, "little"), dtype=np.uint32)
    jobs.append({"op": "decompose", "label": "scalar >= r", "group": group, "scalars": bad, "form": BYTES})
    res = child.run(jobs)
    for f in (0, 1):
        assert res[f]["status"] == 0
        diff = np.nonzero(res[f]["out"] != want)[0]
        assert diff.size == 0, "form %d: word %d differs (scalar %s)" % (f, diff[0], hex(vals[(diff[0] % (4 * n)) // 4 if group == 1 else diff[0] // 8]))
    assert res[2]["status"] == 1


# ---- bases: images and subgroup check ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 2])
def test_endomorphism_images(group):
    """k_bases_endo: (BETA x, y); k_bases_endo_g2: P, psi(P), psi^2(P), psi^3(P) interleaved -- equal to the records k_bases_import makes
    of the oracle's images; identity flag carried"""
    ks = _rand(5, 521 + group) + [0]
    xy, inf = _bases(group, ks)
    pts = []
    for i in range(6):
        F = o.fp_from_mont_limbs
        w = [F(xy[i][6 * t:6 * t + 6]) for t in range(len(xy[i]) // 6)]
        pts.append((w[0], w[1]) if group == 1 else ((w[0], w[1]), (w[2], w[3])))
    if group == 1:
        img = [[(o.fp_mul(o.BETA, p[0]), p[1])] for p in pts]
    else:
        def psi(p):
            q = o.g2_psi((p[0], p[1], o.FP2_ONE))
            return (q[0], q[1])
        img = []
        for p in pts:
            p1 = psi(p); p2 = psi(p1); p3 = psi(p2)
            img.append([p, p1, p2, p3])
    m = len(img[0])
    ixy = np.stack([_aff_wire(group, (q[0], q[1], False)) for im in img for q in im])
    iinf = np.repeat(inf, m)
    jobs = [{"op": "bases", "label": "points", "group": group, "xy": xy, "inf": inf, "endo": True},
            {"op": "bases", "label": "the oracle's images", "group": group, "xy": ixy, "inf": iinf}]
    res = child.run(jobs)
    aw = child.AFF_WORDS[group]
    got, want = res[0]["endo"].reshape(-1, aw), res[1]["rec"].reshape(-1, aw)
    assert np.array_equal(got[:5 * m], want[:5 * m])
    flags = got[:, aw - (4 if group == 1 else 8)]
    assert list(flags) == [0] * (5 * m) + [1] * m
    # the images of the identity carry its flag; no kernel reads their coordinates (the flag is tested first), and they are not compared:
    # k_bases_endo_g2 stores y.c1 of psi^2(identity) as p, not 0 -- canon() maps the value 2p, which only the negation of an exact 0
    # produces, to p


@pytest.mark.parametrize("group", [1, 2])
def test_subgroup_check_counts(kats, group):
    """k_bases_subgroup_check counts exactly the records that are off the subgroup or off the curve; identities and subgroup points pass"""
    F = o.fp_from_mont_limbs
    v = kats["tests"]["g1.test_is_torsion_free" if group == 1 else "g2.test_is_torsion_free"]["fp"]
    A = (F(v[0]), F(v[1]), False) if group == 1 else ((F(v[0]), F(v[1])), (F(v[2]), F(v[3])), False)
    assert (o.g1_is_on_curve if group == 1 else o.g2_is_on_curve)(A) and not (o.g1_is_torsion_free if group == 1 else o.g2_is_torsion_free)(A)
    ks = _rand(3, 531 + group) + [0]
    xy, inf = _bases(group, ks)
    off_curve = xy[1].copy()
    off_curve[0] ^= 2                                                # x changed: not on the curve
    mixed = np.stack([xy[0], _aff_wire(group, A), xy[1], off_curve, xy[3], xy[2], _aff_wire(group, A)])
    minf = np.array([0, 0, 0, 0, 1, 0, 0], dtype=np.uint8)
    jobs = [{"op": "bases", "label": "subgroup points and an identity", "group": group, "xy": xy, "inf": inf, "check": True},
            {"op": "bases", "label": "mixed set", "group": group, "xy": mixed, "inf": minf, "check": True}]
    res = child.run(jobs)
    assert res[0]["nbad"] == 0
    assert res[1]["nbad"] == 3


# ---- k_msm_accumulate<FpPolicy> on hand-built item lists -------------------------------------------------------------------------------
def test_g1_bucket_accumulation_items():
    """items of length 0, 1, 2 and long; the LAST item ends at the last word of `sorted` and its last entry names the last record of
    `bases2` (another: of `bases`) -- the clamped unconditional prefetches against the guard pages; entries on both sides of nsplit,
    negated entries, identity records, doubling and cancellation inside an item; each record against the oracle's sum"""
    ks = _rand(10, 541)
    ID = 8
    ks[ID] = 0                                                       # an identity record
    ks[4] = ks[3]                                                    # a repeated point
    ks[5] = (RR - ks[3]) % RR                                        # and its negative
    n = len(ks)
    NEG = 1 << 31
    E = lambda i: n + i                                              # the image of base i (bases2)
    lists = [[],
             [2],
             [0, 1 | NEG],
             [3, 4, 6],                                              # doubling, then a further point
             [3, 5, 7],                                              # cancellation, then a further point
             [3, 3 | NEG],                                           # cancellation through the sign bit
             [ID, 1, ID, 2, ID],                                     # identity records first / middle / last
             [E(0), 1, E(2) | NEG, E(ID), 9],
             [i % n if i % 3 else E(i % n) | (NEG if i % 2 else 0) for i in range(70)],
             [0, n - 1],                                             # ends with the last record of `bases`
             [0, E(1), E(n - 1) | NEG, E(n - 2)],
             [5, E(n - 1)]]                                          # the last word of `sorted` names the last record of `bases2`
    sorted_, items = [], []
    for d, l in enumerate(lists):
        items.append((len(sorted_), len(l), len(lists) - 1 - d))    # records written in reverse order: dest is the item's own field
        sorted_ += l
    ctrl = [0, 0, len(items), 0]

    def dlog(e):
        i = e & (NEG - 1)
        v = ks[i] if i < n else ks[i - n] * (-LAMBDA) % RR
        return -v if e & NEG else v

    want = _as_points(*_gen_multiples(1, [sum(dlog(e) for e in l) for l in lists]))
    xy, inf = _bases(1, ks)
    jobs = [{"op": "bases", "label": "bases", "group": 1, "xy": xy, "inf": inf, "endo": True},
            {"op": "accumulate", "label": "items", "bases": 0, "nsplit": n, "bases2_endo": True, "sorted": np.array(sorted_, dtype=np.uint32),
             "items": np.array(items, dtype=np.uint32), "ctrl": np.array(ctrl, dtype=np.uint32), "max_items": len(items), "ndest": len(items)},
            # more lanes than items (ctrl[2] decides), no second array
            {"op": "accumulate", "label": "no second array", "bases": 0, "nsplit": 0xFFFFFFFF, "sorted": np.array([1, 2 | NEG, n - 1, n - 2], dtype=np.uint32),
             "items": np.array([(0, 4, 0)], dtype=np.uint32), "ctrl": np.array([0, 0, 1, 0], dtype=np.uint32), "max_items": 300, "ndest": 1}]
    res = child.run(jobs)
    got = _affine(1, res[1]["records"])
    for d, l in enumerate(lists):
        assert got[len(lists) - 1 - d] == want[d], "item %d %s" % (d, [hex(e) for e in l[:6]])
    assert want[0] is None and want[5] is None
    assert _affine(1, res[2]["records"])[0] == _as_points(*_gen_multiples(1, [ks[1] - ks[2] + ks[n - 1] + ks[n - 2]]))[0]
