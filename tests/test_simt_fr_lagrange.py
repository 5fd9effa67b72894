"""The Lagrange-coefficient kernel (bls12_381_amd/csrc/fr_lagrange.hip.h) on the host: compiled for the CPU through tests/simt_harness.py /
tests/simt/emu_harness.h, one thread per lane, launched from the plan of csrc/fr_lagrange_plan.h exactly as api_fr.hip launches it, in
BOTH shapes, at a tiny shape (teams of 4 lanes, an LDS tile of 4 nodes, 2 nodes per lane and pass) and at the shipped ones.  Every
expectation is the formula of tests/fr_lagrange_ref.py in Python integers, compared limb for limb.

One call mixes segments of 0, 1, 2, 3, tile - 1, tile, tile + 1, 2 block + 1 and 3 tiles + 1 nodes, empty segments first and last, and
at every length: z = 0 explicitly, z on the first, a middle and the last node, a node equal to 0 with z = 0, a repeated node adjacent,
at the two ends of the segment and a tile apart, z on a repeated node, small participant ids.  The same call runs with points == NULL,
with and without values, and without lambda.  The device form's bad segments (decreasing offsets, 4097 nodes, an end beyond total) each
raise the status bit, touch nothing -- the arrays end against inaccessible pages -- and leave their neighbours right.  Five seeded
faults (-DFLG_FAULT=n) must each be told from the real kernel.  At the shipped shapes the longest segment is 2 block + 1 nodes."""
import functools

import numpy as np
import pytest

import fr_lagrange_ref as ref
import simt_fr_lagrange_child as child
import simt_harness

# (block, team, tile, r): one team of 4 lanes per workgroup / two teams of 4 lanes in a workgroup of 8
SHAPES = {"tiny block": (4, 4, 4, 2), "tiny wave": (8, 4, 4, 2), "shipped block": None, "shipped wave": None}
WHICH = {"tiny block": 0, "tiny wave": 0, "shipped block": 1, "shipped wave": 2}
# tile and block the edge lengths are built around (shipped wave: the team of 64 lanes is its own tile)
TILE_BLOCK = {"tiny block": (4, 4), "tiny wave": (4, 4), "shipped block": (512, 256), "shipped wave": (64, 64)}


@pytest.fixture(scope="module")
def emu_lib():
    return simt_harness.emu_lib(child.build)


def _lengths(shape_name):
    tile, block = TILE_BLOCK[shape_name]
    ls = [0, 1, 2, 3, tile - 1, tile, tile + 1, 2 * block + 1]
    if shape_name.startswith("tiny") or shape_name == "shipped wave":
        ls.append(3 * tile + 1)                                    # (shipped block: 3 * 512 + 1 is beyond the 2 block + 1 the emulation keeps to)
    return sorted(set(ls))


@functools.lru_cache(maxsize=None)
def _edge(shape_name):
    """the edge call of this shape, packed, and the formula's results with the call's points and with every z = 0 (computed once)"""
    tile, _ = TILE_BLOCK[shape_name]
    segs = ref.edge_segments(_lengths(shape_name), tile, seed=11)
    return segs, ref.pack(segs), ref.expected(segs), ref.expected(segs, zero_points=True)


def _job(shape_name, label, nodes, off, points, values, fault=0, **kw):
    return dict({"op": "lagrange", "label": "%s %s" % (shape_name, label), "nodes": nodes, "offsets": off, "points": points, "values": values,
                 "which": WHICH[shape_name], "shape": SHAPES[shape_name], "fault": fault}, **kw)


def _edge_jobs(shape_name, fault=0):
    """the edge call in its four forms -> [(job, (lam, y, flags) expected, None where the output is absent)]"""
    segs, (nodes, off, points, values), (lam, y, fl), (lam0, y0, fl0) = _edge(shape_name)
    return [(_job(shape_name, "lambda + y", nodes, off, points, values, fault, want_y=True), (lam, y, fl)),
            (_job(shape_name, "points == NULL", nodes, off, None, values, fault, want_y=True), (lam0, y0, fl0)),
            (_job(shape_name, "no values", nodes, off, points, None, fault), (lam, None, fl)),
            (_job(shape_name, "lambda == NULL", nodes, off, points, values, fault, want_lambda=False, want_y=True), (None, y, fl))]


def _check(r, want, label, segs=None):
    assert r["rc"] == 0 and r["status"] == 0, label
    for name, got, exp in zip(("lambda", "y", "flags"), (r["lam"], r["y"], r["flags"]), want):
        if exp is None:
            assert got is None, (label, name)
            continue
        if not np.array_equal(got, exp):
            bad = np.nonzero((got != exp).reshape(got.shape[0], -1).any(axis=1))[0]
            where = ""
            if segs is not None and name != "lambda":
                where = " segments: " + ", ".join(segs[int(k)][0] for k in bad[:6])
            raise AssertionError("%s: %s differs from the formula at %d entries (first %d)%s" % (label, name, len(bad), int(bad[0]), where))


@pytest.mark.parametrize("shape_name", sorted(SHAPES))
def test_edge_call_vs_formula(emu_lib, shape_name):
    segs = _edge(shape_name)[0]
    pairs = _edge_jobs(shape_name)
    for (j, want), r in zip(pairs, child.run([j for j, _ in pairs])):
        _check(r, want, j["label"], segs)
        assert (r["plan"]["tile"], r["plan"]["team"]) == (TILE_BLOCK[shape_name][0], TILE_BLOCK[shape_name][1] if "wave" in shape_name else r["plan"]["block"]), j["label"]
    # what the cases are meant to reach
    lam, _, fl = _edge(shape_name)[2]
    assert fl.min() == 0 and fl.max() == 1


def test_the_formula_has_the_properties_the_header_states():
    """the reference itself: one node gives 1 for every z, z on a node gives the unit vector, a repeated node gives 0 at exactly the
    repeated positions, z on a repeated node gives 0 everywhere, and distinct nodes interpolate a polynomial"""
    import random
    rng = random.Random(3)
    x = [rng.randrange(ref.R) for _ in range(7)]
    assert ref.lagrange([x[0]], 5) == ([1], 1) and ref.lagrange([x[0]], x[0]) == ([1], 1) and ref.lagrange([], 9) == ([], 1)
    assert ref.lagrange(x, x[3]) == ([0, 0, 0, 1, 0, 0, 0], 1)
    rep = x[:6] + [x[2]]
    lam, d = ref.lagrange(rep, 12345)
    assert d == 0 and lam[2] == 0 and lam[6] == 0 and all(lam[i] for i in (0, 1, 3, 4, 5))
    assert ref.lagrange(rep, x[2]) == ([0] * 7, 0)
    coef = [rng.randrange(ref.R) for _ in range(7)]
    f = lambda v: sum(c * pow(v, k, ref.R) for k, c in enumerate(coef)) % ref.R
    assert ref.interpolate(ref.lagrange(x, 0)[0], [f(v) for v in x]) == coef[0]
    assert ref.from_limbs(ref.to_limbs(x)) == x


def test_the_plan_the_emulation_walks_is_the_shipped_one(emu_lib):
    r = child.run([{"op": "plan", "label": "block", "nseg": 2048, "total": 2048 * 512}, {"op": "plan", "label": "wave", "nseg": 1 << 16, "total": 8 << 16, "want_lambda": False},
                   {"op": "plan", "label": "wave 40", "nseg": 100, "total": 4000}, {"op": "plan", "label": "forced wave", "nseg": 8, "total": 8 * 513, "which": 2},
                   {"op": "plan", "label": "tiny", "nseg": 9, "total": 50, "shape": SHAPES["tiny wave"]}])
    assert (r[0]["shape"], r[0]["block"], r[0]["team"], r[0]["tile"], r[0]["r"], r[0]["grid"]) == (1, 256, 256, 512, 4, 2048)
    assert r[0]["lds"] == (512 * 8 + 512 * 8 + 512) * 4 and r[0]["pre_bytes"] == 2048 * 512 * 32 and r[0]["work_bytes"] == 0
    assert (r[1]["shape"], r[1]["team"], r[1]["tile"], r[1]["teams"], r[1]["grid"]) == (2, 8, 8, 32, 2048) and r[1]["work_bytes"] == r[1]["pre_bytes"] == (8 << 16) * 32
    assert (r[2]["shape"], r[2]["team"], r[2]["grid"]) == (2, 64, 25)
    assert (r[3]["shape"], r[3]["team"], r[3]["tile"], r[3]["grid"]) == (2, 64, 64, 2)
    assert (r[4]["shape"], r[4]["teams"], r[4]["grid"], r[4]["lds"]) == (2, 2, 5, 2 * (4 * 8 + 8 * 8 + 8) * 4)


@pytest.mark.parametrize("shape_name", ["tiny block", "tiny wave", "shipped wave"])
def test_bad_segments_raise_the_bit_and_touch_nothing(emu_lib, shape_name):
    """offsets only the device can see: segment 1 decreases, segment 2 has 4097 nodes, segment 4 ends beyond total and segment 5 begins
    there.  Segments 0 and 3 are right; no other entry of any output is written; nothing outside the arrays is read (guard pages)."""
    import random
    rng = random.Random(21)
    total = 4097 + 30
    ints = rng.sample(range(1, 1 << 62), total)
    vals = [rng.randrange(ref.R) for _ in range(total)]
    off = np.array([0, 6, 4, 4101, 4110, total + 3, total], dtype=np.uint32)
    z = [rng.randrange(ref.R) for _ in range(6)]
    j = _job(shape_name, "bad segments", ref.to_limbs(ints), off, ref.to_limbs(z), ref.to_limbs(vals), want_y=True)
    r = child.run([j])[0]
    assert r["rc"] == 0 and r["status"] == child.STATUS_BAD
    lam = np.full((total, 4), child.FILL, dtype=np.uint64)
    y = np.full((6, 4), child.FILL, dtype=np.uint64)
    fl = np.full(6, child.FILL8, dtype=np.uint8)
    for s, (a, b) in ((0, (0, 6)), (3, (4101, 4110))):
        l, d = ref.lagrange(ints[a:b], z[s])
        lam[a:b] = ref.to_limbs(l); y[s] = ref.to_limbs([ref.interpolate(l, vals[a:b])])[0]; fl[s] = d
    assert np.array_equal(r["lam"], lam) and np.array_equal(r["y"], y) and np.array_equal(r["flags"], fl)


def test_refusals_launch_nothing(emu_lib):
    segs = ref.edge_segments([3, 5], 4, seed=2)
    nodes, off, points, values = ref.pack(segs)
    tiny = SHAPES["tiny block"]
    jobs = [{"op": "lagrange", "label": "y without values", "nodes": nodes, "offsets": off, "points": points, "values": None, "want_y": True, "shape": tiny},
            {"op": "lagrange", "label": "neither lambda nor y", "nodes": nodes, "offsets": off, "points": points, "values": values, "want_lambda": False, "shape": tiny},
            {"op": "lagrange", "label": "nseg == 0", "nodes": nodes[:0], "offsets": np.zeros(1, dtype=np.uint32), "points": None, "values": None, "shape": tiny}]
    r = child.run(jobs)
    assert r[0]["rc"] == -1 and (r[0]["lam"] == np.uint64(child.FILL)).all() and (r[0]["y"] == np.uint64(child.FILL)).all()
    assert r[1]["rc"] == -1 and (r[1]["flags"] == child.FILL8).all()
    assert r[2]["rc"] == 0 and r[2]["lam"] is None


FAULTS = {1: "the factor j == i skipped in the first tile only", 2: "a point on a node not recognised", 3: "a repeated node seen only inside its own tile",
          4: "the WAVE shape reading a whole tile past the segment's end", 5: "the y sum dropping the lanes with one node fewer"}
FAULT_CASES = ["tiny block", "tiny wave", "shipped wave"]


@pytest.mark.parametrize("shape_name", FAULT_CASES)
@pytest.mark.parametrize("fault", sorted(FAULTS), ids=["fault%d" % f for f in sorted(FAULTS)])
def test_seeded_faults_are_caught(emu_lib, fault, shape_name):
    """the same cases must tell a kernel with ONE seeded fault from the real one, in both shapes: a suite that passes a broken kernel
    checks nothing.  (Fault 4 exists in the WAVE shape only.)"""
    if fault == 4 and shape_name == "tiny block":
        shape_name = "tiny wave"
    simt_harness.emu_lib(lambda: child.build_fault(fault))
    pairs = _edge_jobs(shape_name, fault=fault)
    caught = False
    for (j, want), r in zip(pairs, child.run([j for j, _ in pairs])):
        try:
            _check(r, want, j["label"])
        except AssertionError:
            caught = True
    assert caught, "no case tells fault %d (%s) from the real kernel (%s)" % (fault, FAULTS[fault], shape_name)
