"""The twisted Edwards kernels (bls12_381_amd/csrc/fr_edwards.hip.h) on the host: every kernel compiled for the CPU through
tests/simt_harness.py / tests/simt/emu_harness.h, launched from the plans of csrc/fr_edwards_plan.h exactly as api_fr.hip launches them, at
a tiny shape (mul_batch: 4 lanes; the MSM: 4 lanes x 2 terms, a chunk of 8 terms; normalize: one wavefront) and at the shipped ones, on
Jubjub (complete) and Bandersnatch (not complete: odd-order points only).  Every expectation comes from the Python-integer reference
(tests/fr_edwards_ref.py through the shared cases of tests/fr_edwards_cases.py -- the cases of tests/test_fr_edwards.py); results are
compared as affine points, exactly.

Four wrong-result variants of the kernels (-DFR_EDWARDS_FAULT=n, built for this emulation only) must each be told from the real kernels
by these cases."""
import numpy as np
import pytest

import fr_edwards_cases as cases
import fr_edwards_ref as ref
import simt_fr_edwards_child as child
import simt_harness

CURVES = ["jubjub", "bandersnatch"]
TINY_MSM = (4, 2)
SHIPPED_CHUNK = 256


@pytest.fixture(scope="module")
def emu_lib():
    return simt_harness.emu_lib(child.build)


def curve(name):
    cv = ref.CURVES[name]
    return (cv.a, cv.d)


def affine_all(name, out):
    cv = ref.CURVES[name]
    v = ref.ints(out)
    return [cv.affine(v[3 * i:3 * i + 3]) for i in range(len(v) // 3)]


def mul_job(name, bits, n, block=0, fault=0):
    c = cases.mul_cases(name)
    return {"op": "mul", "label": "%s bits %d n %d block %d" % (name, bits, n, block), "curve": curve(name), "xy": ref.points_limbs(c["points"][:n]),
            "scalars": ref.scalar_bytes(c["scalars"][bits][:n]), "bits": bits, "block": block, "fault": fault}


@pytest.mark.parametrize("name", CURVES)
def test_mul_batch_vs_reference(emu_lib, name):
    """every bits of the GPU test at n = 257 (five blocks of the shipped shape), n = 63 and 1, and n = 63 at 4 lanes a block: the special
    points against the special scalars (0, 1, 2^bits - 1, s, h s, the carry patterns, 2^256 - 1) and random pairs"""
    want = cases.mul_cases(name)["want"]
    jobs = [mul_job(name, bits, n, block) for bits in cases.MUL_BITS for n, block in ((257, 0), (63, 0), (1, 0), (63, 4))]
    for j, r in zip(jobs, child.run(jobs)):
        n = j["xy"].shape[0]
        assert r["rc"] == 0 and r["status"] == 0, j["label"]
        assert affine_all(name, r["out"]) == want[j["bits"]][:n], j["label"]


def test_mul_batch_plan_is_the_shipped_one(emu_lib):
    r = child.run([{"op": "mul_plan", "label": "253", "n": 1000, "bits": 253}, {"op": "mul_plan", "label": "64", "n": 1000, "bits": 64},
                   {"op": "mul_plan", "label": "1", "n": 1, "bits": 1}])
    assert (r[0]["W"], r[0]["doublings"], r[0]["grid"], r[0]["block"], r[0]["lds"]) == (85, 252, 16, 64, 32768)
    assert (r[1]["W"], r[1]["doublings"]) == (22, 63) and (r[2]["W"], r[2]["doublings"]) == (1, 0)


@pytest.mark.parametrize("name", CURVES)
def test_mul_batch_flags_a_scalar_above_bits(emu_lib, name):
    """one scalar with a bit at `bits`: the status bit is raised and every other output is right"""
    c = cases.mul_cases(name)
    for bits in (3, 64, 253):
        j = mul_job(name, bits, 63)
        ks = list(c["scalars"][bits][:63])
        ks[17] |= 1 << bits
        j["scalars"] = ref.scalar_bytes(ks)
        r = child.run([j])[0]
        assert r["rc"] == 0 and r["status"] == child.STATUS_SCALAR
        got, want = affine_all(name, r["out"]), c["want"][bits][:63]
        assert got[:17] == want[:17] and got[18:] == want[18:]


@pytest.mark.parametrize("name", CURVES)
def test_check_and_normalize(emu_lib, name):
    """points on and off the curve and limbs >= r; projective points with random Z, Z = 1 and Z = 0, at n in {1, 63, 257}, a block of one
    wavefront and the shipped block"""
    cv = ref.CURVES[name]
    pts = cases.mul_cases(name)["points"]
    xy = ref.points_limbs(pts)
    bad = {5: "x", 40: "y", 200: "limbs"}
    for i, how in bad.items():
        if how == "limbs":
            xy[i, 0] = np.frombuffer(ref.RR.to_bytes(32, "little"), dtype=np.uint64)
        else:
            xy[i, 0 if how == "x" else 1] = ref.limbs([(pts[i][0 if how == "x" else 1] + 1) % ref.RR])[0]
    import random
    rng = random.Random(9)
    zs = [1 if i % 7 == 0 else rng.randrange(1, ref.RR) for i in range(len(pts))]
    zero = {0, 33, 62, 256}
    xyz = ref.limbs([c for i, (p, z) in enumerate(zip(pts, zs)) for c in (p[0] * z % ref.RR, p[1] * z % ref.RR, 0 if i in zero else z)]).reshape(-1, 3, 4)
    jobs = [{"op": "check", "label": "check %d" % n, "curve": curve(name), "xy": xy[:n]} for n in (1, 63, 257)]
    jobs += [{"op": "normalize", "label": "normalize %d block %d" % (n, b), "curve": curve(name), "xyz": xyz[:n], "block": b} for n, b in ((1, 0), (63, 64), (257, 64), (257, 0))]
    res = child.run(jobs)
    for j, r in zip(jobs[:3], res[:3]):
        n = j["xy"].shape[0]
        assert r["rc"] == 0 and list(r["ok"]) == [0 if i in bad else 1 for i in range(n)], j["label"]
    for j, r in zip(jobs[3:], res[3:]):
        n = j["xyz"].shape[0]
        assert r["rc"] == 0 and list(r["ok"]) == [0 if i in zero else 1 for i in range(n)], j["label"]
        assert ref.raw(r["xy"]) == ref.raw(ref.points_limbs([(0, 1) if i in zero else pts[i] for i in range(n)])), j["label"]      # limb for limb: canonical
    assert cv.on_curve(pts[5])


@pytest.mark.parametrize("name", CURVES)
def test_table_entries(emu_lib, name):
    """every entry of two small tables is k 2^(window w) B with d x y beside it, limb for limb; a base off the curve raises the flag"""
    cv = ref.CURVES[name]
    bs = cases.base_set(name, 8)["points"][:3]
    jobs = [{"op": "table", "label": "bits %d window %d" % (b, w), "curve": curve(name), "xy": ref.points_limbs(bs), "bits": b, "window": w} for b, w in ((3, 2), (9, 4))]
    off = ref.points_limbs(bs)
    off[1, 1] = ref.limbs([(bs[1][1] + 1) % ref.RR])[0]
    jobs.append({"op": "table", "label": "off the curve", "curve": curve(name), "xy": off, "bits": 3, "window": 2})
    res = child.run(jobs)
    for j, r in zip(jobs[:2], res[:2]):
        W, H, window = r["W"], r["H"], j["window"]
        assert r["rc"] == 0 and r["flag"] == 0 and W == ref.windows(j["bits"], window) and H == 1 << (window - 1) and r["table"].shape[0] == 3 * W * H
        want = []
        for b in bs:
            for w in range(W):
                q = cv.mul(1 << (window * w), b)
                for k in range(1, H + 1):
                    p = cv.mul(k, q)
                    want += [p[0], p[1], cv.d * p[0] * p[1] % ref.RR]
        assert ref.raw(r["table"]) == ref.raw(ref.limbs(want)), j["label"]
    assert res[2]["rc"] == 0 and res[2]["flag"] == 1


def msm_job(name, kind, n, bits, window, shape, fault=0):
    chunk = shape[0] * shape[1] if shape else SHIPPED_CHUNK
    c = cases.msm_case(name, kind, n, bits, chunk)
    return c, {"op": "msm", "label": "%s %s n %d bits %d window %d shape %s" % (name, kind, n, bits, window, shape), "curve": curve(name),
               "xy": ref.points_limbs(cases.base_set(name, n)["points"]), "bits": bits, "window": window, "offsets": c["offsets"], "base_first": c["base_first"],
               "scalars": ref.scalar_bytes(c["scalars"]), "shape": shape, "fault": fault}


TINY_CASES = [("long", 64, 253, 4), ("natural", 64, 253, 4), ("shared", 8, 3, 2), ("shared", 1, 3, 8), ("cancel", 8, 256, 8)]
SHIPPED_CASES = [("long", 1024, 3, 2), ("natural", 64, 253, 4), ("shared", 8, 253, 2)]


@pytest.mark.parametrize("name", CURVES)
@pytest.mark.parametrize("shape_name", ["tiny", "shipped"])
def test_msm_segments_vs_reference(emu_lib, name, shape_name):
    """empty segments, length 1, exactly a chunk, one less, one more, three chunks and five, 300 short ones around a long one, one shared
    slice, overlapping slices, base_first == NULL, the identity and a small-order point among the bases (Jubjub), terms that cancel"""
    shape = TINY_MSM if shape_name == "tiny" else None
    made = [msm_job(name, kind, n, bits, window, shape) for kind, n, bits, window in (TINY_CASES if shape_name == "tiny" else SHIPPED_CASES)]
    for (c, j), r in zip(made, child.run([j for _, j in made], timeout=900)):
        assert r["rc"] == 0 and r["status"] == 0 and r["flag"] == 0, j["label"]
        assert affine_all(name, r["out"]) == c["want"], j["label"]


def test_msm_plan_is_the_shipped_one(emu_lib):
    r = child.run([{"op": "msm_plan", "label": "shipped", "k": 10, "total": 1000}, {"op": "msm_plan", "label": "tiny", "k": 10, "total": 50, "shape": TINY_MSM}])
    assert (r[0]["block"], r[0]["terms"], r[0]["chunk"], r[0]["nchunks"]) == (128, 2, SHIPPED_CHUNK, 4) and r[0]["lds"] == 128 * 38 * 4
    assert r[0]["part_bytes"] == 8 * 128 and r[0]["meta_bytes"] == 32 and r[0]["off_bytes"] == 88
    assert (r[1]["chunk"], r[1]["nchunks"], r[1]["chunks_grid"], r[1]["combine_grid"]) == (8, 7, 7, 14)


@pytest.mark.parametrize("name", CURVES)
def test_msm_device_form_reports_a_broken_segment(emu_lib, name):
    """the device form cannot refuse these: the status bit is raised, nothing outside the (guarded) arrays is touched, and where only a
    base range is wrong every other segment is still right"""
    c, j = msm_job(name, "long", 64, 253, 4, TINY_MSM)
    k = len(c["offsets"]) - 1
    bf = list(c["base_first"])
    victim = 6                                                     # the segment of three chunks and five
    bf[victim] = 64 - 3                                            # its bases run out of the table after three terms
    dec = list(c["offsets"])
    dec[3], dec[4] = dec[4], dec[3]                                # decreasing offsets
    short = dict(j, total=c["offsets"][-1] - 5)                    # offsets[k] != total: the tail is clamped away
    big = list(c["offsets"])
    big[-1] = 0xFFFFFFF0                                           # far beyond total and the scalars
    res = child.run([dict(j, base_first=bf, label="bases outside"), dict(j, offsets=dec, label="decreasing"), dict(short, label="offsets[k] != total"),
                     dict(j, offsets=big, total=c["offsets"][-1], label="an offset beyond total")], timeout=900)
    for r in res:
        assert r["rc"] == 0 and r["status"] & child.STATUS_BAD
    got = affine_all(name, res[0]["out"])
    assert [g for i, g in enumerate(got) if i != victim] == [w for i, w in enumerate(c["want"]) if i != victim]
    assert k == len(got)


@pytest.mark.parametrize("fault", child.FAULTS)
def test_wrong_result_variants_are_caught(emu_lib, fault):
    """each variant changes at least one output of the cases above and none of them leaves its arrays (the child would die)"""
    simt_harness.emu_lib(lambda: child.build_fault(fault))
    name = "jubjub"
    want_mul = cases.mul_cases(name)["want"][253][:63]
    made = [msm_job(name, kind, n, bits, window, TINY_MSM, fault=fault) for kind, n, bits, window in TINY_CASES[:2]]
    jobs = [mul_job(name, 253, 63, fault=fault)] + [j for _, j in made]
    res = child.run(jobs, timeout=900)
    assert all(r["rc"] == 0 for r in res)
    wrong_mul = affine_all(name, res[0]["out"]) != want_mul
    wrong_msm = any(affine_all(name, r["out"]) != c["want"] for (c, _), r in zip(made, res[1:]))
    if fault in (1, 2):
        assert wrong_mul and wrong_msm, "the variant of the recoding / the negation went unnoticed"
    else:
        assert wrong_msm and not wrong_mul, "the variant of the MSM passes went unnoticed"
