"""Poseidon over Fr (blsgpu_fr_poseidon_*), its device code compiled for the HOST (tests/simt/emu_fr_poseidon.cpp), against the textbook
definition in Python integers (tests/fr_poseidon_ref.py: add the constants, pow(x, 5, r), multiply by the matrix -- nothing of the sparse
form).

What runs here is the code the GPU runs: `k_frp_permute` and `k_frp_hash` (also a Merkle level) for every width and both
forms, on the constant image built by csrc/fr_poseidon_plan.h -- the validation, the sparse derivation and the scaling the entry point
runs -- and launched step by step from the plans of that header, at the shipped block (256 lanes) and at a block of 16 lanes, where the
levels of a small tree already span several workgroups.  Results are compared limb for limb, so a non-canonical output does not compare
equal, and every job checks that its inputs were not written.  The library is built with trapping bounds / shift checks, every buffer
(the image included) ends against an inaccessible page, and it runs in a child process under a time limit
(tests/simt_fr_poseidon_child.py), one host thread per lane.

That the tests bite was checked by seeding faults one at a time (each was confirmed to fail, then removed):
  * the carry u dropped (fr_poseidon_build leaves the second half's first constants as given): test_widths_and_rounds,
    test_production_rounds, test_edge_states_and_parameters, test_singular_block_falls_back_to_dense and test_merkle_binary differ
    (both forms use the carried constants);
  * the pending matrix not applied (the frp_matvec<T - 1> call after the sparse rounds removed): the same tests differ except
    test_singular_block_falls_back_to_dense, which runs the dense rounds;
  * an S-box on element 1 as well in the dense partial round: test_widths_and_rounds, test_production_rounds,
    test_edge_states_and_parameters and test_singular_block_falls_back_to_dense differ; test_merkle_binary (sparse handles only) passes;
  * the reductions of the sparse rounds dropped (no frl_carry, `(r & 3) == 3` never true): test_production_rounds differs at t = 3 and
    t = 12 (57 rounds overflow the limbs) and test_widths_and_rounds at t = 12 (five rounds already overflow a dot of six); the short
    instances at t = 3 pass;
  * a Merkle level written where the level below lies (the plan's dst_off taken from the previous level): test_merkle_binary,
    test_merkle_arities, test_merkle_one_leaf_changes_its_path and test_shipped_shape differ."""

import numpy as np
import pytest

import simt_fr_poseidon_child as child
import simt_harness
import fr_poseidon_ref as ref
from bls12_381_amd import synthetic

RR = ref.RR
WIDTHS = [2, 3, 4, 5, 9, 12]
ROUNDS = [(2, 0), (2, 1), (4, 3), (8, 5)]
SMALL = 16
AUTO, DENSE, SPARSE = child.FORM_AUTO, child.FORM_DENSE, child.FORM_SPARSE

_params = {}


def params(t, rf, rp, seed=1):
    key = (t, rf, rp, seed)
    if key not in _params:
        c, m = synthetic.poseidon_test_params(t, rf, rp, seed)
        _params[key] = (t, rf, rp, c, m)
    return _params[key]


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    return simt_harness.emu_lib(child.build)


def rand(n, seed):
    return synthetic.to_ints(synthetic.scalars(n, seed))


def sparse_products(t, rf, rp):
    return rf * (3 * t + t * t) + rp * (2 * t + 2) + (t - 1) ** 2


def dense_products(t, rf, rp):
    return rf * (3 * t + t * t) + rp * (3 + t * t)


def permute_job(p, states, form=AUTO, block=None, inplace=False, note=""):
    t = p[0]
    return {"kind": "permute", "params": p, "form": form, "block": block, "inplace": inplace, "states": states,
            "data": ref.words([x for s in states for x in s]).reshape(len(states), t, 8),
            "label": "permute t=%d rounds=(%d,%d) form=%d n=%d block=%s inplace=%s %s" % (t, p[1], p[2], form, len(states), block, inplace, note)}


def hash_job(p, inputs, tag, form=AUTO, block=None, note=""):
    t = p[0]
    return {"kind": "hash", "params": p, "form": form, "block": block, "tag": tag, "inputs": inputs,
            "data": ref.words([x for s in inputs for x in s]).reshape(len(inputs), t - 1, 8),
            "label": "hash t=%d rounds=(%d,%d) form=%d n=%d block=%s tag=%d %s" % (t, p[1], p[2], form, len(inputs), block, tag % 1000, note)}


def merkle_job(p, leaves, height, k, tag, nodes=True, form=AUTO, block=None, note=""):
    return {"kind": "merkle", "params": p, "form": form, "block": block, "tag": tag, "height": height, "k": k, "nodes": nodes, "leaves": leaves,
            "data": ref.words(leaves),
            "label": "merkle t=%d height=%d k=%d nodes=%s form=%d block=%s %s" % (p[0], height, k, nodes, form, block, note)}


def check(jobs, res):
    for j, r in zip(jobs, res):
        assert "refused" not in r, "%s: refused: %s" % (j["label"], r.get("refused"))
        p = j["params"]
        if j["kind"] == "permute":
            want = [x for s in j["states"] for x in ref.permute(s, *p)]
            got = ref.raw_ints(r["out"].reshape(-1, 8))
        elif j["kind"] == "hash":
            want = [ref.hash_one(j["tag"], s, *p) for s in j["inputs"]]
            got = ref.raw_ints(r["out"])
        else:
            levels, roots = ref.merkle(j["tag"], j["leaves"], j["height"], j["k"], *p)
            want, got = list(roots), ref.raw_ints(r["out"])
            if j["nodes"]:
                flat = [x for lv in levels for x in lv]
                gn = ref.raw_ints(r["nodes"])
                assert len(gn) == len(flat), j["label"]
                bad = [i for i in range(len(flat)) if gn[i] != ref.mont([flat[i]])[0]]
                assert not bad, "%s: %d inner nodes differ, first at %s" % (j["label"], len(bad), bad[:6])
            else:
                assert r["nodes"] is None
        wm = ref.mont(want)
        bad = [i for i in range(len(wm)) if got[i] != wm[i]]
        assert len(got) == len(wm) and not bad, "%s: %d outputs differ, first at %s" % (j["label"], len(bad), bad[:6])
        if not j.get("inplace") and r["data_after"] is not None:
            assert np.array_equal(r["data_after"], j["data"]), "%s: the inputs were written" % j["label"]


def run_and_check(jobs):
    res = child.run(jobs)
    check(jobs, res)
    return res


@pytest.mark.parametrize("t", WIDTHS)
def test_widths_and_rounds(t):
    """every width x rounds (2,0), (2,1), (4,3), (8,5) x both forms: permute of n in {1, 2, 63, 64, 65, block - 1, block + 1} states at the
    small block (in place for the dense form, out of place for the sparse one), n in {255, 257} at the shipped block for (4,3), and
    hash_many of 17 preimages; the form and the product count the handle reports"""
    jobs, meta = [], []
    for rf, rp in ROUNDS:
        p = params(t, rf, rp)
        for form in (AUTO, DENSE):
            for n in (1, 2, 63, 64, 65, SMALL - 1, SMALL + 1):
                states = [rand(t, 1000 * n + 10 * i + rp) for i in range(n)]
                jobs.append(permute_job(p, states, form, SMALL, inplace=form == DENSE))
                meta.append((rf, rp, form))
            if (rf, rp) == (4, 3):
                for n in (255, 257):
                    st = rand(n * t, 7 * n + t)
                    jobs.append(permute_job(p, [st[i * t:(i + 1) * t] for i in range(n)], form, None, inplace=form == AUTO))
                    meta.append((rf, rp, form))
            ins = rand(17 * (t - 1), 31 * t + rf)
            jobs.append(hash_job(p, [ins[i * (t - 1):(i + 1) * (t - 1)] for i in range(17)], 5 + rp, form, SMALL))
            meta.append((rf, rp, form))
    res = run_and_check(jobs)
    for (rf, rp, form), r, j in zip(meta, res, jobs):
        if form == AUTO:
            assert r["form"] == SPARSE and r["products"] == sparse_products(t, rf, rp), j["label"]
        else:
            assert r["form"] == DENSE and r["products"] == dense_products(t, rf, rp), j["label"]
        assert r["kernels"] == [child.K_PERMUTE if j["kind"] == "permute" else child.K_HASH]


@pytest.mark.parametrize("t", [3, 12])
def test_production_rounds(t):
    """(8, 57): 57 partial rounds run the periodic reductions of the sparse form many times over"""
    p = params(t, 8, 57)
    n = 65 if t == 3 else 20
    st = rand(n * t, 99 + t)
    states = [st[i * t:(i + 1) * t] for i in range(n)]
    states[0] = [RR - 1] * t
    jobs = [permute_job(p, states, AUTO), permute_job(p, states[:5], DENSE)]
    res = run_and_check(jobs)
    assert res[0]["form"] == SPARSE and res[0]["products"] == sparse_products(t, 8, 57)
    assert res[1]["form"] == DENSE and res[1]["products"] == dense_products(t, 8, 57)
    assert (t, res[0]["products"], res[1]["products"]) in ((3, 604, 828), (12, 3043, 9819))


@pytest.mark.parametrize("t", WIDTHS)
def test_edge_states_and_parameters(t):
    """states of all 0 and all r - 1 (and one of each); zero round constants; M = identity; constants of r - 1 -- both forms"""
    rf, rp = 4, 3
    _, _, _, c, m = params(t, rf, rp)
    ident = [[1 if i == j else 0 for j in range(t)] for i in range(t)]
    zero_c = [[0] * t for _ in range(rf + rp)]
    top_c = [[RR - 1] * t for _ in range(rf + rp)]
    states = [[0] * t, [RR - 1] * t, [0, RR - 1] * (t // 2) + [0] * (t % 2), rand(t, t)]
    jobs = []
    for cc, mm, note in ((c, m, "edge states"), (zero_c, m, "zero constants"), (c, ident, "identity matrix"), (zero_c, ident, "zero constants, identity"),
                         (top_c, m, "constants r - 1")):
        for form in (AUTO, DENSE):
            jobs.append(permute_job((t, rf, rp, cc, mm), states, form, SMALL, note=note))
    res = run_and_check(jobs)
    for j, r in zip(jobs, res):
        assert r["form"] == (SPARSE if j["form"] == AUTO else DENSE), j["label"]       # the identity's lower-right block is regular


@pytest.mark.parametrize("t", WIDTHS)
def test_singular_block_falls_back_to_dense(t):
    """a matrix whose lower-right (t-1) x (t-1) block is singular (two equal rows there; a zero entry at t = 2): AUTO reports DENSE and the
    result still equals the definition"""
    rf, rp = 4, 3
    _, _, _, c, m = params(t, rf, rp)
    m = [list(row) for row in m]
    if t == 2:
        m[1][1] = 0
    else:
        m[2][1:] = m[1][1:]
    p = (t, rf, rp, c, m)
    states = [rand(t, 50 + i) for i in range(3)]
    res = run_and_check([permute_job(p, states, AUTO, SMALL), permute_job(p, states, DENSE, SMALL)])
    assert res[0]["form"] == DENSE and res[1]["form"] == DENSE
    assert res[0]["products"] == dense_products(t, rf, rp)


def test_hash_many():
    """the tag is honoured (two tags, two sets of digests, both as defined), the digest is element 1 of the permutation of
    (tag, x_1 .. x_(t-1)), the inputs are not written; n over several small blocks"""
    jobs, perms = [], []
    for t in WIDTHS:
        p = params(t, 4, 3)
        n = 2 * SMALL + 3
        ins = rand(n * (t - 1), 17 * t)
        rows = [ins[i * (t - 1):(i + 1) * (t - 1)] for i in range(n)]
        for tag in (0, 1, RR - 1):
            jobs.append(hash_job(p, rows, tag, AUTO, SMALL))
        perms.append(permute_job(p, [[1] + r for r in rows], AUTO, SMALL))
    res = run_and_check(jobs + perms)
    for i, t in enumerate(WIDTHS):
        a, b, c = (res[3 * i + v]["out"] for v in range(3))
        assert not np.array_equal(a, b) and not np.array_equal(b, c)
        assert np.array_equal(b, res[len(jobs) + i]["out"][:, 1, :]), "the digest is element 1 of the permuted state"


@pytest.mark.parametrize("k", [1, 3])
def test_merkle_binary(k):
    """arity 2 at the small block, every height from 0 to 8 (levels of one node up to levels over many workgroups); `nodes` given and
    NULL; every inner node and every root; the launches the plan takes"""
    p = params(3, 2, 1)
    L, C = child.K_LEVEL, child.K_COPY
    want = {h: [L] * h for h in range(1, 9)}
    want[0] = [C]
    jobs = []
    for height in range(0, 9):
        leaves = rand(k << height, 3 * height + k)
        for nodes in (True, False):
            jobs.append(merkle_job(p, leaves, height, k, 7, nodes, AUTO, SMALL))
    res = run_and_check(jobs)
    for j, r in zip(jobs, res):
        assert r["kernels"] == want[j["height"]], j["label"]


def test_merkle_arities():
    """arities 3, 4, 8 and 11 (and 1: t = 2) at heights 0 to 2, k in {1, 3}, `nodes` given and NULL, both forms"""
    jobs = []
    for t in (2, 4, 5, 9, 12):
        p = params(t, 2, 1)
        a = t - 1
        for height in (0, 1, 2):
            for k in (1, 3):
                leaves = rand(k * a ** height, 100 * t + 10 * height + k)
                jobs.append(merkle_job(p, leaves, height, k, 3, True, AUTO, SMALL))
                jobs.append(merkle_job(p, leaves, height, k, 3, False, DENSE, SMALL))
    run_and_check(jobs)


def test_merkle_one_leaf_changes_its_path():
    """changing one leaf changes exactly the nodes on its path to the root, in its own tree"""
    p = params(3, 2, 1)
    height, k, v = 7, 3, 2 * 128 + 77
    leaves = rand(k << height, 5)
    other = list(leaves)
    other[v] = (other[v] + 1) % RR
    ra, rb = child.run([merkle_job(p, leaves, height, k, 1, True, AUTO, SMALL), merkle_job(p, other, height, k, 1, True, AUTO, SMALL)])
    path, off, idx, n = set(), 0, v, k << height
    for _ in range(height):
        idx //= 2
        n //= 2
        path.add(off + idx)
        off += n
    diff = {i for i in range(ra["nodes"].shape[0]) if not np.array_equal(ra["nodes"][i], rb["nodes"][i])}
    assert diff == path
    assert [not np.array_equal(ra["out"][q], rb["out"][q]) for q in range(k)] == [False, False, True]


def test_shipped_shape():
    """the plan's real block of 256 lanes: binary trees of height 10 (levels of several workgroups down to one node), 40 small trees,
    arity 8 with 8^3 leaves; hash_many over a partial last block"""
    L = child.K_LEVEL
    p3, p9 = params(3, 2, 1), params(9, 2, 1)
    jobs = [merkle_job(p3, rand(3 << 10, 1), 10, 3, 2, True), merkle_job(p3, rand(3 << 10, 1), 10, 3, 2, False),
            merkle_job(p3, rand(40 << 6, 2), 6, 40, 2, True), merkle_job(p9, rand(8 ** 3, 3), 3, 1, 2, True)]
    ins = rand(300 * 2, 4)
    jobs.append(hash_job(p3, [ins[2 * i:2 * i + 2] for i in range(300)], 9))
    res = run_and_check(jobs)
    assert [r["kernels"] for r in res] == [[L] * 10, [L] * 10, [L] * 6, [L] * 3, [child.K_HASH]]


def test_create_refusals_name_the_argument():
    """what blsgpu_fr_poseidon_create refuses, through the same validation function: a width outside the set, an odd or out-of-range
    r_full, r_partial out of range, form SPARSE as a request, a round constant and a matrix entry that are not below r (named by index)"""
    t, rf, rp, c, m = params(3, 4, 3)
    bad = []
    for tt in (0, 1, 6, 7, 8, 10, 11, 13):
        cc, mm = [[0] * tt for _ in range(rf + rp)], [[1] * tt for _ in range(tt)]
        bad.append(({"kind": "create", "params": (tt, rf, rp, cc, mm), "label": "t=%d" % tt}, "t must be one of"))
    for r_full in (0, 3, 18):
        cc = [[0] * t for _ in range(r_full + rp)]
        bad.append(({"kind": "create", "params": (t, r_full, rp, cc, m), "label": "r_full=%d" % r_full}, "r_full"))
    bad.append(({"kind": "create", "params": (t, rf, 129, [[0] * t for _ in range(rf + 129)], m), "label": "r_partial=129"}, "r_partial"))
    bad.append(({"kind": "create", "params": (t, rf, rp, c, m), "form": SPARSE, "label": "form=SPARSE"}, "form"))
    raw = ref.limbs([x for row in c for x in row]).copy()
    raw[10] = np.array([0xffffffff00000001, 0x53bda402fffe5bfe, 0x3339d80809a1d805, 0x73eda753299d7d48], dtype=np.uint64)      # r itself
    bad.append(({"kind": "create", "params": (t, rf, rp, c, m), "raw_constants": raw, "label": "constant 10 = r"}, "round_constants[10] (round 3, element 1)"))
    res = child.run([b[0] for b in bad] + [{"kind": "create", "params": (t, rf, rp, c, m), "label": "valid"}])
    for (j, text), r in zip(bad, res):
        assert "refused" in r and text in r["refused"], (j["label"], r)
    assert res[-1]["form"] == SPARSE
