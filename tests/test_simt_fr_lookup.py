"""The Fr lookup tables (blsgpu_fr_lookup_*), their device code compiled for the HOST (tests/simt/emu_fr_lookup.cpp), against a Python
dict over key tuples (tests/fr_lookup_ref.py).

What runs here is the code the GPU runs: `k_frl_build`, `k_frl_count` and `k_frl_finish` launched from the plan of
csrc/fr_lookup_plan.h -- the function api_fr.hip launches from -- with the lanes of a workgroup as threads, at block 64 (a table of
1000 rows is built by sixteen workgroups, 4096 looked-up rows are 64 batches) and at the shipped 256.  mult is compared limb for limb on
the raw 256-bit integers (a non-canonical output does not compare equal), index, missing and distinct as integers.  The table, the
looked-up rows, every output and the handle's own arrays end against an inaccessible page, outputs and counters are pre-filled with
patterns no result has, and everything runs in a child process under a time limit (tests/simt_fr_lookup_child.py).

The same cases run on a build whose hash keeps two bits (every probe chain starts in the last four slots, runs long and wraps), and
test_the_suite_catches_a_seeded_fault builds the library with each of the kernels' five seeded faults (-DFRL_FAULT=n) and requires
the cases of this file to tell it from the real one."""
import pytest

import fr_lookup_ref as ref
import simt_fr_lookup_child as child
import simt_harness
from bls12_381_amd import synthetic
from oracle import bls12_381_ref as o

RR = ref.RR
SMALL = 64                                                         # the small block shape
ROWS, NS, CS = (1, 2, 63, 64, 65, 1000), (0, 1, 777, 4096), (1, 3, 8)


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    return simt_harness.emu_lib(child.build)


class Case:
    """one table and one count call: column sets of integers, the job, the expectation"""

    def __init__(self, what, table, f, negate=0, block=SMALL, lds_rows=0, reverse=0, t_pitch=None, f_pitch=None, outputs=("mult", "index", "missing"), words=None):
        self.what, self.table, self.f, self.negate, self.block, self.lds_rows, self.reverse = what, table, f, negate, block, lds_rows, reverse
        self.t_pitch, self.f_pitch, self.outputs = t_pitch, f_pitch, outputs
        self.words = words                                         # (table words, f words) given directly: keys that are not integers mod r
        self._want = None

    def at(self, **kw):
        c = Case(self.what + " " + " ".join("%s=%s" % kv for kv in sorted(kw.items())), self.table, self.f, self.negate, self.block, self.lds_rows, self.reverse, self.t_pitch, self.f_pitch,
                 self.outputs, self.words)
        c._want = self._want
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def _words(self):
        if self.words is None:
            import numpy as np
            pack = lambda cols: np.stack([ref.mont_words(col) if len(col) else np.zeros((0, 8), dtype=np.uint32) for col in cols])
            self.words = (pack(self.table), pack(self.f))
        return self.words

    def job(self, lib=None):
        t, f = self._words()
        j = {"op": "run", "table": t, "f": f, "negate": self.negate, "block": self.block, "lds_rows": self.lds_rows, "reverse": self.reverse, "outputs": self.outputs, "lib": lib,
             "label": self.what}
        if self.t_pitch:
            j["t_pitch"] = self.t_pitch
        if self.f_pitch:
            j["f_pitch"] = self.f_pitch
        return j

    def want(self):
        if self._want is None:
            self._want = ref.count(self.table, self.f)
        return self._want

    def differs(self, res):
        """the names of the outputs that differ from the reference"""
        mult, index, missing, distinct = self.want()
        bad = []
        if "mult" in self.outputs and ref.raw_ints(res["mult"]) != ref.mult_raw(mult, self.negate):
            bad.append("mult")
        if "index" in self.outputs and [int(x) for x in res["index"]] != index:
            bad.append("index")
        if "missing" in self.outputs and res["missing"] != missing:
            bad.append("missing")
        if res["distinct"] != distinct:
            bad.append("distinct")
        for name in ("mult", "index", "missing"):
            if name not in self.outputs and res[name] is not None:
                bad.append(name + " written")
        return bad

    def check(self, res):
        bad = self.differs(res)
        assert not bad, "%s: %s differ" % (self.what, ", ".join(bad))
        rows = len(self.table[0])
        assert res["slots"] == ref.slots(rows) and res["lds_path"] == (1 if rows <= (self.lds_rows or ref.LDS_ROWS) else 0), self.what


_GRID = {}


def grid_cases():
    """rows x n x c with repeated table rows (every fifth, at scattered earlier positions) and misses (every seventh looked-up row)"""
    if not _GRID:
        out = []
        for rows in ROWS:
            for n in NS:
                for c in CS:
                    t, f, mult, index, missing = synthetic.lookup_tuple_instance(rows, n, c, seed=1000 * rows + 8 * n + c, dup_every=5, miss_every=7)
                    case = Case("rows=%d n=%d c=%d" % (rows, n, c), t, f)
                    assert (mult, index, missing) == case.want()[:3], "synthetic.lookup_tuple_instance and the reference disagree"
                    out.append(case)
        _GRID["cases"] = out
    return _GRID["cases"]


def _scalars(rng, k):
    return [rng.scalar() for _ in range(k)]


def special_cases():
    rng = o.SplitMix64(77)
    out = []
    # every row of the table equal
    key = _scalars(rng, 3)
    t = [[key[j]] * 200 for j in range(3)]
    f = [[key[j]] * 300 + _scalars(rng, 5) for j in range(3)]
    out.append(Case("every table row equal", t, f))
    # each key three times, at scattered positions (row i holds key (i * 37) % 100: the copies are 100 / 37 apart in every order)
    base = [_scalars(rng, 2) for _ in range(100)]
    order = [(i * 37) % 100 for i in range(300)]
    t = [[base[k][j] for k in order] for j in range(2)]
    picks = [(i * 13 + i // 7) % 100 for i in range(500)]
    f = [[base[k][j] for k in picks] for j in range(2)]
    out.append(Case("each key three times, scattered", t, f))
    # 0 and r - 1, and c = 1 keys next to each other
    t = [[0, RR - 1, 1, RR - 2]]
    f = [[RR - 1, 0, 0, 2, RR - 1, RR - 3, 1]]
    out.append(Case("the keys 0 and r - 1", t, f))
    # f all equal to one row / every row a miss, on a table with a repeat
    t = [_scalars(rng, 65)]
    t[0][40] = t[0][3]
    out.append(Case("f all on row 3", t, [[t[0][3]] * 777]))
    out.append(Case("f all on row 3, negated", t, [[t[0][3]] * 777], negate=1))
    out.append(Case("every looked-up row a miss", t, [_scalars(rng, 300)]))
    out.append(Case("n = 0, negated", t, [[]], negate=1))
    # a pitch larger than the column, both sets
    t3 = [_scalars(rng, 70) for _ in range(3)]
    f3 = [[t3[j][(i * 7) % 70] for i in range(150)] for j in range(3)]
    out.append(Case("pitch beyond the columns", t3, f3, t_pitch=75, f_pitch=190))
    # outputs left out
    for outs in (("mult",), ("index",), ("missing",), ("index", "missing"), ()):
        out.append(Case("outputs %s" % (outs,), t3, f3, outputs=outs))
    return out


def top_word_case():
    """c = 8 keys that differ only in the top word of the last column: the keys are given as WORDS (equality is word equality)"""
    import numpy as np
    rng = o.SplitMix64(5)
    rows, n = 130, 400
    row = ref.mont_words(_scalars(rng, 8))                         # one key, (8, 8) words
    t = np.repeat(row[:, None, :], rows, axis=1).copy()            # (8, rows, 8)
    t[7, :, 7] = (t[7, :, 7] & np.uint32(0xFFFF0000)) | np.arange(rows, dtype=np.uint32)
    pick = [(i * 29) % (rows + 20) for i in range(n)]              # 130 .. 149: top words no table row has
    f = np.repeat(row[:, None, :], n, axis=1).copy()
    f[7, :, 7] = (f[7, :, 7] & np.uint32(0xFFFF0000)) | np.array(pick, dtype=np.uint32)
    ints = lambda w: [[tuple(int(x) for x in w[j, i]) for i in range(w.shape[1])] for j in range(w.shape[0])]
    return Case("keys differing in the top word of the last column", ints(t), ints(f), words=(t, f))


def path_cases():
    """both counting paths on the same data: the threshold lowered to 64 sends 65 and 1000 rows through the cache"""
    out = []
    for c in grid_cases():
        rows, n = len(c.table[0]), len(c.f[0])
        if rows in (64, 65, 1000) and n in (777, 4096) and len(c.table) in (1, 3):
            out.append(c.at(lds_rows=64))
    rng = o.SplitMix64(9)
    t = [_scalars(rng, 1000)]
    out.append(Case("cache path, f all on row 3", t, [[t[0][3]] * 4096], lds_rows=64))
    # more distinct hit rows than cache entries share: 1000 rows over 2048 entries still collide, and a collision adds globally
    out.append(Case("cache path, every row once", t, [t[0][::-1]], lds_rows=64))
    return out


def all_cases():
    g = grid_cases()
    return g + special_cases() + [top_word_case()] + path_cases() + [c.at(reverse=1) for c in g if len(c.table[0]) == 1000 and len(c.f[0]) == 777]


def _run(cases, lib=None):
    res = child.run([c.job(lib) for c in cases])
    for c, r in zip(cases, res):
        c.check(r)
    return res


def test_rows_n_and_c_at_block_64():
    _run(grid_cases())


def test_rows_n_and_c_at_the_shipped_block():
    res = _run([c.at(block=0) for c in grid_cases()])
    for c, r in zip(grid_cases(), res):
        assert r["count_grid"] == -(-len(c.f[0]) // ref.BLOCK)


def test_special_tables_and_lookups():
    _run(special_cases() + [top_word_case()])
    _run([c.at(block=0) for c in special_cases()])


def test_both_counting_paths():
    cases = path_cases()
    res = _run(cases)
    assert all(r["lds_path"] == (1 if len(c.table[0]) <= 64 else 0) for c, r in zip(cases, res))
    assert any(r["lds_path"] == 0 for r in res) and any(r["lds_path"] == 1 for r in res)


def test_the_first_row_represents_a_repeated_key_whatever_the_order():
    """the later workgroups build first: only the atomicMin then makes the first row the representative"""
    _run([c.at(reverse=1) for c in grid_cases() if len(c.table[0]) in (65, 1000)] + [c.at(reverse=1) for c in special_cases()[:2]])


def test_a_two_bit_hash_changes_nothing():
    """-DFRL_HASH_BITS=2: every chain starts in the last four slots and wraps; the results are the same"""
    lib = child.build_degenerate()
    cases = [c for c in grid_cases() if len(c.f[0]) in (0, 1, 777)] + special_cases() + [top_word_case()] + path_cases()[-2:]
    _run(cases, lib)


def test_the_plan():
    rows_n = [(r, n) for r in (1, 2, 63, 64, 65, 1000, 4096, 4097, 1 << 20, 1 << 24) for n in (0, 1, 255, 256, 257, 1 << 20, 1 << 28)]
    jobs = [{"op": "plan", "rows": r, "n": n, "label": "plan"} for r, n in rows_n]
    for (rows, n), r in zip(rows_n, child.run(jobs)):
        assert r["ok"] == 1 and r["slots"] == ref.slots(rows) and r["block"] == ref.BLOCK, (rows, n, r)
        assert r["lds_path"] == (1 if rows <= ref.LDS_ROWS else 0) and r["count_lds"] <= 64 * 1024, (rows, n, r)
        assert r["build_grid"] == r["finish_grid"] == -(-rows // 256), (rows, n, r)
        per = r["count_grid"] * 256
        assert (per * r["iters"] >= n > per * (r["iters"] - 1)) if n else (r["count_grid"] == 0 and r["iters"] == 0), (rows, n, r)
    bad = [dict(rows=0, n=1), dict(rows=(1 << 24) + 1, n=1), dict(rows=5, n=(1 << 28) + 1), dict(rows=5, n=5, block=96), dict(rows=5, n=5, lds_rows=4097)]
    assert [r["ok"] for r in child.run([dict(b, op="plan", label="refusal") for b in bad])] == [0] * len(bad)


def test_the_hash_reads_every_word():
    """flipping any single bit-pattern of any single word of a c = 8 key changes the hash (the host function the kernels share)"""
    import numpy as np
    rng = np.random.RandomState(3)
    key = rng.randint(0, 1 << 32, size=64, dtype=np.uint64).astype(np.uint32)
    keys = [key]
    for w in range(64):
        k = key.copy()
        k[w] ^= np.uint32(1 << (w % 32))
        keys.append(k)
    h = child.run([{"op": "hash", "keys": np.stack(keys), "c": 8, "label": "hash"}])[0]["hashes"]
    assert all(x != h[0] for x in h[1:])
    tiny = np.zeros((64, 8), dtype=np.uint32)                      # tiny limbs: only the low word differs
    tiny[:, 0] = np.arange(64)
    ht = child.run([{"op": "hash", "keys": tiny, "c": 1, "label": "hash tiny"}])[0]["hashes"]
    assert len(set(ht)) == 64 and len({x & 127 for x in ht}) > 32


FAULTS = {1: "no atomicMin: the representative is whichever row arrived first", 2: "the probe does not wrap", 3: "the key compare looks at column 0 only",
          4: "a workgroup whose last batch is partial does not flush its LDS counters", 5: "a miss writes index 0 instead of the sentinel"}


@pytest.mark.parametrize("fault", sorted(FAULTS), ids=["fault%d" % f for f in sorted(FAULTS)])
def test_the_suite_catches_a_seeded_fault(fault):
    """the cases above against a library whose kernels carry ONE seeded fault: some case must differ from the reference, or the child must
    die on a guarded page (a probe that runs off the end of the slot array)"""
    lib = child.build_fault(fault)
    cases = [c for c in all_cases() if len(c.f[0]) <= 777 or len(c.table[0]) == 65]
    try:
        res = child.run([c.job(lib) for c in cases])
    except pytest.fail.Exception as e:
        assert fault == 2 and "SIGSEGV" in str(e), "fault %d (%s) ended the child: %s" % (fault, FAULTS[fault], e)
        return
    caught = [c.what for c, r in zip(cases, res) if c.differs(r)]
    assert caught, "no case tells fault %d (%s) from the real kernels" % (fault, FAULTS[fault])
