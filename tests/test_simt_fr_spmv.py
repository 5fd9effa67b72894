"""The sparse matrix-vector product over Fr (blsgpu_fr_spmv*), its device code compiled for the HOST (tests/simt/emu_fr_spmv.cpp), against
Python integers mod r.

What runs here is the code the GPU runs: the upload kernels `k_frsp_prepare` / `k_frsp_validate`, then `k_frsp_tile` and `k_frsp_fixup`
launched step by step from the plan of csrc/fr_spmv_plan.h -- the function api_fr.hip launches from -- with its grids, blocks, LDS sizes
and record sizes.  The plan is driven at small tiles (64 lanes x 2 entries = 128, 128 x 2 = 256), where a row of 300 entries spans three
tiles, and once at the shipped shape (256 x 8 = 2048).  Every expectation is out[v][i] = sum val[p] x[v][col[p]] in Python integers;
results are compared limb for limb, so a non-canonical output does not compare equal.  The output buffer is pre-filled with a
pattern, so a row that nobody writes (the classic hole: an empty row) shows as a difference.

Every launch runs its block on one host thread per lane (the kernels shuffle and meet at barriers); the library is built with trapping
bounds / shift checks, every buffer (HEAD / TAIL / META records included) has exactly the size the plan reserves and ends against an
inaccessible page, and it runs in a child process under a time limit (tests/simt_fr_spmv_child.py).

That the tests bite was checked by seeding faults one at a time (each was confirmed to fail, then removed):
  * the row-end flag dropped in the lane aggregate (`a.f = 0` where a row ends in k_frsp_tile, so the block scan carries a finished
    row's sum into the next row): every test with more than one row fails (test_single_row and test_validation_kernel pass);
  * the carry given to the wrong row (`row` instead of `row0` where the lead sum is stored): the same nine tests fail;
  * the empty-row fill removed (`if (!nnz)` for the FILL step in fr_spmv_plan.h): test_empty_rows, test_plan_launch_lists and
    test_shipped_shape fail -- the pattern shows in the empty rows;
  * the tile guard removed (`cnt = tile` in k_frsp_tile): the child of every product test ends outside a guarded buffer;
  * the fix-up stopping one tile early (`u < t_end` in k_frsp_fixup): every product test fails.

Run time on an 8-core machine: about 15 s, 5 s of them the build of the library."""

import numpy as np
import pytest

import simt_fr_spmv_child as child
import simt_harness
from oracle import bls12_381_ref as o

RR = o.R_ORDER
MONT = o.FR_MONT_R
SMALL = [(64, 2), (128, 2)]
FILL, TILE, FIXUP = child.K_FILL, child.K_TILE, child.K_FIXUP


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    return simt_harness.emu_lib(child.build)


def _words(vals):
    """integers mod r -> (len, 8) u32 Montgomery words"""
    b = b"".join((int(v) % RR * MONT % RR).to_bytes(32, "little") for v in vals)
    return np.frombuffer(b, dtype=np.uint32).reshape(-1, 8)


def _ints(words):
    """(…, 8) u32 words -> the raw 256-bit integers (NOT reduced: a non-canonical output must not compare equal)"""
    w = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, 8)
    return [int.from_bytes(row.tobytes(), "little") for row in w]


class Matrix:
    """rows: a list of lists of (column, value); the CSR arrays and the product in Python integers"""

    def __init__(self, rows, n_cols):
        self.rows, self.n_cols = rows, n_cols
        self.row_ptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint32)
        self.col = np.array([c for r in rows for c, _ in r], dtype=np.uint32)
        self.val = _words([v for r in rows for _, v in r]) if len(self.col) else np.zeros((0, 8), dtype=np.uint32)
        self.nnz = len(self.col)

    def times(self, xs):
        return [[sum(v * x[c] for c, v in r) % RR for r in self.rows] for x in xs]

    def job(self, xs, shape, label):
        return {"op": "spmv", "row_ptr": self.row_ptr, "col": self.col, "val": self.val, "n_cols": self.n_cols, "shape": shape,
                "x": np.stack([_words(x) for x in xs]).reshape(len(xs), self.n_cols, 8), "label": "%s shape=%s k=%d" % (label, shape, len(xs))}


def _by_lengths(lengths, n_cols, seed):
    """a matrix with the given row lengths: random columns (column 0 and n_cols - 1 forced in), random values with 0, 1 and r - 1 among them"""
    r = o.SplitMix64(seed)
    rows = []
    for i, n in enumerate(lengths):
        row = [(r.next() % n_cols, r.scalar()) for _ in range(n)]
        if n >= 1:
            row[0] = ((0, n_cols - 1)[i % 2], row[0][1])
        if n >= 4:
            row[1] = (row[1][0], (0, 1, RR - 1)[i % 3])
            row[-1] = (row[-2][0], row[-1][1])                     # a repeated column: the two entries add
        rows.append(row)
    return Matrix(rows, n_cols)


def _vectors(k, n_cols, seed):
    r = o.SplitMix64(seed)
    xs = [[r.scalar() for _ in range(n_cols)] for _ in range(k)]
    for v, x in enumerate(xs):
        x[0] = (RR - 1, 0, 1)[v % 3]
        x[-1] = (1, RR - 1, 0)[v % 3]
    return xs


def _check(res, m, xs, what):
    want = m.times(xs)
    got = _ints(res["out"])
    flat = [x * MONT % RR for row in want for x in row]
    assert len(got) == len(flat), what
    bad = [i for i in range(len(got)) if got[i] != flat[i]]
    assert not bad, "%s: %d of %d outputs differ, first (vector, row) = %s" % (what, len(bad), len(got), divmod(bad[0], len(m.rows)))


def _run_and_check(cases):
    """cases: (matrix, vectors, shape, label); one child for all of them"""
    results = child.run([m.job(xs, shape, label) for m, xs, shape, label in cases])
    for (m, xs, shape, label), res in zip(cases, results):
        _check(res, m, xs, "%s %s" % (label, shape))
    return results


@pytest.mark.parametrize("shape", SMALL)
def test_single_row(shape):
    """n_rows = 1, every length at which the tiling changes: 1, chunk +- 1, 64 chunk +- 1, tile - 1, tile, tile + 1, 2 tile + 3"""
    block, chunk = shape
    tile = block * chunk
    lengths = sorted({1, max(chunk - 1, 1), chunk + 1, 64 * chunk - 1, 64 * chunk + 1, tile - 1, tile, tile + 1, 2 * tile + 3})
    cases = []
    for n in lengths:
        m = _by_lengths([n], 37, 100 + n)
        cases.append((m, _vectors(1, 37, n), shape, "one row of %d" % n))
    results = _run_and_check(cases)
    for n, res in zip(lengths, results):
        assert res["kernels"] == ([TILE] if n <= tile else [TILE, FIXUP]), n
        assert not res["has_empty"]


@pytest.mark.parametrize("shape", SMALL)
def test_boundaries(shape):
    """rows that end exactly on a tile boundary, a row that begins exactly on one, a tile lying wholly inside one row, two crossing rows
    meeting in one tile, a partial last tile; k = 3"""
    block, chunk = shape
    T = block * chunk
    lengths = [T - 3, 3,                  # the second row ends at T exactly
               2 * T + 5,                 # begins at T exactly, tile 2 lies wholly inside it, ends at 3 T + 5
               T, T,                      # 3 T + 5 .. 4 T + 5 .. 5 T + 5: one row crossing into tile 4, the next one crossing out of it
               T - 5,                     # ends at 6 T exactly
               1, 2, chunk, chunk + 1, 7]  # a partial last tile
    m = _by_lengths(lengths, 50, 7)
    xs = _vectors(3, 50, 8)
    res = _run_and_check([(m, xs, shape, "boundaries")])[0]
    assert res["kernels"] == [TILE, FIXUP]
    # the first row of every tile, as the upload found it
    starts = np.cumsum([0] + lengths)
    want_rows = [int(np.searchsorted(starts, t * T, side="right") - 1) for t in range((m.nnz + T - 1) // T)] + [len(lengths) - 1]
    assert list(res["tile_row"]) == want_rows
    # the resident values are 2^5 val
    assert _ints(res["val_resident"]) == [x * 32 % RR for x in _ints(m.val)]


@pytest.mark.parametrize("shape", SMALL)
def test_empty_rows(shape):
    """empty rows first, last, three in a row, and at a tile boundary (behind a row that ends there and in front of one that begins
    there); the output starts as a pattern, so each of them must be written by somebody"""
    block, chunk = shape
    T = block * chunk
    lengths = [0, 0, 5, 0, 0, 0, T - 5, 0, 0, 3, T + 2, 0, 4, 0]
    m = _by_lengths(lengths, 20, 11)
    xs = _vectors(2, 20, 12)
    res = _run_and_check([(m, xs, shape, "empty rows")])[0]
    assert res["has_empty"] and res["kernels"] == [FILL, TILE, FIXUP]
    # all rows empty, and a matrix without any entry in a single row
    for lengths in ([0, 0, 0, 0, 0], [0]):
        m = _by_lengths(lengths, 9, 13)
        res = _run_and_check([(m, _vectors(3, 9, 14), shape, "nnz = 0")])[0]
        assert res["has_empty"] and res["kernels"] == [FILL]
        assert not res["out"].any()


def test_plan_launch_lists():
    """one tile: TILE alone; more than one: TILE, FIXUP; FILL first exactly when a row is empty or there is no entry at all"""
    shape = (64, 2)
    cases = [(_by_lengths([3, 4, 5], 10, 1), [TILE]), (_by_lengths([128], 10, 2), [TILE]), (_by_lengths([100, 29], 10, 3), [TILE, FIXUP]),
             (_by_lengths([3, 0, 5], 10, 4), [FILL, TILE]), (_by_lengths([100, 0, 29], 10, 5), [FILL, TILE, FIXUP]), (_by_lengths([0, 0], 10, 6), [FILL])]
    results = _run_and_check([(m, _vectors(1, 10, 9), shape, "plan %s" % want) for m, want in cases])
    for (m, want), res in zip(cases, results):
        assert res["kernels"] == want, (m.row_ptr, res["kernels"])


def test_columns_values_and_vectors():
    """repeated and unsorted columns, columns 0 and n_cols - 1, values 0, 1 and r - 1 in val and in x; k = 3, and changing vector 1 changes
    output 1 only"""
    shape = (64, 2)
    n_cols = 6
    rows = [[(5, RR - 1), (0, 1), (5, RR - 1), (3, 0), (0, RR - 1)],      # unsorted, repeated
            [(n_cols - 1, 1)],
            [(0, 0)],
            [(2, RR - 1)] * 130,                                   # one column repeated across a tile boundary
            [(4, 7), (1, 1), (4, RR - 7)]]                         # the repeats cancel
    m = Matrix(rows, n_cols)
    xs = [[0, 1, RR - 1, 5, 6, RR - 1], [RR - 1] * n_cols, [1, 0, 1, 0, 1, 0]]
    xs2 = [xs[0], [3, 1, 4, 1, 5, 9], xs[2]]
    r1, r2 = _run_and_check([(m, xs, shape, "values"), (m, xs2, shape, "values, vector 1 changed")])
    assert np.array_equal(r1["out"][0], r2["out"][0]) and np.array_equal(r1["out"][2], r2["out"][2])
    assert not np.array_equal(r1["out"][1], r2["out"][1])
    # k = 1 gives vector 0 of the k = 3 call
    r3 = _run_and_check([(m, xs[:1], shape, "k = 1")])[0]
    assert np.array_equal(r3["out"][0], r1["out"][0])


@pytest.mark.parametrize("shape", SMALL)
def test_mixed(shape):
    """200 rows of 1-5 entries around one row of five tiles"""
    block, chunk = shape
    T = block * chunk
    r = o.SplitMix64(T)
    lengths = [1 + r.next() % 5 for _ in range(200)]
    lengths[77] = 5 * T
    m = _by_lengths(lengths, 300, 21)
    res = _run_and_check([(m, _vectors(3 if shape == SMALL[0] else 1, 300, 22), shape, "mixed")])[0]
    assert res["kernels"] == [TILE, FIXUP]


def test_shipped_shape():
    """the plan's real 256 lanes x 8 entries: short rows, empty rows and one row of two tiles and a bit, k = 2"""
    T = child.SHIPPED[0] * child.SHIPPED[1]
    r = o.SplitMix64(2048)
    lengths = [r.next() % 6 for _ in range(300)]
    lengths[0] = 0
    lengths[150] = 2 * T + 7
    lengths[-1] = 0
    m = _by_lengths(lengths, 257, 31)
    res = _run_and_check([(m, _vectors(2, 257, 32), child.SHIPPED, "shipped")])[0]
    assert res["kernels"] == [FILL, TILE, FIXUP]


def test_validation_kernel():
    """k_frsp_validate's verdict: 0 for a good matrix, and the bit of each fault -- order (1), column (2), value (4), first entry (8)"""
    good = _by_lengths([3, 0, 300, 2], 10, 41)

    def job(label, **change):
        j = {"op": "validate", "row_ptr": good.row_ptr.copy(), "col": good.col.copy(), "val": good.val.copy(), "n_cols": 10, "label": label}
        for key, (pos, v) in change.items():
            j[key][pos] = v
        return j

    r_words = np.frombuffer(RR.to_bytes(32, "little"), dtype=np.uint32)
    rm1_words = np.frombuffer((RR - 1).to_bytes(32, "little"), dtype=np.uint32)
    jobs = [job("good"), job("order", row_ptr=(2, 2)), job("column", col=(304, 10)), job("value", val=(7, r_words)), job("first", row_ptr=(0, 1)),
            job("largest value", val=(7, rm1_words)), job("largest column", col=(0, 9))]
    flags = [res["flag"] for res in child.run(jobs)]
    assert flags == [0, 1, 2, 4, 8, 0, 0]
