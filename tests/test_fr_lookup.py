"""Fr lookup tables (`blsgpu_fr_lookup_*`; csrc/fr_lookup.hip.h + csrc/fr_lookup_plan.h) on the GPU.

Every case is compared with the Python dict of tests/fr_lookup_ref.py: the multiplicity column limb for limb (the raw 256-bit integers,
so a non-canonical scalar does not compare equal), the indices, the miss count and the number of distinct keys.  The end-to-end case
needs no reference: the multiplicities of a lookup instance, negated, close blsgpu_fr_frac_sum's logUp sum -- and no longer once one
looked-up value is outside the table."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import fr_lookup_ref as ref
from bls12_381_amd import synthetic
from oracle import bls12_381_ref as o

pytestmark = pytest.mark.gpu

RR = ref.RR
BLSGPU_OK, ERR_ARG = 0, -2
FR_MUL = 0                                                         # blsgpu_fr_op
MISS = ref.MISS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    import bls12_381_amd as b
    c = b.Context(0)
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda")


def host(t):
    return t.cpu().numpy().view(np.uint64)


def raw(shape, seed):
    """canonical scalars as raw limbs (any integer below r is the Montgomery form of some scalar): keys need no arithmetic"""
    n = int(np.prod(shape))
    s = np.random.RandomState(seed).randint(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= 0x3F
    return s.view(np.uint64).reshape(tuple(shape) + (4,)).copy()


def key_ints(limbs_):
    """(c, n, 4) limbs -> column set of raw integers (the reference compares tuples, whatever the integers stand for)"""
    return [ref.raw_ints(col) if col.shape[0] else [] for col in limbs_]


def device_count(ctx, lk, f, negate=False, outputs=("mult", "index", "missing"), pitch=None):
    """count_device on a (c, n, 4) array; returns (mult, missing, index), None for an output that was not asked for.  The outputs are
    pre-filled with a pattern, so an output that is not written shows"""
    import torch
    c, n = f.shape[0], f.shape[1]
    pitch = n if pitch is None else pitch
    buf = np.zeros(((c - 1) * pitch + n, 4), dtype=np.uint64)
    for j in range(c):
        buf[j * pitch:j * pitch + n] = f[j]
    d_f = dev(buf) if buf.shape[0] else torch.zeros((1, 4), dtype=torch.int64, device="cuda")
    d_mult = torch.full((lk.rows, 4), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    d_index = torch.full((max(n, 1),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    d_missing = torch.full((1,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    lk.count_device(d_f.data_ptr() if n else None, pitch, n, d_mult.data_ptr() if "mult" in outputs else None, d_index.data_ptr() if "index" in outputs else None,
                    d_missing.data_ptr() if "missing" in outputs else None, negate=negate)
    ctx.synchronize()
    pattern = lambda t: bool((t == 0x5A5A5A5A).all())
    for name, t in (("mult", d_mult), ("index", d_index), ("missing", d_missing)):
        assert name in outputs or pattern(t), "%s was written though it was not asked for" % name
    if buf.shape[0]:
        assert np.array_equal(host(d_f), buf), "f was written to"
    return (host(d_mult) if "mult" in outputs else None, int(host(d_missing)[0]) if "missing" in outputs else None,
            d_index.cpu().numpy().view(np.uint32)[:n] if "index" in outputs else None)


def check(ctx, table, f, negate=False, both=True):
    """a table and looked-up rows as (c, rows, 4) / (c, n, 4) limbs: the device form (and the host form, equal to it) against the reference"""
    want_mult, want_index, want_missing, want_distinct = ref.count(key_ints(table), key_ints(f))
    lk = ctx.fr_lookup(table)
    try:
        assert (lk.cols, lk.rows, lk.distinct, lk.slots) == (table.shape[0], table.shape[1], want_distinct, ref.slots(table.shape[1]))
        mult, missing, index = device_count(ctx, lk, f, negate)
        assert ref.raw_ints(mult) == ref.mult_raw(want_mult, negate), "mult differs"
        assert [int(x) for x in index] == want_index, "index differs"
        assert missing == want_missing
        if both:
            h_mult, h_missing, h_index = lk.count(f, negate=negate, return_index=True)
            assert np.array_equal(h_mult, mult) and h_missing == missing and np.array_equal(h_index, index), "the host form differs from the device form"
    finally:
        lk.close()
    return want_mult, want_index, want_missing


def instance(rows, n, c, seed, dup_every=0, miss_every=0):
    t, f, mult, index, missing = synthetic.lookup_tuple_instance(rows, n, c, seed, dup_every, miss_every)
    return ref.set_limbs(t), ref.set_limbs(f), mult, index, missing


def test_repeats_and_misses_in_both_forms(ctx):
    """rows = 1000, n = 5000, c = 1, every fifth table row a repeat, every seventh looked-up row a miss"""
    t, f, mult, index, missing = instance(1000, 5000, 1, 11, dup_every=5, miss_every=7)
    assert missing == 5000 // 7 and sum(1 for m in mult if m == 0) >= 1000 // 5 - 1
    got = check(ctx, t, f)
    assert got == (mult, index, missing), "synthetic.lookup_tuple_instance and the reference disagree"


@pytest.mark.parametrize("rows", [ref.LDS_ROWS, ref.LDS_ROWS + 1], ids=["lds_path", "cache_path"])
def test_either_side_of_the_path_threshold(ctx, rows):
    t, f, _, _, missing = instance(rows, 1 << 16, 3, 20 + rows, dup_every=9, miss_every=1000)
    assert missing == 65
    check(ctx, t, f, both=False)


@pytest.mark.parametrize("rows", [1 << 12, ref.LDS_ROWS + 1], ids=["lds_path", "cache_path"])
def test_every_lookup_on_one_row(ctx, rows):
    """n = 2^16 lookups all equal to row 3: m[3] = 65536, everything else 0"""
    t = raw((1, rows), 31)
    f = np.repeat(t[:, 3:4], 1 << 16, axis=1)
    lk = ctx.fr_lookup(t)
    mult, missing, index = device_count(ctx, lk, f)
    lk.close()
    want = [0] * rows
    want[3] = 65536
    assert ref.raw_ints(mult) == ref.mult_raw(want) and missing == 0 and (index == 3).all()


def test_a_table_of_identical_rows(ctx):
    t = np.repeat(raw((2, 1), 41), 4096, axis=1)
    f = np.concatenate([np.repeat(t[:, :1], 999, axis=1), raw((2, 1), 42)], axis=1)          # 999 hits and one miss
    lk = ctx.fr_lookup(t)
    assert lk.distinct == 1
    mult, missing, index = device_count(ctx, lk, f)
    lk.close()
    assert ref.raw_ints(mult) == ref.mult_raw([999] + [0] * 4095) and missing == 1
    assert (index[:999] == 0).all() and index[999] == MISS


def test_keys_that_differ_in_the_last_limb_of_the_last_column(ctx):
    rows, n = 5000, 20000
    t = np.repeat(raw((8, 1), 51), rows, axis=1)
    t[7, :, 3] = (t[7, 0, 3] & np.uint64(0x3FFFFFFF00000000)) | np.arange(rows, dtype=np.uint64)
    pick = np.random.RandomState(52).randint(0, rows + 500, size=n)                          # rows .. rows + 499: limbs no table row has
    f = np.repeat(t[:, :1], n, axis=1)
    f[7, :, 3] = (t[7, 0, 3] & np.uint64(0x3FFFFFFF00000000)) | pick.astype(np.uint64)
    _, index, missing = check(ctx, t, f, both=False)
    assert missing == int((pick >= rows).sum()) and index == [int(p) if p < rows else MISS for p in pick]


def test_negate_null_outputs_and_n_zero(ctx):
    t, f, mult, index, missing = instance(700, 3000, 2, 61, dup_every=4, miss_every=11)
    check(ctx, t, f, negate=True)
    lk = ctx.fr_lookup(t)
    for outs in ((), ("mult",), ("index",), ("missing",), ("mult", "index"), ("mult", "missing"), ("index", "missing")):
        m, s, i = device_count(ctx, lk, f, negate=True, outputs=outs)
        assert m is None or ref.raw_ints(m) == ref.mult_raw(mult, True), outs
        assert s is None or s == missing, outs
        assert i is None or [int(x) for x in i] == index, outs
    # n = 0: mult all zero, missing 0, in both forms and with negate
    empty = np.zeros((2, 0, 4), dtype=np.uint64)
    m, s, _ = device_count(ctx, lk, empty, negate=True, outputs=("mult", "missing"))
    assert not m.any() and s == 0
    hm, hs, hi = lk.count(empty, return_index=True)
    assert not hm.any() and hs == 0 and hi.shape == (0,)
    # a pitch beyond the column
    m, s, i = device_count(ctx, lk, f, pitch=3000 + 40)
    assert ref.raw_ints(m) == ref.mult_raw(mult) and s == missing and [int(x) for x in i] == index
    lk.close()


def test_two_calls_on_one_handle(ctx):
    """the counters are the handle's scratch, zeroed by every call: the second call on other rows is not the sum, and the first call
    repeated gives the first result"""
    t, f, mult, _, missing = instance(5000, 30000, 1, 71, dup_every=6, miss_every=13)
    f2 = f[:, ::-1][:, :7777].copy()
    lk = ctx.fr_lookup(t)
    a = device_count(ctx, lk, f)
    b = device_count(ctx, lk, f2)
    c = device_count(ctx, lk, f)
    lk.close()
    assert ref.raw_ints(a[0]) == ref.mult_raw(mult) and a[1] == missing
    assert np.array_equal(a[0], c[0]) and a[1] == c[1] and np.array_equal(a[2], c[2])
    assert ref.raw_ints(b[0]) == ref.mult_raw(ref.count(key_ints(t), key_ints(f2))[0])


def test_from_device_owns_its_copy(ctx):
    import torch
    rows, pitch = 3000, 3100
    t, f, mult, index, missing = instance(rows, 9000, 3, 81, dup_every=7, miss_every=10)
    buf = np.zeros((2 * pitch + rows, 4), dtype=np.uint64)
    for j in range(3):
        buf[j * pitch:j * pitch + rows] = t[j]
    d_t = dev(buf)
    torch.cuda.synchronize()
    lk = ctx.fr_lookup_from_device(3, d_t.data_ptr(), pitch, rows)
    d_t.fill_(0x1111)                                              # the caller's table is overwritten ...
    torch.cuda.synchronize()
    got = device_count(ctx, lk, f)                                 # ... and the results do not change
    assert lk.distinct == len(set(zip(*key_ints(t))))
    lk.close()
    assert ref.raw_ints(got[0]) == ref.mult_raw(mult) and got[1] == missing and [int(x) for x in got[2]] == index


def test_logup_end_to_end(ctx):
    """synthetic.lookup_instance(4096): m from count_device(negate = 1) goes with a ones column into fr_frac_sum_device (c = 2) and the
    row's last element is 0; with one looked-up value outside the table, missing is 1, its index the sentinel, and the sum no longer closes"""
    import torch
    n = 4096
    f, t, m = synthetic.lookup_instance(n)
    gamma = 0x0123456789ABCDEF0123
    lk = ctx.fr_lookup([t])
    d_chal = dev(ref.mont_limbs([0, gamma]))

    def run(f_vals):
        d_den = dev(np.concatenate([ref.mont_limbs(f_vals), ref.mont_limbs(t)]))             # den_a: the columns f and t, pitch n
        d_mult = dev(np.concatenate([ref.mont_limbs([1] * n), np.zeros((n, 4), dtype=np.uint64)]))
        d_index = torch.zeros((n,), dtype=torch.int32, device="cuda")
        d_missing = torch.zeros((1,), dtype=torch.int64, device="cuda")
        d_out = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        lk.count_device(d_den.data_ptr(), n, n, d_mult[n:].data_ptr(), d_index.data_ptr(), d_missing.data_ptr(), negate=True)
        ctx.fr_frac_sum_device(2, d_mult.data_ptr(), d_den.data_ptr(), None, n, d_chal.data_ptr(), n, 1, d_out.data_ptr())
        ctx.synchronize()
        return host(d_mult)[n:], d_index.cpu().numpy().view(np.uint32), int(host(d_missing)[0]), host(d_out)

    mult, index, missing, out = run(f)
    assert ref.raw_ints(mult) == ref.mult_raw(m, True) and missing == 0 and [t[j] for j in index] == f
    assert not out[-1].any() and out[n // 2].any()
    f_bad = list(f)
    f_bad[1234] = next(v for v in range(5, 5 + n + 1) if v not in set(t))
    mult, index, missing, out = run(f_bad)
    assert missing == 1 and index[1234] == MISS and (np.delete(index, 1234) != MISS).all()
    assert out[-1].any()
    lk.close()


def test_f_written_by_the_previous_call(ctx):
    """the looked-up rows are the output of an fr_op_device mul enqueued just before the count on the same stream, no synchronisation between"""
    import torch
    rows, n = 2000, 1 << 15
    rng = o.SplitMix64(91)
    x = [rng.scalar() for _ in range(rows)]
    y = rng.scalar()
    t_vals = [v * y % RR for v in x]
    pick = np.random.RandomState(92).randint(0, rows, size=n)
    lk = ctx.fr_lookup([t_vals])
    d_x = dev(ref.mont_limbs([x[p] for p in pick]))
    d_y = dev(np.repeat(ref.mont_limbs([y]), n, axis=0))
    d_f = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    d_mult = torch.zeros((rows, 4), dtype=torch.int64, device="cuda")
    d_missing = torch.ones((1,), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.fr_op_device(FR_MUL, d_x.data_ptr(), d_y.data_ptr(), n, d_f.data_ptr())
    lk.count_device(d_f.data_ptr(), n, n, d_mult.data_ptr(), None, d_missing.data_ptr())
    ctx.synchronize()
    lk.close()
    assert int(host(d_missing)[0]) == 0
    assert ref.raw_ints(host(d_mult)) == ref.mult_raw(np.bincount(pick, minlength=rows).tolist())


def test_arguments(ctx):
    """every refusal of the header comment is BLSGPU_ERR_ARG with a text naming the cause, before anything is staged or launched"""
    import torch
    lib, h = ctx.lib, ctx.h
    err = lambda: lib.blsgpu_last_error().decode()
    vp = ctypes.c_void_p
    rows, n, c = 100, 300, 2
    t, f = raw((c, rows), 1), raw((c, n), 2)
    d_t, d_f = dev(t.reshape(-1, 4)), dev(f.reshape(-1, 4))
    d_mult = torch.zeros((rows + 40, 4), dtype=torch.int64, device="cuda")      # room for an index (n * 4 bytes) flush against mult's end
    d_index = torch.zeros((n + 2,), dtype=torch.int32, device="cuda")
    d_missing = torch.zeros((2,), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    out = vp()

    def create(ctx_h=h, cc=c, tp=t.ctypes.data, r=rows, o_=ctypes.byref(out)):
        return lib.blsgpu_fr_lookup_create(ctx_h, cc, vp(tp) if tp else None, r, o_)

    def from_device(ctx_h=h, cc=c, tp=d_t.data_ptr(), pitch=rows, r=rows, o_=ctypes.byref(out)):
        return lib.blsgpu_fr_lookup_from_device(ctx_h, cc, vp(tp) if tp else None, pitch, r, o_)

    for make in (create, from_device):
        assert make(ctx_h=None) == ERR_ARG and "context" in err()
        assert make(o_=None) == ERR_ARG and "NULL" in err()
        assert make(cc=0) == ERR_ARG and "c must be" in err()
        assert make(cc=9) == ERR_ARG and "c must be" in err()
        assert make(r=0) == ERR_ARG and "rows" in err()
        assert make(r=(1 << 24) + 1) == ERR_ARG and "rows" in err()
        assert make(tp=None) == ERR_ARG and "NULL" in err()
        assert not out.value
    assert from_device(pitch=rows - 1) == ERR_ARG and "pitch" in err()
    assert from_device(pitch=1 << 63) == ERR_ARG and "2^28" in err()
    assert from_device(pitch=(1 << 28) - 50) == ERR_ARG and "2^28" in err()
    assert from_device(tp=d_t.data_ptr() + 8) == ERR_ARG and "aligned" in err()
    assert not out.value

    lk = ctx.fr_lookup(t)

    def count_device(ctx_h=h, handle=lk.handle, fp=d_f.data_ptr(), pitch=n, nn=n, negate=0, m=d_mult.data_ptr(), i=d_index.data_ptr(), s=d_missing.data_ptr()):
        p = lambda x: vp(x) if x else None
        return lib.blsgpu_fr_lookup_count_device(ctx_h, handle, p(fp), pitch, nn, negate, p(m), p(i), p(s))

    h_mult, h_index, h_missing = np.zeros((rows + 40, 4), dtype=np.uint64), np.zeros(n + 2, dtype=np.uint32), np.zeros(2, dtype=np.uint64)

    def count_host(ctx_h=h, handle=lk.handle, fp=f.ctypes.data, nn=n, negate=0, m=h_mult.ctypes.data, i=h_index.ctypes.data, s=h_missing.ctypes.data):
        p = lambda x: vp(x) if x else None
        return lib.blsgpu_fr_lookup_count(ctx_h, handle, p(fp), nn, negate, p(m), p(i), p(s))

    for call, fbase, mbase, ibase, sbase in ((count_device, d_f.data_ptr(), d_mult.data_ptr(), d_index.data_ptr(), d_missing.data_ptr()),
                                            (count_host, f.ctypes.data, h_mult.ctypes.data, h_index.ctypes.data, h_missing.ctypes.data)):
        assert call(ctx_h=None) == ERR_ARG and "context" in err()
        assert call(handle=None) == ERR_ARG and "handle" in err()
        assert call(fp=None) == ERR_ARG and "NULL" in err()
        assert call(negate=2) == ERR_ARG and "negate" in err()
        assert call(nn=(1 << 28) + 1) == ERR_ARG and "2^28" in err()
        assert call(m=fbase) == ERR_ARG and "overlaps f" in err()                            # mult on f's first column
        assert call(i=fbase + (2 * n - 1) * 32) == ERR_ARG and "overlaps f" in err()         # index on f's last scalar
        assert call(s=fbase + n * 32) == ERR_ARG and "overlaps f" in err()
        assert call(i=mbase + (rows - 1) * 32) == ERR_ARG and "each other" in err()          # index on mult's last scalar
        assert call(s=mbase) == ERR_ARG and "each other" in err()
        assert call(s=ibase + 4 * (n - 2)) == ERR_ARG and "each other" in err()              # missing on index's last two words
        assert call(i=mbase + rows * 32, s=sbase) == BLSGPU_OK                               # flush against mult's end: no overlap
        ctx.synchronize()
    assert count_device(pitch=n - 1) == ERR_ARG and "pitch" in err()
    assert count_device(pitch=1 << 63) == ERR_ARG and "2^28" in err()
    assert count_device(pitch=(1 << 28) - 10) == ERR_ARG and "2^28" in err()
    assert count_device(fp=d_f.data_ptr() + 8) == ERR_ARG and "aligned" in err()
    assert count_device(m=d_mult.data_ptr() + 8) == ERR_ARG and "aligned" in err()
    assert count_device(i=d_index.data_ptr() + 2) == ERR_ARG and "4-byte" in err()
    assert count_device(s=d_missing.data_ptr() + 4) == ERR_ARG and "8-byte" in err()
    # nothing was launched by a refused call: the outputs still hold what the last good call wrote
    before = host(d_mult).copy()
    assert count_device(negate=7) == ERR_ARG
    ctx.synchronize()
    assert np.array_equal(host(d_mult), before)
    with pytest.raises(ValueError):
        lk.count(f[:1])
    lk.close()



def test_cpp_mirror(ctx, tmp_path):
    """include/bls12_381.hpp FrLookup compiled with g++ against libblsgpu.so: counts, indices and misses against a host map"""
    import bls12_381_amd as b
    exe = str(tmp_path / "fr_lookup_test")
    libdir = os.path.dirname(b.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "fr_lookup_test.cpp"),
                           "-L" + libdir, "-lblsgpu", "-Wl,-rpath," + libdir, "-o", exe])
    out = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "fr_lookup ok" in out.stdout, out.stdout + out.stderr
