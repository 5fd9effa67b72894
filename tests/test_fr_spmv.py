"""Sparse matrix-vector products over Fr (`blsgpu_fr_matrix_*`, `blsgpu_fr_spmv*`; csrc/fr_spmv.hip.h + csrc/fr_spmv_plan.h) on the GPU.

Expectations are Python integers mod r on the RAW limbs: a `Scalar`'s limbs are a = v R mod r, the product of two Montgomery forms is
a b / R, and sums are linear, so out_raw[i] = (sum_p val_raw[p] x_raw[col[p]]) / R mod r.  Results are compared limb for limb: a
non-canonical output does not compare equal.  Every matrix that is multiplied went through an upload that validated it; the refused
uploads return before a handle exists."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import bls12_381_ref as o

pytestmark = pytest.mark.gpu

RR = o.R_ORDER
MONT = o.FR_MONT_R
RINV = pow(MONT, -1, RR)
ERR_ARG = -2
BLOCK, CHUNK = 256, 8                                              # csrc/fr_spmv_plan.h: FRSP_BLOCK, FRSP_CHUNK
T = BLOCK * CHUNK                                                  # the shipped tile: non-zeros per workgroup


@pytest.fixture(scope="module")
def ctx():
    import bls12_381_amd as b
    c = b.Context(0)
    yield c
    c.close()


def _limbs(vals):
    """integers mod r -> (len, 4) u64 Montgomery limbs"""
    b = b"".join((int(v) % RR * MONT % RR).to_bytes(32, "little") for v in vals)
    return np.frombuffer(b, dtype=np.uint64).reshape(-1, 4).copy()


def _from_raw(ints):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in ints), dtype=np.uint64).reshape(-1, 4).copy()


def _raw(n, seed):
    """n canonical `Scalar`s as raw limbs (any integer below r is the Montgomery form of some scalar)"""
    s = np.random.RandomState(seed).randint(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= 0x3F                                               # < 2^254 < r
    return s.view(np.uint64).reshape(n, 4).copy()


def _raw_ints(a):
    b = np.ascontiguousarray(a).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def _special(a):
    """0, 1 and r - 1 (as raw limbs) among the first elements"""
    if len(a) >= 3:
        a[:3] = _from_raw([0, MONT % RR, (RR - 1) * MONT % RR])
    return a


def _csr(lengths, n_cols, seed, banded=False):
    """row_ptr, col (u32) for the given row lengths: random columns, or the row index and its neighbours (banded)"""
    row_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint32)
    nnz = int(row_ptr[-1])
    if banded:
        rows = np.repeat(np.arange(len(lengths)), lengths)
        col = ((rows + np.arange(nnz) - row_ptr[rows].astype(np.int64) - 1) % n_cols).astype(np.uint32)
    else:
        col = np.random.RandomState(seed).randint(0, n_cols, size=nnz).astype(np.uint32)
        if nnz:
            col[0], col[-1] = 0, n_cols - 1
    return row_ptr, col


def _expect(row_ptr, col, val_raw, x_raw, n_cols):
    """the product on raw limbs, as a (k, n_rows, 4) array; x_raw: k * n_cols integers"""
    k = len(x_raw) // n_cols
    out = []
    for v in range(k):
        x = x_raw[v * n_cols:(v + 1) * n_cols]
        prod = [a * x[c] for a, c in zip(val_raw, col.tolist())]
        out += [sum(prod[row_ptr[i]:row_ptr[i + 1]]) * RINV % RR for i in range(len(row_ptr) - 1)]
    return _from_raw(out).reshape(k, len(row_ptr) - 1, 4)


def _case(name):
    rs = np.random.RandomState(len(name))
    if name == "one":
        return [1], 1, False
    if name == "random":
        return rs.randint(0, 6, size=1000).tolist(), 777, False
    if name == "long row":
        return [1, 2 * T + 7, 1], 50, False
    if name == "banded":
        return [3] * 4096, 4096, True
    lengths = rs.randint(1, 7, size=1 << 14)
    lengths[5000] = lengths[12345] = 1 << 15
    return lengths.tolist(), 1 << 14, False


@pytest.mark.parametrize("name,k", [("one", 1), ("random", 1), ("random", 4), ("long row", 1), ("banded", 1), ("banded", 4), ("large", 1)])
def test_against_python_integers(ctx, name, k):
    lengths, n_cols, banded = _case(name)
    row_ptr, col = _csr(lengths, n_cols, 17, banded)
    val = _special(_raw(len(col), 3))
    x = _special(_raw(k * n_cols, 4 + k)).reshape(k, n_cols, 4)
    m = ctx.fr_matrix(row_ptr, col, val, n_cols)
    assert (m.rows, m.cols, m.nnz) == (len(lengths), n_cols, len(col))
    got = ctx.fr_spmv(m, x)
    want = _expect(row_ptr.tolist(), col, _raw_ints(val), _raw_ints(x), n_cols)
    bad = np.argwhere((got != want).any(axis=2))
    assert not len(bad), "%s k=%d: %d outputs differ, first (vector, row) %s" % (name, k, len(bad), bad[0])
    assert np.array_equal(ctx.fr_spmv(m, x[0]), got[0])            # a (n_cols, 4) array is k = 1
    m.close()
    assert m.handle is None and m.rows == 0


@pytest.fixture(scope="module")
def mixed(ctx):
    """a matrix with empty rows, short rows and one row across three tiles, its host-form product for k = 3, shared and never modified"""
    rs = np.random.RandomState(9)
    lengths = rs.randint(0, 6, size=3000)
    lengths[0] = lengths[-1] = 0
    lengths[1500] = 2 * T + 100
    n_cols = 2000
    row_ptr, col = _csr(lengths.tolist(), n_cols, 5)
    val = _raw(len(col), 6)
    x = _raw(3 * n_cols, 7).reshape(3, n_cols, 4)
    m = ctx.fr_matrix(row_ptr, col, val, n_cols)
    want = ctx.fr_spmv(m, x)
    assert np.array_equal(want, _expect(row_ptr.tolist(), col, _raw_ints(val), _raw_ints(x), n_cols))
    yield {"row_ptr": row_ptr, "col": col, "val": val, "x": x, "m": m, "want": want, "n_cols": n_cols, "n_rows": len(lengths)}
    m.close()


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    view = a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32)
    return torch.from_numpy(view.copy()).to(torch.device("cuda", 0))


def test_host_form_equals_device_form(ctx, mixed):
    """a matrix made resident from device arrays, multiplied through the device form, against the host forms of both"""
    import torch
    d_rp, d_col, d_val, d_x = _dev(mixed["row_ptr"]), _dev(mixed["col"]), _dev(mixed["val"]), _dev(mixed["x"])
    d_out = torch.full((3 * mixed["n_rows"], 4), 0x5A5A, dtype=torch.int64, device=d_x.device)
    torch.cuda.synchronize()
    m2 = ctx.fr_matrix_from_device(d_rp.data_ptr(), d_col.data_ptr(), d_val.data_ptr(), mixed["n_rows"], mixed["n_cols"])
    assert (m2.rows, m2.cols, m2.nnz) == (mixed["m"].rows, mixed["m"].cols, mixed["m"].nnz)
    d_rp.zero_(), d_col.zero_(), d_val.zero_()                     # the handle keeps its own copy
    torch.cuda.synchronize()
    ctx.fr_spmv_device(m2, d_x.data_ptr(), 3, d_out.data_ptr())
    ctx.synchronize()
    assert np.array_equal(d_out.cpu().numpy().view(np.uint64).reshape(3, -1, 4), mixed["want"])
    assert np.array_equal(d_x.cpu().numpy().view(np.uint64).reshape(3, -1, 4), mixed["x"])
    assert np.array_equal(ctx.fr_spmv(m2, mixed["x"]), mixed["want"])
    m2.close()


def test_on_a_caller_stream_behind_a_producer(ctx, mixed):
    """set_stream(side): the product is ordered behind the fr_op_device call on the same stream that produces its x (x = 2 * half)"""
    import torch
    dev = torch.device("cuda", 0)
    x = mixed["x"].reshape(-1, 4)
    half = _from_raw([a * pow(2, -1, RR) % RR for a in _raw_ints(x)])
    d_half = _dev(half)
    d_x = torch.zeros((len(x), 4), dtype=torch.int64, device=dev)
    d_out = torch.zeros((3 * mixed["n_rows"], 4), dtype=torch.int64, device=dev)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    ctx.set_stream(side.cuda_stream)
    try:
        ctx.fr_op_device(6, d_half.data_ptr(), None, len(x), d_x.data_ptr())
        ctx.fr_spmv_device(mixed["m"], d_x.data_ptr(), 3, d_out.data_ptr())
        ctx.synchronize()
    finally:
        ctx.set_stream(None)
    assert np.array_equal(d_out.cpu().numpy().view(np.uint64).reshape(3, -1, 4), mixed["want"])


def test_one_handle_twenty_calls(ctx, mixed):
    import torch
    d_x = _dev(mixed["x"])
    d_out = torch.zeros((20, 3 * mixed["n_rows"], 4), dtype=torch.int64, device=d_x.device)
    torch.cuda.synchronize()
    for i in range(20):
        ctx.fr_spmv_device(mixed["m"], d_x.data_ptr(), 3, d_out[i].data_ptr())
    ctx.synchronize()
    got = d_out.cpu().numpy().view(np.uint64)
    for i in range(20):
        assert np.array_equal(got[i].reshape(3, -1, 4), mixed["want"]), i


def _r1cs(n, seed):
    """random A, B (three entries per row) and z, and C with one entry per row such that (A z) o (B z) = C z; as the stacked 3n-row CSR"""
    r = o.SplitMix64(seed)
    z = [r.scalar() or 1 for _ in range(n)]
    rows = []
    for _ in range(2 * n):
        rows.append([(r.next() % n, r.scalar()) for _ in range(3)])
    az = [sum(v * z[c] for c, v in row) % RR for row in rows[:n]]
    bz = [sum(v * z[c] for c, v in row) % RR for row in rows[n:]]
    for i in range(n):
        j = r.next() % n
        rows.append([(j, az[i] * bz[i] % RR * pow(z[j], -1, RR) % RR)])
    row_ptr = np.cumsum([0] + [len(row) for row in rows]).astype(np.uint32)
    col = np.array([c for row in rows for c, _ in row], dtype=np.uint32)
    return row_ptr, col, [v for row in rows for _, v in row], z


def test_constraint_system_round_trip(ctx):
    """n = 256: one fr_spmv on the stacked 768-row matrix, then fr_op mul and sub: (A z) o (B z) - C z is all zeros, and is not with one
    entry of z changed"""
    n = 256
    row_ptr, col, vals, z = _r1cs(n, 0xC5)
    m = ctx.fr_matrix(row_ptr, col, vals, n)                       # integer values, accepted as fr_scan's points are
    assert (m.rows, m.cols, m.nnz) == (3 * n, n, 7 * n)
    for change, zero in ((False, True), (True, False)):
        zz = list(z)
        if change:
            zz[int(col[0])] = (zz[int(col[0])] + 1) % RR           # a column that row 0 of A reads
        abc = ctx.fr_spmv(m, _limbs(zz))
        rest = ctx.fr_op(2, ctx.fr_op(0, abc[:n], abc[n:2 * n]), abc[2 * n:])
        assert (not rest.any()) == zero
    m.close()


def test_chain_into_the_transform_without_a_host_copy(ctx):
    """fr_spmv_device -> fr_ntt_many_device on the same buffer: three stacked 256-row blocks are three vectors of 2^8 for the transform"""
    import torch
    n = 256
    row_ptr, col, vals, z = _r1cs(n, 0x7E)
    m = ctx.fr_matrix(row_ptr, col, vals, n)
    x = _limbs(z)
    want = ctx.fr_ntt_many(ctx.fr_spmv(m, x).reshape(3, n, 4))
    d_x = _dev(x)
    d_abc = torch.zeros((3 * n, 4), dtype=torch.int64, device=d_x.device)
    torch.cuda.synchronize()
    ctx.fr_spmv_device(m, d_x.data_ptr(), 1, d_abc.data_ptr())
    ctx.fr_ntt_many_device(d_abc.data_ptr(), 8, 3)
    ctx.synchronize()
    assert np.array_equal(d_abc.cpu().numpy().view(np.uint64).reshape(3, n, 4), want)
    m.close()


def test_refused_uploads(ctx):
    """every malformed matrix is BLSGPU_ERR_ARG from BOTH upload forms, the handle stays NULL and the message names the offender; they
    return before a handle exists, so nothing is ever multiplied with them"""
    import torch
    lib, h = ctx.lib, ctx.h
    n_rows, n_cols = 6, 10
    good_rp = np.array([0, 2, 2, 5, 6, 9, 12], dtype=np.uint32)
    good_col = np.array([0, 9, 3, 3, 4, 1, 7, 8, 9, 0, 5, 2], dtype=np.uint32)
    good_val = _special(_raw(12, 8))
    r_limbs = _from_raw([RR])[0]
    err = lambda: lib.blsgpu_last_error().decode()

    def cases():
        rp = good_rp.copy(); rp[0] = 1
        yield "row_ptr[0] != 0", rp, good_col, good_val, "row_ptr[0]"
        rp = good_rp.copy(); rp[3] = 1
        yield "a decreasing row_ptr", rp, good_col, good_val, "decreases at row 2"
        rp = good_rp.copy(); rp[-1] = (1 << 28) + 1                # the last entry IS the number of non-zeros: all the ABI can check is its range
        yield "last entry out of range", rp, good_col, good_val, "2^28"
        rp = good_rp.copy(); rp[-1] = 8                            # below the entry in front of it
        yield "last entry below the one before", rp, good_col, good_val, "decreases at row 5"
        cl = good_col.copy(); cl[7] = n_cols
        yield "col = n_cols", good_rp, cl, good_val, "col[7]"
        vl = good_val.copy(); vl[4] = r_limbs
        yield "val = r", good_rp, good_col, vl, "val[4]"

    for what, rp, cl, vl, needle in cases():
        out = ctypes.c_void_p(0x1234)
        rc = lib.blsgpu_fr_matrix_upload(h, n_rows, n_cols, rp.ctypes.data, cl.ctypes.data, vl.ctypes.data, ctypes.byref(out))
        assert rc == ERR_ARG and out.value is None and needle in err(), (what, "host", rc, err())
        d_rp, d_cl, d_vl = _dev(rp), _dev(cl), _dev(vl)
        torch.cuda.synchronize()
        out = ctypes.c_void_p(0x1234)
        rc = lib.blsgpu_fr_matrix_from_device(h, n_rows, n_cols, d_rp.data_ptr(), d_cl.data_ptr(), d_vl.data_ptr(), ctypes.byref(out))
        assert rc == ERR_ARG and out.value is None and needle in err(), (what, "device", rc, err())
    out = ctypes.c_void_p(0x1234)
    assert lib.blsgpu_fr_matrix_upload(h, n_rows, n_cols, None, good_col.ctypes.data, good_val.ctypes.data, ctypes.byref(out)) == ERR_ARG and out.value is None
    assert lib.blsgpu_fr_matrix_upload(h, (1 << 28) + 1, n_cols, good_rp.ctypes.data, good_col.ctypes.data, good_val.ctypes.data, ctypes.byref(out)) == ERR_ARG
    d_rp, d_cl, d_vl = _dev(good_rp), _dev(good_col), _dev(good_val)
    assert lib.blsgpu_fr_matrix_from_device(h, n_rows, n_cols, d_rp.data_ptr(), d_cl.data_ptr(), d_vl.data_ptr() + 8, ctypes.byref(out)) == ERR_ARG and "aligned" in err()
    # the Python form knows the array lengths and refuses a last entry that is not len(col)
    with pytest.raises(ValueError):
        ctx.fr_matrix(good_rp, good_col[:-1], good_val[:-1], n_cols)
    with pytest.raises(Exception):
        ctx.fr_matrix(good_rp, good_col, [RR] * 12, n_cols)
    # the largest legal values pass, and the good matrix works afterwards
    cl = good_col.copy(); cl[7] = n_cols - 1
    vl = good_val.copy(); vl[4] = _from_raw([RR - 1])[0]
    m = ctx.fr_matrix(good_rp, cl, vl, n_cols)
    x = _raw(n_cols, 1)
    assert np.array_equal(ctx.fr_spmv(m, x), _expect(good_rp.tolist(), cl, _raw_ints(vl), _raw_ints(x), n_cols)[0])
    m.close()


def test_refused_products(ctx, mixed):
    """every refusal is BLSGPU_ERR_ARG before anything is staged or launched: the output keeps its pattern; k == 0 is a no-op"""
    import torch
    lib, h, m = ctx.lib, ctx.h, mixed["m"]
    n_rows, n_cols = mixed["n_rows"], mixed["n_cols"]
    err = lambda: lib.blsgpu_last_error().decode()
    x = mixed["x"][0].copy()
    y = np.full((n_rows, 4), 0x77, dtype=np.uint64)
    dev = torch.device("cuda", 0)
    # one device buffer that holds x followed by room for out, so that overlapping ranges can be named
    d_buf = torch.full((n_cols + n_rows + 8, 4), 0x77, dtype=torch.int64, device=dev)
    d_buf[:n_cols] = _dev(x)
    torch.cuda.synchronize()
    keep = d_buf.cpu().numpy().copy()
    px, py = x.ctypes.data, y.ctypes.data
    dx, dy = d_buf.data_ptr(), d_buf.data_ptr() + n_cols * 32
    for fn, a, b in ((lib.blsgpu_fr_spmv, px, py), (lib.blsgpu_fr_spmv_device, dx, dy)):
        assert fn(h, None, a, 1, b) == ERR_ARG and "NULL matrix" in err()
        assert fn(h, m.handle, None, 1, b) == ERR_ARG and "NULL" in err()
        assert fn(h, m.handle, a, 1, None) == ERR_ARG and "NULL" in err()
        assert fn(h, m.handle, a, (1 << 28) // n_rows + 1, b) == ERR_ARG and "2^28" in err()      # k * max(n_rows, n_cols) > 2^28
        assert fn(h, m.handle, a, (1 << 63) + 1, b) == ERR_ARG and "2^28" in err()                # k * n overflows 64 bits
        assert fn(h, m.handle, a, 0, b) == 0 and fn(h, m.handle, None, 0, None) == 0
    # any overlap of out with x: out == x, out inside x, out ending inside x, x inside out
    for off in (0, 32, (n_cols - 1) * 32, -32, -(n_rows - 1) * 32):
        assert lib.blsgpu_fr_spmv_device(h, m.handle, dx, 1, dx + off) == ERR_ARG and "overlap" in err(), off
    xx = np.zeros((n_cols + n_rows, 4), dtype=np.uint64)
    assert lib.blsgpu_fr_spmv(h, m.handle, xx.ctypes.data, 1, xx.ctypes.data + 64) == ERR_ARG and "overlap" in err()
    assert lib.blsgpu_fr_spmv_device(h, m.handle, dx + 8, 1, dy) == ERR_ARG and "aligned" in err()
    assert lib.blsgpu_fr_spmv_device(h, m.handle, dx, 1, dy + 8) == ERR_ARG and "aligned" in err()
    ctx.synchronize()
    assert (y == 0x77).all() and np.array_equal(d_buf.cpu().numpy(), keep)
    with pytest.raises(ValueError):
        ctx.fr_spmv(m, np.zeros((n_cols + 1, 4), dtype=np.uint64))
    # adjacent ranges are fine, and the context still works
    assert lib.blsgpu_fr_spmv_device(h, m.handle, dx, 1, dy) == 0
    ctx.synchronize()
    assert np.array_equal(d_buf[n_cols:n_cols + n_rows].cpu().numpy().view(np.uint64), mixed["want"][0])


def test_cpp_mirror(ctx, tmp_path):
    """include/bls12_381.hpp FrMatrix / fr_spmv compiled with g++ against libblsgpu.so: every output against a host loop over bls::fr_op"""
    import bls12_381_amd as b
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "fr_spmv_test")
    libdir = os.path.dirname(b.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "fr_spmv_test.cpp"),
                           "-L" + libdir, "-lblsgpu", "-Wl,-rpath," + libdir, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "fr_spmv ok" in out.stdout, out.stdout + out.stderr
