"""Same-process timing of the sparse matrix-vector product over Fr (blsgpu_fr_spmv_device) against the chain the library's other entry
points would need for the arithmetic alone.

    python tools/fr_spmv_time.py [--window-ms T] [--windows W] [--out profiles/fr_spmv_time.json]

Times are HIP events on the stream the calls are enqueued on (the context is put on a torch stream with set_stream): one pair of events
around R back-to-back device-form calls, after warm-up calls of the same shape; R is chosen per measurement from a first short window
so that a window lasts at least T ms (default 100; `reps` is recorded with every figure); W such windows, the minimum and all of them
are recorded, per call.  The product alternates between TWO right-hand sides, the yardstick multiplies TWO different arrays.

The yardstick, at the shape's own nnz: `fr_op_device` mul over nnz elements plus `fr_scan_many_device` SUM with k = 1 over nnz elements --
the arithmetic of the product through existing entry points, WITHOUT the gather of x[col] and without the differences of the row ends
(which flatters the yardstick).  It moves 192 bytes per non-zero; the product reads at most 68 (value, column, gathered x) plus the output.

Shapes (n = 2^20 rows and columns):
  (a) banded    4 entries per row, columns within +-64 of the row index (the locality of a compiled circuit); nnz = 2^22
  (b) long_rows (a) plus 16 rows of 2^16 entries each, spread over the matrix
  (c) uniform   as (a) with uniformly random columns: recorded only -- its cost is the memory system's (x misses L2)
`vs_chain` = product time / chain time; the requirement is vs_chain <= 1 on (a) and (b).  64 outputs per shape are checked against Python
integers (`outputs_match`).  No test asserts any of these figures."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 1 << 20
R_ORDER = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
R_INV = pow(1 << 256, -1, R_ORDER)


def matrix(shape, rs):
    """row_ptr, col (u32), n_rows"""
    rows = np.repeat(np.arange(N, dtype=np.int64), 4)
    if shape == "uniform":
        col = rs.randint(0, N, size=4 * N)
    else:
        col = np.clip(rows + rs.randint(-64, 65, size=4 * N), 0, N - 1)
    lengths = np.full(N, 4, dtype=np.int64)
    if shape == "long_rows":
        at = (np.arange(16) * (N // 16) + 12345)                   # a long row in front of row at[i]
        lengths = np.insert(lengths, at, 1 << 16)
        starts = np.concatenate([[0], np.cumsum(lengths)])
        pos = at + np.arange(16)                                   # their indices in the new matrix
        col = np.insert(col, np.repeat(at * 4, 1 << 16), rs.randint(0, N, size=16 << 16))
        assert all(starts[p + 1] - starts[p] == 1 << 16 for p in pos)
    row_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint32)
    return row_ptr, col.astype(np.uint32), len(lengths)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bls12_381_amd as b
    ctx = b.Context(0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    ctx.set_stream(stream.cuda_stream)

    def window(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for i in range(reps):
            fn(i)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    def timed(fn):
        """(per-call ms of every window, calls per window)"""
        fn(0), fn(1)                                               # warm-up
        ctx.synchronize()
        reps = max(4, min(20000, int(1.1 * a.window_ms / max(window(fn, 4), 1e-4)) + 1))
        return [window(fn, reps) for _ in range(a.windows)], reps

    def scalars_np(n, seed):
        x = np.random.RandomState(seed).randint(0, 256, size=(n, 32), dtype=np.uint8)
        x[:, 31] &= 0x3F                                           # < 2^254 < r: canonical limbs
        return x.view(np.uint64).reshape(n, 4)

    def to_dev(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).to(dev)

    def ints(x):
        raw = np.ascontiguousarray(x).tobytes()
        return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]

    rec = {"window_ms": a.window_ms, "windows": a.windows, "n": N, "chain_bytes_per_nnz": 192, "product_bytes_per_nnz": 68, "shapes": {}}
    ok = True
    for shape in ("banded", "long_rows", "uniform"):
        rs = np.random.RandomState(len(shape))
        row_ptr, col, n_rows = matrix(shape, rs)
        nnz = len(col)
        val = scalars_np(nnz, 11)
        xs = [scalars_np(N, 12), scalars_np(N, 13)]
        m = ctx.fr_matrix(row_ptr, col, val, N)
        d_x = [to_dev(x) for x in xs]
        d_out = torch.empty((n_rows, 4), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        t, reps = timed(lambda i: ctx.fr_spmv_device(m, d_x[i & 1].data_ptr(), 1, d_out.data_ptr()))
        row = {"n_rows": n_rows, "n_cols": N, "nnz": nnz, "k": 1, "ms": min(t), "ms_all": t, "reps": reps, "nnz_per_s": nnz / min(t) * 1e3,
               "gb_per_s_at_68_bytes": (nnz * 68 + n_rows * 32) / min(t) / 1e6}
        # 64 outputs of the last call (x = xs[(reps - 1) & 1]) against Python integers
        ctx.synchronize()
        got = d_out.cpu().numpy().view(np.uint64)
        x_used = xs[(reps - 1) & 1]
        same = True
        for i in [0, n_rows - 1] + rs.randint(0, n_rows, size=62).tolist() + ([12345, 12345 + N // 16 + 1] if shape == "long_rows" else []):
            lo, hi = int(row_ptr[i]), int(row_ptr[i + 1])
            want = sum(v * xv for v, xv in zip(ints(val[lo:hi]), ints(x_used[col[lo:hi]]))) * R_INV % R_ORDER
            same = same and ints(got[i])[0] == want
        row["outputs_match"] = same
        ok = ok and same
        # k = 3 on the same matrix: the matrix is read once for all three
        d_x3 = [to_dev(np.concatenate([xs[0], xs[1], xs[0]])), to_dev(np.concatenate([xs[1], xs[0], xs[1]]))]
        d_out3 = torch.empty((3 * n_rows, 4), dtype=torch.int64, device=dev)
        t3, reps3 = timed(lambda i: ctx.fr_spmv_device(m, d_x3[i & 1].data_ptr(), 3, d_out3.data_ptr()))
        row.update({"k3_ms": min(t3), "k3_ms_all": t3, "k3_reps": reps3})
        del d_x3, d_out3
        # the yardstick at this nnz
        d_a, d_b = to_dev(val), to_dev(scalars_np(nnz, 14))
        d_p, d_s = torch.empty_like(d_a), torch.empty_like(d_a)
        torch.cuda.synchronize()
        tm, rm = timed(lambda i: ctx.fr_op_device(0, d_a.data_ptr(), d_b.data_ptr(), nnz, d_p.data_ptr()))
        ts, rsn = timed(lambda i: ctx.fr_scan_device(0, d_p.data_ptr(), nnz, 1, d_s.data_ptr()))
        tc, rc_ = timed(lambda i: (ctx.fr_op_device(0, d_a.data_ptr(), d_b.data_ptr(), nnz, d_p.data_ptr()), ctx.fr_scan_device(0, d_p.data_ptr(), nnz, 1, d_s.data_ptr())))
        row.update({"fr_op_mul_ms": min(tm), "fr_op_mul_ms_all": tm, "fr_op_mul_reps": rm, "fr_scan_sum_ms": min(ts), "fr_scan_sum_ms_all": ts, "fr_scan_sum_reps": rsn,
                    "chain_ms": min(tc), "chain_ms_all": tc, "chain_reps": rc_, "vs_chain": min(t) / min(tc), "required": shape != "uniform"})
        rec["shapes"][shape] = row
        print(shape, json.dumps({q: row[q] for q in row if not q.endswith("_all")}), flush=True)
        m.close()
        del d_a, d_b, d_p, d_s, d_x, d_out
    ctx.set_stream(None)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
