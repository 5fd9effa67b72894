"""Same-process timing of the Fr lookup tables (blsgpu_fr_lookup_count_device) against the two yardsticks the call is judged by.

    python tools/fr_lookup_time.py [--calls 10] [--windows 3] [--out profiles/fr_lookup_time.json] [--quick]

Times are HIP events on the stream the calls are enqueued on (the context is put on a torch stream with set_stream): one pair of events
around `calls` back-to-back calls (default 10), after a warm-up call of the same shape; W such windows, the minimum and all of them are
recorded, per call.  Tables of 2^8 / 2^12 / 2^16 / 2^20 rows x n = 2^20 / 2^24 looked-up rows x c = 1 and 3, every call with all three
outputs (mult, index, missing), and three distributions of the looked-up rows:

  uniform   every row drawn uniformly from the table
  one_row   every row equal to one table row
  hot16     90 % of the rows on 16 seeded table rows, the rest uniform

Before anything is timed the multiplicities are checked on the device against torch.bincount of the drawn row numbers (mult times the
raw integer 1 is the count itself: the Montgomery product divides by R), the indices against the row numbers, and missing against 0; a
mismatch ends the run with status 1.  Per table size the build (blsgpu_fr_lookup_from_device, a setup call that allocates and
synchronises) is timed on the host clock.

The yardsticks, in the same run:
  (1) the host route the call replaces, end to end on the host clock: device-to-host copy of f, numpy.unique on a byte view of the rows,
      the join against the (pre-sorted) table, the counts to Montgomery limbs with Python integers (one conversion per distinct count),
      host-to-device copy of m.  Its m is compared with the call's for equality.  It is run once per shape at n = 2^20 and, because the
      sort alone takes tens of seconds there, at ONE shape of n = 2^24 (2^12 rows, c = 1, uniform).
  (2) `fr_op_device` mul over n * c elements: the floor for reading f once (`vs_fr_op_mul`).

No test asserts any of these figures."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOG_ROWS = [8, 12, 16, 20]
LOG_NS = [20, 24]
CS = [1, 3]
DISTS = ["uniform", "one_row", "hot16"]
FR_MUL = 0                                                         # blsgpu_fr_op
R_ORDER = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
MONT_R = (1 << 256) % R_ORDER


def host_route(d_f, table_sorted, table_order, rows, dev):
    """the route without the call: f to the host, unique rows with counts, join, Montgomery limbs, m back to the device"""
    import numpy as np
    import torch
    c, n = d_f.shape[0], d_f.shape[1]
    f = d_f.cpu().numpy()                                                                    # device -> host (synchronises)
    fv = np.ascontiguousarray(f.transpose(1, 0, 2)).reshape(n, c * 4).view(np.dtype((np.void, 32 * c))).reshape(n)
    uniq, counts = np.unique(fv, return_counts=True)
    pos = np.minimum(np.searchsorted(table_sorted, uniq), rows - 1)
    hit = table_sorted[pos] == uniq
    m = np.zeros((rows, 4), dtype=np.uint64)
    limbs = {}
    for v in np.unique(counts[hit]):
        limbs[int(v)] = np.frombuffer((int(v) * MONT_R % R_ORDER).to_bytes(32, "little"), dtype=np.uint64)
    where = table_order[pos[hit]]
    for v, l in limbs.items():
        m[where[counts[hit] == v]] = l
    d_m = torch.from_numpy(m.view(np.int64)).to(dev)                                         # host -> device
    torch.cuda.synchronize()
    return d_m, int(counts[~hit].sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="2^12 and 2^16 rows at n = 2^20 only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import bls12_381_amd as b
    ctx = b.Context(0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    ctx.set_stream(stream.cuda_stream)

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.calls):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / a.calls

    def timed(fn):
        fn()                                                       # warm-up
        ctx.synchronize()
        return [window(fn) for _ in range(a.windows)]

    gen = torch.Generator(device=dev)
    gen.manual_seed(0x100C)

    try:
        commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    rec = {"commit": commit, "calls_per_window": a.calls, "windows": a.windows, "lds_rows": b.FR_LOOKUP_LDS_ROWS, "outputs": ["mult", "index", "missing"], "build": {}, "shapes": {}}
    ok = True
    log_rows = [12, 16] if a.quick else LOG_ROWS
    log_ns = [20] if a.quick else LOG_NS
    one_limbs = torch.zeros((1 << max(LOG_ROWS), 4), dtype=torch.int64, device=dev)
    one_limbs[:, 0] = 1
    for c in CS:
        for lr in log_rows:
            rows = 1 << lr
            # c columns of canonical scalars (every limb below 2^62); 2^20 random 248-bit values are distinct
            d_t = torch.randint(1, 1 << 62, (c, rows, 4), dtype=torch.int64, device=dev, generator=gen)
            torch.cuda.synchronize()
            builds = []
            lk = None
            for _ in range(3):
                if lk is not None:
                    lk.close()
                t0 = time.perf_counter()
                lk = ctx.fr_lookup_from_device(c, d_t.data_ptr(), rows, rows)
                builds.append((time.perf_counter() - t0) * 1e3)
            assert lk.distinct == rows and lk.rows == rows
            rec["build"]["rows=2^%d c=%d" % (lr, c)] = {"rows": rows, "c": c, "slots": lk.slots, "build_ms": min(builds), "build_ms_all": builds}
            t_host = d_t.cpu().numpy().view(np.uint64)
            tv = np.ascontiguousarray(t_host.transpose(1, 0, 2)).reshape(rows, c * 4).view(np.dtype((np.void, 32 * c))).reshape(rows)
            table_order = np.argsort(tv)
            table_sorted = tv[table_order]
            d_mult = torch.empty((rows, 4), dtype=torch.int64, device=dev)
            d_counts = torch.empty((rows, 4), dtype=torch.int64, device=dev)
            d_missing = torch.zeros((1,), dtype=torch.int64, device=dev)
            hot = torch.randint(0, rows, (16,), device=dev, generator=gen)
            for ln in log_ns:
                n = 1 << ln
                d_index = torch.empty((n,), dtype=torch.int32, device=dev)
                d_prod = torch.empty((n * c, 4), dtype=torch.int64, device=dev)
                shape = {"rows": rows, "n": n, "c": c, "path": "lds" if rows <= b.FR_LOOKUP_LDS_ROWS else "cache"}
                call = None
                for dist in DISTS:
                    uni = torch.randint(0, rows, (n,), device=dev, generator=gen)
                    if dist == "uniform":
                        idx = uni
                    elif dist == "one_row":
                        idx = torch.full((n,), rows // 2, dtype=torch.int64, device=dev)
                    else:
                        idx = torch.where(torch.rand((n,), device=dev, generator=gen) < 0.9, hot[torch.randint(0, 16, (n,), device=dev, generator=gen)], uni)
                    d_f = d_t[:, idx].contiguous()                                           # (c, n, 4): column j at j * n scalars
                    torch.cuda.synchronize()
                    call = lambda: lk.count_device(d_f.data_ptr(), n, n, d_mult.data_ptr(), d_index.data_ptr(), d_missing.data_ptr())
                    call()
                    ctx.fr_op_device(FR_MUL, d_mult.data_ptr(), one_limbs.data_ptr(), rows, d_counts.data_ptr())
                    ctx.synchronize()
                    want = torch.bincount(idx, minlength=rows)
                    same = bool(torch.equal(d_counts[:, 0], want)) and not bool(d_counts[:, 1:].any()) and bool(torch.equal(d_index.to(torch.int64), idx)) and int(d_missing[0]) == 0
                    row = {"outputs_match": same}
                    if not same:
                        ok = False
                        print("rows=2^%d n=2^%d c=%d %s: the call DIFFERS from the drawn row numbers" % (lr, ln, c, dist), flush=True)
                    ts = timed(call)
                    row.update({"ms": min(ts), "ms_all": ts, "lookups_per_s": n / min(ts) * 1e3})
                    if ln == 20 or (ln == 24 and lr == 12 and c == 1 and dist == "uniform"):
                        t0 = time.perf_counter()
                        d_m, host_missing = host_route(d_f, table_sorted, table_order, rows, dev)
                        row["host_route_ms"] = (time.perf_counter() - t0) * 1e3
                        row["host_route_matches"] = bool(torch.equal(d_m, d_mult)) and host_missing == 0
                        row["speedup_vs_host_route"] = row["host_route_ms"] / row["ms"]
                        ok = ok and row["host_route_matches"]
                        del d_m
                    shape[dist] = row
                    del d_f, idx, uni
                x = torch.randint(1, 1 << 62, (n * c, 4), dtype=torch.int64, device=dev, generator=gen)
                torch.cuda.synchronize()
                tm = timed(lambda: ctx.fr_op_device(FR_MUL, x.data_ptr(), x.data_ptr(), n * c, d_prod.data_ptr()))
                shape["fr_op_mul_ms"], shape["fr_op_mul_ms_all"] = min(tm), tm
                for dist in DISTS:
                    shape[dist]["vs_fr_op_mul"] = shape[dist]["ms"] / min(tm)
                shape["one_row_over_uniform"] = shape["one_row"]["ms"] / shape["uniform"]["ms"]
                shape["hot16_over_uniform"] = shape["hot16"]["ms"] / shape["uniform"]["ms"]
                key = "rows=2^%d n=2^%d c=%d" % (lr, ln, c)
                rec["shapes"][key] = shape
                print(key, json.dumps({"path": shape["path"], "uniform_ms": shape["uniform"]["ms"], "one_row_ms": shape["one_row"]["ms"], "hot16_ms": shape["hot16"]["ms"],
                                       "fr_op_mul_ms": min(tm), "host_route_ms": shape["uniform"].get("host_route_ms"), "match": all(shape[d]["outputs_match"] for d in DISTS)}), flush=True)
                del d_index, d_prod, x
                torch.cuda.empty_cache()
            lk.close()
            del d_t, d_mult, d_counts
            torch.cuda.empty_cache()
    ctx.set_stream(None)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
