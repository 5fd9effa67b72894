"""Same-process timing of the Fr scans and the batch inversion (blsgpu_fr_scan_many_device, blsgpu_fr_batch_invert_device) against the
element-wise path the library already had.

    python tools/fr_scan_time.py [--window-ms T] [--windows W] [--out profiles/fr_scan_time.json]

Times are HIP events on the stream the calls are enqueued on (the context is put on a torch stream with set_stream): one pair of events
around R back-to-back device-form calls, after warm-up calls of the same shape (scratch, LDS attribute, code objects); R is chosen per
measurement from a first short window so that a window lasts about T ms (default 100; `reps` is recorded with every figure); W such
windows, the minimum and all of them are recorded, per call.  The calls of a window reuse the same buffers: the 4096 x 64 and 256 x 4096
shapes (8 and 32 MB) stay in the 256 MB Infinity Cache from one call to the next, so their figures are cache-warm ones; 2^24 scalars
(512 MB in, 512 MB out) are not.  Yardsticks, in the same process and run:
  * `fr_op_device` op 0 (mul) of TWO DIFFERENT input arrays at the same element count: two reads and one write per element, the traffic
    a scan has (input read by the reduce pass and by the scan pass, output written once) -- `vs_fr_op_mul` = scan time / mul time;
  * `fr_op_device` op 4 (invert, an exponentiation per element) at 2^20: what inversion cost before -- `invert_speedup_2_20` = op 4 time /
    batch inversion time.
Outputs are checked where it is cheap: the batch inversion at 2^20 against op 4, limb for limb (`outputs_match`).  Kernel times come from a
separate `rocprofv3 --kernel-trace --stats` run of this script.  No test asserts any of these figures."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("4096x64", 4096, 64), ("256x4096", 256, 4096), ("16x2^20", 16, 1 << 20), ("1x2^24", 1, 1 << 24)]
OPS = [("sum", 0), ("product", 1), ("horner", 2)]


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
        for _ in range(reps):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    def timed(fn):
        """(per-call ms of every window, calls per window)"""
        fn()                                                       # warm-up
        ctx.synchronize()
        reps = max(3, min(5000, int(a.window_ms / max(window(fn, 3), 1e-4))))
        return [window(fn, reps) for _ in range(a.windows)], reps

    def scalars(n, seed):
        x = np.random.RandomState(seed).randint(0, 256, size=(n, 32), dtype=np.uint8)
        x[:, 31] &= 0x3F                                           # < 2^254 < r: canonical limbs
        x[:, 0] |= 1                                               # none of them zero
        return torch.from_numpy(x.view(np.int64).reshape(n, 4)).to(dev)

    rec = {"window_ms": a.window_ms, "windows": a.windows, "bytes_per_element": 96, "scan": {}, "fr_op_mul": {}, "invert": {}}
    mul_ms = {}
    for name, k, n in SHAPES:
        total = k * n
        d_in = scalars(total, 100 + k)
        d_in2 = scalars(total, 200 + k)
        d_pts = scalars(k, 7)
        d_out = torch.empty_like(d_in)
        torch.cuda.synchronize()
        if total not in mul_ms:
            t, reps = timed(lambda: ctx.fr_op_device(0, d_in.data_ptr(), d_in2.data_ptr(), total, d_out.data_ptr()))
            mul_ms[total] = min(t)
            rec["fr_op_mul"][str(total)] = {"elements": total, "ms": min(t), "ms_all": t, "reps": reps, "gb_per_s": total * 96 / min(t) / 1e6}
            print("fr_op mul", total, json.dumps({"ms": min(t)}), flush=True)
        for op_name, op in OPS:
            t, reps = timed(lambda: ctx.fr_scan_device(op, d_in.data_ptr(), n, k, d_out.data_ptr(), d_points=d_pts.data_ptr() if op == 2 else None))
            row = {"k": k, "len": n, "ms": min(t), "ms_all": t, "reps": reps, "elements_per_s": total / min(t) * 1e3, "gb_per_s": total * 96 / min(t) / 1e6,
                   "fr_op_mul_ms": mul_ms[total], "vs_fr_op_mul": min(t) / mul_ms[total]}
            rec["scan"][op_name + "_" + name] = row
            print(op_name, name, json.dumps({q: row[q] for q in ("ms", "fr_op_mul_ms", "vs_fr_op_mul", "gb_per_s")}), flush=True)
        del d_in, d_in2, d_out, d_pts
    ok = True
    for log_n in (20, 24):
        n = 1 << log_n
        d_in = scalars(n, 300 + log_n)
        d_in[::1000] = 0                                           # one in 1000 of them zero
        d_out = torch.empty_like(d_in)
        d_fl = torch.empty(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        t, reps = timed(lambda: ctx.fr_batch_invert_device(d_in.data_ptr(), n, d_out.data_ptr(), d_fl.data_ptr()))
        row = {"n": n, "ms": min(t), "ms_all": t, "reps": reps, "elements_per_s": n / min(t) * 1e3}
        if log_n == 20:
            d_ref = torch.empty_like(d_in)
            d_fr = torch.empty(n, dtype=torch.uint8, device=dev)
            t4, reps4 = timed(lambda: ctx.fr_op_device(4, d_in.data_ptr(), None, n, d_ref.data_ptr(), d_fr.data_ptr()))
            ctx.synchronize()
            same = bool(torch.equal(d_out, d_ref)) and bool(torch.equal(d_fl, d_fr))
            ok = ok and same
            row.update({"fr_op_invert_ms": min(t4), "fr_op_invert_ms_all": t4, "fr_op_invert_reps": reps4, "outputs_match": same})
            rec["invert_speedup_2_20"] = min(t4) / min(t)
        rec["invert"]["2^%d" % log_n] = row
        print("batch_invert 2^%d" % log_n, json.dumps({q: row[q] for q in row if not q.endswith("_all")}), flush=True)
        del d_in, d_out, d_fl
    ctx.set_stream(None)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
