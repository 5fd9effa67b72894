"""Same-process timing of the Fr fraction scans (blsgpu_fr_grand_product_device, blsgpu_fr_frac_sum_device) against the same columns
composed from the entry points the library had before.

    python tools/fr_frac_time.py [--calls 10] [--windows 3] [--out profiles/fr_frac_time.json] [--only SHAPE]

Times are HIP events on the stream the calls are enqueued on (the context is put on a torch stream with set_stream): one pair of events
around `calls` back-to-back device-form calls (default 10), after a warm-up call of the same shape (scratch, code objects); W such
windows, the minimum and all of them are recorded, per call.  The calls of a window reuse the same buffers: the 4096 x 64 and
256 x 4096 shapes stay in the 256 MB Infinity Cache from one call to the next at small c, so their figures are cache-warm ones;
2^24 scalars per table are not.

The composed route, timed IN THE SAME RUN on the same inputs and compared limb for limb (`outputs_match`, the flags included for the
grand product): beta and gamma as constant-filled arrays of the full length (built once, outside the timed region), per column and
side `fr_op_device` mul / add / add for the factor and, from the second column on, a mul into the running product (4 c - 1 calls a
side), then `fr_batch_invert_device`, one mul and `fr_scan_device` PRODUCT -- 8 c + 1 calls; the fraction sum builds every column's
factor (3), inverts it, multiplies by the multiplicities and, from the second column on, adds, then scans: 6 c calls.  Two cheaper yardsticks over as many
elements: `fr_batch_invert_device` and `fr_scan_device` alone (`vs_invert`, `vs_scan`: fused time over theirs).
The record names the commit, the shapes and the (op, c) tiles.  No test asserts any of these figures."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("4096x64", 4096, 64), ("256x4096", 256, 4096), ("16x2^20", 16, 1 << 20), ("1x2^24", 1, 1 << 24)]
COLS = [1, 3, 8]
MUL, ADD = 0, 1
SUM, PRODUCT = 0, 1


def tile(op, c):
    """csrc/fr_frac_plan.h frf_shape"""
    return 256 * (2 if op == "frac_sum" and c > 4 else 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--only", default=None, help="one shape name, e.g. 256x4096")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
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
    gen.manual_seed(0xF7AC)

    def scalars(n):
        """n canonical scalars made on the device: every limb below 2^62, so the value is below r; none of them zero"""
        x = torch.randint(1, 1 << 62, (n, 4), dtype=torch.int64, device=dev, generator=gen)
        return x

    try:
        commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    rec = {"commit": commit, "calls_per_window": a.calls, "windows": a.windows, "shapes": {name: {"k": k, "len": n} for name, k, n in SHAPES},
           "tiles": {"%s_c%d" % (op, c): tile(op, c) for op in ("grand_product", "frac_sum") for c in COLS}, "yardsticks": {}, "grand_product": {}, "frac_sum": {}}
    ok = True
    P = lambda t, off=0: t.data_ptr() + off * 32
    for name, k, n in SHAPES:
        if a.only and a.only != name:
            continue
        total = k * n
        z = lambda: torch.empty((total, 4), dtype=torch.int64, device=dev)
        d_out, d_want, t_, num, den, inv = z(), z(), z(), z(), z(), z()
        d_fl = torch.empty(total, dtype=torch.uint8, device=dev)
        d_fl2 = torch.empty(total, dtype=torch.uint8, device=dev)
        chal = scalars(2)
        beta = chal[0:1].expand(total, 4).contiguous()
        gamma = chal[1:2].expand(total, 4).contiguous()
        x = scalars(total)
        torch.cuda.synchronize()
        ti = timed(lambda: ctx.fr_batch_invert_device(P(x), total, P(d_out), d_fl.data_ptr()))
        ts = timed(lambda: ctx.fr_scan_device(PRODUCT, P(x), n, k, P(d_out)))
        rec["yardsticks"][name] = {"elements": total, "batch_invert_ms": min(ti), "batch_invert_ms_all": ti, "scan_product_ms": min(ts), "scan_product_ms_all": ts}
        print("yardsticks", name, json.dumps({"batch_invert_ms": min(ti), "scan_product_ms": min(ts)}), flush=True)
        del x
        op = ctx.fr_op_device

        def factor(d_a, d_b, j, dst):
            o = j * total
            op(MUL, P(beta), P(d_b, o), total, P(dst))
            op(ADD, P(dst), P(d_a, o), total, P(dst))
            op(ADD, P(dst), P(gamma), total, P(dst))

        for c in COLS:
            sets = [scalars(c * total) for _ in range(4)]
            na, nb, da, db = sets
            # one zero denominator in 4096, in the last column
            idx = torch.arange(7, total, 4096, device=dev)
            off = (c - 1) * total
            ctx.synchronize()
            torch.cuda.synchronize()
            op(MUL, P(beta), P(db, off), total, P(t_))
            op(ADD, P(t_), P(gamma), total, P(t_))
            op(5, P(t_), None, total, P(t_))                       # neg
            ctx.synchronize()
            da[off + idx] = t_[idx]
            torch.cuda.synchronize()

            def fused_gp():
                ctx.fr_grand_product_device(c, P(na), P(nb), P(da), P(db), total, P(chal), n, k, P(d_out), d_fl.data_ptr(), exclusive=True)

            def composed_gp():
                for j in range(c):
                    for acc, d_a, d_b in ((num, na, nb), (den, da, db)):
                        factor(d_a, d_b, j, t_ if j else acc)
                        if j:
                            op(MUL, P(acc), P(t_), total, P(acc))
                ctx.fr_batch_invert_device(P(den), total, P(inv), d_fl2.data_ptr())
                op(MUL, P(num), P(inv), total, P(d_want))
                ctx.fr_scan_device(PRODUCT, P(d_want), n, k, P(d_want), exclusive=True)

            def fused_fs():
                ctx.fr_frac_sum_device(c, P(na), P(da), P(db), total, P(chal), n, k, P(d_out), d_fl.data_ptr())

            def composed_fs():
                for j in range(c):
                    term = inv if j else num
                    factor(da, db, j, t_)
                    ctx.fr_batch_invert_device(P(t_), total, P(term), d_fl2.data_ptr())
                    op(MUL, P(na, j * total), P(term), total, P(term))
                    if j:
                        op(ADD, P(num), P(term), total, P(num))
                ctx.fr_scan_device(SUM, P(num), n, k, P(d_want))

            for what, fused, composed, calls in (("grand_product", fused_gp, composed_gp, 8 * c + 1), ("frac_sum", fused_fs, composed_fs, 6 * c)):
                tf = timed(fused)
                tc = timed(composed)
                ctx.synchronize()
                same = bool(torch.equal(d_out, d_want))
                zeros = int((d_fl == 0).sum())
                if what == "grand_product":
                    same = same and bool(torch.equal(d_fl, d_fl2))
                same = same and zeros == len(idx)
                ok = ok and same
                row = {"k": k, "len": n, "c": c, "tile": tile(what, c), "ms": min(tf), "ms_all": tf, "composed_ms": min(tc), "composed_ms_all": tc, "composed_calls": calls,
                       "speedup_vs_composed": min(tc) / min(tf), "vs_invert": min(tf) / min(ti), "vs_scan": min(tf) / min(ts), "elements_per_s": total / min(tf) * 1e3,
                       "zero_denominators": zeros, "outputs_match": same}
                rec[what]["%s_c%d" % (name, c)] = row
                print(what, name, "c=%d" % c, json.dumps({q: row[q] for q in ("ms", "composed_ms", "speedup_vs_composed", "vs_invert", "vs_scan", "outputs_match")}), flush=True)
            del sets, na, nb, da, db
        del d_out, d_want, t_, num, den, inv, beta, gamma
        torch.cuda.empty_cache()
    ctx.set_stream(None)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
