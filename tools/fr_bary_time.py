"""Same-process timing of the evaluation-form openings (blsgpu_fr_bary_eval_many_device, blsgpu_fr_bary_open_many_device) against the
coefficient-form route the library already had.

    python tools/fr_bary_time.py [--calls R] [--windows W] [--out profiles/fr_bary_time.json]

Method of tools/fr_scan_time.py: times are HIP events on the stream the calls are enqueued on (the context is put on a torch stream with
set_stream), one pair of events around a window of R back-to-back device-form calls (default 10) after warm-up calls of the same shape
(scratch, LDS attribute, twiddle tables, code objects); W such windows (default 5), the minimum and all of them are recorded, per call.
The calls of a window reuse the same buffers: the 4096 x 64 and 256 x 4096 shapes (8 MB) stay in the 256 MB Infinity Cache from one call
to the next, so their figures are cache-warm ones; 2^24 scalars (512 MB in, 512 MB out) are not.  In the same process and run:
  * `composed`: inverse fr_ntt_many_device, fr_scan_device(HORNER), forward fr_ntt_many_device -- three calls on one buffer pair.  The
    shift of the quotient's coefficients by one place between the scan and the forward transform (a copy for k > 1) is NOT timed, which
    favours this route; `open_vs_composed` = open time / composed time.  `beats_composed`: the fused open is faster by more than the
    spread (max - min) of the composed route's own windows.
  * `fr_op_device` op 0 (mul) of two different arrays at the same element count (96 bytes per element) as the memory yardstick.  Of the
    caller's arrays the fused open moves 64 bytes per element while a row fits a tile of 2048 and 160 above it (`open_array_gb_per_s` uses
    those); on top of that every element reads its 32-byte entry of the twiddle table twice (forward and backward sweep), a table of
    n / 2 entries that the caches hold for the shapes here, read with unit stride in natural order and as a gather in bit-reversed order.
  * `open_bitrev_ms` / `eval_bitrev_ms`: the same calls with BLSGPU_FR_ORDER_BITREV (the gather), same buffers.
Before anything is timed, both routes' y and q are compared limb for limb at every shape (`outputs_match`, with the shift done properly and
one row's point inside the domain); a mismatch ends the run with status 1.  No test asserts any of these figures."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("4096x2^6", 4096, 6), ("256x2^12", 256, 12), ("16x2^20", 16, 20), ("1x2^24", 1, 24)]
R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
TILE = 2048


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
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
        fn()
        fn()                                                       # warm-up
        ctx.synchronize()
        return [window(fn) for _ in range(a.windows)]

    def scalars(n, seed):
        x = np.random.RandomState(seed).randint(0, 256, size=(n, 32), dtype=np.uint8)
        x[:, 31] &= 0x3F                                           # < 2^254 < r: canonical limbs
        return torch.from_numpy(x.view(np.int64).reshape(n, 4)).to(dev)

    def mont(v):
        v = (v << 256) % R_ORDER
        return [(v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)]

    rec = {"calls_per_window": a.calls, "windows": a.windows, "shapes": {}}
    ok = True
    for name, k, log_n in SHAPES:
        n = 1 << log_n
        total = k * n
        d_in = scalars(total, 100 + k).reshape(k, n, 4)
        d_in2 = scalars(total, 200 + k)
        pts = np.array(scalars(k, 7).cpu().numpy().view(np.uint64))
        w = pow(pow(7, (R_ORDER - 1) >> 32, R_ORDER), 1 << (32 - log_n), R_ORDER)      # the root blsgpu_fr_ntt uses: ROOT_OF_UNITY^(2^(32 - log_n))
        pts[k - 1] = mont(pow(w, n - 3, R_ORDER))                  # the last row's point is D[n - 3]
        d_pts = torch.from_numpy(pts.view(np.int64)).to(dev)
        d_y = torch.zeros((k, 4), dtype=torch.int64, device=dev)
        d_q = torch.zeros_like(d_in)
        d_c = d_in.clone()
        d_h = torch.zeros_like(d_in)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            ctx.fr_bary_open_device(d_in.data_ptr(), log_n, k, d_pts.data_ptr(), d_y.data_ptr(), d_q.data_ptr())
            ctx.fr_ntt_many_device(d_c.data_ptr(), log_n, k, inverse=True)
            ctx.fr_scan_device(2, d_c.data_ptr(), n, k, d_h.data_ptr(), d_points=d_pts.data_ptr())
            ctx.synchronize()
            d_qc = torch.cat([d_h[:, 1:, :], torch.zeros((k, 1, 4), dtype=torch.int64, device=dev)], dim=1).contiguous()
            stream.synchronize()
            ctx.fr_ntt_many_device(d_qc.data_ptr(), log_n, k, inverse=False)
            ctx.synchronize()
            same = bool(torch.equal(d_y, d_h[:, 0, :])) and bool(torch.equal(d_q, d_qc)) and bool(torch.equal(d_y[k - 1], d_in[k - 1, n - 3]))
        del d_qc
        ok = ok and same
        print(name, "outputs_match", same, flush=True)
        if not same:
            rec["shapes"][name] = {"k": k, "log_n": log_n, "outputs_match": False}
            continue

        def composed():
            ctx.fr_ntt_many_device(d_c.data_ptr(), log_n, k, inverse=True)
            ctx.fr_scan_device(2, d_c.data_ptr(), n, k, d_h.data_ptr(), d_points=d_pts.data_ptr())
            ctx.fr_ntt_many_device(d_h.data_ptr(), log_n, k, inverse=False)

        t_mul = timed(lambda: ctx.fr_op_device(0, d_in.data_ptr(), d_in2.data_ptr(), total, d_h.data_ptr()))
        t_comp = timed(composed)
        t_eval = timed(lambda: ctx.fr_bary_eval_device(d_in.data_ptr(), log_n, k, d_pts.data_ptr(), d_y.data_ptr()))
        t_open = timed(lambda: ctx.fr_bary_open_device(d_in.data_ptr(), log_n, k, d_pts.data_ptr(), d_y.data_ptr(), d_q.data_ptr()))
        t_eval_br = timed(lambda: ctx.fr_bary_eval_device(d_in.data_ptr(), log_n, k, d_pts.data_ptr(), d_y.data_ptr(), order=1))
        t_open_br = timed(lambda: ctx.fr_bary_open_device(d_in.data_ptr(), log_n, k, d_pts.data_ptr(), d_y.data_ptr(), d_q.data_ptr(), order=1))
        t_comp2 = timed(composed)                                  # again after the fused calls: the spread covers drift over the run
        comp_all = t_comp + t_comp2
        open_bytes = 64 if n <= TILE else 160
        row = {"k": k, "log_n": log_n, "elements": total, "outputs_match": True,
               "eval_ms": min(t_eval), "eval_ms_all": t_eval, "open_ms": min(t_open), "open_ms_all": t_open,
               "composed_ms": min(comp_all), "composed_ms_all": comp_all, "composed_spread_ms": max(comp_all) - min(comp_all),
               "fr_op_mul_ms": min(t_mul), "fr_op_mul_ms_all": t_mul, "fr_op_mul_gb_per_s": total * 96 / min(t_mul) / 1e6,
               "eval_bitrev_ms": min(t_eval_br), "eval_bitrev_ms_all": t_eval_br, "open_bitrev_ms": min(t_open_br), "open_bitrev_ms_all": t_open_br,
               "open_array_bytes_per_element": open_bytes, "open_array_gb_per_s": total * open_bytes / min(t_open) / 1e6,
               "eval_array_gb_per_s": total * 32 / min(t_eval) / 1e6, "table_bytes_per_element": 64,
               "open_vs_composed": min(t_open) / min(comp_all), "eval_vs_composed": min(t_eval) / min(comp_all),
               "open_vs_fr_op_mul": min(t_open) / min(t_mul),
               "beats_composed": bool(min(comp_all) - max(t_open) > max(comp_all) - min(comp_all))}
        rec["shapes"][name] = row
        print(name, json.dumps({q: row[q] for q in row if not q.endswith("_all")}), flush=True)
        del d_in, d_in2, d_q, d_c, d_h
    ctx.set_stream(None)
    rec["outputs_match"] = ok
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
