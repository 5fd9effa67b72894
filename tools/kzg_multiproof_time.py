"""Same-process timing of the amortised KZG openings (blsgpu_kzg_multiproof_create / _proofs_device, blsgpu_kzg_cells_device), every figure
next to the yardstick it is judged by, measured in the same run.

    python tools/kzg_multiproof_time.py [--reps R] [--out profiles/kzg_multiproof_time.json] [--quick] [--shapes "12,0,16;16,6,16" --merge]

Times are HIP events recorded on the stream the context launches on, around WINDOWS of 10 calls after a warm-up call of the same shape
(tables, code objects, scratch); a figure is a window's time over 10, and median, minimum, maximum and every window are recorded.
`create` is a host clock around the call, which synchronises.  The inputs are seeded: an SRS of [s_m] G1 for random s_m, polynomials of
random canonical scalars.

  shapes     (log_n, log_l) x count: (12, 6) x 1 / 16 / 256, (12, 0) x 16, (16, 6) x 16
  stages     one more call with blsgpu_kernel_timing on: the kernels of proofs_device grouped into its stages
  yardstick  the route the call replaces, built from shipped entry points: a transposed copy of the coefficients into 2c l rows of c per
             polynomial (row (i, t) = p[t], p[l + t], ...), fr_scan_many_device HORNER in X^l with a_i as the row's point, then the
             count * 2c MSMs of n terms over the shared SRS (g1_msm_segments_device with base_first all 0 where n <= 4096, else
             g1_msm_many_device), the SRS permuted once to the rows' order with an identity where the scan leaves p(a_i).  Where the
             route's MSM would exceed its own limit of 2^27 terms it is measured for `yardstick_count` polynomials and scaled by
             count / yardstick_count (`scaled`: true).  Its outputs are compared with the new call's after batch_normalize.
  bar        at (12, 6) the new call must be faster than the route by more than the spread (max - min) of the route's own windows."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WINDOW = 10
STAGES = (("coefficients (evaluation form only)", ("k_kzg_scalar_copy",)), ("rows + transposition + segments", ("k_kzg_coeff_rows", "k_kzg_transpose", "k_kzg_segments")),
          ("Fr transforms", ("k_fr_",)), ("Toeplitz MSM", ("k_msm_seg", "k_proj_export")), ("G1 transforms", ("k_gntt",)),
          ("identities + output order", ("k_kzg_identity_fill", "k_kzg_point_permute")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kzg_multiproof_time.json"))
    ap.add_argument("--quick", action="store_true", help="(12, 6) x 1 and x 16 only")
    ap.add_argument("--shapes", default="", help="log_n,log_l,count;... instead of the built-in list")
    ap.add_argument("--merge", action="store_true", help="keep the shapes an existing record at --out holds (a second run for the shapes a first one missed)")
    a = ap.parse_args()
    import torch
    import bls12_381_amd as b
    from oracle import bls12_381_ref as o
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    ctx = b.Context(0)
    ctx.set_stream(side.cuda_stream)
    R = o.R_ORDER

    def windows(fn, reps, calls=WINDOW):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(side):
                e0.record(side)
                for _ in range(calls):
                    fn()
                e1.record(side)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / calls)
        return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "spread_ms": max(ms) - min(ms), "calls_per_window": calls, "all_ms": ms}

    def scalars(n, seed):
        """n canonical scalars as (n, 4) int64 Montgomery limbs on the device: any value below 2^254 < r is one"""
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        s = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=g)
        s[:, 31] &= 0x3F
        return s.view(torch.int64).reshape(n, 4)

    def limbs(vals):
        return np.array([o.fr_to_mont_limbs(int(v) % R) for v in vals], dtype=np.uint64).reshape(-1, 4)

    def affine(d_xyz, n):
        d_xy = torch.zeros((n, 12), dtype=torch.int64, device=dev)
        d_inf = torch.zeros(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()                                   # the buffers were zeroed on another stream than the context's
        ctx.batch_normalize_device(1, d_xyz.data_ptr(), n, d_xy.data_ptr(), d_inf.data_ptr())
        ctx.synchronize()
        xy, inf = d_xy.cpu().numpy(), d_inf.cpu().numpy()
        xy[inf != 0] = 0
        return xy, inf

    shapes = [(12, 6, 1), (12, 6, 16)] if a.quick else [(12, 6, 1), (12, 6, 16), (12, 6, 256), (12, 0, 16), (16, 6, 16)]
    if a.shapes:
        shapes = [tuple(int(x) for x in s.split(",")) for s in a.shapes.split(";")]
    rec = {"reps": a.reps, "window": WINDOW, "device": torch.cuda.get_device_name(0), "runs": 1, "shapes": {}}
    if a.merge and a.out and os.path.exists(a.out):
        with open(a.out) as fh:
            old = json.load(fh)
        rec["shapes"] = old.get("shapes", {})
        rec["runs"] = old.get("runs", 1) + 1
    srs_of = {}
    for log_n, log_l, count in shapes:
        n, l, c = 1 << log_n, 1 << log_l, 1 << (log_n - log_l)
        name = "(%d, %d) x %d" % (log_n, log_l, count)
        if log_n not in srs_of:
            srs_of[log_n] = ctx.bases_from_scalars(1, scalars(n, 11 + log_n).cpu().numpy().view(np.uint8).reshape(n, 32))
        srs = srs_of[log_n]
        out = {"log_n": log_n, "log_l": log_l, "count": count, "cells_per_polynomial": 2 * c}
        t0 = time.perf_counter()
        h = ctx.kzg_multiproof_create(srs, log_n, log_l)
        ctx.synchronize()
        out["create_first_ms"] = (time.perf_counter() - t0) * 1e3
        h.close()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            h2 = ctx.kzg_multiproof_create(srs, log_n, log_l)
            ctx.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
            h2.close()
        out["create_ms"] = {"median_ms": statistics.median(ts), "all_ms": ts, "what": "host clock around the call, which synchronises"}
        h = ctx.kzg_multiproof_create(srs, log_n, log_l)
        with torch.cuda.stream(side):
            d_p = scalars(count * n, 1000 + log_n + count)
            d_out = torch.zeros((count * 2 * c, 18), dtype=torch.int64, device=dev)
            d_cells = torch.zeros((count * 2 * n, 4), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        reps = a.reps if count * n <= (1 << 18) else max(2, a.reps // 2)
        calls = WINDOW if count * n <= (1 << 18) else 2
        for form, fname in ((b.KZG_FORM_COEFFS, "coeffs"), (b.KZG_FORM_EVALS, "evals_bitrev")):
            order = b.FR_ORDER_BITREV if form else b.FR_ORDER_NATURAL
            out["proofs_device_" + fname] = windows(lambda: h.proofs_device(d_p.data_ptr(), count, d_out.data_ptr(), form, order), reps, calls)
            out["cells_device_" + fname] = windows(lambda: ctx.kzg_cells_device(d_p.data_ptr(), log_n, log_l, count, d_cells.data_ptr(), form, order), reps, calls)
        # the stage split of one call in coefficient form
        ctx.kernel_timing(True)
        h.proofs_device(d_p.data_ptr(), count, d_out.data_ptr(), b.KZG_FORM_COEFFS, b.FR_ORDER_NATURAL)
        ctx.synchronize()
        rep = ctx.kernel_timing_report()
        ctx.kernel_timing(False)
        out["kernels"] = rep
        out["stages_ms"] = {s: sum(v["total_ms"] for kname, v in rep.items() if any(p in kname for p in pre)) for s, pre in STAGES}
        out["stages_ms"]["other"] = sum(v["total_ms"] for v in rep.values()) - sum(out["stages_ms"].values())
        new_xy = affine(d_out, count * 2 * c)
        # ---- the yardstick: transposed copy -> HORNER in X^l -> count * 2c MSMs over the shared SRS ------------------------------------
        yc = count
        while yc > 1 and yc * 2 * c * n > (1 << 27):
            yc //= 2
        if yc * 2 * c * n > (1 << 27):
            out["yardstick"] = {"measured": False, "why": "one polynomial's quotients exceed the MSM's limit of 2^27 terms"}
        else:
            w = o.fr_omega(log_n + 1)
            a_i = limbs([pow(w, i * l, R) for i in range(2 * c)])                                     # natural order
            with torch.cuda.stream(side):
                d_pts = torch.from_numpy(np.repeat(a_i, l, axis=0).view(np.int64)).to(dev).repeat(yc, 1).contiguous()      # one point per row (v, i, t)
                d_rows = torch.zeros((yc * 2 * c * l, c, 4), dtype=torch.int64, device=dev)
                d_q = torch.zeros_like(d_rows)
                d_y = torch.zeros((yc * 2 * c, 18), dtype=torch.int64, device=dev)
                d_off = torch.from_numpy((np.arange(yc * 2 * c + 1, dtype=np.uint32) * n).view(np.int32)).to(dev)
                d_bf = torch.zeros(yc * 2 * c, dtype=torch.int32, device=dev)
            # the SRS in the rows' order: S'[t c + 0] = identity (the scan leaves p(a_i) there), S'[t c + 1 + s] = S[s l + t]
            xy, inf = srs.download()
            pxy, pinf = np.zeros((n, 12), dtype=np.uint64), np.ones(n, dtype=np.uint8)
            for t in range(l):
                pxy[t * c + 1:(t + 1) * c] = xy[t:(c - 1) * l + t:l][:c - 1]
                pinf[t * c + 1:(t + 1) * c] = inf[t:(c - 1) * l + t:l][:c - 1]
            srs_rows = ctx.upload_bases(1, pxy, pinf)
            torch.cuda.synchronize()

            def route():
                with torch.cuda.stream(side):
                    d_rows.view(yc, 2 * c, l, c, 4).copy_(d_p[:yc * n].view(yc, 1, c, l, 4).permute(0, 1, 3, 2, 4).expand(yc, 2 * c, l, c, 4))
                ctx.fr_scan_device(b.FR_SCAN_HORNER, d_rows.data_ptr(), c, yc * 2 * c * l, d_q.data_ptr(), d_points=d_pts.data_ptr())
                ctx.set_scalar_form(1)
                try:
                    if n <= 4096:
                        ctx.msm_segments_device(srs_rows, d_q.data_ptr(), d_off.data_ptr(), yc * 2 * c, yc * 2 * c * n, d_y.data_ptr(), d_base_first=d_bf.data_ptr())
                    else:
                        b._lib.check(ctx.lib.blsgpu_g1_msm_many_device(ctx.h, srs_rows.handle, 0, d_q.data_ptr(), n, yc * 2 * c, d_y.data_ptr()), "msm_many_device")
                finally:
                    ctx.set_scalar_form(0)

            big = yc * 2 * c * n > (1 << 24)
            y = windows(route, 2 if big else a.reps, 1 if big else WINDOW)
            old_xy = affine(d_y, yc * 2 * c)
            same = bool(np.array_equal(old_xy[1], new_xy[1][:yc * 2 * c]) and np.array_equal(old_xy[0], new_xy[0][:yc * 2 * c]))
            scale = count / yc
            new = out["proofs_device_coeffs"]
            out["yardstick"] = dict(y, measured=True, yardstick_count=yc, scaled=yc != count, route_ms_for_count=y["median_ms"] * scale, outputs_equal=same,
                                    what="transposed copy + fr_scan_many_device HORNER + %s" % ("g1_msm_segments_device" if n <= 4096 else "g1_msm_many_device"),
                                    speedup=y["median_ms"] * scale / new["median_ms"],
                                    faster_beyond_route_spread=bool(y["median_ms"] * scale - new["median_ms"] > y["spread_ms"] * scale))
            srs_rows.free()
            del d_rows, d_q, d_pts, d_y
        h.close()
        del d_p, d_out, d_cells
        torch.cuda.empty_cache()
        rec["shapes"][name] = out
        print(name, json.dumps({"create_ms": out["create_ms"]["median_ms"], "proofs_ms": out["proofs_device_coeffs"]["median_ms"], "proofs_evals_ms": out["proofs_device_evals_bitrev"]["median_ms"],
                                "cells_ms": out["cells_device_coeffs"]["median_ms"], "stages_ms": out["stages_ms"],
                                "yardstick": {k: v for k, v in out["yardstick"].items() if k != "all_ms"}}), flush=True)
        if a.out:                                                 # the record so far: a later shape that runs out of time loses nothing
            with open(a.out, "w") as fh:
                json.dump(rec, fh, indent=1)
    for s in srs_of.values():
        s.free()
    ctx.set_stream(None)
    ctx.close()
    missed = [n for n, r in rec["shapes"].items() if r["log_n"] == 12 and r["log_l"] == 6 and r["yardstick"].get("measured") and
              not (r["yardstick"]["outputs_equal"] and r["yardstick"]["faster_beyond_route_spread"])]
    for m in missed:
        print("MISSED", m, flush=True)
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())
