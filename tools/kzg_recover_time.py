"""Same-process timing of KZG cell recovery (blsgpu_kzg_recover_device), every figure next to the yardsticks it is judged by, measured in
the same run.

    python tools/kzg_recover_time.py [--reps R] [--out profiles/kzg_recover_time.json] [--only "(12, 6) x 16"]

Times are HIP events recorded on the stream the context launches on, around WINDOWS of 10 calls after a warm-up call of the same shape
(tables, code objects, scratch); a figure is a window's time over 10, and median, minimum, maximum and every window are recorded.  The
inputs are honest: random polynomials, their cells from blsgpu_kzg_cells_device, half of the cells dropped -- so every timed call must
also return ok = 1 for every polynomial and all 2c cells limb for limb (`outputs_ok`); a figure whose call failed that is not kept.

  shapes      (12, 6) x 1 / 16 / 256 polynomials (the 128 cells of a data-availability blob, bit-reversed numbering) with a random half
              missing and with the second half missing, polys and out_cells both taken; (16, 6) x 16 with a random half missing
  floor       (a) the three blsgpu_fr_ntt_many_device calls of (log_n + 1, count) the call makes -- inverse, forward on the coset 7,
              inverse on the coset 7 -- plus blsgpu_kzg_cells_device on count polynomials (the fourth transform): what no recovery by
              this route can beat
  route       (b) what a user had before this call: EZ and the two tables prepared on the HOST (outside the timed region; here: arrays
              of the right size in device memory), the tables expanded to the full 2n per polynomial, then blsgpu_fr_op_device mul with
              the expanded tables around the same three transforms (one product before them, one between), and blsgpu_kzg_cells_device.
              The check of the upper half and the zeroing are not in it.  At (12, 6) x 1 the route is also run on honest tables from
              Python integers and its coefficients compared with the call's (`route_agrees`).
  stages      one more call with blsgpu_kernel_timing on: `new_kernel_share` is the part of the kernel time spent in k_kzg_rec_*."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
WINDOW = 10
ORDER = 1                                                          # BLSGPU_FR_ORDER_BITREV
GEN = 7
SHAPES = [(12, 6, 1), (12, 6, 16), (12, 6, 256), (16, 6, 16)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kzg_recover_time.json"))
    ap.add_argument("--only", default=None, help='one shape, e.g. "(12, 6) x 16"; merged into the record that --out holds')
    a = ap.parse_args()
    import torch
    import bls12_381_amd as b
    from oracle import bls12_381_ref as o
    import kzg_recover_ref as rr
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

    def scalars(count, seed):
        """count canonical scalars as (count, 4) int64 Montgomery limbs on the device: any value below 2^254 < r is one"""
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        s = torch.randint(0, 256, (count, 32), dtype=torch.uint8, device=dev, generator=g)
        s[:, 31] &= 0x3F
        return s.view(torch.int64).reshape(count, 4)

    def up(arr, dt):
        return torch.from_numpy(np.ascontiguousarray(arr).view(dt).reshape(-1).copy()).to(dev)

    rec = {"tool": "tools/kzg_recover_time.py", "window": WINDOW, "reps": a.reps, "order": "bitrev", "device": torch.cuda.get_device_name(0), "shapes": {}}
    if a.only and a.out and os.path.exists(a.out):
        with open(a.out) as fh:
            rec["shapes"] = json.load(fh).get("shapes", {})
    ok_all = True
    for log_n, log_l, count in SHAPES:
        shape = "(%d, %d) x %d" % (log_n, log_l, count)
        if a.only and a.only != shape:
            continue
        n, l, c = 1 << log_n, 1 << log_l, 1 << (log_n - log_l)
        c2 = 2 * c
        with torch.cuda.stream(side):
            d_p = scalars(count * n, 100 + count)
            d_full = torch.zeros((count * c2, l * 4), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        ctx.kzg_cells_device(d_p.data_ptr(), log_n, log_l, count, d_full.data_ptr(), 0, ORDER)
        ctx.synchronize()
        rng = np.random.default_rng(7 + count)
        patterns = {"random half missing": [sorted(rng.permutation(c2)[:c].tolist()) for _ in range(count)]}
        if log_n == 12:
            patterns["second half missing"] = [list(range(c)) for _ in range(count)]
        for pname, received in patterns.items():
            name = "%s, %s" % (shape, pname)
            out = {"log_n": log_n, "log_l": log_l, "count": count, "cells_received": count * c}
            col = np.array([i for rec_ in received for i in rec_], dtype=np.uint32)
            offsets = (np.arange(count + 1) * c).astype(np.uint32)
            pick = up(np.array([v * c2 + i for v, rec_ in enumerate(received) for i in rec_], dtype=np.int64), np.int64)
            with torch.cuda.stream(side):
                d_half = d_full.index_select(0, pick).contiguous()
                d_col, d_off = up(col, np.int32), up(offsets, np.int32)
                d_polys = torch.zeros((count * n, 4), dtype=torch.int64, device=dev)
                d_cells = torch.zeros((count * c2, l * 4), dtype=torch.int64, device=dev)
                d_ok = torch.zeros(count, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            call = lambda: ctx.kzg_recover_device(d_col.data_ptr(), d_off.data_ptr(), count, count * c, d_half.data_ptr(), log_n, log_l, d_polys.data_ptr(), d_cells.data_ptr(),
                                                  d_ok.data_ptr(), ORDER)
            out["recover_device"] = windows(call, a.reps)
            ctx.synchronize()
            out["outputs_ok"] = bool(d_ok.cpu().numpy().all()) and bool(torch.equal(d_cells, d_full)) and bool(torch.equal(d_polys, d_p))
            ok_all = ok_all and out["outputs_ok"]
            ctx.kernel_timing(True)
            call()
            ctx.synchronize()
            rep = ctx.kernel_timing_report()
            ctx.kernel_timing(False)
            total = sum(x["total_ms"] for x in rep.values())
            new = sum(x["total_ms"] for kname, x in rep.items() if "k_kzg_rec" in kname)
            out["kernels"] = rep
            out["kernel_total_ms"], out["new_kernels_ms"], out["new_kernel_share"] = total, new, new / total if total else 0.0
            out["launches_per_call"] = sum(x["launches"] for x in rep.values())
            # (a) the floor: the three transforms of the working vector and the cells of the result
            with torch.cuda.stream(side):
                d_work = scalars(count * 2 * n, 3)
                d_tab_d, d_tab_c = scalars(count * 2 * n, 4), scalars(count * 2 * n, 5)
                d_ez = scalars(count * 2 * n, 6)
            torch.cuda.synchronize()

            def floor():
                ctx.fr_ntt_many_device(d_work.data_ptr(), log_n + 1, count, True)
                ctx.fr_ntt_many_device(d_work.data_ptr(), log_n + 1, count, False, GEN)
                ctx.fr_ntt_many_device(d_work.data_ptr(), log_n + 1, count, True, GEN)
                ctx.kzg_cells_device(d_p.data_ptr(), log_n, log_l, count, d_cells.data_ptr(), 0, ORDER)

            def route():
                ctx.fr_op_device(0, d_ez.data_ptr(), d_tab_d.data_ptr(), count * 2 * n, d_work.data_ptr())
                ctx.fr_ntt_many_device(d_work.data_ptr(), log_n + 1, count, True)
                ctx.fr_ntt_many_device(d_work.data_ptr(), log_n + 1, count, False, GEN)
                ctx.fr_op_device(0, d_work.data_ptr(), d_tab_c.data_ptr(), count * 2 * n, d_ez.data_ptr())
                ctx.fr_ntt_many_device(d_ez.data_ptr(), log_n + 1, count, True, GEN)
                ctx.kzg_cells_device(d_p.data_ptr(), log_n, log_l, count, d_cells.data_ptr(), 0, ORDER)

            out["floor_transforms_and_cells"] = windows(floor, a.reps)
            out["host_prepared_route"] = windows(route, a.reps)
            out["over_floor"] = out["recover_device"]["median_ms"] / out["floor_transforms_and_cells"]["median_ms"]
            out["over_route"] = out["recover_device"]["median_ms"] / out["host_prepared_route"]["median_ms"]
            if (log_n, count) == (12, 1):                           # the route on honest tables gives the call's coefficients
                cells_host = d_half.cpu().numpy().view(np.uint64).reshape(-1, 4)
                ints = [o.fr_from_mont_limbs([int(w) for w in row]) for row in cells_host]
                cells_int = [ints[kk * l:(kk + 1) * l] for kk in range(c)]
                table, status = rr.slots(col.tolist(), offsets.tolist(), c, log_n, log_l)
                zd, zc = rr.tables(table[0], status[0], log_n, log_l, ORDER)
                ez = rr.ez(table[0], cells_int, zd, log_n, log_l, ORDER)
                limbs = lambda vals: np.array([o.fr_to_mont_limbs(int(x) % R) for x in vals], dtype=np.uint64)
                d_e = up(limbs(ez), np.int64)
                d_zi = up(limbs([pow(zc[j % c2], R - 2, R) for j in range(2 * n)]), np.int64)
                torch.cuda.synchronize()
                ctx.fr_ntt_many_device(d_e.data_ptr(), log_n + 1, 1, True)
                ctx.fr_ntt_many_device(d_e.data_ptr(), log_n + 1, 1, False, GEN)
                d_q = torch.zeros_like(d_e)
                torch.cuda.synchronize()
                ctx.fr_op_device(0, d_e.data_ptr(), d_zi.data_ptr(), 2 * n, d_q.data_ptr())
                ctx.fr_ntt_many_device(d_q.data_ptr(), log_n + 1, 1, True, GEN)
                ctx.synchronize()
                q = d_q.view(2 * n, 4)
                out["route_agrees"] = bool(torch.equal(q[:n], d_p.view(n, 4))) and not bool(q[n:].any())
                ok_all = ok_all and out["route_agrees"]
            if out["outputs_ok"]:
                rec["shapes"][name] = out
            print(name, json.dumps({"recover_ms": out["recover_device"]["median_ms"], "floor_ms": out["floor_transforms_and_cells"]["median_ms"],
                                    "route_ms": out["host_prepared_route"]["median_ms"], "over_floor": out["over_floor"], "over_route": out["over_route"],
                                    "new_kernel_share": out["new_kernel_share"], "new_kernels_ms": out["new_kernels_ms"], "launches": out["launches_per_call"],
                                    "outputs_ok": out["outputs_ok"], "route_agrees": out.get("route_agrees")}), flush=True)
            if a.out:                                               # the record so far: a later shape that runs out of time loses nothing
                os.makedirs(os.path.dirname(a.out), exist_ok=True)
                with open(a.out, "w") as fh:
                    json.dump(rec, fh, indent=1)
            del d_work, d_tab_d, d_tab_c, d_ez, d_half, d_polys, d_cells
        del d_p, d_full
        torch.cuda.empty_cache()
    ctx.set_stream(None)
    ctx.close()
    if not ok_all:
        print("MISSED: a timed call returned a wrong result", flush=True)
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
