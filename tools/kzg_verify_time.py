"""Same-process timing of batched KZG cell-proof verification (blsgpu_kzg_verify_cells_device), every figure next to the yardsticks it is
judged by, measured in the same run.

    python tools/kzg_verify_time.py [--reps R] [--out profiles/kzg_verify_time.json] [--quick]

Times are HIP events recorded on the stream the context launches on, around WINDOWS of 10 calls after a warm-up call of the same shape
(tables, code objects, scratch); a figure is a window's time over 10, and median, minimum, maximum and every window are recorded.  The
inputs are honest: a powers-of-tau SRS, random polynomials, their cells and proofs from blsgpu_kzg_cells_device /
blsgpu_kzg_multiproof_proofs_device, their commitments from one segmented MSM over the SRS -- so every timed call must also return
verdict 1 for every batch, and one with a changed cell verdict 0 (`verdicts_ok`).

  shapes      (12, 6) with m = 128 x {1, 16, 64} cells (the cells of 1, 16, 64 blobs, bit-reversed numbering): as ONE batch, as one batch
              per blob and as one batch per cell; m = 2048 as batches of one cell is the last of these at 16 blobs
  yardsticks  the one-cell-per-batch form of the same call over the same cells (the gain of the combination); blsgpu_g1_mul_batch_device
              over 3 m products and blsgpu_pairing_batch_device over nseg pairings on their own (the floor the chain cannot beat), the
              products with and without blsgpu_set_assume_subgroup
  stages      one more call with blsgpu_kernel_timing on: the kernels of the chain grouped into its stages; `fr_share` is the part of
              the kernels that are new with this call (offsets, weights, fold, finish)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WINDOW = 10
STAGES = (("offsets + weights + gather", ("k_kzgv_offsets", "k_kzgv_weights")), ("point products", ("k_mul_batch",)),
          ("normalisation + segment sums", ("k_proj_import", "k_batch_normalize", "k_proj_to_affine", "k_gsum")), ("cell copy + inverse transforms", ("k_kzg_scalar_copy", "k_fr_")),
          ("fold", ("k_kzgv_fold",)), ("MSM over S[0..l)", ("k_msm_seg", "k_proj_export")), ("finish + verdict", ("k_kzgv_finish", "k_kzgv_verdict")))
NEW = ("offsets + weights + gather", "fold", "finish + verdict")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kzg_verify_time.json"))
    ap.add_argument("--quick", action="store_true", help="1 and 16 blobs only")
    a = ap.parse_args()
    import torch
    import bls12_381_amd as b
    from oracle import bls12_381_ref as o
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    ctx = b.Context(0)
    ctx.set_stream(side.cuda_stream)
    R = o.R_ORDER
    log_n, log_l, n, l, c2 = 12, 6, 4096, 64, 128

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

    def affine(d_xyz, count):
        d_xy = torch.zeros((count, 12), dtype=torch.int64, device=dev)
        d_inf = torch.zeros(count, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()                                   # the buffers were zeroed on another stream than the context's
        ctx.batch_normalize_device(1, d_xyz.data_ptr(), count, d_xy.data_ptr(), d_inf.data_ptr())
        ctx.synchronize()
        return d_xy, d_inf

    def u32(values):
        return torch.from_numpy(np.asarray(values, dtype=np.uint32).view(np.int32)).to(dev)

    tau = o.SplitMix64(7594).scalar()
    srs = ctx.bases_from_scalars(1, [pow(tau, u, R) for u in range(n)])
    q2 = ctx.bases_from_scalars(2, [pow(tau, l, R)])
    q_xy = q2.download()[0][0]
    q2.free()
    mp = ctx.kzg_multiproof_create(srs, log_n, log_l)
    handle = ctx.kzg_cell_verifier_create(srs, log_n, log_l, q_xy)
    rec = {"reps": a.reps, "window": WINDOW, "device": torch.cuda.get_device_name(0), "log_n": log_n, "log_l": log_l, "shapes": {}}
    ok_all = True
    for blobs in ((1, 16) if a.quick else (1, 16, 64)):
        m = blobs * c2
        with torch.cuda.stream(side):
            d_p = scalars(blobs * n, 100 + blobs)
            d_cells = torch.zeros((m * l, 4), dtype=torch.int64, device=dev)
            d_proofs = torch.zeros((m, 18), dtype=torch.int64, device=dev)
            d_commit = torch.zeros((blobs, 18), dtype=torch.int64, device=dev)
            d_off = u32(np.arange(blobs + 1) * n)
            d_bf = torch.zeros(blobs, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ctx.kzg_cells_device(d_p.data_ptr(), log_n, log_l, blobs, d_cells.data_ptr(), b.KZG_FORM_COEFFS, b.FR_ORDER_BITREV)
        mp.proofs_device(d_p.data_ptr(), blobs, d_proofs.data_ptr(), b.KZG_FORM_COEFFS, b.FR_ORDER_BITREV)
        ctx.set_scalar_form(1)
        try:
            ctx.msm_segments_device(srs, d_p.data_ptr(), d_off.data_ptr(), blobs, blobs * n, d_commit.data_ptr(), d_base_first=d_bf.data_ptr())
        finally:
            ctx.set_scalar_form(0)
        ctx.synchronize()
        pxy, pinf = affine(d_proofs, m)
        cxy, cinf = affine(d_commit, blobs)
        d_row, d_col = u32(np.arange(m) // c2), u32(np.arange(m) % c2)
        d_wrong = d_cells.clone()
        d_wrong[(m - 1) * l + 5, 0] ^= 1
        torch.cuda.synchronize()
        cuts = {"one batch": [0, m], "one batch per blob": list(range(0, m + 1, c2)), "one batch per cell": list(range(m + 1))}
        for cut, offsets in cuts.items():
            nseg = len(offsets) - 1
            name = "m = %d, %s" % (m, cut)
            d_offsets = u32(offsets)
            d_r = scalars(nseg, 7 + nseg)
            d_verdict = torch.zeros(nseg, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()

            def call(cells=d_cells):
                handle.verify_device(cxy.data_ptr(), cinf.data_ptr(), blobs, d_row.data_ptr(), d_col.data_ptr(), cells.data_ptr(), pxy.data_ptr(), pinf.data_ptr(), d_offsets.data_ptr(),
                                     nseg, m, d_r.data_ptr(), d_verdict.data_ptr(), None, b.FR_ORDER_BITREV)

            out = {"blobs": blobs, "m": m, "nseg": nseg, "verify_device": windows(call, a.reps)}
            ctx.synchronize()
            good = d_verdict.cpu().numpy().copy()
            call(d_wrong)
            ctx.synchronize()
            bad = d_verdict.cpu().numpy()
            out["verdicts_ok"] = bool((good == 1).all() and bad[-1] == 0 and (bad[:-1] == 1).all())
            ok_all = ok_all and out["verdicts_ok"]
            out["verify_device_assume_subgroup"] = None
            ctx.set_assume_subgroup(True)
            try:
                out["verify_device_assume_subgroup"] = windows(call, a.reps)
                ctx.synchronize()
                ok_all = ok_all and bool((d_verdict.cpu().numpy() == 1).all())
            finally:
                ctx.set_assume_subgroup(False)
            # the stage split of one call
            ctx.kernel_timing(True)
            call()
            ctx.synchronize()
            rep = ctx.kernel_timing_report()
            ctx.kernel_timing(False)
            out["kernels"] = rep
            out["stages_ms"] = {s: sum(x["total_ms"] for kname, x in rep.items() if any(p in kname for p in pre)) for s, pre in STAGES}
            total = sum(x["total_ms"] for x in rep.values())
            out["stages_ms"]["pairing products + identity test"] = total - sum(out["stages_ms"].values())
            out["fr_share"] = sum(out["stages_ms"][s] for s in NEW) / total if total else 0.0
            out["dominant_stage"] = max(out["stages_ms"], key=out["stages_ms"].get)
            # the floor: the 3 m products and the nseg pairings on their own
            with torch.cuda.stream(side):
                d_s3 = scalars(3 * m, 5)
                d_xy3 = pxy.repeat(3, 1).contiguous()
                d_inf3 = pinf.repeat(3).contiguous()
                d_out3 = torch.zeros((3 * m, 18), dtype=torch.int64, device=dev)
                d_g2 = torch.from_numpy(np.tile(q_xy, (nseg, 1)).view(np.int64)).to(dev)
                d_g1 = pxy[:1].repeat(nseg, 1).contiguous()
                d_z = torch.zeros(nseg, dtype=torch.uint8, device=dev)
                d_gt = torch.zeros((nseg, 72), dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            ctx.set_scalar_form(1)
            try:
                out["mul_batch_3m"] = windows(lambda: ctx.mul_batch_device(1, d_xy3.data_ptr(), d_inf3.data_ptr(), d_s3.data_ptr(), 3 * m, d_out3.data_ptr()), a.reps)
                ctx.set_assume_subgroup(True)
                try:
                    out["mul_batch_3m_assume_subgroup"] = windows(lambda: ctx.mul_batch_device(1, d_xy3.data_ptr(), d_inf3.data_ptr(), d_s3.data_ptr(), 3 * m, d_out3.data_ptr()), a.reps)
                finally:
                    ctx.set_assume_subgroup(False)
            finally:
                ctx.set_scalar_form(0)
            out["pairing_batch_nseg"] = windows(lambda: ctx.pairing_batch_device(d_g1.data_ptr(), d_g2.data_ptr(), nseg, d_gt.data_ptr(), d_z.data_ptr(), d_z.data_ptr()),
                                                a.reps if nseg <= 2048 else 2, WINDOW if nseg <= 2048 else 2)
            out["floor_ms"] = out["mul_batch_3m"]["median_ms"] + out["pairing_batch_nseg"]["median_ms"]
            rec["shapes"][name] = out
            del d_s3, d_xy3, d_inf3, d_out3, d_g2, d_g1, d_gt
        per_cell = rec["shapes"]["m = %d, one batch per cell" % m]["verify_device"]["median_ms"]
        for cut in ("one batch", "one batch per blob"):
            s = rec["shapes"]["m = %d, %s" % (m, cut)]
            s["one_cell_per_batch_ms"] = per_cell
            s["gain_of_the_combination"] = per_cell / s["verify_device"]["median_ms"]
        for cut in cuts:
            s = rec["shapes"]["m = %d, %s" % (m, cut)]
            print("m = %d, %s" % (m, cut), json.dumps({"verify_ms": s["verify_device"]["median_ms"], "assume_subgroup_ms": s["verify_device_assume_subgroup"]["median_ms"],
                                                       "floor_ms": s["floor_ms"], "mul_batch_3m_ms": s["mul_batch_3m"]["median_ms"], "pairings_ms": s["pairing_batch_nseg"]["median_ms"],
                                                       "fr_share": s["fr_share"], "dominant": s["dominant_stage"], "verdicts_ok": s["verdicts_ok"], "stages_ms": s["stages_ms"]}), flush=True)
        if a.out:                                                 # the record so far: a later shape that runs out of time loses nothing
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "w") as fh:
                json.dump(rec, fh, indent=1)
        del d_p, d_cells, d_proofs, d_wrong
        torch.cuda.empty_cache()
    handle.close()
    mp.close()
    srs.free()
    ctx.set_stream(None)
    ctx.close()
    if not ok_all:
        print("MISSED: a timed call returned a wrong verdict", flush=True)
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
