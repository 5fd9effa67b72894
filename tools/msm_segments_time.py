"""Same-box timing of the segmented MSM (blsgpu_g{1,2}_msm_segments_device) against what a caller does without it.

    python tools/msm_segments_time.py [--reps R] [--out profiles/msm_segments_time.json] [--only NAME]

Shapes and baselines (issue "segmented MSM"):
    g1_4096x64     4096 segments x 64 points, disjoint bases    a loop of blsgpu_g1_msm_device calls ending in one synchronise
    g1_1024x256    1024 x 256, disjoint                         the same loop
    g1_256x4096    256 x 4096 over SHARED bases                 blsgpu_g1_msm_many
    g2_1024x64     1024 x 64, disjoint                          a loop of blsgpu_g2_msm_device calls
Seeded inputs; the new path and the baseline run in the same process, alternating, and their outputs are compared as affine points.
Times are whole calls (host wall clock around the enqueue and one synchronise).  `mac32_frac` is a whole-call figure computed the way
bench.py computes its roofline: canonical MAC32 of the bucket additions (one complete mixed addition of 11 Fp products x 300 MAC32 per
(point, 4-bit window); G2: 3 Fp products per Fp2 product) / time / the v_mad_u64_u32 rate measured live (Context.mad_throughput).
Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("g1_4096x64", 1, 4096, 64, "loop"), ("g1_1024x256", 1, 1024, 256, "loop"),
          ("g1_256x4096", 1, 256, 4096, "many"), ("g2_1024x64", 2, 1024, 64, "loop")]


def scalars(n, seed):
    rs = np.random.RandomState(seed)
    s = rs.randint(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= 0x3F
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    import torch
    import bls12_381_amd as b
    from bls12_381_amd._lib import check
    ctx = b.Context(0)
    dev = torch.device("cuda", 0)
    peak = max(ctx.mad_throughput(2000) for _ in range(3))
    rec = {"peak_mac32_per_s": peak, "reps": a.reps, "shapes": {}}
    for name, g, k, ln, base in SHAPES:
        if a.only and a.only != name:
            continue
        W = 18 if g == 1 else 36
        shared = base == "many"
        total = k * ln
        bases = ctx.bases_from_scalars(g, scalars(ln if shared else total, 1000 + g))
        S = scalars(total, 2000 + k + ln)
        off = (np.arange(k + 1, dtype=np.uint32) * ln).astype(np.uint32)
        d_s = torch.from_numpy(S).to(dev)
        d_off = torch.from_numpy(off.view(np.int32)).to(dev)
        d_bf = torch.zeros(k, dtype=torch.int32, device=dev) if shared else None
        d_new = torch.zeros((k, W), dtype=torch.int64, device=dev)
        d_old = torch.zeros((k, W), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()

        def run_new():
            ctx.msm_segments_device(bases, d_s.data_ptr(), d_off.data_ptr(), k, total, d_new.data_ptr(),
                                    d_base_first=None if d_bf is None else d_bf.data_ptr())
            ctx.synchronize()

        def run_old():
            if shared:
                fn = ctx.lib.blsgpu_g1_msm_many_device if g == 1 else ctx.lib.blsgpu_g2_msm_many_device
                check(fn(ctx.h, bases.handle, 0, d_s.data_ptr(), ln, k, d_old.data_ptr()), "msm_many_device")
            else:
                for j in range(k):
                    ctx.msm_device(bases, d_s[j * ln].data_ptr(), ln, d_old[j].data_ptr(), first=j * ln)
            ctx.synchronize()

        run_new(); run_old()                                       # warm-up (scratch, code objects)
        tn, to = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter(); run_new(); tn.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); run_old(); to.append(time.perf_counter() - t0)
        A = ctx.batch_normalize(g, d_new.cpu().numpy().view(np.uint64))
        B = ctx.batch_normalize(g, d_old.cpu().numpy().view(np.uint64))
        same = bool(np.array_equal(A[1], B[1]) and np.array_equal(A[0][A[1] == 0], B[0][B[1] == 0]))
        sn, so = min(tn), min(to)
        mac32 = total * 64 * 11 * 300 * (3 if g == 2 else 1)
        rec["shapes"][name] = {"group": g, "segments": k, "len": ln, "baseline": "msm_many" if shared else "loop of msm_device",
                               "segments_ms": sn * 1e3, "baseline_ms": so * 1e3, "speedup": so / sn,
                               "segments_points_per_s": total / sn, "baseline_points_per_s": total / so,
                               "mac32_frac_whole_call": mac32 / sn / peak, "outputs_match": same,
                               "segments_ms_all": [x * 1e3 for x in tn], "baseline_ms_all": [x * 1e3 for x in to]}
        print(name, json.dumps({x: rec["shapes"][name][x] for x in ("segments_ms", "baseline_ms", "speedup", "outputs_match")}), flush=True)
        if not same:
            print("MISMATCH", name, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)
    ok = all(v["outputs_match"] for v in rec["shapes"].values())
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
