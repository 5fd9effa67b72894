"""Same-box timing of the batched Fr transform (blsgpu_fr_ntt_many_device) against what a caller does without it.

    python tools/fr_ntt_many_time.py [--reps R] [--out profiles/fr_ntt_many_time.json] [--only NAME]

Baseline = a loop of blsgpu_fr_ntt_device calls, one per vector, ended by one synchronise; for the coset rows that loop is preceded
(forward) or followed (inverse) by ONE blsgpu_fr_op_device multiplication of the whole array by a prebuilt power table (g^j, or g^-j,
repeated per vector; building it is timed on neither side, and the new path's own table is built by the warm-up call).
Seeded inputs; the new path and the baseline run in the same process, alternating, each on its own copy of the input, and their
outputs are compared limb for limb (`outputs_match`); a mismatch makes the exit status non-zero.  Times are whole calls (host wall
clock around the enqueue and one synchronise), the minimum and all repetitions are recorded.  `passes` is the number of kernels of
the new path that read and write every element once (fr_plan.h), `bytes_per_element_pass` = 64 (32 read + 32 written), and
`gb_per_s` = total * 64 * passes / time: to be read against HBM bandwidth on the shapes that do not fit the caches.
Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name, k, log_n, coset, inverse
SHAPES = [("4096x2^6", 4096, 6, False, False), ("4096x2^8", 4096, 8, False, False), ("256x2^12", 256, 12, False, False),
          ("64x2^16", 64, 16, False, False), ("16x2^20", 16, 20, False, False), ("4x2^24", 4, 24, False, False),
          ("256x2^12_coset_fwd", 256, 12, True, False), ("256x2^12_coset_inv", 256, 12, True, True),
          ("16x2^20_coset_fwd", 16, 20, True, False), ("16x2^20_coset_inv", 16, 20, True, True)]
R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def passes_of(log_n):
    """kernels of the new path that touch every element (fr_plan.h): the tile kernel + the global passes above it"""
    if log_n <= 10:
        return 1
    m = log_n - 10
    return 1 + ((m + 6) // 7 if log_n >= 20 else (m + 1) // 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    import torch
    import bls12_381_amd as b
    from bls12_381_amd._lib import check
    ctx = b.Context(0)
    dev = torch.device("cuda", 0)
    g = b.FR_GENERATOR
    rec = {"reps": a.reps, "coset": g, "bytes_per_element_pass": 64, "shapes": {}}
    for name, k, log_n, coset, inverse in SHAPES:
        if a.only and a.only != name:
            continue
        n = 1 << log_n
        total = k * n
        rs = np.random.RandomState(1000 + log_n + k)
        x = rs.randint(0, 256, size=(total, 32), dtype=np.uint8)
        x[:, 31] &= 0x3F                                           # < 2^254 < r: canonical limbs
        d_in = torch.from_numpy(x.view(np.int64).reshape(total, 4)).to(dev)
        d_new = torch.empty_like(d_in)
        d_old = torch.empty_like(d_in)
        d_pw = None
        if coset:
            # g^j (forward) / g^-j (inverse), j < n, as Montgomery limbs, repeated for every vector
            base = pow(g, -1, R_ORDER) if inverse else g
            vals, cur = [], 1
            for _ in range(n):
                vals.append(cur * (1 << 256) % R_ORDER)
                cur = cur * base % R_ORDER
            pw = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype=np.int64).reshape(n, 4)
            d_pw = torch.from_numpy(pw.copy()).to(dev).repeat(k, 1).contiguous()
        torch.cuda.synchronize()

        def run_new():
            ctx.fr_ntt_many_device(d_new.data_ptr(), log_n, k, inverse=inverse, coset=g if coset else None)
            ctx.synchronize()

        def run_old():
            if coset and not inverse:
                check(ctx.lib.blsgpu_fr_op_device(ctx.h, 0, d_old.data_ptr(), d_pw.data_ptr(), total, d_old.data_ptr(), None), "fr_op_device")
            for v in range(k):
                ctx.fr_ntt_device(d_old.data_ptr() + v * n * 32, log_n, inverse)
            if coset and inverse:
                check(ctx.lib.blsgpu_fr_op_device(ctx.h, 0, d_old.data_ptr(), d_pw.data_ptr(), total, d_old.data_ptr(), None), "fr_op_device")
            ctx.synchronize()

        def timed(fn, d):
            d.copy_(d_in); torch.cuda.synchronize()
            t0 = time.perf_counter(); fn(); return time.perf_counter() - t0

        timed(run_new, d_new); timed(run_old, d_old)               # warm-up (scratch, tables, code objects)
        tn, to = [], []
        for _ in range(a.reps):
            tn.append(timed(run_new, d_new))
            to.append(timed(run_old, d_old))
        same = bool(torch.equal(d_new, d_old))
        sn, so = min(tn), min(to)
        p = passes_of(log_n)
        rec["shapes"][name] = {"k": k, "log_n": log_n, "coset": coset, "inverse": inverse,
                               "baseline": ("fr_op_device + " if coset and not inverse else "") + "loop of fr_ntt_device" + (" + fr_op_device" if coset and inverse else ""),
                               "many_ms": sn * 1e3, "baseline_ms": so * 1e3, "speedup": so / sn, "baseline_spread_max_over_min": max(to) / so,
                               "many_elements_per_s": total / sn, "passes": p, "gb_per_s": total * 64 * p / sn / 1e9, "outputs_match": same,
                               "many_ms_all": [t * 1e3 for t in tn], "baseline_ms_all": [t * 1e3 for t in to]}
        print(name, json.dumps({q: rec["shapes"][name][q] for q in ("many_ms", "baseline_ms", "speedup", "baseline_spread_max_over_min", "gb_per_s", "outputs_match")}), flush=True)
        if not same:
            print("MISMATCH", name, flush=True)
        del d_in, d_new, d_old, d_pw
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)
    ok = all(v["outputs_match"] for v in rec["shapes"].values())
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
