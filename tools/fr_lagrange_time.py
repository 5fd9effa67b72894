"""Same-process timing of the Lagrange coefficients (blsgpu_fr_lagrange_segments_device) and of the combines
(blsgpu_g{1,2}_lagrange_combine_device) against the yardsticks they are judged by.

    python tools/fr_lagrange_time.py [--calls 10] [--windows 3] [--out profiles/fr_lagrange_time.json] [--quick]

Times are HIP events on the stream the calls are enqueued on (the context is put on a torch stream with set_stream): one pair of events
around `calls` back-to-back calls (default 10), after a warm-up call of the same shape; W such windows, the minimum and all of them are
recorded, per call.  Nodes are seeded random scalars, every z_s random, lambda and y both written.

  coefficients   2048 x 512, 64 x 4096, 2^16 x 8, and 2^16 x 8 around one segment of 4096.  A call that takes longer than a second is
                 timed as ONE call after its warm-up.
  yardstick      the route the call replaces, for the equal-length shapes whose t x t matrices fit 2^28 elements (2^16 x 8; 2048 x 512
                 and 64 x 4096 do not, so 256 x 512 is run for both sides as well): blsgpu_fr_scan_many_device PRODUCT over the
                 expanded matrices x_i - x_j and z - x_j with 1 on the diagonal -- the expansion (two fr_op_device subtractions and the
                 diagonal) is OUTSIDE the timed region, only the two scans are timed, which is a lower bound of that route; then, untimed,
                 blsgpu_fr_batch_invert_device and one product, and the coefficients must equal the call's limb for limb.
  product rate   blsgpu_fr_op_device mul over 2^24 elements; every shape records its t^2 nseg products over that rate, and over the rate
                 the estimate in the issue was made from (2.0 10^11 products/s, the Poseidon kernels'), next to what was measured.
  combines       G1 2048 x 512 and G2 2048 x 128: the shipped route (coefficients -> mul_batch -> segment sums, one call) with
                 assume_subgroup off and on, against the other route composed from public calls: blsgpu_fr_lagrange_segments_device, then
                 blsgpu_g{1,2}_msm_segments_device with Montgomery scalars over bases made by `*_bases_from_device` from the same shares
                 (that upload, with its subgroup test and its synchronisation, is timed separately and is NOT in the route's figure).
                 The sums are compared as affine points before anything is timed.

No test asserts any of these figures."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ESTIMATE_RATE = 2.0e11                                             # products/s the estimate beforehand was made from
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="segment counts scaled down by 16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import bls12_381_amd as b
    from bls12_381_amd import api
    ctx = b.Context(0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    ctx.set_stream(stream.cuda_stream)
    scale = 16 if a.quick else 1

    def window(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(calls):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / calls

    def timed(fn):
        first = window(fn, 1)                                      # warm-up (its own time decides how the rest is timed)
        ctx.synchronize()
        if first > 1000.0:
            return [window(fn, 1)]
        return [window(fn, a.calls) for _ in range(a.windows)]

    t = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)
    buf = lambda n: torch.empty(max(n, 16), dtype=torch.uint8, device=dev)

    def random_scalars(n, seed):
        """n canonical scalars as Montgomery limbs (any canonical integer is the Montgomery form of some scalar): 32 bytes, top two bits clear"""
        rs = np.random.RandomState(seed)
        s = rs.randint(0, 256, size=(n, 32), dtype=np.uint8)
        s[:, 31] &= 0x3F
        return s

    try:
        commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    rec = {"commit": commit, "calls_per_window": a.calls, "windows": a.windows, "quick": a.quick, "estimate_rate_products_per_s": ESTIMATE_RATE, "coefficients": {},
           "yardstick": {}, "combine": {}}
    ok = True

    # the product-rate reference
    n_mul = 1 << 24
    d_a, d_b, d_c = t(random_scalars(n_mul, 1)), t(random_scalars(n_mul, 2)), buf(n_mul * 32)
    tm = timed(lambda: ctx.fr_op_device(0, d_a.data_ptr(), d_b.data_ptr(), n_mul, d_c.data_ptr()))
    mul_rate = n_mul / min(tm) * 1e3
    rec["fr_op_mul"] = {"n": n_mul, "ms": min(tm), "ms_all": tm, "products_per_s": mul_rate}
    print("fr_op_mul", json.dumps(rec["fr_op_mul"]), flush=True)
    del d_a, d_b, d_c

    def coefficients(name, lens, seed):
        nseg, total = len(lens), int(sum(lens))
        off = np.zeros(nseg + 1, dtype=np.uint32)
        off[1:] = np.cumsum(lens)
        d_n, d_v, d_p, d_off = t(random_scalars(total, seed)), t(random_scalars(total, seed + 1)), t(random_scalars(nseg, seed + 2)), t(off)
        d_lam, d_y, d_fl = buf(total * 32), buf(nseg * 32), buf(nseg)
        call = lambda: ctx.fr_lagrange_segments_device(d_n.data_ptr(), d_off.data_ptr(), nseg, total, d_p.data_ptr(), d_v.data_ptr(), d_lam.data_ptr(), d_y.data_ptr(), d_fl.data_ptr())
        ts = timed(call)
        products = float(sum(int(l) * int(l) for l in lens))
        row = {"nseg": nseg, "total": total, "longest": int(max(lens)), "ms": min(ts), "ms_all": ts, "products": products, "products_per_s": products / min(ts) * 1e3,
               "products_over_fr_op_mul_rate_ms": products / mul_rate * 1e3, "estimate_ms": products / ESTIMATE_RATE * 1e3,
               "all_distinct": bool((d_fl[:nseg] == 1).all().item())}
        row["measured_over_estimate"] = row["ms"] / row["estimate_ms"]
        rec["coefficients"][name] = row
        print(name, json.dumps({k: v for k, v in row.items() if not k.endswith("_all")}), flush=True)
        return d_n, d_p, d_off, d_lam

    def yardstick(name, nseg, tl, seed):
        """the composed route over the expanded matrices of nseg segments of tl nodes; its coefficients against the call's"""
        nonlocal ok
        total, cells = nseg * tl, nseg * tl * tl
        d_n, d_p, d_off, d_lam = coefficients(name, [tl] * nseg, seed)
        with torch.cuda.stream(stream):
            x = d_n.view(nseg, tl, 32)
            rows = x[:, :, None, :].expand(nseg, tl, tl, 32).contiguous()
            cols = x[:, None, :, :].expand(nseg, tl, tl, 32).contiguous()
            zs = d_p.view(nseg, 1, 1, 32).expand(nseg, tl, tl, 32).contiguous()
            diff, num = buf(cells * 32), buf(cells * 32)
            ctx.fr_op_device(2, rows.data_ptr(), cols.data_ptr(), cells, diff.data_ptr())
            ctx.fr_op_device(2, zs.data_ptr(), cols.data_ptr(), cells, num.data_ptr())
            one = t(np.frombuffer(((1 << 256) % R).to_bytes(32, "little"), dtype=np.uint8))
            ar = torch.arange(tl, device=dev)
            diff.view(nseg, tl, tl, 32)[:, ar, ar, :] = one
            num.view(nseg, tl, tl, 32)[:, ar, ar, :] = one
            del rows, cols, zs
            sd, sn = buf(cells * 32), buf(cells * 32)
        stream.synchronize()
        scans = lambda: (ctx.fr_scan_device(api.FR_SCAN_PRODUCT, diff.data_ptr(), tl, nseg * tl, sd.data_ptr()),
                         ctx.fr_scan_device(api.FR_SCAN_PRODUCT, num.data_ptr(), tl, nseg * tl, sn.data_ptr()))
        ts = timed(scans)
        with torch.cuda.stream(stream):
            dd = sd.view(nseg * tl, tl, 32)[:, tl - 1, :].contiguous()
            nn = sn.view(nseg * tl, tl, 32)[:, tl - 1, :].contiguous()
            inv, lam = buf(total * 32), buf(total * 32)
            ctx.fr_batch_invert_device(dd.data_ptr(), total, inv.data_ptr())
            ctx.fr_op_device(0, nn.data_ptr(), inv.data_ptr(), total, lam.data_ptr())
        ctx.synchronize()
        same = bool(torch.equal(lam[:total * 32], d_lam[:total * 32]))
        ok = ok and same
        mine = rec["coefficients"][name]["ms"]
        rec["yardstick"][name] = {"nseg": nseg, "t": tl, "matrix_elements": 2 * cells, "scans_ms": min(ts), "scans_ms_all": ts, "scans_over_call": min(ts) / mine,
                                  "limb_identical": same, "matrix_bytes_over_input_bytes": float(tl)}
        print(name, "yardstick", json.dumps({k: v for k, v in rec["yardstick"][name].items() if not k.endswith("_all")}), flush=True)
        torch.cuda.empty_cache()

    coefficients("2048x512", [512] * (2048 // scale), 10)
    coefficients("64x4096", [4096] * max(64 // scale, 1), 20)
    yardstick("65536x8", (1 << 16) // scale, 8, 30)
    yardstick("256x512", max(256 // scale, 1), 512, 40)
    half = (1 << 15) // scale
    coefficients("65536x8_plus_4096", [8] * half + [4096] + [8] * half, 50)
    torch.cuda.empty_cache()

    def normalized(group, d_xyz, n):
        w = 12 * group
        d_aff, d_i = buf(n * w * 8), buf(n)
        ctx.batch_normalize_device(group, d_xyz.data_ptr(), n, d_aff.data_ptr(), d_i.data_ptr())
        ctx.synchronize()
        return d_aff[:n * w * 8].view(n, w * 8), d_i[:n]

    def combine(name, group, nseg, tl, seed):
        nonlocal ok
        import time
        total = nseg * tl
        xy, inf = ctx.bases_from_scalars(group, random_scalars(total, seed)).download()
        d_xy, d_inf = t(xy), t(inf)
        off = np.arange(nseg + 1, dtype=np.uint32) * tl
        d_n, d_p, d_off = t(random_scalars(total, seed + 1)), t(random_scalars(nseg, seed + 2)), t(off)
        d_out, d_alt, d_lam, d_fl = buf(nseg * 144 * group), buf(nseg * 144 * group), buf(total * 32), buf(nseg)
        shipped = lambda: ctx.lagrange_combine_device(group, d_xy.data_ptr(), d_inf.data_ptr(), d_n.data_ptr(), d_off.data_ptr(), nseg, total, d_p.data_ptr(), d_out.data_ptr(),
                                                      d_fl.data_ptr())
        row = {"group": group, "nseg": nseg, "t": tl}
        ts = timed(shipped)
        row["shipped_ms"], row["shipped_ms_all"] = min(ts), ts
        ctx.set_assume_subgroup(True)
        ts = timed(shipped)
        ctx.set_assume_subgroup(False)
        row["shipped_assume_subgroup_ms"], row["shipped_assume_subgroup_ms_all"] = min(ts), ts
        h0 = time.perf_counter()
        bases = ctx.bases_from_device(group, d_xy.data_ptr(), d_inf.data_ptr(), total)
        ctx.synchronize()
        row["bases_from_device_host_ms"] = (time.perf_counter() - h0) * 1e3

        def other():
            ctx.fr_lagrange_segments_device(d_n.data_ptr(), d_off.data_ptr(), nseg, total, d_p.data_ptr(), 0, d_lam.data_ptr(), 0, 0)
            ctx.msm_segments_device(bases, d_lam.data_ptr(), d_off.data_ptr(), nseg, total, d_alt.data_ptr())
        ctx.set_scalar_form(1)
        try:
            ts = timed(other)
        finally:
            ctx.set_scalar_form(0)
        row["msm_segments_route_ms"], row["msm_segments_route_ms_all"] = min(ts), ts
        ax, ai = normalized(group, d_out, nseg)
        bx, bi = normalized(group, d_alt, nseg)
        row["routes_agree"] = bool(torch.equal(ai, bi)) and bool(torch.equal(ax[ai == 0], bx[bi == 0]))
        ok = ok and row["routes_agree"]
        row["msm_segments_route_over_shipped"] = row["msm_segments_route_ms"] / row["shipped_ms"]
        row["msm_segments_route_over_shipped_assume_subgroup"] = row["msm_segments_route_ms"] / row["shipped_assume_subgroup_ms"]
        rec["combine"][name] = row
        print(name, json.dumps({k: v for k, v in row.items() if not k.endswith("_all")}), flush=True)
        torch.cuda.empty_cache()

    combine("g1_2048x512", 1, 2048 // scale, 512, 60)
    combine("g2_2048x128", 2, 2048 // scale, 128, 70)
    ctx.set_stream(None)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
