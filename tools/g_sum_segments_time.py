"""Same-process timing of the segmented point sums (blsgpu_g{1,2}_sum_segments_device) and of aggregate verification
(blsgpu_bls_fast_aggregate_verify_batch_device) against the yardsticks they are judged by.

    python tools/g_sum_segments_time.py [--calls 10] [--windows 3] [--out profiles/g_sum_segments_time.json] [--quick]

Times are HIP events on the stream the calls are enqueued on (the context is put on a torch stream with set_stream): one pair of events
around `calls` back-to-back calls (default 10), after a warm-up call of the same shape; W such windows, the minimum and all of them are
recorded, per call.  Shapes (keys [k] G made on the device, resident in the wire format):

  g1_2048x512_gathered   2048 segments x 512 keys gathered at random from 2^20 resident keys (and the same terms laid out contiguously)
  g1_64x16384            64 x 16384, contiguous
  g1_65536x8             2^16 x 8, contiguous
  g1_65536x8_plus_2^19   2^16 segments of 8 around one of 2^19, contiguous
  g2_2048x128            2048 x 128 over 2^18 resident G2 keys, contiguous

Next to each shape, in the same run:
  (1) blsgpu_g{1,2}_msm_segments_device with all-one scalars over the same terms -- the route the call replaces.  Contiguous shapes only (it
      cannot gather), and only where no segment is longer than BLSGPU_SEG_LEN_MAX = 4096 points, which that call refuses: the other shapes
      record `msm_segments: null` and why.  Its sums are compared with the call's as affine points before anything is timed.
  (2) blsgpu_g{1,2}_sum_device over `total` projective points -- the library's existing addition rate (ONE team of lanes folds the array:
      it was written for 8 partials).  A call takes seconds, so it is timed as ONE call after one warm-up, whatever --calls says.
Then the aggregate verifier at n = 2^11 signatures x 512 keys each (mode 0, keys gathered from the 2^20) against
blsgpu_bls_verify_batch_device at n = 2^11: the difference is what the aggregation costs.

No test asserts any of these figures."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEG_LEN_MAX = 4096                                                 # include/bls12_381_hip.h BLSGPU_SEG_LEN_MAX
# Fp::one() in the wire format: R = 2^384 mod p (src/fp.rs:83-90)
MONT_ONE = [0x760900000002fffd, 0xebf4000bc40c0002, 0x5f48985753c758ba, 0x77ce585370525745, 0x5c071a97a256ec6d, 0x15f65ec3fa80e493]


def scalars(n, seed):
    import numpy as np
    rs = np.random.RandomState(seed)
    s = rs.randint(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= 0x3F
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="2^16 resident keys, shapes scaled down by 16, no sum_device yardstick")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import bls12_381_amd as b
    ctx = b.Context(0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    ctx.set_stream(stream.cuda_stream)

    def window(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(calls):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / calls

    def timed(fn, calls=None, windows=None):
        fn()                                                       # warm-up
        ctx.synchronize()
        return [window(fn, calls or a.calls) for _ in range(windows or a.windows)]

    t = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)
    scale = 16 if a.quick else 1
    try:
        commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    rec = {"commit": commit, "calls_per_window": a.calls, "windows": a.windows, "quick": a.quick, "shapes": {}}
    ok = True

    def keys(group, n, seed):
        """n resident keys in the wire format: (d_xy, d_inf, the bases handle the MSM yardstick reads them through)"""
        xy, inf = ctx.bases_from_scalars(group, scalars(n, seed)).download()
        d_xy, d_inf = t(xy), t(inf)
        return d_xy, d_inf, ctx.bases_from_device(group, d_xy.data_ptr(), d_inf.data_ptr(), n)

    def normalized(group, d_xyz, n):
        w = 12 * group
        d_a = torch.empty(n * w * 8, dtype=torch.uint8, device=dev)
        d_i = torch.empty(n, dtype=torch.uint8, device=dev)
        ctx.batch_normalize_device(group, d_xyz.data_ptr(), n, d_a.data_ptr(), d_i.data_ptr())
        ctx.synchronize()
        return d_a.view(n, w * 8), d_i

    def same(group, d_x, d_y, n):
        ax, ix = normalized(group, d_x, n)
        ay, iy = normalized(group, d_y, n)
        live = ix == 0
        return bool(torch.equal(ix, iy)) and bool(torch.equal(ax[live], ay[live]))

    def shape(name, group, d_xy, d_inf, npoints, bases, lens, gather_seed=None):
        nonlocal ok
        w = 12 * group
        nseg, total = len(lens), int(sum(lens))
        off = np.zeros(nseg + 1, dtype=np.uint64)
        off[1:] = np.cumsum(lens)
        d_off = t(off)
        d_out = torch.empty(nseg * 18 * group * 8, dtype=torch.uint8, device=dev)
        row = {"group": group, "nseg": nseg, "total": total, "npoints": npoints, "longest": int(max(lens))}
        if gather_seed is not None:
            idx = torch.randint(0, npoints, (total,), dtype=torch.int64, device=dev, generator=torch.Generator(device=dev).manual_seed(gather_seed))
            d_idx = idx.to(torch.int32)
            call = lambda: ctx.sum_segments_device(group, d_xy.data_ptr(), d_inf.data_ptr(), npoints, d_idx.data_ptr(), d_off.data_ptr(), nseg, total, d_out.data_ptr())
            ts = timed(call)
            row["gathered_ms"], row["gathered_ms_all"] = min(ts), ts
            # the same terms laid out contiguously: the gather must not change a sum
            c_xy = d_xy.view(npoints, w * 8)[idx].contiguous().view(-1)
            c_inf = d_inf[idx].contiguous()
            keep = d_out.clone()
            cbases = ctx.bases_from_device(group, c_xy.data_ptr(), c_inf.data_ptr(), total)
        else:
            c_xy, c_inf, cbases, keep = d_xy, d_inf, bases, None
        call = lambda: ctx.sum_segments_device(group, c_xy.data_ptr(), c_inf.data_ptr(), total, 0, d_off.data_ptr(), nseg, total, d_out.data_ptr())
        ts = timed(call)
        row["ms"], row["ms_all"] = min(ts), ts
        row["adds_per_s"] = total / min(ts) * 1e3
        if keep is not None:
            row["gather_matches_contiguous"] = same(group, keep, d_out, nseg)
            ok = ok and row["gather_matches_contiguous"]
        # (1) the all-ones segmented MSM
        if max(lens) <= SEG_LEN_MAX:
            ones = np.zeros((total, 32), dtype=np.uint8)
            ones[:, 0] = 1
            d_s, d_o32 = t(ones), t(off.astype(np.uint32))
            d_m = torch.empty(nseg * 18 * group * 8, dtype=torch.uint8, device=dev)
            mcall = lambda: ctx.msm_segments_device(cbases, d_s.data_ptr(), d_o32.data_ptr(), nseg, total, d_m.data_ptr())
            tm = timed(mcall)
            row["msm_segments_ms"], row["msm_segments_ms_all"] = min(tm), tm
            row["msm_segments_matches"] = same(group, d_m, d_out, nseg)
            row["msm_segments_over_sum_segments"] = min(tm) / row["ms"]
            ok = ok and row["msm_segments_matches"]
            del d_s, d_m
        else:
            row["msm_segments_ms"] = None
            row["msm_segments_why_not"] = "a segment is longer than BLSGPU_SEG_LEN_MAX = %d points: the call refuses it" % SEG_LEN_MAX
        # (2) the existing fold of `total` projective points by one team: ONE timed call
        if not a.quick:
            d_p = torch.zeros((total, 3, w // 2 * 8), dtype=torch.uint8, device=dev)
            d_p[:, :2, :] = c_xy[:total * w * 8].view(total, 2, w // 2 * 8)
            d_p[:, 2, :] = t(np.array(MONT_ONE + [0] * (w // 2 - 6), dtype=np.uint64))                                           # Z = 1
            d_r = torch.empty(18 * group * 8, dtype=torch.uint8, device=dev)
            scall = lambda: ctx.point_sum_device(group, d_p.data_ptr(), total, d_r.data_ptr())
            tsu = timed(scall, calls=1, windows=1)
            row["sum_device_ms"] = tsu[0]
            row["sum_device_over_sum_segments"] = tsu[0] / row["ms"]
            del d_p
        rec["shapes"][name] = row
        print(name, json.dumps({k: v for k, v in row.items() if not k.endswith("_all")}), flush=True)
        torch.cuda.empty_cache()

    nk1 = (1 << 20) // scale
    d_xy1, d_inf1, bases1 = keys(1, nk1, 31)
    shape("g1_2048x512_gathered", 1, d_xy1, d_inf1, nk1, bases1, [512] * (2048 // scale), gather_seed=7)
    shape("g1_64x16384", 1, d_xy1, d_inf1, nk1, bases1, [16384] * (64 // scale))
    shape("g1_65536x8", 1, d_xy1, d_inf1, nk1, bases1, [8] * ((1 << 16) // scale))
    half = (1 << 15) // scale
    shape("g1_65536x8_plus_2^19", 1, d_xy1, d_inf1, nk1, bases1, [8] * half + [(1 << 19) // scale] + [8] * half)
    nk2 = (1 << 18) // scale
    d_xy2, d_inf2, bases2 = keys(2, nk2, 32)
    shape("g2_2048x128", 2, d_xy2, d_inf2, nk2, bases2, [128] * (2048 // scale))
    del d_xy2, d_inf2, bases2
    torch.cuda.empty_cache()

    # aggregate verification: n signatures x 512 keys each against n plain verifications (mode 0: keys in G1, signatures in G2)
    n, per = (1 << 11) // scale, 512
    dst = b"BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_"
    rs = np.random.RandomState(99)
    msgs = [bytes(rs.randint(0, 256, size=32, dtype=np.uint8)) for _ in range(n)]
    hxy, hinf = ctx.batch_normalize(2, ctx.hash_to_curve(2, msgs, dst))
    sig_b = ctx.points_to_bytes(2, hxy, hinf, compressed=True)        # valid encodings of subgroup points: every stage runs, the verdicts are 0
    kxy = d_xy1.view(nk1, 96)[:n].cpu().numpy().view(np.uint64)
    pk_b = ctx.points_to_bytes(1, kxy, np.zeros(n, dtype=np.uint8), compressed=True)
    moff = np.arange(n + 1, dtype=np.uint64) * 32
    koff = np.arange(n + 1, dtype=np.uint64) * per
    d_idx = torch.randint(0, nk1, (n * per,), dtype=torch.int64, device=dev, generator=torch.Generator(device=dev).manual_seed(11)).to(torch.int32)
    d_sig, d_pk, d_msgs, d_moff, d_koff, d_dst = t(sig_b), t(pk_b), t(np.frombuffer(b"".join(msgs), dtype=np.uint8)), t(moff), t(koff), t(np.frombuffer(dst, dtype=np.uint8))
    d_v = torch.empty(n, dtype=torch.uint8, device=dev)
    agg = lambda: ctx.bls_fast_aggregate_verify_device(0, d_xy1.data_ptr(), d_inf1.data_ptr(), nk1, d_idx.data_ptr(), d_koff.data_ptr(), n * per, d_sig.data_ptr(),
                                                       d_msgs.data_ptr(), d_moff.data_ptr(), n, d_dst.data_ptr(), len(dst), d_v.data_ptr())
    plain = lambda: ctx.bls_verify_batch_device(0, d_pk.data_ptr(), d_sig.data_ptr(), d_msgs.data_ptr(), d_moff.data_ptr(), n, d_dst.data_ptr(), len(dst), d_v.data_ptr())
    ta, tp = timed(agg), timed(plain)
    rec["aggregate_verify"] = {"mode": 0, "n": n, "keys_per_signature": per, "resident_keys": nk1, "aggregate_ms": min(ta), "aggregate_ms_all": ta, "verify_batch_ms": min(tp),
                               "verify_batch_ms_all": tp, "aggregation_costs_ms": min(ta) - min(tp)}
    print("aggregate_verify", json.dumps({k: v for k, v in rec["aggregate_verify"].items() if not k.endswith("_all")}), flush=True)
    ctx.set_stream(None)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
