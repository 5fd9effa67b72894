"""Same-process timing of the twisted Edwards entry points (blsgpu_fr_edwards_mul_batch_device, _msm_segments_device, the table builds)
with their yardsticks.

    python tools/fr_edwards_time.py [--calls R] [--windows W] [--out profiles/fr_edwards_time.json]

Method of tools/fr_poseidon_time.py: times are HIP events on the stream the calls are enqueued on (the context is put on a torch stream
with set_stream), one pair of events around a window of R back-to-back device-form calls (default 10) after two warm-up calls of the same
shape; W such windows (default 5), the minimum and all of them are recorded, per call.  The curves are the TEST parameter sets of
tests/fr_edwards_ref.py (the library ships none).  Next to every figure, in the same process and run:
  * `estimate_ms`: the shape's count of field products (the formulas' products, one per fr_mul: a doubling 9, a unified addition 11, a
    table addition 8) divided by the product rate of the Poseidon kernels measured in this run (t = 3, sparse, 2^16 preimages).  The
    formula was fixed before the first run; `measured_over_estimate` is the miss.
  * for the MSM shapes, `mul_batch_route_ms`: the same terms through mul_batch alone, the variable-base route a caller had without the
    tables.  It leaves the sums out, so it flatters that route.
Outputs are compared where two routes compute the same thing (`outputs_match`).  No test asserts any of these figures."""
import argparse
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DBL, ADD, MIXED = 9, 11, 8                                         # field products of ed_dbl / ed_add / ed_add_mixed (csrc/fr_edwards.hip.h)
MUL_WINDOW = 3


def mul_products(bits):
    w = (bits + MUL_WINDOW) // MUL_WINDOW
    return 1 + 3 * ADD + MUL_WINDOW * (w - 1) * DBL + w * ADD      # T = x y, the lane's table, the doublings, the window additions


def msm_products(bits, window):
    return ((bits + window) // window) * MIXED                     # per term; the trees and the combine pass are left out


def table_products(n, bits, window):
    w, h = (bits + window) // window, 1 << (window - 1)
    return n * sum(window * i * DBL + (h - 1) * ADD + 1 + 4 * h for i in range(w))      # doublings, multiples, then 4 products an entry to normalise


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bls12_381_amd as b
    from bls12_381_amd import synthetic
    import fr_edwards_ref as ref
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

    def timed(fn):
        fn()
        fn()                                                       # warm-up
        ctx.synchronize()
        return [window(fn, a.calls) for _ in range(a.windows)]

    def to_dev(arr, view):
        return torch.from_numpy(np.ascontiguousarray(arr).view(view)).to(dev)

    def rand_scalars(n, bits, seed):
        x = np.random.RandomState(seed).randint(0, 256, size=(n, 32), dtype=np.uint8)
        full, rest = bits // 8, bits % 8
        x[:, full + (1 if rest else 0):] = 0
        if rest:
            x[:, full] &= (1 << rest) - 1
        return x

    # ---- the product rate the estimates are made from: the t = 3 Poseidon hash of this run ---------------------------------------------------
    c, m = synthetic.poseidon_test_params(3, 8, 57, 1)
    hp = ctx.fr_poseidon(3, 8, 57, c, m)
    n_p = 1 << 16
    d_pin = to_dev(rand_scalars(n_p * 2, 254, 1), np.int64)
    d_pout = torch.zeros((n_p, 4), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    tp = timed(lambda: hp.hash_many_device(d_pin.data_ptr(), n_p, d_pout.data_ptr(), tag=1))
    rate = hp.products_per_permutation * n_p / (min(tp) * 1e-3)
    rec = {"calls_per_window": a.calls, "windows": a.windows, "poseidon_t3_n2^16_ms": min(tp), "poseidon_products_per_s": rate,
           "products": {"dbl": DBL, "add": ADD, "mixed_add": MIXED}, "mul_batch": {}, "msm_segments": {}, "table_build": {}}
    print("poseidon rate %.3g products/s" % rate, flush=True)

    def row_of(ts, products):
        est = products / rate * 1e3
        return {"ms": min(ts), "ms_all": ts, "products": products, "estimate_ms": est, "measured_over_estimate": min(ts) / est}

    curves = {name: ctx.fr_edwards(ref.CURVES[name].a, ref.CURVES[name].d) for name in ("jubjub", "bandersnatch")}
    pools = {}
    for name in curves:
        rng = random.Random(77)
        pools[name] = ref.points_limbs([ref.CURVES[name].odd_order_point(rng) for _ in range(256)])
    ok = True

    # ---- mul_batch ----------------------------------------------------------------------------------------------------------------------------
    e = curves["jubjub"]
    for log_n in (16, 20):
        n = 1 << log_n
        d_xy = to_dev(np.tile(pools["jubjub"], (n // 256, 1, 1)), np.int64)
        d_out = torch.zeros((n, 3, 4), dtype=torch.int64, device=dev)
        for bits in (64, 253):
            d_k = to_dev(rand_scalars(n, bits, bits + log_n), np.uint8)
            torch.cuda.synchronize()
            ts = timed(lambda: e.mul_batch_device(d_xy.data_ptr(), d_k.data_ptr(), bits, n, d_out.data_ptr()))
            row = row_of(ts, mul_products(bits) * n)
            row.update({"n": n, "bits": bits, "products_per_s": mul_products(bits) * n / (min(ts) * 1e-3)})
            rec["mul_batch"]["n2^%d_bits%d" % (log_n, bits)] = row
            print("mul_batch n=2^%d bits=%d" % (log_n, bits), json.dumps({q: row[q] for q in row if not q.endswith("_all")}), flush=True)
        del d_xy, d_out

    # ---- msm_segments over shared bases, the table builds, and the same terms through mul_batch ------------------------------------------------
    for label, name, k, seg, bits, win in (("verkle_2^12x256", "bandersnatch", 1 << 12, 256, 253, 8), ("sapling_2^16x3", "jubjub", 1 << 16, 3, 252, 4)):
        e = curves[name]
        total = k * seg
        bases = pools[name][:seg]
        d_b = to_dev(bases, np.int64)
        torch.cuda.synchronize()
        made = []

        def build():
            made.append(e.bases_from_device(d_b.data_ptr(), seg, bits, win))
            if len(made) > 1:
                made.pop(0).close()

        tb = timed(build)
        t = made[-1]
        rowb = row_of(tb, table_products(seg, bits, win))
        rowb.update({"bases": seg, "bits": bits, "window": win, "includes": "allocation, build, normalisation, the flag's read-back and its synchronisation; every call but the first also frees the table before it"})
        rec["table_build"][label] = rowb
        print("table_build", label, json.dumps({q: rowb[q] for q in rowb if not q.endswith("_all")}), flush=True)
        sc = rand_scalars(total, bits, 5 + seg)
        d_k = to_dev(sc, np.uint8)
        d_off = to_dev(np.arange(0, total + 1, seg, dtype=np.uint32), np.int32)
        d_bf = torch.zeros(k, dtype=torch.int32, device=dev)
        d_out = torch.zeros((k, 3, 4), dtype=torch.int64, device=dev)
        d_xy = to_dev(np.tile(bases, (k, 1, 1)), np.int64)
        d_prod = torch.zeros((total, 3, 4), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        tm = timed(lambda: t.msm_segments_device(d_off.data_ptr(), d_k.data_ptr(), k, total, d_out.data_ptr(), d_bf.data_ptr()))
        tv = timed(lambda: e.mul_batch_device(d_xy.data_ptr(), d_k.data_ptr(), bits, total, d_prod.data_ptr()))
        # the two routes agree on the first segments: the products of segment j, normalised and summed on the host, are out[j]
        ctx.synchronize()
        cv = ref.CURVES[name]
        check_segs = 2
        prods = ref.points_of(e.normalize(d_prod[:check_segs * seg].cpu().numpy().view(np.uint64))[0])
        got = ref.points_of(e.normalize(d_out[:check_segs].cpu().numpy().view(np.uint64))[0])
        same = got == [cv.sum(prods[j * seg:(j + 1) * seg]) for j in range(check_segs)]
        ok = ok and same
        row = row_of(tm, msm_products(bits, win) * total)
        row.update({"segments": k, "terms_per_segment": seg, "bits": bits, "window": win, "terms_per_s": total / (min(tm) * 1e-3), "mul_batch_route_ms": min(tv),
                    "mul_batch_route_ms_all": tv, "mul_batch_route_over_msm": min(tv) / min(tm), "outputs_match": bool(same)})
        rec["msm_segments"][label] = row
        print("msm_segments", label, json.dumps({q: row[q] for q in row if not q.endswith("_all")}), flush=True)
        t.close()
        del d_xy, d_prod, d_k
    ctx.set_stream(None)
    rec["outputs_match"] = ok
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
