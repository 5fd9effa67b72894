"""Same-process timing of Poseidon over Fr (blsgpu_fr_poseidon_hash_many_device, blsgpu_fr_poseidon_merkle_device) with its yardsticks.

    python tools/fr_poseidon_time.py [--calls R] [--windows W] [--out profiles/fr_poseidon_time.json]

Method of tools/fr_bary_time.py: times are HIP events on the stream the calls are enqueued on (the context is put on a torch stream with
set_stream), one pair of events around a window of R back-to-back device-form calls (default 10) after two warm-up calls of the same shape;
W such windows (default 5), the minimum and all of them are recorded, per call.  The instances are TEST parameters
(bls12_381_amd.synthetic.poseidon_test_params) with (R_F, R_P) = (8, 57).  In the same process and run:
  * `frac`: the canonical MAC32 rate, products_per_permutation x 128 per permutation over the time, as a fraction of the v_mad_u64_u32
    peak of blsgpu_mad_throughput measured in this run.  products_per_permutation counts field products; the kernels' lazy products are
    9 x 9 limbs with shared reductions, so this is the project's normalised figure, not an instruction count.
  * dense next to sparse for every width, with the product-count ratio next to the time ratio.
  * `composed`: the t = 3 hash at n = 2^16 by the textbook rounds out of fr_op_device calls on t arrays of n scalars (constants and matrix
    entries replicated into arrays once, outside the timing): about 1400 launches, timed ONCE and checked limb-identical.
  * merkle against a loop of hash_many_device calls per level (merkle is one launch per level too: what is compared is the call itself),
    outputs compared.  An earlier revision finished the last levels of whole trees in one launch in LDS; it lost to this loop (1.60 x at
    4096 trees of 64 leaves, 0.98 x at one tree of 2^20) and was removed.
No test asserts any of these figures."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
RF, RP = 8, 57


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bls12_381_amd as b
    from bls12_381_amd import synthetic
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

    def scalars(n, seed):
        x = np.random.RandomState(seed).randint(0, 256, size=(n, 32), dtype=np.uint8)
        x[:, 31] &= 0x3F                                           # < 2^254 < r: canonical limbs
        return torch.from_numpy(x.view(np.int64).reshape(n, 4)).to(dev)

    def mont(v):
        v = (v << 256) % R_ORDER
        return [(v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)]

    peak = max(ctx.mad_throughput(2000) for _ in range(3))
    rec = {"calls_per_window": a.calls, "windows": a.windows, "rounds": [RF, RP], "peak_mac32_per_s": peak, "hash_many": {}, "merkle": {}}
    ok = True
    handles = {}
    for t in (2, 3, 4, 5, 9, 12):
        c, m = synthetic.poseidon_test_params(t, RF, RP, 1)
        handles[t] = (ctx.fr_poseidon(t, RF, RP, c, m), ctx.fr_poseidon(t, RF, RP, c, m, form=b.FR_POSEIDON_DENSE), c, m)

    def hash_row(t, n):
        hs, hd = handles[t][0], handles[t][1]
        d_in = scalars(n * (t - 1), 10 * t + 1)
        d_a, d_b = torch.zeros((n, 4), dtype=torch.int64, device=dev), torch.zeros((n, 4), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()                                   # the buffers were filled on torch's own stream
        with torch.cuda.stream(stream):
            hs.hash_many_device(d_in.data_ptr(), n, d_a.data_ptr(), tag=1)
            hd.hash_many_device(d_in.data_ptr(), n, d_b.data_ptr(), tag=1)
            ctx.synchronize()
            same = bool(torch.equal(d_a, d_b))
        ts = timed(lambda: hs.hash_many_device(d_in.data_ptr(), n, d_a.data_ptr(), tag=1))
        td = timed(lambda: hd.hash_many_device(d_in.data_ptr(), n, d_b.data_ptr(), tag=1))
        ps, pd = hs.products_per_permutation, hd.products_per_permutation
        row = {"t": t, "n": n, "sparse_equals_dense": same, "sparse_ms": min(ts), "sparse_ms_all": ts, "dense_ms": min(td), "dense_ms_all": td,
               "sparse_products": ps, "dense_products": pd, "sparse_perms_per_s": n / min(ts) * 1e3, "dense_perms_per_s": n / min(td) * 1e3,
               "sparse_frac": ps * 128 * n / (min(ts) * 1e-3) / peak, "dense_frac": pd * 128 * n / (min(td) * 1e-3) / peak,
               "dense_over_sparse_time": min(td) / min(ts), "dense_over_sparse_products": pd / ps}
        return row, same, (d_in, d_a)

    for t, n in ((3, 1 << 10), (3, 1 << 16), (3, 1 << 20), (2, 1 << 16), (4, 1 << 16), (5, 1 << 16), (9, 1 << 16), (12, 1 << 16)):
        row, same, _ = hash_row(t, n)
        ok = ok and same
        rec["hash_many"]["t%d_n2^%d" % (t, n.bit_length() - 1)] = row
        print("hash_many t=%d n=%d" % (t, n), json.dumps({q: row[q] for q in row if not q.endswith("_all")}), flush=True)

    # ---- the yardstick the library offered before: the same t = 3 hash out of fr_op_device calls ------------------------------------------
    t, n = 3, 1 << 16
    hs, _, c, m = handles[t]
    d_in = scalars(n * 2, 31).reshape(n, 2, 4)
    d_fused = torch.zeros((n, 4), dtype=torch.int64, device=dev)
    rep = lambda v: torch.from_numpy(np.array(mont(v), dtype=np.uint64).view(np.int64)).to(dev).repeat(n, 1).contiguous()
    buf = lambda: torch.zeros((n, 4), dtype=torch.int64, device=dev)
    d_c = [[rep(c[r][i]) for i in range(t)] for r in range(RF + RP)]
    d_m = [[rep(m[i][j]) for j in range(t)] for i in range(t)]
    s = [rep(1), d_in[:, 0, :].contiguous(), d_in[:, 1, :].contiguous()]
    x, acc = [buf() for _ in range(t)], [[buf(), buf()] for _ in range(t)]
    ta, tb, tc, tm = buf(), buf(), buf(), buf()
    launches = [0]

    def op(code, pa, pb, po):                                      # no operand is ever the output: every call reads and writes distinct arrays
        ctx.fr_op_device(code, pa.data_ptr(), None if pb is None else pb.data_ptr(), n, po.data_ptr())
        launches[0] += 1

    def composed():
        cur = s
        launches[0] = 0
        for r in range(RF + RP):
            full = r < RF // 2 or r >= RF // 2 + RP
            for i in range(t):
                if full or i == 0:
                    op(1, cur[i], d_c[r][i], ta)
                    op(3, ta, None, tb)
                    op(3, tb, None, tc)
                    op(0, tc, ta, x[i])
                else:
                    op(1, cur[i], d_c[r][i], x[i])
            nxt = []
            for i in range(t):
                w = 0
                op(0, x[0], d_m[i][0], acc[i][w])
                for j in range(1, t):
                    op(0, x[j], d_m[i][j], tm)
                    op(1, acc[i][w], tm, acc[i][1 - w])
                    w = 1 - w
                nxt.append(acc[i][w])
            cur = nxt
        return cur[1]

    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        hs.hash_many_device(d_in.data_ptr(), n, d_fused.data_ptr(), tag=1)
        got = composed()
        ctx.synchronize()
        same = bool(torch.equal(got, d_fused))
        ok = ok and same
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        composed()
        e1.record(stream)
        e1.synchronize()
        t_comp = e0.elapsed_time(e1)
    t_fused = timed(lambda: hs.hash_many_device(d_in.data_ptr(), n, d_fused.data_ptr(), tag=1))
    rec["composed_t3_n2^16"] = {"launches": launches[0], "composed_ms_once": t_comp, "fused_ms": min(t_fused), "fused_ms_all": t_fused, "outputs_match": same,
                                "composed_over_fused": t_comp / min(t_fused)}
    print("composed", json.dumps({q: v for q, v in rec["composed_t3_n2^16"].items() if not q.endswith("_all")}), flush=True)
    del d_c, d_m, s, x

    # ---- merkle against a loop of hash_many_device calls per level ---------------------------------------------------------------------------
    for name, t, height, k in (("arity2_1x2^20", 3, 20, 1), ("arity2_4096x2^6", 3, 6, 4096), ("arity8_1x8^6", 9, 6, 1)):
        hs = handles[t][0]
        aa = t - 1
        leaves = k * aa ** height
        d_leaves = scalars(leaves, 50 + t + k)
        count = k * (aa ** height - 1) // (aa - 1)
        d_nodes, d_nodes2 = torch.zeros((count, 4), dtype=torch.int64, device=dev), torch.zeros((count, 4), dtype=torch.int64, device=dev)
        d_roots = torch.zeros((k, 4), dtype=torch.int64, device=dev)

        def loop():
            src, off, nn = d_leaves.data_ptr(), 0, leaves
            for _ in range(height):
                nn //= aa
                hs.hash_many_device(src, nn, d_nodes2.data_ptr() + off * 32, tag=1)
                src = d_nodes2.data_ptr() + off * 32
                off += nn

        torch.cuda.synchronize()                                   # the buffers were filled on torch's own stream
        with torch.cuda.stream(stream):
            hs.merkle_device(d_leaves.data_ptr(), height, k, d_roots.data_ptr(), d_nodes.data_ptr(), tag=1)
            loop()
            ctx.synchronize()
            same = bool(torch.equal(d_nodes, d_nodes2)) and bool(torch.equal(d_roots, d_nodes[count - k:]))
        ok = ok and same
        tm = timed(lambda: hs.merkle_device(d_leaves.data_ptr(), height, k, d_roots.data_ptr(), d_nodes.data_ptr(), tag=1))
        tn = timed(lambda: hs.merkle_device(d_leaves.data_ptr(), height, k, d_roots.data_ptr(), None, tag=1))
        tl = timed(loop)
        ps = hs.products_per_permutation
        row = {"t": t, "height": height, "k": k, "leaves": leaves, "permutations": count, "outputs_match": same, "merkle_ms": min(tm), "merkle_ms_all": tm,
               "merkle_without_nodes_ms": min(tn), "merkle_without_nodes_ms_all": tn, "hash_many_loop_ms": min(tl), "hash_many_loop_ms_all": tl,
               "perms_per_s": count / min(tm) * 1e3, "frac": ps * 128 * count / (min(tm) * 1e-3) / peak, "merkle_over_loop": min(tm) / min(tl)}
        rec["merkle"][name] = row
        print("merkle", name, json.dumps({q: row[q] for q in row if not q.endswith("_all")}), flush=True)
        del d_leaves, d_nodes, d_nodes2
    ctx.set_stream(None)
    rec["outputs_match"] = ok
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
