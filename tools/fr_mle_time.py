"""Same-process timing of the sumcheck round over multilinear tables (blsgpu_fr_sumcheck_round_device) and of a whole sumcheck against the
same work composed from the entry points the library had before: `fr_op_device` and `fr_scan_many_device`.

    python tools/fr_mle_time.py [--m 20 24] [--window-ms T] [--windows W] [--out profiles/fr_mle_time.json]

Times are HIP events on the stream the calls are enqueued on (the context is put on a torch stream with set_stream): one pair of events
around R back-to-back calls, after warm-up calls of the same shape; R is chosen per measurement from a first short window so that a
window lasts at least T ms (default 100; `reps` is recorded with every figure); W such windows, the minimum and all of them are recorded.

The workload is Spartan's outer sumcheck: k = 4 tables (eq, Az, Bz, Cz) of 2^m scalars, the summand f0 f1 f2 - f0 f3, D = 3.
  fused round      ONE call: fold every table at the previous challenge in place, then the four evaluations of the folded tables
  composed round   the same numbers from existing entry points: per table sub / mul / add for the fold (the challenge replicated into a
                   vector beforehand, not timed), sub and two adds for delta, f(2), f(3); per evaluation point three muls, a sub and a
                   `fr_scan_many_device` SUM whose last element is the total -- 48 calls
  whole sumcheck   round 1 plain, rounds 2 .. m fused, the last challenge by a fold; the composition does the same m times over halving
                   sizes.  Both paths run on the device forms with challenges fixed beforehand (no host round trip in either) and start
                   with the same device-to-device copy of the tables, which the rounds consume (`copy_ms` is that copy alone).
Before anything is timed the two paths are run once and compared limb for limb: every round's evaluations and the final values
(`paths_agree`); the tool exits non-zero otherwise.  The yardstick is never the code under test.

Recorded per round call: the bytes it must move -- k 2^m 32 read, plus half of that written when fused -- the resulting GB/s, and next to it
`fr_op_device` mul over equal traffic (96 bytes per element) measured in the same run.  `round_vs_composed` and `sumcheck_vs_composed` are
new time / composed time; the requirement is that both are below 1 at every m.  No test asserts any of these figures."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R_ORDER = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
K = 4
TERMS = [(1, [0, 1, 2]), (R_ORDER - 1, [0, 3])]
MUL, ADD, SUB = 0, 1, 2
SUM = 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, nargs="+", default=[20, 24])
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bls12_381_amd as b
    ctx = b.Context(0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    ctx.set_stream(stream.cuda_stream)

    def window(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for i in range(reps):
            fn(i)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    def timed(fn):
        """(per-call ms of every window, calls per window)"""
        fn(0), fn(1)                                               # warm-up
        ctx.synchronize()
        reps = max(2, min(20000, int(1.1 * a.window_ms / max(window(fn, 2), 1e-4)) + 1))
        return [window(fn, reps) for _ in range(a.windows)], reps

    def scalars_np(n, seed):
        x = np.random.RandomState(seed).randint(0, 256, size=(n, 32), dtype=np.uint8)
        x[:, 31] &= 0x3F                                           # < 2^254 < r: canonical limbs
        return x.view(np.uint64).reshape(n, 4)

    def to_dev(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).to(dev)

    def scalars_dev(n, seed):
        """n canonical scalars made on the device: every limb below 2^62, so the value is below 2^254 < r"""
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        return torch.randint(0, 1 << 62, (n, 4), dtype=torch.int64, device=dev, generator=g)

    def empty(n):
        return torch.empty((max(n, 1), 4), dtype=torch.int64, device=dev)

    op = lambda o, x, y, n, out: ctx.fr_op_device(o, x, y, n, out)
    P = lambda t, off=0: t.data_ptr() + off * 32

    rec = {"window_ms": a.window_ms, "windows": a.windows, "k": K, "terms": "f0 f1 f2 - f0 f3", "sizes": {}}
    ok = True
    with torch.cuda.stream(stream):
        for m in a.m:
            n, h = 1 << m, 1 << (m - 1)
            src = scalars_dev(K * n, 100 + m)                      # the tables, never written
            work = torch.empty_like(src)                           # what the new path consumes
            chal_np = scalars_np(m, 7)
            chal = to_dev(chal_np)
            # the composition's buffers: two sets of folded tables (ping-pong: fr_op's operands do not alias its output), the challenges
            # replicated (round s folds tables of 2^(m-s+2) scalars: 2^(m-s+1) copies of challenge s - 1), and the per-round temporaries
            fold_a, fold_b = empty(K * h), empty(K * h)
            rep = {s: chal[s - 1:s].repeat(max(n >> s, 1), 1) for s in range(1, m + 1)}
            d1, d2 = empty(h), empty(h)
            delta, f2, f3 = empty(K * h), empty(K * h), empty(K * h)
            p1, p2, q, sm, sc = empty(h), empty(h), empty(h), empty(h), empty(h)
            ev_new, ev_old = torch.zeros((m, 4, 4), dtype=torch.int64, device=dev), torch.zeros((m, 4, 4), dtype=torch.int64, device=dev)
            val_new, val_old = empty(K), empty(K)

            def comp_fold(tabs, length, r_vec, dst):
                """tabs: pointers of K tables of `length` scalars -> K tables of length / 2 at dst (packed); returns their pointers"""
                half = length // 2
                out = []
                for j, t in enumerate(tabs):
                    op(SUB, t + half * 32, t, half, P(d1))
                    op(MUL, P(d1), P(r_vec), half, P(d2))
                    op(ADD, t, P(d2), half, P(dst, j * half))
                    out.append(P(dst, j * half))
                return out

            def comp_evals(tabs, length, ev_row):
                """the four evaluations of the round polynomial of K tables of `length` scalars into ev_row (4 scalars)"""
                half = length // 2
                lo = list(tabs)
                hi = [t + half * 32 for t in tabs]
                for j in range(K):
                    op(SUB, hi[j], lo[j], half, P(delta, j * half))
                    op(ADD, hi[j], P(delta, j * half), half, P(f2, j * half))
                    op(ADD, P(f2, j * half), P(delta, j * half), half, P(f3, j * half))
                at = [lo, hi, [P(f2, j * half) for j in range(K)], [P(f3, j * half) for j in range(K)]]
                for t in range(4):
                    f = at[t]
                    op(MUL, f[0], f[1], half, P(p1))
                    op(MUL, P(p1), f[2], half, P(p2))
                    op(MUL, f[0], f[3], half, P(q))
                    op(SUB, P(p2), P(q), half, P(sm))
                    ctx.fr_scan_device(SUM, P(sm), half, 1, P(sc))
                    ev_row[t].copy_(sc[half - 1])

            def composed_round(i):
                """one fused round's work on the untouched tables: fold at challenge 1, evaluations of the folded tables"""
                tabs = comp_fold([P(src, j * n) for j in range(K)], n, rep[1], fold_a)
                comp_evals(tabs, h, ev_old[1])

            def composed_sumcheck(i):
                work.copy_(src)
                tabs, length = [P(work, j * n) for j in range(K)], n
                comp_evals(tabs, length, ev_old[0])
                dst = fold_a
                for s in range(2, m + 1):
                    tabs = comp_fold(tabs, length, rep[s - 1], dst)
                    length //= 2
                    comp_evals(tabs, length, ev_old[s - 1])
                    dst = fold_b if dst is fold_a else fold_a
                last = comp_fold(tabs, length, rep[m], dst)
                for j in range(K):
                    val_old[j].copy_(dst[j])
                return last

            def new_sumcheck(i):
                work.copy_(src)
                ctx.fr_sumcheck_round_device(P(work), n, m, K, TERMS, P(ev_new))
                for s in range(2, m + 1):
                    ctx.fr_sumcheck_round_device(P(work), n, m - s + 2, K, TERMS, P(ev_new, (s - 1) * 4), d_r_prev=P(chal, s - 2))
                ctx.fr_mle_fold_device(P(work), n, 1, K, P(chal, m - 1), P(work), n)
                for j in range(K):
                    val_new[j].copy_(work[j * n])

            # the two paths agree limb for limb before anything is timed
            new_sumcheck(0)
            composed_sumcheck(0)
            ctx.synchronize()
            agree = bool(torch.equal(ev_new, ev_old)) and bool(torch.equal(val_new[:K], val_old[:K]))
            ok = ok and agree
            row = {"m": m, "paths_agree": agree}
            # one round call
            work.copy_(src)
            ev1 = empty(4)
            bytes_plain, bytes_fused = K * n * 32, K * n * 32 + K * h * 32
            t, reps = timed(lambda i: ctx.fr_sumcheck_round_device(P(work), n, m, K, TERMS, P(ev1), d_r_prev=P(chal)))
            row.update({"fused_round_ms": min(t), "fused_round_ms_all": t, "fused_round_reps": reps, "fused_round_bytes": bytes_fused, "fused_round_gb_per_s": bytes_fused / min(t) / 1e6})
            t, reps = timed(lambda i: ctx.fr_sumcheck_round_device(P(work), n, m, K, TERMS, P(ev1)))
            row.update({"plain_round_ms": min(t), "plain_round_ms_all": t, "plain_round_reps": reps, "plain_round_bytes": bytes_plain, "plain_round_gb_per_s": bytes_plain / min(t) / 1e6})
            t, reps = timed(composed_round)
            row.update({"composed_round_ms": min(t), "composed_round_ms_all": t, "composed_round_reps": reps, "composed_round_calls": 48})
            row["round_vs_composed"] = row["fused_round_ms"] / row["composed_round_ms"]
            # fr_op mul over the traffic of a fused round: 96 bytes per element
            ne = bytes_fused // 96
            ma, mb, mo = scalars_dev(ne, 3), scalars_dev(ne, 4), empty(ne)
            t, reps = timed(lambda i: op(MUL, P(ma), P(mb), ne, P(mo)))
            row.update({"fr_op_mul_elements": ne, "fr_op_mul_ms": min(t), "fr_op_mul_ms_all": t, "fr_op_mul_reps": reps, "fr_op_mul_gb_per_s": ne * 96 / min(t) / 1e6})
            del ma, mb, mo
            # the whole sumcheck
            t, reps = timed(lambda i: work.copy_(src))
            row.update({"copy_ms": min(t)})
            t, reps = timed(new_sumcheck)
            row.update({"sumcheck_ms": min(t), "sumcheck_ms_all": t, "sumcheck_reps": reps})
            t, reps = timed(composed_sumcheck)
            row.update({"composed_sumcheck_ms": min(t), "composed_sumcheck_ms_all": t, "composed_sumcheck_reps": reps})
            row["sumcheck_vs_composed"] = row["sumcheck_ms"] / row["composed_sumcheck_ms"]
            row["sumcheck_vs_composed_without_copy"] = (row["sumcheck_ms"] - row["copy_ms"]) / (row["composed_sumcheck_ms"] - row["copy_ms"])
            rec["sizes"][str(m)] = row
            print("m=%d" % m, json.dumps({k: v for k, v in row.items() if not k.endswith("_all")}), flush=True)
            del src, work, fold_a, fold_b, rep, d1, d2, delta, f2, f3, p1, p2, q, sm, sc
    ctx.set_stream(None)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
