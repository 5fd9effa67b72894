"""Same-process timing of the group transforms (blsgpu_g1_ntt_many_device / blsgpu_g2_ntt_many_device), every figure next to the yardstick
it is judged by, measured in the same run.

    python tools/g_ntt_time.py [--reps R] [--out profiles/g_ntt_time.json] [--skip-msm]

Times are HIP events recorded on the stream the context launches on, around one call, after a warm-up call of the same shape (tables,
code objects); median, minimum, maximum and every repetition are recorded.  The inputs are seeded subgroup points ([s] G from
mul_batch_device); a transform works in place and its time does not depend on the values, so the repetitions transform the same
buffer again and again.

  yardstick   the vouched ladder: mul_batch_device under set_assume_subgroup(1), 2^20 G1 points / 2^18 G2 points -> products per second
  throughput  G1 256 x 2^12 and 1 x 2^20, G2 64 x 2^12, forward and inverse, in the shape the plan chooses; `expected_ms` = the call's
              product count, (N/2)(log_n - 1) plus N for the inverse, over the yardstick rate; `ratio` = measured / expected (target <= 1.15)
  latency     G1 1 x 2^12 and 1 x 2^8, G2 1 x 2^10: the lane shape and the team shape, each forced with BLSGPU_GNTT_TEAM_MAX on a context
              of its own, and which one the built-in constant of csrc/gntt_plan.h chooses (it counts B for G1 and 2 B for G2)
  sweep       both shapes at growing numbers of butterflies per stage B (k x 2^10 points): where the crossover constant comes from
  n_msms      orientation for the README: one 2^12 G1 transform written as 2^12 MSMs of 2^12 points over shared bases in ONE call
              (msm_segments_device, base_first all 0), the only single-call formulation without this entry point"""
import argparse
import json
import os
import re
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ENV = "BLSGPU_GNTT_TEAM_MAX"
LANE_MAX, TEAM_MAX = 0, 1 << 40


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "g_ntt_time.json"))
    ap.add_argument("--skip-msm", action="store_true")
    a = ap.parse_args()
    import torch
    import bls12_381_amd as b
    from oracle import bls12_381_ref as o
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    with open(os.path.join(ROOT, "bls12_381_amd", "csrc", "gntt_plan.h")) as fh:
        built_in = int(re.search(r"GNTT_TEAM_MAX_B = (\d+);", fh.read()).group(1))

    def context(team_max=None):
        os.environ.pop(ENV, None)
        if team_max is not None:
            os.environ[ENV] = str(team_max)
        c = b.Context(0)
        os.environ.pop(ENV, None)
        c.set_stream(side.cuda_stream)
        c.set_assume_subgroup(True)
        return c

    ctxs = {"plan": context(), "lane": context(LANE_MAX), "team": context(TEAM_MAX)}
    ctx = ctxs["plan"]

    def timed(fn, reps=a.reps):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(side):
                e0.record(side)
                fn()
                e1.record(side)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "all_ms": ms}

    gens = {1: o.fp_to_mont_limbs(o.G1_GEN[0]) + o.fp_to_mont_limbs(o.G1_GEN[1]),
            2: o.fp_to_mont_limbs(o.G2_GEN[0][0]) + o.fp_to_mont_limbs(o.G2_GEN[0][1]) + o.fp_to_mont_limbs(o.G2_GEN[1][0]) + o.fp_to_mont_limbs(o.G2_GEN[1][1])}

    def scalars(n, seed):
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        s = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=g)
        s[:, 31] &= 0x3F                                            # < 2^254 < r
        return s

    def points(g, n, seed):
        """(d_xy, d_s, d_xyz): the generator n times, n seeded scalars, and [s_i] G as projective wire points"""
        with torch.cuda.stream(side):
            d_xy = torch.from_numpy(np.array(gens[g], dtype=np.uint64).view(np.int64)).to(dev).repeat(n, 1).contiguous()
            d_s = scalars(n, seed)
            d_xyz = torch.zeros((n, 18 * g), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        ctx.mul_batch_device(g, d_xy.data_ptr(), None, d_s.data_ptr(), n, d_xyz.data_ptr())
        ctx.synchronize()
        return d_xy, d_s, d_xyz

    rec = {"reps": a.reps, "built_in_team_max_b": built_in, "yardstick": {}, "throughput": {}, "latency": {}, "sweep": {}}
    rate = {}
    for g, log_n in ((1, 20), (2, 18)):
        n = 1 << log_n
        d_xy, d_s, d_xyz = points(g, n, 7 + g)
        t = timed(lambda: ctx.mul_batch_device(g, d_xy.data_ptr(), None, d_s.data_ptr(), n, d_xyz.data_ptr()))
        rate[g] = n / (t["median_ms"] * 1e-3)
        rec["yardstick"]["G%d" % g] = dict(t, points=n, what="mul_batch_device, set_assume_subgroup(1)", products_per_s=rate[g])
        print("yardstick G%d" % g, json.dumps({"median_ms": t["median_ms"], "products_per_s": rate[g]}), flush=True)
        del d_xy, d_s, d_xyz

    def products(k, log_n, inverse):
        N = k << log_n
        return (N // 2) * (log_n - 1) + (N if inverse else 0)

    for g, k, log_n in ((1, 256, 12), (1, 1, 20), (2, 64, 12)):
        _, _, d_xyz = points(g, k << log_n, 100 * g + log_n)
        for inverse in (False, True):
            t = timed(lambda: ctx.g_ntt_many_device(g, d_xyz.data_ptr(), log_n, k, inverse=inverse))
            p = products(k, log_n, inverse)
            expected = p / rate[g] * 1e3
            name = "G%d %dx2^%d %s" % (g, k, log_n, "inverse" if inverse else "forward")
            rec["throughput"][name] = dict(t, group=g, k=k, log_n=log_n, inverse=inverse, products=p, yardstick_products_per_s=rate[g], expected_ms=expected,
                                           ratio=t["median_ms"] / expected, target_ratio=1.15, shape="team" if (k << log_n) // 2 * g <= built_in else "lane")
            print(name, json.dumps({"median_ms": t["median_ms"], "expected_ms": expected, "ratio": t["median_ms"] / expected}), flush=True)
        del d_xyz

    def both_shapes(g, k, log_n, inverse=False):
        _, _, d_xyz = points(g, k << log_n, 500 * g + log_n + k)
        out = {}
        for shape in ("lane", "team"):
            c = ctxs[shape]
            out[shape] = timed(lambda: c.g_ntt_many_device(g, d_xyz.data_ptr(), log_n, k, inverse=inverse))
        B = (k << log_n) // 2
        out.update(group=g, k=k, log_n=log_n, butterflies_per_stage=B, plan_choice="team" if B * g <= built_in else "lane",
                   faster="team" if out["team"]["median_ms"] < out["lane"]["median_ms"] else "lane")
        chosen, other = out[out["plan_choice"]], out["team" if out["plan_choice"] == "lane" else "lane"]
        # the plan's own choice is the faster one by the medians, or within the other shape's run-to-run spread (max - min) of it
        out["plan_choice_ok"] = bool(chosen["median_ms"] <= other["median_ms"] + (other["max_ms"] - other["min_ms"]))
        return out

    for g, k, log_n in ((1, 1, 12), (1, 1, 8), (2, 1, 10)):
        name = "G%d %dx2^%d" % (g, k, log_n)
        rec["latency"][name] = r = both_shapes(g, k, log_n)
        print("latency", name, json.dumps({"lane_ms": r["lane"]["median_ms"], "team_ms": r["team"]["median_ms"], "plan": r["plan_choice"], "ok": r["plan_choice_ok"]}), flush=True)
    for g, ks in ((1, (2, 8, 16, 32, 64, 128, 256)), (2, (2, 8, 16, 32, 64, 128))):
        for k in ks:
            name = "G%d %dx2^10" % (g, k)
            rec["sweep"][name] = r = both_shapes(g, k, 10)
            print("sweep", name, json.dumps({"B": r["butterflies_per_stage"], "lane_ms": r["lane"]["median_ms"], "team_ms": r["team"]["median_ms"]}), flush=True)

    if not a.skip_msm:
        # one 2^12 transform as 2^12 MSMs of 2^12 points over shared bases: seeded scalars stand in for the matrix w^(jm) (an MSM's time
        # does not depend on the values), the bases are resident, one call
        log_n = 12
        n = 1 << log_n
        bases = ctx.bases_from_scalars(1, scalars(n, 3).cpu().numpy())
        with torch.cuda.stream(side):
            d_s = scalars(n * n, 4)
            d_off = torch.from_numpy((np.arange(n + 1, dtype=np.uint32) * n).view(np.int32)).to(dev)
            d_bf = torch.zeros(n, dtype=torch.int32, device=dev)
            d_out = torch.zeros((n, 18), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        t = timed(lambda: ctx.msm_segments_device(bases, d_s.data_ptr(), d_off.data_ptr(), n, n * n, d_out.data_ptr(), d_base_first=d_bf.data_ptr()), reps=3)
        one = rec["latency"]["G1 1x2^12"]
        rec["n_msms"] = dict(t, log_n=log_n, what="msm_segments_device: 4096 segments of 4096 scalars, base_first all 0",
                             g_ntt_ms=one[one["plan_choice"]]["median_ms"])
        print("n_msms", json.dumps({"median_ms": t["median_ms"], "g_ntt_ms": rec["n_msms"]["g_ntt_ms"]}), flush=True)
        bases.free()
    for c in ctxs.values():
        c.set_stream(None)
        c.close()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)
    # the conditions the figures are judged by: a miss is printed and makes the exit status non-zero (the record is written either way)
    missed = ["throughput %s: ratio %.3f > %.2f" % (n, r["ratio"], r["target_ratio"]) for n, r in rec["throughput"].items() if r["ratio"] > r["target_ratio"]]
    missed += ["latency %s: the plan chooses %s, %s is faster beyond the spread" % (n, r["plan_choice"], r["faster"]) for n, r in rec["latency"].items() if not r["plan_choice_ok"]]
    for m in missed:
        print("MISSED", m, flush=True)
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())
