"""Same-process timing of the Fr expression programs (blsgpu_fr_expr_eval_device) against the same expression composed from the entry
points the library had before.

    python tools/fr_expr_time.py [--calls 10] [--windows 3] [--out profiles/fr_expr_time.json] [--only LOG_N]

Times are HIP events on the stream the calls are enqueued on (the context is put on a torch stream with set_stream): one pair of events
around `calls` back-to-back calls (default 10), after a warm-up call of the same shape; W such windows, the minimum and all of them are
recorded, per call.  At N = 2^16, 2^20 and 2^24 rows:

  (a) the standard vanilla-PLONK quotient program of bls12_381_amd.synthetic (36 instructions, 21 products per row, 15 full-length
      columns of which z is also read at the next row, log_stride = 2, 1 / Z_H as a column of 4, four challenges as columns of 1);
  (b) the one-instruction program MUL col0 col1 against `fr_op_device` mul over as many elements: what the interpreter costs over a
      bare element-wise kernel with the same traffic (`overhead_vs_fr_op`: time of (b) over time of fr_op);
  (c) program (a) COMPOSED (class Composed below): one `fr_op_device` call per instruction on full-length temporaries (two for a
      MAD: there is no fused multiply-add among the element-wise ops), the two wrapped `hipMemcpyAsync` copies of every rotated
      full-length operand timed with them, and the constants, the challenges and the periodic column expanded to full length OUTSIDE
      the timed region.  (a) and (c) are compared limb for limb before anything is timed; a mismatch ends the run with status 1.

`fr_op_device` mul over N elements in the same run is the yardstick of every row (`vs_fr_op_mul`).  The columns are seeded random
scalars, not a satisfying instance: the arithmetic does not care.  No test asserts any of these figures;
tests/test_fr_expr.py::test_against_the_composed_route holds Composed against the fused call."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOG_NS = [16, 20, 24]
LOG_STRIDE = 2
FR_MUL, FR_ADD, FR_SUB = 0, 1, 2                                   # blsgpu_fr_op


class Composed:
    """An expression program run instruction by instruction with `fr_op_device` on full-length temporaries: the route a caller had
    before blsgpu_fr_expr_eval_device.  `prepare` (untimed) expands what fr_op cannot broadcast -- constants, columns shorter than N --
    `run` (timed) enqueues the calls and the wrapped copies of every rotated full-length operand on `stream`, the torch stream the
    context has been put on with set_stream."""

    def __init__(self, ctx, stream, n_regs, consts_limbs, instrs, log_n, log_stride, device):
        import torch
        self.ctx, self.stream, self.log_n, self.log_stride, self.n, self.device = ctx, stream, log_n, log_stride, 1 << log_n, device
        self.instrs = instrs
        z = lambda: torch.empty((self.n, 4), dtype=torch.int64, device=device)
        self.regs = [z() for _ in range(n_regs)]
        self.rot = [z(), z()]                                      # the rotated copies of operand a and operand b
        self.prod = z()                                            # a MAD's product
        self.consts = [c.reshape(1, 4).expand(self.n, 4).contiguous() for c in consts_limbs]
        self.expanded = {}
        self.calls = self.copies = 0

    def prepare(self, cols, col_log_len):
        """cols: one (2^len, 4) int64 device tensor (or None) per column.  A column shorter than N is expanded here, with each of the
        rotations the program reads it at applied, so `run` sees a full-length operand and copies nothing for it."""
        import torch
        self.cols, self.ll = cols, col_log_len
        idx = torch.arange(self.n, device=self.device)
        for ins in self.instrs:
            for x in ins[2:]:
                if isinstance(x, tuple) and x[0] == "col":
                    j, rot = x[1], (x[2] if len(x) == 3 else 0)
                    ll = self.log_n if col_log_len is None else col_log_len[j]
                    if ll < self.log_n and (j, rot) not in self.expanded:
                        self.expanded[(j, rot)] = cols[j][(idx + rot * (1 << self.log_stride)) % (1 << ll)].contiguous()

    def _copy(self, dst, src):
        """a device-to-device hipMemcpyAsync of a contiguous range on the context's stream (torch's copy of contiguous tensors is one)"""
        dst.copy_(src, non_blocking=True)
        self.copies += 1

    def _rotated(self, src, rot, dst):
        """dst[i] = src[(i + rot * 2^log_stride) mod N]: two wrapped copies (one when the shift is 0 mod N)"""
        s = rot * (1 << self.log_stride) % self.n
        self._copy(dst[:self.n - s], src[s:])
        if s:
            self._copy(dst[self.n - s:], src[:s])

    def _operand(self, x, slot):
        if isinstance(x, int):
            return self.regs[x]
        if x[0] == "reg":
            return self.regs[x[1]]
        if x[0] == "const":
            return self.consts[x[1]]
        j, rot = x[1], (x[2] if len(x) == 3 else 0)
        if (j, rot) in self.expanded:
            return self.expanded[(j, rot)]
        if rot == 0:
            return self.cols[j]
        self._rotated(self.cols[j], rot, self.rot[slot])
        return self.rot[slot]

    def run(self):
        """enqueue the whole program; returns the tensor that holds the result (the last instruction's dst)"""
        import torch
        op = self.ctx.fr_op_device
        n = self.n
        self.calls = self.copies = 0
        with torch.cuda.stream(self.stream):
            for ins in self.instrs:
                name, dst = ins[0].upper(), self.regs[ins[1]]
                a = self._operand(ins[2], 0)
                if name == "MOV":
                    self._copy(dst, a)
                    continue
                b = self._operand(ins[3], 1)
                if name == "MAD":
                    op(FR_MUL, a.data_ptr(), b.data_ptr(), n, self.prod.data_ptr())
                    op(FR_ADD, dst.data_ptr(), self.prod.data_ptr(), n, dst.data_ptr())
                    self.calls += 2
                else:
                    op({"ADD": FR_ADD, "SUB": FR_SUB, "MUL": FR_MUL}[name], a.data_ptr(), b.data_ptr(), n, dst.data_ptr())
                    self.calls += 1
        return self.regs[self.instrs[-1][1]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--only", type=int, default=None, help="one log_n, e.g. 20")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bls12_381_amd as b
    from bls12_381_amd import synthetic
    ctx = b.Context(0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    ctx.set_stream(stream.cuda_stream)

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.calls):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / a.calls

    def timed(fn):
        fn()                                                       # warm-up
        ctx.synchronize()
        return [window(fn) for _ in range(a.windows)]

    gen = torch.Generator(device=dev)
    gen.manual_seed(0xE7A1)

    def scalars(n):
        """n canonical scalars made on the device: every limb below 2^62, so the value is below r; none of them zero"""
        return torch.randint(1, 1 << 62, (n, 4), dtype=torch.int64, device=dev, generator=gen)

    try:
        commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    n_cols, n_regs, consts, instrs = synthetic.plonk_quotient_program()
    plonk = ctx.fr_expr(n_cols, n_regs, consts, instrs)
    one = ctx.fr_expr(2, 1, None, [("MUL", 0, ("col", 0), ("col", 1))])
    consts_dev = torch.from_numpy(b.api._fr_limbs(consts, (-1,), "consts").view("int64")).to(dev)
    rec = {"commit": commit, "calls_per_window": a.calls, "windows": a.windows, "log_stride": LOG_STRIDE,
           "program": {"instructions": plonk.instructions, "products_per_row": plonk.products_per_row, "registers": plonk.regs, "columns": plonk.cols,
                       "full_length_columns_read": 15, "rotated_operands": 1}, "rows": {}}
    ok = True
    for log_n in LOG_NS:
        if a.only is not None and a.only != log_n:
            continue
        n = 1 << log_n
        ll = synthetic.plonk_col_log_len(log_n, LOG_STRIDE)
        cols = [scalars(1 << l) for l in ll]
        d_out = torch.empty((n, 4), dtype=torch.int64, device=dev)
        comp = Composed(ctx, stream, n_regs, [consts_dev[i] for i in range(len(consts))], instrs, log_n, LOG_STRIDE, dev)
        comp.prepare(cols, ll)
        torch.cuda.synchronize()
        ptrs = [c.data_ptr() for c in cols]
        fused = lambda: plonk.eval_device(ptrs, log_n, d_out.data_ptr(), log_stride=LOG_STRIDE, col_log_len=ll)
        fused()
        want = comp.run()
        ctx.synchronize()
        same = bool(torch.equal(d_out, want))
        ok = ok and same
        if not same:
            print("log_n=%d: the fused call and the composed route DIFFER" % log_n, flush=True)
            break
        ta = timed(fused)
        tc = timed(comp.run)
        x, y = cols[0], cols[1]
        tb = timed(lambda: one.eval_device([x.data_ptr(), y.data_ptr()], log_n, d_out.data_ptr()))
        tm = timed(lambda: ctx.fr_op_device(FR_MUL, x.data_ptr(), y.data_ptr(), n, d_out.data_ptr()))
        row = {"rows": n, "plonk_ms": min(ta), "plonk_ms_all": ta, "composed_ms": min(tc), "composed_ms_all": tc, "composed_fr_op_calls": comp.calls,
               "composed_copies": comp.copies, "speedup_vs_composed": min(tc) / min(ta), "one_mul_ms": min(tb), "one_mul_ms_all": tb, "fr_op_mul_ms": min(tm),
               "fr_op_mul_ms_all": tm, "overhead_vs_fr_op": min(tb) / min(tm), "vs_fr_op_mul": min(ta) / min(tm),
               "products_per_s": plonk.products_per_row * n / min(ta) * 1e3, "outputs_match": same}
        rec["rows"]["2^%d" % log_n] = row
        print("2^%d" % log_n, json.dumps({q: row[q] for q in ("plonk_ms", "composed_ms", "speedup_vs_composed", "one_mul_ms", "fr_op_mul_ms", "overhead_vs_fr_op", "outputs_match")}), flush=True)
        del cols, comp, d_out, want, x, y
        torch.cuda.empty_cache()
    ctx.set_stream(None)
    plonk.close()
    one.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
