"""Builds the multilinear emulation library (tests/simt/emu_fr_mle.cpp) and runs its entry points in a CHILD process (tests/test_simt_fr_mle.py).

Over tests/simt_harness.py: the library is built with trapping bounds / shift checks, every buffer the kernels touch has exactly the size
the plan asks the host to reserve -- tables of (k - 1) * pitch + 2^m scalars, records, scratch -- and ends flush against an inaccessible
page (emu_guarded), so a kernel bug ends the process that runs it: `run(jobs)` starts `python tests/simt_fr_mle_child.py IN OUT` with the
pickled jobs, under a time limit, and turns a signal, a time-out or a non-zero exit into a pytest failure that names the job.

A job is a dict with "op" and "label", optionally "shape" (block, chunk); the result list has one dict per job.  Tables are (k, 2^m, 8) u32
Montgomery words, placed `pitch` scalars apart in a buffer whose other words hold SENTINEL:
  fold   tables, r (8,), [pitch_in], [pitch_out], [inplace]          -> out: the whole output buffer (scalars, 8), in_after, kernels
  eq     point (m, 8)                                                -> out (2^m, 8), kernels
  eval   tables, point (m, 8), [pitch]                               -> out (k, 8), in_after, kernels
  round  tables, term_ptr, term_tab, coef (n_terms, 4) u64, [r_prev (8,)], [pitch]
                                                                     -> evals (D + 1, 8), after: the whole table buffer, kernels, degree
`kernels` is the sequence of fr_mle_plan.h FrMleKernel values the plan ran.
Test infrastructure only: the product never imports this file."""
import ctypes

import numpy as np

import simt_harness

ROOT, CLANG = simt_harness.ROOT, simt_harness.CLANG
LIB = simt_harness.lib_path("emu_fr_mle_test")
K_FOLD, K_EQ, K_ROUND, K_ROUND_FUSED, K_FINISH, K_COPY = 0, 1, 2, 3, 4, 5
SHIPPED = (256, 4)                                                 # fr_mle_plan.h FRM_BLOCK, FRM_CHUNK
SENTINEL = 0xA5C3F00D


def build():
    """build/libemu_fr_mle_test.so, rebuilt when a source is newer"""
    return simt_harness.build("emu_fr_mle_test", "emu_fr_mle.cpp")


def run(jobs, timeout=300):
    """the jobs in a fresh child process; returns their results or fails the calling test"""
    return simt_harness.run(__file__, jobs, timeout)


# ---- child side --------------------------------------------------------------------------------------------------------------
class _Child(simt_harness.Child):
    def __init__(self):
        super().__init__(LIB)
        vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        self.lib.emu_frm_fold.argtypes = [vp, sz, vp, sz, ci, sz, vp, ci, ci, vp]
        self.lib.emu_frm_eq.argtypes = [vp, ci, vp, ci, ci, vp]
        self.lib.emu_frm_eval_scratch.restype = sz
        self.lib.emu_frm_eval_scratch.argtypes = [ci, sz, ci, ci]
        self.lib.emu_frm_eval.argtypes = [vp, sz, ci, sz, vp, vp, vp, ci, ci, vp]
        self.lib.emu_frm_round_recs.restype = ctypes.c_long
        self.lib.emu_frm_round_recs.argtypes = [ci, sz, ci, ci, ci, ci]
        self.lib.emu_frm_prog_degree.argtypes = [sz, sz, vp, vp, vp]
        self.lib.emu_frm_round.argtypes = [vp, sz, ci, sz, sz, vp, vp, vp, vp, vp, vp, ci, ci, vp]

    def tables(self, t, pitch):
        """k tables `pitch` scalars apart in a buffer of exactly (k - 1) * pitch + n scalars, SENTINEL in between"""
        t = np.ascontiguousarray(t, dtype=np.uint32)
        k, n = t.shape[0], t.shape[1]
        if k == 0:
            return None, None
        a, p = self.buf(((k - 1) * pitch + n) * 8, fill=SENTINEL)
        for j in range(k):
            a[j * pitch * 8:(j * pitch + n) * 8] = t[j].reshape(-1)
        return a, p

    @staticmethod
    def kernels(kern, rc):
        return [int(v) for v in kern.view(np.int32)[:rc]]

    def fold(self, j):
        t = np.ascontiguousarray(j["tables"], dtype=np.uint32)
        k, n = t.shape[0], t.shape[1]
        m = n.bit_length() - 1
        block, chunk = j.get("shape") or SHIPPED
        pin = j.get("pitch_in") or n
        din, ain = self.tables(t, pin)
        if j.get("inplace"):
            pout, dout, aout = pin, din, ain
        else:
            pout = j.get("pitch_out") or n // 2
            dout, aout = self.buf(((k - 1) * pout + n // 2) * 8, fill=SENTINEL) if k else (None, None)
        _, ar = self.buf(8, j["r"])
        kern, akern = self.buf(32)
        rc = self.lib.emu_frm_fold(ain, pin, aout, pout, m, k, ar, block, chunk, akern)
        assert rc >= 0, "emu_frm_fold refused the arguments"
        return {"out": None if dout is None else dout.copy().reshape(-1, 8), "in_after": None if din is None else din.copy().reshape(-1, 8), "kernels": self.kernels(kern, rc)}

    def eq(self, j):
        pt = np.ascontiguousarray(j["point"], dtype=np.uint32).reshape(-1, 8)
        m = pt.shape[0]
        block, chunk = j.get("shape") or SHIPPED
        _, ap = self.buf(m * 8, pt)
        dout, aout = self.buf((1 << m) * 8, fill=SENTINEL)
        kern, akern = self.buf(32)
        rc = self.lib.emu_frm_eq(ap, m, aout, block, chunk, akern)
        assert rc >= 0, "emu_frm_eq refused the arguments"
        return {"out": dout.copy().reshape(-1, 8), "kernels": self.kernels(kern, rc)}

    def eval(self, j):
        t = np.ascontiguousarray(j["tables"], dtype=np.uint32)
        k, n = t.shape[0], t.shape[1]
        m = n.bit_length() - 1
        block, chunk = j.get("shape") or SHIPPED
        pitch = j.get("pitch") or n
        din, ain = self.tables(t, pitch)
        pt = np.ascontiguousarray(j["point"], dtype=np.uint32).reshape(-1, 8)
        _, ap = self.buf(m * 8, pt)
        dout, aout = self.buf(k * 8, fill=SENTINEL)
        _, ascr = self.buf(int(self.lib.emu_frm_eval_scratch(m, k, block, chunk)) * 8, fill=SENTINEL)
        kern, akern = self.buf(32)
        rc = self.lib.emu_frm_eval(ain, pitch, m, k, ap, aout, ascr, block, chunk, akern)
        assert rc >= 0, "emu_frm_eval refused the arguments"
        return {"out": None if dout is None else dout.copy().reshape(-1, 8), "in_after": None if din is None else din.copy().reshape(-1, 8), "kernels": self.kernels(kern, rc)}

    def round(self, j):
        t = np.ascontiguousarray(j["tables"], dtype=np.uint32)
        k, n = t.shape[0], t.shape[1]
        m = n.bit_length() - 1
        block, chunk = j.get("shape") or SHIPPED
        pitch = j.get("pitch") or n
        din, ain = self.tables(t, pitch)
        tp = np.ascontiguousarray(j["term_ptr"], dtype=np.uint32)
        tt = np.ascontiguousarray(j["term_tab"], dtype=np.uint8)
        cf = np.ascontiguousarray(j["coef"], dtype=np.uint64).reshape(-1, 4)
        nt = tp.shape[0] - 1
        _, atp = self.buf(nt + 1, tp)
        _, att = self.buf(tt.shape[0], tt, dtype=np.uint8)
        _, acf = self.buf(nt * 4, cf, dtype=np.uint64)
        deg = self.lib.emu_frm_prog_degree(k, nt, atp, att, acf)
        assert deg >= 1, "the program was refused"
        fused = j.get("r_prev") is not None
        _, ar = self.buf(8, j["r_prev"]) if fused else (None, None)
        recs = int(self.lib.emu_frm_round_recs(m, k, deg, 1 if fused else 0, block, chunk))
        assert recs >= 0, "the plan refused the shape"
        _, arec = self.buf(recs * (deg + 1) * 8, fill=SENTINEL)
        dev, aev = self.buf((deg + 1) * 8, fill=SENTINEL)
        kern, akern = self.buf(32)
        rc = self.lib.emu_frm_round(ain, pitch, m, k, nt, atp, att, acf, ar, aev, arec, block, chunk, akern)
        assert rc >= 0, "emu_frm_round refused the arguments (%d)" % rc
        return {"evals": dev.copy().reshape(-1, 8), "after": din.copy().reshape(-1, 8), "kernels": self.kernels(kern, rc), "degree": deg}


if __name__ == "__main__":
    _Child.main()
