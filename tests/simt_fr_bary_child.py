"""Builds the evaluation-form opening emulation library (tests/simt/emu_fr_bary.cpp) and runs it in a CHILD process (tests/test_simt_fr_bary.py).

Over tests/simt_harness.py: the library is built with trapping bounds / shift checks, every buffer the kernels touch has exactly the
size the plan asks the host to reserve and ends flush against an inaccessible page (emu_guarded), so a kernel bug ends the process that
runs it: `run(jobs)` starts `python tests/simt_fr_bary_child.py IN OUT` with the pickled jobs, under a time limit, and turns a signal, a
time-out or a non-zero exit into a pytest failure that names the job.

A job is a dict with "label" and
  evals (k, n, 8 u32 Montgomery words), points (k, 8 u32), [open (bool)], [order (0 natural, 1 bit-reversed)], [shape (block, chunk)]
and its result a dict: y (k, 8 u32), q (k, n, 8 u32) or None, kernels (the fr_bary_plan.h FrBaryKernel values the plan ran), evals_after,
points_after.  Test infrastructure only: the product never imports this file."""
import ctypes

import numpy as np

import simt_harness

ROOT, CLANG = simt_harness.ROOT, simt_harness.CLANG
LIB = simt_harness.lib_path("emu_fr_bary_test")
K_ROWS, K_TILE, K_ROW, K_QUOT = 0, 1, 2, 3
SHIPPED = (256, 8)                                                 # fr_bary_plan.h FRB_BLOCK, FRB_CHUNK
REC_WORDS, ROWREC_WORDS = 28, 12                                   # fr_bary_plan.h FRB_REC_WORDS, FRB_ROWREC_WORDS


def build():
    """build/libemu_fr_bary_test.so, rebuilt when a source is newer"""
    return simt_harness.build("emu_fr_bary_test", "emu_fr_bary.cpp")


def run(jobs, timeout=300):
    """the jobs in a fresh child process; returns their results or fails the calling test"""
    return simt_harness.run(__file__, jobs, timeout)


# ---- child side --------------------------------------------------------------------------------------------------------------
class _Child(simt_harness.Child):
    OP = "bary"

    def __init__(self):
        super().__init__(LIB)
        vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        self.lib.emu_fr_bary_recs.argtypes = [ci, sz, ci, ci, ci, vp]
        self.lib.emu_fr_bary.argtypes = [ci, vp, ci, sz, vp, ci, vp, vp, ci, ci, vp, vp, vp, vp]

    def bary(self, j):
        x = np.ascontiguousarray(j["evals"], dtype=np.uint32)
        k, n = x.shape[0], x.shape[1]
        log_n = n.bit_length() - 1
        assert n == 1 << log_n
        block, chunk = j.get("shape") or SHIPPED
        is_open = 1 if j.get("open") else 0
        recs = (ctypes.c_size_t * 2)()
        steps = self.lib.emu_fr_bary_recs(log_n, k, is_open, block, chunk, ctypes.cast(recs, ctypes.c_void_p))
        assert steps >= 0, "the plan refused the shape"
        dev, pev = self.buf(k * n * 8, x)
        dpt, ppt = self.buf(k * 8, j["points"])
        dy, py = self.buf(k * 8, fill=0xA5A5A5A5)
        dq, pq = self.buf(k * n * 8, fill=0xA5A5A5A5) if is_open else (None, None)
        _, ptw = self.buf(n * 8 if log_n and k else 0)               # the entry point reserves n scalars for the table of log_n
        _, prec = self.buf(int(recs[0]) * REC_WORDS, fill=0xA5A5A5A5)
        _, prow = self.buf(int(recs[1]) * ROWREC_WORDS, fill=0xA5A5A5A5)
        kern, pkern = self.buf(8)
        rc = self.lib.emu_fr_bary(is_open, pev, log_n, k, ppt, j.get("order", 0), py, pq, block, chunk, ptw, prec, prow, pkern)
        assert rc >= 0, "emu_fr_bary refused the arguments"
        return {"y": np.zeros((0, 8), dtype=np.uint32) if dy is None else dy.copy().reshape(k, 8),
                "q": None if not is_open else (np.zeros((0, n, 8), dtype=np.uint32) if dq is None else dq.copy().reshape(k, n, 8)),
                "kernels": [int(v) for v in kern.view(np.int32)[:rc]],
                "evals_after": None if dev is None else dev.copy().reshape(k, n, 8), "points_after": None if dpt is None else dpt.copy().reshape(k, 8)}


if __name__ == "__main__":
    _Child.main()
