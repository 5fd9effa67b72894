"""Builds the Fr scan emulation library (tests/simt/emu_fr_scan.cpp) and runs its entry points in a CHILD process (tests/test_simt_fr_scan.py).

Over tests/simt_harness.py: the library is built with trapping bounds / shift checks, every buffer the kernels touch has exactly the size
the plan asks the host to reserve and ends flush against an inaccessible page (emu_guarded), so a kernel bug ends the process that runs
it: `run(jobs)` starts `python tests/simt_fr_scan_child.py IN OUT` with the pickled jobs, under a time limit, and turns a signal, a
time-out or a non-zero exit into a pytest failure that names the job.

A job is a dict with "op" and "label"; the result list has one dict per job:
  scan    scan_op (0 sum, 1 product, 2 horner), data (k, len, 8 u32 Montgomery words), [points (k, 8 u32)], [exclusive], [shape (block, chunk)],
          [inplace]                                                                                      -> out (k, len, 8 u32), kernels
  invert  data (n, 8 u32), [flags (bool)], [shape], [inplace]                                            -> out (n, 8 u32), flags (n u8 | None), kernels
`kernels` is the sequence of fr_scan_plan.h FrScanKernel values the plan ran.
Test infrastructure only: the product never imports this file."""
import ctypes

import numpy as np

import simt_harness

ROOT, CLANG = simt_harness.ROOT, simt_harness.CLANG
LIB = simt_harness.lib_path("emu_fr_scan_test")
K_SINGLE, K_REDUCE, K_AGG_REDUCE, K_AGG_SCAN, K_SCAN, K_INVERT = 0, 1, 2, 3, 4, 5
SHIPPED = (256, 8)                                                 # fr_scan_plan.h FRS_BLOCK, FRS_CHUNK
REC_WORDS = {0: 12, 1: 12, 2: 20}                                  # fr_scan_plan.h frs_rec_words(op)


def build():
    """build/libemu_fr_scan_test.so, rebuilt when a source is newer"""
    return simt_harness.build("emu_fr_scan_test", "emu_fr_scan.cpp")


def run(jobs, timeout=300):
    """the jobs in a fresh child process; returns their results or fails the calling test"""
    return simt_harness.run(__file__, jobs, timeout)


# ---- child side --------------------------------------------------------------------------------------------------------------
class _Child(simt_harness.Child):
    def __init__(self):
        super().__init__(LIB)
        vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        self.lib.emu_fr_scan_recs.argtypes = [sz, sz, ci, ci, vp]
        self.lib.emu_fr_scan.argtypes = [ci, ci, vp, vp, vp, sz, sz, ci, ci, vp, vp, vp, vp, vp, vp]
        self.lib.emu_fr_invert.argtypes = [vp, vp, vp, sz, ci, ci, vp]

    def scan(self, j):
        x = np.ascontiguousarray(j["data"], dtype=np.uint32)
        k, n = x.shape[0], x.shape[1]
        block, chunk = j.get("shape") or SHIPPED
        recs = (ctypes.c_size_t * 5)()
        steps = self.lib.emu_fr_scan_recs(n, k, block, chunk, ctypes.cast(recs, ctypes.c_void_p))
        assert steps >= 0, "the plan refused the shape"
        din, pin = self.buf(k * n * 8, x)
        dout, pout = (din, pin) if j.get("inplace") else self.buf(k * n * 8)
        pts = j.get("points")
        _, ppts = self.buf(k * 8, pts) if pts is not None else (None, None)
        scratch = [self.buf(int(recs[i]) * (8 if i in (2, 3) else REC_WORDS[j["scan_op"]]))[1] for i in range(5)]
        kern, pkern = self.buf(8)
        rc = self.lib.emu_fr_scan(j["scan_op"], 1 if j.get("exclusive") else 0, pin, pout, ppts, n, k, block, chunk, *scratch, pkern)
        assert rc >= 0, "emu_fr_scan refused the arguments"
        out = np.zeros((k, n, 8), dtype=np.uint32) if dout is None else dout.copy().reshape(k, n, 8)
        return {"out": out, "kernels": [int(v) for v in kern.view(np.int32)[:rc]], "in_after": None if din is None else din.copy().reshape(k, n, 8)}

    def invert(self, j):
        x = np.ascontiguousarray(j["data"], dtype=np.uint32)
        n = x.shape[0]
        block, chunk = j.get("shape") or SHIPPED
        din, pin = self.buf(n * 8, x)
        dout, pout = (din, pin) if j.get("inplace") else self.buf(n * 8)
        fl, pfl = self.buf(n, dtype=np.uint8) if j.get("flags") else (None, None)
        if fl is not None:
            fl[:] = 7                                              # every flag must be written
        kern, pkern = self.buf(8)
        rc = self.lib.emu_fr_invert(pin, pout, pfl, n, block, chunk, pkern)
        assert rc >= 0, "emu_fr_invert refused the arguments"
        out = np.zeros((n, 8), dtype=np.uint32) if dout is None else dout.copy().reshape(n, 8)
        return {"out": out, "flags": None if fl is None else fl.copy(), "kernels": [int(v) for v in kern.view(np.int32)[:rc]]}


if __name__ == "__main__":
    _Child.main()
