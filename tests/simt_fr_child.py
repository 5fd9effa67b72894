"""Builds the Fr transform emulation library (tests/simt/emu_fr.cpp) and runs its entry points in a CHILD process (tests/test_simt_fr.py).

Over tests/simt_harness.py: the library is built with trapping bounds / shift checks, every buffer the kernels touch ends flush against an
inaccessible page (emu_guarded), so a kernel bug ends the process that runs it: `run(jobs)` starts `python tests/simt_fr_child.py IN OUT`
with the pickled jobs, under a time limit, and turns a signal, a time-out or a non-zero exit into a pytest failure that names the job.

A job is a dict with "op" and "label"; the result list has one dict per job:
  many    data (k, n, 8 u32 Montgomery words), inverse, [coset (8 u32)], [cols (tlog, dmax, block)], [threads]  -> out (k, n, 8 u32), kernels
  single  data (n, 8 u32), inverse, [threads]                                                                     -> out (n, 8 u32)
`kernels` is the sequence of fr_plan.h FrKernel values the plan ran (0 cols, 1 stage2, 2 stage1, 3 tile).
Test infrastructure only: the product never imports this file."""
import ctypes

import numpy as np

import simt_harness

ROOT, CLANG = simt_harness.ROOT, simt_harness.CLANG
LIB = simt_harness.lib_path("emu_fr_test")
K_COLS, K_STAGE2, K_STAGE1, K_TILE = 0, 1, 2, 3


def build():
    """build/libemu_fr_test.so, rebuilt when a source is newer"""
    return simt_harness.build("emu_fr_test", "emu_fr.cpp")


def run(jobs, timeout=300):
    """the jobs in a fresh child process; returns their results or fails the calling test"""
    return simt_harness.run(__file__, jobs, timeout)


# ---- child side --------------------------------------------------------------------------------------------------------------
class _Child(simt_harness.Child):
    def __init__(self):
        super().__init__(LIB)
        vp = ctypes.c_void_p
        self.lib.emu_fr_ntt_many.argtypes = [vp, vp, vp, vp, vp, ctypes.c_int, ctypes.c_size_t, ctypes.c_int, vp] + [ctypes.c_int] * 5 + [vp]
        self.lib.emu_fr_tile_single.argtypes = [vp, vp, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int]

    def many(self, j):
        x = np.ascontiguousarray(j["data"], dtype=np.uint32)
        k, n = x.shape[0], x.shape[1]
        log_n = n.bit_length() - 1
        data, pdata = self.buf(k * n * 8, x)
        _, ptmp = self.buf(k * n * 8)
        _, ptw = self.buf((n - 1) * 8)
        _, pninv = self.buf(8)
        coset = j.get("coset")
        pcs = pcoset = None
        if coset is not None:
            _, pcs = self.buf(n * 8)
            _, pcoset = self.buf(8, coset)
        cols = j.get("cols")
        kern, pkern = self.buf(40)
        rc = self.lib.emu_fr_ntt_many(pdata, ptmp, ptw, pcs, pninv, log_n, k, 1 if j.get("inverse") else 0, pcoset, 1 if cols else 0,
                                      *(cols or (0, 0, 0)), 1 if j.get("threads") else 0, pkern)
        assert rc >= 0, "emu_fr_ntt_many refused the arguments"
        return {"out": data.copy().reshape(k, n, 8), "kernels": [int(v) for v in kern.view(np.int32)[:rc]]}

    def single(self, j):
        x = np.ascontiguousarray(j["data"], dtype=np.uint32)
        n = x.shape[0]
        _, px = self.buf(n * 8, x)
        y, py = self.buf(n * 8)
        _, ptw = self.buf((n - 1) * 8)
        _, pninv = self.buf(8)
        rc = self.lib.emu_fr_tile_single(px, py, ptw, pninv, n.bit_length() - 1, 1 if j.get("inverse") else 0, 1 if j.get("threads") else 0)
        assert rc > 0
        return {"out": y.copy().reshape(n, 8)}


if __name__ == "__main__":
    _Child.main()
