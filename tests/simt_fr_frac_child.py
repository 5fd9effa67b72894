"""Builds the Fr fraction-scan emulation library (tests/simt/emu_fr_frac.cpp) and runs its entry points in a CHILD process
(tests/test_simt_fr_frac.py).

Over tests/simt_harness.py: the library is built with trapping bounds / shift checks, every buffer the kernels touch has exactly
the size the plan asks the host to reserve (a column set: the plan's table_reach scalars) and ends flush against an inaccessible page
(emu_guarded), so a kernel bug ends the process that runs it: `run(jobs)` starts `python tests/simt_fr_frac_child.py IN OUT` with the
pickled jobs, under a time limit, and turns a signal, a time-out or a non-zero exit into a pytest failure that names the job.

A job is a dict with "op" and "label"; the result list has one dict per job:
  frac   frac_op (0 grand product, 1 fraction sum), c, len, k, chal (2, 8 u32), xa / xb / da / db (packed sets of (c - 1) * pitch + k * len
         scalars as (.., 8) u32, or None), [pitch], [alias: da is the very buffer of xa], [exclusive], [shape (block, chunk)], [flags (bool)]
                                                                              -> out (k * len, 8 u32), flags (k * len u8 | None), kernels
  plan   frac_op, c, len, k, [pitch], [shape]                                 -> steps, kinds, grids, recs, block, chunk, lds, reach
`kernels` / `kinds` hold fr_scan_plan.h FrScanKernel values, the front as 100 + its mode.
Test infrastructure only: the product never imports this file."""
import ctypes

import numpy as np

import simt_fr_scan_child as scan_child
import simt_harness

ROOT, CLANG = simt_harness.ROOT, simt_harness.CLANG
LIB = simt_harness.lib_path("emu_fr_frac_test")
GRAND_PRODUCT, FRAC_SUM = 0, 1
K_AGG_REDUCE, K_AGG_SCAN, K_SCAN = scan_child.K_AGG_REDUCE, scan_child.K_AGG_SCAN, scan_child.K_SCAN
K_FRONT_SINGLE, K_FRONT_REDUCE = 100 + scan_child.K_SINGLE, 100 + scan_child.K_REDUCE
K_FRONT = 6                                                        # fr_frac_plan.h FRF_K_FRONT, what a run reports for the front
REC_WORDS = 12                                                     # fr_scan_plan.h frs_rec_words(SUM | PRODUCT)


def build():
    """build/libemu_fr_frac_test.so, rebuilt when a source is newer"""
    return simt_harness.build("emu_fr_frac_test", "emu_fr_frac.cpp")


def run(jobs, timeout=300):
    """the jobs in a fresh child process; returns their results or fails the calling test"""
    return simt_harness.run(__file__, jobs, timeout)


# ---- child side --------------------------------------------------------------------------------------------------------------
class _Child(scan_child._Child):
    def __init__(self):
        simt_harness.Child.__init__(self, LIB)                     # not the scan child's: its prototypes name the scan library's entry points
        vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        self.lib.emu_fr_frac_plan.argtypes = [ci, ci, sz, sz, sz, ci, ci, vp, vp, vp]
        self.lib.emu_fr_frac.argtypes = [ci, ci, ci, vp, vp, vp, vp, sz, vp, sz, sz, vp, vp, ci, ci, vp, vp, vp, vp, vp, vp]

    def plan(self, j):
        block, chunk = j.get("shape") or (0, 0)
        n, k = j["len"], j["k"]
        pitch = j.get("pitch", n * k)
        info = (ctypes.c_size_t * 9)()
        kinds = (ctypes.c_int * 8)()
        grids = (ctypes.c_uint * 8)()
        steps = self.lib.emu_fr_frac_plan(j["frac_op"], j["c"], n, k, pitch, block, chunk, ctypes.cast(info, ctypes.c_void_p), ctypes.cast(kinds, ctypes.c_void_p),
                                          ctypes.cast(grids, ctypes.c_void_p))
        return {"steps": steps, "kinds": [int(kinds[i]) for i in range(max(steps, 0))], "grids": [int(grids[i]) for i in range(max(steps, 0))],
                "recs": [int(info[i]) for i in range(5)], "block": int(info[5]), "chunk": int(info[6]), "lds": int(info[7]), "reach": int(info[8])}

    def frac(self, j):
        pl = self.plan(j)
        assert pl["steps"] >= 0, "the plan refused the shape"
        block, chunk = j.get("shape") or (0, 0)
        n, k, c = j["len"], j["k"], j["c"]
        total = n * k
        pitch = j.get("pitch", total)
        ptr = {}
        for name in ("xa", "xb", "da", "db"):
            x = j.get(name)
            if name == "da" and j.get("alias"):
                ptr[name] = ptr["xa"]
                continue
            if x is None:
                ptr[name] = None
                continue
            x = np.ascontiguousarray(x, dtype=np.uint32).reshape(-1, 8)
            assert total == 0 or x.shape[0] == pl["reach"], (name, x.shape, pl["reach"])
            ptr[name] = self.buf(x.size, x)[1]
        _, pchal = self.buf(16, j["chal"])
        dout, pout = self.buf(total * 8)
        if dout is not None:
            dout[:] = 0xA5A5A5A5                                   # every element must be written
        fl, pfl = self.buf(total, dtype=np.uint8) if j.get("flags") else (None, None)
        if fl is not None:
            fl[:] = 7
        scratch = [self.buf(pl["recs"][i] * (8 if i in (2, 3) else REC_WORDS))[1] for i in range(5)]
        kern, pkern = self.buf(8)
        rc = self.lib.emu_fr_frac(j["frac_op"], 1 if j.get("exclusive") else 0, c, ptr["xa"], ptr["xb"], ptr["da"], ptr["db"], pitch, pchal, n, k, pout, pfl,
                                  block, chunk, *scratch, pkern)
        assert rc >= 0, "emu_fr_frac refused the arguments"
        out = np.zeros((0, 8), dtype=np.uint32) if dout is None else dout.copy().reshape(total, 8)
        return {"out": out, "flags": None if fl is None else fl.copy(), "kernels": [int(v) for v in kern.view(np.int32)[:rc]]}


if __name__ == "__main__":
    _Child.main()
