"""Builds the segmented point-sum emulation library (tests/simt/emu_gsum.cpp) and runs its entry points in a CHILD process
(tests/test_simt_gsum.py).

Over tests/simt_harness.py: the library is built with trapping bounds / shift checks, every buffer the kernels touch has exactly the
size the caller owns or the plan asks the host to reserve and ends flush against an inaccessible page (emu_guarded), so a kernel bug --
an index >= npoints that is dereferenced after all -- ends the process that runs it: `run(jobs)` starts
`python tests/simt_gsum_child.py IN OUT` with the pickled jobs, under a time limit, and turns a signal, a time-out or a non-zero exit
into a pytest failure that names the job.

A job is a dict with "op" and "label"; the result list has one dict per job:
  sum    group, xy (npoints, 12 | 24) u64, inf (npoints,) u8, idx (total,) u32 | None, offsets (nseg + 1,) u64, [total], [shape (block, terms)],
         [fault]                                                              -> rc, out (nseg, 18 | 36) u64, status
  plan   group, nseg, total, [shape]                                          -> ok, part_bytes, meta_bytes, chunk, nchunks, chunks_grid, combine_grid, lds, block, terms
Test infrastructure only: the product never imports this file."""
import ctypes

import numpy as np

import simt_harness

LIB = simt_harness.lib_path("emu_gsum_test")
FAULTS = (1, 2, 3, 4)                                              # gsum.hip.h GSUM_FAULT
STATUS_BAD = 16                                                    # gsum_plan.h GSUM_STATUS_BAD


def build():
    """build/libemu_gsum_test.so, rebuilt when a source is newer"""
    return simt_harness.build("emu_gsum_test", "emu_gsum.cpp")


def build_fault(n):
    """the same library with seeded fault n (-DGSUM_FAULT=n)"""
    return simt_harness.build("emu_gsum_fault%d_test" % n, "emu_gsum.cpp", defines=("GSUM_FAULT=%d" % n,))


def fault_lib_path(n):
    return simt_harness.lib_path("emu_gsum_fault%d_test" % n)


def run(jobs, timeout=300):
    """the jobs in a fresh child process; returns their results or fails the calling test"""
    return simt_harness.run(__file__, jobs, timeout)


# ---- child side --------------------------------------------------------------------------------------------------------------
class _Child(simt_harness.Child):
    def __init__(self):
        simt_harness.Child.__init__(self, LIB)
        self.libs = {0: self.lib}

    def _lib(self, fault):
        if fault not in self.libs:
            lib = ctypes.CDLL(fault_lib_path(fault))
            lib.emu_guarded.restype = ctypes.c_void_p
            lib.emu_guarded.argtypes = [ctypes.c_size_t]
            self.libs[fault] = lib
        lib = self.libs[fault]
        vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        lib.emu_gsum_plan.argtypes = [ci, sz, sz, ci, ci, vp]
        lib.emu_gsum.argtypes = [ci, vp, vp, sz, vp, vp, sz, sz, ci, ci, vp, vp, vp, vp]
        return lib

    def plan(self, j):
        block, terms = j.get("shape") or (0, 0)
        info = (ctypes.c_size_t * 9)()
        ok = self._lib(j.get("fault", 0)).emu_gsum_plan(j["group"], j["nseg"], j["total"], block, terms, ctypes.cast(info, ctypes.c_void_p))
        names = ("part_bytes", "meta_bytes", "chunk", "nchunks", "chunks_grid", "combine_grid", "lds", "block", "terms")
        return dict({"ok": ok}, **{n: int(info[i]) for i, n in enumerate(names)})

    def sum(self, j):
        lib = self._lib(j.get("fault", 0))
        g = j["group"]
        off = np.ascontiguousarray(j["offsets"], dtype=np.uint64).reshape(-1)
        nseg = off.shape[0] - 1
        total = int(j.get("total", off[-1]))
        pl = self.plan({"group": g, "nseg": nseg, "total": total, "shape": j.get("shape"), "fault": j.get("fault", 0)})
        assert pl["ok"], "the plan refused the shape"
        block, terms = j.get("shape") or (0, 0)
        xy = np.ascontiguousarray(j["xy"], dtype=np.uint64).reshape(-1, 12 * g)
        npoints = xy.shape[0]
        _, pxy = self.buf(xy.size, xy, dtype=np.uint64)
        _, pinf = self.buf(npoints, j["inf"], dtype=np.uint8)
        pidx = None if j.get("idx") is None else self.buf(len(j["idx"]), j["idx"])[1]
        _, poff = self.buf(nseg + 1, off, dtype=np.uint64)
        dout, pout = self.buf(nseg * 18 * g, dtype=np.uint64, fill=0xA5A5A5A5A5A5A5A5)      # every segment must be written
        _, ppart = self.buf(pl["part_bytes"] // 4, fill=0xDEADBEEF)
        _, pmeta = self.buf(pl["meta_bytes"] // 4, fill=0xDEADBEEF)
        st, pst = self.buf(1)
        rc = lib.emu_gsum(g, pxy, pinf, npoints, pidx, poff, nseg, total, block, terms, pout, ppart, pmeta, pst)
        out = np.zeros((0, 18 * g), dtype=np.uint64) if dout is None else dout.copy().reshape(nseg, 18 * g)
        return {"rc": rc, "out": out, "status": int(st[0])}


if __name__ == "__main__":
    _Child.main()
