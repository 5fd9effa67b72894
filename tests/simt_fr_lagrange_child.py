"""Builds the Lagrange-coefficient emulation library (tests/simt/emu_fr_lagrange.cpp) and runs its entry points in a CHILD process
(tests/test_simt_fr_lagrange.py).

Over tests/simt_harness.py: the library is built with trapping bounds / shift checks, every buffer the kernel touches has exactly the
size the caller owns or the plan asks the host to reserve and ends flush against an inaccessible page (emu_guarded), so a kernel bug -- a
segment that breaks the offsets contract and is used as an address after all -- ends the process that runs it: `run(jobs)` starts
`python tests/simt_fr_lagrange_child.py IN OUT` with the pickled jobs, under a time limit, and turns a signal, a time-out or a non-zero
exit into a pytest failure that names the job.

A job is a dict with "op" and "label"; the result list has one dict per job:
  lagrange  nodes (total, 4) u64, offsets (nseg + 1,) u32, points (nseg, 4) | None, values (total, 4) | None, want_lambda, want_y, [want_flags],
            [total], [which], [shape (block, team, tile, r)], [fault]          -> rc, lam, y, flags (untouched entries keep FILL / FILL8), status
  plan      nseg, total, want_lambda, [which], [shape]                         -> ok, shape, block, team, tile, r, teams, grid, lds, pre_bytes, work_bytes
Test infrastructure only: the product never imports this file."""
import ctypes

import numpy as np

import simt_harness

LIB = simt_harness.lib_path("emu_fr_lagrange_test")
FAULTS = (1, 2, 3, 4, 5)                                           # fr_lagrange.hip.h FLG_FAULT
STATUS_BAD = 32                                                    # fr_lagrange_plan.h FLG_STATUS_BAD
FILL = 0xA5A5A5A5A5A5A5A5
FILL8 = 0xA5


def build():
    """build/libemu_fr_lagrange_test.so, rebuilt when a source is newer"""
    return simt_harness.build("emu_fr_lagrange_test", "emu_fr_lagrange.cpp")


def build_fault(n):
    """the same library with seeded fault n (-DFLG_FAULT=n)"""
    return simt_harness.build("emu_fr_lagrange_fault%d_test" % n, "emu_fr_lagrange.cpp", defines=("FLG_FAULT=%d" % n,))


def fault_lib_path(n):
    return simt_harness.lib_path("emu_fr_lagrange_fault%d_test" % n)


def run(jobs, timeout=600):
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
        lib.emu_flg_plan.argtypes = [sz, sz, ci, ci, ci, ci, ci, ci, vp]
        lib.emu_flg.argtypes = [vp, vp, sz, sz, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp, vp, vp]
        return lib

    def plan(self, j):
        block, team, tile, r = j.get("shape") or (0, 0, 0, 0)
        info = (ctypes.c_size_t * 10)()
        ok = self._lib(j.get("fault", 0)).emu_flg_plan(j["nseg"], j["total"], 1 if j.get("want_lambda", True) else 0, j.get("which", 0), block, team, tile, r,
                                                       ctypes.cast(info, ctypes.c_void_p))
        names = ("shape", "block", "team", "tile", "r", "teams", "grid", "lds", "pre_bytes", "work_bytes")
        return dict({"ok": ok}, **{n: int(info[i]) for i, n in enumerate(names)})

    def lagrange(self, j):
        lib = self._lib(j.get("fault", 0))
        off = np.ascontiguousarray(j["offsets"], dtype=np.uint32).reshape(-1)
        nseg = off.shape[0] - 1
        nodes = np.ascontiguousarray(j["nodes"], dtype=np.uint64).reshape(-1, 4)
        total = int(j.get("total", nodes.shape[0]))
        want_lambda, want_y, want_flags = j.get("want_lambda", True), j.get("want_y", False), j.get("want_flags", True)
        pl = self.plan({"nseg": nseg, "total": total, "want_lambda": want_lambda, "which": j.get("which", 0), "shape": j.get("shape"), "fault": j.get("fault", 0)})
        assert pl["ok"], "the plan refused the shape"
        block, team, tile, r = j.get("shape") or (0, 0, 0, 0)
        _, pn = self.buf(nodes.size, nodes, dtype=np.uint64)
        _, poff = self.buf(nseg + 1, off)
        ppts = None if j.get("points") is None else self.buf(nseg * 4, j["points"], dtype=np.uint64)[1]
        pval = None if j.get("values") is None else self.buf(total * 4, j["values"], dtype=np.uint64)[1]
        dlam, plam = self.buf(total * 4, dtype=np.uint64, fill=FILL) if want_lambda else (None, None)
        dy, py = self.buf(nseg * 4, dtype=np.uint64, fill=FILL) if want_y else (None, None)
        dfl, pfl = self.buf(nseg, dtype=np.uint8, fill=FILL8) if want_flags else (None, None)
        _, pwork = self.buf(pl["work_bytes"] // 4, fill=0xDEADBEEF)
        _, ppre = self.buf(pl["pre_bytes"] // 4, fill=0xDEADBEEF)
        st, pst = self.buf(1)
        rc = lib.emu_flg(pn, poff, nseg, total, ppts, pval, plam, py, pfl, j.get("which", 0), block, team, tile, r, pwork, ppre, pst)
        cp = lambda d, shape: None if d is None else d.copy().reshape(shape)
        return {"rc": rc, "lam": cp(dlam, (total, 4)), "y": cp(dy, (nseg, 4)), "flags": cp(dfl, (nseg,)), "status": int(st[0]), "plan": pl}


if __name__ == "__main__":
    _Child.main()
