"""Builds the emulation library of KZG cell recovery (tests/simt/emu_kzg_recover.cpp) and runs its entry points in a CHILD process
(tests/test_simt_kzg_recover.py).

Over tests/simt_harness.py: the library is built with trapping bounds / shift checks, every buffer the kernels touch has exactly the size
the plan asks the host to reserve and ends flush against an inaccessible page (emu_guarded), so a kernel bug ends the process that runs
it: `run(jobs)` starts `python tests/simt_kzg_recover_child.py IN OUT` with the pickled jobs, under a time limit, and turns a signal, a
time-out or a non-zero exit into a pytest failure that names the job.

A job is a dict with "op" and "label":
  recover  log_n, log_l, order, col, offsets, [m], cells (m x l ints), [tile], [root_tile], [fault]
           -> eff, mis, slot, status, sticky, rootd, rootc, zd, zc, ez, scaled, q, upper, polys, ok: every stage's output, the kernels fed
              with the outputs of the kernels before them and the transforms / the inversion between them done here in Python integers
  finish   log_n, log_l, q (count x 2n ints), status, [fault]   -> upper, polys, ok: the check and the finish on their own
  plan     log_n, log_l, count, m, [coef_scratch], [tile]       -> the numbers of emu_kzgr_plan
Test infrastructure only: the product never imports this file."""
import ctypes

import numpy as np

import kzg_ref as k
import kzg_recover_ref as rr
import simt_harness
from oracle import bls12_381_ref as o

LIB = simt_harness.lib_path("emu_kzg_recover_test")
FAULTS = (1, 2, 3)                                                 # kzg_recover.hip.h KZG_REC_FAULT
FILL = 0xA5A5A5A5A5A5A5A5
PLAN_NAMES = ("ok", "bytes", "eff", "mis", "slot", "status", "upper", "rootd", "rootc", "zd", "zc", "work", "coef", "scalars", "tables", "offsets_grid", "slots_grid", "roots_grid",
              "vanish_per_poly", "vanish_grid", "scatter_block", "scatter_grid", "scale_grid", "finish_per_poly", "finish_grid")


def build():
    """build/libemu_kzg_recover_test.so, rebuilt when a source is newer"""
    return simt_harness.build("emu_kzg_recover_test", "emu_kzg_recover.cpp")


def build_fault(n):
    """the same library with seeded fault n (-DKZG_REC_FAULT=n)"""
    return simt_harness.build("emu_kzg_recover_fault%d_test" % n, "emu_kzg_recover.cpp", defines=("KZG_REC_FAULT=%d" % n,))


def fault_lib_path(n):
    return simt_harness.lib_path("emu_kzg_recover_fault%d_test" % n)


def run(jobs, timeout=300):
    """the jobs in a fresh child process; returns their results or fails the calling test"""
    return simt_harness.run(__file__, jobs, timeout)


def _fr(vals):
    return np.array([o.fr_to_mont_limbs(int(v) % k.R) for v in vals], dtype=np.uint64).reshape(-1, 4)


def _ints(limbs):
    return [o.fr_from_mont_limbs([int(w) for w in row]) for row in np.asarray(limbs).reshape(-1, 4)]


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
        lib.emu_kzgr_plan.argtypes = [ci, ci, sz, sz, ci, ci, vp]
        lib.emu_kzgr_offsets.argtypes = [vp, sz, sz, ci, ci, vp, vp]
        lib.emu_kzgr_slots.argtypes = [vp, vp, vp, sz, sz, ci, ci, vp, vp, vp, vp]
        lib.emu_kzgr_roots.argtypes = [vp, vp, ci, ci]
        lib.emu_kzgr_vanish.argtypes = [vp, vp, vp, vp, sz, ci, ci, ci, ci, vp, vp]
        lib.emu_kzgr_scatter.argtypes = [vp, vp, vp, sz, sz, ci, ci, ci, ci, vp]
        lib.emu_kzgr_scale.argtypes = [vp, vp, sz, ci, ci]
        lib.emu_kzgr_check.argtypes = [vp, sz, ci, ci, vp]
        lib.emu_kzgr_finish.argtypes = [vp, vp, vp, sz, ci, ci, vp, vp]
        return lib

    def plan(self, j):
        info = (ctypes.c_size_t * len(PLAN_NAMES))()
        self._lib(j.get("fault", 0)).emu_kzgr_plan(j["log_n"], j["log_l"], j["count"], j["m"], j.get("coef_scratch", 0), j.get("tile", 0), ctypes.cast(info, ctypes.c_void_p))
        return {n: int(info[i]) for i, n in enumerate(PLAN_NAMES)}

    def _finish(self, lib, q, pq, status, pstatus, upper, pupper, count, log_n, log_l, res):
        n = 1 << log_n
        assert lib.emu_kzgr_check(pq, count, log_n, log_l, pupper) == 0
        res["upper"] = [int(x) for x in upper]
        out, pout = self.buf(count * n * 4, dtype=np.uint64, fill=FILL)
        ok, pok = self.buf(count, dtype=np.uint8, fill=0xA5)
        assert lib.emu_kzgr_finish(pq, pstatus, pupper, count, log_n, log_l, pout, pok) == 0
        res["polys"] = np.array(_ints(out), dtype=object).reshape(count, n).tolist()
        res["ok"] = [int(x) for x in ok]

    def finish(self, j):
        lib = self._lib(j.get("fault", 0))
        log_n, log_l, count = j["log_n"], j["log_l"], len(j["q"])
        q, pq = self.buf(count * (2 << log_n) * 4, _fr([x for row in j["q"] for x in row]), dtype=np.uint64)
        status, pstatus = self.buf(count, np.array(j["status"], dtype=np.uint32))
        upper, pupper = self.buf(count, fill=0)
        res = {}
        self._finish(lib, q, pq, status, pstatus, upper, pupper, count, log_n, log_l, res)
        return res

    def recover(self, j):
        lib = self._lib(j.get("fault", 0))
        log_n, log_l, order, tile = j["log_n"], j["log_l"], j["order"], j.get("tile", 0)
        n, l, c2 = 1 << log_n, 1 << log_l, 2 << (log_n - log_l)
        count = len(j["offsets"]) - 1
        m = j.get("m", len(j["col"]))
        pl = self.plan(dict(j, count=count, m=m))
        assert pl["ok"]
        res = {}
        off, poff = self.buf(count + 1, np.array(j["offsets"], dtype=np.uint32))
        col, pcol = self.buf(m, np.array(j["col"], dtype=np.uint32))
        cells, pcells = self.buf(m * l * 4, _fr([x for c in j["cells"] for x in c]) if m else None, dtype=np.uint64)
        eff, peff = self.buf(count + 1, fill=0xDEADBEEF)
        mis, pmis = self.buf(count + 1, dtype=np.uint8, fill=0xA5)
        assert lib.emu_kzgr_offsets(poff, count, m, log_n, log_l, peff, pmis) == 0
        res["eff"], res["mis"] = [int(x) for x in eff], [int(x) for x in mis]
        slot, pslot = self.buf(count * c2, dtype=np.int32, fill=0x5A5A5A5A)
        status, pstatus = self.buf(count, fill=0xDEADBEEF)
        upper, pupper = self.buf(count, fill=0xDEADBEEF)
        sticky, psticky = self.buf(4, fill=0)
        assert lib.emu_kzgr_slots(peff, pmis, pcol, count, m, log_n, log_l, pslot, pstatus, pupper, psticky) == 0
        res["slot"] = np.array(slot).reshape(count, c2).tolist()
        res["status"], res["sticky"] = [int(x) for x in status], int(sticky[0])
        assert all(int(x) == 0 for x in upper), "k_kzg_rec_slots did not clear the upper words"
        rd, prd = self.buf(c2 * 4, dtype=np.uint64, fill=FILL)
        rc, prc = self.buf(c2 * 4, dtype=np.uint64, fill=FILL)
        assert lib.emu_kzgr_roots(prd, prc, log_n, log_l) == 0
        res["rootd"], res["rootc"] = _ints(rd), _ints(rc)
        zd, pzd = self.buf(count * c2 * 4, dtype=np.uint64, fill=FILL)
        zc, pzc = self.buf(count * c2 * 4, dtype=np.uint64, fill=FILL)
        assert lib.emu_kzgr_vanish(pslot, pstatus, prd, prc, count, log_n, log_l, order, j.get("root_tile", 0), pzd, pzc) == 0
        res["zd"] = np.array(_ints(zd), dtype=object).reshape(count, c2).tolist()
        res["zc"] = np.array(_ints(zc), dtype=object).reshape(count, c2).tolist()
        work, pwork = self.buf(count * 2 * n * 4, dtype=np.uint64, fill=FILL)
        assert lib.emu_kzgr_scatter(pslot, pcells, pzd, count, m, log_n, log_l, order, tile, pwork) == 0
        res["ez"] = np.array(_ints(work), dtype=object).reshape(count, 2 * n).tolist()
        # the batch inversion and the first two transforms
        zc[:] = _fr([pow(x, k.R - 2, k.R) for row in res["zc"] for x in row]).reshape(-1)
        fwd = [rr.coset_ntt(o.fr_ntt(list(row), inverse=True), False) for row in res["ez"]]
        work[:] = _fr([x for row in fwd for x in row]).reshape(-1)
        assert lib.emu_kzgr_scale(pwork, pzc, count, log_n, log_l) == 0
        res["unscaled"] = fwd
        res["scaled"] = np.array(_ints(work), dtype=object).reshape(count, 2 * n).tolist()
        res["q"] = [rr.coset_ntt(row, True) for row in res["scaled"]]
        work[:] = _fr([x for row in res["q"] for x in row]).reshape(-1)
        self._finish(lib, work, pwork, status, pstatus, upper, pupper, count, log_n, log_l, res)
        return res


if __name__ == "__main__":
    _Child.main()
