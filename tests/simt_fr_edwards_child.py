"""Builds the twisted Edwards emulation library (tests/simt/emu_fr_edwards.cpp) and runs its entry points in a CHILD process
(tests/test_simt_fr_edwards.py).

Over tests/simt_harness.py: the library is built with trapping bounds / shift checks, every buffer the kernels touch has exactly the
size the caller owns or the plan asks the host to reserve and ends flush against an inaccessible page (emu_guarded), so a kernel bug
ends the process that runs it: `run(jobs)` starts `python tests/simt_fr_edwards_child.py IN OUT` with the pickled jobs, under a time
limit, and turns a signal, a time-out or a non-zero exit into a pytest failure that names the job.

A job is a dict with "op", "label" and "curve" = (a, d) as integers; the result list has one dict per job:
  check      xy (n, 2, 4) u64                                                        -> rc, ok
  normalize  xyz (n, 3, 4) u64, [block]                                              -> rc, xy, ok
  mul        xy, scalars (n, 32) u8, bits, [block], [fault]                          -> rc, out (n, 3, 4), status
  mul_plan   n, bits, [block]                                                        -> ok, W, doublings, grid, block, lds
  table      xy, bits, window                                                        -> rc, flag, table (entries, 3, 4) u64, W, H
  msm        xy (the bases), bits, window, offsets, base_first | None, scalars, [total], [shape (block, terms)], [fault]
                                                                                     -> rc, out (k, 3, 4), status, flag
  msm_plan   k, total, [shape]                                                       -> ok, off_bytes, part_bytes, meta_bytes, chunk, nchunks, ...
Test infrastructure only: the product never imports this file."""
import ctypes

import numpy as np

import fr_edwards_ref as ref
import simt_harness

LIB = simt_harness.lib_path("emu_fr_edwards_test")
FAULTS = (1, 2, 3, 4)                                              # fr_edwards.hip.h FR_EDWARDS_FAULT
STATUS_SCALAR, STATUS_BAD = 1, 1 << 8                              # fr_edwards_plan.h FRED_STATUS_*


def build():
    """build/libemu_fr_edwards_test.so, rebuilt when a source is newer"""
    return simt_harness.build("emu_fr_edwards_test", "emu_fr_edwards.cpp")


def build_fault(n):
    """the same library with wrong-result variant n (-DFR_EDWARDS_FAULT=n)"""
    return simt_harness.build("emu_fr_edwards_fault%d_test" % n, "emu_fr_edwards.cpp", defines=("FR_EDWARDS_FAULT=%d" % n,))


def fault_lib_path(n):
    return simt_harness.lib_path("emu_fr_edwards_fault%d_test" % n)


def run(jobs, timeout=600):
    """the jobs in a fresh child process; returns their results or fails the calling test"""
    return simt_harness.run(__file__, jobs, timeout)


# ---- child side --------------------------------------------------------------------------------------------------------------
class _Child(simt_harness.Child):
    def __init__(self):
        simt_harness.Child.__init__(self, LIB)
        self.libs = {0: self.lib}
        self.tables = {}

    def _lib(self, fault):
        if fault not in self.libs:
            lib = ctypes.CDLL(fault_lib_path(fault))
            lib.emu_guarded.restype = ctypes.c_void_p
            lib.emu_guarded.argtypes = [ctypes.c_size_t]
            self.libs[fault] = lib
        lib = self.libs[fault]
        vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        lib.emu_fred_check.argtypes = [vp, vp, vp, sz, vp]
        lib.emu_fred_normalize.argtypes = [vp, vp, vp, sz, vp, vp, ci]
        lib.emu_fred_mul_plan.argtypes = [sz, ci, ci, vp]
        lib.emu_fred_mul.argtypes = [vp, vp, vp, vp, ci, sz, vp, vp, ci]
        lib.emu_fred_table_plan.argtypes = [sz, ci, ci, vp]
        lib.emu_fred_table.argtypes = [vp, vp, vp, sz, ci, ci, vp, vp]
        lib.emu_fred_msm_plan.argtypes = [sz, sz, ci, ci, vp]
        lib.emu_fred_msm.argtypes = [vp, vp, vp, sz, ci, ci, vp, vp, vp, sz, sz, ci, ci, vp, vp, vp, vp, vp]
        return lib

    def _curve(self, j):
        a, d = j["curve"]
        return self.buf(4, ref.limbs([a]), dtype=np.uint64)[1], self.buf(4, ref.limbs([d]), dtype=np.uint64)[1]

    def _u64(self, arr):
        a = np.ascontiguousarray(arr, dtype=np.uint64)
        return self.buf(a.size, a, dtype=np.uint64)[1] if a.size else None

    def check(self, j):
        pa, pd = self._curve(j)
        xy = np.ascontiguousarray(j["xy"], dtype=np.uint64).reshape(-1, 2, 4)
        ok, pok = self.buf(xy.shape[0], dtype=np.uint8, fill=0xA5)
        rc = self.lib.emu_fred_check(pa, pd, self._u64(xy), xy.shape[0], pok)
        return {"rc": rc, "ok": ok.copy()}

    def normalize(self, j):
        pa, pd = self._curve(j)
        xyz = np.ascontiguousarray(j["xyz"], dtype=np.uint64).reshape(-1, 3, 4)
        n = xyz.shape[0]
        out, pout = self.buf(n * 8, dtype=np.uint64, fill=0xA5A5A5A5A5A5A5A5)
        ok, pok = self.buf(n, dtype=np.uint8, fill=0xA5)
        rc = self.lib.emu_fred_normalize(pa, pd, self._u64(xyz), n, pout, pok, j.get("block", 0))
        return {"rc": rc, "xy": out.copy().reshape(n, 2, 4), "ok": ok.copy()}

    def mul_plan(self, j):
        info = (ctypes.c_size_t * 5)()
        ok = self.lib.emu_fred_mul_plan(j["n"], j["bits"], j.get("block", 0), ctypes.cast(info, ctypes.c_void_p))
        return dict({"ok": ok}, **{n: int(info[i]) for i, n in enumerate(("W", "doublings", "grid", "block", "lds"))})

    def mul(self, j):
        lib = self._lib(j.get("fault", 0))
        pa, pd = self._curve(j)
        xy = np.ascontiguousarray(j["xy"], dtype=np.uint64).reshape(-1, 2, 4)
        n = xy.shape[0]
        sc = np.ascontiguousarray(j["scalars"], dtype=np.uint8).reshape(n, 32)
        out, pout = self.buf(n * 12, dtype=np.uint64, fill=0xA5A5A5A5A5A5A5A5)
        st, pst = self.buf(1)
        rc = lib.emu_fred_mul(pa, pd, self._u64(xy), self._u64(sc.view(np.uint64)), j["bits"], n, pout, pst, j.get("block", 0))
        return {"rc": rc, "out": out.copy().reshape(n, 3, 4), "status": int(st[0])}

    def _table(self, j, fault=0):
        """the table of the job's bases, built once per (bases, bits, window) by the REAL kernels (no variant touches the build)"""
        xy = np.ascontiguousarray(j["xy"], dtype=np.uint64).reshape(-1, 2, 4)
        key = (xy.tobytes(), j["bits"], j["window"], j["curve"])
        if key not in self.tables:
            info = (ctypes.c_size_t * 4)()
            assert self.lib.emu_fred_table_plan(xy.shape[0], j["bits"], j["window"], ctypes.cast(info, ctypes.c_void_p)), "the table plan refused"
            pa, pd = self._curve(j)
            tab, ptab = self.buf(int(info[3]) // 8, dtype=np.uint64, fill=0xA5A5A5A5A5A5A5A5)
            fl, pfl = self.buf(1)
            rc = self.lib.emu_fred_table(pa, pd, self._u64(xy), xy.shape[0], j["bits"], j["window"], ptab, pfl)
            self.tables[key] = (rc, int(fl[0]), tab, ptab, int(info[0]), int(info[1]))
        return self.tables[key]

    def table(self, j):
        rc, flag, tab, _, W, H = self._table(j)
        return {"rc": rc, "flag": flag, "table": tab.copy().reshape(-1, 3, 4), "W": W, "H": H}

    def msm_plan(self, j):
        block, terms = j.get("shape") or (0, 0)
        info = (ctypes.c_size_t * 10)()
        ok = self._lib(j.get("fault", 0)).emu_fred_msm_plan(j["k"], j["total"], block, terms, ctypes.cast(info, ctypes.c_void_p))
        names = ("off_bytes", "part_bytes", "meta_bytes", "chunk", "nchunks", "chunks_grid", "combine_grid", "lds", "block", "terms")
        return dict({"ok": ok}, **{n: int(info[i]) for i, n in enumerate(names)})

    def msm(self, j):
        lib = self._lib(j.get("fault", 0))
        rc_t, flag, _, ptab, _, _ = self._table(j)
        assert rc_t == 0
        pa, pd = self._curve(j)
        off = np.ascontiguousarray(j["offsets"], dtype=np.uint32).reshape(-1)
        k = off.shape[0] - 1
        total = int(j.get("total", off[-1]))
        pl = self.msm_plan({"k": k, "total": total, "shape": j.get("shape"), "fault": j.get("fault", 0)})
        assert pl["ok"], "the plan refused the shape"
        block, terms = j.get("shape") or (0, 0)
        nbases = np.asarray(j["xy"]).reshape(-1, 2, 4).shape[0]
        pbf = None if j.get("base_first") is None else self.buf(k, np.asarray(j["base_first"], dtype=np.uint32))[1]
        sc = np.ascontiguousarray(j["scalars"], dtype=np.uint8).reshape(-1, 32)
        psc = self.buf(max(sc.shape[0], 1) * 4, sc.view(np.uint64) if sc.shape[0] else None, dtype=np.uint64)[1]      # exactly the scalars the caller owns
        out, pout = self.buf(k * 12, dtype=np.uint64, fill=0xA5A5A5A5A5A5A5A5)                                      # every segment must be written
        _, poff64 = self.buf(pl["off_bytes"] // 8, dtype=np.uint64, fill=0xDEADBEEFDEADBEEF)
        _, ppart = self.buf(pl["part_bytes"] // 4, fill=0xDEADBEEF)
        _, pmeta = self.buf(pl["meta_bytes"] // 4, fill=0xDEADBEEF)
        st, pst = self.buf(1)
        rc = lib.emu_fred_msm(pa, pd, ptab, nbases, j["bits"], j["window"], pbf, self.buf(k + 1, off)[1], psc, k, total, block, terms, pout, poff64, ppart, pmeta, pst)
        res = np.zeros((0, 3, 4), dtype=np.uint64) if out is None else out.copy().reshape(k, 3, 4)
        return {"rc": rc, "out": res, "status": int(st[0]), "flag": flag}


if __name__ == "__main__":
    _Child.main()
