"""Builds the emulation library of the amortised KZG openings (tests/simt/emu_kzg.cpp) and runs its entry points in a CHILD process
(tests/test_simt_kzg.py).

Over tests/simt_harness.py: the library is built with trapping bounds / shift checks, every buffer the kernels touch has exactly the size
the plan asks the host to reserve and ends flush against an inaccessible page (emu_guarded), so a kernel bug ends the process that runs
it: `run(jobs)` starts `python tests/simt_kzg_child.py IN OUT` with the pickled jobs, under a time limit, and turns a signal, a time-out
or a non-zero exit into a pytest failure that names the job.

A job is a dict with "op" and "label"; one job runs the whole data movement of one call, with the transforms and the MSM between the
stages done here in Python integers (tests/kzg_ref.py: the group-as-scalars model, a point [s] G1 being a wire record that carries s):
  proofs  log_n, log_l, sigma (n ints), polys (count x n ints: coefficients or evaluations), form, order, [tile], [fault]
          -> rows, seg (the scalars behind the rows / transposition kernels), xhat, offsets, base_first, filled (the upper half after the
             fill: True where every record is the identity), proofs (count x 2c ints)
  cells   log_n, log_l, polys, form, order, [tile], [fault]   -> cells (count x 2c x l ints)
  plan    log_n, log_l, count, form, [tile]                   -> the numbers of emu_kzg_plan
Test infrastructure only: the product never imports this file."""
import ctypes

import numpy as np

import kzg_ref as k
import simt_harness
from oracle import bls12_381_ref as o

LIB = simt_harness.lib_path("emu_kzg_test")
FAULTS = (1, 2, 3)                                                 # kzg.hip.h KZG_FAULT
FP_ONE = o.fp_to_mont_limbs(1)


def build():
    """build/libemu_kzg_test.so, rebuilt when a source is newer"""
    return simt_harness.build("emu_kzg_test", "emu_kzg.cpp")


def build_fault(n):
    """the same library with seeded fault n (-DKZG_FAULT=n)"""
    return simt_harness.build("emu_kzg_fault%d_test" % n, "emu_kzg.cpp", defines=("KZG_FAULT=%d" % n,))


def fault_lib_path(n):
    return simt_harness.lib_path("emu_kzg_fault%d_test" % n)


def run(jobs, timeout=300):
    """the jobs in a fresh child process; returns their results or fails the calling test"""
    return simt_harness.run(__file__, jobs, timeout)


def _fr(vals):
    return np.array([o.fr_to_mont_limbs(int(v) % k.R) for v in vals], dtype=np.uint64).reshape(-1, 4)


def _ints(limbs):
    return [o.fr_from_mont_limbs([int(w) for w in row]) for row in np.asarray(limbs).reshape(-1, 4)]


def _records(scalars):
    """[s] G1 in the model: X carries s (four limbs), Y a tag, Z = 1; s = None is the identity (Z = 0)"""
    out = np.zeros((len(scalars), 18), dtype=np.uint64)
    for i, s in enumerate(scalars):
        if s is None:
            out[i, 6:12] = FP_ONE
            continue
        out[i, 0:4] = [(int(s) >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)]
        out[i, 6] = 0x7A6
        out[i, 12:18] = FP_ONE
    return out


def _scalars_of(records):
    """the scalar a record carries; None for an identity record, which must be exactly (0 : 1 : 0)"""
    out = []
    for r in np.asarray(records).reshape(-1, 18):
        if not r[12:18].any():
            assert not r[0:6].any() and list(r[6:12]) == FP_ONE, "an identity record that is not (0 : 1 : 0)"
            out.append(None)
        else:
            assert list(r[12:18]) == FP_ONE and r[6] == 0x7A6, "a record that is neither a model point nor the identity"
            out.append(sum(int(r[j]) << (64 * j) for j in range(4)))
    return out


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
        lib.emu_kzg_plan.argtypes = [ci, ci, sz, ci, ci, vp]
        lib.emu_kzg_srs_rows.argtypes = [vp, vp, vp, ci, ci]
        lib.emu_kzg_srs_transpose.argtypes = [vp, vp, ci, ci]
        lib.emu_kzg_copy.argtypes = [vp, vp, sz, ci, ci, ci]
        lib.emu_kzg_coeff_rows.argtypes = [vp, vp, sz, ci, ci, ci]
        lib.emu_kzg_transpose.argtypes = [vp, vp, sz, ci, ci, ci]
        lib.emu_kzg_segments.argtypes = [vp, vp, sz, ci, ci]
        lib.emu_kzg_fill.argtypes = [vp, sz, ci, ci]
        lib.emu_kzg_permute.argtypes = [vp, vp, sz, ci, ci, ci]
        lib.emu_kzg_cells_map.argtypes = [vp, vp, sz, ci, ci, ci, ci]
        return lib

    def plan(self, j):
        info = (ctypes.c_size_t * 13)()
        self._lib(j.get("fault", 0)).emu_kzg_plan(j["log_n"], j["log_l"], j["count"], j.get("form", 0), j.get("tile", 0), ctypes.cast(info, ctypes.c_void_p))
        names = ("ok", "msm", "scalars", "points", "vectors", "coeff_bytes", "rows_bytes", "seg_bytes", "point_bytes", "offset_bytes", "base_first_bytes", "transpose_grid", "transpose_block")
        return {n: int(info[i]) for i, n in enumerate(names)}

    def _coeffs(self, lib, j, count, n, log_n):
        """the coefficients as the later stages read them: the caller's array, or the copy in scratch after the inverse transform"""
        x, px = self.buf(count * n * 4, _fr([v for p in j["polys"] for v in p]), dtype=np.uint64)
        if j["form"] != k.EVALS:
            return x, px
        c, pc = self.buf(count * n * 4, dtype=np.uint64, fill=0xA5A5A5A5A5A5A5A5)
        assert lib.emu_kzg_copy(px, pc, count, log_n, log_n, 1 if j["order"] == k.BITREV else 0) == 0
        rows = np.array(_ints(c)).reshape(count, n)
        c[:] = _fr([v for r in rows for v in o.fr_ntt(list(r), inverse=True)]).reshape(-1)
        return c, pc

    def proofs(self, j):
        lib = self._lib(j.get("fault", 0))
        log_n, log_l, tile = j["log_n"], j["log_l"], j.get("tile", 0)
        n, l, c = 1 << log_n, 1 << log_l, 1 << (log_n - log_l)
        count = len(j["polys"])
        pl = self.plan(dict(j, count=count))
        assert pl["ok"]
        res = {}
        if not pl["msm"]:
            out, pout = self.buf(count * 2 * 18, dtype=np.uint64, fill=0xA5A5A5A5A5A5A5A5)
            assert lib.emu_kzg_fill(pout, count, log_n, log_l) == 0
            res["proofs"] = np.array([0 if s is None else s for s in _scalars_of(out)], dtype=object).reshape(count, 2).tolist()
            return res
        # create: the gather, the l transforms of size 2c (here), the transposition
        sx = np.zeros((n, 12), dtype=np.uint64)
        for i, s in enumerate(j["sigma"]):                          # the model carries sigma as a plain integer in X; None is an identity in the SRS
            if s is not None:
                sx[i, 0:4] = [(int(s) >> (64 * w)) & 0xFFFFFFFFFFFFFFFF for w in range(4)]
                sx[i, 6] = 0x7A6
        inf = np.array([1 if s is None else 0 for s in j["sigma"]], dtype=np.uint8)
        _, pxy = self.buf(n * 12, sx, dtype=np.uint64)
        _, pinf = self.buf(n, inf, dtype=np.uint8)
        shat, pshat = self.buf(2 * n * 18, dtype=np.uint64, fill=0xA5A5A5A5A5A5A5A5)
        assert lib.emu_kzg_srs_rows(pxy, pinf, pshat, log_n, log_l) == 0
        res["srs_rows"] = np.array(_scalars_of(shat), dtype=object).reshape(l, 2 * c).tolist()
        tr = [o.fr_ntt([0 if s is None else s for s in row]) for row in res["srs_rows"]]
        shat[:] = _records([v for row in tr for v in row]).reshape(-1)
        xh, pxh = self.buf(2 * n * 18, dtype=np.uint64, fill=0xA5A5A5A5A5A5A5A5)
        assert lib.emu_kzg_srs_transpose(pshat, pxh, log_n, log_l) == 0
        xhat = [0 if s is None else s for s in _scalars_of(xh)]
        res["xhat"] = xhat
        # the call
        _, pc = self._coeffs(lib, j, count, n, log_n)
        rows, prows = self.buf(pl["rows_bytes"] // 8, dtype=np.uint64, fill=0xA5A5A5A5A5A5A5A5)
        assert lib.emu_kzg_coeff_rows(pc, prows, count, log_n, log_l, j["form"]) == 0
        res["rows"] = np.array(_ints(rows), dtype=object).reshape(count, l, 2 * c).tolist()
        rows[:] = _fr([v for poly in res["rows"] for row in poly for v in o.fr_ntt(list(row))]).reshape(-1)
        seg, pseg = self.buf(pl["seg_bytes"] // 8, dtype=np.uint64, fill=0xA5A5A5A5A5A5A5A5)
        assert lib.emu_kzg_transpose(prows, pseg, count, log_n, log_l, tile) == 0
        res["seg"] = np.array(_ints(seg), dtype=object).reshape(count, 2 * c * l).tolist()
        off, poff = self.buf(pl["offset_bytes"] // 4, fill=0xDEADBEEF)
        bf, pbf = self.buf(pl["base_first_bytes"] // 4, fill=0xDEADBEEF)
        assert lib.emu_kzg_segments(poff, pbf, count, log_n, log_l) == 0
        res["offsets"], res["base_first"] = off.tolist(), bf.tolist()
        flat = [v for poly in res["seg"] for v in poly]
        sums = [sum(flat[int(off[s]) + t] * xhat[int(bf[s]) + t] for t in range(int(off[s + 1]) - int(off[s]))) % k.R for s in range(count * 2 * c)]
        inv = [v for v0 in range(count) for v in o.fr_ntt(sums[v0 * 2 * c:(v0 + 1) * 2 * c], inverse=True)]
        pts, ppts = self.buf(pl["point_bytes"] // 8, _records(inv), dtype=np.uint64)
        assert lib.emu_kzg_fill(ppts, count, log_n, log_l) == 0
        got = np.array(_scalars_of(pts), dtype=object).reshape(count, 2 * c)
        res["filled"] = all(s is None for s in got[:, c:].reshape(-1)) and all(s is not None for s in got[:, :c].reshape(-1))
        fwd = [v for row in got for v in o.fr_ntt([0 if s is None else s for s in row])]
        pts[:] = _records(fwd).reshape(-1)
        out, pout = self.buf(count * 2 * c * 18, dtype=np.uint64, fill=0xA5A5A5A5A5A5A5A5)
        assert lib.emu_kzg_permute(ppts, pout, count, log_n, log_l, j["order"]) == 0
        res["proofs"] = np.array(_scalars_of(out), dtype=object).reshape(count, 2 * c).tolist()
        return res

    def cells(self, j):
        lib = self._lib(j.get("fault", 0))
        log_n, log_l = j["log_n"], j["log_l"]
        n = 1 << log_n
        count = len(j["polys"])
        _, pc = self._coeffs(lib, j, count, n, log_n)
        ext, pext = self.buf(count * 2 * n * 4, dtype=np.uint64, fill=0xA5A5A5A5A5A5A5A5)
        assert lib.emu_kzg_copy(pc, pext, count, log_n, log_n + 1, 0) == 0
        rows = np.array(_ints(ext), dtype=object).reshape(count, 2 * n)
        assert all(v == 0 for v in rows[:, n:].reshape(-1)), "the extension is not zero"
        ext[:] = _fr([v for r in rows for v in o.fr_ntt(list(r))]).reshape(-1)
        cells, pcells = self.buf(count * 2 * n * 4, dtype=np.uint64, fill=0xA5A5A5A5A5A5A5A5)
        assert lib.emu_kzg_cells_map(pext, pcells, count, log_n, log_l, j["order"], j.get("tile", 0)) == 0
        return {"cells": np.array(_ints(cells), dtype=object).reshape(count, 2 * (n >> log_l), 1 << log_l).tolist()}


if __name__ == "__main__":
    _Child.main()
