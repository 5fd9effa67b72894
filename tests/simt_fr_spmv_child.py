"""Builds the Fr sparse matrix-vector emulation library (tests/simt/emu_fr_spmv.cpp) and runs its entry points in a CHILD process
(tests/test_simt_fr_spmv.py).

Over tests/simt_harness.py: the library is built with trapping bounds / shift checks, every buffer the kernels touch has exactly the
size the plan asks the host to reserve and ends flush against an inaccessible page (emu_guarded), so a kernel bug ends the process that
runs it: `run(jobs)` starts `python tests/simt_fr_spmv_child.py IN OUT` with the pickled jobs, under a time limit, and turns a signal,
a time-out or a non-zero exit into a pytest failure that names the job.

A job is a dict with "op" and "label"; the result list has one dict per job:
  spmv      row_ptr (n_rows + 1 u32), col (nnz u32), val (nnz, 8 u32 Montgomery words), n_cols, x (k, n_cols, 8 u32), [shape (block, chunk)]
            -> out (k, n_rows, 8 u32), kernels, has_empty, tile_row, val_resident (nnz, 8)
            the upload kernel (k_frsp_prepare) and then the plan; `out` is pre-filled with a pattern, so a row nobody writes shows
  validate  row_ptr, col, val, n_cols -> flag (k_frsp_validate's verdict bits)
`kernels` is the sequence of fr_spmv_plan.h FrSpmvKernel values the plan ran.
Test infrastructure only: the product never imports this file."""
import ctypes

import numpy as np

import simt_harness

ROOT, CLANG = simt_harness.ROOT, simt_harness.CLANG
LIB = simt_harness.lib_path("emu_fr_spmv_test")
K_FILL, K_TILE, K_FIXUP = 0, 1, 2
SHIPPED = (256, 8)                                                 # fr_spmv_plan.h FRSP_BLOCK, FRSP_CHUNK
PATTERN = 0xA5A5A5A5


def build():
    """build/libemu_fr_spmv_test.so, rebuilt when a source is newer"""
    return simt_harness.build("emu_fr_spmv_test", "emu_fr_spmv.cpp")


def run(jobs, timeout=300):
    """the jobs in a fresh child process; returns their results or fails the calling test"""
    return simt_harness.run(__file__, jobs, timeout)


# ---- child side --------------------------------------------------------------------------------------------------------------
class _Child(simt_harness.Child):
    def __init__(self):
        super().__init__(LIB)
        vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        self.lib.emu_fr_spmv_sizes.argtypes = [sz, sz, sz, ci, ci, ci, vp]
        self.lib.emu_fr_spmv_validate.argtypes = [vp, vp, vp, sz, sz, sz, vp]
        self.lib.emu_fr_spmv_validate.restype = None
        self.lib.emu_fr_spmv_prepare.argtypes = [vp, vp, vp, vp, vp, sz, sz, ci, ci]
        self.lib.emu_fr_spmv.argtypes = [vp, vp, vp, vp, sz, sz, sz, ci, vp, vp, sz, ci, ci, vp, vp, vp, vp]

    def _matrix(self, j):
        rp = np.ascontiguousarray(j["row_ptr"], dtype=np.uint32)
        col = np.ascontiguousarray(j["col"], dtype=np.uint32)
        val = np.ascontiguousarray(j["val"], dtype=np.uint32).reshape(-1, 8)
        return rp, col, val, len(rp) - 1, len(col)

    def validate(self, j):
        rp, col, val, n_rows, nnz = self._matrix(j)
        _, prp = self.buf(n_rows + 1, rp)
        _, pcol = self.buf(nnz, col)
        _, pval = self.buf(nnz * 8, val)
        flag, pflag = self.buf(1)
        self.lib.emu_fr_spmv_validate(prp, pcol, pval, n_rows, j["n_cols"], nnz, pflag)
        return {"flag": int(flag[0])}

    def spmv(self, j):
        rp, col, val, n_rows, nnz = self._matrix(j)
        assert int(rp[-1]) == nnz and len(val) == nnz
        x = np.ascontiguousarray(j["x"], dtype=np.uint32)
        k, n_cols = x.shape[0], j["n_cols"]
        assert x.shape == (k, n_cols, 8)
        block, chunk = j.get("shape") or SHIPPED
        _, prp = self.buf(n_rows + 1, rp)
        _, pcol = self.buf(nnz, col)
        res, pres = self.buf(nnz * 8, val)                         # the upload folds 2^5 in place, as the host form does
        tiles = (nnz + block * chunk - 1) // (block * chunk)
        trow, ptrow = self.buf(tiles + 1)
        flag, pflag = self.buf(2)
        assert self.lib.emu_fr_spmv_prepare(prp, pres, pres, ptrow, pflag, n_rows, nnz, block, chunk) == 0
        has_empty = int(flag[1]) != 0
        sizes = (ctypes.c_size_t * 3)()
        steps = self.lib.emu_fr_spmv_sizes(n_rows, nnz, k, 1 if has_empty else 0, block, chunk, ctypes.cast(sizes, ctypes.c_void_p))
        assert steps >= 0 and int(sizes[0]) == tiles
        _, px = self.buf(k * n_cols * 8, x)
        out, pout = self.buf(k * n_rows * 8, fill=PATTERN)
        _, phead = self.buf(int(sizes[1]) * 8, fill=PATTERN)
        _, ptail = self.buf(int(sizes[1]) * 8, fill=PATTERN)
        _, pmeta = self.buf(int(sizes[2]), fill=PATTERN)
        kern, pkern = self.buf(8)
        rc = self.lib.emu_fr_spmv(prp, pcol, pres, ptrow, n_rows, n_cols, nnz, 1 if has_empty else 0, px, pout, k, block, chunk, phead, ptail, pmeta, pkern)
        assert rc == steps, "emu_fr_spmv refused the arguments"
        return {"out": out.copy().reshape(k, n_rows, 8), "kernels": [int(v) for v in kern.view(np.int32)[:rc]], "has_empty": has_empty,
                "tile_row": trow.copy(), "val_resident": None if res is None else res.copy().reshape(-1, 8)}


if __name__ == "__main__":
    _Child.main()
