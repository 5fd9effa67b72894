"""Builds the Fr expression emulation library (tests/simt/emu_fr_expr.cpp) and runs its entry points in a CHILD process
(tests/test_simt_fr_expr.py).

Over tests/simt_harness.py: the library is built with trapping bounds / shift checks, every column has exactly 2^col_log_len scalars, the
image exactly the words the handle uploads and `out` exactly 2^log_n scalars, each ending flush against an inaccessible page
(emu_guarded), so a kernel bug ends the process that runs it: `run(jobs)` starts `python tests/simt_fr_expr_child.py IN OUT` with the
pickled jobs, under a time limit, and turns a signal, a time-out or a non-zero exit into a pytest failure that names the job.

A job is a dict with "op" and "label"; the result list has one dict per job:
  eval    n_cols, n_regs, consts ((n, 4) u64 Montgomery limbs or None), code (flat u32 words), cols (per column: (len, 8) u32 words, None,
          or an int = "the very buffer of that earlier column"), col_log_len (list or None), log_n, log_stride, [shape (block, chunk)],
          [lib: another build of the library]                                  -> out (2^log_n, 8 u32), grid
  build   n_cols, n_regs, consts, code, [n_consts, n_instr: override the counts] -> ok, error, products, cols_read, max_rot
  plan    log_n, n_regs, [shape]                                               -> ok, grid, block, chunk, lds, tile, rows
Test infrastructure only: the product never imports this file."""
import ctypes

import numpy as np

import simt_harness

LIB = simt_harness.lib_path("emu_fr_expr_test")
MAX_COLS = 32
FAULTS = (1, 2, 3, 4, 5)                                           # fr_expr.hip.h FRX_FAULT


def build():
    """build/libemu_fr_expr_test.so, rebuilt when a source is newer"""
    return simt_harness.build("emu_fr_expr_test", "emu_fr_expr.cpp")


def build_fault(n):
    """the same library with seeded fault n (-DFRX_FAULT=n)"""
    return simt_harness.build("emu_fr_expr_fault%d_test" % n, "emu_fr_expr.cpp", defines=("FRX_FAULT=%d" % n,))


def run(jobs, timeout=300):
    """the jobs in a fresh child process; returns their results or fails the calling test"""
    return simt_harness.run(__file__, jobs, timeout)


# ---- child side --------------------------------------------------------------------------------------------------------------
class _Child(simt_harness.Child):
    def __init__(self):
        simt_harness.Child.__init__(self, LIB)
        self.libs = {None: self.lib}
        self._proto(self.lib)

    @staticmethod
    def _proto(lib):
        vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        lib.emu_fr_expr_plan.argtypes = [ci, ci, ci, ci, vp]
        lib.emu_fr_expr_build.argtypes = [ci, ci, ci, vp, sz, vp, vp, vp, vp, sz]
        lib.emu_fr_expr_eval.argtypes = [vp, vp, vp, ci, ci, ci, ci, vp]

    def _lib(self, path):
        if path not in self.libs:
            lib = ctypes.CDLL(path)
            self._proto(lib)
            self.libs[path] = lib
        return self.libs[path]

    def plan(self, j):
        block, chunk = j.get("shape") or (0, 0)
        info = (ctypes.c_size_t * 6)()
        ok = self.lib.emu_fr_expr_plan(j["log_n"], j["n_regs"], block, chunk, ctypes.cast(info, ctypes.c_void_p))
        return {"ok": ok, "grid": int(info[0]), "block": int(info[1]), "chunk": int(info[2]), "lds": int(info[3]), "tile": int(info[4]), "rows": int(info[5])}

    def _build(self, j):
        """-> (result dict, image address)"""
        consts = j.get("consts")
        n_consts = j.get("n_consts", 0 if consts is None else len(consts))
        code = np.ascontiguousarray(j["code"], dtype=np.uint32).reshape(-1)
        n_instr = j.get("n_instr", code.size // 3)
        pconsts = None if consts is None else self.buf(max(len(consts), 1) * 4, consts if len(consts) else None, dtype=np.uint64)[1]
        pcode = self.buf(code.size, code)[1] if code.size else None
        info = (ctypes.c_size_t * 4)()
        err = ctypes.create_string_buffer(256)
        words = 4 + 3 * 256 + 8 * 32
        image, pimage = self.buf(words)
        rc = self.lib.emu_fr_expr_build(j["n_cols"], j["n_regs"], n_consts, pconsts, n_instr, pcode, pimage, ctypes.cast(info, ctypes.c_void_p), err, 256)
        assert int(info[3]) == words, "the image size moved"
        return {"ok": rc == 0, "error": err.value.decode(), "products": int(info[0]), "cols_read": int(info[1]), "max_rot": int(info[2])}, pimage

    def build(self, j):
        return self._build(j)[0]

    def eval(self, j):
        res, pimage = self._build(j)
        assert res["ok"], "the program was refused: " + res["error"]
        log_n = j["log_n"]
        ll = j.get("col_log_len")
        ptrs = (ctypes.c_void_p * MAX_COLS)()
        lens = (ctypes.c_uint32 * MAX_COLS)()
        for c, x in enumerate(j["cols"]):
            if x is None:
                continue
            lens[c] = log_n if ll is None else ll[c]
            if isinstance(x, int):
                ptrs[c] = ptrs[x]
                continue
            x = np.ascontiguousarray(x, dtype=np.uint32).reshape(-1, 8)
            assert x.shape[0] == 1 << lens[c], (c, x.shape, lens[c])
            ptrs[c] = self.buf(x.size, x)[1]
        dout, pout = self.buf(8 << log_n)
        dout[:] = 0xA5A5A5A5                                       # every row must be written
        block, chunk = j.get("shape") or (0, 0)
        grid = self._lib(j.get("lib")).emu_fr_expr_eval(pimage, ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(lens, ctypes.c_void_p), log_n, j["log_stride"], block, chunk, pout)
        assert grid >= 0, "the plan refused the shape"
        return {"out": dout.copy().reshape(-1, 8), "grid": grid}


if __name__ == "__main__":
    _Child.main()
