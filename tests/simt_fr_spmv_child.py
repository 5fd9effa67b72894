"""Builds the Fr sparse matrix-vector emulation library (tests/simt/emu_fr_spmv.cpp) and runs its entry points in a CHILD process
(tests/test_simt_fr_spmv.py).

As tests/simt_fr_scan_child.py: the library is built with trapping bounds / shift checks, every buffer the kernels touch has exactly the
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
import os
import pickle
import signal
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
LIB = os.path.join(ROOT, "build", "libemu_fr_spmv_test.so")
K_FILL, K_TILE, K_FIXUP = 0, 1, 2
SHIPPED = (256, 8)                                                 # fr_spmv_plan.h FRSP_BLOCK, FRSP_CHUNK
PATTERN = 0xA5A5A5A5


def build():
    """build/libemu_fr_spmv_test.so, rebuilt when a source is newer (as the other emulation libraries are)"""
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    src = os.path.join(ROOT, "tests", "simt", "emu_fr_spmv.cpp")
    csrc = os.path.join(ROOT, "bls12_381_amd", "csrc")
    deps = [src, os.path.join(ROOT, "tests", "simt", "hip", "hip_runtime.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in deps):
        tmp = LIB + ".tmp%d" % os.getpid()
        subprocess.check_call([CLANG, "-O1", "-std=c++17", "-pthread", "-fPIC", "-shared", "-Wno-unused-value", "-Wno-psabi",
                               "-fsanitize=bounds,shift", "-fsanitize-trap=all",
                               "-I" + os.path.join(ROOT, "tests", "simt"), "-I" + csrc, src, "-o", tmp])
        os.replace(tmp, LIB)
    return LIB


def run(jobs, timeout=300):
    """the jobs in a fresh child process; returns their results or fails the calling test"""
    import pytest
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.pkl"), os.path.join(d, "out.pkl")
        with open(fin, "wb") as fh:
            pickle.dump(jobs, fh)
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, text=True)
        except subprocess.TimeoutExpired as e:
            err = e.stderr if isinstance(e.stderr, str) else (e.stderr or b"").decode()
            pytest.fail("the emulation did not finish in %d s (a lane waiting at a barrier for ever?); last job: %s" % (timeout, _last_job(err)))
        if p.returncode != 0:
            what = "signal %s" % signal.Signals(-p.returncode).name if p.returncode < 0 else "exit status %d" % p.returncode
            hint = {"SIGILL": " (a trapping bounds / shift check)", "SIGTRAP": " (a trapping bounds / shift check)",
                    "SIGSEGV": " (an access outside a guarded buffer)"}.get(what.split()[-1], "")
            pytest.fail("the emulation child ended with %s%s in job: %s\n%s" % (what, hint, _last_job(p.stderr), p.stderr[-2000:]))
        with open(fout, "rb") as fh:
            return pickle.load(fh)


def _last_job(err):
    marks = [l for l in (err or "").splitlines() if l.startswith("JOB ")]
    return marks[-1][4:] if marks else "(none started)"


# ---- child side --------------------------------------------------------------------------------------------------------------
class _Child:
    def __init__(self):
        self.lib = ctypes.CDLL(LIB)
        self.lib.emu_guarded.restype = ctypes.c_void_p
        self.lib.emu_guarded.argtypes = [ctypes.c_size_t]
        vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        self.lib.emu_fr_spmv_sizes.argtypes = [sz, sz, sz, ci, ci, ci, vp]
        self.lib.emu_fr_spmv_validate.argtypes = [vp, vp, vp, sz, sz, sz, vp]
        self.lib.emu_fr_spmv_validate.restype = None
        self.lib.emu_fr_spmv_prepare.argtypes = [vp, vp, vp, vp, vp, sz, sz, ci, ci]
        self.lib.emu_fr_spmv.argtypes = [vp, vp, vp, vp, sz, sz, sz, ci, vp, vp, sz, ci, ci, vp, vp, vp, vp]

    def buf(self, words, init=None, fill=0):
        """guarded buffer of exactly `words` u32 (its last word is the last accessible one), as (numpy view, address); None for none"""
        if words == 0:
            return None, None
        p = self.lib.emu_guarded(words * 4)
        assert p, "emu_guarded failed"
        a = np.frombuffer((ctypes.c_uint32 * words).from_address(p), dtype=np.uint32)
        a[:] = fill
        if init is not None:
            a[:] = np.ascontiguousarray(init, dtype=np.uint32).reshape(-1)
        return a, ctypes.c_void_p(p)

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


def _main(fin, fout):
    with open(fin, "rb") as fh:
        jobs = pickle.load(fh)
    c = _Child()
    results = []
    for i, j in enumerate(jobs):
        sys.stderr.write("JOB %d %s: %s\n" % (i, j["op"], j.get("label", "")))
        sys.stderr.flush()
        results.append(getattr(c, j["op"])(j))
    with open(fout, "wb") as fh:
        pickle.dump(results, fh)


if __name__ == "__main__":
    _main(sys.argv[1], sys.argv[2])
