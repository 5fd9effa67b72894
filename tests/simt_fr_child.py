"""Builds the Fr transform emulation library (tests/simt/emu_fr.cpp) and runs its entry points in a CHILD process (tests/test_simt_fr.py).

As tests/simt_msm_child.py: the library is built with trapping bounds / shift checks, every buffer the kernels touch ends flush against an
inaccessible page (emu_guarded), so a kernel bug ends the process that runs it: `run(jobs)` starts `python tests/simt_fr_child.py IN OUT`
with the pickled jobs, under a time limit, and turns a signal, a time-out or a non-zero exit into a pytest failure that names the job.

A job is a dict with "op" and "label"; the result list has one dict per job:
  many    data (k, n, 8 u32 Montgomery words), inverse, [coset (8 u32)], [cols (tlog, dmax, block)], [threads]  -> out (k, n, 8 u32), kernels
  single  data (n, 8 u32), inverse, [threads]                                                                     -> out (n, 8 u32)
`kernels` is the sequence of fr_plan.h FrKernel values the plan ran (0 cols, 1 stage2, 2 stage1, 3 tile).
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
LIB = os.path.join(ROOT, "build", "libemu_fr_test.so")
K_COLS, K_STAGE2, K_STAGE1, K_TILE = 0, 1, 2, 3


def build():
    """build/libemu_fr_test.so, rebuilt when a source is newer (as the other emulation libraries are)"""
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    src = os.path.join(ROOT, "tests", "simt", "emu_fr.cpp")
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
        vp = ctypes.c_void_p
        self.lib.emu_fr_ntt_many.argtypes = [vp, vp, vp, vp, vp, ctypes.c_int, ctypes.c_size_t, ctypes.c_int, vp] + [ctypes.c_int] * 5 + [vp]
        self.lib.emu_fr_tile_single.argtypes = [vp, vp, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int]

    def buf(self, words, init=None):
        """guarded u32 buffer of exactly `words` words (its last word is the last accessible one), as (numpy view, address)"""
        n = max(words, 1) * 4
        p = self.lib.emu_guarded(n)
        assert p, "emu_guarded failed"
        a = np.frombuffer((ctypes.c_uint32 * max(words, 1)).from_address(p), dtype=np.uint32)
        a[:] = 0
        if init is not None:
            a[:words] = np.ascontiguousarray(init, dtype=np.uint32).reshape(-1)
        return a[:words], ctypes.c_void_p(p)

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
