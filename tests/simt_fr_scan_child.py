"""Builds the Fr scan emulation library (tests/simt/emu_fr_scan.cpp) and runs its entry points in a CHILD process (tests/test_simt_fr_scan.py).

As tests/simt_fr_child.py: the library is built with trapping bounds / shift checks, every buffer the kernels touch has exactly the size
the plan asks the host to reserve and ends flush against an inaccessible page (emu_guarded), so a kernel bug ends the process that runs
it: `run(jobs)` starts `python tests/simt_fr_scan_child.py IN OUT` with the pickled jobs, under a time limit, and turns a signal, a
time-out or a non-zero exit into a pytest failure that names the job.

A job is a dict with "op" and "label"; the result list has one dict per job:
  scan    scan_op (0 sum, 1 product, 2 horner), data (k, len, 8 u32 Montgomery words), [points (k, 8 u32)], [exclusive], [shape (block, chunk)],
          [inplace]                                                                                      -> out (k, len, 8 u32), kernels
  invert  data (n, 8 u32), [flags (bool)], [shape], [inplace]                                            -> out (n, 8 u32), flags (n u8 | None), kernels
`kernels` is the sequence of fr_scan_plan.h FrScanKernel values the plan ran.
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
LIB = os.path.join(ROOT, "build", "libemu_fr_scan_test.so")
K_SINGLE, K_REDUCE, K_AGG_REDUCE, K_AGG_SCAN, K_SCAN, K_INVERT = 0, 1, 2, 3, 4, 5
SHIPPED = (256, 8)                                                 # fr_scan_plan.h FRS_BLOCK, FRS_CHUNK
REC_WORDS = {0: 12, 1: 12, 2: 20}                                  # fr_scan_plan.h frs_rec_words(op)


def build():
    """build/libemu_fr_scan_test.so, rebuilt when a source is newer (as the other emulation libraries are)"""
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    src = os.path.join(ROOT, "tests", "simt", "emu_fr_scan.cpp")
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
        self.lib.emu_fr_scan_recs.argtypes = [sz, sz, ci, ci, vp]
        self.lib.emu_fr_scan.argtypes = [ci, ci, vp, vp, vp, sz, sz, ci, ci, vp, vp, vp, vp, vp, vp]
        self.lib.emu_fr_invert.argtypes = [vp, vp, vp, sz, ci, ci, vp]

    def buf(self, words, init=None, dtype=np.uint32):
        """guarded buffer of exactly `words` items (its last item is the last accessible one), as (numpy view, address); None for none"""
        if words == 0:
            return None, None
        size = np.dtype(dtype).itemsize
        p = self.lib.emu_guarded(words * size)
        assert p, "emu_guarded failed"
        ct = ctypes.c_uint32 if size == 4 else ctypes.c_uint8
        a = np.frombuffer((ct * words).from_address(p), dtype=dtype)
        a[:] = 0
        if init is not None:
            a[:] = np.ascontiguousarray(init, dtype=dtype).reshape(-1)
        return a, ctypes.c_void_p(p)

    def scan(self, j):
        x = np.ascontiguousarray(j["data"], dtype=np.uint32)
        k, n = x.shape[0], x.shape[1]
        block, chunk = j.get("shape") or SHIPPED
        recs = (ctypes.c_size_t * 5)()
        steps = self.lib.emu_fr_scan_recs(n, k, block, chunk, ctypes.cast(recs, ctypes.c_void_p))
        assert steps >= 0, "the plan refused the shape"
        din, pin = self.buf(k * n * 8, x)
        dout, pout = (din, pin) if j.get("inplace") else self.buf(k * n * 8)
        pts = j.get("points")
        _, ppts = self.buf(k * 8, pts) if pts is not None else (None, None)
        scratch = [self.buf(int(recs[i]) * (8 if i in (2, 3) else REC_WORDS[j["scan_op"]]))[1] for i in range(5)]
        kern, pkern = self.buf(8)
        rc = self.lib.emu_fr_scan(j["scan_op"], 1 if j.get("exclusive") else 0, pin, pout, ppts, n, k, block, chunk, *scratch, pkern)
        assert rc >= 0, "emu_fr_scan refused the arguments"
        out = np.zeros((k, n, 8), dtype=np.uint32) if dout is None else dout.copy().reshape(k, n, 8)
        return {"out": out, "kernels": [int(v) for v in kern.view(np.int32)[:rc]], "in_after": None if din is None else din.copy().reshape(k, n, 8)}

    def invert(self, j):
        x = np.ascontiguousarray(j["data"], dtype=np.uint32)
        n = x.shape[0]
        block, chunk = j.get("shape") or SHIPPED
        din, pin = self.buf(n * 8, x)
        dout, pout = (din, pin) if j.get("inplace") else self.buf(n * 8)
        fl, pfl = self.buf(n, dtype=np.uint8) if j.get("flags") else (None, None)
        if fl is not None:
            fl[:] = 7                                              # every flag must be written
        kern, pkern = self.buf(8)
        rc = self.lib.emu_fr_invert(pin, pout, pfl, n, block, chunk, pkern)
        assert rc >= 0, "emu_fr_invert refused the arguments"
        out = np.zeros((n, 8), dtype=np.uint32) if dout is None else dout.copy().reshape(n, 8)
        return {"out": out, "flags": None if fl is None else fl.copy(), "kernels": [int(v) for v in kern.view(np.int32)[:rc]]}


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
