"""Builds the evaluation-form opening emulation library (tests/simt/emu_fr_bary.cpp) and runs it in a CHILD process (tests/test_simt_fr_bary.py).

As tests/simt_fr_scan_child.py: the library is built with trapping bounds / shift checks, every buffer the kernels touch has exactly the
size the plan asks the host to reserve and ends flush against an inaccessible page (emu_guarded), so a kernel bug ends the process that
runs it: `run(jobs)` starts `python tests/simt_fr_bary_child.py IN OUT` with the pickled jobs, under a time limit, and turns a signal, a
time-out or a non-zero exit into a pytest failure that names the job.

A job is a dict with "label" and
  evals (k, n, 8 u32 Montgomery words), points (k, 8 u32), [open (bool)], [order (0 natural, 1 bit-reversed)], [shape (block, chunk)]
and its result a dict: y (k, 8 u32), q (k, n, 8 u32) or None, kernels (the fr_bary_plan.h FrBaryKernel values the plan ran), evals_after,
points_after.  Test infrastructure only: the product never imports this file."""
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
LIB = os.path.join(ROOT, "build", "libemu_fr_bary_test.so")
K_ROWS, K_TILE, K_ROW, K_QUOT = 0, 1, 2, 3
SHIPPED = (256, 8)                                                 # fr_bary_plan.h FRB_BLOCK, FRB_CHUNK
REC_WORDS, ROWREC_WORDS = 28, 12                                   # fr_bary_plan.h FRB_REC_WORDS, FRB_ROWREC_WORDS


def build():
    """build/libemu_fr_bary_test.so, rebuilt when a source is newer (as the other emulation libraries are)"""
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    src = os.path.join(ROOT, "tests", "simt", "emu_fr_bary.cpp")
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
        self.lib.emu_fr_bary_recs.argtypes = [ci, sz, ci, ci, ci, vp]
        self.lib.emu_fr_bary.argtypes = [ci, vp, ci, sz, vp, ci, vp, vp, ci, ci, vp, vp, vp, vp]

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

    def bary(self, j):
        x = np.ascontiguousarray(j["evals"], dtype=np.uint32)
        k, n = x.shape[0], x.shape[1]
        log_n = n.bit_length() - 1
        assert n == 1 << log_n
        block, chunk = j.get("shape") or SHIPPED
        is_open = 1 if j.get("open") else 0
        recs = (ctypes.c_size_t * 2)()
        steps = self.lib.emu_fr_bary_recs(log_n, k, is_open, block, chunk, ctypes.cast(recs, ctypes.c_void_p))
        assert steps >= 0, "the plan refused the shape"
        dev, pev = self.buf(k * n * 8, x)
        dpt, ppt = self.buf(k * 8, j["points"])
        dy, py = self.buf(k * 8, fill=0xA5A5A5A5)
        dq, pq = self.buf(k * n * 8, fill=0xA5A5A5A5) if is_open else (None, None)
        _, ptw = self.buf(n * 8 if log_n and k else 0)               # the entry point reserves n scalars for the table of log_n
        _, prec = self.buf(int(recs[0]) * REC_WORDS, fill=0xA5A5A5A5)
        _, prow = self.buf(int(recs[1]) * ROWREC_WORDS, fill=0xA5A5A5A5)
        kern, pkern = self.buf(8)
        rc = self.lib.emu_fr_bary(is_open, pev, log_n, k, ppt, j.get("order", 0), py, pq, block, chunk, ptw, prec, prow, pkern)
        assert rc >= 0, "emu_fr_bary refused the arguments"
        return {"y": np.zeros((0, 8), dtype=np.uint32) if dy is None else dy.copy().reshape(k, 8),
                "q": None if not is_open else (np.zeros((0, n, 8), dtype=np.uint32) if dq is None else dq.copy().reshape(k, n, 8)),
                "kernels": [int(v) for v in kern.view(np.int32)[:rc]],
                "evals_after": None if dev is None else dev.copy().reshape(k, n, 8), "points_after": None if dpt is None else dpt.copy().reshape(k, 8)}


def _main(fin, fout):
    with open(fin, "rb") as fh:
        jobs = pickle.load(fh)
    c = _Child()
    results = []
    for i, j in enumerate(jobs):
        sys.stderr.write("JOB %d: %s\n" % (i, j.get("label", "")))
        sys.stderr.flush()
        results.append(c.bary(j))
    with open(fout, "wb") as fh:
        pickle.dump(results, fh)


if __name__ == "__main__":
    _main(sys.argv[1], sys.argv[2])
