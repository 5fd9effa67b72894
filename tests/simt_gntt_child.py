"""Builds the group transform emulation library (tests/simt/emu_gntt.cpp) and runs its entry points in a CHILD process (tests/test_simt_gntt.py).

As tests/simt_fr_child.py: the library is built with trapping bounds / shift checks, every buffer the kernels touch has exactly the size the
host reserves for it and ends flush against an inaccessible page (emu_guarded), so a kernel bug ends the process that runs it: `run(jobs)`
starts `python tests/simt_gntt_child.py IN OUT` with the pickled jobs, under a time limit, and turns a signal, a time-out or a non-zero exit
into a pytest failure that names the job.

A job is a dict with "op" and "label"; the result list has one dict per job:
  many  group (1 | 2), data (k, n, 36 | 72 u32: projective wire points), inverse, [team_max]  -> out (same shape), steps, shape
  plan  group, log_n, k, [team_max]                                                            -> steps [(kernel, shape, grid, block, lds, stage)]
`team_max` is put into BLSGPU_GNTT_TEAM_MAX for the call -- the override the library reads (csrc/diag.h) -- and decides between the
lane shape (0) and the team shape (1) of csrc/gntt_plan.h; absent, the plan's built-in constant applies.
Test infrastructure only: the product never imports this file."""
import ctypes
import os
import pickle
import re
import signal
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
LIB = os.path.join(ROOT, "build", "libemu_gntt_test.so")
K_PERMUTE, K_FIRST, K_STAGE = 0, 1, 2
LANE, TEAM = 0, 1
ENV = "BLSGPU_GNTT_TEAM_MAX"
with open(os.path.join(ROOT, "bls12_381_amd", "csrc", "gntt_plan.h")) as _fh:
    TEAM_MAX_B = int(re.search(r"GNTT_TEAM_MAX_B = (\d+);", _fh.read()).group(1))       # the built-in crossover, as the header states it


def build():
    """build/libemu_gntt_test.so, rebuilt when a source is newer (as the other emulation libraries are)"""
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    src = os.path.join(ROOT, "tests", "simt", "emu_gntt.cpp")
    csrc = os.path.join(ROOT, "bls12_381_amd", "csrc")
    deps = [src, os.path.join(ROOT, "tests", "simt", "hip", "hip_runtime.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in deps):
        tmp = LIB + ".tmp%d" % os.getpid()
        subprocess.check_call([CLANG, "-O1", "-std=c++17", "-pthread", "-fPIC", "-shared", "-Wno-unused-value", "-Wno-psabi",
                               "-fsanitize=bounds,shift", "-fsanitize-trap=all",
                               "-I" + os.path.join(ROOT, "tests", "simt"), "-I" + csrc, src, "-o", tmp])
        os.replace(tmp, LIB)
    return LIB


def run(jobs, timeout=600):
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
        self.lib.emu_gntt_many.argtypes = [ctypes.c_int, vp, vp, vp, ctypes.c_int, ctypes.c_size_t, ctypes.c_int, vp]
        self.lib.emu_gntt_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_longlong, vp]

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

    @staticmethod
    def _override(j):
        os.environ.pop(ENV, None)
        if j.get("team_max") is not None:
            os.environ[ENV] = str(j["team_max"])

    def steps(self, group, log_n, k):
        out, pout = self.buf(6 * 25)
        rc = self.lib.emu_gntt_plan(group, log_n, k, -1, pout)
        assert rc >= 0, "emu_gntt_plan refused the arguments"
        return [tuple(int(v) for v in out.view(np.int32)[6 * i:6 * i + 6]) for i in range(rc)]

    def plan(self, j):
        self._override(j)
        return {"steps": self.steps(j["group"], j["log_n"], j["k"])}

    def many(self, j):
        self._override(j)
        x = np.ascontiguousarray(j["data"]).view(np.uint32)
        k, n, w = x.shape
        assert w == 36 * j["group"]
        log_n = n.bit_length() - 1
        data, pdata = self.buf(k * n * w, x)
        _, ptw = self.buf((n - 1) * 8)                   # 2^log_n - 1 table entries: what the library reserves at least
        _, pninv = self.buf(8)
        shape, pshape = self.buf(1)
        rc = self.lib.emu_gntt_many(j["group"], pdata, ptw, pninv, log_n, k, 1 if j.get("inverse") else 0, pshape)
        assert rc >= 0, "emu_gntt_many refused the arguments"
        return {"out": data.copy().reshape(k, n, w), "steps": self.steps(j["group"], log_n, k), "shape": int(shape[0])}


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
