"""What the host emulations of the device code share on the Python side (tests/simt_*_child.py, tests/test_simt_*.py): the one compile
line of the emulation libraries, the child-process round trip that turns a crash into a named test failure, and the base class of the
child side.  The C++ half is tests/simt/emu_harness.h.

An emulation library is built with trapping bounds / shift checks, and every buffer its kernels touch ends flush against an inaccessible
page (emu_guarded), so a kernel bug ends the process that runs it.  A family module therefore runs its jobs in a CHILD process:
`run(__file__, jobs, timeout)` starts `python <family module> IN OUT` with the pickled jobs, under a time limit, and turns a signal, a
time-out or a non-zero exit into a pytest failure that names the job; the family module's `__main__` is `_Child.main()`, the job loop below.
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
SIMT = os.path.join(ROOT, "tests", "simt")
CSRC = os.path.join(ROOT, "bls12_381_amd", "csrc")


def lib_path(name):
    return os.path.join(ROOT, "build", "lib%s.so" % name)


def build(name, source, defines=(), sanitize=True):
    """build/lib<name>.so from tests/simt/<source>, rebuilt when the source, a file under tests/simt or a csrc header is newer.
    sanitize: the trapping bounds / shift checks -- for a library that runs in a child process, where a trap ends only the child."""
    lib = lib_path(name)
    os.makedirs(os.path.dirname(lib), exist_ok=True)
    src = os.path.join(SIMT, source)
    deps = [src] + [os.path.join(d, f) for d, _, fs in os.walk(SIMT) for f in fs] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(d) for d in deps):
        tmp = lib + ".tmp%d" % os.getpid()                         # another pytest process may be loading the library right now
        subprocess.check_call([CLANG, "-O1", "-std=c++17", "-pthread", "-fPIC", "-shared", "-Wno-unused-value", "-Wno-psabi"]
                              + (["-fsanitize=bounds,shift", "-fsanitize-trap=all"] if sanitize else []) + ["-D" + d for d in defines]
                              + ["-I" + SIMT, "-I" + CSRC, src, "-o", tmp])
        os.replace(tmp, lib)
    return lib


def emu_lib(build_fn):
    """the body of a test module's `emu_lib` fixture: the built library, or a skip where there is no host clang++"""
    import pytest
    if not os.path.exists(CLANG):
        pytest.skip("no host clang++ in this image")
    return build_fn()


def run(child_module_file, jobs, timeout, stuck="a lane waiting at a barrier for ever?"):
    """the jobs in a fresh child process (`python child_module_file IN OUT`); returns their results or fails the calling test"""
    import pytest
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.pkl"), os.path.join(d, "out.pkl")
        with open(fin, "wb") as fh:
            pickle.dump(jobs, fh)
        try:
            p = subprocess.run([sys.executable, os.path.abspath(child_module_file), fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, text=True)
        except subprocess.TimeoutExpired as e:
            err = e.stderr if isinstance(e.stderr, str) else (e.stderr or b"").decode()
            pytest.fail("the emulation did not finish in %d s (%s); last job: %s" % (timeout, stuck, _last_job(err)))
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


class Child:
    """The child side of a family: its library and one method per job "op", each taking the job and returning its result dict.
    `results` holds the results of the jobs before the current one (a job may refer to an earlier one by its index)."""
    OP = None                                                      # the handler of every job, in a family whose jobs carry no "op"

    def __init__(self, lib):
        self.lib = ctypes.CDLL(lib)
        self.lib.emu_guarded.restype = ctypes.c_void_p
        self.lib.emu_guarded.argtypes = [ctypes.c_size_t]
        self.results = []

    def buf(self, words, init=None, dtype=np.uint32, fill=0):
        """guarded buffer of exactly `words` items (its last item is the last accessible one), as (numpy view, address); None for none"""
        if words == 0:
            return None, None
        size = np.dtype(dtype).itemsize
        p = self.lib.emu_guarded(words * size)
        assert p, "emu_guarded failed"
        ct = {1: ctypes.c_uint8, 4: ctypes.c_uint32, 8: ctypes.c_uint64}[size]
        a = np.frombuffer((ct * words).from_address(p), dtype=dtype)
        a[:] = fill
        if init is not None:
            a[:] = np.ascontiguousarray(init, dtype=dtype).reshape(-1)
        return a, ctypes.c_void_p(p)

    @classmethod
    def main(cls):
        """`python <family module> IN OUT`: the jobs pickled in IN, one after the other, their results into OUT.  Each job's JOB line
        reaches stderr before the job starts: it is how `run` names the job a crash or a time-out happened in."""
        with open(sys.argv[1], "rb") as fh:
            jobs = pickle.load(fh)
        c = cls()
        for i, j in enumerate(jobs):
            sys.stderr.write("JOB %d%s: %s\n" % (i, " " + j["op"] if cls.OP is None else "", j.get("label", "")))
            sys.stderr.flush()
            c.results.append(getattr(c, cls.OP or j["op"])(j))
        with open(sys.argv[2], "wb") as fh:
            pickle.dump(c.results, fh)
