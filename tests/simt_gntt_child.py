"""Builds the group transform emulation library (tests/simt/emu_gntt.cpp) and runs its entry points in a CHILD process (tests/test_simt_gntt.py).

Over tests/simt_harness.py: the library is built with trapping bounds / shift checks, every buffer the kernels touch has exactly the size the
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
import re

import numpy as np

import simt_harness

ROOT, CLANG = simt_harness.ROOT, simt_harness.CLANG
LIB = simt_harness.lib_path("emu_gntt_test")
K_PERMUTE, K_FIRST, K_STAGE = 0, 1, 2
LANE, TEAM = 0, 1
ENV = "BLSGPU_GNTT_TEAM_MAX"
with open(os.path.join(ROOT, "bls12_381_amd", "csrc", "gntt_plan.h")) as _fh:
    TEAM_MAX_B = int(re.search(r"GNTT_TEAM_MAX_B = (\d+);", _fh.read()).group(1))       # the built-in crossover, as the header states it


def build():
    """build/libemu_gntt_test.so, rebuilt when a source is newer"""
    return simt_harness.build("emu_gntt_test", "emu_gntt.cpp")


def run(jobs, timeout=600):
    """the jobs in a fresh child process; returns their results or fails the calling test"""
    return simt_harness.run(__file__, jobs, timeout)


# ---- child side --------------------------------------------------------------------------------------------------------------
class _Child(simt_harness.Child):
    def __init__(self):
        super().__init__(LIB)
        vp = ctypes.c_void_p
        self.lib.emu_gntt_many.argtypes = [ctypes.c_int, vp, vp, vp, ctypes.c_int, ctypes.c_size_t, ctypes.c_int, vp]
        self.lib.emu_gntt_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_longlong, vp]

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


if __name__ == "__main__":
    _Child.main()
