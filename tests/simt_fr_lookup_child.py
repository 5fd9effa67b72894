"""Builds the Fr lookup emulation library (tests/simt/emu_fr_lookup.cpp) and runs its entry points in a CHILD process
(tests/test_simt_fr_lookup.py).

Over tests/simt_harness.py: the library is built with trapping bounds / shift checks, and the table, the looked-up rows and every output
have exactly the size the call states, each ending flush against an inaccessible page (emu_guarded; the library allocates the handle's
keys, slots and counters the same way), so a kernel bug ends the process that runs it: `run(jobs)` starts
`python tests/simt_fr_lookup_child.py IN OUT` with the pickled jobs, under a time limit, and turns a signal, a time-out or a non-zero
exit into a pytest failure that names the job.

A job is a dict with "op" and "label"; the result list has one dict per job:
  run     table, f ((c, rows, 8) / (c, n, 8) u32 Montgomery words), [t_pitch, f_pitch], [negate], [block], [lds_rows: the path threshold],
          [reverse: build the later workgroups first], [outputs: which of "mult", "index", "missing" are not NULL], [lib: another build]
                                         -> mult ((rows, 8) u32 or None), index ((n,) u32 or None), missing (int or None), distinct, slots,
                                            lds_path, count_grid
  plan    rows, n, [block], [lds_rows]   -> ok, slots, block, build_grid, lds_path, count_lds, count_grid, iters, finish_grid
  hash    keys ((k, 8 c) u32), c         -> hashes (k ints)
Test infrastructure only: the product never imports this file."""
import ctypes

import numpy as np

import simt_harness

LIB = simt_harness.lib_path("emu_fr_lookup_test")
FAULTS = (1, 2, 3, 4, 5)                                           # fr_lookup.hip.h FRL_FAULT


def build():
    """build/libemu_fr_lookup_test.so, rebuilt when a source is newer"""
    return simt_harness.build("emu_fr_lookup_test", "emu_fr_lookup.cpp")


def build_degenerate():
    """the same library with the hash cut to two bits (-DFRL_HASH_BITS=2): long probe chains that wrap past the end of the slot array"""
    return simt_harness.build("emu_fr_lookup_hash2_test", "emu_fr_lookup.cpp", defines=("FRL_HASH_BITS=2",))


def build_fault(n):
    """the same library with seeded fault n (-DFRL_FAULT=n); fault 2 (a probe that does not wrap) on the two-bit hash, whose chains wrap"""
    return simt_harness.build("emu_fr_lookup_fault%d_test" % n, "emu_fr_lookup.cpp", defines=("FRL_FAULT=%d" % n,) + (("FRL_HASH_BITS=2",) if n == 2 else ()))


def run(jobs, timeout=600):
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
        lib.emu_fr_lookup_plan.argtypes = [sz, sz, ci, sz, vp]
        lib.emu_fr_lookup_hash.argtypes = [vp, ci]
        lib.emu_fr_lookup_hash.restype = ctypes.c_uint32
        lib.emu_fr_lookup_run.argtypes = [ci, vp, sz, sz, vp, sz, sz, ci, ci, sz, ci, vp, vp, vp, vp]

    def _lib(self, path):
        if path not in self.libs:
            lib = ctypes.CDLL(path)
            self._proto(lib)
            self.libs[path] = lib
        return self.libs[path]

    def plan(self, j):
        info = (ctypes.c_size_t * 8)()
        ok = self.lib.emu_fr_lookup_plan(j["rows"], j["n"], j.get("block", 0), j.get("lds_rows", 0), ctypes.cast(info, ctypes.c_void_p))
        names = ("slots", "block", "build_grid", "lds_path", "count_lds", "count_grid", "iters", "finish_grid")
        return dict({"ok": ok}, **{k: int(v) for k, v in zip(names, info)})

    def hash(self, j):
        keys = np.ascontiguousarray(j["keys"], dtype=np.uint32).reshape(-1, 8 * j["c"])
        out = []
        for k in keys:
            out.append(int(self.lib.emu_fr_lookup_hash(self.buf(k.size, k)[1], j["c"])))
        return {"hashes": out}

    def _set(self, x, pitch):
        """a (c, len, 8) column set in a buffer of exactly (c - 1) * pitch + len scalars -> address (None for len == 0)"""
        x = np.ascontiguousarray(x, dtype=np.uint32)
        c, n = x.shape[0], x.shape[1]
        if n == 0:
            return None
        a, p = self.buf(((c - 1) * pitch + n) * 8, fill=0x5A5A5A5A)
        for col in range(c):
            a[col * pitch * 8:(col * pitch + n) * 8] = x[col].reshape(-1)
        return p

    def run(self, j):
        t, f = np.asarray(j["table"]), np.asarray(j["f"])
        c, rows, n = t.shape[0], t.shape[1], f.shape[1]
        assert f.shape[0] == c
        tp, fp = j.get("t_pitch", rows), j.get("f_pitch", n)
        outputs = j.get("outputs", ("mult", "index", "missing"))
        mult, pmult = self.buf(rows * 8, fill=0xA5A5A5A5) if "mult" in outputs else (None, None)
        index, pindex = self.buf(n, fill=0xA5A5A5A5) if "index" in outputs else (None, None)
        missing, pmissing = self.buf(1, dtype=np.uint64, fill=0xA5A5A5A5A5A5A5A5) if "missing" in outputs else (None, None)
        info = (ctypes.c_size_t * 4)()
        rc = self._lib(j.get("lib")).emu_fr_lookup_run(c, self._set(t, tp), tp, rows, self._set(f, fp), fp, n, int(j.get("negate", 0)), j.get("block", 0), j.get("lds_rows", 0),
                                                     int(j.get("reverse", 0)), pmult, pindex, pmissing, ctypes.cast(info, ctypes.c_void_p))
        assert rc == 0, "the plan refused the shape"
        return {"mult": None if mult is None else mult.copy().reshape(-1, 8), "index": (np.zeros(0, dtype=np.uint32) if "index" in outputs else None) if index is None else index.copy(), "missing": None if missing is None else int(missing[0]),
                "distinct": int(info[0]), "slots": int(info[1]), "lds_path": int(info[2]), "count_grid": int(info[3])}


if __name__ == "__main__":
    _Child.main()
