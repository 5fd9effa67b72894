"""Builds the Poseidon emulation library (tests/simt/emu_fr_poseidon.cpp) and runs it in a CHILD process (tests/test_simt_fr_poseidon.py).

Over tests/simt_harness.py: the library is built with trapping bounds / shift checks, every buffer the kernels touch -- the constant
image included -- has exactly the size the entry point reserves and ends flush against an inaccessible page (emu_guarded), so a kernel
bug ends the process that runs it: `run(jobs)` starts `python tests/simt_fr_poseidon_child.py IN OUT` with the pickled jobs, under a time
limit, and turns a signal, a time-out or a non-zero exit into a pytest failure that names the job.

A job is a dict with "label" and
  params   (t, r_full, r_partial, constants, mds) as Python ints (tests/fr_poseidon_ref.py), [form (0 AUTO, 1 DENSE)]
  kind     "create" (only build the instance), "permute", "hash", "merkle"
  data     permute: (n, t, 8) u32 Montgomery words; hash: (n, t - 1, 8); merkle: (k * a^height, 8)
  [tag]    an int (hash, merkle), [height], [k], [nodes (bool)], [inplace (bool)], [block]
and its result a dict: form, products, out (permute: (n, t, 8); hash: (n, 8); merkle: the roots (k, 8)), nodes ((count, 8) or None),
kernels (the fr_poseidon_plan.h FrPoseidonKernel values the plan ran), data_after; a refused "create" gives {"refused": text}.
Test infrastructure only: the product never imports this file."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fr_poseidon_ref as ref  # noqa: E402
import simt_harness  # noqa: E402

ROOT, CLANG = simt_harness.ROOT, simt_harness.CLANG
LIB = simt_harness.lib_path("emu_fr_poseidon_test")
K_PERMUTE, K_HASH, K_LEVEL, K_COPY = 0, 1, 2, 4
FORM_AUTO, FORM_DENSE, FORM_SPARSE = 0, 1, 2
SHIPPED = 256                                                      # fr_poseidon_plan.h FRP_BLOCK


def build():
    """build/libemu_fr_poseidon_test.so, rebuilt when a source is newer"""
    return simt_harness.build("emu_fr_poseidon_test", "emu_fr_poseidon.cpp")


def run(jobs, timeout=600):
    """the jobs in a fresh child process; returns their results or fails the calling test"""
    return simt_harness.run(__file__, jobs, timeout)


# ---- child side --------------------------------------------------------------------------------------------------------------
class _Child(simt_harness.Child):
    OP = "job"

    def __init__(self):
        super().__init__(LIB)
        vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        self.lib.emu_frp_create.argtypes = [ci, ci, ci, vp, vp, ci, vp, vp, sz]
        self.lib.emu_frp_plan.argtypes = [ci, sz, ci, ci, ci, vp]
        self.lib.emu_frp_run.argtypes = [ci, vp, vp, sz, ci, ci, vp, vp, ci, vp]
        self.last = None

    def create(self, j):
        t, rf, rp, consts, mds = j["params"]
        key = (t, rf, rp, j.get("form", FORM_AUTO), j.get("params_id"))
        if key[4] is not None and self.last is not None and self.last[0] == key:
            return self.last[1]
        flat = [c for row in consts for c in row]
        rc = np.ascontiguousarray(j["raw_constants"] if "raw_constants" in j else ref.limbs(flat), dtype=np.uint64)
        mm = np.ascontiguousarray(ref.limbs([m for row in mds for m in row]), dtype=np.uint64)
        info = (ctypes.c_size_t * 3)()
        err = ctypes.create_string_buffer(256)
        rc_ = self.lib.emu_frp_create(t, rf, rp, rc.ctypes.data_as(ctypes.c_void_p), mm.ctypes.data_as(ctypes.c_void_p), j.get("form", FORM_AUTO),
                                      ctypes.cast(info, ctypes.c_void_p), ctypes.cast(err, ctypes.c_void_p), 256)
        if rc_ == -1:
            self.last = None
            return {"refused": err.value.decode()}
        assert rc_ == 0, "emu_frp_create failed"
        res = {"form": int(info[0]), "products": int(info[1]), "image_words": int(info[2])}
        self.last = (key, res)
        return res

    def job(self, j):
        res = dict(self.create(j))
        kind = j["kind"]
        if kind == "create" or "refused" in res:
            return res
        t = j["params"][0]
        block = j.get("block") or SHIPPED
        data = np.ascontiguousarray(j["data"], dtype=np.uint32)
        kern, pkern = self.buf(40)
        ddata, pdata = self.buf(data.size, data)
        tag, ptag = self.buf(8, ref.words([j.get("tag", 0)]))
        sizes = (ctypes.c_size_t * 3)()
        if kind in ("permute", "hash"):
            n = data.shape[0]
            ki = 0 if kind == "permute" else 1
            assert self.lib.emu_frp_plan(ki, n, 0, 0, block, ctypes.cast(sizes, ctypes.c_void_p)) >= 0
            if kind == "permute" and j.get("inplace"):
                dout, pout = ddata, pdata
            else:
                dout, pout = self.buf(n * (t if kind == "permute" else 1) * 8, fill=0xA5A5A5A5)
            before = data.copy()
            rc = self.lib.emu_frp_run(ki, ptag, pdata, n, 0, 0, pout, None, block, pkern)
            assert rc >= 0, "emu_frp_run refused the arguments"
            shape = (n, t, 8) if kind == "permute" else (n, 8)
            res.update(out=np.zeros(shape, dtype=np.uint32) if dout is None else dout.copy().reshape(shape), nodes=None,
                       data_after=before if j.get("inplace") else (None if ddata is None else ddata.copy().reshape(data.shape)))
        else:
            k, height, keep = j["k"], j["height"], 1 if j.get("nodes", True) else 0
            steps = self.lib.emu_frp_plan(2, k, height, keep, block, ctypes.cast(sizes, ctypes.c_void_p))
            assert steps >= 0, "the plan refused the shape"
            assert int(sizes[0]) * 8 == data.size, "leaves: expected k * a^height scalars"
            count = int(sizes[1])
            dnodes, pnodes = self.buf((count if keep else int(sizes[2])) * 8, fill=0xA5A5A5A5)
            droots, proots = self.buf(k * 8, fill=0xA5A5A5A5)
            rc = self.lib.emu_frp_run(2, ptag, pdata, k, height, keep, proots, pnodes, block, pkern)
            assert rc >= 0, "emu_frp_run refused the arguments"
            res.update(out=np.zeros((0, 8), dtype=np.uint32) if droots is None else droots.copy().reshape(k, 8),
                       nodes=(np.zeros((0, 8), dtype=np.uint32) if dnodes is None else dnodes.copy().reshape(count, 8)) if keep else None,
                       data_after=None if ddata is None else ddata.copy().reshape(data.shape))
        res["kernels"] = [int(v) for v in kern.view(np.int32)[:rc]]
        return res


if __name__ == "__main__":
    _Child.main()
