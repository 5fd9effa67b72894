"""Builds the emulation library of the MSM's integer front end (tests/simt/emu_msm_front.cpp) and runs its entry points in a CHILD process
(tests/test_simt_msm_front.py), over tests/simt_harness.py: trapping bounds / shift checks, every buffer flush against an
inaccessible page, a crash or a time-out becomes a pytest failure that names the job.

Every buffer a kernel reads or writes has exactly the size csrc/msm_plan.h msm_sizes gives for it (the field in brackets) -- none of the
`bytes / 8 + 256` slack of DevBuf::reserve (host.h), in which an entry written a little past the end changes nothing on the GPU:
  ent / sorted / rank   total * 4 bytes, total = nwin * ns                                              (ent, sorted, cursor)
  hist                  (3 * SORT_MAX_COUNTERS + 4) * 4 for the fast sort; nb * 4 for the fallback (what msm_sort_fallback clears)   (hist)
  offs                  (nb + 1) * 4                                                                    (offs)
  bsum                  4096 * 4                                                                        (bsum)
  items                 max_items * sizeof(ItemDesc), max_items = total / cap + nb + 1                  (MsmShape max_items; items)
  heavy                 2 * nb * sizeof(uint4)                                                          (heavy)
  ctrl                  (4 + 2 * ITEM_BINS) * 4                                                         (ctrl)

A job is a dict with "op" and "label":
  state     (none)                                                  -> fresh sort state for the jobs after it (hist zeroed once, as at allocation)
  fast      words, values (stored sort scalars), c, nwin, merged, stride  -> offs, sorted, status, hist_zero, ctrl_zero
            runs on the CURRENT sort state (hist, ctrl): consecutive jobs share it, as consecutive calls share a slot
  fallback  values, c, nwin                                         -> offs, sorted, status
  items     offs, cap                                               -> ctrl (4 words), items (ctrl[2], 3), heavy (ctrl[1], 4), big (ctrl[3])
  consts    (none)                                                  -> the constants of msm.hip.h / limits.h the model restates
Test infrastructure only: the product never imports this file."""
import ctypes

import numpy as np

import simt_harness

LIB = simt_harness.lib_path("emu_msm_front_test")
CONSTS = ["SORT_TILE", "SORT_THREADS", "SORT_MAX_COUNTERS", "ITEM_CAP_MAX", "ITEM_BINS", "ITEM_BLOCK_BUCKETS", "HEAVY_SMALL", "HEAVY_BIG_BLOCKS",
          "sizeof_ItemDesc", "sizeof_uint4"]


def build():
    """build/libemu_msm_front_test.so, rebuilt when a source is newer"""
    return simt_harness.build("emu_msm_front_test", "emu_msm_front.cpp")


def run(jobs, timeout=300):
    return simt_harness.run(__file__, jobs, timeout)


def words_of(values, words):
    """stored sort scalars (integers below 2^(32 words)) as the u32 words the kernels read"""
    if not len(values):
        return np.zeros(0, np.uint32)
    return np.frombuffer(b"".join(int(v).to_bytes(4 * words, "little") for v in values), dtype=np.uint32).copy()


# ---- child side --------------------------------------------------------------------------------------------------------------
class _Child(simt_harness.Child):
    def __init__(self):
        super().__init__(LIB)
        self.k = {name: int(self.lib.emu_front_constants(i)) for i, name in enumerate(CONSTS)}
        self.nctrl = 4 + 2 * self.k["ITEM_BINS"]
        self.state(None)

    def consts(self, j):
        return dict(self.k)

    def state(self, j):
        self.hist, self.phist = self.buf(3 * self.k["SORT_MAX_COUNTERS"] + 4)
        self.ctrl, self.pctrl = self.buf(self.nctrl, fill=0xdeadbeef)           # the sort clears the item-control words itself
        return {}

    def fast(self, j):
        words, c, nwin, merged = int(j["words"]), int(j["c"]), int(j["nwin"]), int(j.get("merged", 0))
        vals = j["values"]
        ns = len(vals)
        nb = (1 if merged else nwin) << (c - 1)
        total = nwin * ns
        assert self.lib.emu_sort_counters(c, nwin, merged) > 0 and ns > 0
        _, pin = self.buf(ns * words, words_of(vals, words))
        ent, pent = self.buf(total, fill=0xffffffff)
        srt, psrt = self.buf(total, fill=0xffffffff)
        offs, poffs = self.buf(nb + 1, fill=0xffffffff)
        status, pstatus = self.buf(1)
        self.lib.emu_sort_fast(words, pin, ns, c, nwin, merged, ctypes.c_uint32(int(j.get("stride", 0))), self.phist, self.pctrl, pent, psrt, poffs, pstatus)
        m = self.k["SORT_MAX_COUNTERS"]
        return {"offs": offs.copy(), "sorted": srt.copy(), "status": int(status[0]), "hist_zero": not self.hist[:m].any(),
                "ctrl_zero": not self.ctrl.any()}

    def fallback(self, j):
        c, nwin = int(j["c"]), int(j["nwin"])
        vals = j["values"]
        n = len(vals)
        nb, total = nwin << (c - 1), nwin * n
        _, pin = self.buf(n * 8, words_of(vals, 8))
        _, phist = self.buf(nb)
        _, pbsum = self.buf(4096, fill=0xffffffff)
        _, pent = self.buf(total, fill=0xeeeeeeee)
        _, prank = self.buf(total, fill=0xeeeeeeee)
        srt, psrt = self.buf(total, fill=0xffffffff)
        offs, poffs = self.buf(nb + 1, fill=0xffffffff)
        status, pstatus = self.buf(1)
        self.lib.emu_sort_fallback(pin, n, c, nwin, phist, pbsum, pent, prank, poffs, psrt, pstatus)
        return {"offs": offs.copy(), "sorted": srt.copy(), "status": int(status[0])}

    def items(self, j):
        offs = np.ascontiguousarray(j["offs"], dtype=np.uint32)
        nb, cap = len(offs) - 1, int(j["cap"])
        max_items = int(offs[-1]) // cap + nb + 1
        _, poffs = self.buf(nb + 1, offs)
        ctrl, pctrl = self.buf(self.nctrl)
        items, pitems = self.buf(max_items * 3, fill=0xffffffff)
        assert self.k["sizeof_ItemDesc"] == 12 and self.k["sizeof_uint4"] == 16
        heavy, pheavy = self.buf(2 * nb * 4, fill=0xffffffff)
        self.lib.emu_items(poffs, nb, ctypes.c_uint32(cap), pctrl, pitems, pheavy)
        c4 = [int(x) for x in ctrl[:4]]
        assert c4[2] <= max_items and c4[1] <= nb and c4[3] <= nb
        h = heavy.reshape(2 * nb, 4)
        return {"ctrl": c4, "items": items.reshape(max_items, 3)[:c4[2]].copy(), "rest_untouched": bool((items.reshape(max_items, 3)[c4[2]:] == 0xffffffff).all()),
                "heavy": h[:c4[1]].copy(), "big": h[nb:nb + c4[3], 0].copy()}


if __name__ == "__main__":
    _Child.main()
