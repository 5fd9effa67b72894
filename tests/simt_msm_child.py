"""Builds the MSM emulation library (tests/simt/emu_msm.cpp) and runs its entry points in a CHILD process (tests/test_simt_msm.py).

Over tests/simt_harness.py: the library is built with trapping bounds / shift checks, and every buffer the kernels read ends flush
against an inaccessible page (emu_guarded), so a kernel bug ends the process that runs it: `run(jobs)` starts
`python tests/simt_msm_child.py IN OUT` with the pickled jobs, under a time limit, and turns a signal, a time-out or a non-zero exit into a
pytest failure that names the job.

A job is a dict with "op" and "label"; the result list has one dict per job:
  bases       group, xy (n, 12|24 u64 wire), inf (n u8) or None, [endo], [check]  -> rec, endo (u32 words), nbad
  segments    bases (index of an earlier bases job), split, offsets, scalars (total, 8 u32), form, k, [base_first], [batch], [total],
              [nbases]                                                            -> out (k, 18|36 u64), status, wsums (wire, last batch)
  decompose   group, scalars (n, 8 u32), form                                     -> out (u32 words), status
  accumulate  bases, nsplit, sorted, items (m, 3 u32), ctrl (4 u32), max_items, ndest, [bases2_endo]    -> records (ndest, 18 u64 wire)
The point kernels of the large MSM, one stage per job (tests/test_simt_msm_points.py); points travel as projective wire limbs
((n, 18|36) u64) and live in PROJ-record buffers of exactly the stated number of records, each against a guard page:
  accumulate_g2  bases, sorted, items, ctrl, max_items, ndest                       -> records
  heavy       group, records, heavy (m, 4 u32), big (indices into heavy), ctrl, nb  -> records (in place)
  level       group, form (0 team2, 1 team, 2 pair), E (nseg * n), nseg, n, M, off  -> R, T (nseg * n / M each)
  tree        group, E, nseg, n, M                                                  -> out (nseg * ceil(n / M))
  tree_multi  group, nseg, trees [(E, n, M)]                                        -> outs
  shift_add   group, x, y (nseg each), k                                            -> out
  combine     group, wsums (nwin), c                                                -> out (1)
  reduce      group, records (nseg * nbw), nseg, nbw, [fault]                       -> wsums (nseg), levels: the whole reduction by the
              schedule of csrc/msm_plan.h, in buffers of the sizes of msm_sizes
Test infrastructure only: the product never imports this file."""
import ctypes

import numpy as np

import simt_harness

ROOT, CLANG = simt_harness.ROOT, simt_harness.CLANG
LIB = simt_harness.lib_path("emu_msm_test")
AFF_WORDS = {1: 32, 2: 64}
PROJ_WORDS = {1: 44, 2: 84}
WIRE = {1: 6, 2: 12}                                               # u64 limbs per field element on the wire
NWIN = {(1, 1): 32, (1, 0): 64, (2, 1): 16, (2, 0): 64}            # msm_seg.hip.h SegCfg::NWIN by (group, split)


def build():
    """build/libemu_msm_test.so, rebuilt when a source is newer"""
    return simt_harness.build("emu_msm_test", "emu_msm.cpp")


def run(jobs, timeout=300):
    """the jobs in a fresh child process; returns their results or fails the calling test"""
    return simt_harness.run(__file__, jobs, timeout, stuck="a lane waiting for a partner that never comes?")


# ---- child side --------------------------------------------------------------------------------------------------------------
class _Child(simt_harness.Child):
    def __init__(self):
        super().__init__(LIB)

    def guarded(self, a):
        """a copy of the array that ends flush against an inaccessible page; returns its address (None for None)"""
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        n = max(a.nbytes, 4)
        p = self.lib.emu_guarded(n)
        assert p, "emu_guarded failed"
        if a.nbytes:
            ctypes.memmove(p + n - a.nbytes, a.ctypes.data, a.nbytes)
        return ctypes.c_void_p(p + n - a.nbytes)

    def out(self, words):
        """zeroed guarded u32 output buffer as a numpy view"""
        n = max(words, 1) * 4
        p = self.lib.emu_guarded(n)
        buf = (ctypes.c_uint32 * max(words, 1)).from_address(p)
        a = np.frombuffer(buf, dtype=np.uint32)
        a[:] = 0
        return a[:words] if words else a[:0], ctypes.c_void_p(p)

    def bases(self, j):
        g = j["group"]
        xy = np.ascontiguousarray(j["xy"], dtype=np.uint64).reshape(-1, 2 * WIRE[g])
        n = xy.shape[0]
        rec, prec = self.out(n * AFF_WORDS[g])
        inf = None if j.get("inf") is None else np.ascontiguousarray(j["inf"], dtype=np.uint8)
        self.lib.emu_bases_import(g, self.guarded(xy), self.guarded(inf), prec, ctypes.c_size_t(n))
        res = {"rec": rec.copy(), "n": n, "group": g, "endo": None, "nbad": None}
        if j.get("check"):
            bad, pbad = self.out(1)
            self.lib.emu_bases_subgroup_check(g, self.guarded(rec), ctypes.c_size_t(n), pbad)
            res["nbad"] = int(bad[0])
        if j.get("endo"):
            endo, pendo = self.out(n * AFF_WORDS[g] * (1 if g == 1 else 4))
            self.lib.emu_bases_endo(g, self.guarded(rec), pendo, ctypes.c_size_t(n))
            res["endo"] = endo.copy()
        return res

    def segments(self, j):
        b = self.results[j["bases"]]
        g, split = b["group"], int(j["split"])
        k = int(j["k"])
        batch = int(j.get("batch") or max(k, 1))
        off = np.ascontiguousarray(j["offsets"], dtype=np.uint32)
        s = np.ascontiguousarray(j["scalars"], dtype=np.uint32).reshape(-1, 8)
        total = int(j["total"]) if j.get("total") is not None else s.shape[0]
        nbases = int(j["nbases"]) if j.get("nbases") is not None else b["n"]
        bf = None if j.get("base_first") is None else np.ascontiguousarray(j["base_first"], dtype=np.uint32)
        nwin, pw, ww = NWIN[(g, split)], PROJ_WORDS[g], 2 * WIRE[g]
        status, pstatus = self.out(1)
        wsums, pws = self.out(batch * nwin * pw)
        srec, psrec = self.out(batch * pw)
        out, pout = self.out(k * 3 * ww)
        endo = self.guarded(b["endo"]) if split else None
        assert not split or b["endo"] is not None
        self.lib.emu_msm_segments(g, split, self.guarded(b["rec"]), endo, ctypes.c_size_t(nbases), self.guarded(bf), self.guarded(off), self.guarded(s),
                                  ctypes.c_size_t(k), ctypes.c_size_t(batch), ctypes.c_size_t(total), int(j["form"]), pstatus, pws, psrec, pout)
        nlast = (k - 1) % batch + 1 if k else 0
        wire, pwire = self.out(nlast * nwin * 3 * ww)
        self.lib.emu_proj_export(g, self.guarded(wsums), pwire, ctypes.c_size_t(nlast * nwin))
        return {"out": out.copy().view(np.uint64).reshape(k, 3 * WIRE[g]), "status": int(status[0]),
                "wsums": wire.copy().view(np.uint64).reshape(nlast, nwin, 3 * WIRE[g])}

    def decompose(self, j):
        s = np.ascontiguousarray(j["scalars"], dtype=np.uint32).reshape(-1, 8)
        n = s.shape[0]
        out, pout = self.out(n * 8)
        status, pstatus = self.out(1)
        self.lib.emu_decompose(int(j["group"]), self.guarded(s), pout, n, pstatus, int(j["form"]))
        return {"out": out.copy(), "status": int(status[0])}

    def accumulate(self, j):
        b = self.results[j["bases"]]
        assert b["group"] == 1
        items = np.ascontiguousarray(j["items"], dtype=np.uint32).reshape(-1, 3)
        ndest = int(j["ndest"])
        rec, prec = self.out(ndest * PROJ_WORDS[1])
        bases2 = self.guarded(b["endo"]) if j.get("bases2_endo") else None
        self.lib.emu_msm_accumulate_g1(self.guarded(b["rec"]), bases2, ctypes.c_uint32(int(j["nsplit"])), self.guarded(np.ascontiguousarray(j["sorted"], dtype=np.uint32)),
                                       self.guarded(items), self.guarded(np.ascontiguousarray(j["ctrl"], dtype=np.uint32)), prec, ctypes.c_uint32(int(j["max_items"])))
        wire, pwire = self.out(ndest * 36)
        self.lib.emu_proj_export(1, self.guarded(rec), pwire, ctypes.c_size_t(ndest))
        return {"records": wire.copy().view(np.uint64).reshape(ndest, 18)}

    # ---- the point kernels of the large MSM ---------------------------------------------------------------------------------------
    def recs(self, group, wire):
        """projective wire limbs -> a guarded buffer of exactly that many PROJ records (k_proj_import); (view, address, n)"""
        wire = np.ascontiguousarray(wire, dtype=np.uint64).reshape(-1, 3 * WIRE[group])
        n = wire.shape[0]
        rec, prec = self.buf(n * PROJ_WORDS[group])
        self.lib.emu_proj_import(group, self.guarded(wire), prec, ctypes.c_size_t(n))
        return rec, prec, n

    def empty(self, group, n):
        return self.buf(n * PROJ_WORDS[group])

    def wire(self, group, rec, n):
        out, pout = self.out(n * 6 * WIRE[group])
        self.lib.emu_proj_export(group, self.guarded(rec), pout, ctypes.c_size_t(n))
        return out.copy().view(np.uint64).reshape(n, 3 * WIRE[group])

    def accumulate_g2(self, j):
        b = self.results[j["bases"]]
        assert b["group"] == 2
        items = np.ascontiguousarray(j["items"], dtype=np.uint32).reshape(-1, 3)
        ndest = int(j["ndest"])
        rec, prec = self.empty(2, ndest)
        _, pbases = self.buf(len(b["rec"]), b["rec"])
        _, psorted = self.buf(len(j["sorted"]), j["sorted"])
        _, pitems = self.buf(items.size, items)
        _, pctrl = self.buf(4, j["ctrl"])
        self.lib.emu_msm_accumulate_g2(pbases, psorted, pitems, pctrl, prec, ctypes.c_uint32(int(j["max_items"])))
        return {"records": self.wire(2, rec, ndest)}

    def heavy(self, j):
        g, nb = int(j["group"]), int(j["nb"])
        rec, prec, n = self.recs(g, j["records"])
        heavy, pheavy = self.buf(2 * nb * 4, fill=0xffffffff)
        h = heavy.reshape(2 * nb, 4)
        for i, e in enumerate(j["heavy"]):
            h[i] = e
        for i, e in enumerate(j["big"]):
            h[nb + i, 0] = e
        _, pctrl = self.buf(4, j["ctrl"])
        self.lib.emu_msm_heavy(g, pheavy, pctrl, prec, ctypes.c_uint32(nb))
        return {"records": self.wire(g, rec, n)}

    def level(self, j):
        g, nseg, n, M = int(j["group"]), int(j["nseg"]), int(j["n"]), int(j["M"])
        _, pe, ne = self.recs(g, j["E"])
        assert ne == nseg * n and n % M == 0
        chains = nseg * (n // M)
        r, pr = self.empty(g, chains)
        t, pt = self.empty(g, chains)
        self.lib.emu_wsum_level(g, int(j["form"]), pe, pr, pt, nseg, n, M, int(j["off"]))
        return {"R": self.wire(g, r, chains), "T": self.wire(g, t, chains)}

    def tree(self, j):
        g, nseg, n, M = int(j["group"]), int(j["nseg"]), int(j["n"]), int(j["M"])
        _, pe, ne = self.recs(g, j["E"])
        assert ne == nseg * n
        m = nseg * ((n + M - 1) // M)
        o, po = self.empty(g, m)
        self.lib.emu_tree_sum(g, pe, po, nseg, n, M)
        return {"out": self.wire(g, o, m)}

    def tree_multi(self, j):
        g, nseg = int(j["group"]), int(j["nseg"])
        k = len(j["trees"])
        ins, outs, views, ns, ms = (ctypes.c_void_p * k)(), (ctypes.c_void_p * k)(), [], (ctypes.c_int * k)(), (ctypes.c_int * k)()
        for i, (E, n, M) in enumerate(j["trees"]):
            _, pe, ne = self.recs(g, E)
            assert ne == nseg * n
            m = nseg * ((n + M - 1) // M)
            o, po = self.empty(g, m)
            ins[i], outs[i], ns[i], ms[i] = pe.value, po.value, n, M
            views.append((o, m))
        self.lib.emu_tree_sum_multi(g, k, ins, outs, ns, ms, nseg)
        return {"outs": [self.wire(g, o, m) for o, m in views]}

    def shift_add(self, j):
        g = int(j["group"])
        rx, px, n = self.recs(g, j["x"])
        _, py, _ = self.recs(g, j["y"])
        self.lib.emu_shift_add(g, px, py, px, n, int(j["k"]))       # in place, as api_msm.hip msm_reduce runs it (accbuf is x and out)
        return {"out": self.wire(g, rx, n)}

    def combine(self, j):
        g = int(j["group"])
        _, pw, n = self.recs(g, j["wsums"])
        o, po = self.empty(g, 1)
        self.lib.emu_msm_combine(g, pw, po, n, int(j["c"]))
        return {"out": self.wire(g, o, 1)}

    def reduce(self, j):
        g, nseg, nbw = int(j["group"]), int(j["nseg"]), int(j["nbw"])
        _, prec, n = self.recs(g, j["records"])
        assert n == nseg * nbw
        words = (ctypes.c_size_t * 5)()
        self.lib.emu_msm_reduce_words(g, nseg, ctypes.c_uint32(nbw), words)
        pair = lambda w: (ctypes.c_void_p * 2)(self.buf(w, fill=0xffffffff)[1].value, self.buf(w, fill=0xffffffff)[1].value)
        lvlR, (_, plvlT), tsum, wacc = pair(words[0]), self.buf(words[1], fill=0xffffffff), pair(words[2]), pair(words[3])
        assert words[4] == nseg * PROJ_WORDS[g]
        ws, pws = self.empty(g, nseg)
        levels = self.lib.emu_msm_reduce(g, prec, nseg, ctypes.c_uint32(nbw), lvlR, plvlT, tsum, wacc, pws, int(j.get("fault", 0)))
        return {"wsums": self.wire(g, ws, nseg), "levels": int(levels)}


if __name__ == "__main__":
    _Child.main()
