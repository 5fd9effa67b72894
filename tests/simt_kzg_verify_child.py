"""Builds the emulation library of batched KZG cell-proof verification (tests/simt/emu_kzg_verify.cpp) and runs its entry points in a
CHILD process (tests/test_simt_kzg_verify.py).

Over tests/simt_harness.py: the library is built with trapping bounds / shift checks, every buffer the kernels touch has exactly the size
the caller owns or the plan asks the host to reserve and ends flush against an inaccessible page (emu_guarded), so a kernel bug ends the
process that runs it: `run(jobs)` starts `python tests/simt_kzg_verify_child.py IN OUT` with the pickled jobs, under a time limit, and
turns a signal, a time-out or a non-zero exit into a pytest failure that names the job.

A job is a dict with "op" and "label"; one job runs the kernels of one call in the order of the chain, with the stages between them done
here in Python integers (tests/kzg_verify_ref.py: the group-as-scalars model) -- except the finish, whose point arithmetic is real: it
gets [s] G1 from the oracle for the sums the model gives and its pairs come back as affine oracle points.
  verify  log_n, log_l, order, commits, row, col, cells, proofs (scalars), offsets, r, sigma, [chunk], [fault], [finish]
          -> eff, mis, status, rho, rhoa, gathered (the 3 m pairs hold the right points), badidx, agg, [ab (affine triples), bad, verdict, qidx, poff]
  roots   log_n                                                    -> the table winv^(2^b) as ints
  plan    log_n, log_l, m, nseg, [chunk]                           -> ok, chunk, nchunks, bytes
Test infrastructure only: the product never imports this file."""
import ctypes

import numpy as np

import kzg_ref as k
import kzg_verify_ref as v
import simt_harness
from oracle import bls12_381_ref as o

LIB = simt_harness.lib_path("emu_kzg_verify_test")
FAULTS = (1, 2, 3)                                                 # kzg_verify.hip.h KZGV_FAULT
STATUS_BAD = 64                                                    # kzg_verify_plan.h KZGV_STATUS_BAD
R = k.R
FP_ONE = o.fp_to_mont_limbs(1)
FILL = 0xA5A5A5A5A5A5A5A5


def build():
    """build/libemu_kzg_verify_test.so, rebuilt when a source is newer"""
    return simt_harness.build("emu_kzg_verify_test", "emu_kzg_verify.cpp")


def build_fault(n):
    """the same library with seeded fault n (-DKZGV_FAULT=n)"""
    return simt_harness.build("emu_kzg_verify_fault%d_test" % n, "emu_kzg_verify.cpp", defines=("KZGV_FAULT=%d" % n,))


def fault_lib_path(n):
    return simt_harness.lib_path("emu_kzg_verify_fault%d_test" % n)


def run(jobs, timeout=600):
    """the jobs in a fresh child process; returns their results or fails the calling test"""
    return simt_harness.run(__file__, jobs, timeout)


def _fr(vals):
    return np.array([o.fr_to_mont_limbs(int(x) % R) for x in vals], dtype=np.uint64).reshape(-1, 4)


def _ints(limbs):
    """None for limbs that are no canonical scalar: a slot a (faulty) kernel never wrote still holds the fill pattern"""
    rows = [[int(w) for w in row] for row in np.asarray(limbs).reshape(-1, 4)]
    return [o.fr_from_mont_limbs(row) if sum(w << (64 * i) for i, w in enumerate(row)) < R else None for row in rows]


def _model_points(scalars):
    """[s] G1 in the model: an affine wire record whose x carries s and whose y carries a tag; s = 0 is the identity (its flag set)"""
    xy = np.zeros((len(scalars), 12), dtype=np.uint64)
    inf = np.zeros(len(scalars), dtype=np.uint8)
    for i, s in enumerate(scalars):
        if s == 0:
            inf[i] = 1
            continue
        xy[i, 0:4] = [(int(s) >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)]
        xy[i, 6] = 0x7A6
    return xy, inf


def _proj(scalar):
    """[s] G1 as a projective wire point (18 u64); the identity is (0 : 1 : 0)"""
    x, y, inf = o.g1_to_affine(o.g1_mul(o.g1_from_affine(o.G1_GEN), int(scalar) % R))
    if inf:
        return [0] * 6 + FP_ONE + [0] * 6
    return o.fp_to_mont_limbs(x) + o.fp_to_mont_limbs(y) + FP_ONE


def _affine_of(rec):
    """a projective wire point -> the oracle's affine triple"""
    x, y, z = (o.fp_from_mont_limbs([int(w) for w in rec[6 * i:6 * i + 6]]) for i in range(3))
    if z == 0:
        return o.G1_IDENTITY_AFF
    zi = o.fp_inv(z)
    return (x * zi % o.P, y * zi % o.P, False)


# ---- child side --------------------------------------------------------------------------------------------------------------
class _Child(simt_harness.Child):
    def __init__(self):
        simt_harness.Child.__init__(self, LIB)
        self.libs = {0: self.lib}

    def _lib(self, fault):
        if fault not in self.libs:
            lib = ctypes.CDLL(fault_lib_path(fault))
            lib.emu_guarded.restype = ctypes.c_void_p
            lib.emu_guarded.argtypes = [ctypes.c_size_t]
            self.libs[fault] = lib
        lib = self.libs[fault]
        vp, sz, ci, cu = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint
        lib.emu_kzgv_plan.argtypes = [ci, ci, sz, sz, cu, vp]
        lib.emu_kzgv_roots.argtypes = [vp, ci]
        lib.emu_kzgv_offsets.argtypes = [vp, sz, sz, ci, ci, vp, vp, vp, vp, vp, vp]
        lib.emu_kzgv_weights.argtypes = [vp, sz, sz, vp, vp, sz, vp, vp, vp, vp, vp, vp, ci, ci, ci, vp, vp, vp, vp, vp]
        lib.emu_kzgv_cell_copy.argtypes = [vp, vp, sz, ci, ci, ci]
        lib.emu_kzgv_fold.argtypes = [vp, sz, sz, vp, vp, vp, vp, ci, ci, ci, cu, vp, vp]
        lib.emu_kzgv_finish.argtypes = [vp, vp, vp, vp, sz, ci, ci, vp, vp, vp, vp, vp, vp, vp]
        return lib

    def plan(self, j):
        info = (ctypes.c_size_t * 20)()
        self._lib(j.get("fault", 0)).emu_kzgv_plan(j["log_n"], j["log_l"], j["m"], j["nseg"], j.get("chunk", 0), ctypes.cast(info, ctypes.c_void_p))
        names = ("ok", "chunk", "nchunks", "bytes", "eff", "mis", "badidx", "off64", "msm_off", "base_first", "scal", "pxy", "pinf", "cellc", "part", "agg", "ab", "qidx", "poff", "bad")
        return {n: int(info[i]) for i, n in enumerate(names)}

    def roots(self, j):
        tab, ptab = self.buf((j["log_n"] + 1) * 4, dtype=np.uint64, fill=FILL)
        self._lib(0).emu_kzgv_roots(ptab, j["log_n"])
        return {"tab": _ints(tab)}

    def verify(self, j):
        lib = self._lib(j.get("fault", 0))
        log_n, log_l, order, chunk = j["log_n"], j["log_l"], j["order"], j.get("chunk", 0)
        l = 1 << log_l
        offsets, row, col = j["offsets"], j["row"], j["col"]
        nseg, m, ncommit = len(offsets) - 1, len(row), len(j["commits"])
        pl = self.plan({"log_n": log_n, "log_l": log_l, "m": m, "nseg": nseg, "chunk": chunk, "fault": j.get("fault", 0)})
        assert pl["ok"]
        res = {}
        tab, ptab = self.buf((log_n + 1) * 4, dtype=np.uint64, fill=FILL)
        lib.emu_kzgv_roots(ptab, log_n)
        # the offsets
        _, poff = self.buf(nseg + 1, np.array(offsets, dtype=np.uint32))
        eff, peff = self.buf(nseg + 1, fill=0xDEADBEEF)
        mis, pmis = self.buf(nseg + 1, dtype=np.uint8, fill=0xA5)
        off64, poff64 = self.buf(3 * nseg + 1, dtype=np.uint64, fill=FILL)
        msm_off, pmsm_off = self.buf(nseg + 1, fill=0xDEADBEEF)
        bf, pbf = self.buf(nseg, fill=0xDEADBEEF)
        status, pstatus = self.buf(1)
        assert lib.emu_kzgv_offsets(poff, nseg, m, log_n, log_l, peff, pmis, poff64, pmsm_off, pbf, pstatus) == 0
        res["eff"], res["mis"], res["off64"], res["msm_off"], res["base_first"] = eff.tolist(), mis.tolist(), off64.tolist(), msm_off.tolist(), bf.tolist()
        # the weights and the gather
        badidx, pbadidx = self.buf(nseg, dtype=np.uint8)
        cxy, cinf = _model_points(j["commits"])
        pxy_in, pinf_in = _model_points(j["proofs"])
        rho = rhoa = []
        scal = pscal = None
        if m:
            _, prow = self.buf(m, np.array(row, dtype=np.uint32))
            _, pcol = self.buf(m, np.array(col, dtype=np.uint32))
            _, pr = self.buf(nseg * 4, _fr(j["r"]), dtype=np.uint64)
            _, pcxy = self.buf(ncommit * 12, cxy, dtype=np.uint64)
            _, pcinf = self.buf(ncommit, cinf, dtype=np.uint8)
            _, ppxy = self.buf(m * 12, pxy_in, dtype=np.uint64)
            _, ppinf = self.buf(m, pinf_in, dtype=np.uint8)
            scal, pscal = self.buf(3 * m * 4, dtype=np.uint64, fill=FILL)
            gxy, pgxy = self.buf(3 * m * 12, dtype=np.uint64, fill=FILL)
            ginf, pginf = self.buf(3 * m, dtype=np.uint8, fill=0xA5)
            assert lib.emu_kzgv_weights(peff, nseg, m, prow, pcol, ncommit, pr, ptab, pcxy, pcinf, ppxy, ppinf, log_n, log_l, order, pscal, pgxy, pginf, pbadidx, pstatus) == 0
            s3 = _ints(scal)
            rho, rhoa = s3[:m], s3[m:2 * m]
            assert s3[2 * m:] == rho, "the third third does not repeat rho"
            g = gxy.reshape(3, m, 12)
            f = ginf.reshape(3, m)
            ok = np.array_equal(g[0], pxy_in) and np.array_equal(g[1], pxy_in) and np.array_equal(f[0], pinf_in) and np.array_equal(f[1], pinf_in)
            for kk in range(m):
                if row[kk] < ncommit and col[kk] < (2 << (log_n - log_l)):
                    ok = ok and np.array_equal(g[2, kk], cxy[row[kk]]) and f[2, kk] == cinf[row[kk]]
                else:
                    ok = ok and not g[2, kk].any() and f[2, kk] == 1
            res["gathered"] = bool(ok)
        res["rho"], res["rhoa"], res["badidx"], res["status"] = rho, rhoa, badidx.tolist(), int(status[0])
        # the cells in natural coset order, their inverse transforms (here), the fold
        agg, pagg = self.buf(nseg * l * 4, dtype=np.uint64, fill=FILL)
        part, ppart = self.buf(2 * pl["nchunks"] * l * 4, dtype=np.uint64, fill=FILL)      # exactly the records the plan counts
        pcellc = pcol2 = None
        if m:
            _, pcells = self.buf(m * l * 4, _fr([e for c in j["cells"] for e in c]), dtype=np.uint64)
            cellc, pcellc = self.buf(m * l * 4, dtype=np.uint64, fill=FILL)
            assert lib.emu_kzgv_cell_copy(pcells, pcellc, m, log_n, log_l, order) == 0
            nat = np.array(_ints(cellc), dtype=object).reshape(m, l)
            res["natural"] = nat.tolist()
            cellc[:] = _fr([e for rw in nat for e in (o.fr_ntt(list(rw), inverse=True) if log_l else list(rw))]).reshape(-1)
            _, pcol2 = self.buf(m, np.array(col, dtype=np.uint32))
        assert lib.emu_kzgv_fold(peff, nseg, m, pcol2, pscal, pcellc, ptab, log_n, log_l, order, chunk, pagg, ppart) == 0
        res["agg"] = np.array(_ints(agg), dtype=object).reshape(nseg, l).tolist()
        if not j.get("finish"):
            return res
        # the finish on real points: the sums of the thirds and the MSM from the model, [s] G1 from the oracle
        es = res["eff"]
        T = [[sum(x * p for x, p in zip(w[es[s]:es[s + 1]], pts[es[s]:es[s + 1]])) % R for s in range(nseg)]
             for w, pts in ((rho, j["proofs"]), (rhoa, j["proofs"]), (rho, [j["commits"][rw] if rw < ncommit else 0 for rw in row]))]
        M = [sum(a * sg for a, sg in zip(res["agg"][s], j["sigma"])) % R for s in range(nseg)]
        _, psum = self.buf(3 * nseg * 18, np.array([_proj(x) for t in T for x in t], dtype=np.uint64), dtype=np.uint64)
        _, pmsm = self.buf(nseg * 18, np.array([_proj(x) for x in M], dtype=np.uint64), dtype=np.uint64)
        ab, pab = self.buf(2 * nseg * 18, dtype=np.uint64, fill=FILL)
        out_ab, pout_ab = self.buf(2 * nseg * 18, dtype=np.uint64, fill=FILL)
        qidx, pqidx = self.buf(2 * nseg, fill=0xDEADBEEF)
        poffs, ppoffs = self.buf(nseg + 1, dtype=np.uint64, fill=FILL)
        bad, pbad = self.buf(nseg, dtype=np.uint8, fill=0xA5)
        want = [(T[0][s], (T[2][s] + T[1][s] - M[s]) % R) for s in range(nseg)]
        isone = np.array([1 if (a * j["T"] - b_) % R == 0 else 0 for a, b_ in want], dtype=np.uint8)
        _, pisone = self.buf(nseg, isone, dtype=np.uint8)
        verdict, pverdict = self.buf(nseg, dtype=np.uint8, fill=0xA5)
        assert lib.emu_kzgv_finish(psum, pmsm, pmis, pbadidx, nseg, log_n, log_l, pab, pout_ab, pqidx, ppoffs, pbad, pisone, pverdict) == 0
        assert np.array_equal(ab, out_ab), "the caller's pair differs from the chain's"
        res["ab"] = [_affine_of(rec) for rec in ab.reshape(-1, 18)]
        res["bad"], res["verdict"], res["qidx"], res["poff"] = bad.tolist(), verdict.tolist(), qidx.tolist(), poffs.tolist()
        return res


if __name__ == "__main__":
    _Child.main()
