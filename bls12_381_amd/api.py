"""Host-side mirror of the zkcrypto/bls12_381 surface for the accelerated hot path.

Same names, argument meaning and error behaviour as the reference's operator / trait API
(/root/reference/src/lib.rs:49-83): `Scalar`, `G1Affine`, `G1Projective`, `G2Affine`, `G2Projective`, `Gt`,
`MillerLoopResult`, `G2Prepared`, `pairing`, `multi_miller_loop`, `Bls12` -- every group / pairing
operation below is executed by the HIP kernels through the C ABI (include/bls12_381_hip.h).  Values are
carried in the reference's own in-memory format (canonical Montgomery limbs, R = 2^384), as numpy uint64
arrays, so they can be handed to / taken from a Rust caller unchanged.

Only (de)serialisation (big-endian byte encodings, src/notes/serialization.rs) and `Scalar` bookkeeping
run on the host in Python integers; they are format conversion, not part of the compute path.
"""
import contextlib
import ctypes

import numpy as np

from . import _lib
from ._lib import BlsGpuError, check

# ---- curve constants (src/fp.rs:70-77, src/scalar.rs:76-81, src/g1.rs:197-217, src/g2.rs:210-250) ----
P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
_MONT_R = (1 << 384) % P
_MONT_RINV = pow(_MONT_R, -1, P)
_G1X = 0x17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB
_G1Y = 0x08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1
_G2X = (0x024AA2B2F08F0A91260805272DC51051C6E47AD4FA403B02B4510B647AE3D1770BAC0326A805BBEFD48056C8C121BDB8,
        0x13E02B6052719F607DACD3A088274F65596BD0D09920B61AB5DA61BBDC7F5049334CF11213945D57E5AC7D055D042B7E)
_G2Y = (0x0CE5D527727D6E118CC9CDC6DA2E351AADFD9BAA8CBDD3A76D429A695160D12C923AC9CC3BACA289E193548608B82801,
        0x0606C4A02EA734CC32ACD2B02BC28B99CB3E287E85A763AF267492AB572E99AB3F370D275CEC1DA1AAA9075FF05F79BE)


def fp_to_limbs(x):
    """integer in [0,p) -> 6 Montgomery limbs (np.uint64), the reference's `Fp([u64; 6])`"""
    v = (int(x) * _MONT_R) % P
    return np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(6)], dtype=np.uint64)


def limbs_to_fp(l):
    v = 0
    for i, w in enumerate(np.asarray(l, dtype=np.uint64).reshape(-1)[:6]):
        v |= int(w) << (64 * i)
    return (v * _MONT_RINV) % P


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _u64(a, shape):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a.reshape(shape)


def _flags(f, n):
    if f is None:
        return None
    f = np.ascontiguousarray(f, dtype=np.uint8).reshape(-1)
    if f.shape[0] != n:
        raise ValueError("infinity flag array has the wrong length")
    return f


FR_SCAN_SUM, FR_SCAN_PRODUCT, FR_SCAN_HORNER = 0, 1, 2      # include/bls12_381_hip.h: BLSGPU_FR_SCAN_*
FR_FRAC_MAX_COLS, FR_FRAC_TILE = 8, 1024                   # include/bls12_381_hip.h: BLSGPU_FR_FRAC_*
FR_ORDER_NATURAL, FR_ORDER_BITREV = 0, 1                    # include/bls12_381_hip.h: BLSGPU_FR_ORDER_*
KZG_FORM_COEFFS, KZG_FORM_EVALS = 0, 1                      # include/bls12_381_hip.h: BLSGPU_KZG_FORM_*
FR_POSEIDON_AUTO, FR_POSEIDON_DENSE, FR_POSEIDON_SPARSE = 0, 1, 2      # include/bls12_381_hip.h: BLSGPU_FR_POSEIDON_*
FR_EXPR_ADD, FR_EXPR_SUB, FR_EXPR_MUL, FR_EXPR_MAD, FR_EXPR_MOV = 0, 1, 2, 3, 4      # include/bls12_381_hip.h: BLSGPU_FR_EXPR_*
FR_EXPR_MAX_COLS, FR_EXPR_MAX_REGS, FR_EXPR_MAX_CONSTS, FR_EXPR_MAX_INSTR = 32, 8, 32, 256
FR_LOOKUP_LDS_ROWS, FR_LOOKUP_MISS = 4096, 0xFFFFFFFF    # include/bls12_381_hip.h: BLSGPU_FR_LOOKUP_*
FR_GENERATOR = 7                          # scalar.rs:99-105 GENERATOR (`MULTIPLICATIVE_GENERATOR` :708): the usual coset shift


def _coset_limbs(coset):
    """None | Python int in [1, r) | four Montgomery limbs -> four Montgomery limbs (np.uint64) or None"""
    if coset is None:
        return None
    if isinstance(coset, (int, np.integer)):
        g = int(coset)
        if not 0 < g < R_ORDER:
            raise ValueError("coset: an integer shift must be in [1, r)")
        v = (g << 256) % R_ORDER
        return np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
    return _u64(coset, (4,)).copy()


def _point_limbs(points, k, what="fr_scan"):
    """k Python ints in [0, r) | a (k, 4) array of Montgomery limbs -> (k, 4) Montgomery limbs (np.uint64), converted as _coset_limbs does"""
    if isinstance(points, (int, np.integer)):
        points = [points]
    if isinstance(points, (list, tuple)) and all(isinstance(p, (int, np.integer)) for p in points):
        if len(points) != k:
            raise ValueError("%s: one point per row" % what)
        out = np.zeros((k, 4), dtype=np.uint64)
        for i, p in enumerate(points):
            z = int(p)
            if not 0 <= z < R_ORDER:
                raise ValueError("%s: an integer point must be in [0, r)" % what)
            v = (z << 256) % R_ORDER
            out[i] = [(v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)]
        return out
    return _u64(points, (k, 4)).copy()


_R_WORDS = np.frombuffer(R_ORDER.to_bytes(32, "little"), dtype="<u8")
SCALAR_BYTES, SCALAR_MONT = 0, 1          # include/bls12_381_hip.h: BLSGPU_SCALAR_BYTES / BLSGPU_SCALAR_MONT
EXPAND_XMD_SHA256, EXPAND_XMD_SHA512, EXPAND_XOF_SHAKE128, EXPAND_XOF_SHAKE256 = 0, 1, 2, 3      # BLSGPU_EXPAND_*


def scalars_are_canonical(sb):
    """(n,32) uint8 little-endian -> True iff every row is < r (vectorised lexicographic compare, top word first)."""
    w = np.ascontiguousarray(sb).reshape(-1, 32).view("<u8")
    lt = np.zeros(len(w), dtype=bool)
    eq = np.ones(len(w), dtype=bool)
    for k in (3, 2, 1, 0):
        lt |= eq & (w[:, k] < _R_WORDS[k])
        eq &= w[:, k] == _R_WORDS[k]
    return bool(lt.all())


def _builds_bytes(scalars):
    """True when scalars_to_bytes builds the bytes itself (ints / Scalars), False when it passes a raw uint8 array through"""
    return not (isinstance(scalars, np.ndarray) and scalars.dtype == np.uint8)


def scalars_to_bytes(scalars):
    """iterable of ints / Scalars / (n,32) uint8 array -> (n,32) uint8 little-endian canonical (Scalar::to_bytes)"""
    if isinstance(scalars, np.ndarray) and scalars.dtype == np.uint8:
        s = np.ascontiguousarray(scalars).reshape(-1, 32)
        if not scalars_are_canonical(s):
            raise ValueError("scalar bytes are not canonical (>= r): Scalar::from_bytes would return None (scalar.rs:256-280)")
        return s
    out = np.zeros((len(scalars), 32), dtype=np.uint8)
    for i, s in enumerate(scalars):
        v = s.value if isinstance(s, Scalar) else int(s) % R_ORDER
        out[i] = np.frombuffer(v.to_bytes(32, "little"), dtype=np.uint8)
    return out


class ResidentBases:
    """Device-resident base points in the library's internal form (`blsgpu_bases`)."""

    def __init__(self, ctx, handle, group):
        self.ctx, self.handle, self.group = ctx, handle, group

    def __len__(self):
        return int(_lib.load().blsgpu_bases_len(self.handle))

    @property
    def subgroup_state(self):
        """1: every base passed the device-side is_torsion_free (or the set was built as [k]G); 2: assumed by the caller
        (Context.set_assume_subgroup); 0: some base is outside the prime-order subgroup -- the MSM then runs on plain windows
        (exact for every curve point, like the reference's `multiply`, g1.rs:754-774)."""
        return int(_lib.load().blsgpu_bases_subgroup_state(self.handle))

    def precompute(self, window_bits=0):
        """Build resident window-shifted tables (see blsgpu_bases_precompute); later MSMs use them automatically."""
        check(_lib.load().blsgpu_bases_precompute(self.ctx.h, self.handle, window_bits), "bases_precompute")
        return self

    def download(self, first=0, count=None):
        n = len(self) - first if count is None else count
        w = 12 if self.group == 1 else 24
        xy = np.zeros((n, w), dtype=np.uint64)
        inf = np.zeros(n, dtype=np.uint8)
        check(_lib.load().blsgpu_bases_download(self.ctx.h, self.handle, first, n, _ptr(xy), _ptr(inf)), "bases_download")
        return xy, inf

    def free(self):
        if self.handle:
            _lib.load().blsgpu_bases_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class FrMatrix:
    """A CSR matrix over Fr resident on the device (`blsgpu_fr_matrix`): validated and planned once by Context.fr_matrix, multiplied
    many times by Context.fr_spmv."""

    def __init__(self, ctx, handle):
        self.ctx, self.handle = ctx, handle

    def _size(self, fn):
        return int(fn(self.handle)) if self.handle else 0

    @property
    def rows(self):
        return self._size(self.ctx.lib.blsgpu_fr_matrix_rows)

    @property
    def cols(self):
        return self._size(self.ctx.lib.blsgpu_fr_matrix_cols)

    @property
    def nnz(self):
        return self._size(self.ctx.lib.blsgpu_fr_matrix_nnz)

    def close(self):
        if self.handle:
            self.ctx.lib.blsgpu_fr_matrix_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _fr_limbs(values, shape, what):
    """Python ints in [0, r) (nested lists allowed) | an array of Montgomery limbs -> a `shape` + (4,) u64 array of Montgomery limbs"""
    if isinstance(values, np.ndarray):
        return _u64(values, tuple(shape) + (4,)).copy()
    flat = list(values) if isinstance(values, (list, tuple)) else [values]
    while flat and isinstance(flat[0], (list, tuple)):
        flat = [x for row in flat for x in row]
    if all(isinstance(x, (int, np.integer)) for x in flat):
        return _point_limbs(flat, len(flat), what).reshape(tuple(shape) + (4,))
    return _u64(np.array(values, dtype=np.uint64), tuple(shape) + (4,)).copy()


_FR_EXPR_OPS = {"ADD": FR_EXPR_ADD, "SUB": FR_EXPR_SUB, "MUL": FR_EXPR_MUL, "MAD": FR_EXPR_MAD, "MOV": FR_EXPR_MOV}


def fr_expr_operand(x):
    """an operand word of an expression program (BLSGPU_FR_EXPR_REG / _COL / _CONST): a bare int or ("reg", i) is register i,
    ("col", j) or ("col", j, rot) column j rotated by rot rows (a signed 16-bit integer), ("const", i) constant i"""
    if isinstance(x, (int, np.integer)):
        x = ("reg", int(x))
    kind = str(x[0]).lower()
    idx = int(x[1])
    if not 0 <= idx <= 0xFF:
        raise ValueError("fr_expr: an operand index must be in [0, 255]")
    if kind == "reg" and len(x) == 2:
        return idx
    if kind == "col" and len(x) in (2, 3):
        rot = int(x[2]) if len(x) == 3 else 0
        if not -32768 <= rot <= 32767:
            raise ValueError("fr_expr: a rotation must fit a signed 16-bit integer")
        return 0x40000000 | ((rot & 0xFFFF) << 8) | idx
    if kind == "const" and len(x) == 2:
        return 0x80000000 | idx
    raise ValueError("fr_expr: an operand is a register number, (\"reg\", i), (\"col\", j[, rot]) or (\"const\", i)")


def fr_expr_assemble(instrs):
    """tuples like ("MAD", 2, ("col", 3, +1), ("const", 0)) -- (op, dst register, a, b), MOV without b -- -> the (n_instr, 3) u32 code words of
    blsgpu_fr_expr_create.  Only the FORMAT is handled here: the rules (ranges, read-before-write) are checked by the library."""
    code = np.zeros((len(instrs), 3), dtype=np.uint32)
    for i, ins in enumerate(instrs):
        op = _FR_EXPR_OPS.get(str(ins[0]).upper()) if not isinstance(ins[0], (int, np.integer)) else int(ins[0])
        if op is None or len(ins) not in (3, 4) or (len(ins) == 3 and op != FR_EXPR_MOV):
            raise ValueError("fr_expr: instruction %d must be (op, dst, a, b) with op in ADD / SUB / MUL / MAD, or (\"MOV\", dst, a)" % i)
        dst = int(ins[1])
        if not (0 <= op <= 0xFF and 0 <= dst <= 0xFF):
            raise ValueError("fr_expr: instruction %d: op and dst must be in [0, 255]" % i)
        code[i] = (op | (dst << 8), fr_expr_operand(ins[2]), fr_expr_operand(ins[3]) if len(ins) == 4 else 0)
    return code


class FrLookup:
    """A lookup table over Fr resident on the device (`blsgpu_fr_lookup`): an index over rows of c scalars built once by
    Context.fr_lookup; .count gives the logUp multiplicity column, the table row of every looked-up row and the number of misses
    (include/bls12_381_hip.h)."""

    def __init__(self, ctx, handle):
        self.ctx, self.handle = ctx, handle

    def _get(self, fn):
        return int(fn(self.handle)) if self.handle else 0

    @property
    def cols(self):
        return self._get(self.ctx.lib.blsgpu_fr_lookup_cols)

    @property
    def rows(self):
        return self._get(self.ctx.lib.blsgpu_fr_lookup_rows)

    @property
    def distinct(self):
        """the number of different keys among the table's rows"""
        return self._get(self.ctx.lib.blsgpu_fr_lookup_distinct)

    @property
    def slots(self):
        return self._get(self.ctx.lib.blsgpu_fr_lookup_slots)

    def count(self, f, negate=False, return_index=False):
        """f: the looked-up rows as a (c, n, 4) u64 array of Montgomery limbs ((n, 4) for c = 1) or Python ints in [0, r) nested the same
        way.  Returns (mult, missing[, index]): mult the (rows, 4) multiplicities (first-occurrence rule; r - m with negate), missing
        the number of rows of f in no table row, index the (n,) u32 table rows (FR_LOOKUP_MISS for a miss)."""
        v = _fr_lookup_set(f, self.cols, "fr_lookup.count")
        n = v.shape[1]
        mult = np.zeros((self.rows, 4), dtype=np.uint64)
        index = np.zeros(n, dtype=np.uint32) if return_index else None
        missing = np.zeros(1, dtype=np.uint64)
        check(self.ctx.lib.blsgpu_fr_lookup_count(self.ctx.h, self.handle, _ptr(v) if n else None, n, 1 if negate else 0, _ptr(mult), _ptr(index), _ptr(missing)), "fr_lookup_count")
        return (mult, int(missing[0]), index) if return_index else (mult, int(missing[0]))

    def count_device(self, d_f, pitch, n, d_mult=None, d_index=None, d_missing=None, negate=False):
        """the same on rows in device memory (column j at j * pitch scalars): device pointers as ints, any output None; asynchronous on
        the context's stream.  A handle serves one stream at a time."""
        check(self.ctx.lib.blsgpu_fr_lookup_count_device(self.ctx.h, self.handle, d_f, int(pitch), int(n), 1 if negate else 0, d_mult, d_index, d_missing), "fr_lookup_count_device")

    def close(self):
        if self.handle:
            self.ctx.lib.blsgpu_fr_lookup_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class KzgMultiproof:
    """The circulant form of an SRS prefix resident on the device (`blsgpu_kzg_multiproof`), built once by Context.kzg_multiproof_create:
    .proofs gives all 2c cell proofs of many polynomials in one call (include/bls12_381_hip.h)."""

    def __init__(self, ctx, handle):
        self.ctx, self.handle = ctx, handle

    @property
    def log_n(self):
        return int(self.ctx.lib.blsgpu_kzg_multiproof_log_n(self.handle))

    @property
    def log_l(self):
        return int(self.ctx.lib.blsgpu_kzg_multiproof_log_l(self.handle))

    @property
    def cells(self):
        """2c, the number of cells (and proofs) per polynomial"""
        return int(self.ctx.lib.blsgpu_kzg_multiproof_cells(self.handle))

    def proofs(self, polys, form=KZG_FORM_COEFFS, order=FR_ORDER_NATURAL):
        """polys: count polynomials of n scalars as a (count, n, 4) u64 array of Montgomery limbs or Python ints in [0, r) nested the same
        way: coefficients, or (KZG_FORM_EVALS) the values on the domain of fr_bary_* in `order`.  Returns the (count, 2c, 18) projective
        wire points of the proofs, numbered by `order`; compare after batch_normalize."""
        v = _kzg_polys(polys, 1 << self.log_n, "kzg_multiproof.proofs")
        out = np.zeros((v.shape[0], self.cells, 18), dtype=np.uint64)
        check(self.ctx.lib.blsgpu_kzg_multiproof_proofs(self.ctx.h, self.handle, _ptr(v) if v.shape[0] else None, v.shape[0], int(form), int(order),
                                                        _ptr(out) if v.shape[0] else None), "kzg_multiproof_proofs")
        return out

    def proofs_device(self, d_polys, count, d_out_xyz, form=KZG_FORM_COEFFS, order=FR_ORDER_NATURAL):
        """the same on count * n scalars in device memory -> count * 2c wire points in device memory (device pointers as ints, 16-byte
        aligned, no overlap); asynchronous on the context's stream"""
        check(self.ctx.lib.blsgpu_kzg_multiproof_proofs_device(self.ctx.h, self.handle, d_polys, int(count), int(form), int(order), d_out_xyz), "kzg_multiproof_proofs_device")

    def close(self):
        if self.handle:
            self.ctx.lib.blsgpu_kzg_multiproof_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class KzgCellVerifier:
    """A verifier of KZG cell proofs resident on the device (`blsgpu_kzg_cell_verifier`), built once by Context.kzg_cell_verifier_create:
    S[0..l), the `G2Prepared` table {q, -G2} and the powers of w.  .verify decides every batch of (commitment, cell index, cell, proof)
    tuples by one two-term pairing product (include/bls12_381_hip.h)."""

    def __init__(self, ctx, handle):
        self.ctx, self.handle = ctx, handle

    @property
    def log_n(self):
        return int(self.ctx.lib.blsgpu_kzg_cell_verifier_log_n(self.handle))

    @property
    def log_l(self):
        return int(self.ctx.lib.blsgpu_kzg_cell_verifier_log_l(self.handle))

    @property
    def cells(self):
        """2c, the number of cells per polynomial"""
        return int(self.ctx.lib.blsgpu_kzg_cell_verifier_cells(self.handle))

    def verify(self, commit_xy, commit_inf, row, col, cells, proof_xy, proof_inf, offsets, r, order=FR_ORDER_NATURAL, return_ab=False):
        """commit_xy (ncommit, 12) u64 affine wire points with their infinity bytes (None: none is the identity); row / col: m u32 each;
        cells: (m, l, 4) u64 Montgomery limbs or Python ints in [0, r) nested the same way, entries numbered by `order` as kzg_cells
        writes them; proof_xy (m, 12) with proof_inf; offsets: nseg + 1 u32, batch s owns the cells offsets[s] .. offsets[s + 1]; r: nseg
        challenges (limbs or ints).  Returns the nseg verdict bytes, and with return_ab the (nseg, 2, 18) projective wire points
        (A_s, B_s) as well (compare after batch_normalize)."""
        l = 1 << self.log_l
        off = np.ascontiguousarray(offsets, dtype=np.uint32).reshape(-1)
        nseg = max(off.shape[0] - 1, 0)
        m = int(off[-1]) if nseg else 0
        cxy = _u64(commit_xy, (-1, 12)) if commit_xy is not None else np.zeros((0, 12), dtype=np.uint64)
        ncommit = cxy.shape[0]
        cinf = np.zeros(ncommit, dtype=np.uint8) if commit_inf is None else _flags(commit_inf, ncommit)
        rw = np.ascontiguousarray(row, dtype=np.uint32).reshape(-1)
        cl = np.ascontiguousarray(col, dtype=np.uint32).reshape(-1)
        pxy = _u64(proof_xy, (-1, 12)) if m else np.zeros((0, 12), dtype=np.uint64)
        if rw.shape[0] != m or cl.shape[0] != m or pxy.shape[0] != m:
            raise ValueError("kzg_cell_verifier.verify: row, col and proof_xy must hold offsets[-1] entries")
        pinf = np.zeros(m, dtype=np.uint8) if proof_inf is None else _flags(proof_inf, m)
        v = _fr_limbs(cells, (m, l), "kzg_cell_verifier.verify: cells") if m else np.zeros((0, l, 4), dtype=np.uint64)
        ch = _fr_limbs(r, (nseg,), "kzg_cell_verifier.verify: r") if nseg else np.zeros((0, 4), dtype=np.uint64)
        verdict = np.zeros(nseg, dtype=np.uint8)
        ab = np.zeros((nseg, 2, 18), dtype=np.uint64) if return_ab else None
        some = lambda a: _ptr(a) if a.size else None
        check(self.ctx.lib.blsgpu_kzg_verify_cells(self.ctx.h, self.handle, some(cxy), some(cinf), ncommit, some(rw), some(cl), some(v), some(pxy), some(pinf),
                                                   _ptr(off) if nseg else None, nseg, some(ch), int(order), some(verdict), some(ab) if return_ab else None), "kzg_verify_cells")
        return (verdict, ab) if return_ab else verdict

    def verify_device(self, d_commit_xy, d_commit_inf, ncommit, d_row, d_col, d_cells, d_proof_xy, d_proof_inf, d_offsets, nseg, m, d_r, d_verdict, d_out_ab=None,
                      order=FR_ORDER_NATURAL):
        """the same on arrays in device memory (device pointers as ints; scalars 16-byte aligned, points 8-byte, u32 arrays 4-byte; no
        overlap of an output with anything); asynchronous on the context's stream.  A bad index or a broken batch gives that batch verdict 0
        and is reported by the next synchronize."""
        check(self.ctx.lib.blsgpu_kzg_verify_cells_device(self.ctx.h, self.handle, d_commit_xy, d_commit_inf, int(ncommit), d_row, d_col, d_cells, d_proof_xy, d_proof_inf, d_offsets,
                                                          int(nseg), int(m), d_r, int(order), d_verdict, d_out_ab), "kzg_verify_cells_device")

    def close(self):
        if self.handle:
            self.ctx.lib.blsgpu_kzg_cell_verifier_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _kzg_polys(polys, n, what):
    """count polynomials of n scalars -> a contiguous (count, n, 4) u64 array of Montgomery limbs ((n, 4) / a flat list of n ints: count = 1)"""
    if isinstance(polys, np.ndarray):
        v = np.ascontiguousarray(polys, dtype=np.uint64)
        if v.ndim == 2:
            v = v.reshape((1,) + v.shape)
    else:
        rows = list(polys)
        if rows and not isinstance(rows[0], (list, tuple, np.ndarray)):
            rows = [rows]
        v = _fr_limbs(rows, (len(rows), n), what) if rows else np.zeros((0, n, 4), dtype=np.uint64)
    if v.ndim != 3 or v.shape[1] != n or v.shape[2] != 4:
        raise ValueError("%s: expected a (count, %d, 4) array" % (what, n))
    return v


def _fr_lookup_set(values, c, what):
    """a column set of keys -> a contiguous (c, n, 4) u64 array of Montgomery limbs.  c None: taken from the input ((n, 4) / a flat list
    of ints is c = 1)"""
    if isinstance(values, np.ndarray):
        v = np.ascontiguousarray(values, dtype=np.uint64)
        if v.ndim == 2:
            v = v.reshape((1,) + v.shape)
        if v.ndim != 3 or v.shape[2] != 4:
            raise ValueError("%s: expected a (c, n, 4) or (n, 4) array" % what)
    else:
        cols = list(values)
        if not cols or not isinstance(cols[0], (list, tuple)):
            cols = [cols]
        n = len(cols[0])
        if any(len(col) != n for col in cols):
            raise ValueError("%s: the columns differ in length" % what)
        v = _fr_limbs(cols, (len(cols), n), what) if n else np.zeros((len(cols), 0, 4), dtype=np.uint64)
    if c is not None and v.shape[0] != c:
        raise ValueError("%s: expected %d columns" % (what, c))
    return v


class FrExpr:
    """An Fr expression program resident on the device (`blsgpu_fr_expr`): a straight-line program over columns, registers and constants,
    validated once by Context.fr_expr and evaluated per row in one pass (include/bls12_381_hip.h)."""

    def __init__(self, ctx, handle):
        self.ctx, self.handle = ctx, handle

    def _get(self, fn):
        return int(fn(self.handle)) if self.handle else 0

    @property
    def cols(self):
        return self._get(self.ctx.lib.blsgpu_fr_expr_cols)

    @property
    def regs(self):
        return self._get(self.ctx.lib.blsgpu_fr_expr_regs)

    @property
    def instructions(self):
        return self._get(self.ctx.lib.blsgpu_fr_expr_instructions)

    @property
    def products_per_row(self):
        return self._get(self.ctx.lib.blsgpu_fr_expr_products)

    @property
    def cols_read(self):
        """bit j: some instruction reads column j"""
        return self._get(self.ctx.lib.blsgpu_fr_expr_cols_read)

    def _lens(self, col_log_len):
        if col_log_len is None:
            return None
        ll = np.ascontiguousarray(col_log_len, dtype=np.uint8).reshape(-1)
        if ll.shape[0] != self.cols:
            raise ValueError("fr_expr.eval: col_log_len needs one entry per column")
        return ll

    def eval(self, cols, log_n, log_stride=0, col_log_len=None):
        """cols: one entry per column -- an (len, 4) u64 array of Montgomery limbs, a list of Python ints in [0, r), or None for a column
        the program does not read; column j has 2^col_log_len[j] scalars (None: every column has 2^log_n).  Entries that are the SAME
        array object reach the device as one buffer.  Returns the (2^log_n, 4) result."""
        if len(cols) != self.cols:
            raise ValueError("fr_expr.eval: expected %d columns" % self.cols)
        ll = self._lens(col_log_len)
        keep, ptrs = {}, (ctypes.c_void_p * len(cols))()
        for j, c in enumerate(cols):
            if c is None:
                continue
            if id(c) not in keep:
                keep[id(c)] = _fr_limbs(c, (1 << (int(ll[j]) if ll is not None else log_n),), "fr_expr.eval column %d" % j)
            ptrs[j] = keep[id(c)].ctypes.data
        out = np.zeros((1 << log_n, 4), dtype=np.uint64)
        check(self.ctx.lib.blsgpu_fr_expr_eval(self.ctx.h, self.handle, ptrs, _ptr(ll), int(log_n), int(log_stride), _ptr(out)), "fr_expr_eval")
        return out

    def eval_device(self, d_cols, log_n, d_out, log_stride=0, col_log_len=None):
        """the same on columns in device memory: d_cols is one device pointer (an int or None) per column; asynchronous on the context's
        stream, no scratch"""
        if len(d_cols) != self.cols:
            raise ValueError("fr_expr.eval_device: expected %d columns" % self.cols)
        ptrs = (ctypes.c_void_p * len(d_cols))(*[None if p is None else int(p) for p in d_cols])
        check(self.ctx.lib.blsgpu_fr_expr_eval_device(self.ctx.h, self.handle, ptrs, _ptr(self._lens(col_log_len)), int(log_n), int(log_stride), d_out), "fr_expr_eval_device")

    def close(self):
        if self.handle:
            self.ctx.lib.blsgpu_fr_expr_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FrPoseidon:
    """A Poseidon instance over Fr resident on the device (`blsgpu_fr_poseidon`): width, rounds, round constants and matrix are the
    CALLER's (the library ships no standard parameter set), validated and planned once by Context.fr_poseidon.  Scalars go in and come
    out as u64 arrays of Montgomery limbs; Python ints in [0, r) are accepted for inputs and for the tag."""

    def __init__(self, ctx, handle):
        self.ctx, self.handle = ctx, handle

    def _get(self, fn):
        return int(fn(self.handle)) if self.handle else 0

    @property
    def width(self):
        return self._get(self.ctx.lib.blsgpu_fr_poseidon_width)

    @property
    def rounds_full(self):
        return self._get(self.ctx.lib.blsgpu_fr_poseidon_rounds_full)

    @property
    def rounds_partial(self):
        return self._get(self.ctx.lib.blsgpu_fr_poseidon_rounds_partial)

    @property
    def form(self):
        """FR_POSEIDON_DENSE or FR_POSEIDON_SPARSE: the partial rounds the handle runs"""
        return self._get(self.ctx.lib.blsgpu_fr_poseidon_form)

    @property
    def products_per_permutation(self):
        return self._get(self.ctx.lib.blsgpu_fr_poseidon_products)

    def _tag(self, tag):
        return _fr_limbs(tag, (), "fr_poseidon tag")

    def permute(self, states):
        """n states of t scalars ((n, t, 4) limbs or n x t ints) -> the permuted states as a new (n, t, 4) array"""
        v = _fr_limbs(states, (-1, self.width), "fr_poseidon.permute")
        out = np.zeros_like(v)
        check(self.ctx.lib.blsgpu_fr_poseidon_permute(self.ctx.h, self.handle, _ptr(v), v.shape[0], _ptr(out)), "fr_poseidon_permute")
        return out

    def hash_many(self, inputs, tag=0):
        """n preimages of t - 1 scalars -> n digests (n, 4): element 1 of the permutation of (tag, x_1 .. x_(t-1))"""
        v = _fr_limbs(inputs, (-1, self.width - 1), "fr_poseidon.hash_many")
        out = np.zeros((v.shape[0], 4), dtype=np.uint64)
        check(self.ctx.lib.blsgpu_fr_poseidon_hash_many(self.ctx.h, self.handle, _ptr(self._tag(tag)), _ptr(v), v.shape[0], _ptr(out)), "fr_poseidon_hash_many")
        return out

    def merkle(self, leaves, height, k=1, tag=0, with_nodes=True):
        """k trees of (t-1)^height leaves each, tree after tree ((k * a^height, 4) limbs or ints).  Returns (roots (k, 4), nodes): nodes
        holds every inner level, level 1 first and the roots last (None with with_nodes=False)."""
        a = self.width - 1
        v = _fr_limbs(leaves, (k * a ** height,), "fr_poseidon.merkle")
        count = k * height if a == 1 else k * (a ** height - 1) // (a - 1)
        nodes = np.zeros((count, 4), dtype=np.uint64) if with_nodes else None
        roots = np.zeros((k, 4), dtype=np.uint64)
        check(self.ctx.lib.blsgpu_fr_poseidon_merkle(self.ctx.h, self.handle, _ptr(self._tag(tag)), _ptr(v), int(height), int(k), _ptr(nodes), _ptr(roots)), "fr_poseidon_merkle")
        return roots, nodes

    def permute_device(self, d_states, n, d_out):
        """the same on n * t scalars in device memory, asynchronous on the context's stream; d_out == d_states is the in-place form"""
        check(self.ctx.lib.blsgpu_fr_poseidon_permute_device(self.ctx.h, self.handle, d_states, int(n), d_out), "fr_poseidon_permute_device")

    def hash_many_device(self, d_inputs, n, d_out, tag=0):
        """n * (t - 1) scalars at d_inputs -> n digests at d_out; the tag is a host-side parameter"""
        check(self.ctx.lib.blsgpu_fr_poseidon_hash_many_device(self.ctx.h, self.handle, _ptr(self._tag(tag)), d_inputs, int(n), d_out), "fr_poseidon_hash_many_device")

    def merkle_device(self, d_leaves, height, k, d_roots, d_nodes=None, tag=0):
        """k trees over k * (t-1)^height scalars at d_leaves -> k roots at d_roots and, if d_nodes is given, every inner level there"""
        check(self.ctx.lib.blsgpu_fr_poseidon_merkle_device(self.ctx.h, self.handle, _ptr(self._tag(tag)), d_leaves, int(height), int(k), d_nodes, d_roots), "fr_poseidon_merkle_device")

    def close(self):
        if self.handle:
            self.ctx.lib.blsgpu_fr_poseidon_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FrEdwards:
    """A twisted Edwards curve a x^2 + y^2 = 1 + d x^2 y^2 over Fr (`blsgpu_fr_edwards`; Jubjub and Bandersnatch are such curves).  The
    constants are the CALLER's: the library ships no parameter set.  Affine points are (n, 2, 4) u64 arrays of Montgomery limbs (or n
    pairs of Python ints in [0, r)), results (n, 3, 4) arrays (X : Y : Z) whose representative is unspecified: compare after
    normalize.  Scalars are plain 256-bit integers (Python ints or (n, 32) little-endian bytes), NOT Fr elements; `bits` in [1, 256]
    says how many low bits are read.  On a curve that is not `complete` every input point must have odd order."""

    def __init__(self, ctx, handle):
        self.ctx, self.handle = ctx, handle

    @property
    def complete(self):
        """True exactly when a is a square and d is not: the addition law then has no exceptional case at all"""
        return bool(self.ctx.lib.blsgpu_fr_edwards_complete(self.handle)) if self.handle else False

    @staticmethod
    def points(xy, what="fr_edwards"):
        return _fr_limbs(xy, (-1, 2), what)

    @staticmethod
    def scalars(values, what="fr_edwards"):
        """Python ints in [0, 2^256) or an array of 32 little-endian bytes each -> (n, 32) u8"""
        if isinstance(values, np.ndarray):
            return np.ascontiguousarray(values, dtype=np.uint8).reshape(-1, 32)
        vals = [int(v) for v in values]
        if any(v < 0 or v >> 256 for v in vals):
            raise ValueError("%s: a scalar must be in [0, 2^256)" % what)
        return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype=np.uint8).reshape(-1, 32).copy()

    def check(self, xy):
        """ok[i] = 1 iff point i satisfies the curve equation (limbs >= r never do)"""
        v = self.points(xy, "fr_edwards.check")
        ok = np.zeros(v.shape[0], dtype=np.uint8)
        check(self.ctx.lib.blsgpu_fr_edwards_check(self.ctx.h, self.handle, _ptr(v), v.shape[0], _ptr(ok)), "fr_edwards_check")
        return ok

    def normalize(self, xyz):
        """(n, 3, 4) projective points -> ((n, 2, 4) affine points, ok): (0, 1) and ok = 0 where Z = 0"""
        v = _u64(xyz, (-1, 3, 4)).copy()
        xy = np.zeros((v.shape[0], 2, 4), dtype=np.uint64)
        ok = np.zeros(v.shape[0], dtype=np.uint8)
        check(self.ctx.lib.blsgpu_fr_edwards_normalize(self.ctx.h, self.handle, _ptr(v), v.shape[0], _ptr(xy), _ptr(ok)), "fr_edwards_normalize")
        return xy, ok

    def mul_batch(self, xy, scalars, bits=256):
        """out[i] = scalars[i] * P_i for n independent pairs -> (n, 3, 4); the work depends on `bits` alone"""
        v = self.points(xy, "fr_edwards.mul_batch")
        k = self.scalars(scalars, "fr_edwards.mul_batch")
        if k.shape[0] != v.shape[0]:
            raise ValueError("fr_edwards.mul_batch: one scalar per point")
        out = np.zeros((v.shape[0], 3, 4), dtype=np.uint64)
        check(self.ctx.lib.blsgpu_fr_edwards_mul_batch(self.ctx.h, self.handle, _ptr(v), _ptr(k), int(bits), v.shape[0], _ptr(out)), "fr_edwards_mul_batch")
        return out

    def bases(self, xy, bits, window):
        """a fixed-base table for the n bases xy: scalars of `bits` bits, signed windows of `window` in [2, 8] bits -> FrEdwardsBases"""
        v = self.points(xy, "fr_edwards.bases")
        h = ctypes.c_void_p()
        check(self.ctx.lib.blsgpu_fr_edwards_bases_create(self.ctx.h, self.handle, _ptr(v), v.shape[0], int(bits), int(window), ctypes.byref(h)), "fr_edwards_bases_create")
        return FrEdwardsBases(self.ctx, h, int(bits), int(window))

    def bases_from_device(self, d_xy, n, bits, window):
        """the same from n affine points in device memory (16-byte aligned); the table is the handle's own memory"""
        h = ctypes.c_void_p()
        check(self.ctx.lib.blsgpu_fr_edwards_bases_from_device(self.ctx.h, self.handle, d_xy, int(n), int(bits), int(window), ctypes.byref(h)), "fr_edwards_bases_from_device")
        return FrEdwardsBases(self.ctx, h, int(bits), int(window))

    def check_device(self, d_xy, n, d_ok):
        check(self.ctx.lib.blsgpu_fr_edwards_check_device(self.ctx.h, self.handle, d_xy, int(n), d_ok), "fr_edwards_check_device")

    def normalize_device(self, d_xyz, n, d_xy, d_ok=None):
        check(self.ctx.lib.blsgpu_fr_edwards_normalize_device(self.ctx.h, self.handle, d_xyz, int(n), d_xy, d_ok), "fr_edwards_normalize_device")

    def mul_batch_device(self, d_xy, d_scalars, bits, n, d_out_xyz):
        """asynchronous on the context's stream; a scalar above `bits` is reported by the next Context.synchronize"""
        check(self.ctx.lib.blsgpu_fr_edwards_mul_batch_device(self.ctx.h, self.handle, d_xy, d_scalars, int(bits), int(n), d_out_xyz), "fr_edwards_mul_batch_device")

    def close(self):
        if self.handle:
            self.ctx.lib.blsgpu_fr_edwards_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FrEdwardsBases:
    """A fixed-base table on a twisted Edwards curve over Fr (`blsgpu_fr_edwards_bases`): for every base and every signed window the
    2^(window-1) multiples, resident on the device.  msm_segments runs many independent fixed-base MSMs of any length in one call."""

    def __init__(self, ctx, handle, bits, window):
        self.ctx, self.handle, self.bits, self.window = ctx, handle, bits, window

    def __len__(self):
        return int(self.ctx.lib.blsgpu_fr_edwards_bases_len(self.handle)) if self.handle else 0

    def msm_segments(self, offsets, scalars, base_first=None):
        """out[j] = sum_i scalars[offsets[j] + i] * B[base_first[j] + i] (base_first=None: offsets[j]) -> (k, 3, 4); the contract of
        Context.msm_segments with segments of any length"""
        off = np.ascontiguousarray(offsets, dtype=np.uint32).reshape(-1)
        if off.shape[0] < 1:
            raise ValueError("fr_edwards.msm_segments: offsets holds k + 1 values")
        k = off.shape[0] - 1
        bf = None if base_first is None else np.ascontiguousarray(base_first, dtype=np.uint32).reshape(-1)
        if bf is not None and bf.shape[0] != k:
            raise ValueError("fr_edwards.msm_segments: base_first holds k values")
        sc = FrEdwards.scalars(scalars, "fr_edwards.msm_segments")
        if k and sc.shape[0] != int(off[k]):
            raise ValueError("fr_edwards.msm_segments: offsets[k] scalars expected")
        out = np.zeros((k, 3, 4), dtype=np.uint64)
        check(self.ctx.lib.blsgpu_fr_edwards_msm_segments(self.ctx.h, self.handle, _ptr(bf), _ptr(off), _ptr(sc) if sc.shape[0] else None, k, _ptr(out)), "fr_edwards_msm_segments")
        return out

    def msm_segments_device(self, d_offsets, d_scalars, k, total, d_out_xyz, d_base_first=None):
        """asynchronous on the context's stream; a broken segment or a scalar above `bits` is reported by the next Context.synchronize"""
        check(self.ctx.lib.blsgpu_fr_edwards_msm_segments_device(self.ctx.h, self.handle, d_base_first, d_offsets, d_scalars, int(k), int(total), d_out_xyz), "fr_edwards_msm_segments_device")

    def close(self):
        if self.handle:
            self.ctx.lib.blsgpu_fr_edwards_bases_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _term_program(terms):
    """[(coefficient as a Python int in [0, r) or four Montgomery limbs, [table indices]), ...] -> (n_terms, term_ptr u32, term_tab u8, coef (n, 4) u64):
    the term program of include/bls12_381_hip.h (the library validates it)"""
    terms = list(terms)
    ptr, tab = [0], []
    coef = np.zeros((max(len(terms), 1), 4), dtype=np.uint64)
    for t, (c, idx) in enumerate(terms):
        idx = [int(i) for i in idx]
        if any(not 0 <= i < 256 for i in idx):
            raise ValueError("fr_sumcheck: a table index is out of range")
        tab += idx
        ptr.append(len(tab))
        coef[t] = _point_limbs(c if isinstance(c, (int, np.integer)) else np.asarray(c), 1)[0]
    return len(terms), np.array(ptr, dtype=np.uint32), np.array(tab if tab else [0], dtype=np.uint8), coef


def fr_limbs_to_int(limbs):
    """four Montgomery limbs of a canonical Scalar -> the Python int it stands for"""
    v = 0
    for i, w in enumerate(np.asarray(limbs, dtype=np.uint64).reshape(-1)[:4]):
        v |= int(w) << (64 * i)
    return v * pow(1 << 256, -1, R_ORDER) % R_ORDER


class FrSumcheck:
    """A sumcheck in progress (`blsgpu_fr_sumcheck`): the tables live in device memory of the handle's own and are consumed by the rounds.
    Order: round() -> evaluations, round(r_1) ..., while vars_left > 1, then finish(r_m) -> the k values f_j(point)."""

    def __init__(self, ctx, handle, k):
        self.ctx, self.handle, self.k = ctx, handle, k

    @property
    def vars_left(self):
        return int(self.ctx.lib.blsgpu_fr_sumcheck_vars_left(self.handle)) if self.handle else 0

    @property
    def degree(self):
        return int(self.ctx.lib.blsgpu_fr_sumcheck_degree(self.handle)) if self.handle else 0

    def round(self, r_prev=None):
        """the round polynomial's values at 0 .. degree as a (degree + 1, 4) array of Montgomery limbs; r_prev: None in the first round,
        afterwards the previous round's challenge (a Python int in [0, r) or four Montgomery limbs), which is folded in first"""
        out = np.zeros((self.degree + 1, 4), dtype=np.uint64)
        r = None if r_prev is None else _point_limbs(r_prev, 1)
        check(self.ctx.lib.blsgpu_fr_sumcheck_round(self.ctx.h, self.handle, _ptr(r), _ptr(out)), "fr_sumcheck_round")
        return out

    def finish(self, r):
        """binds the last variable at r; returns the (k, 4) values f_j(point), point[b] = the challenge of round m - b"""
        out = np.zeros((self.k, 4), dtype=np.uint64)
        check(self.ctx.lib.blsgpu_fr_sumcheck_finish(self.ctx.h, self.handle, _ptr(_point_limbs(r, 1)), _ptr(out)), "fr_sumcheck_finish")
        return out

    def close(self):
        if self.handle:
            self.ctx.lib.blsgpu_fr_sumcheck_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PreparedG2Table:
    """m `G2Prepared` values resident on the device (`blsgpu_g2_prepared`): the 68 line-coefficient triples of each point
    (pairings.rs:487-546), named by index in the `*_prepared` Miller loops."""

    def __init__(self, ctx, handle):
        self.ctx, self.handle = ctx, handle

    def __len__(self):
        return int(self.ctx.lib.blsgpu_g2_prepared_len(self.handle)) if self.handle else 0

    def coeffs(self, index):
        """(infinity, (68, 3, 12) u64): `G2Prepared { infinity, coeffs }` of point `index` in the reference's value format"""
        out = np.zeros((68, 3, 12), dtype=np.uint64)
        inf = np.zeros(1, dtype=np.uint8)
        check(self.ctx.lib.blsgpu_g2_prepared_coeffs(self.ctx.h, self.handle, index, _ptr(out), _ptr(inf)), "g2_prepared_coeffs")
        return bool(inf[0]), out

    def free(self):
        if self.handle:
            self.ctx.lib.blsgpu_g2_prepared_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


UNPREPARED = 0xffffffff


class Context:
    """One device + one HIP stream + scratch memory (`blsgpu_ctx`).  Not re-entrant."""

    def __init__(self, device=0):
        self.lib = _lib.load()
        h = ctypes.c_void_p()
        check(self.lib.blsgpu_create(device, ctypes.byref(h)), "blsgpu_create")
        self.h = h
        self.device = device
        self.scalar_form = SCALAR_BYTES

    def close(self):
        if getattr(self, "h", None):
            self.lib.blsgpu_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- plumbing ------------------------------------------------------------------------------------
    def set_stream(self, stream_ptr):
        check(self.lib.blsgpu_set_stream(self.h, ctypes.c_void_p(stream_ptr) if stream_ptr else None), "set_stream")

    def synchronize(self):
        check(self.lib.blsgpu_synchronize(self.h), "synchronize")

    def set_pipelining(self, on):
        check(self.lib.blsgpu_set_pipelining(self.h, 1 if on else 0), "set_pipelining")

    def join(self, lag=0):
        check(self.lib.blsgpu_join_lag(self.h, lag), "join")

    def set_msm_window(self, c):
        """Pippenger window width in bits: 0 = automatic, else 4..16.  With the endomorphism split active (subgroup base sets)
        the width applies to the 128-bit (G1) / 64-bit (G2) sub-scalars."""
        check(self.lib.blsgpu_set_msm_window(self.h, c), "set_msm_window")

    def set_assume_subgroup(self, on):
        """Skip the per-upload `is_torsion_free` pass over uploaded bases (the caller vouches that every point is in the
        prime-order subgroup, e.g. values that came from the checked decoders).  Default off: every upload is tested and a
        set with an off-subgroup point falls back to plain windows, which match the reference's `multiply` on any curve point."""
        check(self.lib.blsgpu_set_assume_subgroup(self.h, 1 if on else 0), "set_assume_subgroup")

    def pairing_layout(self, n):
        """which kernels a pairing / Miller-loop / final-exponentiation call with n items runs: 256 = wide (one item per
        workgroup, small batches), 4 = quad, 2 = lane pair (include/bls12_381_hip.h `blsgpu_pairing_layout`)"""
        r = int(self.lib.blsgpu_pairing_layout(self.h, n))
        if r < 0:
            check(r, "pairing_layout")
        return r

    def msm_accumulate_stats(self, enable):
        """(average ms, launches) of the accumulation kernel since the last call (HIP events on its stream); then reset and
        switch the measurement off (False / 0) or on (True / 1: every launch; N: every N-th launch)"""
        avg, cnt = ctypes.c_double(), ctypes.c_uint()
        check(self.lib.blsgpu_msm_accumulate_stats(self.h, int(enable), ctypes.byref(avg), ctypes.byref(cnt)), "msm_accumulate_stats")
        return avg.value, cnt.value

    def kernel_timing(self, on):
        """record the HIP-event duration of every kernel this context launches (blsgpu_kernel_timing); read with kernel_timing_report()"""
        check(self.lib.blsgpu_kernel_timing(self.h, 1 if on else 0), "kernel_timing")

    def kernel_timing_report(self):
        """{kernel name: {"launches", "total_ms", "min_ms", "max_ms"}} in first-launch order; clears the records"""
        buf = ctypes.create_string_buffer(1 << 16)
        need = ctypes.c_size_t(0)
        check(self.lib.blsgpu_kernel_timing_report(self.h, buf, len(buf), ctypes.byref(need)), "kernel_timing_report")
        out = {}
        for line in buf.value.decode().splitlines():
            name, n, tot, mn, mx = line.split("\t")
            out[name] = {"launches": int(n), "total_ms": float(tot), "min_ms": float(mn), "max_ms": float(mx)}
        return out

    def set_profiling(self, on):
        check(self.lib.blsgpu_set_profiling(self.h, 1 if on else 0), "set_profiling")

    def last_msm_phase_ms(self):
        names = ["digits", "scan", "scatter", "order", "accumulate", "reduce", "combine", "total"]
        out = {}
        for i, nm in enumerate(names):
            v = ctypes.c_float()
            check(self.lib.blsgpu_last_msm_phase_ms(self.h, i, ctypes.byref(v)), "last_msm_phase_ms")
            out[nm] = v.value
        return out

    # -- bases -----------------------------------------------------------------------------------------
    def upload_bases(self, group, xy, infinity=None):
        w = 12 if group == 1 else 24
        xy = _u64(xy, (-1, w))
        n = xy.shape[0]
        inf = _flags(infinity, n)
        h = ctypes.c_void_p()
        fn = self.lib.blsgpu_g1_bases_upload if group == 1 else self.lib.blsgpu_g2_bases_upload
        check(fn(self.h, _ptr(xy), _ptr(inf), n, ctypes.byref(h)), "bases_upload")
        return ResidentBases(self, h, group)

    def bases_from_device(self, group, d_xy, d_inf, n):
        h = ctypes.c_void_p()
        fn = self.lib.blsgpu_g1_bases_from_device if group == 1 else self.lib.blsgpu_g2_bases_from_device
        check(fn(self.h, ctypes.c_void_p(d_xy), ctypes.c_void_p(d_inf) if d_inf else None, n, ctypes.byref(h)), "bases_from_device")
        return ResidentBases(self, h, group)

    def bases_from_scalars(self, group, scalars):
        s = scalars_to_bytes(scalars)
        h = ctypes.c_void_p()
        check(self.lib.blsgpu_bases_from_scalars(self.h, group, _ptr(s), s.shape[0], ctypes.byref(h)), "bases_from_scalars")
        return ResidentBases(self, h, group)

    # -- MSM -------------------------------------------------------------------------------------------
    def msm(self, bases, scalars, first=0):
        """sum_i scalars[i] * bases[first+i] -> projective wire limbs (18 or 36 uint64)."""
        s = scalars_to_bytes(scalars)
        n = s.shape[0]
        out = np.zeros(18 if bases.group == 1 else 36, dtype=np.uint64)
        fn = self.lib.blsgpu_g1_msm if bases.group == 1 else self.lib.blsgpu_g2_msm
        with self._bytes_form(_builds_bytes(scalars)):
            check(fn(self.h, bases.handle, first, _ptr(s), n, _ptr(out)), "msm")
        return out

    def msm_device(self, bases, d_scalars, n, d_out, first=0):
        fn = self.lib.blsgpu_g1_msm_device if bases.group == 1 else self.lib.blsgpu_g2_msm_device
        check(fn(self.h, bases.handle, first, ctypes.c_void_p(d_scalars), n, ctypes.c_void_p(d_out)), "msm_device")

    # scalars as the reference stores them: (n, 4) u64 Montgomery limbs of `Scalar([u64; 4])` (scalar.rs:23-27); `to_bytes` runs on the device
    def set_scalar_form(self, form):
        """SCALAR_BYTES (0, default) or SCALAR_MONT (1) for every later scalar argument of this context (blsgpu_set_scalar_form).
        Raw uint8 scalar arrays and device pointers are read in this form; ints and Scalars are always converted to canonical bytes
        and read as such (the wrappers pin SCALAR_BYTES for those calls)."""
        check(self.lib.blsgpu_set_scalar_form(self.h, int(form)), "set_scalar_form")
        self.scalar_form = int(form)

    @contextlib.contextmanager
    def _bytes_form(self, built):
        """SCALAR_BYTES for one call whose scalar bytes the wrapper `built` itself from ints / Scalars; the context's form is restored
        afterwards"""
        if not built or self.scalar_form == SCALAR_BYTES:
            yield
            return
        check(self.lib.blsgpu_set_scalar_form(self.h, SCALAR_BYTES), "set_scalar_form")
        try:
            yield
        finally:
            check(self.lib.blsgpu_set_scalar_form(self.h, self.scalar_form), "set_scalar_form")

    def msm_mont(self, bases, scalar_limbs, first=0):
        """sum_i scalars[i] * bases[first+i] with scalars as (n, 4) u64 Montgomery limbs (`&[Scalar]` memory)."""
        s = _u64(scalar_limbs, (-1, 4))
        out = np.zeros(18 if bases.group == 1 else 36, dtype=np.uint64)
        fn = self.lib.blsgpu_g1_msm_mont if bases.group == 1 else self.lib.blsgpu_g2_msm_mont
        check(fn(self.h, bases.handle, first, _ptr(s), s.shape[0], _ptr(out)), "msm_mont")
        return out

    def msm_mont_device(self, bases, d_scalar_limbs, n, d_out, first=0):
        fn = self.lib.blsgpu_g1_msm_mont_device if bases.group == 1 else self.lib.blsgpu_g2_msm_mont_device
        check(fn(self.h, bases.handle, first, ctypes.c_void_p(d_scalar_limbs), n, ctypes.c_void_p(d_out)), "msm_mont_device")

    def mul_batch_mont(self, group, xy, infinity, scalar_limbs):
        """mul_batch with the scalars as (n, 4) u64 Montgomery limbs"""
        w = 12 if group == 1 else 24
        xy = _u64(xy, (-1, w))
        s = _u64(scalar_limbs, (xy.shape[0], 4))
        inf = _flags(infinity, xy.shape[0])
        out = np.zeros((xy.shape[0], 18 if group == 1 else 36), dtype=np.uint64)
        fn = self.lib.blsgpu_g1_mul_batch_mont if group == 1 else self.lib.blsgpu_g2_mul_batch_mont
        check(fn(self.h, _ptr(xy), _ptr(inf), _ptr(s), xy.shape[0], _ptr(out)), "mul_batch_mont")
        return out

    def mul_batch_mont_device(self, group, d_xy, d_inf, d_scalar_limbs, n, d_out):
        fn = self.lib.blsgpu_g1_mul_batch_mont_device if group == 1 else self.lib.blsgpu_g2_mul_batch_mont_device
        check(fn(self.h, ctypes.c_void_p(d_xy), ctypes.c_void_p(d_inf) if d_inf else None, ctypes.c_void_p(d_scalar_limbs), n, ctypes.c_void_p(d_out)), "mul_batch_mont_device")

    def msm_many(self, bases, scalar_sets):
        """k MSMs over the same resident bases; scalar_sets: (k, n, 32) uint8 (or a list of k scalar lists).  Returns (k, 18|36)."""
        built = False
        if isinstance(scalar_sets, np.ndarray) and scalar_sets.dtype == np.uint8:
            s = np.ascontiguousarray(scalar_sets)
        else:
            s = np.stack([scalars_to_bytes(x) for x in scalar_sets])
            built = any(_builds_bytes(x) for x in scalar_sets)
        k, n = s.shape[0], s.shape[1]
        out = np.zeros((k, 18 if bases.group == 1 else 36), dtype=np.uint64)
        fn = self.lib.blsgpu_g1_msm_many if bases.group == 1 else self.lib.blsgpu_g2_msm_many
        with self._bytes_form(built):
            check(fn(self.h, bases.handle, 0, _ptr(s), n, k, _ptr(out)), "msm_many")
        return out

    def msm_segments(self, bases, scalars, offsets, base_first=None):
        """k independent MSMs in one call (blsgpu_g{1,2}_msm_segments): segment j = scalars[offsets[j]:offsets[j+1]] over
        bases[base_first[j] : base_first[j] + len_j] (base_first None: bases[offsets[j] : offsets[j+1]]).  scalars: ints /
        Scalars / (total, 32) uint8 (`Scalar::to_bytes`); offsets: k + 1 values.  Returns (k, 18|36) uint64 projective limbs."""
        off = np.ascontiguousarray(offsets, dtype=np.uint32).reshape(-1)
        if off.shape[0] < 1:
            raise ValueError("msm_segments: offsets needs k + 1 entries")
        k = off.shape[0] - 1
        s = scalars_to_bytes(scalars) if len(scalars) else np.zeros((0, 32), dtype=np.uint8)
        if s.shape[0] != int(off[-1]):
            raise ValueError("msm_segments: offsets[k] differs from the number of scalars")
        bf = None if base_first is None else np.ascontiguousarray(base_first, dtype=np.uint32).reshape(-1)
        if bf is not None and bf.shape[0] != k:
            raise ValueError("msm_segments: base_first needs k entries")
        out = np.zeros((k, 18 if bases.group == 1 else 36), dtype=np.uint64)
        fn = self.lib.blsgpu_g1_msm_segments if bases.group == 1 else self.lib.blsgpu_g2_msm_segments
        check(fn(self.h, bases.handle, _ptr(bf), _ptr(off), _ptr(s), k, _ptr(out)), "msm_segments")
        return out

    def msm_segments_device(self, bases, d_scalars, d_offsets, k, total, d_out, d_base_first=None):
        """device form of msm_segments: u32 offsets (k + 1) / base_first (k or None), scalars in the context's scalar form and the
        (k, 18|36) u64 result in device memory; enqueued on the context's stream (contract violations: reported by synchronize())"""
        fn = self.lib.blsgpu_g1_msm_segments_device if bases.group == 1 else self.lib.blsgpu_g2_msm_segments_device
        check(fn(self.h, bases.handle, ctypes.c_void_p(d_base_first) if d_base_first else None, ctypes.c_void_p(d_offsets),
                 ctypes.c_void_p(d_scalars) if d_scalars else None, k, total, ctypes.c_void_p(d_out)), "msm_segments_device")

    def msm_bytes(self, group, bases_uncompressed, scalars):
        """MSM on the reference's public encodings: bases = n uncompressed encodings (bytes), scalars = ints / (n,32) bytes;
        returns the uncompressed encoding of the sum."""
        size = 96 if group == 1 else 192
        buf = np.frombuffer(bytes(bases_uncompressed), dtype=np.uint8).copy() if not isinstance(bases_uncompressed, np.ndarray) else np.ascontiguousarray(bases_uncompressed, dtype=np.uint8)
        n = buf.size // size
        s = scalars_to_bytes(scalars)
        if s.shape[0] != n:
            raise ValueError("msm_bytes: bases and scalars differ in length")
        out = np.zeros(size, dtype=np.uint8)
        fn = self.lib.blsgpu_g1_msm_bytes if group == 1 else self.lib.blsgpu_g2_msm_bytes
        check(fn(self.h, _ptr(buf), _ptr(s), n, _ptr(out)), "msm_bytes")
        return out.tobytes()

    def set_bases_cache(self, entries):
        """keep the base arrays of repeated one-shot MSMs (`msm_host`, the mirrored `msm_g1` / `msm_g2`) resident: see blsgpu_set_bases_cache"""
        check(self.lib.blsgpu_set_bases_cache(self.h, int(entries)), "set_bases_cache")

    def set_bases_cache_verify(self, on):
        """recognise cached base arrays by a hash of every word (safe for buffers that are reused with other contents): blsgpu_set_bases_cache_verify"""
        check(self.lib.blsgpu_set_bases_cache_verify(self.h, 1 if on else 0), "set_bases_cache_verify")

    def msm_host(self, group, xy, infinity, scalars):
        w = 12 if group == 1 else 24
        xy = _u64(xy, (-1, w))
        s = scalars_to_bytes(scalars)
        if s.shape[0] != xy.shape[0]:
            raise ValueError("bases and scalars differ in length")
        inf = _flags(infinity, xy.shape[0])
        out = np.zeros(18 if group == 1 else 36, dtype=np.uint64)
        fn = self.lib.blsgpu_g1_msm_host if group == 1 else self.lib.blsgpu_g2_msm_host
        with self._bytes_form(_builds_bytes(scalars)):
            check(fn(self.h, _ptr(xy), _ptr(inf), _ptr(s), xy.shape[0], _ptr(out)), "msm_host")
        return out

    def mul_batch(self, group, xy, infinity, scalars):
        """out[i] = scalars[i] * points[i]: n affine points (n, 12|24) + n scalars -> (n, 18|36) projective wire limbs
        (`&G1Affine * &Scalar` element-wise, g1.rs:573-579 / g2.rs:626-632; exact for every curve point)."""
        w = 12 if group == 1 else 24
        xy = _u64(xy, (-1, w))
        s = scalars_to_bytes(scalars)
        if s.shape[0] != xy.shape[0]:
            raise ValueError("points and scalars differ in length")
        inf = _flags(infinity, xy.shape[0])
        out = np.zeros((xy.shape[0], 18 if group == 1 else 36), dtype=np.uint64)
        fn = self.lib.blsgpu_g1_mul_batch if group == 1 else self.lib.blsgpu_g2_mul_batch
        with self._bytes_form(_builds_bytes(scalars)):
            check(fn(self.h, _ptr(xy), _ptr(inf), _ptr(s), xy.shape[0], _ptr(out)), "mul_batch")
        return out

    def mul_batch_device(self, group, d_xy, d_inf, d_scalars, n, d_out):
        fn = self.lib.blsgpu_g1_mul_batch_device if group == 1 else self.lib.blsgpu_g2_mul_batch_device
        check(fn(self.h, ctypes.c_void_p(d_xy), ctypes.c_void_p(d_inf) if d_inf else None, ctypes.c_void_p(d_scalars), n, ctypes.c_void_p(d_out)), "mul_batch_device")

    # -- group helpers -----------------------------------------------------------------------------------
    def point_sum(self, group, xyz):
        w = 18 if group == 1 else 36
        xyz = _u64(xyz, (-1, w))
        out = np.zeros(w, dtype=np.uint64)
        fn = self.lib.blsgpu_g1_sum if group == 1 else self.lib.blsgpu_g2_sum
        check(fn(self.h, _ptr(xyz), xyz.shape[0], _ptr(out)), "sum")
        return out

    def point_sum_device(self, group, d_xyz, n, d_out):
        fn = self.lib.blsgpu_g1_sum_device if group == 1 else self.lib.blsgpu_g2_sum_device
        check(fn(self.h, ctypes.c_void_p(d_xyz), n, ctypes.c_void_p(d_out)), "sum_device")

    def sum_segments(self, group, xy, infinity, offsets, idx=None):
        """Segmented, gathered sums (blsgpu_g{1,2}_sum_segments): xy (npoints, 12 | 24) u64 affine wire points with their infinity bytes,
        offsets (nseg + 1) u64 in CSR form, idx (offsets[-1],) u32 or None (term t is point t).  -> (nseg, 18 | 36) u64 projective
        points, segment s the sum of the points idx[offsets[s]:offsets[s + 1]]; an empty segment gives the identity."""
        w = 12 if group == 1 else 24
        xy = _u64(xy, (-1, w))
        npoints = xy.shape[0]
        inf = np.zeros(npoints, dtype=np.uint8) if infinity is None else _flags(infinity, npoints)
        off = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
        if off.shape[0] < 1:
            raise ValueError("sum_segments: offsets needs nseg + 1 entries")
        nseg, total = off.shape[0] - 1, int(off[-1])
        ix = None
        if idx is not None:
            ix = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1)
            if ix.shape[0] != total:
                raise ValueError("sum_segments: idx needs offsets[-1] entries")
        out = np.zeros((nseg, 18 if group == 1 else 36), dtype=np.uint64)
        fn = self.lib.blsgpu_g1_sum_segments if group == 1 else self.lib.blsgpu_g2_sum_segments
        check(fn(self.h, _ptr(xy) if npoints else None, _ptr(inf) if npoints else None, npoints, _ptr(ix) if total else None, _ptr(off), nseg, total,
                 _ptr(out) if nseg else None), "sum_segments")
        return out

    def sum_segments_device(self, group, d_xy, d_inf, npoints, d_idx, d_offsets, nseg, total, d_out):
        """device form of sum_segments: asynchronous on the context's stream; an index >= npoints is skipped and reported by synchronize()"""
        fn = self.lib.blsgpu_g1_sum_segments_device if group == 1 else self.lib.blsgpu_g2_sum_segments_device
        vp = lambda p: ctypes.c_void_p(p) if p else None
        check(fn(self.h, vp(d_xy), vp(d_inf), npoints, vp(d_idx), vp(d_offsets), nseg, total, vp(d_out)), "sum_segments_device")

    def batch_normalize(self, group, xyz):
        w = 18 if group == 1 else 36
        xyz = _u64(xyz, (-1, w))
        n = xyz.shape[0]
        xy = np.zeros((n, w * 2 // 3), dtype=np.uint64)
        inf = np.zeros(n, dtype=np.uint8)
        fn = self.lib.blsgpu_g1_batch_normalize if group == 1 else self.lib.blsgpu_g2_batch_normalize
        check(fn(self.h, _ptr(xyz), n, _ptr(xy), _ptr(inf)), "batch_normalize")
        return xy, inf

    def point_op(self, group, op, a, b=None, b_inf=None):
        w = 18 if group == 1 else 36
        a = _u64(a, (-1, w))
        n = a.shape[0]
        if b is not None:
            b = _u64(b, (n, -1))
        out = np.zeros((n, w), dtype=np.uint64)
        check(self.lib.blsgpu_point_op(self.h, group, op, _ptr(a), _ptr(b), _ptr(_flags(b_inf, n)), n, _ptr(out)), "point_op")
        return out

    # -- batched (de)serialisation + validation --------------------------------------------------------------
    def points_from_bytes(self, group, data, compressed=True, checked=True):
        """data: (n, 48|96|192) uint8 or bytes.  Returns (xy, infinity, ok) like `from_compressed` & friends."""
        size = (48 if group == 1 else 96) * (1 if compressed else 2)
        buf = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
        buf = buf.reshape(-1, size)
        n = buf.shape[0]
        xy = np.zeros((n, 12 if group == 1 else 24), dtype=np.uint64)
        inf = np.zeros(n, dtype=np.uint8); ok = np.zeros(n, dtype=np.uint8)
        fn = self.lib.blsgpu_g1_from_bytes_batch if group == 1 else self.lib.blsgpu_g2_from_bytes_batch
        check(fn(self.h, _ptr(buf), n, 1 if compressed else 0, 1 if checked else 0, _ptr(xy), _ptr(inf), _ptr(ok)), "from_bytes_batch")
        return xy, inf, ok

    def points_to_bytes(self, group, xy, infinity=None, compressed=True):
        w = 12 if group == 1 else 24
        xy = _u64(xy, (-1, w))
        n = xy.shape[0]
        size = (48 if group == 1 else 96) * (1 if compressed else 2)
        out = np.zeros((n, size), dtype=np.uint8)
        fn = self.lib.blsgpu_g1_to_bytes_batch if group == 1 else self.lib.blsgpu_g2_to_bytes_batch
        check(fn(self.h, _ptr(xy), _ptr(_flags(infinity, n)), n, 1 if compressed else 0, _ptr(out)), "to_bytes_batch")
        return out

    # -- field self-test hooks ---------------------------------------------------------------------------
    def _elem_op(self, fn, words, op, a, b):
        a = _u64(a, (-1, words))
        if b is not None:
            b = _u64(b, (a.shape[0], words))
        out = np.zeros_like(a)
        check(fn(self.h, op, _ptr(a), _ptr(b), a.shape[0], _ptr(out)), "field op")
        return out

    def fp_op(self, op, a, b=None):
        return self._elem_op(self.lib.blsgpu_fp_op, 6, op, a, b)

    def fp2_op(self, op, a, b=None):
        return self._elem_op(self.lib.blsgpu_fp2_op, 12, op, a, b)

    def fp6_op(self, op, a, b=None):
        return self._elem_op(self.lib.blsgpu_fp6_op, 36, op, a, b)

    def fp12_op(self, op, a, b=None):
        return self._elem_op(self.lib.blsgpu_fp12_op, 72, op, a, b)

    # ---- hash-to-curve (reference: src/hash_to_curve/) ----
    def hash_to_curve(self, group, msgs, dst, encode_only=False):
        """`G::hash_to_curve(msg, dst)` (or `encode_to_curve`) with ExpandMsgXmd<Sha256> for a list of byte strings;
        returns (n, 18 | 36) u64 projective points in the reference's limbs."""
        msgs = [bytes(m) for m in msgs]
        n = len(msgs)
        offs = np.zeros(n + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64) if n else 0
        blob = np.frombuffer(b"".join(msgs) + b"\0", dtype=np.uint8).copy()
        d = np.frombuffer(bytes(dst) + b"\0", dtype=np.uint8).copy()
        out = np.zeros((n, 18 if group == 1 else 36), dtype=np.uint64)
        fn = self.lib.blsgpu_g1_hash_to_curve_batch if group == 1 else self.lib.blsgpu_g2_hash_to_curve_batch
        check(fn(self.h, _ptr(blob), _ptr(offs), n, _ptr(d), len(dst), 1 if encode_only else 0, _ptr(out)), "hash_to_curve")
        return out

    @staticmethod
    def _msgs(msgs, dst):
        msgs = [bytes(m) for m in msgs]
        offs = np.zeros(len(msgs) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64) if msgs else 0
        blob = np.frombuffer(b"".join(msgs) + b"\0", dtype=np.uint8).copy()
        d = np.frombuffer(bytes(dst) + b"\0", dtype=np.uint8).copy()
        return len(msgs), blob, offs, d

    def hash_to_curve_expander(self, group, expander, msgs, dst, encode_only=False):
        """`hash_to_curve::<X>` / `encode_to_curve::<X>` with X chosen by `expander` (EXPAND_XMD_SHA256 / _XMD_SHA512 / _XOF_SHAKE128 / _XOF_SHAKE256:
        expand_msg.rs:167-328); returns (n, 18 | 36) u64 projective points"""
        n, blob, offs, d = self._msgs(msgs, dst)
        out = np.zeros((n, 18 if group == 1 else 36), dtype=np.uint64)
        check(self.lib.blsgpu_hash_to_curve_expander_batch(self.h, group, int(expander), _ptr(blob), _ptr(offs), n, _ptr(d), len(dst), 1 if encode_only else 0, _ptr(out)), "hash_to_curve_expander")
        return out

    def hash_to_curve_from_uniform(self, group, uniform, encode_only=False):
        """the part of hash_to_curve behind the expander (mod.rs:86-108): `uniform` = (n, count * M * 64) bytes per message (count = 1 | 2, M = 1 for G1,
        2 for G2) -> from_okm -> map_to_curve -> sum -> clear_h; returns (n, 18 | 36) u64 projective points"""
        per = (1 if encode_only else 2) * (1 if group == 1 else 2) * 64
        u = np.ascontiguousarray(np.asarray(uniform, dtype=np.uint8)).reshape(-1, per)
        out = np.zeros((u.shape[0], 18 if group == 1 else 36), dtype=np.uint64)
        check(self.lib.blsgpu_hash_to_curve_from_uniform_batch(self.h, group, _ptr(u), u.shape[0], 1 if encode_only else 0, _ptr(out)), "hash_to_curve_from_uniform")
        return out

    def expand_message(self, expander, msgs, dst, len_in_bytes):
        """`ExpandMessage::init_expand` + reading all the bytes: (n, len_in_bytes) uint8"""
        n, blob, offs, d = self._msgs(msgs, dst)
        out = np.zeros((n, len_in_bytes), dtype=np.uint8)
        check(self.lib.blsgpu_expand_message_batch(self.h, int(expander), _ptr(blob), _ptr(offs), n, _ptr(d), len(dst), len_in_bytes, _ptr(out)), "expand_message")
        return out

    def hash_to_scalar(self, expander, msgs, dst, count=1):
        """`hash_to_field::<X, Scalar>` (mod.rs:32-49, map_scalar.rs:10-25): (n, count, 4) u64 Montgomery limbs"""
        n, blob, offs, d = self._msgs(msgs, dst)
        out = np.zeros((n, count, 4), dtype=np.uint64)
        check(self.lib.blsgpu_hash_to_scalar_batch(self.h, int(expander), _ptr(blob), _ptr(offs), n, _ptr(d), len(dst), count, _ptr(out)), "hash_to_scalar")
        return out

    # ---- scalar field Fr (reference: src/scalar.rs) ----
    def fr_op(self, op, a, b=None, return_flags=False):
        """element-wise Scalar arithmetic on (n, 4) u64 Montgomery limbs; op 0 mul, 1 add, 2 sub, 3 square, 4 invert,
        5 neg, 6 double.  For invert, return_flags also returns the `is_some` bytes (0 where the input was zero)."""
        a = _u64(a, (-1, 4))
        if b is not None:
            b = _u64(b, (a.shape[0], 4))
        out = np.zeros_like(a)
        flags = np.ones(a.shape[0], dtype=np.uint8)
        check(self.lib.blsgpu_fr_op(self.h, op, _ptr(a), _ptr(b), a.shape[0], _ptr(out), _ptr(flags)), "fr_op")
        return (out, flags) if return_flags else out

    def fr_op_device(self, op, d_a, d_b, n, d_out, d_flags=None):
        """fr_op on n scalars in device memory (d_b: None for the unary ops), asynchronous on the context's stream"""
        check(self.lib.blsgpu_fr_op_device(self.h, int(op), d_a, d_b, n, d_out, d_flags), "fr_op_device")

    def fr_ntt(self, values, inverse=False):
        """radix-2 transform of 2^k Scalars ((n, 4) u64 Montgomery limbs), natural order in and out; see
        include/bls12_381_hip.h for the definition."""
        v = _u64(values, (-1, 4)).copy()
        n = v.shape[0]
        if n == 0 or n & (n - 1):
            raise ValueError("fr_ntt: length must be a power of two")
        check(self.lib.blsgpu_fr_ntt(self.h, _ptr(v), n.bit_length() - 1, 1 if inverse else 0), "fr_ntt")
        return v

    def fr_ntt_device(self, d_ptr, log_n, inverse=False):
        check(self.lib.blsgpu_fr_ntt_device(self.h, d_ptr, log_n, 1 if inverse else 0), "fr_ntt_device")

    def fr_ntt_many(self, values, inverse=False, coset=None):
        """k independent transforms in one call: `values` is a (k, n, 4) u64 array of Montgomery limbs, n a power of two; returns a new
        array.  coset: None, or the shift g as a Python int in [1, r) or four Montgomery limbs (FR_GENERATOR = 7 is the reference's):
        forward gives the values on g * <w>, inverse takes them back (include/bls12_381_hip.h)."""
        v = np.array(values, dtype=np.uint64)
        if v.ndim != 3 or v.shape[2] != 4:
            raise ValueError("fr_ntt_many: expected a (k, n, 4) array")
        k, n = v.shape[0], v.shape[1]
        if k and (n == 0 or n & (n - 1)):
            raise ValueError("fr_ntt_many: the vector length must be a power of two")
        v = np.ascontiguousarray(v)
        check(self.lib.blsgpu_fr_ntt_many(self.h, _ptr(v), max(n.bit_length() - 1, 0), k, 1 if inverse else 0, _ptr(_coset_limbs(coset))), "fr_ntt_many")
        return v

    def fr_ntt_many_device(self, d_ptr, log_n, k, inverse=False, coset=None):
        """the same on k * 2^log_n scalars in device memory, in place, asynchronous on the context's stream (`coset` stays a host value)"""
        check(self.lib.blsgpu_fr_ntt_many_device(self.h, d_ptr, log_n, k, 1 if inverse else 0, _ptr(_coset_limbs(coset))), "fr_ntt_many_device")

    def fr_scan(self, op, values, points=None, exclusive=False):
        """recurrences along k rows in one call (include/bls12_381_hip.h): `values` is a (k, len, 4) u64 array of Montgomery limbs (a
        (len, 4) array is k = 1), op FR_SCAN_SUM / FR_SCAN_PRODUCT (inclusive, or exclusive) or FR_SCAN_HORNER: row v = the coefficients
        of p_v, points[v] = z (Python ints in [0, r) or a (k, 4) array of Montgomery limbs) -> out[v][0] = p_v(z), out[v][1:] = the
        quotient (p_v(X) - p_v(z)) / (X - z).  Returns a new array of the same shape."""
        v = np.ascontiguousarray(np.array(values, dtype=np.uint64))
        one = v.ndim == 2
        if one:
            v = v.reshape((1,) + v.shape)
        if v.ndim != 3 or v.shape[2] != 4:
            raise ValueError("fr_scan: expected a (k, len, 4) or (len, 4) array")
        if op not in (FR_SCAN_SUM, FR_SCAN_PRODUCT, FR_SCAN_HORNER):
            raise ValueError("fr_scan: unknown op")
        k, n = v.shape[0], v.shape[1]
        pts = None
        if op == FR_SCAN_HORNER:
            if exclusive:
                raise ValueError("fr_scan: exclusive is not defined for HORNER")
            if points is None:
                raise ValueError("fr_scan: HORNER needs one point per row")
            pts = _point_limbs(points, k)
        out = np.zeros_like(v)
        check(self.lib.blsgpu_fr_scan_many(self.h, int(op), 1 if exclusive else 0, _ptr(v), n, k, _ptr(pts), _ptr(out)), "fr_scan")
        return out[0] if one else out

    def fr_scan_device(self, op, d_in, length, k, d_out, d_points=None, exclusive=False):
        """the same on k * length scalars in device memory (d_points: k scalars in device memory for HORNER), d_out == d_in allowed,
        asynchronous on the context's stream"""
        check(self.lib.blsgpu_fr_scan_many_device(self.h, int(op), 1 if exclusive else 0, d_in, length, k, d_points, d_out), "fr_scan_device")

    def fr_batch_invert(self, values, return_flags=False):
        """element-wise inverses of an (n, 4) u64 array of Montgomery limbs by Montgomery's trick: limb-identical to fr_op(4, ...), 0 for a
        zero; return_flags also returns the `is_some` bytes (0 where the input was zero)"""
        a = _u64(values, (-1, 4))
        out = np.zeros_like(a)
        flags = np.ones(a.shape[0], dtype=np.uint8)
        check(self.lib.blsgpu_fr_batch_invert(self.h, _ptr(a), a.shape[0], _ptr(out), _ptr(flags)), "fr_batch_invert")
        return (out, flags) if return_flags else out

    def fr_batch_invert_device(self, d_in, n, d_out, d_flags=None):
        check(self.lib.blsgpu_fr_batch_invert_device(self.h, d_in, n, d_out, d_flags), "fr_batch_invert_device")

    def _fr_ids(self, v, n, what):
        """n scalars as (n, 4) u64 Montgomery limbs: such an array as it is, or integers (participant ids) through fr_from_bytes"""
        if isinstance(v, np.ndarray) and v.dtype == np.uint64 and v.ndim == 2 and v.shape[1] == 4:
            a = np.ascontiguousarray(v)
        else:
            ints = [int(x) for x in np.asarray(v, dtype=object).reshape(-1)]
            if any(x < 0 or x >= (1 << 256) for x in ints):
                raise ValueError("%s: an integer does not fit 32 bytes" % what)
            raw = np.frombuffer(b"".join(x.to_bytes(32, "little") for x in ints), dtype=np.uint8).reshape(-1, 32)
            a, ok = self.fr_from_bytes(raw) if ints else (np.zeros((0, 4), dtype=np.uint64), np.ones(0, dtype=np.uint8))
            if not ok.all():
                raise ValueError("%s: an integer is not below r" % what)
        if a.shape[0] != n:
            raise ValueError("%s: expected %d scalars" % (what, n))
        return a

    @staticmethod
    def _lagrange_offsets(offsets, what):
        off = np.ascontiguousarray(offsets, dtype=np.uint32).reshape(-1)
        if off.shape[0] < 1:
            raise ValueError("%s: offsets needs nseg + 1 entries" % what)
        return off, off.shape[0] - 1, int(off[-1])

    def fr_lagrange_segments(self, nodes, offsets, points=None, values=None, want_lambda=True, want_y=None):
        """Lagrange coefficients at arbitrary nodes (blsgpu_fr_lagrange_segments): nodes (total, 4) u64 Montgomery limbs or integers
        (participant ids), offsets (nseg + 1) u32 in CSR form, points nseg scalars (limbs or integers) or None (every z = 0), values like
        nodes or None.  -> (lambda (total, 4) or None, y (nseg, 4) or None, distinct flags (nseg,) u8): lambda_i = prod_{j != i}
        (z - x_j) * inv0(prod_{j != i} (x_i - x_j)), y[s] = sum lambda_i values_i; want_y defaults to `values is not None`."""
        off, nseg, total = self._lagrange_offsets(offsets, "fr_lagrange_segments")
        x = self._fr_ids(nodes, total, "fr_lagrange_segments: nodes")
        z = None if points is None else self._fr_ids(points, nseg, "fr_lagrange_segments: points")
        v = None if values is None else self._fr_ids(values, total, "fr_lagrange_segments: values")
        if want_y is None:
            want_y = values is not None
        lam = np.zeros((total, 4), dtype=np.uint64) if want_lambda else None
        y = np.zeros((nseg, 4), dtype=np.uint64) if want_y else None
        flags = np.ones(nseg, dtype=np.uint8)
        check(self.lib.blsgpu_fr_lagrange_segments(self.h, _ptr(x) if total else None, _ptr(off), nseg, _ptr(z), _ptr(v) if total else None, _ptr(lam), _ptr(y),
                                                   _ptr(flags) if nseg else None), "fr_lagrange_segments")
        return lam, y, flags

    def fr_lagrange_segments_device(self, d_nodes, d_offsets, nseg, total, d_points=None, d_values=None, d_lambda=None, d_y=None, d_flags=None):
        """device form: asynchronous on the context's stream; a segment that breaks the offsets contract writes nothing and is reported
        by synchronize()"""
        vp = lambda p: ctypes.c_void_p(p) if p else None
        check(self.lib.blsgpu_fr_lagrange_segments_device(self.h, vp(d_nodes), vp(d_offsets), nseg, total, vp(d_points), vp(d_values), vp(d_lambda), vp(d_y), vp(d_flags)),
              "fr_lagrange_segments_device")

    def lagrange_combine(self, group, xy, infinity, nodes, offsets, points=None):
        """Interpolation in the exponent (blsgpu_g{1,2}_lagrange_combine): xy (total, 12 | 24) u64 affine wire shares with their infinity
        bytes, nodes / offsets / points as for fr_lagrange_segments.  -> ((nseg, 18 | 36) u64 projective points, segment s the sum of
        lambda_i * share_i, and the distinct flags)."""
        w = 12 if group == 1 else 24
        off, nseg, total = self._lagrange_offsets(offsets, "lagrange_combine")
        xy = _u64(xy, (-1, w))
        if xy.shape[0] != total:
            raise ValueError("lagrange_combine: expected offsets[-1] shares")
        inf = np.zeros(total, dtype=np.uint8) if infinity is None else _flags(infinity, total)
        x = self._fr_ids(nodes, total, "lagrange_combine: nodes")
        z = None if points is None else self._fr_ids(points, nseg, "lagrange_combine: points")
        out = np.zeros((nseg, 18 if group == 1 else 36), dtype=np.uint64)
        flags = np.ones(nseg, dtype=np.uint8)
        fn = self.lib.blsgpu_g1_lagrange_combine if group == 1 else self.lib.blsgpu_g2_lagrange_combine
        check(fn(self.h, _ptr(xy) if total else None, _ptr(inf) if total else None, _ptr(x) if total else None, _ptr(off), nseg, _ptr(z), _ptr(out) if nseg else None,
                 _ptr(flags) if nseg else None), "lagrange_combine")
        return out, flags

    def lagrange_combine_device(self, group, d_xy, d_inf, d_nodes, d_offsets, nseg, total, d_points, d_out, d_flags=None):
        """device form of lagrange_combine: three stages on the context's stream, no synchronisation"""
        fn = self.lib.blsgpu_g1_lagrange_combine_device if group == 1 else self.lib.blsgpu_g2_lagrange_combine_device
        vp = lambda p: ctypes.c_void_p(p) if p else None
        check(fn(self.h, vp(d_xy), vp(d_inf), vp(d_nodes), vp(d_offsets), nseg, total, vp(d_points), vp(d_out), vp(d_flags)), "lagrange_combine_device")

    @staticmethod
    def _frac_set(what, name, s, shape=None):
        """a column set as a contiguous (c, k, len, 4) u64 array (a (c, len, 4) array is k = 1); None stays None"""
        if s is None:
            return None
        v = np.ascontiguousarray(np.array(s, dtype=np.uint64))
        if v.ndim == 3:
            v = v.reshape((v.shape[0], 1) + v.shape[1:])
        if v.ndim != 4 or v.shape[3] != 4:
            raise ValueError("%s: %s must be a (c, k, len, 4) or (c, len, 4) array" % (what, name))
        if shape is not None and v.shape != shape:
            raise ValueError("%s: %s has shape %s, expected %s" % (what, name, v.shape, shape))
        return v

    def fr_grand_product(self, num_a, num_b, den_a, den_b, beta, gamma, exclusive=False, return_flags=False):
        """the accumulator column of a permutation argument in one call (include/bls12_381_hip.h): column sets of shape (c, k, len, 4) u64
        Montgomery limbs ((c, len, 4) is k = 1), c in [1, 8]; num_b / den_b may be None (no beta term); beta, gamma: Python ints in
        [0, r) or (4,) limb arrays.  f[i] = prod_j (num_a_j + beta num_b_j + gamma)[i] * inv0(prod_j (den_a_j + beta den_b_j + gamma)[i]),
        out = the PRODUCT scan of f along each row (exclusive: out[v][0] = 1).  Returns a (k, len, 4) array ((len, 4) for k = 1 input);
        return_flags also returns the (k, len) bytes that are 0 where a denominator factor was zero."""
        what = "fr_grand_product"
        one = np.ndim(num_a) == 3
        na = self._frac_set(what, "num_a", num_a)
        if na is None:
            raise ValueError("fr_grand_product: num_a is required")
        da = na if den_a is num_a else self._frac_set(what, "den_a", den_a, na.shape)
        if da is None:
            raise ValueError("fr_grand_product: den_a is required")
        nb, db = self._frac_set(what, "num_b", num_b, na.shape), self._frac_set(what, "den_b", den_b, na.shape)
        c, k, n = na.shape[:3]
        out = np.zeros((k, n, 4), dtype=np.uint64)
        flags = np.ones((k, n), dtype=np.uint8)
        check(self.lib.blsgpu_fr_grand_product(self.h, 1 if exclusive else 0, c, _ptr(na), _ptr(nb), _ptr(da), _ptr(db), _ptr(_point_limbs([beta, gamma], 2)), n, k,
                                               _ptr(out), _ptr(flags)), what)
        if one:
            out, flags = out[0], flags[0]
        return (out, flags) if return_flags else out

    def fr_grand_product_device(self, c, d_num_a, d_num_b, d_den_a, d_den_b, pitch, d_challenges, length, k, d_out, d_flags=None, exclusive=False):
        """the same on column sets in device memory (table j of a set at + j * pitch scalars; d_num_b / d_den_b may be None),
        d_challenges = (beta, gamma) in DEVICE memory, asynchronous on the context's stream"""
        check(self.lib.blsgpu_fr_grand_product_device(self.h, 1 if exclusive else 0, c, d_num_a, d_num_b, d_den_a, d_den_b, pitch, d_challenges, length, k, d_out, d_flags),
              "fr_grand_product_device")

    def fr_frac_sum(self, mult, den_a, den_b, beta, gamma, exclusive=False, return_flags=False):
        """the accumulator column of a log-derivative lookup argument in one call: f[i] = sum_j mult_j[i] * inv0(gamma + den_a_j[i] + beta
        den_b_j[i]), out = the SUM scan of f along each row.  Shapes and challenges as fr_grand_product; mult None: every multiplicity
        is 1 (signs belong in mult); den_b None: no beta term."""
        what = "fr_frac_sum"
        one = np.ndim(den_a) == 3
        da = self._frac_set(what, "den_a", den_a)
        if da is None:
            raise ValueError("fr_frac_sum: den_a is required")
        m, db = self._frac_set(what, "mult", mult, da.shape), self._frac_set(what, "den_b", den_b, da.shape)
        c, k, n = da.shape[:3]
        out = np.zeros((k, n, 4), dtype=np.uint64)
        flags = np.ones((k, n), dtype=np.uint8)
        check(self.lib.blsgpu_fr_frac_sum(self.h, 1 if exclusive else 0, c, _ptr(m), _ptr(da), _ptr(db), _ptr(_point_limbs([beta, gamma], 2)), n, k, _ptr(out), _ptr(flags)), what)
        if one:
            out, flags = out[0], flags[0]
        return (out, flags) if return_flags else out

    def fr_frac_sum_device(self, c, d_mult, d_den_a, d_den_b, pitch, d_challenges, length, k, d_out, d_flags=None, exclusive=False):
        """the same on column sets in device memory (d_mult / d_den_b may be None), asynchronous on the context's stream"""
        check(self.lib.blsgpu_fr_frac_sum_device(self.h, 1 if exclusive else 0, c, d_mult, d_den_a, d_den_b, pitch, d_challenges, length, k, d_out, d_flags), "fr_frac_sum_device")

    def _fr_bary_args(self, what, evals, points):
        v = np.ascontiguousarray(np.array(evals, dtype=np.uint64))
        one = v.ndim == 2
        if one:
            v = v.reshape((1,) + v.shape)
        if v.ndim != 3 or v.shape[2] != 4:
            raise ValueError("%s: expected a (k, n, 4) or (n, 4) array" % what)
        k, n = v.shape[0], v.shape[1]
        if n == 0 or n & (n - 1):
            raise ValueError("%s: the row length must be a power of two" % what)
        return v, one, k, n.bit_length() - 1, _point_limbs(points, k, what)

    def fr_bary_eval(self, evals, points, order=FR_ORDER_NATURAL):
        """polynomials in evaluation form (include/bls12_381_hip.h: blsgpu_fr_bary_eval_many): `evals` is a (k, n, 4) u64 array of
        Montgomery limbs (an (n, 4) array is k = 1), row v = p_v on the n-th roots of unity in natural (FR_ORDER_NATURAL) or bit-reversed
        (FR_ORDER_BITREV) order, points[v] = z_v (Python ints in [0, r) or a (k, 4) array of Montgomery limbs, as fr_scan takes them).
        Returns y = p_v(z_v) as a (k, 4) array ((4,) for k = 1 given as (n, 4)); a point inside the domain is handled exactly."""
        v, one, k, log_n, pts = self._fr_bary_args("fr_bary_eval", evals, points)
        y = np.zeros((k, 4), dtype=np.uint64)
        check(self.lib.blsgpu_fr_bary_eval_many(self.h, _ptr(v), log_n, k, _ptr(pts), int(order), _ptr(y)), "fr_bary_eval")
        return y[0] if one else y

    def fr_bary_open(self, evals, points, order=FR_ORDER_NATURAL):
        """as fr_bary_eval, and the evaluations q of the quotient (p_v(X) - y_v) / (X - z_v) on the same domain in the same order (the
        scalars of a KZG proof over a Lagrange SRS).  Returns (y, q), q of the shape of `evals`."""
        v, one, k, log_n, pts = self._fr_bary_args("fr_bary_open", evals, points)
        y = np.zeros((k, 4), dtype=np.uint64)
        q = np.zeros_like(v)
        check(self.lib.blsgpu_fr_bary_open_many(self.h, _ptr(v), log_n, k, _ptr(pts), int(order), _ptr(y), _ptr(q)), "fr_bary_open")
        return (y[0], q[0]) if one else (y, q)

    def fr_bary_eval_device(self, d_evals, log_n, k, d_points, d_y, order=FR_ORDER_NATURAL):
        """the same on k * 2^log_n scalars in device memory (d_points, d_y: k scalars), asynchronous on the context's stream"""
        check(self.lib.blsgpu_fr_bary_eval_many_device(self.h, d_evals, log_n, k, d_points, int(order), d_y), "fr_bary_eval_device")

    def fr_bary_open_device(self, d_evals, log_n, k, d_points, d_y, d_q, order=FR_ORDER_NATURAL):
        """the same with the quotient written to d_q (k * 2^log_n scalars, no overlap with the inputs: there is no in-place form)"""
        check(self.lib.blsgpu_fr_bary_open_many_device(self.h, d_evals, log_n, k, d_points, int(order), d_y, d_q), "fr_bary_open_device")

    def fr_poseidon(self, t, r_full, r_partial, constants, mds, form=FR_POSEIDON_AUTO):
        """a Poseidon instance made resident (include/bls12_381_hip.h: blsgpu_fr_poseidon_create): width t in {2, 3, 4, 5, 9, 12}, r_full
        (even) full and r_partial partial rounds, constants[(r_full + r_partial)][t] and the t x t matrix mds as Python ints in [0, r) or
        arrays of Montgomery limbs.  The parameters are the caller's: the library ships no standard set
        (bls12_381_amd.synthetic.poseidon_test_params makes seeded TEST parameters).  form=FR_POSEIDON_AUTO takes the sparse partial
        rounds when they can be derived, FR_POSEIDON_DENSE the textbook ones.  Returns an FrPoseidon."""
        rc = _fr_limbs(constants, (-1,), "fr_poseidon constants")
        mm = _fr_limbs(mds, (-1,), "fr_poseidon mds")
        t, r_full, r_partial = int(t), int(r_full), int(r_partial)
        if t < 1 or r_full < 0 or r_partial < 0 or rc.shape[0] != (r_full + r_partial) * t or mm.shape[0] != t * t:
            raise ValueError("fr_poseidon: expected (r_full + r_partial) * t round constants and t * t matrix entries")
        h = ctypes.c_void_p()
        check(self.lib.blsgpu_fr_poseidon_create(self.h, t, r_full, r_partial, _ptr(rc), _ptr(mm), int(form), ctypes.byref(h)), "fr_poseidon")
        return FrPoseidon(self, h)

    def fr_edwards(self, a, d):
        """a twisted Edwards curve a x^2 + y^2 = 1 + d x^2 y^2 over Fr (include/bls12_381_hip.h: blsgpu_fr_edwards_create): a and d as
        Python ints in [0, r) or Montgomery limbs, the caller's (the library ships no parameter set).  a = 0, d = 0 and a = d are refused.
        Returns an FrEdwards (.complete, .check, .normalize, .mul_batch, .bases -> FrEdwardsBases.msm_segments)."""
        aa = _fr_limbs(a, (), "fr_edwards a")
        dd = _fr_limbs(d, (), "fr_edwards d")
        h = ctypes.c_void_p()
        check(self.lib.blsgpu_fr_edwards_create(self.h, _ptr(aa), _ptr(dd), ctypes.byref(h)), "fr_edwards")
        return FrEdwards(self, h)

    def fr_lookup(self, table):
        """a lookup table made resident (include/bls12_381_hip.h: blsgpu_fr_lookup_create): `table` is a (c, rows, 4) u64 array of
        Montgomery limbs ((rows, 4) for c = 1) or Python ints in [0, r) nested the same way; a key is a row of c scalars.  Returns an
        FrLookup (.count, .count_device, .rows / .cols / .distinct / .slots, .close())."""
        t = _fr_lookup_set(table, None, "fr_lookup")
        h = ctypes.c_void_p()
        check(self.lib.blsgpu_fr_lookup_create(self.h, t.shape[0], _ptr(t), t.shape[1], ctypes.byref(h)), "fr_lookup")
        return FrLookup(self, h)

    def fr_lookup_from_device(self, c, d_table, pitch, rows):
        """the same from c columns in device memory (column j at j * pitch scalars); the handle keeps its own copy"""
        h = ctypes.c_void_p()
        check(self.lib.blsgpu_fr_lookup_from_device(self.h, int(c), d_table, int(pitch), int(rows), ctypes.byref(h)), "fr_lookup_from_device")
        return FrLookup(self, h)

    def fr_expr(self, n_cols, n_regs, consts, instrs):
        """an expression program made resident (include/bls12_381_hip.h: blsgpu_fr_expr_create): n_cols columns, n_regs registers, consts
        as Python ints in [0, r) or an (n, 4) array of Montgomery limbs (None or empty: none), instrs either tuples for fr_expr_assemble
        or an (n_instr, 3) u32 array of code words.  The program is validated here, once; a bad one raises with the instruction index
        and the rule.  Returns an FrExpr (.eval, .eval_device, .close())."""
        code = np.ascontiguousarray(instrs, dtype=np.uint32).reshape(-1, 3) if isinstance(instrs, np.ndarray) else fr_expr_assemble(list(instrs))
        cs = None
        if consts is not None and len(consts):
            cs = _fr_limbs(consts, (-1,), "fr_expr consts")
        h = ctypes.c_void_p()
        check(self.lib.blsgpu_fr_expr_create(self.h, int(n_cols), int(n_regs), 0 if cs is None else cs.shape[0], _ptr(cs), code.shape[0], _ptr(code), ctypes.byref(h)), "fr_expr")
        return FrExpr(self, h)

    def fr_matrix(self, row_ptr, col, val, n_cols):
        """a CSR matrix made resident (include/bls12_381_hip.h: blsgpu_fr_matrix_upload): row_ptr has n_rows + 1 entries from 0 to
        nnz = len(col), non-decreasing; col[p] < n_cols; val is nnz Python ints in [0, r) or an (nnz, 4) u64 array of Montgomery limbs
        (accepted as fr_scan's points are).  Columns inside a row may repeat (they add) and come in any order; rows may be empty.  The
        whole structure is validated here, once; a bad matrix raises.  Returns an FrMatrix (.rows, .cols, .nnz, .close())."""
        rp = np.ascontiguousarray(row_ptr, dtype=np.uint32).reshape(-1)
        cl = np.ascontiguousarray(col, dtype=np.uint32).reshape(-1)
        if rp.shape[0] < 1:
            raise ValueError("fr_matrix: row_ptr needs n_rows + 1 entries")
        if int(rp[-1]) != cl.shape[0]:
            raise ValueError("fr_matrix: row_ptr[n_rows] must equal the number of non-zeros len(col)")
        vl = _point_limbs(list(val) if isinstance(val, (list, tuple)) else val, cl.shape[0]) if cl.shape[0] else np.zeros((0, 4), dtype=np.uint64)
        h = ctypes.c_void_p()
        check(self.lib.blsgpu_fr_matrix_upload(self.h, rp.shape[0] - 1, int(n_cols), _ptr(rp), _ptr(cl), _ptr(vl), ctypes.byref(h)), "fr_matrix")
        return FrMatrix(self, h)

    def fr_matrix_from_device(self, d_row_ptr, d_col, d_val, n_rows, n_cols):
        """the same from arrays already in device memory (u32 row_ptr / col, four u64 limbs per value; d_val 16-byte aligned): validated by a
        kernel, copied into the handle's own buffers -- the caller's are free again on return"""
        h = ctypes.c_void_p()
        check(self.lib.blsgpu_fr_matrix_from_device(self.h, int(n_rows), int(n_cols), d_row_ptr, d_col, d_val, ctypes.byref(h)), "fr_matrix_from_device")
        return FrMatrix(self, h)

    def fr_spmv(self, m, x):
        """out[v][i] = sum_p val[p] x[v][col[p]] over row i's entries: x is a (k, n_cols, 4) u64 array of Montgomery limbs ((n_cols, 4) is
        k = 1) -> a new (k, n_rows, 4) (or (n_rows, 4)) array.  Stack A, B and C into one matrix of 3n rows to apply all three in one call."""
        v = np.ascontiguousarray(np.array(x, dtype=np.uint64))
        one = v.ndim == 2
        if one:
            v = v.reshape((1,) + v.shape)
        if v.ndim != 3 or v.shape[2] != 4 or v.shape[1] != m.cols:
            raise ValueError("fr_spmv: expected a (k, n_cols, 4) or (n_cols, 4) array")
        out = np.zeros((v.shape[0], m.rows, 4), dtype=np.uint64)
        check(self.lib.blsgpu_fr_spmv(self.h, m.handle, _ptr(v), v.shape[0], _ptr(out)), "fr_spmv")
        return out[0] if one else out

    def fr_spmv_device(self, m, d_x, k, d_out):
        """the same on k * n_cols scalars in device memory -> k * n_rows scalars at d_out (no overlap with d_x), asynchronous on the
        context's stream"""
        check(self.lib.blsgpu_fr_spmv_device(self.h, m.handle, d_x, k, d_out), "fr_spmv_device")

    @staticmethod
    def _mle_tables(values, what):
        """(k, 2^m, 4) or (2^m, 4) Montgomery limbs -> (array (k, 2^m, 4), m, was a single table)"""
        v = np.ascontiguousarray(np.array(values, dtype=np.uint64))
        one = v.ndim == 2
        if one:
            v = v.reshape((1,) + v.shape)
        if v.ndim != 3 or v.shape[2] != 4:
            raise ValueError(what + ": expected a (k, 2^m, 4) or (2^m, 4) array")
        n = v.shape[1]
        if v.shape[0] and (n == 0 or n & (n - 1)):
            raise ValueError(what + ": the table length must be a power of two")
        return v, max(n.bit_length() - 1, 0), one

    def fr_mle_fold(self, tables, r):
        """binds the TOP variable of k multilinear tables at r (include/bls12_381_hip.h): `tables` is a (k, 2^m, 4) u64 array of
        Montgomery limbs ((2^m, 4) is k = 1), m >= 1, r a Python int in [0, r) or four Montgomery limbs -> a new (k, 2^(m-1), 4) array,
        out[j][i] = f_j[i] + r (f_j[i + 2^(m-1)] - f_j[i])"""
        v, m, one = self._mle_tables(tables, "fr_mle_fold")
        out = np.zeros((v.shape[0], v.shape[1] // 2, 4), dtype=np.uint64)
        check(self.lib.blsgpu_fr_mle_fold(self.h, _ptr(v), m, v.shape[0], _ptr(_point_limbs(r, 1)), _ptr(out)), "fr_mle_fold")
        return out[0] if one else out

    def fr_mle_fold_device(self, d_in, pitch_in, m, k, d_r, d_out, pitch_out):
        """the same on k tables of 2^m scalars in device memory, table j at j * pitch scalars; d_r: one scalar in device memory;
        d_out == d_in with equal pitches folds in place; asynchronous on the context's stream"""
        check(self.lib.blsgpu_fr_mle_fold_device(self.h, d_in, pitch_in, m, k, d_r, d_out, pitch_out), "fr_mle_fold_device")

    def fr_eq_table(self, point):
        """the table eq(point)[i] = prod_b (bit b of i ? point[b] : 1 - point[b]) as a (2^m, 4) array of Montgomery limbs; point: m Python
        ints in [0, r) or an (m, 4) array of Montgomery limbs (m = 0: the table [1])"""
        m = len(point)
        pts = _point_limbs(list(point) if isinstance(point, (list, tuple)) else point, m) if m else None
        out = np.zeros((1 << m, 4), dtype=np.uint64)
        check(self.lib.blsgpu_fr_eq_table(self.h, _ptr(pts), m, _ptr(out)), "fr_eq_table")
        return out

    def fr_eq_table_device(self, d_point, m, d_out):
        """the same from m scalars in device memory into 2^m scalars at d_out, asynchronous on the context's stream"""
        check(self.lib.blsgpu_fr_eq_table_device(self.h, d_point, m, d_out), "fr_eq_table_device")

    def fr_mle_eval(self, tables, point):
        """f_j(point) for k multilinear tables ((k, 2^m, 4) or (2^m, 4) Montgomery limbs), point[b] the value of x_b (m Python ints or an
        (m, 4) array) -> (k, 4) (or (4,)) Montgomery limbs"""
        v, m, one = self._mle_tables(tables, "fr_mle_eval")
        if len(point) != m:
            raise ValueError("fr_mle_eval: the point needs one coordinate per variable")
        pts = _point_limbs(list(point) if isinstance(point, (list, tuple)) else point, m) if m else None
        out = np.zeros((v.shape[0], 4), dtype=np.uint64)
        check(self.lib.blsgpu_fr_mle_eval(self.h, _ptr(v), m, v.shape[0], _ptr(pts), _ptr(out)), "fr_mle_eval")
        return out[0] if one else out

    def fr_mle_eval_device(self, d_tables, pitch, m, k, d_point, d_out):
        """the same on tables in device memory (not written) -> k scalars at d_out, asynchronous on the context's stream"""
        check(self.lib.blsgpu_fr_mle_eval_device(self.h, d_tables, pitch, m, k, d_point, d_out), "fr_mle_eval_device")

    def fr_sumcheck_round_device(self, d_tables, pitch, m, k, terms, d_evals, d_r_prev=None):
        """one round polynomial of sum_x sum_t coef_t prod_e f_e(x) over k tables in device memory: terms is a list of
        (coefficient, [table indices]); d_evals receives degree + 1 scalars.  With d_r_prev (one scalar in device memory) the tables are
        first folded at it IN PLACE and the evaluations are those of the folded tables (include/bls12_381_hip.h).  Asynchronous."""
        n, ptr, tab, coef = _term_program(terms)
        check(self.lib.blsgpu_fr_sumcheck_round_device(self.h, d_tables, pitch, m, k, n, _ptr(ptr), _ptr(tab), _ptr(coef), d_r_prev, d_evals), "fr_sumcheck_round_device")

    def fr_sumcheck(self, tables, terms):
        """begins a sumcheck over k tables ((k, 2^m, 4) Montgomery limbs, copied to the device) and the summand
        sum_t coef_t prod_e f_e: terms is a list of (coefficient as a Python int in [0, r) or four Montgomery limbs, [table indices]).
        Returns an FrSumcheck (.round(r_prev=None), .finish(r), .vars_left, .degree, .close())."""
        v, m, _ = self._mle_tables(tables, "fr_sumcheck")
        n, ptr, tab, coef = _term_program(terms)
        h = ctypes.c_void_p()
        check(self.lib.blsgpu_fr_sumcheck_begin(self.h, _ptr(v), m, v.shape[0], n, _ptr(ptr), _ptr(tab), _ptr(coef), ctypes.byref(h)), "fr_sumcheck")
        return FrSumcheck(self, h, v.shape[0])

    def fr_sumcheck_device(self, d_tables, pitch, m, k, terms):
        """the same from k tables of 2^m scalars in device memory, table j at j * pitch scalars (copied: the caller's stay as they are)"""
        n, ptr, tab, coef = _term_program(terms)
        h = ctypes.c_void_p()
        check(self.lib.blsgpu_fr_sumcheck_begin_device(self.h, d_tables, pitch, m, k, n, _ptr(ptr), _ptr(tab), _ptr(coef), ctypes.byref(h)), "fr_sumcheck_device")
        return FrSumcheck(self, h, k)

    def fr_sumcheck_prove(self, tables, terms, challenge):
        """drives every round of a sumcheck: challenge(round_index, evals_as_ints) -> int is called with round_index = 1 .. m and that
        round's evaluations at 0 .. degree as Python ints, and returns the round's challenge.  Returns (round_evals, point, values):
        the list of per-round evaluation lists, the point with point[b] the value of x_b, and the (k, 4) Montgomery limbs f_j(point)."""
        return self._sumcheck_drive(self.fr_sumcheck(tables, terms), challenge)

    @staticmethod
    def _sumcheck_drive(sc, challenge):
        try:
            m = sc.vars_left
            rounds, chal, r = [], [], None
            for s in range(1, m + 1):
                ev = [fr_limbs_to_int(e) for e in sc.round(r)]
                rounds.append(ev)
                r = int(challenge(s, ev)) % R_ORDER
                chal.append(r)
            values = sc.finish(r)
            return rounds, chal[::-1], values
        finally:
            sc.close()

    def g_ntt_many(self, group, points, inverse=False):
        """k independent radix-2 transforms over GROUP elements in one call (include/bls12_381_hip.h: Y[m] = sum_j [w^(jm)] P[j], the w of
        fr_ntt; the inverse turns a monomial SRS into its Lagrange form).  `points` is a (k, n, 18 | 36) u64 array of projective wire
        points, or a pair (xy, infinity) of (k, n, 12 | 24) affine coordinates and (k, n) flags, lifted here to Z = 1 / Z = 0; n a power
        of two.  Every point must lie in the prime-order subgroup.  Returns a new (k, n, 18 | 36) array."""
        w = 18 if group == 1 else 36
        c = w // 3
        if isinstance(points, tuple):
            xy, inf = points
            xy = np.asarray(xy, dtype=np.uint64)
            if xy.ndim != 3 or xy.shape[2] != 2 * c:
                raise ValueError("g_ntt_many: expected (k, n, %d) affine coordinates" % (2 * c))
            flags = np.zeros(xy.shape[:2], dtype=bool) if inf is None else np.asarray(inf).astype(bool)
            if flags.shape != xy.shape[:2]:
                raise ValueError("g_ntt_many: the infinity flags must be a (k, n) array")
            v = np.zeros(xy.shape[:2] + (w,), dtype=np.uint64)
            v[:, :, :2 * c] = xy
            v[:, :, 2 * c:2 * c + 6] = fp_to_limbs(1)
            v[flags] = 0
            v[flags, c:c + 6] = fp_to_limbs(1)                   # (0 : 1 : 0)
        else:
            v = np.array(points, dtype=np.uint64)
            if v.ndim != 3 or v.shape[2] != w:
                raise ValueError("g_ntt_many: expected a (k, n, %d) array" % w)
        k, n = v.shape[0], v.shape[1]
        if k and (n == 0 or n & (n - 1)):
            raise ValueError("g_ntt_many: the vector length must be a power of two")
        v = np.ascontiguousarray(v)
        fn = self.lib.blsgpu_g1_ntt_many if group == 1 else self.lib.blsgpu_g2_ntt_many
        check(fn(self.h, _ptr(v), max(n.bit_length() - 1, 0), k, 1 if inverse else 0), "g_ntt_many")
        return v

    def g_ntt_many_device(self, group, d_ptr, log_n, k, inverse=False):
        """the same on k * 2^log_n projective wire points in device memory (16-byte aligned), in place, asynchronous on the context's stream:
        mul_batch_device -> g_ntt_many_device -> batch_normalize_device -> bases_from_device needs no host copy"""
        fn = self.lib.blsgpu_g1_ntt_many_device if group == 1 else self.lib.blsgpu_g2_ntt_many_device
        check(fn(self.h, ctypes.c_void_p(d_ptr) if d_ptr else None, log_n, k, 1 if inverse else 0), "g_ntt_many_device")

    def kzg_multiproof_create(self, srs_g1, log_n, log_l):
        """amortised KZG openings (include/bls12_381_hip.h): the handle for polynomials of 2^log_n coefficients opened on cosets of
        2^log_l points over the first 2^log_n points of the resident G1 bases `srs_g1`.  A setup call; the handle keeps no reference to
        the SRS."""
        h = ctypes.c_void_p()
        check(self.lib.blsgpu_kzg_multiproof_create(self.h, srs_g1.handle if srs_g1 is not None else None, int(log_n), int(log_l), ctypes.byref(h)), "kzg_multiproof_create")
        return KzgMultiproof(self, h)

    def kzg_cell_verifier_create(self, srs_g1, log_n, log_l, q_xy, q_inf=False):
        """batched verification of KZG cell proofs (include/bls12_381_hip.h): the handle for cells of 2^log_l points of polynomials of
        2^log_n coefficients over the first 2^log_l points of the resident G1 bases `srs_g1` and the affine G2 wire point q (24 u64),
        meant as [tau^l] G2; the caller vouches that q is in the subgroup.  A setup call; the handle keeps no reference to the SRS."""
        q = _u64(q_xy, (24,)) if q_xy is not None else None
        qi = np.array([1 if q_inf else 0], dtype=np.uint8)
        h = ctypes.c_void_p()
        check(self.lib.blsgpu_kzg_cell_verifier_create(self.h, srs_g1.handle if srs_g1 is not None else None, int(log_n), int(log_l), _ptr(q), _ptr(qi), ctypes.byref(h)),
              "kzg_cell_verifier_create")
        return KzgCellVerifier(self, h)

    def kzg_cells(self, polys, log_l, form=KZG_FORM_COEFFS, order=FR_ORDER_NATURAL):
        """the 2c cells of l = 2^log_l evaluations of every polynomial: polys as for KzgMultiproof.proofs (n a power of two); returns a
        (count, 2c, l, 4) array of Montgomery limbs, cells numbered by `order`"""
        if isinstance(polys, np.ndarray):
            n = polys.shape[-2]
        else:
            rows = list(polys)
            n = len(rows[0]) if rows and isinstance(rows[0], (list, tuple, np.ndarray)) else len(rows)
        if n == 0 or n & (n - 1):
            raise ValueError("kzg_cells: the number of scalars per polynomial must be a power of two")
        v = _kzg_polys(polys, n, "kzg_cells")
        log_n = n.bit_length() - 1
        if not 0 <= log_l <= log_n:
            raise ValueError("kzg_cells: log_l must be in [0, log_n]")
        out = np.zeros((v.shape[0], 2 * (n >> log_l), 1 << log_l, 4), dtype=np.uint64)
        check(self.lib.blsgpu_kzg_cells(self.h, _ptr(v) if v.shape[0] else None, log_n, int(log_l), v.shape[0], int(form), int(order), _ptr(out) if v.shape[0] else None), "kzg_cells")
        return out

    def kzg_cells_device(self, d_polys, log_n, log_l, count, d_cells, form=KZG_FORM_COEFFS, order=FR_ORDER_NATURAL):
        """the same on count * 2^log_n scalars in device memory -> count * 2^(log_n + 1) scalars (16-byte aligned, no overlap);
        asynchronous on the context's stream"""
        check(self.lib.blsgpu_kzg_cells_device(self.h, d_polys, int(log_n), int(log_l), int(count), int(form), int(order), d_cells), "kzg_cells_device")

    def kzg_recover(self, col, offsets, cells, log_n, log_l, order=FR_ORDER_NATURAL, want_polys=True, want_cells=False):
        """polynomials rebuilt from c or more of their 2c cells (include/bls12_381_hip.h): offsets: count + 1 u32, polynomial v owns the
        received cells offsets[v] .. offsets[v + 1]; col: m u32 cell numbers in `order`; cells: (m, l, 4) u64 Montgomery limbs or Python
        ints in [0, r) nested the same way, entries numbered as kzg_cells writes them.  Returns (polys, out_cells, ok): the (count, n, 4)
        coefficients (None without want_polys), the (count, 2c, l, 4) cells of the recovered polynomials (None without want_cells) and
        the count ok bytes; a polynomial with ok = 0 (inconsistent cells) has zero rows."""
        n, l = 1 << log_n, 1 << log_l
        off = np.ascontiguousarray(offsets, dtype=np.uint32).reshape(-1)
        count = max(off.shape[0] - 1, 0)
        m = int(off[-1]) if count else 0
        cl = np.ascontiguousarray(col, dtype=np.uint32).reshape(-1)
        if cl.shape[0] != m:
            raise ValueError("kzg_recover: col must hold offsets[-1] entries")
        v = _fr_limbs(cells, (m, l), "kzg_recover: cells") if m else np.zeros((0, l, 4), dtype=np.uint64)
        polys = np.zeros((count, n, 4), dtype=np.uint64) if want_polys else None
        out = np.zeros((count, 2 * (n >> log_l), l, 4), dtype=np.uint64) if want_cells else None
        ok = np.zeros(count, dtype=np.uint8)
        some = lambda a: _ptr(a) if a is not None and a.size else None
        check(self.lib.blsgpu_kzg_recover(self.h, some(cl), _ptr(off) if count else None, count, some(v), int(log_n), int(log_l), int(order), some(polys), some(out), some(ok)),
              "kzg_recover")
        return polys, out, ok

    def kzg_recover_device(self, d_col, d_offsets, count, m, d_cells, log_n, log_l, d_polys, d_out_cells, d_ok, order=FR_ORDER_NATURAL):
        """the same on arrays in device memory (device pointers as ints; scalars 16-byte aligned, u32 arrays 4-byte; no overlap of an output
        with anything; d_polys or d_out_cells may be None); asynchronous on the context's stream.  A malformed polynomial (a bad or
        duplicate cell number, fewer than c cells, broken offsets) gets ok = 0 and is reported by the next synchronize."""
        check(self.lib.blsgpu_kzg_recover_device(self.h, d_col, d_offsets, int(count), int(m), d_cells, int(log_n), int(log_l), int(order), d_polys, d_out_cells, d_ok),
              "kzg_recover_device")

    def fr_to_bytes(self, limbs, return_flags=False):
        """`Scalar::to_bytes` (scalar.rs:284-296) over (n, 4) u64 Montgomery limbs -> (n, 32) uint8; flags: limbs below r"""
        a = _u64(limbs, (-1, 4))
        out = np.zeros((a.shape[0], 32), dtype=np.uint8)
        ok = np.ones(a.shape[0], dtype=np.uint8)
        check(self.lib.blsgpu_fr_to_bytes(self.h, _ptr(a), a.shape[0], _ptr(out), _ptr(ok)), "fr_to_bytes")
        return (out, ok) if return_flags else out

    def fr_from_bytes(self, data):
        """`Scalar::from_bytes` (scalar.rs:256-280) over (n, 32) uint8 -> ((n, 4) u64 Montgomery limbs, is_some bytes)"""
        b = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data, dtype=np.uint8).reshape(-1, 32)
        out = np.zeros((b.shape[0], 4), dtype=np.uint64)
        ok = np.ones(b.shape[0], dtype=np.uint8)
        check(self.lib.blsgpu_fr_from_bytes(self.h, _ptr(b), b.shape[0], _ptr(out), _ptr(ok)), "fr_from_bytes")
        return out, ok

    def fr_from_bytes_wide(self, data):
        """`Scalar::from_bytes_wide` (scalar.rs:300-331) over (n, 64) uint8 -> (n, 4) u64 Montgomery limbs"""
        b = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data, dtype=np.uint8).reshape(-1, 64)
        out = np.zeros((b.shape[0], 4), dtype=np.uint64)
        check(self.lib.blsgpu_fr_from_bytes_wide(self.h, _ptr(b), b.shape[0], _ptr(out)), "fr_from_bytes_wide")
        return out

    def fr_to_bytes_device(self, d_limbs, n, d_bytes, d_ok=None):
        check(self.lib.blsgpu_fr_to_bytes_device(self.h, ctypes.c_void_p(d_limbs), n, ctypes.c_void_p(d_bytes), ctypes.c_void_p(d_ok) if d_ok else None), "fr_to_bytes_device")

    def fr_from_bytes_device(self, d_bytes, n, d_limbs, d_ok=None):
        check(self.lib.blsgpu_fr_from_bytes_device(self.h, ctypes.c_void_p(d_bytes), n, ctypes.c_void_p(d_limbs), ctypes.c_void_p(d_ok) if d_ok else None), "fr_from_bytes_device")

    def fr_from_bytes_wide_device(self, d_bytes, n, d_limbs):
        check(self.lib.blsgpu_fr_from_bytes_wide_device(self.h, ctypes.c_void_p(d_bytes), n, ctypes.c_void_p(d_limbs)), "fr_from_bytes_wide_device")

    def fp_mul_throughput(self, iters=2000):
        v = ctypes.c_double()
        check(self.lib.blsgpu_fp_mul_throughput(self.h, iters, ctypes.byref(v)), "fp_mul_throughput")
        return v.value

    def mad_throughput(self, iters=2000):
        v = ctypes.c_double()
        check(self.lib.blsgpu_mad_throughput(self.h, iters, ctypes.byref(v)), "mad_throughput")
        return v.value

    # -- pairings ------------------------------------------------------------------------------------------
    def _pair_args(self, g1_xy, g1_inf, g2_xy, g2_inf):
        g1 = _u64(g1_xy, (-1, 12))
        g2 = _u64(g2_xy, (-1, 24))
        if g1.shape[0] != g2.shape[0]:
            raise ValueError("G1 and G2 inputs differ in length")
        n = g1.shape[0]
        return g1, _flags(g1_inf, n), g2, _flags(g2_inf, n), n

    def pairing_batch(self, g1_xy, g1_inf, g2_xy, g2_inf):
        g1, f1, g2, f2, n = self._pair_args(g1_xy, g1_inf, g2_xy, g2_inf)
        out = np.zeros((n, 72), dtype=np.uint64)
        check(self.lib.blsgpu_pairing_batch(self.h, _ptr(g1), _ptr(f1), _ptr(g2), _ptr(f2), n, _ptr(out)), "pairing_batch")
        return out

    def miller_loop_batch(self, g1_xy, g1_inf, g2_xy, g2_inf):
        g1, f1, g2, f2, n = self._pair_args(g1_xy, g1_inf, g2_xy, g2_inf)
        out = np.zeros((n, 72), dtype=np.uint64)
        check(self.lib.blsgpu_miller_loop_batch(self.h, _ptr(g1), _ptr(f1), _ptr(g2), _ptr(f2), n, _ptr(out)), "miller_loop_batch")
        return out

    def multi_miller_loop(self, g1_xy, g1_inf, g2_xy, g2_inf):
        g1, f1, g2, f2, n = self._pair_args(g1_xy, g1_inf, g2_xy, g2_inf)
        out = np.zeros(72, dtype=np.uint64)
        check(self.lib.blsgpu_multi_miller_loop(self.h, _ptr(g1), _ptr(f1), _ptr(g2), _ptr(f2), n, _ptr(out)), "multi_miller_loop")
        return out

    def multi_miller_loop_many(self, g1_xy, g1_inf, g2_xy, g2_inf, offsets, final_exp=True):
        """N independent `multi_miller_loop`s (CSR offsets over the terms) -> (N, 72): `MillerLoopResult`s, or -- final_exp --
        `Gt`s (`blsgpu_multi_miller_loop_many`; pairings.rs:554-603 once per segment)"""
        g1, f1, g2, f2, n = self._pair_args(g1_xy, g1_inf, g2_xy, g2_inf)
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64))
        if off.ndim != 1 or off.shape[0] < 1 or int(off[-1]) != n:
            raise ValueError("multi_miller_loop_many: offsets must be nseg + 1 values ending at the number of terms")
        nseg = off.shape[0] - 1
        out = np.zeros((nseg, 72), dtype=np.uint64)
        check(self.lib.blsgpu_multi_miller_loop_many(self.h, _ptr(g1), _ptr(f1), _ptr(g2), _ptr(f2), _ptr(off), nseg, 1 if final_exp else 0, _ptr(out)),
              "multi_miller_loop_many")
        return out

    def multi_miller_loop_many_device(self, d_g1, d_g2, d_offsets, nseg, total_terms, d_out, max_seg_terms=0, final_exp=True, d_g1_inf=None, d_g2_inf=None):
        check(self.lib.blsgpu_multi_miller_loop_many_device(self.h, ctypes.c_void_p(d_g1), ctypes.c_void_p(d_g1_inf), ctypes.c_void_p(d_g2), ctypes.c_void_p(d_g2_inf),
                                                            ctypes.c_void_p(d_offsets), nseg, total_terms, max_seg_terms, 1 if final_exp else 0, ctypes.c_void_p(d_out)),
              "multi_miller_loop_many_device")

    # -- the widened rows with device pointers (a chain that stays in HBM) and bulk signature verification -------------
    def batch_normalize_device(self, group, d_xyz, n, d_xy, d_inf):
        fn = self.lib.blsgpu_g1_batch_normalize_device if group == 1 else self.lib.blsgpu_g2_batch_normalize_device
        check(fn(self.h, ctypes.c_void_p(d_xyz), n, ctypes.c_void_p(d_xy), ctypes.c_void_p(d_inf)), "batch_normalize_device")

    def points_from_bytes_device(self, group, d_bytes, n, d_xy, d_inf, d_ok, compressed=True, checked=True):
        fn = self.lib.blsgpu_g1_from_bytes_batch_device if group == 1 else self.lib.blsgpu_g2_from_bytes_batch_device
        check(fn(self.h, ctypes.c_void_p(d_bytes), n, 1 if compressed else 0, 1 if checked else 0, ctypes.c_void_p(d_xy), ctypes.c_void_p(d_inf), ctypes.c_void_p(d_ok)),
              "from_bytes_batch_device")

    def points_to_bytes_device(self, group, d_xy, d_inf, n, d_out, compressed=True):
        fn = self.lib.blsgpu_g1_to_bytes_batch_device if group == 1 else self.lib.blsgpu_g2_to_bytes_batch_device
        check(fn(self.h, ctypes.c_void_p(d_xy), ctypes.c_void_p(d_inf), n, 1 if compressed else 0, ctypes.c_void_p(d_out)), "to_bytes_batch_device")

    def gt_mul_scalar_batch_device(self, d_gt, d_scalars, n, d_out):
        check(self.lib.blsgpu_gt_mul_scalar_batch_device(self.h, ctypes.c_void_p(d_gt), ctypes.c_void_p(d_scalars), n, ctypes.c_void_p(d_out)), "gt_mul_scalar_batch_device")

    def gt_is_identity_device(self, d_gt, n, d_flags):
        check(self.lib.blsgpu_gt_is_identity_device(self.h, ctypes.c_void_p(d_gt), n, ctypes.c_void_p(d_flags)), "gt_is_identity_device")

    def bls_verify_batch(self, mode, pk_bytes, sig_bytes, msgs, dst):
        """Bulk BLS verification from bytes (blsgpu_bls_verify_batch): mode 0 = public keys in G1 (48 B) / signatures in G2 (96 B),
        mode 1 the other way round; msgs: list of bytes.  -> (n,) uint8: 1 valid, 0 invalid, 2 bad public key, 3 bad signature"""
        n = len(msgs)
        pk = np.ascontiguousarray(np.frombuffer(bytes(pk_bytes), dtype=np.uint8)) if not isinstance(pk_bytes, np.ndarray) else np.ascontiguousarray(pk_bytes, dtype=np.uint8).reshape(-1)
        sg = np.ascontiguousarray(np.frombuffer(bytes(sig_bytes), dtype=np.uint8)) if not isinstance(sig_bytes, np.ndarray) else np.ascontiguousarray(sig_bytes, dtype=np.uint8).reshape(-1)
        if pk.shape[0] != n * (48 if mode == 0 else 96) or sg.shape[0] != n * (96 if mode == 0 else 48):
            raise ValueError("bls_verify_batch: key / signature bytes do not match the number of messages")
        off = np.zeros(n + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(m) for m in msgs])
        blob = np.frombuffer(b"".join(bytes(m) for m in msgs), dtype=np.uint8).copy() if int(off[-1]) else np.zeros(1, dtype=np.uint8)
        d = np.frombuffer(bytes(dst), dtype=np.uint8).copy() if len(dst) else np.zeros(1, dtype=np.uint8)
        out = np.zeros(n, dtype=np.uint8)
        check(self.lib.blsgpu_bls_verify_batch(self.h, mode, _ptr(pk), _ptr(sg), _ptr(blob), _ptr(off), n, _ptr(d), len(dst), _ptr(out)), "bls_verify_batch")
        return out

    def bls_verify_batch_device(self, mode, d_pk, d_sig, d_msgs, d_offsets, n, d_dst, dst_len, d_verdict):
        check(self.lib.blsgpu_bls_verify_batch_device(self.h, mode, ctypes.c_void_p(d_pk), ctypes.c_void_p(d_sig), ctypes.c_void_p(d_msgs), ctypes.c_void_p(d_offsets), n,
                                                      ctypes.c_void_p(d_dst), dst_len, ctypes.c_void_p(d_verdict)), "bls_verify_batch_device")

    def bls_fast_aggregate_verify(self, mode, d_keys_xy, d_keys_inf, nkeys, subsets, sig_bytes, msgs, dst):
        """Aggregate BLS verification (blsgpu_bls_fast_aggregate_verify_batch): signature i over msgs[i] by the keys subsets[i] (a list of
        index lists) of a key set RESIDENT on the device (d_keys_xy / d_keys_inf: device addresses of nkeys decoded affine points, G1 in
        mode 0, G2 in mode 1).  -> (n,) uint8: 1 valid, 0 invalid, 3 bad signature"""
        n = len(msgs)
        if len(subsets) != n:
            raise ValueError("bls_fast_aggregate_verify: one subset per message")
        sg = np.ascontiguousarray(np.frombuffer(bytes(sig_bytes), dtype=np.uint8)) if not isinstance(sig_bytes, np.ndarray) else np.ascontiguousarray(sig_bytes, dtype=np.uint8).reshape(-1)
        if sg.shape[0] != n * (96 if mode == 0 else 48):
            raise ValueError("bls_fast_aggregate_verify: signature bytes do not match the number of messages")
        koff = np.zeros(n + 1, dtype=np.uint64)
        koff[1:] = np.cumsum([len(s) for s in subsets])
        total = int(koff[-1])
        idx = np.array([i for s in subsets for i in s], dtype=np.uint32) if total else np.zeros(1, dtype=np.uint32)
        off = np.zeros(n + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(m) for m in msgs])
        blob = np.frombuffer(b"".join(bytes(m) for m in msgs), dtype=np.uint8).copy() if int(off[-1]) else np.zeros(1, dtype=np.uint8)
        d = np.frombuffer(bytes(dst), dtype=np.uint8).copy() if len(dst) else np.zeros(1, dtype=np.uint8)
        out = np.zeros(n, dtype=np.uint8)
        check(self.lib.blsgpu_bls_fast_aggregate_verify_batch(self.h, mode, ctypes.c_void_p(d_keys_xy), ctypes.c_void_p(d_keys_inf), nkeys, _ptr(idx), _ptr(koff), total, _ptr(sg),
                                                              _ptr(blob), _ptr(off), n, _ptr(d), len(dst), _ptr(out)), "bls_fast_aggregate_verify_batch")
        return out

    def bls_fast_aggregate_verify_device(self, mode, d_keys_xy, d_keys_inf, nkeys, d_idx, d_key_offsets, total_keys, d_sig, d_msgs, d_msg_offsets, n, d_dst, dst_len, d_verdict):
        vp = lambda p: ctypes.c_void_p(p) if p else None
        check(self.lib.blsgpu_bls_fast_aggregate_verify_batch_device(self.h, mode, vp(d_keys_xy), vp(d_keys_inf), nkeys, vp(d_idx), vp(d_key_offsets), total_keys, vp(d_sig),
                                                                     vp(d_msgs), vp(d_msg_offsets), n, vp(d_dst), dst_len, vp(d_verdict)), "bls_fast_aggregate_verify_batch_device")

    # -- G2Prepared resident on the device (pairings.rs:487-546) and its consumers (:554-603) -----------------------
    def g2_prepare(self, g2_xy, g2_inf=None):
        g2 = _u64(g2_xy, (-1, 24))
        m = g2.shape[0]
        h = ctypes.c_void_p()
        check(self.lib.blsgpu_g2_prepare(self.h, _ptr(g2), _ptr(_flags(g2_inf, m)) if g2_inf is not None else None, m, ctypes.byref(h)), "g2_prepare")
        return PreparedG2Table(self, h)

    def g2_prepare_device(self, d_g2, d_inf, m):
        h = ctypes.c_void_p()
        check(self.lib.blsgpu_g2_prepare_device(self.h, ctypes.c_void_p(d_g2), ctypes.c_void_p(d_inf), m, ctypes.byref(h)), "g2_prepare_device")
        return PreparedG2Table(self, h)

    def _prepared_args(self, g1_xy, g1_inf, q_index, g2_xy, g2_inf):
        g1 = _u64(g1_xy, (-1, 12))
        n = g1.shape[0]
        qi = None
        if q_index is not None:
            qi = np.ascontiguousarray(np.asarray(q_index, dtype=np.uint32))
            if qi.shape != (n,):
                raise ValueError("q_index must name one table entry (or UNPREPARED) per term")
        g2 = None
        if g2_xy is not None:
            g2 = _u64(g2_xy, (-1, 24))
            if g2.shape[0] != n:
                raise ValueError("G1 and G2 inputs differ in length")
        f2 = _flags(g2_inf, n) if (g2 is not None and g2_inf is not None) else None
        return g1, _flags(g1_inf, n), g2, f2, qi, n

    def multi_miller_loop_prepared(self, g1_xy, g1_inf, table, q_index, g2_xy=None, g2_inf=None):
        """prod_i ML(g1[i], Q_i) with Q_i = table[q_index[i]] or -- q_index[i] = UNPREPARED -- g2[i] (pairings.rs:554-603)"""
        g1, f1, g2, f2, qi, n = self._prepared_args(g1_xy, g1_inf, q_index, g2_xy, g2_inf)
        out = np.zeros(72, dtype=np.uint64)
        check(self.lib.blsgpu_multi_miller_loop_prepared(self.h, _ptr(g1), _ptr(f1), _ptr(g2) if g2 is not None else None, _ptr(f2) if f2 is not None else None,
                                                         _ptr(qi) if qi is not None else None, table.handle if table is not None else None, n, _ptr(out)),
              "multi_miller_loop_prepared")
        return out

    def multi_miller_loop_prepared_many(self, g1_xy, g1_inf, table, q_index, offsets, g2_xy=None, g2_inf=None, final_exp=True):
        g1, f1, g2, f2, qi, n = self._prepared_args(g1_xy, g1_inf, q_index, g2_xy, g2_inf)
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64))
        if off.ndim != 1 or off.shape[0] < 1 or int(off[-1]) != n:
            raise ValueError("multi_miller_loop_prepared_many: offsets must be nseg + 1 values ending at the number of terms")
        nseg = off.shape[0] - 1
        out = np.zeros((nseg, 72), dtype=np.uint64)
        check(self.lib.blsgpu_multi_miller_loop_prepared_many(self.h, _ptr(g1), _ptr(f1), _ptr(g2) if g2 is not None else None, _ptr(f2) if f2 is not None else None,
                                                              _ptr(qi) if qi is not None else None, table.handle if table is not None else None, _ptr(off), nseg,
                                                              1 if final_exp else 0, _ptr(out)), "multi_miller_loop_prepared_many")
        return out

    def multi_miller_loop_prepared_device(self, d_g1, table, d_q_index, n, d_out, d_g2=None, d_g1_inf=None, d_g2_inf=None):
        check(self.lib.blsgpu_multi_miller_loop_prepared_device(self.h, ctypes.c_void_p(d_g1), ctypes.c_void_p(d_g1_inf), ctypes.c_void_p(d_g2), ctypes.c_void_p(d_g2_inf),
                                                                ctypes.c_void_p(d_q_index), table.handle if table is not None else None, n, ctypes.c_void_p(d_out)),
              "multi_miller_loop_prepared_device")

    def multi_miller_loop_prepared_many_device(self, d_g1, table, d_q_index, d_offsets, nseg, total_terms, d_out, max_seg_terms=0, final_exp=True, d_g2=None, d_g1_inf=None,
                                               d_g2_inf=None):
        check(self.lib.blsgpu_multi_miller_loop_prepared_many_device(self.h, ctypes.c_void_p(d_g1), ctypes.c_void_p(d_g1_inf), ctypes.c_void_p(d_g2), ctypes.c_void_p(d_g2_inf),
                                                                     ctypes.c_void_p(d_q_index), table.handle if table is not None else None, ctypes.c_void_p(d_offsets), nseg,
                                                                     total_terms, max_seg_terms, 1 if final_exp else 0, ctypes.c_void_p(d_out)),
              "multi_miller_loop_prepared_many_device")

    def wide_status(self):
        """'' when the small-batch (wide) pairing programs are loaded, otherwise the reason they are not"""
        return (self.lib.blsgpu_wide_status(self.h) or b"").decode()

    def final_exponentiation_batch(self, f):
        f = _u64(f, (-1, 72))
        out = np.zeros_like(f)
        check(self.lib.blsgpu_final_exponentiation_batch(self.h, _ptr(f), f.shape[0], _ptr(out)), "final_exponentiation")
        return out

    def gt_mul_scalar_batch(self, gt, scalars):
        """out[i] = gt[i] * scalars[i] (`&Gt * &Scalar`, pairings.rs:297-322); scalars: ints or (n, 32) little-endian bytes"""
        gt = _u64(gt, (-1, 72))
        sb = scalars_to_bytes(scalars)
        if sb.shape[0] != gt.shape[0]:
            raise ValueError("gt_mul_scalar_batch: lengths differ")
        out = np.zeros_like(gt)
        with self._bytes_form(_builds_bytes(scalars)):
            check(self.lib.blsgpu_gt_mul_scalar_batch(self.h, _ptr(gt), _ptr(sb), gt.shape[0], _ptr(out)), "gt_mul_scalar_batch")
        return out

    # device-pointer variants (asynchronous on the context's stream); pointers are plain ints (e.g. tensor.data_ptr())
    def pairing_batch_device(self, d_g1, d_g2, n, d_out, d_g1_inf=None, d_g2_inf=None):
        check(self.lib.blsgpu_pairing_batch_device(self.h, ctypes.c_void_p(d_g1), ctypes.c_void_p(d_g1_inf), ctypes.c_void_p(d_g2), ctypes.c_void_p(d_g2_inf), n,
                                                   ctypes.c_void_p(d_out)), "pairing_batch_device")

    def miller_loop_batch_device(self, d_g1, d_g2, n, d_out, d_g1_inf=None, d_g2_inf=None):
        check(self.lib.blsgpu_miller_loop_batch_device(self.h, ctypes.c_void_p(d_g1), ctypes.c_void_p(d_g1_inf), ctypes.c_void_p(d_g2), ctypes.c_void_p(d_g2_inf), n,
                                                       ctypes.c_void_p(d_out)), "miller_loop_batch_device")

    def multi_miller_loop_device(self, d_g1, d_g2, n, d_out, d_g1_inf=None, d_g2_inf=None):
        check(self.lib.blsgpu_multi_miller_loop_device(self.h, ctypes.c_void_p(d_g1), ctypes.c_void_p(d_g1_inf), ctypes.c_void_p(d_g2), ctypes.c_void_p(d_g2_inf), n,
                                                       ctypes.c_void_p(d_out)), "multi_miller_loop_device")

    def final_exponentiation_device(self, d_in, n, d_out):
        check(self.lib.blsgpu_final_exponentiation_device(self.h, ctypes.c_void_p(d_in), n, ctypes.c_void_p(d_out)), "final_exponentiation_device")

    def fp12_product_device(self, d_in, n, d_out):
        check(self.lib.blsgpu_fp12_product_device(self.h, ctypes.c_void_p(d_in), n, ctypes.c_void_p(d_out)), "fp12_product_device")

    def fp12_product(self, f):
        f = _u64(f, (-1, 72))
        out = np.zeros(72, dtype=np.uint64)
        check(self.lib.blsgpu_fp12_product(self.h, _ptr(f), f.shape[0], _ptr(out)), "fp12_product")
        return out


class GroupBases:
    """Resident bases sharded over the members of a Group (`blsgpu_group_bases`): member k holds a contiguous slice."""

    def __init__(self, group, handle, gid):
        self.group, self.handle, self.gid = group, handle, gid

    def __len__(self):
        return int(_lib.load().blsgpu_group_bases_len(self.handle))

    def free(self):
        if self.handle:
            _lib.load().blsgpu_group_bases_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class GroupPreparedG2:
    """the same `G2Prepared` table on every member of a Group (`blsgpu_group_g2_prepared`)"""

    def __init__(self, group, handle):
        self.group, self.handle = group, handle

    def __len__(self):
        return int(_lib.load().blsgpu_group_g2_prepared_len(self.handle)) if self.handle else 0

    def free(self):
        if self.handle:
            _lib.load().blsgpu_group_g2_prepared_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Group:
    """The hot path sharded over several GPUs of one node from ONE process (`blsgpu_group`, include/bls12_381_hip.h): one
    context and one host thread per listed device; partial results (one group element per member) are folded with `Sum`
    (g1.rs:161-171) / `MillerLoopResult + MillerLoopResult` (pairings.rs:179-186).  A device may be listed more than once."""

    def __init__(self, devices):
        self.lib = _lib.load()
        devs = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
        h = ctypes.c_void_p()
        check(self.lib.blsgpu_group_create(devs, len(devices), ctypes.byref(h)), "group_create")
        self.h = h
        self.scalar_form = SCALAR_BYTES

    def close(self):
        if getattr(self, "h", None):
            self.lib.blsgpu_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return int(self.lib.blsgpu_group_size(self.h))

    def _set_members_form(self, form):
        for k in range(len(self)):
            check(self.lib.blsgpu_set_scalar_form(ctypes.c_void_p(self.lib.blsgpu_group_ctx(self.h, k)), int(form)), "set_scalar_form")

    def set_scalar_form(self, form):
        """Context.set_scalar_form on every member (what the `*_sharded_device` MSMs read); `msm` with ints / Scalars still pins SCALAR_BYTES"""
        self._set_members_form(form)
        self.scalar_form = int(form)

    def set_assume_subgroup(self, on):
        for k in range(len(self)):
            check(self.lib.blsgpu_set_assume_subgroup(ctypes.c_void_p(self.lib.blsgpu_group_ctx(self.h, k)), 1 if on else 0), "set_assume_subgroup")

    def upload_bases(self, group, xy, infinity=None):
        w = 12 if group == 1 else 24
        xy = _u64(xy, (-1, w))
        n = xy.shape[0]
        inf = _flags(infinity, n)
        h = ctypes.c_void_p()
        check(self.lib.blsgpu_group_bases_upload(self.h, group, _ptr(xy), _ptr(inf), n, ctypes.byref(h)), "group_bases_upload")
        return GroupBases(self, h, group)

    def bases_from_scalars(self, group, scalars):
        sb = scalars_to_bytes(scalars)
        h = ctypes.c_void_p()
        check(self.lib.blsgpu_group_bases_from_scalars(self.h, group, _ptr(sb), sb.shape[0], ctypes.byref(h)), "group_bases_from_scalars")
        return GroupBases(self, h, group)

    def msm(self, bases, scalars):
        sb = scalars_to_bytes(scalars)
        out = np.zeros(18 if bases.gid == 1 else 36, dtype=np.uint64)
        fn = self.lib.blsgpu_g1_msm_sharded if bases.gid == 1 else self.lib.blsgpu_g2_msm_sharded
        pin = _builds_bytes(scalars) and self.scalar_form != SCALAR_BYTES
        if pin:
            self._set_members_form(SCALAR_BYTES)
        try:
            check(fn(self.h, bases.handle, _ptr(sb), sb.shape[0], _ptr(out)), "msm_sharded")
        finally:
            if pin:
                self._set_members_form(self.scalar_form)
        return out

    # device-pointer, asynchronous MSMs on every member (the pipelined headline path from one process)
    def member_ctx(self, k):
        """raw handle of member k's context (blsgpu_group_ctx) for per-context calls through the ctypes layer"""
        return ctypes.c_void_p(self.lib.blsgpu_group_ctx(self.h, k))

    def shard_sizes(self, n):
        """points per member for n resident points (the rule of blsgpu_group_bases_*: contiguous slices, sizes differ by at most one)"""
        w = len(self)
        return [n // w + (1 if k < n % w else 0) for k in range(w)]

    def set_pipelining(self, on):
        check(self.lib.blsgpu_group_set_pipelining(self.h, 1 if on else 0), "group_set_pipelining")

    def synchronize(self):
        check(self.lib.blsgpu_group_synchronize(self.h), "group_synchronize")

    def msm_sharded_device(self, bases, d_scalars, d_partials):
        """member k: partial sum of its whole resident slice times the scalars at d_scalars[k] -> d_partials[k] (device pointers as ints,
        each in member k's device memory); only enqueues"""
        w = len(self)
        sp = (ctypes.c_void_p * w)(*[ctypes.c_void_p(int(p)) for p in d_scalars])
        op = (ctypes.c_void_p * w)(*[ctypes.c_void_p(int(p)) for p in d_partials])
        fn = self.lib.blsgpu_g1_msm_sharded_device if bases.gid == 1 else self.lib.blsgpu_g2_msm_sharded_device
        check(fn(self.h, bases.handle, sp, op), "msm_sharded_device")

    def partials_fold(self, gid, d_partials, lag=0):
        """the sum of the members' partial sums at d_partials (waiting, per member, for all but the `lag` most recent MSM calls)"""
        w = len(self)
        op = (ctypes.c_void_p * w)(*[ctypes.c_void_p(int(p)) for p in d_partials])
        out = np.zeros(18 if gid == 1 else 36, dtype=np.uint64)
        fn = self.lib.blsgpu_g1_partials_fold if gid == 1 else self.lib.blsgpu_g2_partials_fold
        check(fn(self.h, op, lag, _ptr(out)), "partials_fold")
        return out

    def pairings_sharded_device(self, mode, d_g1, d_g2, counts, d_out, d_g1_inf=None, d_g2_inf=None):
        """member k: mode 0 pairings / 1 raw Miller values / 2 its local multi_miller_loop product of counts[k] pairs at d_g1[k], d_g2[k] -> d_out[k]; enqueues only"""
        w = len(self)
        arr = lambda ps: (ctypes.c_void_p * w)(*[ctypes.c_void_p(int(p)) for p in ps]) if ps is not None else None
        cnt = (ctypes.c_size_t * w)(*[int(c) for c in counts])
        check(self.lib.blsgpu_pairings_sharded_device(self.h, mode, arr(d_g1), arr(d_g1_inf), arr(d_g2), arr(d_g2_inf), cnt, arr(d_out)), "pairings_sharded_device")

    def fp12_partials_fold_device(self, d_partials, d_out, final_exp=False):
        w = len(self)
        op = (ctypes.c_void_p * w)(*[ctypes.c_void_p(int(p)) for p in d_partials])
        check(self.lib.blsgpu_fp12_partials_fold_device(self.h, op, 1 if final_exp else 0, ctypes.c_void_p(int(d_out))), "fp12_partials_fold_device")

    # G2Prepared tables on every member; the prepared Miller loops sharded like the unprepared ones
    def g2_prepare(self, g2_xy, g2_inf=None):
        g2 = _u64(g2_xy, (-1, 24))
        m = g2.shape[0]
        h = ctypes.c_void_p()
        check(self.lib.blsgpu_group_g2_prepare(self.h, _ptr(g2), _ptr(_flags(g2_inf, m)) if g2_inf is not None else None, m, ctypes.byref(h)), "group_g2_prepare")
        return GroupPreparedG2(self, h)

    def multi_miller_loop_prepared(self, g1_xy, g1_inf, table, q_index, g2_xy=None, g2_inf=None, final_exp=False):
        g1, f1, g2, f2, qi, n = Context._prepared_args(self, g1_xy, g1_inf, q_index, g2_xy, g2_inf)
        out = np.zeros(72, dtype=np.uint64)
        check(self.lib.blsgpu_multi_miller_loop_prepared_sharded(self.h, _ptr(g1), _ptr(f1), _ptr(g2) if g2 is not None else None, _ptr(f2) if f2 is not None else None,
                                                                 _ptr(qi) if qi is not None else None, table.handle if table is not None else None, n, 1 if final_exp else 0,
                                                                 _ptr(out)), "multi_miller_loop_prepared_sharded")
        return out

    def multi_miller_loop_prepared_many(self, g1_xy, g1_inf, table, q_index, offsets, g2_xy=None, g2_inf=None, final_exp=True):
        g1, f1, g2, f2, qi, n = Context._prepared_args(self, g1_xy, g1_inf, q_index, g2_xy, g2_inf)
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64))
        if off.ndim != 1 or off.shape[0] < 1 or int(off[-1]) != n:
            raise ValueError("multi_miller_loop_prepared_many: offsets must be nseg + 1 values ending at the number of terms")
        nseg = off.shape[0] - 1
        out = np.zeros((nseg, 72), dtype=np.uint64)
        check(self.lib.blsgpu_multi_miller_loop_prepared_many_sharded(self.h, _ptr(g1), _ptr(f1), _ptr(g2) if g2 is not None else None, _ptr(f2) if f2 is not None else None,
                                                                      _ptr(qi) if qi is not None else None, table.handle if table is not None else None, _ptr(off), nseg,
                                                                      1 if final_exp else 0, _ptr(out)), "multi_miller_loop_prepared_many_sharded")
        return out

    def partials_fold_device(self, gid, d_partials, d_out, lag=0):
        """the same fold queued on the members' streams: the sum lands at d_out (member 0's device memory), nothing is synchronised"""
        w = len(self)
        op = (ctypes.c_void_p * w)(*[ctypes.c_void_p(int(p)) for p in d_partials])
        fn = self.lib.blsgpu_g1_partials_fold_device if gid == 1 else self.lib.blsgpu_g2_partials_fold_device
        check(fn(self.h, op, lag, ctypes.c_void_p(int(d_out))), "partials_fold_device")

    _pair_args = Context._pair_args

    def pairing_batch(self, g1_xy, g1_inf, g2_xy, g2_inf):
        g1, f1, g2, f2, n = self._pair_args(g1_xy, g1_inf, g2_xy, g2_inf)
        out = np.zeros((n, 72), dtype=np.uint64)
        check(self.lib.blsgpu_pairing_batch_sharded(self.h, _ptr(g1), _ptr(f1), _ptr(g2), _ptr(f2), n, _ptr(out)), "pairing_batch_sharded")
        return out

    def miller_loop_batch(self, g1_xy, g1_inf, g2_xy, g2_inf):
        g1, f1, g2, f2, n = self._pair_args(g1_xy, g1_inf, g2_xy, g2_inf)
        out = np.zeros((n, 72), dtype=np.uint64)
        check(self.lib.blsgpu_miller_loop_batch_sharded(self.h, _ptr(g1), _ptr(f1), _ptr(g2), _ptr(f2), n, _ptr(out)), "miller_loop_batch_sharded")
        return out

    def multi_miller_loop(self, g1_xy, g1_inf, g2_xy, g2_inf, final_exp=False):
        g1, f1, g2, f2, n = self._pair_args(g1_xy, g1_inf, g2_xy, g2_inf)
        out = np.zeros(72, dtype=np.uint64)
        check(self.lib.blsgpu_multi_miller_loop_sharded(self.h, _ptr(g1), _ptr(f1), _ptr(g2), _ptr(f2), n, 1 if final_exp else 0, _ptr(out)), "multi_miller_loop_sharded")
        return out

    def multi_miller_loop_many(self, g1_xy, g1_inf, g2_xy, g2_inf, offsets, final_exp=True):
        g1, f1, g2, f2, n = self._pair_args(g1_xy, g1_inf, g2_xy, g2_inf)
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64))
        if off.ndim != 1 or off.shape[0] < 1 or int(off[-1]) != n:
            raise ValueError("multi_miller_loop_many: offsets must be nseg + 1 values ending at the number of terms")
        nseg = off.shape[0] - 1
        out = np.zeros((nseg, 72), dtype=np.uint64)
        check(self.lib.blsgpu_multi_miller_loop_many_sharded(self.h, _ptr(g1), _ptr(f1), _ptr(g2), _ptr(f2), _ptr(off), nseg, 1 if final_exp else 0, _ptr(out)),
              "multi_miller_loop_many_sharded")
        return out


_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


# ======================================================================================================
# value types mirroring the reference
# ======================================================================================================
class Scalar:
    """Element of Fr (src/scalar.rs).  Only `to_bytes`/`from_bytes` are on the hot path (the bit source
    of scalar multiplication, scalar.rs:284-296); arithmetic is plain Python integers mod r."""

    __slots__ = ("value",)

    def __init__(self, value=0):
        self.value = int(value) % R_ORDER

    @staticmethod
    def zero(): return Scalar(0)
    @staticmethod
    def one(): return Scalar(1)

    @staticmethod
    def from_bytes(b):
        """scalar.rs:256-280: 32 little-endian bytes, None (CtOption none) if not canonical."""
        v = int.from_bytes(bytes(b), "little")
        return Scalar(v) if v < R_ORDER else None

    @staticmethod
    def from_bytes_wide(b):
        """scalar.rs:300-331: 64 little-endian bytes reduced mod r."""
        return Scalar(int.from_bytes(bytes(b), "little"))

    def to_bytes(self): return self.value.to_bytes(32, "little")
    def __add__(self, o): return Scalar(self.value + o.value)
    def __sub__(self, o): return Scalar(self.value - o.value)
    def __neg__(self): return Scalar(-self.value)
    def __mul__(self, o):
        if isinstance(o, Scalar):
            return Scalar(self.value * o.value)
        return NotImplemented
    def invert(self): return None if self.value == 0 else Scalar(pow(self.value, -1, R_ORDER))
    def __eq__(self, o): return isinstance(o, Scalar) and self.value == o.value
    def __hash__(self): return hash(self.value)
    def __repr__(self): return f"Scalar(0x{self.value:064x})"


def _fp_bytes(l):
    return limbs_to_fp(l).to_bytes(48, "big")


def _lex_largest(v):
    return v > (P - 1) // 2


class _Group:
    """shared plumbing of the four point types; G = 1 or 2, W = u64 words per coordinate"""
    G = 1
    W = 6


class G1Affine(_Group):
    """src/g1.rs:28-32.  `xy` = 12 uint64 Montgomery limbs (x | y), `infinity` bool."""
    G, W = 1, 6

    def __init__(self, xy, infinity=False):
        self.xy = _u64(xy, (2 * self.W,)).copy()
        self.infinity = bool(infinity)

    @classmethod
    def identity(cls):
        one = fp_to_limbs(1)
        z = np.zeros(6, dtype=np.uint64)
        if cls.G == 1:
            return cls(np.concatenate([z, one]), True)
        return cls(np.concatenate([z, z, one, z]), True)

    @classmethod
    def generator(cls):
        if cls.G == 1:
            return cls(np.concatenate([fp_to_limbs(_G1X), fp_to_limbs(_G1Y)]))
        return cls(np.concatenate([fp_to_limbs(_G2X[0]), fp_to_limbs(_G2X[1]), fp_to_limbs(_G2Y[0]), fp_to_limbs(_G2Y[1])]))

    def is_identity(self): return self.infinity

    def __neg__(self):
        if self.infinity:
            # g1.rs:121-130: conditional_select(&-y, &Fp::one(), infinity) -- the identity keeps its (0, 1, inf) limbs
            return type(self)(self.xy.copy(), True)
        xy = self.xy.copy()
        for k in range(self.W // 6):
            off = self.W + 6 * k
            xy[off:off + 6] = fp_to_limbs((-limbs_to_fp(xy[off:off + 6])) % P)
        return type(self)(xy, self.infinity)

    def __eq__(self, o):
        return type(o) is type(self) and ((self.infinity and o.infinity) or
                                          (self.infinity == o.infinity and bool(np.array_equal(self.xy, o.xy))))

    def to_projective(self):
        one = fp_to_limbs(1)
        z = np.zeros(self.W, dtype=np.uint64)
        if not self.infinity:
            z[:6] = one
        return self._PROJ(np.concatenate([self.xy, z]))

    def __mul__(self, s):
        """`&G1Affine * &Scalar` (g1.rs:573-579): the batched variable-base kernel with one element."""
        ctx = default_context()
        out = ctx.mul_batch(self.G, self.xy[None, :], np.array([self.infinity], dtype=np.uint8), [s])
        return self._PROJ(out[0])

    @classmethod
    def mul_batch(cls, points, scalars):
        """points.iter().zip(scalars).map(|(p, s)| p * s) as ONE device call: [G1Projective] (`Mul` over slices)."""
        points = list(points)
        if not points:
            return []
        xy = np.stack([p.xy for p in points]); inf = np.array([p.infinity for p in points], dtype=np.uint8)
        out = default_context().mul_batch(cls.G, xy, inf, scalars)
        return [cls._PROJ(o) for o in out]

    # -- encodings (src/notes/serialization.rs; g1.rs:221-260, g2.rs:254-299) --
    def to_uncompressed(self):
        if self.G == 1:
            res = bytearray((b"\0" * 96) if self.infinity else _fp_bytes(self.xy[0:6]) + _fp_bytes(self.xy[6:12]))
        else:
            res = bytearray((b"\0" * 192) if self.infinity else
                            _fp_bytes(self.xy[6:12]) + _fp_bytes(self.xy[0:6]) + _fp_bytes(self.xy[18:24]) + _fp_bytes(self.xy[12:18]))
        if self.infinity:
            res[0] |= 1 << 6
        return bytes(res)

    def to_compressed(self):
        if self.G == 1:
            res = bytearray((b"\0" * 48) if self.infinity else _fp_bytes(self.xy[0:6]))
            big = (not self.infinity) and _lex_largest(limbs_to_fp(self.xy[6:12]))
        else:
            res = bytearray((b"\0" * 96) if self.infinity else _fp_bytes(self.xy[6:12]) + _fp_bytes(self.xy[0:6]))
            y0, y1 = limbs_to_fp(self.xy[12:18]), limbs_to_fp(self.xy[18:24])
            big = (not self.infinity) and (_lex_largest(y1) or (y1 == 0 and _lex_largest(y0)))
        res[0] |= 1 << 7
        if self.infinity:
            res[0] |= 1 << 6
        if big:
            res[0] |= 1 << 5
        return bytes(res)

    @classmethod
    def from_uncompressed_unchecked(cls, b):
        """g1.rs:273-322 / g2.rs:311-380; None where the reference returns CtOption::none."""
        b = bytes(b)
        n = 2 * cls.W // 6
        if len(b) != 48 * n:
            return None
        c, i, s = (b[0] >> 7) & 1, (b[0] >> 6) & 1, (b[0] >> 5) & 1
        vals = [int.from_bytes((bytes([b[0] & 0x1F]) + b[1:48]) if k == 0 else b[48 * k:48 * k + 48], "big") for k in range(n)]
        if any(v >= P for v in vals) or c or s or (i and any(vals)):
            return None
        if i:
            return cls.identity()
        if cls.G == 1:
            return cls(np.concatenate([fp_to_limbs(vals[0]), fp_to_limbs(vals[1])]))
        return cls(np.concatenate([fp_to_limbs(vals[1]), fp_to_limbs(vals[0]), fp_to_limbs(vals[3]), fp_to_limbs(vals[2])]))

    @classmethod
    def _decode(cls, b, compressed, checked):
        b = bytes(b)
        if len(b) != (48 if compressed else 96) * cls.G:
            return None                  # the reference takes a fixed-size array; any other input has no decoding (CtOption none)
        xy, inf, ok = default_context().points_from_bytes(cls.G, b, compressed, checked)
        return cls(xy[0], bool(inf[0])) if ok[0] else None

    @classmethod
    def from_compressed(cls, b):
        """g1.rs:326-332 / g2.rs:390-395 (decompression + subgroup check on the GPU); None = CtOption::none."""
        return cls._decode(b, True, True)

    @classmethod
    def from_compressed_unchecked(cls, b): return cls._decode(b, True, False)

    @classmethod
    def from_uncompressed(cls, b):
        """g1.rs:264-267 (on-curve + subgroup check on the GPU)."""
        return cls._decode(b, False, True)

    def __repr__(self):
        return f"{type(self).__name__}({'identity' if self.infinity else self.to_compressed().hex()})"


class G1Projective(_Group):
    """src/g1.rs:442-446.  `xyz` = 18 uint64 Montgomery limbs (X | Y | Z), x = X/Z; identity (0:1:0)."""
    G, W = 1, 6
    _AFF = G1Affine

    def __init__(self, xyz):
        self.xyz = _u64(xyz, (3 * self.W,)).copy()

    @classmethod
    def identity(cls): return cls._AFF.identity().to_projective()
    @classmethod
    def generator(cls): return cls._AFF.generator().to_projective()

    def is_identity(self):
        return not self.xyz[2 * self.W:].any()

    def to_affine(self):
        """`G1Affine::from(&G1Projective)` (g1.rs:49-63)."""
        xy, inf = default_context().batch_normalize(self.G, self.xyz[None, :])
        return self._AFF(xy[0], bool(inf[0]))

    @classmethod
    def batch_normalize(cls, points):
        """`G1Projective::batch_normalize` (g1.rs:806-839)."""
        if not points:
            return []
        xy, inf = default_context().batch_normalize(cls.G, np.stack([p.xyz for p in points]))
        return [cls._AFF(xy[i], bool(inf[i])) for i in range(len(points))]

    def __add__(self, o):
        ctx = default_context()
        if isinstance(o, self._AFF):
            return type(self)(ctx.point_op(self.G, 2, self.xyz[None, :], o.xy[None, :], np.array([o.infinity], dtype=np.uint8))[0])
        return type(self)(ctx.point_op(self.G, 0, self.xyz[None, :], o.xyz[None, :])[0])

    def __neg__(self):
        a = self.xyz.copy()
        for k in range(self.W // 6):
            off = self.W + 6 * k
            a[off:off + 6] = fp_to_limbs((-limbs_to_fp(a[off:off + 6])) % P)
        return type(self)(a)

    def __sub__(self, o): return self + (-o)
    def double(self): return type(self)(default_context().point_op(self.G, 1, self.xyz[None, :])[0])

    def __mul__(self, s):
        """`&G1Projective * &Scalar` (g1.rs:556-562)."""
        return self.to_affine() * s

    @classmethod
    def sum(cls, points):
        """`Sum for G1Projective` (g1.rs:161-171)."""
        pts = list(points)
        if not pts:
            return cls.identity()
        return cls(default_context().point_sum(cls.G, np.stack([p.xyz for p in pts])))

    @classmethod
    def hash_to_curve(cls, msg, dst):
        """`<G as HashToCurve<ExpandMsgXmd<Sha256>>>::hash_to_curve(msg, dst)` (hash_to_curve/mod.rs:86-92)"""
        return cls(default_context().hash_to_curve(cls.G, [msg], dst)[0])

    @classmethod
    def encode_to_curve(cls, msg, dst):
        """`...::encode_to_curve(msg, dst)` (hash_to_curve/mod.rs:103-108)"""
        return cls(default_context().hash_to_curve(cls.G, [msg], dst, encode_only=True)[0])

    @classmethod
    def hash_to_curve_batch(cls, msgs, dst, encode_only=False):
        out = default_context().hash_to_curve(cls.G, msgs, dst, encode_only=encode_only)
        return [cls(row) for row in out]

    def __eq__(self, o):
        """projective equality (g1.rs:479-496) decided on canonical affine forms"""
        return type(o) is type(self) and self.to_affine() == o.to_affine()

    def __repr__(self): return f"{type(self).__name__}({self.to_affine()!r})"


class G2Affine(G1Affine):
    """src/g2.rs.  `xy` = 24 uint64 limbs (x.c0 x.c1 y.c0 y.c1)."""
    G, W = 2, 12


class G2Projective(G1Projective):
    G, W = 2, 12
    _AFF = G2Affine


G1Affine._PROJ = G1Projective
G2Affine._PROJ = G2Projective


class Gt:
    """Target group element (src/pairings.rs:204-337), written additively like the reference: `+` is the
    Fp12 product, `-x` the conjugate.  `f` = 72 uint64 limbs in struct order."""

    def __init__(self, f):
        self.f = _u64(f, (72,)).copy()

    @staticmethod
    def identity():
        f = np.zeros(72, dtype=np.uint64)
        f[:6] = fp_to_limbs(1)
        return Gt(f)

    @staticmethod
    def generator():
        """pairings.rs:359-475: e(G1::generator, G2::generator)."""
        return pairing(G1Affine.generator(), G2Affine.generator())

    def __add__(self, o): return Gt(default_context().fp12_op(0, self.f[None, :], o.f[None, :])[0])
    def __neg__(self): return Gt(default_context().fp12_op(8, self.f[None, :])[0])
    def __sub__(self, o): return self + (-o)
    def double(self): return Gt(default_context().fp12_op(3, self.f[None, :])[0])

    def __mul__(self, s):
        """`&Gt * &Scalar` (pairings.rs:297-322): double-and-add over the 255 low bits."""
        v = s.value if isinstance(s, Scalar) else int(s) % R_ORDER
        return Gt(default_context().gt_mul_scalar_batch(self.f[None, :], [v])[0])

    @staticmethod
    def sum(items):
        items = list(items)
        if not items:
            return Gt.identity()
        return Gt(default_context().fp12_product(np.stack([g.f for g in items])))

    def __eq__(self, o): return isinstance(o, Gt) and bool(np.array_equal(self.f, o.f))
    def __repr__(self): return f"Gt({self.f[:2]}...)"


class MillerLoopResult:
    """src/pairings.rs:26.  Deliberately has no equality, like the reference (:21-26)."""

    def __init__(self, f):
        self.f = _u64(f, (72,)).copy()

    @staticmethod
    def default(): return MillerLoopResult(Gt.identity().f)

    def final_exponentiation(self):
        """pairings.rs:48-176."""
        return Gt(default_context().final_exponentiation_batch(self.f[None, :])[0])

    def __add__(self, o):
        """pairings.rs:179-186: product of the underlying Fp12 values."""
        return MillerLoopResult(default_context().fp12_op(0, self.f[None, :], o.f[None, :])[0])


class G2Prepared:
    """src/pairings.rs:487-546.  Opaque in the reference (private fields).  `G2Prepared(q)` keeps the affine point (its lines are
    then computed on the fly in every Miller loop, as in rounds 1-4); `G2Prepared.resident(q)` / `G2Prepared.resident_many(points)`
    do what `From<G2Affine>` does in the reference: the 68 coefficient triples are computed ONCE, into a device-resident table
    (`blsgpu_g2_prepare`), and every later `multi_miller_loop` only evaluates them."""

    def __init__(self, q, table=None, index=None):
        if not isinstance(q, G2Affine):
            raise TypeError("G2Prepared::from expects a G2Affine")
        self.q, self.table, self.index = q, table, index

    @classmethod
    def resident_many(cls, points):
        points = list(points)
        xy = np.stack([q.xy for q in points]) if points else np.zeros((0, 24), dtype=np.uint64)
        table = default_context().g2_prepare(xy, np.array([q.infinity for q in points], dtype=np.uint8))
        return [cls(q, table, i) for i, q in enumerate(points)]

    @classmethod
    def resident(cls, q):
        return cls.resident_many([q])[0]

    def coeffs(self):
        """(infinity, (68, 3, 12) u64) of a resident value"""
        if self.table is None:
            raise ValueError("G2Prepared.coeffs: not resident (use G2Prepared.resident)")
        return self.table.coeffs(self.index)


def pairing(p, q):
    """`pairing(&G1Affine, &G2Affine) -> Gt` (src/pairings.rs:607-653)."""
    out = default_context().pairing_batch(p.xy[None, :], np.array([p.infinity], dtype=np.uint8), q.xy[None, :],
                                          np.array([q.infinity], dtype=np.uint8))
    return Gt(out[0])


def multi_miller_loop(terms):
    """`multi_miller_loop(&[(&G1Affine, &G2Prepared)]) -> MillerLoopResult` (src/pairings.rs:554-603)."""
    terms = list(terms)
    n = len(terms)
    g1 = np.zeros((n, 12), dtype=np.uint64)
    g2 = np.zeros((n, 24), dtype=np.uint64)
    f1 = np.zeros(n, dtype=np.uint8)
    f2 = np.zeros(n, dtype=np.uint8)
    for i, (p, prep) in enumerate(terms):
        g1[i], f1[i], g2[i], f2[i] = p.xy, p.infinity, prep.q.xy, prep.q.infinity
    table, qi = _resident_indices([prep for _, prep in terms])
    if table is not None:
        return MillerLoopResult(default_context().multi_miller_loop_prepared(g1, f1, table, qi, g2, f2))
    return MillerLoopResult(default_context().multi_miller_loop(g1, f1, g2, f2))


def _resident_indices(preps):
    """the table shared by the resident `G2Prepared` values among `preps` and the per-term indices (terms of another table, or not
    resident, are UNPREPARED: their lines are computed on the fly from the affine point they also hold); (None, None) if none is resident"""
    table = next((p.table for p in preps if p.table is not None), None)
    if table is None:
        return None, None
    return table, np.array([p.index if p.table is table else UNPREPARED for p in preps], dtype=np.uint32)


def multi_miller_loop_many(equations, final_exp=True):
    """One `multi_miller_loop` per equation (a list of lists of `(&G1Affine, &G2Prepared)` terms) in ONE device call: the bulk
    form of the pattern `E::multi_miller_loop(&terms).final_exponentiation()` of signature verification (pairings.rs:554-603,
    817-824).  Returns a list of `Gt` (final_exp) or `MillerLoopResult`."""
    eqs = [list(e) for e in equations]
    n = sum(len(e) for e in eqs)
    g1 = np.zeros((n, 12), dtype=np.uint64)
    g2 = np.zeros((n, 24), dtype=np.uint64)
    f1 = np.zeros(n, dtype=np.uint8)
    f2 = np.zeros(n, dtype=np.uint8)
    off = np.zeros(len(eqs) + 1, dtype=np.uint64)
    i = 0
    for s, e in enumerate(eqs):
        for p, prep in e:
            g1[i], f1[i], g2[i], f2[i] = p.xy, p.infinity, prep.q.xy, prep.q.infinity
            i += 1
        off[s + 1] = i
    table, qi = _resident_indices([prep for e in eqs for _, prep in e])
    if table is not None:
        out = default_context().multi_miller_loop_prepared_many(g1, f1, table, qi, off, g2, f2, final_exp)
    else:
        out = default_context().multi_miller_loop_many(g1, f1, g2, f2, off, final_exp)
    return [Gt(v) if final_exp else MillerLoopResult(v) for v in out]


def _msm(group, bases, scalars):
    ctx = default_context()
    proj = G1Projective if group == 1 else G2Projective
    if isinstance(bases, ResidentBases):
        return proj(ctx.msm(bases, scalars))
    bases = list(bases)
    if len(bases) != len(scalars):
        raise ValueError("bases and scalars differ in length")
    w = 12 if group == 1 else 24
    xy = np.stack([b.xy for b in bases]) if bases else np.zeros((0, w), dtype=np.uint64)
    inf = np.array([b.infinity for b in bases], dtype=np.uint8)
    return proj(ctx.msm_host(group, xy, inf, scalars))


def msm_g1(bases, scalars):
    """bases.iter().zip(scalars).map(|(p, s)| p * s).sum::<G1Projective>()"""
    return _msm(1, bases, scalars)


def msm_g2(bases, scalars):
    return _msm(2, bases, scalars)


class Bls12:
    """`pairing::Engine` + `MultiMillerLoop` for BLS12-381 (src/pairings.rs:790-824)."""
    Fr, G1, G1Affine, G2, G2Affine, Gt, G2Prepared, Result = Scalar, G1Projective, G1Affine, G2Projective, G2Affine, Gt, G2Prepared, MillerLoopResult

    @staticmethod
    def pairing(p, q): return pairing(p, q)
    @staticmethod
    def multi_miller_loop(terms): return multi_miller_loop(terms)
