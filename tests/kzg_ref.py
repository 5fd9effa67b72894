"""The contract of the amortised KZG openings (include/bls12_381_hip.h: blsgpu_kzg_multiproof_*, blsgpu_kzg_cells*) in Python integers
over oracle/bls12_381_ref.py, for the tests of the plan, the host emulation and the GPU.  It touches nothing of the library.

Notation: n = 2^log_n coefficients, l = 2^log_l points per cell, c = n / l, w = fr_omega(log_n + 1) of order 2n.  The SRS is a list of
n SCALARS sigma_m standing for the points S[m] = [sigma_m] G1 (the "group as scalars" model: every group operation of the pipeline
becomes the same operation mod r), so a proof is the scalar Sum_u q_i[u] sigma_u and the expected point is [that] G1.

  cosets / cells / proofs_by_division   the definition: q_i = floor(p / (X^l - a_i)) by the recurrence q_i[u] = p[u + l] + a_i q_i[u + l]
  h_vector / proofs_by_h                the h_d form: proofs (natural order) = NTT_2c(h_0 .. h_{c-1}, 0 x c)
  srs_rows / coeff_rows / pipeline      the circulant route stage by stage, as csrc/kzg_plan.h orders it
Test infrastructure only: the product never imports this file."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import bls12_381_ref as o                            # noqa: E402

R = o.R_ORDER
NATURAL, BITREV = 0, 1                                           # BLSGPU_FR_ORDER_*
COEFFS, EVALS = 0, 1                                             # BLSGPU_KZG_FORM_*


def bitrev(i, bits):
    r = 0
    for b in range(bits):
        r |= ((i >> b) & 1) << (bits - 1 - b)
    return r


def coset_shift_exponent(i, log_n, log_l, order):
    """e with h_i = w^e"""
    return bitrev(i, log_n + 1 - log_l) if order == BITREV else i


def cell_point_exponent(i, t, log_n, log_l, order):
    """e with entry t of cell i = w^e"""
    c2 = 2 << (log_n - log_l)
    return bitrev((i << log_l) + t, log_n + 1) if order == BITREV else i + c2 * t


def evaluate(p, x):
    acc = 0
    for a in reversed(p):
        acc = (acc * x + a) % R
    return acc


def cells(p, log_n, log_l, order):
    """cells[i][t] by direct evaluation"""
    w = o.fr_omega(log_n + 1)
    return [[evaluate(p, pow(w, cell_point_exponent(i, t, log_n, log_l, order), R)) for t in range(1 << log_l)] for i in range(2 << (log_n - log_l))]


def cells_by_ntt(p, log_n, log_l, order):
    """the same through E = the size-2n transform of p zero-extended"""
    E = o.fr_ntt(list(p) + [0] * len(p))
    return [[E[cell_point_exponent(i, t, log_n, log_l, order)] for t in range(1 << log_l)] for i in range(2 << (log_n - log_l))]


def quotient(p, log_l, a):
    """floor(p / (X^l - a)): n - l coefficients"""
    n, l = len(p), 1 << log_l
    q = [0] * n                                                  # q[u] for u < n - l, zero beyond
    for u in range(n - l - 1, -1, -1):
        q[u] = (p[u + l] + a * (q[u + l] if u + l < n - l else 0)) % R
    return q[:n - l]


def proofs_by_division(p, sigma, log_n, log_l, order):
    """proofs[i] as the scalar Sum_u q_i[u] sigma_u"""
    w = o.fr_omega(log_n + 1)
    out = []
    for i in range(2 << (log_n - log_l)):
        a = pow(w, coset_shift_exponent(i, log_n, log_l, order) << log_l, R)
        q = quotient(p, log_l, a)
        out.append(sum(x * s for x, s in zip(q, sigma)) % R)
    return out


def h_vector(p, sigma, log_n, log_l):
    l, c = 1 << log_l, 1 << (log_n - log_l)
    return [sum(p[(s + d + 1) * l + t] * sigma[s * l + t] for s in range(c - 1 - d) for t in range(l)) % R for d in range(c)]


def proofs_by_h(p, sigma, log_n, log_l, order):
    c = 1 << (log_n - log_l)
    nat = o.fr_ntt(h_vector(p, sigma, log_n, log_l) + [0] * c)
    return [nat[coset_shift_exponent(i, log_n, log_l, order)] for i in range(2 * c)]


# ---- the circulant route, stage by stage ---------------------------------------------------------------------------------------------
def srs_rows(sigma, log_n, log_l):
    """S^_t for t < l: 2c entries, an SRS index or None for the identity"""
    l, c = 1 << log_l, 1 << (log_n - log_l)
    return [[(c - 2 - j) * l + t if j <= c - 2 else None for j in range(2 * c)] for t in range(l)]


def coeff_rows(log_n, log_l):
    """c^_t for t < l: 2c entries, a coefficient index or None for zero"""
    l, c = 1 << log_l, 1 << (log_n - log_l)
    rows = []
    for t in range(l):
        row = [(c - 1) * l + t] + [None] * (c + 1) + [j * l + t for j in range(1, c - 1)]
        rows.append(row[:2 * c] if c > 1 else [None, None])
    return rows


def xhat(sigma, log_n, log_l):
    """X^ laid out [m][t] (the handle's base set), as scalars"""
    rows = [o.fr_ntt([0 if s is None else sigma[s] for s in row]) for row in srs_rows(sigma, log_n, log_l)]
    l, c2 = 1 << log_l, 2 << (log_n - log_l)
    return [rows[t][m] for m in range(c2) for t in range(l)]


def segment_scalars(p, log_n, log_l):
    """the scalars of the Toeplitz MSM in segment order [m][t]"""
    rows = [o.fr_ntt([0 if s is None else p[s] for s in row]) for row in coeff_rows(log_n, log_l)]
    l, c2 = 1 << log_l, 2 << (log_n - log_l)
    return [rows[t][m] for m in range(c2) for t in range(l)]


def pipeline(p, sigma, log_n, log_l, order):
    """proofs through every stage of the circulant route, as scalars"""
    l, c = 1 << log_l, 1 << (log_n - log_l)
    if c == 1:
        return [0, 0]
    X, f = xhat(sigma, log_n, log_l), segment_scalars(p, log_n, log_l)
    seg = [sum(f[m * l + t] * X[m * l + t] for t in range(l)) % R for m in range(2 * c)]
    h = o.fr_ntt(seg, inverse=True)
    nat = o.fr_ntt(h[:c] + [0] * c)
    return [nat[coset_shift_exponent(i, log_n, log_l, order)] for i in range(2 * c)]


def to_evals(p, order):
    """the n values of p on <w^2> in `order`, as blsgpu_fr_bary_* reads them"""
    v = o.fr_ntt(list(p))
    log_n = len(p).bit_length() - 1
    return [v[bitrev(i, log_n)] for i in range(len(p))] if order == BITREV else v


def random_poly(rng, n):
    return [rng.scalar() for _ in range(n)]
