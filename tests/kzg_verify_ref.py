"""The contract of batched KZG cell-proof verification (include/bls12_381_hip.h: blsgpu_kzg_verify_cells*) in Python integers, in the
group-as-scalars model of tests/kzg_ref.py: commitments, proofs, S[u] and q are SCALARS standing for multiples of the generators, so
A_s and B_s are scalars and verdict = (A_s T - B_s) mod r == 0 with q = [T] G2.  It touches nothing of the library.

  interpolate / interpolate_direct   I_k by the identity I[u] = h^(-u) INTT_l(v)[u] / by Lagrange's formula on the cell's own points
  weights / aggregate / batch        rho_k and rho_k a_k, agg[s][u], (A_s, B_s, verdict) -- the stages the host emulation compares one by one
  honest / consistent                the two kinds of input whose verdict is 1 by construction
Test infrastructure only: the product never imports this file."""
import kzg_ref as k
from oracle import bls12_381_ref as o

R = k.R
NATURAL, BITREV = k.NATURAL, k.BITREV


def shift(col, log_n, log_l, order):
    """h_col"""
    return pow(o.fr_omega(log_n + 1), k.coset_shift_exponent(col, log_n, log_l, order), R)


def natural_cell(cell, log_l, order):
    """v: the cell in natural coset order, v[i] the value at h g^i"""
    return [cell[k.bitrev(i, log_l)] for i in range(len(cell))] if order == BITREV else list(cell)


def interpolate(cell, col, log_n, log_l, order):
    """the l coefficients of I: degree < l, I = cell[t] at entry t of cell `col`"""
    c = o.fr_ntt(natural_cell(cell, log_l, order), inverse=True) if log_l else list(cell)
    hinv = pow(shift(col, log_n, log_l, order), R - 2, R)
    return [v * pow(hinv, u, R) % R for u, v in enumerate(c)]


def interpolate_direct(cell, col, log_n, log_l, order):
    """the same by Lagrange's formula over the points kzg_ref.cell_point_exponent names: O(l^2), no transform, no coset identity"""
    w = o.fr_omega(log_n + 1)
    xs = [pow(w, k.cell_point_exponent(col, t, log_n, log_l, order), R) for t in range(1 << log_l)]
    out = [0] * len(xs)
    for i, xi in enumerate(xs):
        num, den = [1], 1                                          # prod_{j != i} (X - x_j), prod (x_i - x_j)
        for j, xj in enumerate(xs):
            if j != i:
                num = [((num[d - 1] if d else 0) - xj * (num[d] if d < len(num) else 0)) % R for d in range(len(num) + 1)]
                den = den * (xi - xj) % R
        f = cell[i] * pow(den, R - 2, R) % R
        out = [(a + f * b) % R for a, b in zip(out, num)]
    return out


def weights(col, offsets, r, log_n, log_l, order):
    """(rho, rho a) per cell"""
    rho, rhoa = [], []
    for s in range(len(offsets) - 1):
        for kk in range(offsets[s], offsets[s + 1]):
            x = pow(r[s], kk - offsets[s], R)
            rho.append(x)
            rhoa.append(x * pow(shift(col[kk], log_n, log_l, order), 1 << log_l, R) % R)
    return rho, rhoa


def aggregate(col, cells, offsets, r, log_n, log_l, order):
    """agg[s][u] = sum_k rho_k I_k[u]"""
    rho, _ = weights(col, offsets, r, log_n, log_l, order)
    out = []
    for s in range(len(offsets) - 1):
        acc = [0] * (1 << log_l)
        for kk in range(offsets[s], offsets[s + 1]):
            acc = [(a + rho[kk] * b) % R for a, b in zip(acc, interpolate(cells[kk], col[kk], log_n, log_l, order))]
        out.append(acc)
    return out


def batch(commits, row, col, cells, proofs, offsets, r, sigma, T, log_n, log_l, order):
    """[(A_s, B_s, verdict)] by the definition"""
    rho, rhoa = weights(col, offsets, r, log_n, log_l, order)
    agg = aggregate(col, cells, offsets, r, log_n, log_l, order)
    out = []
    for s in range(len(offsets) - 1):
        ks = range(offsets[s], offsets[s + 1])
        A = sum(rho[kk] * proofs[kk] for kk in ks) % R
        B = (sum(rho[kk] * commits[row[kk]] + rhoa[kk] * proofs[kk] for kk in ks) - sum(a * sg for a, sg in zip(agg[s], sigma))) % R
        out.append((A, B, 1 if (A * T - B) % R == 0 else 0))
    return out


def honest(rng, log_n, log_l, order, nrows, row, col):
    """powers of tau: (commits, cells, proofs, sigma[0..l), T) for the cells (row[k], col[k]) of nrows random polynomials"""
    n, l = 1 << log_n, 1 << log_l
    tau = rng.scalar()
    sigma = [pow(tau, u, R) for u in range(n)]
    polys = [k.random_poly(rng, n) for _ in range(nrows)]
    all_cells = [k.cells_by_ntt(p, log_n, log_l, order) for p in polys]
    all_proofs = [k.proofs_by_division(p, sigma, log_n, log_l, order) for p in polys]
    commits = [k.evaluate(p, tau) for p in polys]
    return commits, [all_cells[i][j] for i, j in zip(row, col)], [all_proofs[i][j] for i, j in zip(row, col)], sigma[:l], pow(tau, l, R)


def consistent(rng, log_n, log_l, order, col, offsets, r, zero_sigma=0, zero_proof=None):
    """an arbitrary SRS: sigma_u independent with sigma[zero_sigma] = 0, T, the proofs and the cells random; batch s has ONE commitment,
    row s, solved from the equation: C = (A T - rest) / sum rho.  The verdict of every batch with sum rho != 0 is 1 by the definition.
    Returns (commits, row, cells, proofs, sigma, T)."""
    l, m, nseg = 1 << log_l, len(col), len(offsets) - 1
    sigma = [rng.scalar() for _ in range(l)]
    sigma[zero_sigma % l] = 0
    T = rng.scalar()
    proofs = [rng.scalar() for _ in range(m)]
    if zero_proof is not None and m:
        proofs[zero_proof % m] = 0
    cells = [[rng.scalar() for _ in range(l)] for _ in range(m)]
    row = [s for s in range(nseg) for _ in range(offsets[s], offsets[s + 1])]
    rho, _ = weights(col, offsets, r, log_n, log_l, order)
    zero = batch([0] * nseg, row, col, cells, proofs, offsets, r, sigma, T, log_n, log_l, order)
    commits = []
    for s in range(nseg):
        tot = sum(rho[offsets[s]:offsets[s + 1]]) % R
        A, rest, _ = zero[s]
        commits.append((A * T - rest) * pow(tot, R - 2, R) % R if tot else 0)
    return commits, row, cells, proofs, sigma, T
