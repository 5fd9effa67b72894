"""The contract of KZG cell recovery (include/bls12_381_hip.h: blsgpu_kzg_recover[_device]) in Python integers over tests/kzg_ref.py and
oracle/bls12_381_ref.py, for the tests of the plan, the host emulation and the GPU.  It touches nothing of the library.

Notation (csrc/kzg_recover_plan.h): n = 2^log_n, l = 2^log_l, c = n / l, w = fr_omega(log_n + 1), cell i the coset h_i <w^(2c)> with
h_i = w^e_i, e_i = residue(i); g = 7.  For one polynomial with M its missing cells:
  Zs(Y) = prod_{i in M} (Y - (w^l)^e_i),   Zd[rho] = Zs((w^l)^rho),   Zc[rho] = Zs(g^l (w^l)^rho)
  EZ[j] = received value at w^j times Zd[j mod 2c], 0 elsewhere
  Q = inverse coset transform of (forward coset transform of (inverse transform of EZ)) / Zc;  ok = Q[n..2n) all zero;  poly = Q[0..n)

  effective / slots          the offsets the kernels walk (the running-maximum rule) and the slot table with the status words
  roots / tables / ez        the stages before the transforms
  stages / recover           every stage's output for a whole call, and the result alone
Test infrastructure only: the product never imports this file."""
import kzg_ref as k
from oracle import bls12_381_ref as o

R = k.R
G = 7                                                             # the reference's GENERATOR (scalar.rs:99-105)
ST_OFFSETS, ST_COL, ST_DUP, ST_FEW = 1, 2, 4, 8                   # kzg_recover_plan.h KZGR_ST_*


def residue(i, log_n, log_l, order):
    return k.coset_shift_exponent(i, log_n, log_l, order)


def cell_of_index(j, log_n, log_l, order):
    """natural index j of the size-2n transform -> (cell number, entry): the inverse of kzg_ref.cell_point_exponent"""
    log_c = log_n - log_l
    rho, row = j & ((2 << log_c) - 1), j >> (log_c + 1)
    return (k.bitrev(rho, log_c + 1), k.bitrev(row, log_l)) if order == k.BITREV else (rho, row)


def effective(offsets, m):
    """(eff, mis) of the running-maximum rule: eff[0] = 0, eff[count] = m, the caller's offsets clamped to m between"""
    count = len(offsets) - 1
    eff, mis, run = [], [], 0
    for i, off in enumerate(offsets):
        v = 0 if i == 0 else m if i == count else min(off, m)
        run = max(run, v)
        eff.append(run)
        mis.append(1 if off != run else 0)
    return eff, mis


def slots(col, offsets, m, log_n, log_l):
    """(slot table count x 2c, status words): slot[v][i] = the index of the received cell numbered i, -1 for a missing one; a polynomial
    with a non-zero status has an all -1 table"""
    c2 = 2 << (log_n - log_l)
    eff, mis = effective(offsets, m)
    table, status = [], []
    for v in range(len(offsets) - 1):
        st, row, got = 0, [-1] * c2, 0
        if mis[v] or mis[v + 1]:
            st = ST_OFFSETS
        else:
            for kk in range(eff[v], eff[v + 1]):
                if col[kk] >= c2:
                    st |= ST_COL
                elif row[col[kk]] >= 0:
                    st |= ST_DUP
                else:
                    row[col[kk]] = kk
                    got += 1
        if got * 2 < c2:
            st |= ST_FEW
        table.append([-1] * c2 if st else row)
        status.append(st)
    return table, status


def roots(log_n, log_l):
    """(rootd, rootc): (w^l)^rho and g^l (w^l)^rho for rho < 2c"""
    c2 = 2 << (log_n - log_l)
    wl = pow(o.fr_omega(log_n + 1), 1 << log_l, R)
    gl = pow(G, 1 << log_l, R)
    rd = [pow(wl, rho, R) for rho in range(c2)]
    return rd, [gl * x % R for x in rd]


def tables(slot_row, status, log_n, log_l, order):
    """(Zd, Zc) of one polynomial, ones for a bad status"""
    c2 = 2 << (log_n - log_l)
    rd, rc = roots(log_n, log_l)
    if status:
        return [1] * c2, [1] * c2
    a = [rd[residue(i, log_n, log_l, order)] for i in range(c2) if slot_row[i] < 0]

    def zs(y):
        acc = 1
        for x in a:
            acc = acc * (y - x) % R
        return acc
    return [zs(y) for y in rd], [zs(y) for y in rc]


def ez(slot_row, cells, zd, log_n, log_l, order):
    """EZ of one polynomial: 2n values; cells[k][t] over ALL received cells of the call"""
    out = []
    c2 = 2 << (log_n - log_l)
    for j in range(2 << log_n):
        i, t = cell_of_index(j, log_n, log_l, order)
        s = slot_row[i]
        out.append(0 if s < 0 else cells[s][t] * zd[j % c2] % R)
    return out


def coset_ntt(x, inverse):
    """blsgpu_fr_ntt_many with coset = g"""
    if inverse:
        y, gi = o.fr_ntt(list(x), inverse=True), pow(G, R - 2, R)
        return [v * pow(gi, j, R) % R for j, v in enumerate(y)]
    return o.fr_ntt([v * pow(G, j, R) % R for j, v in enumerate(x)])


def stages(col, offsets, cells, log_n, log_l, order):
    """every stage of one call: a dict of slot, status, zd, zc (not inverted), ez, scaled (the vector after the scaling), q, polys, ok"""
    m, n, c2 = len(col), 1 << log_n, 2 << (log_n - log_l)
    table, status = slots(col, offsets, m, log_n, log_l)
    res = {"slot": table, "status": status, "zd": [], "zc": [], "ez": [], "scaled": [], "q": [], "polys": [], "ok": []}
    for v, row in enumerate(table):
        zd, zc = tables(row, status[v], log_n, log_l, order)
        e = ez(row, cells, zd, log_n, log_l, order)
        f = coset_ntt(o.fr_ntt(e, inverse=True), False)
        sc = [x * pow(zc[j % c2], R - 2, R) % R for j, x in enumerate(f)]
        q = coset_ntt(sc, True)
        good = status[v] == 0 and not any(q[n:])
        for key, val in (("zd", zd), ("zc", zc), ("ez", e), ("scaled", sc), ("q", q), ("polys", q[:n] if good else [0] * n), ("ok", 1 if good else 0)):
            res[key].append(val)
    return res


def recover(col, offsets, cells, log_n, log_l, order):
    """(polys, ok) of one call"""
    s = stages(col, offsets, cells, log_n, log_l, order)
    return s["polys"], s["ok"]


# ---- inputs the tests share ----------------------------------------------------------------------------------------------------------
def patterns(rng, log_n, log_l):
    """name -> the received cell numbers, in the order they are listed"""
    c = 1 << (log_n - log_l)
    c2 = 2 * c
    perm = list(range(c2))
    for i in range(c2 - 1, 0, -1):
        j = rng.next() % (i + 1)
        perm[i], perm[j] = perm[j], perm[i]
    shuffled = list(range(c2))
    for i in range(c2 - 1, 0, -1):
        j = rng.next() % (i + 1)
        shuffled[i], shuffled[j] = shuffled[j], shuffled[i]
    return {"exactly-c-random": sorted(perm[:c]), "c-plus-1": sorted(perm[:c + 1]), "all": list(range(c2)), "first-half": list(range(c)), "second-half": list(range(c, c2)),
            "every-other": list(range(1, c2, 2)), "shuffled": shuffled[:c + (1 if c > 1 else 0)]}


def special_polys(rng, n, l):
    """the zero polynomial, one of degree < l, coefficients 0 / 1 / r - 1, and a random one"""
    low = [rng.scalar() for _ in range(l)] + [0] * (n - l)
    edge = [(0, 1, R - 1)[i % 3] for i in range(n)]
    return [[0] * n, low, edge, k.random_poly(rng, n)]


def call_inputs(polys, received, log_n, log_l, order):
    """(col, offsets, cells) of a call that lists cells `received[v]` of polys[v]"""
    col, offsets, cells = [], [0], []
    for p, rec in zip(polys, received):
        full = k.cells_by_ntt(p, log_n, log_l, order)
        for i in rec:
            col.append(i)
            cells.append(list(full[i]))
        offsets.append(len(col))
    return col, offsets, cells


def malformed_cases(log_n, log_l, order):
    """(polys, name -> (col, offsets, cells, m, the polynomials that must be bad)): a malformed polynomial between good ones.  Under the
    running-maximum rule a decreasing offset breaks the polynomial it ends and the one it begins, an offset beyond m every polynomial
    behind it"""
    rng = o.SplitMix64(4400 + 64 * log_n + 4 * log_l + order)
    n, l, c = 1 << log_n, 1 << log_l, 1 << (log_n - log_l)
    c2 = 2 * c
    polys = [k.random_poly(rng, n) for _ in range(4)]
    full = [k.cells_by_ntt(p, log_n, log_l, order) for p in polys]

    def call(recs):
        col, offsets, cells = [], [0], []
        for v, rec in enumerate(recs):
            for i in rec:
                col.append(i)
                cells.append(list(full[v][i % c2]))
            offsets.append(len(col))
        return col, offsets, cells

    half, most = list(range(c)), list(range(c2 - 1, c - 2 if c > 1 else -1, -1))
    cases = {}
    col, off, cells = call([half, list(range(c - 1)), most])
    cases["c - 1 cells"] = (col, off, cells, len(col), [1])
    col, off, cells = call([half, list(range(c)) + [0], most])
    cases["a duplicate"] = (col, off, cells, len(col), [1])
    col, off, cells = call([half, list(range(c)) + [c2], most])
    cases["col = 2c"] = (col, off, cells, len(col), [1])
    col, off, cells = call([half, list(range(c)) + [0xFFFFFFFF], most])
    cases["col = 2^32 - 1"] = (col, off, cells, len(col), [1])
    col, off, cells = call([half, half, most, half])
    off2 = list(off)
    off2[2] = off[1] - 1                                           # polynomial 1 ends before it begins: it and the one behind it are broken
    cases["a decreasing offset"] = (col, off2, cells, len(col), [1, 2])
    off3 = list(off)
    off3[2] = len(col) + 5                                          # beyond m: everything from polynomial 1 on is broken
    cases["an offset beyond m"] = (col, off3, cells, len(col), [1, 2, 3])
    return polys, cases
