"""The Fr fraction scans (blsgpu_fr_grand_product / blsgpu_fr_frac_sum) in Python integers mod r: the defining formulas, nothing else.

A column set is a list of c tables, a table a list of k rows, a row a list of len integers; None stands for a NULL set.
Test infrastructure only: the product never imports this file."""
from oracle import bls12_381_ref as o

RR = o.R_ORDER
MONT = o.FR_MONT_R


def inv0(x):
    x %= RR
    return pow(x, -1, RR) if x else 0


def _factor(a, b, j, v, i, beta, gamma):
    return (a[j][v][i] + (beta * b[j][v][i] if b is not None else 0) + gamma) % RR


def _scan(f, product, exclusive):
    out = []
    for row in f:
        acc = 1 if product else 0
        res = []
        for x in row:
            nxt = acc * x % RR if product else (acc + x) % RR
            res.append(acc if exclusive else nxt)
            acc = nxt
        out.append(res)
    return out


def grand_product(num_a, num_b, den_a, den_b, beta, gamma, exclusive=False):
    """-> (out rows, flag rows)"""
    c, k, n = len(num_a), len(num_a[0]), len(num_a[0][0])
    f, flags = [], []
    for v in range(k):
        fr, fl = [], []
        for i in range(n):
            nn, dd, ok = 1, 1, 1
            for j in range(c):
                nn = nn * _factor(num_a, num_b, j, v, i, beta, gamma) % RR
                d = _factor(den_a, den_b, j, v, i, beta, gamma)
                ok &= 1 if d else 0
                dd = dd * d % RR
            fr.append(nn * inv0(dd) % RR)
            fl.append(ok)
        f.append(fr)
        flags.append(fl)
    return _scan(f, True, exclusive), flags


def frac_sum(mult, den_a, den_b, beta, gamma, exclusive=False):
    """-> (out rows, flag rows)"""
    c, k, n = len(den_a), len(den_a[0]), len(den_a[0][0])
    f, flags = [], []
    for v in range(k):
        fr, fl = [], []
        for i in range(n):
            s, ok = 0, 1
            for j in range(c):
                d = _factor(den_a, den_b, j, v, i, beta, gamma)
                ok &= 1 if d else 0
                s = (s + (mult[j][v][i] if mult is not None else 1) * inv0(d)) % RR
            fr.append(s)
            fl.append(ok)
        f.append(fr)
        flags.append(fl)
    return _scan(f, False, exclusive), flags


def mont_words(vals):
    """integers mod r -> (n, 8) u32 Montgomery words"""
    import numpy as np
    b = b"".join((int(v) % RR * MONT % RR).to_bytes(32, "little") for v in vals)
    return np.frombuffer(b, dtype=np.uint32).reshape(-1, 8)


def raw_ints(words):
    """(..., 8) u32 words -> the raw 256-bit integers (NOT reduced: a non-canonical output must not compare equal)"""
    import numpy as np
    w = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, 8)
    return [int.from_bytes(row.tobytes(), "little") for row in w]


def mont(vals):
    return [int(v) % RR * MONT % RR for v in vals]


def pack_set(tables, pitch=None, poison=None):
    """a column set -> ((c - 1) * pitch + k * len, 8) u32 words, table j at j * pitch; the gaps hold `poison` (an integer) or zeros"""
    import numpy as np
    c, k, n = len(tables), len(tables[0]), len(tables[0][0])
    total = k * n
    pitch = total if pitch is None else pitch
    out = np.zeros(((c - 1) * pitch + total, 8), dtype=np.uint32)
    if poison is not None and len(out):
        out[:] = mont_words([poison])[0]
    for j, t in enumerate(tables):
        out[j * pitch:j * pitch + total] = mont_words([x for row in t for x in row])
    return out
