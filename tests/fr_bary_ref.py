"""What blsgpu_fr_bary_eval_many / blsgpu_fr_bary_open_many must return, in Python integers and by the DEFINITION: interpolate the row
(oracle fr_ntt, inverse), evaluate by Horner, divide by (X - z) synthetically, transform the quotient back -- no barycentric formula here.
Shared by tests/test_simt_fr_bary.py and tests/test_fr_bary.py.  Test infrastructure only."""
import numpy as np

from oracle import bls12_381_ref as o

RR = o.R_ORDER
MONT = o.FR_MONT_R
NATURAL, BITREV = 0, 1


def bitrev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


def exponents(log_n, order):
    """e[i] with D[i] = w^e[i]"""
    n = 1 << log_n
    return [bitrev(i, log_n) for i in range(n)] if order == BITREV else list(range(n))


def domain_point(log_n, order, j):
    return pow(o.fr_omega(log_n), exponents(log_n, order)[j], RR)


def expect(f, z, order):
    """(y, q) of one row f (n integers mod r, in the given order) at the point z"""
    n = len(f)
    log_n = n.bit_length() - 1
    e = exponents(log_n, order)
    nat = [0] * n
    for i in range(n):
        nat[e[i]] = f[i] % RR
    c = o.fr_ntt(nat, inverse=True) if n > 1 else list(nat)
    qc = [0] * n
    acc = 0
    for i in range(n - 1, -1, -1):                                 # acc_i = c_i + z acc_(i+1): y = acc_0, the quotient's coefficient i - 1 is acc_i
        acc = (c[i] + z * acc) % RR
        if i:
            qc[i - 1] = acc
    qn = o.fr_ntt(qc) if n > 1 else [0]
    return acc, [qn[e[i]] for i in range(n)]


def words(vals):
    """integers mod r -> (len, 8) u32 Montgomery words"""
    b = b"".join((int(v) % RR * MONT % RR).to_bytes(32, "little") for v in vals)
    return np.frombuffer(b, dtype=np.uint32).reshape(-1, 8)


def raw_ints(w):
    """(..., 8) u32 words -> the raw 256-bit integers (NOT reduced: a non-canonical output must not compare equal)"""
    w = np.ascontiguousarray(w, dtype=np.uint32).reshape(-1, 8)
    return [int.from_bytes(row.tobytes(), "little") for row in w]


def mont(vals):
    return [int(v) % RR * MONT % RR for v in vals]
