"""The Fr lookup tables (blsgpu_fr_lookup_*) over Python integers: a dict from key tuples to the first table row that holds the key.
What tests/test_simt_fr_lookup.py, tests/test_fr_lookup.py and tools/fr_lookup_time.py compare the kernels against.

A table and the looked-up rows are COLUMN sets here as in the library: `cols[j][i]` is scalar j of row i, a key is the tuple
(cols[0][i], ..., cols[c - 1][i]).  Test infrastructure only: the product never imports this file."""
from oracle import bls12_381_ref as o

RR = o.R_ORDER
MONT = o.FR_MONT_R
MISS = 0xFFFFFFFF                                                  # BLSGPU_FR_LOOKUP_MISS
LDS_ROWS = 4096                                                    # BLSGPU_FR_LOOKUP_LDS_ROWS
BLOCK = 256                                                        # fr_lookup_plan.h FRL_BLOCK


def keys(cols):
    """column set -> the list of key tuples, one per row"""
    return list(zip(*cols)) if cols and len(cols[0]) else []


def slots(rows):
    """fr_lookup_plan.h frl_slots: the power of two >= 2 * rows"""
    s = 2
    while s < 2 * rows:
        s *= 2
    return s


def count(table, f):
    """table, f: column sets of the same width.  Returns (mult, index, missing, distinct): mult[j] = how many rows of f equal row j of the
    table if j is the FIRST row with that key, else 0; index[i] = the first table row equal to row i of f, or MISS"""
    first = {}
    tk = keys(table)
    for j, k in enumerate(tk):
        first.setdefault(k, j)
    mult, index, missing = [0] * len(tk), [], 0
    for k in keys(f):
        j = first.get(k)
        if j is None:
            missing += 1
            index.append(MISS)
        else:
            mult[j] += 1
            index.append(j)
    return mult, index, missing, len(first)


def mult_scalars(mult, negate=False):
    """the counts as the integers mod r the multiplicity column holds (r - m with negate, 0 stays 0)"""
    return [(-m) % RR if negate else m % RR for m in mult]


def mont_words(vals):
    """integers mod r -> (n, 8) u32 Montgomery words"""
    import numpy as np
    b = b"".join((int(v) % RR * MONT % RR).to_bytes(32, "little") for v in vals)
    return np.frombuffer(b, dtype=np.uint32).reshape(-1, 8).copy()


def mont_limbs(vals):
    """integers mod r -> (n, 4) u64 Montgomery limbs"""
    import numpy as np
    return mont_words(vals).view(np.uint64).reshape(-1, 4).copy()


def set_limbs(cols):
    """column set of integers -> (c, n, 4) u64 Montgomery limbs"""
    import numpy as np
    if not len(cols[0]):
        return np.zeros((len(cols), 0, 4), dtype=np.uint64)
    return np.stack([mont_limbs(col) for col in cols])


def raw_ints(words_):
    """(..., 8) u32 words or (..., 4) u64 limbs -> the raw 256-bit integers (NOT reduced: a non-canonical output must not compare equal)"""
    import numpy as np
    w = np.ascontiguousarray(words_).view(np.uint8).reshape(-1, 32)
    return [int.from_bytes(row.tobytes(), "little") for row in w]


def mult_raw(mult, negate=False):
    """what the mult output must hold, as raw 256-bit integers: the canonical Montgomery form of the counts"""
    return [v * MONT % RR for v in mult_scalars(mult, negate)]
