"""Fr expression programs (blsgpu_fr_expr_*) in Python integers mod r: an interpreter of the program format of
include/bls12_381_hip.h that applies the rotation / modulo / stride rule literally, and nothing else.

A program is a list of (op, dst, a, b) tuples of integers and operand tuples ("reg", i) / ("col", j, rot) / ("const", i), MOV with b = None;
`words` turns it into the code words independently of the product's assembler.  Columns are lists of integers of length 2^log_len.
The expression is row-local, so `run` evaluates any subset of the rows.
Test infrastructure only: the product never imports this file."""
from oracle import bls12_381_ref as o

RR = o.R_ORDER
MONT = o.FR_MONT_R
ADD, SUB, MUL, MAD, MOV = 0, 1, 2, 3, 4
OPS = {"ADD": ADD, "SUB": SUB, "MUL": MUL, "MAD": MAD, "MOV": MOV}
BLOCK = 256                                                        # fr_expr_plan.h FRX_BLOCK


def shipped_chunk(log_n):
    """fr_expr_plan.h frx_shape: rows per lane (tests/test_simt_fr_expr.py holds this mirror against the plan at every log_n)"""
    return 4 if log_n >= 20 else 2 if log_n == 19 else 1


def operand_word(x):
    kind, idx = x[0], x[1]
    if kind == "reg":
        return idx
    if kind == "col":
        return 0x40000000 | ((x[2] & 0xFFFF) << 8) | idx
    assert kind == "const"
    return 0x80000000 | idx


def words(prog):
    """the code words, n_instr x 3, as a flat list of ints"""
    out = []
    for op, dst, a, b in prog:
        out += [OPS[op] | (dst << 8), operand_word(a), 0 if b is None else operand_word(b)]
    return out


def run(prog, n_regs, consts, cols, col_log_len, log_n, log_stride, rows=None):
    """the result of every row in `rows` (default: all 2^log_n) as integers mod r; cols[j] may be None for a column that is never read"""
    n = 1 << log_n
    out = []
    for i in (range(n) if rows is None else rows):
        regs = [None] * n_regs                                     # None: not written in THIS row -- reading it is a bug of the program

        def val(x):
            if x[0] == "reg":
                assert regs[x[1]] is not None, "register read before it was written"
                return regs[x[1]]
            if x[0] == "const":
                return consts[x[1]]
            j, rot = x[1], x[2]
            length = 1 << (log_n if col_log_len is None else col_log_len[j])
            return cols[j][(i + rot * (1 << log_stride)) % length]

        last = None
        for op, dst, a, b in prog:
            if op == "MOV":
                v = val(a)
            elif op == "ADD":
                v = (val(a) + val(b)) % RR
            elif op == "SUB":
                v = (val(a) - val(b)) % RR
            elif op == "MUL":
                v = val(a) * val(b) % RR
            else:
                assert op == "MAD" and regs[dst] is not None
                v = (regs[dst] + val(a) * val(b)) % RR
            regs[dst] = v
            last = v
        out.append(last)
    return out


def mont(vals):
    return [int(v) % RR * MONT % RR for v in vals]


def mont_words(vals):
    """integers mod r -> (n, 8) u32 Montgomery words"""
    import numpy as np
    b = b"".join((int(v) % RR * MONT % RR).to_bytes(32, "little") for v in vals)
    return np.frombuffer(b, dtype=np.uint32).reshape(-1, 8)


def mont_limbs(vals):
    """integers mod r -> (n, 4) u64 Montgomery limbs"""
    import numpy as np
    return mont_words(vals).view(np.uint64).reshape(-1, 4).copy()


def raw_ints(words_):
    """(..., 8) u32 words or (..., 4) u64 limbs -> the raw 256-bit integers (NOT reduced: a non-canonical output must not compare equal)"""
    import numpy as np
    w = np.ascontiguousarray(words_).view(np.uint8).reshape(-1, 32)
    return [int.from_bytes(row.tobytes(), "little") for row in w]


def from_mont(raw):
    """raw Montgomery integers -> the values mod r"""
    rinv = pow(MONT, -1, RR)
    return [int(v) * rinv % RR for v in raw]


def from_tuples(instrs):
    """the tuples Context.fr_expr takes (bare ints for registers, ("col", j) for an unrotated column, MOV without b) -> this module's form"""
    def operand(x):
        if isinstance(x, int):
            return ("reg", x)
        return (x[0], x[1], x[2] if len(x) == 3 else 0) if x[0] == "col" else (x[0], x[1])
    return [(i[0], i[1], operand(i[2]), operand(i[3]) if len(i) == 4 else None) for i in instrs]


def to_tuples(prog):
    """this module's form -> tuples for Context.fr_expr / fr_expr_assemble"""
    return [(op, dst, a) if b is None else (op, dst, a, b) for op, dst, a, b in prog]


def kind_matrix_program():
    """every op with every pair of operand kinds, REG with itself (a square) and a MAD whose operands include its dst; every result is
    added into register 3, which the last instruction leaves as the row's result.  Columns 0, 1 (column 1 also read at rotation -1),
    constants 0, 1, four registers.  Returns (prog, n_cols, n_regs, n_consts)."""
    R0, R1, R2, ACC = ("reg", 0), ("reg", 1), ("reg", 2), ("reg", 3)
    C0, C1, C1R = ("col", 0, 0), ("col", 1, 0), ("col", 1, -1)
    K0, K1 = ("const", 0), ("const", 1)
    prog = [("MOV", 0, C0, None), ("MOV", 1, K1, None), ("MOV", 3, R0, None)]      # MOV of every kind
    kinds = {"reg": (R0, R1), "col": (C0, C1R), "const": (K0, K1)}
    for op in ("ADD", "SUB", "MUL", "MAD"):
        for ka in ("reg", "col", "const"):
            for kb in ("reg", "col", "const"):
                if op == "MAD":
                    prog.append(("MOV", 2, C1, None))                # MAD reads its dst: give it a value of this row
                prog.append((op, 2, kinds[ka][0], kinds[kb][1]))
                prog.append(("ADD", 3, ACC, R2))
    prog += [("MUL", 2, R1, R1), ("ADD", 3, ACC, R2),                 # a square
             ("MOV", 2, C0, None), ("MAD", 2, R2, R2), ("ADD", 3, ACC, R2),      # dst + dst * dst
             ("MAD", 2, R2, C1), ("MAD", 3, R2, ACC),                 # MAD with its dst as one operand, as the other
             ("SUB", 0, R0, R0), ("SUB", 3, ACC, R0)]                 # x - x = 0
    return prog, 2, 4, 2
