"""Seeded synthetic inputs for benchmarks and full-size tests.

Scalars are drawn exactly as the survey prescribes: a SplitMix64 stream, 32 random bytes per candidate, top bit
cleared, candidates >= r rejected -- i.e. uniform in [0, r), all 255 bits in play (the top window and its carry
included).  The generator is vectorised with numpy and produces the SAME sequence as the scalar-at-a-time
`oracle.bls12_381_ref.SplitMix64(seed).scalar()` (a CPU test pins that), so small prefixes can be cross-checked
against the oracle while 2^24-element vectors still take well under a second.

Nothing here touches the GPU or the oracle: it only makes bytes.
"""
import numpy as np

R_ORDER = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
SEED = 0xB1512381

_GAMMA = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)
_R_WORDS = np.frombuffer(R_ORDER.to_bytes(32, "little"), dtype="<u8")


def splitmix64(seed, first, count):
    """outputs number first+1 .. first+count of SplitMix64(seed) as a uint64 array (output k = mix(seed + k*gamma))"""
    with np.errstate(over="ignore"):
        k = np.arange(first + 1, first + count + 1, dtype=np.uint64)
        z = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + k * _GAMMA
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        return z ^ (z >> np.uint64(31))


def _lt_r(w):
    lt = np.zeros(len(w), dtype=bool)
    eq = np.ones(len(w), dtype=bool)
    for k in (3, 2, 1, 0):
        lt |= eq & (w[:, k] < _R_WORDS[k])
        eq &= w[:, k] == _R_WORDS[k]
    return lt


def scalars(n, seed=SEED):
    """n scalars uniform in [0, r) as an (n, 32) uint8 array of little-endian canonical bytes (Scalar::to_bytes format)."""
    out = np.zeros((n, 4), dtype="<u8")
    have, used = 0, 0
    while have < n:
        m = max(1024, int((n - have) * 1.12) + 64)            # acceptance rate r / 2^255 = 0.906
        w = splitmix64(seed, used, 4 * m).reshape(m, 4)
        w[:, 3] &= np.uint64(0x7FFFFFFFFFFFFFFF)
        ok = np.flatnonzero(_lt_r(w))
        take = ok[:n - have]
        out[have:have + len(take)] = w[take]
        have += len(take)
        # the stream position after the last candidate that was looked at (accepted or rejected)
        used += 4 * (int(take[-1]) + 1 if have >= n and len(take) else m)
    return out.view(np.uint8).reshape(n, 32)


def to_ints(sb):
    """(n, 32) uint8 little-endian -> list of Python ints"""
    sb = np.ascontiguousarray(sb)
    return [int.from_bytes(sb[i].tobytes(), "little") for i in range(sb.shape[0])]


def dot_mod_r(a_bytes, b_bytes):
    """sum_i a_i * b_i mod r for two (n, 32) byte arrays: the discrete-log side of  MSM(s, [k_i]G) = [sum s_i k_i]G.
    Python big integers, chunked so that 2^24 terms stay in the seconds range."""
    n = a_bytes.shape[0]
    tot = 0
    step = 1 << 16
    for lo in range(0, n, step):
        a = to_ints(a_bytes[lo:lo + step]); b = to_ints(b_bytes[lo:lo + step])
        tot += sum(x * y for x, y in zip(a, b))
    return tot % R_ORDER


def poseidon_test_params(t, r_full, r_partial, seed=SEED):
    """TEST parameters for a Poseidon instance of width t -- NOT the parameters of any standard or deployed instance, and not vetted
    for security.  Returns (constants, mds) as Python ints in [0, r): (r_full + r_partial) rows of t seeded round constants, and the
    t x t Cauchy matrix 1 / (x_i + y_j) over seeded pairwise distinct x_0 .. x_(t-1), y_0 .. y_(t-1) with no x_i + y_j = 0 (every
    square submatrix of a Cauchy matrix is regular, so the sparse form of the partial rounds exists)."""
    need = (r_full + r_partial) * t
    vals = to_ints(scalars(need + 4 * t + 16, (seed ^ (t << 32) ^ (r_full << 40) ^ (r_partial << 48)) & 0xFFFFFFFFFFFFFFFF))
    constants = [vals[r * t:(r + 1) * t] for r in range(r_full + r_partial)]
    xs, ys = [], []
    for v in vals[need:]:
        if len(xs) < t:
            if v not in xs:
                xs.append(v)
        elif len(ys) < t:
            if v not in ys and all((x + v) % R_ORDER for x in xs):
                ys.append(v)
    assert len(xs) == t and len(ys) == t
    mds = [[pow((x + y) % R_ORDER, R_ORDER - 2, R_ORDER) for y in ys] for x in xs]
    return constants, mds


def column_set(c, k, n, seed=SEED):
    """a seeded column set for the fraction scans: c tables of k rows of n scalars, as nested lists of Python ints in [0, r)"""
    vals = to_ints(scalars(c * k * n, (seed ^ (c << 32) ^ (k << 40) ^ (n << 20)) & 0xFFFFFFFFFFFFFFFF))
    return [[vals[(j * k + v) * n:(j * k + v + 1) * n] for v in range(k)] for j in range(c)]


def permutation_with_copy_cycles(c, log_n, seed=SEED, max_cycle=8):
    """a seeded copy-constraint instance for a permutation argument over c wire columns of n = 2^log_n rows: the c n positions are cut
    into cycles of 1 .. max_cycle positions (seeded, scattered over rows and columns), sigma maps a position to the next one of its
    cycle, and every wire value is constant on its cycle.  Returns (wires, ids, sigmas), each c lists of n Python ints: the labels are
    id_j[i] = 7^j w^i with w = 7^((r - 1) / n) (7 generates Fr*, so the cosets 7^j <w> are disjoint for j < 2^32 / n) and
    sigma_j[i] = the id label of sigma(j, i).  With any beta, gamma: prod_{j,i} (w + beta id + gamma) / (w + beta sigma + gamma) = 1."""
    n = 1 << log_n
    total = c * n
    words = splitmix64((seed ^ (c << 32) ^ (log_n << 40)) & 0xFFFFFFFFFFFFFFFF, 0, 2 * total)
    order = np.argsort(words[:total], kind="stable")                 # a seeded shuffle of the positions
    w = pow(7, (R_ORDER - 1) >> log_n, R_ORDER)
    label, acc = [], 1
    for _ in range(n):
        label.append(acc)
        acc = acc * w % R_ORDER
    ident = [[pow(7, j, R_ORDER) * label[i] % R_ORDER for i in range(n)] for j in range(c)]
    values = to_ints(scalars(total, seed ^ 0x5A5A))
    wires = [[0] * n for _ in range(c)]
    sigmas = [[0] * n for _ in range(c)]
    at = 0
    while at < total:
        size = min(1 + int(words[total + at] % np.uint64(max_cycle)), total - at)
        cyc = [int(p) for p in order[at:at + size]]
        for q, p in enumerate(cyc):
            nxt = cyc[(q + 1) % size]
            wires[p // n][p % n] = values[at]
            sigmas[p // n][p % n] = ident[nxt // n][nxt % n]
        at += size
    return wires, ident, sigmas


def lookup_instance(n, seed=SEED):
    """a seeded logUp instance of n rows: a table t of n distinct scalars, n looked-up values f drawn from it (some entries often, some
    never) and the multiplicities m[i] = how often t[i] occurs in f.  Returns (f, t, m) as lists of Python ints; with any gamma that
    meets no -f[i], -t[i]:  sum_i 1 / (gamma + f[i]) - m[i] / (gamma + t[i]) = 0."""
    t = to_ints(scalars(n, seed ^ 0x7AB1E))
    assert len(set(t)) == n
    picks = splitmix64(seed ^ 0x100C, 0, n)
    idx = [int(p % np.uint64(max(n // 3, 1))) * 3 % n for p in picks]        # only every third entry is ever looked up
    m = [0] * n
    for i in idx:
        m[i] += 1
    return [t[i] for i in idx], t, m


def lookup_tuple_instance(rows, n, c, seed=SEED, dup_every=0, miss_every=0):
    """a seeded lookup instance over keys of c scalars: a table of `rows` keys and n looked-up keys, as COLUMN sets (table[j][i] is scalar
    j of row i).  dup_every = d > 0: every d-th table row (i % d == d - 1, i >= d) repeats the key of an EARLIER row at a seeded,
    scattered position; miss_every = m > 0: every m-th looked-up row (i % m == m - 1) is a fresh key that is in no table row.  The other
    looked-up rows are drawn from the table rows (repeated ones included), a third of the rows far more often than the rest.
    Returns (table, f, mult, index, missing) as Python ints: mult[j] = how often the key of row j occurs in f if j is the FIRST table
    row with that key, else 0; index[i] = that first row for f's row i, or 0xFFFFFFFF for a miss; missing = the number of misses."""
    vals = to_ints(scalars((rows + n) * c, seed ^ 0x7AB1E5))
    keys = [tuple(vals[i * c:(i + 1) * c]) for i in range(rows)]
    fresh = [tuple(vals[(rows + i) * c:(rows + i + 1) * c]) for i in range(n)]
    picks = splitmix64(seed ^ 0x100C7, 0, rows + n)
    if dup_every > 0:
        for i in range(dup_every, rows):
            if i % dup_every == dup_every - 1:
                keys[i] = keys[int(picks[i] % np.uint64(i))]
    first = {}
    for j, k in enumerate(keys):
        first.setdefault(k, j)
    assert not any(k in first for k in fresh)
    f, mult, index, missing = [], [0] * rows, [], 0
    hot = max(rows // 3, 1)
    for i in range(n):
        if miss_every > 0 and i % miss_every == miss_every - 1:
            f.append(fresh[i]); index.append(0xFFFFFFFF); missing += 1
            continue
        p = int(picks[rows + i])
        j = (p >> 8) % hot if p & 3 else (p >> 8) % rows
        f.append(keys[j]); index.append(first[keys[j]]); mult[first[keys[j]]] += 1
    cols = lambda ks, m: [[k[j] for k in ks] for j in range(c)] if m else [[] for _ in range(c)]
    return cols(keys, rows), cols(f, n), mult, index, missing


# ---- a vanilla PLONK instance and its quotient expression (blsgpu_fr_expr_*) ---------------------------------------------------------
# the column map of plonk_quotient_program: full-length columns first, then the periodic one, then the challenges (length 1)
PLONK_COLS = {name: j for j, name in enumerate(
    ["a", "b", "c", "qL", "qR", "qO", "qM", "qC", "s1", "s2", "s3", "z", "X", "L1", "zh_inv", "beta", "gamma", "alpha", "alpha2"])}
PLONK_K = (1, 7, 49)                      # the coset labels of the three wire columns: id_j = k_j X (permutation_with_copy_cycles)


def plonk_instance(log_n, seed=SEED):
    """a seeded SATISFYING vanilla-PLONK instance on the domain of n = 2^log_n rows, as a dict of lists of n Python ints in [0, r):
    wires a, b, c with copy constraints (permutation_with_copy_cycles), their sigma columns s1, s2, s3 (labels k_j w^i, k = PLONK_K),
    seeded selectors qL, qR, qO, qM and the qC that satisfies  qL a + qR b + qO c + qM a b + qC = 0  in every row, and the permutation
    accumulator z (z[0] = 1, z[i + 1] = z[i] prod_j (w_j + beta k_j w^i + gamma) / (w_j + beta s_j + gamma)[i], closing at z[n] = 1);
    "beta", "gamma", "alpha" are ints."""
    n = 1 << log_n
    (a, b, c), ident, (s1, s2, s3) = permutation_with_copy_cycles(3, log_n, seed)
    sel = to_ints(scalars(4 * n + 3, seed ^ 0x5E1EC7))
    qL, qR, qO, qM = (sel[i * n:(i + 1) * n] for i in range(4))
    beta, gamma, alpha = sel[4 * n:]
    qC = [-(qL[i] * a[i] + qR[i] * b[i] + qO[i] * c[i] + qM[i] * a[i] * b[i]) % R_ORDER for i in range(n)]
    z, acc = [], 1
    for i in range(n):
        z.append(acc)
        num = den = 1
        for w, idc, sg in ((a, ident[0], s1), (b, ident[1], s2), (c, ident[2], s3)):
            num = num * (w[i] + beta * idc[i] + gamma) % R_ORDER
            den = den * (w[i] + beta * sg[i] + gamma) % R_ORDER
        acc = acc * num % R_ORDER * pow(den, R_ORDER - 2, R_ORDER) % R_ORDER
    assert acc == 1, "the permutation product does not close"
    return {"a": a, "b": b, "c": c, "qL": qL, "qR": qR, "qO": qO, "qM": qM, "qC": qC, "s1": s1, "s2": s2, "s3": s3, "z": z,
            "beta": beta, "gamma": gamma, "alpha": alpha}


def plonk_quotient_program():
    """the standard program over PLONK_COLS:
        (qL a + qR b + qO c + qM a b + qC  +  alpha perm  +  alpha^2 (z - 1) L1) * zh_inv
        perm = z prod_j (w_j + beta k_j X + gamma)  -  z(next row) prod_j (w_j + beta s_j + gamma)
    Returns (n_cols, n_regs, consts, instrs) for Context.fr_expr: constants (k_1, k_2, 1) = (7, 49, 1) as ints, instructions as
    tuples for fr_expr_assemble.  21 field products per row; the next row is rotation +1 (times 2^log_stride on an extended domain)."""
    C = lambda name, rot=0: ("col", PLONK_COLS[name], rot)
    K1, K2, ONE = ("const", 0), ("const", 1), ("const", 2)
    ins = [("MUL", 0, C("qL"), C("a")), ("MAD", 0, C("qR"), C("b")), ("MAD", 0, C("qO"), C("c")), ("MUL", 1, C("qM"), C("a")), ("MAD", 0, 1, C("b")),
           ("ADD", 0, 0, C("qC")),
           ("MUL", 1, C("beta"), C("X")),
           ("ADD", 2, C("a"), C("gamma")), ("ADD", 2, 2, 1),
           ("MUL", 3, 1, K1), ("ADD", 3, 3, C("b")), ("ADD", 3, 3, C("gamma")), ("MUL", 2, 2, 3),
           ("MUL", 3, 1, K2), ("ADD", 3, 3, C("c")), ("ADD", 3, 3, C("gamma")), ("MUL", 2, 2, 3),
           ("MUL", 2, 2, C("z")),
           ("MUL", 3, C("beta"), C("s1")), ("ADD", 3, 3, C("a")), ("ADD", 3, 3, C("gamma")),
           ("MUL", 4, C("beta"), C("s2")), ("ADD", 4, 4, C("b")), ("ADD", 4, 4, C("gamma")), ("MUL", 3, 3, 4),
           ("MUL", 4, C("beta"), C("s3")), ("ADD", 4, 4, C("c")), ("ADD", 4, 4, C("gamma")), ("MUL", 3, 3, 4),
           ("MUL", 3, 3, C("z", 1)),
           ("SUB", 2, 2, 3),
           ("MAD", 0, C("alpha"), 2),
           ("SUB", 1, C("z"), ONE), ("MUL", 1, 1, C("L1")),
           ("MAD", 0, C("alpha2"), 1),
           ("MUL", 0, 0, C("zh_inv"))]
    return len(PLONK_COLS), 5, [PLONK_K[1], PLONK_K[2], 1], ins


def plonk_col_log_len(log_n, log_stride):
    """col_log_len of the PLONK_COLS map on an extended domain of 2^log_n rows: zh_inv has 2^log_stride values, the challenges one"""
    ll = [log_n] * len(PLONK_COLS)
    ll[PLONK_COLS["zh_inv"]] = log_stride
    for name in ("beta", "gamma", "alpha", "alpha2"):
        ll[PLONK_COLS[name]] = 0
    return ll
