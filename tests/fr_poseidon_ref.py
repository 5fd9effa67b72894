"""The Poseidon permutation over Fr by its textbook definition, in Python integers (test infrastructure only).

Independent of the sparse form the library derives: every round adds the round constants, raises to the fifth power with pow(x, 5, r)
(every element in a full round, element 0 in a partial one) and multiplies by the matrix.  Values are plain integers in [0, r);
`mont` / `words` give the canonical Montgomery limbs the library reads and writes, so comparisons are limb for limb."""
import numpy as np

RR = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
R_MONT = (1 << 256) % RR
R_INV = pow(R_MONT, RR - 2, RR)


def permute(state, t, r_full, r_partial, constants, mds):
    s = [int(x) % RR for x in state]
    assert len(s) == t and len(constants) == r_full + r_partial
    half = r_full // 2
    for r in range(r_full + r_partial):
        s = [(x + c) % RR for x, c in zip(s, constants[r])]
        if r < half or r >= half + r_partial:
            s = [pow(x, 5, RR) for x in s]
        else:
            s[0] = pow(s[0], 5, RR)
        s = [sum(m * x for m, x in zip(row, s)) % RR for row in mds]
    return s


def hash_one(tag, xs, t, r_full, r_partial, constants, mds):
    return permute([tag] + list(xs), t, r_full, r_partial, constants, mds)[1]


def merkle(tag, leaves, height, k, t, r_full, r_partial, constants, mds):
    """k trees of (t-1)^height leaves, tree after tree -> (levels, roots): levels[l - 1] = level l of all trees, tree-major"""
    a = t - 1
    assert len(leaves) == k * a ** height
    cur, levels = list(leaves), []
    for _ in range(height):
        cur = [hash_one(tag, cur[i * a:(i + 1) * a], t, r_full, r_partial, constants, mds) for i in range(len(cur) // a)]
        levels.append(cur)
    return levels, cur


def mont(vals):
    """integers -> their Montgomery form as integers"""
    return [(int(v) * R_MONT) % RR for v in vals]


def words(vals):
    """integers in [0, r) -> (n, 8) u32 words of their canonical Montgomery limbs"""
    out = np.zeros((len(vals), 8), dtype=np.uint32)
    for i, v in enumerate(mont(vals)):
        for w in range(8):
            out[i, w] = (v >> (32 * w)) & 0xFFFFFFFF
    return out


def limbs(vals):
    """integers in [0, r) -> (n, 4) u64 Montgomery limbs"""
    return words(vals).view(np.uint64).reshape(len(vals), 4)


def raw_ints(w):
    """(n, 8) u32 or (n, 4) u64 limbs -> the integers the limbs spell (NOT reduced: a non-canonical output stays visible)"""
    a = np.ascontiguousarray(w)
    a = a.view(np.uint32).reshape(-1, 8)
    return [sum(int(a[i, j]) << (32 * j) for j in range(8)) for i in range(a.shape[0])]
