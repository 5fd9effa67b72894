"""The definition of blsgpu_fr_lagrange_segments in Python integers mod r, and the edge-case calls its suites share (tests/test_simt_fr_lagrange.py,
tests/test_fr_lagrange.py, tests/test_lagrange_combine.py).  The reference is the formula of include/bls12_381_hip.h and nothing else:

    N_i = prod_{j != i} (z - x_j)      D_i = prod_{j != i} (x_i - x_j)      lambda_i = N_i * inv0(D_i)      y = sum_i lambda_i v_i

literally the double product, with pow(D, -1, r) and inv0(0) = 0.  Test infrastructure only: the product never imports this file."""
import random

import numpy as np

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
MONT = (1 << 256) % R
MONT_INV = pow(MONT, -1, R)


def inv0(v):
    return pow(v, -1, R) if v % R else 0


def lagrange(nodes, z):
    """(the coefficients, the distinct flag) of one segment"""
    lam, distinct = [], 1
    for i, xi in enumerate(nodes):
        n = d = 1
        for j, xj in enumerate(nodes):
            if j != i:
                n = n * (z - xj) % R
                d = d * (xi - xj) % R
        if d == 0:
            distinct = 0
        lam.append(n * inv0(d) % R)
    return lam, distinct


def interpolate(lam, values):
    return sum(l * v for l, v in zip(lam, values)) % R


# ---- Montgomery limbs ----------------------------------------------------------------------------------------------------------
def to_limbs(ints):
    """integers mod r -> (n, 4) u64 canonical Montgomery limbs"""
    out = np.zeros((len(ints), 4), dtype=np.uint64)
    for k, v in enumerate(ints):
        m = v % R * MONT % R
        for i in range(4):
            out[k, i] = (m >> (64 * i)) & 0xFFFFFFFFFFFFFFFF
    return out


def from_limbs(a):
    a = np.asarray(a, dtype=np.uint64).reshape(-1, 4)
    return [sum(int(a[k, i]) << (64 * i) for i in range(4)) * MONT_INV % R for k in range(a.shape[0])]


# ---- the edge call ----------------------------------------------------------------------------------------------------------------
# every scenario a segment of the edge call can take; (name, least length)
SCENARIOS = (("plain", 0), ("z zero", 1), ("z on first", 1), ("z on middle", 1), ("z on last", 1), ("node 0 with z 0", 1), ("repeat adjacent", 2),
             ("repeat at both ends", 2), ("repeat across tiles", 2), ("z on repeated", 2), ("small ids", 1))
LONG = 300                                                         # from this length on a segment takes only the LONG_SCENARIOS (the formula is t^2 big-integer products)
LONG_SCENARIOS = ("plain", "z on middle", "repeat at both ends", "repeat across tiles", "z on repeated")


def segment(t, scenario, tile, rng):
    """(nodes, z, values) of one segment of t nodes"""
    nodes = []
    seen = set()
    while len(nodes) < t:
        v = rng.randrange(1, R)
        if v not in seen:
            seen.add(v); nodes.append(v)
    z = rng.randrange(1, R)
    while z in seen:
        z = rng.randrange(1, R)
    if scenario == "z zero":
        z = 0
    elif scenario == "z on first":
        z = nodes[0]
    elif scenario == "z on middle":
        z = nodes[t // 2]
    elif scenario == "z on last":
        z = nodes[t - 1]
    elif scenario == "node 0 with z 0":
        nodes[t // 3] = 0; z = 0
    elif scenario == "repeat adjacent":
        nodes[t // 2] = nodes[t // 2 - 1]
    elif scenario == "repeat at both ends":
        nodes[t - 1] = nodes[0]
    elif scenario == "repeat across tiles":
        a = min(1, t - 2)
        nodes[min(a + tile, t - 1)] = nodes[a]
    elif scenario == "z on repeated":
        nodes[t - 1] = nodes[(t - 1) // 2]; z = nodes[t - 1]
    elif scenario == "small ids":                                  # participant ids 1 .. n with some absent, z = 0
        nodes = rng.sample(range(1, 2 * t + 2), t); z = 0
    return nodes, z, [rng.randrange(R) for _ in range(t)]


def edge_segments(lengths, tile, seed, long=LONG):
    """[(name, nodes, z, values)]: an empty segment first and last, and every scenario that fits at every length"""
    rng = random.Random(seed)
    segs = [("empty first", [], rng.randrange(R), [])]
    for t in lengths:
        for name, least in SCENARIOS:
            if t < least or (t == 0 and name != "plain") or (t >= long and name not in LONG_SCENARIOS):
                continue
            segs.append(("%d %s" % (t, name),) + segment(t, name, tile, rng))
    segs.append(("empty last", [], 0, []))
    return segs


def pack(segs):
    """-> nodes (total, 4), offsets (nseg + 1,) u32, points (nseg, 4), values (total, 4)"""
    off = np.zeros(len(segs) + 1, dtype=np.uint32)
    for k, s in enumerate(segs):
        off[k + 1] = off[k] + len(s[1])
    nodes = to_limbs([x for s in segs for x in s[1]])
    return nodes, off, to_limbs([s[2] for s in segs]), to_limbs([v for s in segs for v in s[3]])


def expected(segs, zero_points=False):
    """-> lambda (total, 4), y (nseg, 4), flags (nseg,) u8 by the formula; zero_points: every z = 0 (points == NULL)"""
    lam_all, ys, flags = [], [], []
    for _, nodes, z, values in segs:
        lam, d = lagrange(nodes, 0 if zero_points else z)
        lam_all += lam; ys.append(interpolate(lam, values)); flags.append(d)
    return to_limbs(lam_all), to_limbs(ys), np.array(flags, dtype=np.uint8)
