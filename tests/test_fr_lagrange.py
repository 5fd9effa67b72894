"""Lagrange coefficients at arbitrary nodes on the GPU (blsgpu_fr_lagrange_segments[_device]): the edge call of tests/fr_lagrange_ref.py
through the C ABI, host and device forms, against the formula in Python integers limb for limb; one segment of 4096 nodes against the
identities that pin its coefficients; many short and a few long segments through the shape the plan picks and through the other one;
the composition of fr_op / fr_scan / fr_batch_invert over an expanded difference matrix; every refusal; the sticky bit.

Lengths of the edge call: 0, 1, 2, 63, 64, 65, block - 1, block, block + 1, 2 block + 1 (= the LDS tile + 1) and 4096, with block = 256
and the tile = 512 of csrc/fr_lagrange_plan.h."""
import ctypes
import functools
import os
import random

import numpy as np
import pytest

import fr_lagrange_ref as ref

pytestmark = pytest.mark.gpu

ERR_ARG = -2
BLOCK, TILE = 256, 512                                             # fr_lagrange_plan.h: the BLOCK shape
FILL = 0xA5


@pytest.fixture(scope="module")
def ctx():
    import bls12_381_amd as b
    return b.default_context()


@pytest.fixture(scope="module")
def forced():
    """contexts that take the BLOCK / the WAVE shape whatever the lengths (BLSGPU_LAGRANGE_SHAPE is read when a context is created)"""
    import bls12_381_amd as b
    made = {}
    for name in ("block", "wave"):
        os.environ["BLSGPU_LAGRANGE_SHAPE"] = name
        try:
            made[name] = b.Context(0)
        finally:
            del os.environ["BLSGPU_LAGRANGE_SHAPE"]
    yield made
    for c in made.values():
        c.close()


@functools.lru_cache(maxsize=None)
def edge():
    """the edge call with a plain segment of 4096 nodes in front of its last, empty one; the formula's results for all but that segment"""
    segs = ref.edge_segments([0, 1, 2, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1, TILE + 1], TILE, seed=31, long=200)
    rng = random.Random(32)
    big = ("4096 plain",) + ref.segment(4096, "plain", TILE, rng)
    short = segs[:-1]
    lam, y, fl = ref.expected(short)
    lam0, y0, fl0 = ref.expected(short, zero_points=True)
    return short + [big, segs[-1]], ref.pack(short + [big, segs[-1]]), (lam, y, fl), (lam0, y0, fl0)


def on_device(arrs):
    import torch
    dev = torch.device("cuda", 0)
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev) for a in arrs]


def device_call(c, nodes, off, points, values, want_lambda=True, want_y=True, total=None, sync=True):
    """the device form with every output pre-filled with 0xA5 -> (lam | None, y | None, flags)"""
    import torch
    nseg = off.shape[0] - 1
    total = nodes.shape[0] if total is None else total
    d_n, d_off, d_p, d_v = on_device([nodes, off, points, values])
    mk = lambda n: torch.full((max(n, 16),), FILL, dtype=torch.uint8, device=d_off.device)
    d_lam, d_y, d_fl = mk(nodes.shape[0] * 32), mk(nseg * 32), mk(nseg)
    ptr = lambda t: 0 if t is None else t.data_ptr()
    c.fr_lagrange_segments_device(ptr(d_n), ptr(d_off), nseg, total, ptr(d_p), ptr(d_v), ptr(d_lam) if want_lambda else 0, ptr(d_y) if want_y else 0, ptr(d_fl))
    if sync:
        c.synchronize()
    else:
        torch.cuda.synchronize()
    back = lambda t, n: t.cpu().numpy()[:n * 32].view(np.uint64).reshape(n, 4)
    return back(d_lam, nodes.shape[0]) if want_lambda else None, back(d_y, nseg) if want_y else None, d_fl.cpu().numpy()[:nseg]


def same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.nonzero((got != want).reshape(got.shape[0], -1).any(axis=1))[0]
        raise AssertionError("%s differs from the formula at %d entries, first %d" % (what, len(bad), int(bad[0])))


def check_big_segment(nodes, z, values, lam_limbs, y_limbs, what):
    """the coefficients of the 4096-node segment: for 16 sampled i, lambda_i D_i (z - x_i) = l(z), with D_i and l(z) in O(t) each; the
    moments sum lambda_i x_i^k = z^k for k = 0, 1, t - 1 (the interpolation of X^k is exact below degree t); y from the coefficients"""
    R = ref.R
    t = len(nodes)
    lam = ref.from_limbs(lam_limbs)
    ell = 1
    for x in nodes:
        ell = ell * (z - x) % R
    rng = random.Random(5)
    for i in [0, 1, t - 1] + [rng.randrange(t) for _ in range(13)]:
        d = 1
        for j, x in enumerate(nodes):
            if j != i:
                d = d * (nodes[i] - x) % R
        assert lam[i] * d % R * ((z - nodes[i]) % R) % R == ell, "%s: lambda[%d]" % (what, i)
    for k in (0, 1, t - 1):
        assert sum(l * pow(x, k, R) for l, x in zip(lam, nodes)) % R == pow(z, k, R), "%s: moment %d" % (what, k)
    if y_limbs is not None:
        assert ref.from_limbs(y_limbs)[0] == ref.interpolate(lam, values), "%s: y" % what


@pytest.mark.parametrize("form", ["host", "device"])
def test_edge_call_host_and_device_forms(ctx, form):
    segs, (nodes, off, points, values), (lam, y, fl), _ = edge()
    if form == "host":
        glam, gy, gfl = ctx.fr_lagrange_segments(nodes, off, points, values)
    else:
        glam, gy, gfl = device_call(ctx, nodes, off, points, values)
    a, b = int(off[-3]), int(off[-2])                              # the segment of 4096
    assert b - a == 4096 and b == nodes.shape[0]
    same(glam[:a], lam, form + " lambda"); same(gy[:-2], y, form + " y"); same(gfl[:-2], fl, form + " flags")
    assert gfl[-2:].tolist() == [1, 1] and not gy[-1].any()
    check_big_segment(segs[-2][1], segs[-2][2], segs[-2][3], glam[a:b], gy[-2:-1], form + " 4096")
    assert fl.min() == 0 and fl.max() == 1


def test_points_null_values_absent_lambda_absent(ctx):
    segs, (nodes, off, points, values), (lam, y, fl), (lam0, y0, fl0) = edge()
    a = int(off[-3])
    glam, gy, gfl = device_call(ctx, nodes, off, None, values)
    same(glam[:a], lam0, "z = 0 lambda"); same(gy[:-2], y0, "z = 0 y"); same(gfl[:-2], fl0, "z = 0 flags")
    check_big_segment(segs[-2][1], 0, segs[-2][3], glam[a:], gy[-2:-1], "z = 0 4096")
    glam, gy, gfl = device_call(ctx, nodes, off, points, None, want_y=False)
    same(glam[:a], lam, "no values lambda"); same(gfl[:-2], fl, "no values flags")
    glam, gy, gfl = device_call(ctx, nodes, off, points, values, want_lambda=False)
    same(gy[:-2], y, "no lambda y"); same(gfl[:-2], fl, "no lambda flags")
    hl, hy, hf = ctx.fr_lagrange_segments(nodes, off, points, values, want_lambda=False)
    assert hl is None
    same(hy[:-2], y, "host no lambda y")
    assert np.array_equal(hy, gy)
    # integers in place of limbs: participant ids through fr_from_bytes
    ids = [[1, 2, 3], [5, 9, 2, 7]]
    hl, hy, hf = ctx.fr_lagrange_segments(ids[0] + ids[1], [0, 3, 7], values=[10, 20, 30, 1, 2, 3, 4])
    want = [ref.lagrange(s, 0)[0] for s in ids]
    assert ref.from_limbs(hl) == want[0] + want[1] and ref.from_limbs(hy) == [ref.interpolate(want[0], [10, 20, 30]), ref.interpolate(want[1], [1, 2, 3, 4])]


@functools.lru_cache(maxsize=None)
def shaped(kind):
    rng = random.Random(40 + len(kind))
    nseg, t = ((1 << 12), 8) if kind == "short" else (8, 513)
    names = [n for n, least in ref.SCENARIOS if least <= t]
    segs = [("%s %d" % (kind, k),) + ref.segment(t, names[k % len(names)] if kind == "short" else ref.LONG_SCENARIOS[k % 5], 8 if kind == "short" else TILE, rng) for k in range(nseg)]
    return ref.pack(segs), ref.expected(segs)


@pytest.mark.parametrize("kind", ["short", "long"])
@pytest.mark.parametrize("shape", ["plan", "block", "wave"])
def test_many_short_and_few_long_segments_in_both_shapes(ctx, forced, kind, shape):
    """2^12 segments of 8 (the plan: teams of 8 lanes) and 8 segments of 513 (the plan: a workgroup each), each also through the other shape"""
    (nodes, off, points, values), (lam, y, fl) = shaped(kind)
    c = ctx if shape == "plan" else forced[shape]
    glam, gy, gfl = device_call(c, nodes, off, points, values)
    same(glam, lam, "%s %s lambda" % (kind, shape)); same(gy, y, "%s %s y" % (kind, shape)); same(gfl, fl, "%s %s flags" % (kind, shape))


def test_agrees_with_the_composition_over_the_difference_matrix(ctx):
    """one segment of 64 nodes: the 64 x 64 matrices x_i - x_j and z - x_j (1 on the diagonal) by fr_op, their row products by fr_scan,
    inv0 by fr_batch_invert, the product by fr_op -- the route this call replaces, limb for limb"""
    from bls12_381_amd import api
    rng = random.Random(77)
    t = 64
    x, z, v = ref.segment(t, "repeat adjacent", 8, rng)
    xl, zl = ref.to_limbs(x), ref.to_limbs([z])
    one = ref.to_limbs([1])
    rows, cols = np.repeat(xl, t, axis=0), np.tile(xl, (t, 1))
    diff = ctx.fr_op(2, rows, cols).reshape(t, t, 4)
    num = ctx.fr_op(2, np.tile(zl, (t * t, 1)), cols).reshape(t, t, 4)
    for i in range(t):
        diff[i, i] = one[0]; num[i, i] = one[0]
    d = ctx.fr_scan(api.FR_SCAN_PRODUCT, diff)[:, -1, :]
    n = ctx.fr_scan(api.FR_SCAN_PRODUCT, num)[:, -1, :]
    want = ctx.fr_op(0, n, ctx.fr_batch_invert(d))
    off = np.array([0, t], dtype=np.uint32)
    glam, _, gfl = device_call(ctx, xl, off, zl, None, want_y=False)
    assert np.array_equal(glam, want) and gfl.tolist() == [0]
    assert ref.from_limbs(glam) == ref.lagrange(x, z)[0]


def test_refusals(ctx):
    import torch
    segs = ref.edge_segments([3, 5, 8], 4, seed=3)
    nodes, off, points, values = ref.pack(segs)
    nseg, total = off.shape[0] - 1, nodes.shape[0]
    lam, y, fl = np.zeros((total, 4), dtype=np.uint64), np.zeros((nseg, 4), dtype=np.uint64), np.zeros(nseg, dtype=np.uint8)
    host = ctx.lib.blsgpu_fr_lagrange_segments
    p = lambda a, o=0: ctypes.c_void_p(a.ctypes.data + o)
    good = (p(nodes), p(off), nseg, p(points), p(values), p(lam), p(y), p(fl))
    assert host(ctx.h, *good) == 0
    for what, i, arg in (("NULL nodes", 0, None), ("NULL offsets", 1, None), ("y without values", 4, None), ("nseg > 2^27", 2, (1 << 27) + 1), ("lambda on the nodes", 5, p(nodes)),
                         ("y on the points", 6, p(points)), ("flags on the values", 7, p(values, 5)), ("y inside lambda", 6, p(lam, 32)), ("lambda on the offsets", 5, p(off))):
        args = list(good); args[i] = arg
        assert host(ctx.h, *args) == ERR_ARG, what
    args = list(good); args[5] = args[6] = None
    assert host(ctx.h, *args) == ERR_ARG, "neither lambda nor y"
    first = off.copy(); first[0] = 1
    dec = off.copy(); dec[2], dec[3] = off[3], off[2]
    assert dec[2] > dec[3]
    assert host(ctx.h, p(nodes), p(first), *good[2:]) == ERR_ARG, "offsets[0] != 0"
    assert host(ctx.h, p(nodes), p(dec), *good[2:]) == ERR_ARG, "decreasing offsets"
    big, big_out, big_off = np.zeros((4097, 4), dtype=np.uint64), np.zeros((4097, 4), dtype=np.uint64), np.array([0, 4097], dtype=np.uint32)
    assert host(ctx.h, p(big), p(big_off), 1, None, None, p(big_out), None, None) == ERR_ARG, "a segment of 4097 nodes"
    with pytest.raises(Exception, match="fr_lagrange_segments"):
        ctx.fr_lagrange_segments(nodes, off, points, None, want_y=True)
    # device form
    d_n, d_off, d_p, d_v = on_device([nodes, off, points, values])
    d_lam = torch.zeros(total * 32 + 32, dtype=torch.uint8, device=d_n.device)
    d_y = torch.zeros(nseg * 32 + 32, dtype=torch.uint8, device=d_n.device)
    d_fl = torch.zeros(nseg + 16, dtype=torch.uint8, device=d_n.device)
    dev = ctx.lib.blsgpu_fr_lagrange_segments_device
    v = lambda t, o=0: ctypes.c_void_p(t.data_ptr() + o)
    good = (v(d_n), v(d_off), nseg, total, v(d_p), v(d_v), v(d_lam), v(d_y), v(d_fl))
    assert dev(ctx.h, *good) == 0
    ctx.synchronize()
    for what, i, arg in (("NULL d_nodes", 0, None), ("NULL d_offsets", 1, None), ("y without values", 5, None), ("nseg > 2^27", 2, (1 << 27) + 1), ("total > 2^27", 3, (1 << 27) + 1),
                         ("total 2^64 - 1", 3, (1 << 64) - 1), ("misaligned d_nodes", 0, v(d_n, 8)), ("misaligned d_offsets", 1, v(d_off, 2)), ("misaligned d_points", 4, v(d_p, 4)),
                         ("misaligned d_values", 5, v(d_v, 8)), ("misaligned d_lambda", 6, v(d_lam, 8)), ("misaligned d_y", 7, v(d_y, 8)), ("d_lambda on d_nodes", 6, v(d_n)),
                         ("d_y on d_points", 7, v(d_p)), ("d_y inside d_lambda", 7, v(d_lam, 32)), ("d_flags on d_values", 8, v(d_v, 3)), ("d_flags on d_y", 8, v(d_y, 31))):
        args = list(good); args[i] = arg
        assert dev(ctx.h, *args) == ERR_ARG, what
    args = list(good); args[6] = args[7] = None
    assert dev(ctx.h, *args) == ERR_ARG, "neither lambda nor y"
    ctx.synchronize()                                               # nothing was launched, nothing is flagged


def test_cpp_mirror(ctx, tmp_path):
    """include/bls12_381.hpp fr_lagrange_segments / g{1,2}_lagrange_combine compiled with g++ against libblsgpu.so: y against a host loop
    over bls::fr_op, the unit vector for a point on a node, the flag of a repeated node, the combines on shares whose result is known"""
    import subprocess
    import bls12_381_amd as b
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "fr_lagrange_test")
    libdir = os.path.dirname(b.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "fr_lagrange_test.cpp"),
                           "-L" + libdir, "-lblsgpu", "-Wl,-rpath," + libdir, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "fr_lagrange ok" in out.stdout, out.stdout + out.stderr


def test_nseg_zero_and_empty_segments(ctx):
    assert ctx.lib.blsgpu_fr_lagrange_segments_device(ctx.h, None, None, 0, 0, None, None, None, None, None) == 0
    assert ctx.lib.blsgpu_fr_lagrange_segments(ctx.h, None, None, 0, None, None, None, None, None) == 0
    lam, y, fl = ctx.fr_lagrange_segments(np.zeros((0, 4), dtype=np.uint64), np.zeros(1001, dtype=np.uint32), values=np.zeros((0, 4), dtype=np.uint64))
    assert lam.shape == (0, 4) and not y.any() and fl.tolist() == [1] * 1000
    ctx.synchronize()


@pytest.mark.parametrize("shape", ["block", "wave"])
def test_bad_segments_set_the_sticky_bit_and_write_nothing(forced, shape):
    """what only the device sees: segment 1 decreases, segment 2 has 4097 nodes, segment 4 ends beyond total, segment 5 begins there.
    synchronize reports BLSGPU_ERR_ARG once and clears the bit; segments 0 and 3 are right, no other entry is written; a clean call follows"""
    import bls12_381_amd as b
    c = forced[shape]
    rng = random.Random(21)
    total = 4097 + 30
    ints = rng.sample(range(1, 1 << 62), total)
    vals = [rng.randrange(ref.R) for _ in range(total)]
    off = np.array([0, 6, 4, 4101, 4110, total + 3, total], dtype=np.uint32)
    z = [rng.randrange(ref.R) for _ in range(6)]
    glam, gy, gfl = device_call(c, ref.to_limbs(ints), off, ref.to_limbs(z), ref.to_limbs(vals), sync=False)
    with pytest.raises(b.BlsGpuError, match="fr_lagrange_segments_device"):
        c.synchronize()
    c.synchronize()                                                 # cleared
    fill64 = np.uint64(0xA5A5A5A5A5A5A5A5)
    lam = np.full((total, 4), fill64, dtype=np.uint64)
    y = np.full((6, 4), fill64, dtype=np.uint64)
    fl = np.full(6, FILL, dtype=np.uint8)
    for s, (a, e) in ((0, (0, 6)), (3, (4101, 4110))):
        l, d = ref.lagrange(ints[a:e], z[s])
        lam[a:e] = ref.to_limbs(l); y[s] = ref.to_limbs([ref.interpolate(l, vals[a:e])])[0]; fl[s] = d
    assert np.array_equal(glam, lam) and np.array_equal(gy, y) and np.array_equal(gfl, fl)
    good = np.array([0, 6, 6, 4101 - 4095, 4110 - 4095], dtype=np.uint32)      # a clean call after it
    glam, gy, gfl = device_call(c, ref.to_limbs(ints[:15]), good, None, ref.to_limbs(vals[:15]))
    assert ref.from_limbs(glam[:6]) == ref.lagrange(ints[:6], 0)[0] and gfl.tolist() == [1, 1, 1, 1]
