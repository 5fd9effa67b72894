"""Group transforms (`blsgpu_g1_ntt_many*` / `blsgpu_g2_ntt_many*`, csrc/gntt.hip.h + csrc/gntt_plan.h): k radix-2 transforms over G1 / G2
points in one call.

Every comparison is exact, on affine points.  Small sizes are compared with the definition Y[m] = sum_j [w^(jm)] P[j] evaluated term by
term in the oracle (tests/g_ntt_points.py); larger ones with the discrete-log identity -- the transform of [s_j] G is [fr_ntt(s)_m] G --
where the scalars come from the oracle's `fr_ntt` (or from `ctx.fr_ntt_many`), the points [.] G from `ctx.bases_from_scalars`, which
has oracle tests of its own, and 16 positions of every case from oracle products as well.  Which of the two launch shapes ran is read
from the kernel names of `kernel_timing_report`, never from a time; the other shape is forced through BLSGPU_GNTT_TEAM_MAX on a
context of its own and must give the same points."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import bls12_381_ref as o
from g_ntt_points import G, RR, naive, scalars
from simt_gntt_child import TEAM_MAX_B                            # the built-in crossover, as csrc/gntt_plan.h states it

pytestmark = pytest.mark.gpu

ERR_ARG = -2
LANE, TEAM = "k_gntt_stage<LaneS>", "k_gntt_stage<TeamS>"
ENV = "BLSGPU_GNTT_TEAM_MAX"


@pytest.fixture(scope="module")
def ctx():
    import bls12_381_amd as b
    c = b.Context(0)
    yield c
    c.close()


def _forced(team_max):
    """a context whose plan takes the team shape up to `team_max` lane-shape lanes per stage (the switch is read when a context is created)"""
    import bls12_381_amd as b
    old = os.environ.get(ENV)
    os.environ[ENV] = str(team_max)
    try:
        return b.Context(0)
    finally:
        if old is None:
            os.environ.pop(ENV)
        else:
            os.environ[ENV] = old


def _affine(ctx, g, xyz):
    """(…, 18 | 36) projective wire points -> (xy, inf) with the coordinates of identities zeroed: one form per group element"""
    xy, inf = ctx.batch_normalize(g, np.ascontiguousarray(xyz).reshape(-1, 18 * g))
    xy = xy.copy()
    xy[inf != 0] = 0
    return xy, inf


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _base_points(ctx, g, ss):
    """[s] G for every s (integers, or (n, 32) canonical bytes), as (xy, inf) affine wire arrays, through the fixed-base path"""
    bases = ctx.bases_from_scalars(g, ss if isinstance(ss, np.ndarray) else [int(s) % RR for s in ss])
    xy, inf = bases.download()
    bases.free()
    xy = xy.copy()
    xy[inf != 0] = 0
    return xy, inf


def _spot_check(g, got, want_scalars, count=16):
    """`count` positions of an (xy, inf) result against oracle products [s] G"""
    n = len(want_scalars)
    xy, inf = got
    for i in sorted({0, n - 1} | {(7919 * t + 13) % n for t in range(count - 2)}):
        want = G[g].to_affine(G[g].base_mul(want_scalars[i]))
        have = G[g].affine(np.concatenate([xy[i], np.array(o.fp_to_mont_limbs(1) + [0] * (6 * g - 6), dtype=np.uint64)]))[0] if not inf[i] else G[g].to_affine(G[g].identity)
        assert have == want, "position %d" % i


def _shape_of(report):
    names = [k for k in report if k.startswith("k_gntt_stage")]
    assert len(names) == 1, report.keys()
    return names[0]


@pytest.mark.parametrize("g", [1, 2], ids=["G1", "G2"])
def test_naive_definition(ctx, g):
    """n <= 16, k in {1, 7}, both directions: the identity at the first, a middle and the last position of a vector, one vector all
    identity; the seven vectors are arrangements of the same points, so the oracle's n^2 products per direction are computed once"""
    grp = G[g]
    for n in (1, 2, 4, 8, 16):
        pts = [grp.base_mul(s) for s in scalars(n, 40 * g + n)]
        ident = grp.identity
        vecs = [list(pts)]
        for v in range(1, 7):
            vecs.append([pts[(j * (2 * v + 1) + v) % n] for j in range(n)])          # an odd stride and a shift: a permutation of the points
        for pos in sorted({0, n // 2, n - 1}):
            vecs[2][pos] = ident
        vecs[4] = [ident] * n
        for k, use in ((1, vecs[:1]), (7, vecs)):
            x = np.stack([grp.wire(v) for v in use])
            for inverse in (False, True):
                got = grp.affine(ctx.g_ntt_many(g, x, inverse=inverse))
                want = [a for v in use for a in grp.affine_of(naive(grp, v, inverse))]
                bad = [i for i in range(len(want)) if got[i] != want[i]]
                assert not bad, "G%d n=%d k=%d inverse=%s: %d points differ, first at %d" % (g, n, k, inverse, len(bad), bad[0])


@pytest.mark.parametrize("g,log_n,k", [(1, 6, 64), (1, 10, 4), (1, 12, 1), (1, 12, 16), (2, 6, 16), (2, 10, 2), (2, 12, 1)])
def test_discrete_log_identity_oracle_scalars(ctx, g, log_n, k):
    """P[j] = [s_j] G -> [fr_ntt(s)_m] G with fr_ntt from the oracle, every position; 0, 1 and r - 1 among the s_j; the affine (xy, infinity)
    form of the call (s_j = 0 is an identity with its flag set); inverse after forward is the input"""
    n = 1 << log_n
    ss = [scalars(n, 1000 * log_n + 10 * k + v, special=True) for v in range(k)]
    flat = [s for v in ss for s in v]
    xy, inf = _base_points(ctx, g, flat)
    y = ctx.g_ntt_many(g, (xy.reshape(k, n, -1), inf.reshape(k, n)))
    want_s = [s for v in ss for s in o.fr_ntt(v)]
    got = _affine(ctx, g, y)
    assert _same(got, _base_points(ctx, g, want_s))
    _spot_check(g, got, want_s)
    back = ctx.g_ntt_many(g, y, inverse=True)
    assert _same(_affine(ctx, g, back), (xy, inf))


@pytest.mark.parametrize("g,log_n,k", [(1, 16, 1), (1, 12, 256), (2, 14, 1)])
def test_discrete_log_identity_library_scalars(g, log_n, k):
    """the same identity with ctx.fr_ntt_many for the scalars and ctx.bases_from_scalars for the points, 16 positions against the oracle,
    through BOTH shapes: the plan's own choice (read from the kernel names) and the other one, forced"""
    import bls12_381_amd as b
    n = 1 << log_n
    B = k * n // 2
    raw = np.random.RandomState(log_n * 100 + k).randint(0, 256, size=(k * n, 32), dtype=np.uint8)
    raw[:, 31] &= 0x3F                                              # < 2^254 < r: the Montgomery limbs of some scalar
    limbs = raw.view(np.uint64).reshape(k, n, 4)
    results = {}
    for name, team_max in (("default", None), ("team", 1 << 40), ("lane", 0)):
        c = b.Context(0) if team_max is None else _forced(team_max)
        try:
            s_bytes = c.fr_to_bytes(limbs.reshape(-1, 4))
            want_bytes = c.fr_to_bytes(c.fr_ntt_many(limbs).reshape(-1, 4))
            xy, inf = _base_points(c, g, s_bytes)
            c.kernel_timing(True)
            y = c.g_ntt_many(g, (xy.reshape(k, n, -1), inf.reshape(k, n)))
            shape = _shape_of(c.kernel_timing_report())
            c.kernel_timing(False)
            got = _affine(c, g, y)
            assert _same(got, _base_points(c, g, want_bytes)), name
            if name == "default":
                want_s = [int.from_bytes(r.tobytes(), "little") for r in want_bytes]
                _spot_check(g, got, want_s)
                if log_n <= 14:                                     # the library's scalars against the oracle's where it can afford them
                    assert o.fr_ntt([int.from_bytes(r.tobytes(), "little") for r in s_bytes[:n]]) == want_s[:n]
            results[name] = (shape, got)
        finally:
            c.close()
    assert results["team"][0] == TEAM and results["lane"][0] == LANE
    assert results["default"][0] == (TEAM if B * g <= TEAM_MAX_B else LANE)      # lane-shape lanes: a lane pair per G2 butterfly
    assert _same(results["team"][1], results["lane"][1]) and _same(results["default"][1], results["lane"][1])


def test_monomial_srs_to_lagrange_form(ctx):
    """the SRS use: L = inverse transform of [tau^j] G1, normalised and uploaded as bases; for evaluation-form vectors y,
    msm(y, L) == msm(fr_ntt(y, inverse), monomial SRS) as affine points"""
    log_n = 12
    n = 1 << log_n
    tau = o.SplitMix64(0x7A0).scalar()
    powers, cur = [], 1
    for _ in range(n):
        powers.append(cur)
        cur = cur * tau % RR
    mono = ctx.bases_from_scalars(1, powers)
    xy, inf = mono.download()
    lag_xyz = ctx.g_ntt_many(1, (xy[None], inf[None]), inverse=True)[0]
    lxy, linf = ctx.batch_normalize(1, lag_xyz)
    lagrange = ctx.upload_bases(1, lxy, linf)
    for seed in (1, 2):
        y = scalars(n, 0x5125 + seed, special=seed == 2)
        coeff = o.fr_ntt(y, inverse=True)
        a = _affine(ctx, 1, ctx.msm(lagrange, y)[None, :])
        c = _affine(ctx, 1, ctx.msm(mono, coeff)[None, :])
        assert _same(a, c), seed
        if seed == 1:                                               # and the oracle's word on the common value
            want = o.g1_to_affine(G[1].base_mul(sum(cj * pj for cj, pj in zip(coeff, powers)) % RR))
            assert G[1].affine(ctx.msm(lagrange, y))[0] == want
    mono.free()
    lagrange.free()


def test_device_chain_on_a_caller_stream_and_between_pipelined_msm_calls(ctx):
    """mul_batch_device -> g_ntt_many_device -> batch_normalize_device on a caller's stream, no host copy in between; then the device form
    enqueued between two pipelined msm_device calls"""
    import torch
    dev = torch.device("cuda", 0)
    log_n, k = 8, 6
    n = 1 << log_n
    ss = [scalars(n, 900 + v, special=True) for v in range(k)]
    flat = [s for v in ss for s in v]
    want = _base_points(ctx, 1, [s for v in ss for s in o.fr_ntt(v)])
    gen = np.array(o.fp_to_mont_limbs(o.G1_GEN[0]) + o.fp_to_mont_limbs(o.G1_GEN[1]), dtype=np.uint64)
    d_gen = torch.from_numpy(np.tile(gen, (k * n, 1)).view(np.int64)).to(dev)
    d_s = torch.from_numpy(np.frombuffer(b"".join(s.to_bytes(32, "little") for s in flat), dtype=np.uint8).copy()).to(dev)
    d_xyz = torch.zeros((k * n, 18), dtype=torch.int64, device=dev)
    d_xy = torch.zeros((k * n, 12), dtype=torch.int64, device=dev)
    d_inf = torch.zeros(k * n, dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    ctx.set_stream(side.cuda_stream)
    try:
        ctx.mul_batch_device(1, d_gen.data_ptr(), None, d_s.data_ptr(), k * n, d_xyz.data_ptr())
        ctx.g_ntt_many_device(1, d_xyz.data_ptr(), log_n, k)
        ctx.batch_normalize_device(1, d_xyz.data_ptr(), k * n, d_xy.data_ptr(), d_inf.data_ptr())
        ctx.synchronize()
    finally:
        ctx.set_stream(None)
    xy, inf = d_xy.cpu().numpy().view(np.uint64).copy(), d_inf.cpu().numpy()
    xy[inf != 0] = 0
    assert _same((xy, inf), want)
    # between pipelined MSM calls
    m = 1 << 14
    S = np.random.RandomState(5).randint(0, 256, size=(2 * m, 32), dtype=np.uint8)
    S[:, 31] &= 0x3F
    bases = ctx.bases_from_scalars(1, S[:m])
    d_S = torch.from_numpy(S).to(dev)
    d_msm = torch.zeros((2, 18), dtype=torch.int64, device=dev)
    pxy, pinf = _base_points(ctx, 1, flat)
    x = ctx.g_ntt_many(1, (pxy.reshape(k, n, 12), pinf.reshape(k, n)), inverse=True)      # the inverse of it: the transform below brings the points back
    d_x = torch.from_numpy(x.view(np.int64)).to(dev)
    torch.cuda.synchronize()
    ctx.set_pipelining(True)
    try:
        ctx.msm_device(bases, d_S[0:m].data_ptr(), m, d_msm[0].data_ptr())
        ctx.g_ntt_many_device(1, d_x.data_ptr(), log_n, k)
        ctx.msm_device(bases, d_S[m:2 * m].data_ptr(), m, d_msm[1].data_ptr())
        ctx.join()
        ctx.synchronize()
    finally:
        ctx.set_pipelining(False)
    assert _same(_affine(ctx, 1, d_x.cpu().numpy().view(np.uint64)), (pxy, pinf))
    got = ctx.batch_normalize(1, d_msm.cpu().numpy().view(np.uint64))
    for i in range(2):
        ref = ctx.batch_normalize(1, ctx.msm(bases, S[i * m:(i + 1) * m])[None, :])
        assert np.array_equal(got[0][i], ref[0][0]) and got[1][i] == ref[1][0], i
    bases.free()


def test_arguments(ctx):
    """every refusal is BLSGPU_ERR_ARG with a text, before anything is staged or launched, and leaves the context usable and the buffers
    untouched; k == 0 and log_n == 0 are no-ops"""
    import torch
    lib, h = ctx.lib, ctx.h
    err = lambda: lib.blsgpu_last_error().decode()
    for g, host_fn, dev_fn in ((1, lib.blsgpu_g1_ntt_many, lib.blsgpu_g1_ntt_many_device), (2, lib.blsgpu_g2_ntt_many, lib.blsgpu_g2_ntt_many_device)):
        w = 18 * g
        x = G[g].wire([G[g].base_mul(s) for s in scalars(8, 3 + g)])
        keep = x.copy()
        d = torch.from_numpy(x.view(np.int64)).to(torch.device("cuda", 0))
        for fn, ptr in ((host_fn, x.ctypes.data_as(ctypes.c_void_p)), (dev_fn, ctypes.c_void_p(d.data_ptr()))):
            assert fn(h, ptr, -1, 1, 0) == ERR_ARG and "log_n" in err()
            assert fn(h, ptr, 25, 1, 0) == ERR_ARG and "log_n" in err()
            for log_n in (0, 3, 24):
                assert fn(h, ptr, log_n, ((1 << 24) >> log_n) + 1, 1) == ERR_ARG and "2^24" in err()
            assert fn(h, ptr, 3, (1 << 64) - 1, 0) == ERR_ARG and "2^24" in err()        # k << log_n overflows 64 bits
            assert fn(h, ptr, 3, (1 << 61) + 1, 0) == ERR_ARG
            assert fn(h, None, 3, 1, 0) == ERR_ARG and "NULL" in err()
            assert fn(h, None, 3, 0, 0) == 0 and fn(h, ptr, 3, 0, 1) == 0                  # k == 0
            assert fn(h, ptr, 0, 8, 1) == 0                                                  # log_n == 0: every point is its own transform
        assert dev_fn(h, ctypes.c_void_p(d.data_ptr() + 8), 2, 1, 0) == ERR_ARG and "aligned" in err()
        ctx.synchronize()
        assert np.array_equal(x, keep) and np.array_equal(d.cpu().numpy().view(np.uint64), keep)
        with pytest.raises(ValueError):
            ctx.g_ntt_many(g, np.zeros((2, 3, w), dtype=np.uint64))                         # not a power of two
        with pytest.raises(ValueError):
            ctx.g_ntt_many(g, np.zeros((2, 4, w + 1), dtype=np.uint64))
        with pytest.raises(ValueError):
            ctx.g_ntt_many(g, (np.zeros((2, 4, 12 * g), dtype=np.uint64), np.zeros((2, 3), dtype=np.uint8)))
        # the context is still usable; k == 0 through the Python form returns an empty array
        y = ctx.g_ntt_many(g, x[None])
        assert G[g].affine(ctx.g_ntt_many(g, y, inverse=True)) == G[g].affine(x)
        assert ctx.g_ntt_many(g, np.zeros((0, 8, w), dtype=np.uint64)).shape == (0, 8, w)


def test_cpp_mirror(ctx, tmp_path):
    """include/bls12_381.hpp g1_ntt_many / g2_ntt_many compiled with g++ against libblsgpu.so: round trips on 4 x 2^6 G1 points and 2^4 G2 points"""
    import bls12_381_amd as b
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "g_ntt_test")
    libdir = os.path.dirname(b.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "g_ntt_test.cpp"),
                           "-L" + libdir, "-lblsgpu", "-Wl,-rpath," + libdir, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "g_ntt_many ok" in out.stdout, out.stdout + out.stderr
