"""The large MSM through the public API with inputs built to FILL what the other GPU tests reach only where entries happen to fall:
every bucket of every window at every window width and decomposition (B1), bucket loads at the edges of the work-item cut and of
the cut-bucket fold (B2), and dense uniform scalars at the windows `pick_window` never chooses for the sizes the suite runs (B3).
The stage-by-stage half of the same work runs on the host: tests/test_simt_msm_front.py, tests/test_simt_msm_points.py.

Expected values come from the oracle by the discrete-log identity: bases [k_i] G (Context.bases_from_scalars), result
[sum k_i s_i] G, compared as uncompressed affine bytes.  `test_bases_are_the_oracles_multiples` downloads 64 bases per group and
compares them with the C oracle's double-and-add, so the identity does not rest on the library alone.

The level form of the window reduction a case takes follows from api_msm.hip (TEAM = 8, TEAM_LANES_MAX = 131072; nseg windows,
G = 2^(c-4) chains at the bottom level): team2 while nseg * G <= 8192, team while <= 16384, the pair forms above.  B1 runs every
width 4..16 in all four configurations, so each form of each group gets a bottom level in which every record is a non-trivial
point: G1 GLV pair at c = 15, 16; G1 plain team at 13, pair at 14..16; G2 psi team at 15, 16; G2 plain team at 13, g2pair at
14..16; team2 below.
"""
import numpy as np
import pytest

import decomp_model as dm
import msm_pipe_model as mm
from oracle import bls12_381_ref as o

gpu = pytest.mark.gpu                                               # per test: the construction check below needs no GPU

RR = o.R_ORDER
NB = 1 << 16                                                        # resident bases per group
CONFIGS = {"g1_glv": (1, "default", 4, 126), "g1_plain": (1, "plain", 8, 254), "g2_psi": (2, "default", 2, 62), "g2_plain": (2, "plain", 8, 254)}
#           name: (group, context, words per sort scalar, usable bits of a sort scalar)


class _Env:
    """the three contexts, and per (context, group) one resident set of NB bases [k_i] G"""

    def __init__(self):
        import bls12_381_amd as b
        from bls12_381_amd import synthetic as sy
        self.ctx = {"default": b.Context(0)}
        for name, hook, value in (("plain", "BLSGPU_NO_GLV", "1"), ("cap16", "BLSGPU_ITEM_CAP", "16")):
            with pytest.MonkeyPatch.context() as mp:                # the hooks are read when a context is created
                mp.setenv(hook, value)
                self.ctx[name] = b.Context(0)
        self.ks = {g: sy.to_ints(sy.scalars(NB, sy.SEED + 0x510 + g)) for g in (1, 2)}
        self.sets = {}

    def bases(self, ctx_name, group):
        if (ctx_name, group) not in self.sets:
            self.sets[(ctx_name, group)] = self.ctx[ctx_name].bases_from_scalars(group, self.ks[group])
        return self.sets[(ctx_name, group)]

    def close(self):
        for s in self.sets.values():
            s.free()
        for c in self.ctx.values():
            c.close()


@pytest.fixture(scope="module")
def env():
    e = _Env()
    yield e
    e.close()


def _want(group, tot):
    if group == 1:
        return o.g1_to_uncompressed(o.g1_to_affine(o.g1_affine_mul(o.G1_GEN, tot % RR)))
    return o.g2_to_uncompressed(o.g2_to_affine(o.g2_affine_mul(o.G2_GEN, tot % RR)))


def _got(ctx, group, out):
    import bls12_381_amd as b
    xy, inf = ctx.batch_normalize(group, np.asarray(out)[None, :])
    return (b.G1Affine if group == 1 else b.G2Affine)(xy[0], bool(inf[0])).to_uncompressed()


def _bytes(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint8).reshape(-1, 32).copy()


def _mont(vals):
    return np.array([o.fr_to_mont_limbs(int(v)) for v in vals], dtype=np.uint64).reshape(-1, 4)


def _dot(ks, ss):
    return sum(k * s for k, s in zip(ks, ss)) % RR


def _check(env, ctx_name, group, ss, window, ks=None, bases=None, mont=False):
    ctx = env.ctx[ctx_name]
    bases = bases or env.bases(ctx_name, group)
    ks = ks or env.ks[group]
    ctx.set_msm_window(window)
    try:
        out = ctx.msm_mont(bases, _mont(ss)) if mont else ctx.msm(bases, _bytes(ss))
    finally:
        ctx.set_msm_window(0)
    assert _got(ctx, group, out) == _want(group, _dot(ks, ss))


# ---- the stored sub-scalars of a configuration (what the sort reads), by the decomposition models ---------------------------------
def _compose(config, parts):
    """the scalar whose decomposition is `parts` (magnitudes below the usable width; GLV halves may be negative): plain: the value
    itself; GLV: k1 + k2 L (the phi term stands for -[L] P, so a positive k2 is stored as subtracted); psi: sum d_j X^j (odd terms
    stored as subtracted: psi = [-X])"""
    if config.endswith("plain"):
        return parts[0]
    if config == "g1_glv":
        return dm.glv_value(abs(parts[0]), int(parts[0] < 0), abs(parts[1]), int(parts[1] >= 0))
    return dm.gls_value([(parts[0], 0), (parts[1], 1), (parts[2], 0), (parts[3], 1)])


def _expect_stored(config, parts):
    """what the decomposition must store for the constructed parts: magnitude | flag << top bit"""
    if config.endswith("plain"):
        return [parts[0]]
    if config == "g1_glv":
        return [abs(parts[0]) | (int(parts[0] < 0) << 127), abs(parts[1]) | (int(parts[1] >= 0) << 127)]
    return [m | ((j & 1) << 63) for j, m in enumerate(parts)]


def _stored(config, k):
    """the sort scalars of k as the decomposition kernel stores them: [(value with its sign bit, words)]"""
    if config.endswith("plain"):
        return [k]
    if config == "g1_glv":
        k1, neg1, k2, sub2, _ = dm.glv_model(k)
        return [k1 | (neg1 << 127), k2 | (sub2 << 127)]
    return [m | (s << 63) for m, s in dm.gls_model(k)]


def _covering_scalars(config, c):
    """2^c scalars (at most NB) whose sort scalars hit every entry of every full window exactly once per part; asserted with the
    decomposition and recoding models before anything runs on the GPU"""
    group, _, words, usable = CONFIGS[config]
    nparts = {8: 1, 4: 2, 2: 4}[words]
    rng = o.SplitMix64(0xB1 + 64 * c + words)
    cols, nfull = zip(*[mm.covering_values(c, usable, rng, signed=config == "g1_glv") for _ in range(nparts)])
    nfull = nfull[0]
    rows = [[col[i] for col in cols] for i in range(1 << c)]
    ss = [_compose(config, row) for row in rows]
    assert all(0 <= s < RR for s in ss)
    nwin = mm.nwin_of(c, words)
    stored = [_stored(config, s) for s in ss]
    assert stored == [_expect_stored(config, row) for row in rows], "the split does not return the constructed parts"
    for p in range(nparts):
        # a part stored as subtracted while its value is positive (k2 of GLV, the odd psi digits) enters with every sign flipped
        flip = int(config == "g1_glv" and p == 1 or config == "g2_psi" and p & 1)
        digits = [mm.recode(st[p], c, nwin, words) for st in stored]
        assert mm.coverage(digits, c, nfull, flip), "window coverage is not 100 %"
    return ss


@pytest.mark.parametrize("c", [4, 5, 7, 9, 13, 15, 16])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_covering_construction_on_the_cpu(config, c):
    """no GPU: the construction, the round trip through the split models and the 100 % coverage of every full window (asserted inside
    `_covering_scalars`) for the three usable widths, and every scalar below r"""
    ss = _covering_scalars(config, c)
    assert len(ss) == 1 << c and max(ss) < RR


@pytest.mark.parametrize("group", [1, 2])
@gpu
def test_bases_are_the_oracles_multiples(env, group):
    """64 of the resident bases (first, last, a stride in between) against the C oracle's double-and-add of the generator"""
    from oracle import c_oracle
    idx = [0, 1, NB - 1] + list(range(1000, NB, NB // 61))[:61]
    gen = o.G1_GEN if group == 1 else o.G2_GEN
    limbs = lambda x: np.array(o.fp_to_mont_limbs(x), dtype=np.uint64)
    gw = np.concatenate([limbs(gen[0]), limbs(gen[1])]) if group == 1 else np.concatenate([limbs(gen[0][0]), limbs(gen[0][1]), limbs(gen[1][0]), limbs(gen[1][1])])
    want, winf = c_oracle.mul_batch_affine(group, np.tile(gw, (len(idx), 1)), None, _bytes([env.ks[group][i] for i in idx]))
    bases = env.bases("default", group)
    for j, i in enumerate(idx):
        xy, inf = bases.download(i, 1)
        assert not inf[0] and not winf[j] and np.array_equal(xy[0], want[j]), i


# ---- B1 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", range(4, 17))
@pytest.mark.parametrize("config", list(CONFIGS))
@gpu
def test_every_bucket_of_every_full_window(env, config, c):
    """n = 2^c scalars whose signed digits run through all 2^c values in every window that lies wholly below the usable width (254
    bits plain, 126 per GLV half, 62 per psi digit): every bucket of those windows holds exactly one entry per part with either sign
    (two at magnitude < 2^(c-1), one at 2^(c-1)), so a wrong weight anywhere in the chunked running sums, a T tree or the Horner pass
    over the levels moves the result.  The narrower top window is left to the uniform-random tests."""
    group, ctx_name, _, _ = CONFIGS[config]
    _check(env, ctx_name, group, _covering_scalars(config, c), c)


@pytest.mark.parametrize("c", [4, 13, 16])
@pytest.mark.parametrize("config", list(CONFIGS))
@gpu
def test_every_bucket_montgomery_form(env, config, c):
    """the same inputs as Montgomery limbs (`&[Scalar]` memory): the plain configurations reduce them in k_scalars_from_mont, the
    split ones inside their decomposition kernels"""
    group, ctx_name, _, _ = CONFIGS[config]
    _check(env, ctx_name, group, _covering_scalars(config, c), c, mont=True)


# ---- B2 ----------------------------------------------------------------------------------------------------------------------
B2_C, B2_N, B2_WIN, B2_MAG = 13, 4096, 1, 1234


def _signed_digit(v, c, w):
    mag, neg = mm.recode(v, c, w + 1, 8)[w]
    return -mag if neg else mag


def _loaded_scalars(config, L, seed):
    """B2_N scalars in which exactly L sort scalars -- the first part of scalars 0 .. L-1 -- have magnitude B2_MAG in window B2_WIN (the
    odd ones as a negative digit), and no other sort scalar of any part does; everything else uniform.  Changing one signed digit of
    a value changes no other digit (the digit set makes the representation unique)."""
    group, _, words, usable = CONFIGS[config]
    nparts = {8: 1, 4: 2, 2: 4}[words]
    rng = o.SplitMix64(seed)
    sh = B2_C * B2_WIN
    ss = []
    for i in range(B2_N):
        parts = []
        for p in range(nparts):
            v = (rng.next() | (rng.next() << 64)) % (1 << (usable - 1)) | (1 << (usable - 1))      # the top bit keeps every value positive
            d = _signed_digit(v, B2_C, B2_WIN)
            if p == 0 and i < L:
                v += ((-B2_MAG if i & 1 else B2_MAG) - d) << sh
            elif abs(d) == B2_MAG:
                v += (1 if d > 0 else -1) << sh
            parts.append(v)
        ss.append(_compose(config, parts))
    nwin = mm.nwin_of(B2_C, words)
    flat = [st for s in ss for st in _stored(config, s)]
    loads = [len(b) for b in mm.bucket_entries(flat, B2_C, nwin, words)]
    assert loads[B2_WIN * (1 << (B2_C - 1)) + B2_MAG - 1] == L
    assert mm.item_cap(len(flat), B2_C) == 128
    return ss


@pytest.mark.parametrize("L", [127, 128, 129, 2048, 2049, 2177])
@pytest.mark.parametrize("config", ["g1_glv", "g2_psi"])
@gpu
def test_bucket_load_at_item_and_fold_edges(env, config, L):
    """one bucket with exactly L entries at cap = 128: 1, 1, 2, 16, 17 and 18 work items, i.e. uncut, cut and folded by one lane
    (<= HEAVY_SMALL partials), cut and folded by a block.  Among its bases a repeated one and one with its negative."""
    group, ctx_name, _, _ = CONFIGS[config]
    ks = list(env.ks[group][:B2_N])
    ks[2] = ks[0]                                                  # both even: the same digit on the same point (a doubling)
    ks[6] = RR - ks[4]                                             # P and -P with the same digit
    ks[5] = ks[3]; ks[9] = RR - ks[7]                              # ... and among the negated entries
    ctx = env.ctx[ctx_name]
    bases = ctx.bases_from_scalars(group, ks)
    try:
        _check(env, ctx_name, group, _loaded_scalars(config, L, 0xB2 + L + group), B2_C, ks=ks, bases=bases)
    finally:
        bases.free()


@pytest.mark.parametrize("group", [1, 2])
@gpu
def test_every_bucket_cut_and_block_folded(env, group):
    """BLSGPU_ITEM_CAP = 16, window 8, uniform scalars: 2^17 sort scalars (2 x 2^16 GLV halves / 4 x 2^15 psi digits) over 128 buckets
    per window load every bucket of a full window with ~1000 entries, more than 16 x 16: every one of the 2048 (G1: 16 windows) /
    1024 (G2: 8 windows) buckets bar the narrow top window's is folded by a block, more than HEAVY_BIG_BLOCKS of them."""
    from bls12_381_amd import synthetic as sy
    n = 1 << (16 if group == 1 else 15)
    config = "g1_glv" if group == 1 else "g2_psi"
    sb = sy.scalars(n, sy.SEED + 0xB20 + group)
    ss = sy.to_ints(sb)
    low = np.array([st & 0xff for s in ss for st in _stored(config, s)])         # window 0: no carry comes in
    mag = np.where(low > 128, 256 - low, low)
    loads = np.bincount(mag, minlength=129)[1:]
    nb = mm.nwin_of(8, 4 if group == 1 else 2) * 128
    assert loads.min() > 16 * mm.HEAVY_SMALL and nb - 128 > mm.HEAVY_BIG_BLOCKS
    _check(env, "cap16", group, ss, 8)


# ---- B3 ----------------------------------------------------------------------------------------------------------------------
def _uniform(group, c, count=1):
    from bls12_381_amd import synthetic as sy
    n = 1 << (15 if group == 1 else 13)
    return [sy.to_ints(sy.scalars(n, sy.SEED + 0xB30 + 16 * c + 4 * group + j)) for j in range(count)]


@pytest.mark.parametrize("c", [7, 10, 14, 15])
@pytest.mark.parametrize("config", list(CONFIGS))
@gpu
def test_dense_uniform_at_unpicked_windows(env, config, c):
    """2^15 (G2: 2^13) uniform scalars at window widths `pick_window` does not choose for any size the suite runs"""
    group, ctx_name, _, _ = CONFIGS[config]
    _check(env, ctx_name, group, _uniform(group, c)[0], c)


@pytest.mark.parametrize("group", [1, 2])
@gpu
def test_dense_uniform_pipelined_across_window_changes(env, group):
    """the same through msm_many with k = 3 on the default context, one call per width: the pipeline slots are reused by calls
    whose bucket count, level count and buffer sizes differ from those of the call that used the slot last"""
    ctx, bases = env.ctx["default"], env.bases("default", group)
    try:
        for c in (7, 15, 10, 14):
            sets = _uniform(group, c, 3)
            ctx.set_msm_window(c)
            outs = ctx.msm_many(bases, np.stack([_bytes(s) for s in sets]))
            for s, out in zip(sets, outs):
                assert _got(ctx, group, out) == _want(group, _dot(env.ks[group], s)), c
    finally:
        ctx.set_msm_window(0)


# ---- launch plan ---------------------------------------------------------------------------------------------------------------
# (label, group, context, n, forced window, table window, words per sort scalar)
PLAN_SHAPES = [("g1 default", 1, "default", 256, 0, 0, 4), ("g2 default", 2, "default", 64, 0, 0, 2), ("g1 window 16", 1, "default", 4096, 16, 0, 4),
               ("g1 tables 9", 1, "default", 256, 0, 9, 8), ("g1 plain", 1, "plain", 256, 0, 0, 8)]


def plan_shape_launches(label):
    """what tests/msm_pipe_model.py predicts for one call of a PLAN_SHAPES case: kernel name -> launches"""
    _, group, _, n, window, table, words = next(s for s in PLAN_SHAPES if s[0] == label)
    c = table or window or mm.pick_window(n * (8 // words), mm.SBITS[words])
    return mm.launch_counts(group, words, c, merged=bool(table))


@gpu
def test_launches_follow_the_plan(env):
    """one call per shape with kernel timing on: the result against the oracle, and the launches of kernel_timing_report() against the
    counts the model derives from the plan (csrc/msm_plan.h through tests/msm_pipe_model.py launch_counts): the sort kernels of the
    path taken, three item kernels, one accumulation, one fold, the level launches by form, one multi-job tree launch per step that
    has a pass, the shift-adds, one combine and one export.  `g1 window 16` has five levels, four of them with a tree."""
    assert [lv["G"] > 1 for lv in mm.reduction_schedule(8, 1 << 15)["levels"]] == [True] * 4 + [False]
    for label, group, ctx_name, n, window, table, _ in PLAN_SHAPES:
        ctx = env.ctx[ctx_name]
        ks = env.ks[group][:n]
        ss = [int(x) for x in _uniform(group, 9)[0][:n]]
        bases = ctx.bases_from_scalars(group, ks)
        try:
            if table:
                bases.precompute(table)
            ctx.set_msm_window(window)
            ctx.synchronize()
            ctx.kernel_timing(True)
            ctx.kernel_timing_report()
            out = ctx.msm(bases, _bytes(ss))
            report = ctx.kernel_timing_report()
        finally:
            ctx.kernel_timing(False)
            ctx.set_msm_window(0)
            bases.free()
        assert _got(ctx, group, out) == _want(group, _dot(ks, ss)), label
        assert {k: v["launches"] for k, v in report.items()} == plan_shape_launches(label), label
