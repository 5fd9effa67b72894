"""Segmented, gathered point sums on the GPU (blsgpu_g{1,2}_sum_segments[_device]): the edge inputs of tests/g_sum_points.py through the C
ABI, host and device forms, G1 and G2, compared after batch_normalize with the affine sums of oracle/bls12_381_ref.py limb for limb;
a skewed call; agreement with the all-ones segmented MSM; every refusal; the sticky flag for an index outside the point set."""
import ctypes
import functools

import numpy as np
import pytest

import g_sum_points as gp

pytestmark = pytest.mark.gpu

ERR_ARG = -2
CHUNK = {1: 256 * 8, 2: 128 * 8}                                   # gsum_plan.h: the shipped shapes


@pytest.fixture(scope="module")
def ctx():
    import bls12_381_amd as b
    return b.default_context()


@functools.lru_cache(maxsize=None)
def edge(group):
    segs = gp.edge_segments(group, CHUNK[group], seed=40 + group)
    return segs, gp.expected(group, segs)


@functools.lru_cache(maxsize=None)
def skewed(group):
    segs = gp.skewed_segments(group, 300, 2500, seed=50 + group)
    return segs, gp.expected(group, segs)


def same_points(ctx, group, out_xyz, want, what, skip=()):
    """batch_normalize of the sums against the oracle's affine points, limb for limb"""
    xy, inf = ctx.batch_normalize(group, out_xyz)
    wxy, winf = gp.wire_points(group, [w if w is not None else gp.pool(group).points[0] for w in want])
    keep = np.array([i not in skip for i in range(len(want))])
    assert np.array_equal(inf[keep], winf[keep]), what
    live = keep & (winf == 0)
    assert np.array_equal(xy[live], wxy[live]), "%s: segments %s" % (what, np.nonzero((xy != wxy).any(axis=1) & live)[0][:10])


def on_device(arrs):
    import torch
    dev = torch.device("cuda", 0)
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev) for a in arrs]


def device_call(ctx, group, xy, inf, idx, off, sync=True):
    import torch
    nseg, total = off.shape[0] - 1, int(off[-1])
    d_xy, d_inf, d_idx, d_off = on_device([xy, inf, idx, off])
    d_out = torch.full((max(nseg, 1) * 18 * group * 8,), 0xA5, dtype=torch.uint8, device=d_xy.device)
    ctx.sum_segments_device(group, d_xy.data_ptr(), d_inf.data_ptr(), xy.shape[0], d_idx.data_ptr() if d_idx is not None else 0, d_off.data_ptr(), nseg, total, d_out.data_ptr())
    if sync:
        ctx.synchronize()
    else:
        torch.cuda.synchronize()
    return d_out.cpu().numpy().view(np.uint64).reshape(-1, 18 * group)[:nseg]


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("form", ["idx", "no idx"])
def test_edge_inputs_host_and_device_forms(ctx, group, form):
    segs, want = edge(group)
    xy, inf, idx, off = (gp.gathered if form == "idx" else gp.contiguous)(group, segs)
    same_points(ctx, group, ctx.sum_segments(group, xy, inf, off, idx), want, "G%d host form, %s" % (group, form))
    same_points(ctx, group, device_call(ctx, group, xy, inf, idx, off), want, "G%d device form, %s" % (group, form))


@pytest.mark.parametrize("group", [1, 2])
def test_skewed_call(ctx, group):
    """300 segments of at most 8 terms around one of 2500: short segments share workgroups, the long one spans chunks"""
    segs, want = skewed(group)
    xy, inf, idx, off = gp.gathered(group, segs)
    assert 3400 < int(off[-1]) < 4300
    same_points(ctx, group, device_call(ctx, group, xy, inf, idx, off), want, "G%d skewed" % group)


@pytest.mark.parametrize("group", [1, 2])
def test_agrees_with_the_all_ones_segmented_msm(ctx, group):
    """the route this call replaces: msm_segments with every scalar 1 over the same contiguous terms"""
    from bls12_381_amd import synthetic as sy
    n = 1500
    bases = ctx.bases_from_scalars(group, sy.scalars(n, 600 + group))
    xy, inf = bases.download()
    lens = [0, 1, 2, 64, 65, 63, 500, 0, 300, 5]
    lens.append(n - sum(lens))
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    a = ctx.batch_normalize(group, ctx.sum_segments(group, xy, inf, off))
    b = ctx.batch_normalize(group, ctx.msm_segments(bases, [1] * n, off.astype(np.uint32)))
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[0][a[1] == 0], b[0][b[1] == 0])
    assert a[1].tolist() == [1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0]


def test_refusals(ctx):
    import torch
    segs, _ = skewed(1)
    xy, inf, idx, off = gp.gathered(1, segs[:20])
    nseg, total, npoints = 20, int(off[-1]), xy.shape[0]
    out = np.zeros((nseg, 18), dtype=np.uint64)
    host = ctx.lib.blsgpu_g1_sum_segments
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert host(ctx.h, p(xy), p(inf), npoints, p(idx), p(off), nseg, total, p(out)) == 0
    for what, args in {
        "NULL xy": (None, p(inf), npoints, p(idx), p(off), nseg, total, p(out)),
        "NULL infinity": (p(xy), None, npoints, p(idx), p(off), nseg, total, p(out)),
        "NULL offsets": (p(xy), p(inf), npoints, p(idx), None, nseg, total, p(out)),
        "NULL out": (p(xy), p(inf), npoints, p(idx), p(off), nseg, total, None),
        "total > 2^28": (p(xy), p(inf), npoints, p(idx), p(off), nseg, (1 << 28) + 1, p(out)),
        "npoints >= 2^32": (p(xy), p(inf), 1 << 32, p(idx), p(off), nseg, total, p(out)),
        "no idx, total > npoints": (p(xy), p(inf), npoints, None, p(off), nseg, total, p(out)),
        "total != offsets[nseg]": (p(xy), p(inf), npoints, p(idx), p(off), nseg, total - 1, p(out)),
    }.items():
        assert host(ctx.h, *args) == ERR_ARG, what
    assert total > npoints and off[6] > off[5]
    dec = off.copy(); dec[5], dec[6] = off[6], off[5]
    assert dec[5] > dec[6] and host(ctx.h, p(xy), p(inf), npoints, p(idx), p(dec), nseg, total, p(out)) == ERR_ARG, "decreasing offsets"
    big = off.copy(); big[5] = np.uint64(0xFFFFFFFFFFFFFFFF)
    assert host(ctx.h, p(xy), p(inf), npoints, p(idx), p(big), nseg, total, p(out)) == ERR_ARG, "an offset of 2^64 - 1"
    bad = idx.copy(); bad[7] = npoints
    assert host(ctx.h, p(xy), p(inf), npoints, p(bad), p(off), nseg, total, p(out)) == ERR_ARG, "an index >= npoints"
    with pytest.raises(Exception, match="sum_segments"):
        ctx.sum_segments(1, xy, inf, off, bad)
    # device form
    d_xy, d_inf, d_idx, d_off = on_device([xy, inf, idx, off])
    d_out = torch.zeros(nseg * 144 + 16, dtype=torch.uint8, device=d_xy.device)
    dev = ctx.lib.blsgpu_g1_sum_segments_device
    v = lambda t, o=0: ctypes.c_void_p(t.data_ptr() + o)
    good = (v(d_xy), v(d_inf), npoints, v(d_idx), v(d_off), nseg, total, v(d_out))
    assert dev(ctx.h, *good) == 0
    ctx.synchronize()
    for what, i, arg in (("NULL d_xy", 0, None), ("NULL d_inf", 1, None), ("NULL d_offsets", 4, None), ("NULL d_out", 7, None), ("total > 2^28", 6, (1 << 28) + 1),
                         ("npoints >= 2^32", 2, 1 << 32), ("misaligned d_xy", 0, v(d_xy, 4)), ("misaligned d_idx", 3, v(d_idx, 2)), ("misaligned d_offsets", 4, v(d_off, 4)),
                         ("misaligned d_out", 7, v(d_out, 4))):
        args = list(good); args[i] = arg
        assert dev(ctx.h, *args) == ERR_ARG, what
    args = list(good); args[3] = None
    assert dev(ctx.h, *args) == ERR_ARG, "no idx, total > npoints"
    ctx.synchronize()                                               # nothing was launched, nothing is flagged


def test_nseg_zero_is_a_no_op(ctx):
    assert ctx.sum_segments(1, np.zeros((0, 12), dtype=np.uint64), None, [0]).shape == (0, 18)
    assert ctx.lib.blsgpu_g2_sum_segments_device(ctx.h, None, None, 0, None, None, 0, 0, None) == 0
    assert ctx.lib.blsgpu_g1_sum_segments(ctx.h, None, None, 0, None, None, 0, 0, None) == 0
    ctx.synchronize()


@pytest.mark.parametrize("group", [1, 2])
def test_empty_segments_only(ctx, group):
    """segments but no terms: every sum is the identity, no point array is needed"""
    off = np.zeros(1001, dtype=np.uint64)
    out = ctx.sum_segments(group, np.zeros((0, 12 * group), dtype=np.uint64), None, off)
    xy, inf = ctx.batch_normalize(group, out)
    assert inf.tolist() == [1] * 1000


@pytest.mark.parametrize("group", [1, 2])
def test_an_index_outside_the_set_sets_the_sticky_flag(ctx, group):
    """device form: the term is skipped (never read), synchronize reports BLSGPU_ERR_ARG once and clears the flag, the other segments are right"""
    import bls12_381_amd as b
    segs, want = skewed(group)
    xy, inf, idx, off = gp.gathered(group, segs)
    idx = idx.copy()
    long_seg = 150
    assert len(segs[long_seg]) == 2500
    idx[int(off[long_seg]) + 1234] = xy.shape[0]
    idx[int(off[3])] = 0xFFFFFFFF if len(segs[3]) else idx[int(off[3])]
    skip = {long_seg, 3}
    out = device_call(ctx, group, xy, inf, idx, off, sync=False)
    with pytest.raises(b.BlsGpuError, match="sum_segments_device: an index"):
        ctx.synchronize()
    ctx.synchronize()                                               # cleared
    same_points(ctx, group, out, want, "G%d with a bad index" % group, skip=skip)
