"""G1 MSMs through the bucket accumulation on the GPU, canonical encodings against the oracle.

The accumulation kernel's field products keep every column sum in source order (fe.hip.h `mac()`); what the host emulation cannot
show is that the GPU build of that form computes the same, in the kernel's generic branch and in its exceptional ones.  The inputs
make the buckets meet them: repeated bases with repeated scalars (P + P), a base next to its negative (cancellation, and a further
point after it), scalars 0 and r - 1, the recoding edges of tests/msm_edge_values.py, identity bases, buckets with one entry; in one
call and through the pipeline; the segmented MSM, which shares the mixed addition; and uniform scalars at 2^14."""
import numpy as np
import pytest

from oracle import bls12_381_ref as o
from msm_edge_values import carry_values

pytestmark = pytest.mark.gpu
RR = o.R_ORDER


@pytest.fixture(scope="module")
def ctx():
    import bls12_381_amd as b
    c = b.Context(0)
    yield c
    c.close()


def _encoding(ctx, proj):
    import bls12_381_amd as b
    xy, inf = ctx.batch_normalize(1, np.asarray(proj, dtype=np.uint64)[None, :])
    return b.G1Affine(xy[0], bool(inf[0])).to_uncompressed()


def _want(ks, ss):
    tot = sum(k * s for k, s in zip(ks, ss)) % RR
    return o.g1_to_uncompressed(o.g1_to_affine(o.g1_affine_mul(o.G1_GEN, tot))) if tot else o.g1_to_uncompressed(o.G1_IDENTITY_AFF)


def _edge_case(n, seed):
    """bases [k_i] G and scalars of n entries in blocks: the recoding edges, then groups that collide inside buckets"""
    r = o.SplitMix64(seed)
    ks = [r.scalar() for _ in range(n)]
    ss = [r.scalar() for _ in range(n)]
    edge = carry_values()
    step = max(1, len(edge) // (n // 4))
    for i, v in enumerate(edge[::step][:n // 4]):                    # a quarter: scalars at the recoding edges
        ss[i] = v
    q = n // 4
    for i in range(q, q + n // 8, 4):                                # P + P, then P + P + (-P) ... in every window of the scalar
        ks[i + 1] = ks[i]; ks[i + 2] = (RR - ks[i]) % RR; ks[i + 3] = ks[i]
        ss[i + 1] = ss[i + 2] = ss[i + 3] = ss[i]
    h = q + n // 8
    for i in range(h, h + n // 16, 2):                               # a base and its negative alone: the bucket ends at infinity
        ks[i + 1] = (RR - ks[i]) % RR
        ss[i + 1] = ss[i]
    t = h + n // 16
    for i in range(t, t + 16):                                       # identity bases, scalars 0 and r - 1, one repeated scalar
        ks[i] = 0 if i % 2 else ks[i]
    ss[t + 16] = 0; ss[t + 17] = RR - 1; ss[t + 18] = RR - 1; ks[t + 18] = ks[t + 17]
    for i in range(t + 19, t + 19 + n // 8):
        ss[i] = ss[t + 19]
    return ks, ss


@pytest.mark.parametrize("log_n", [10, 12])
def test_edge_scalars_single_call_and_pipelined(ctx, log_n):
    torch = pytest.importorskip("torch")
    from bls12_381_amd.api import scalars_to_bytes
    n = 1 << log_n
    ks, ss = _edge_case(n, 0xACC0 + log_n)
    want = _want(ks, ss)
    bases = ctx.bases_from_scalars(1, ks)
    assert _encoding(ctx, ctx.msm(bases, ss)) == want, "single call"
    dev = torch.device("cuda", 0)
    sb = scalars_to_bytes(ss)
    d_s = torch.from_numpy(np.ascontiguousarray(sb)).to(dev)
    outs = [torch.zeros(18, dtype=torch.int64, device=dev) for _ in range(3)]
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_pipelining(True)
    try:
        for d_o in outs:
            ctx.msm_device(bases, d_s.data_ptr(), n, d_o.data_ptr())
        ctx.join(0)
        torch.cuda.synchronize()
    finally:
        ctx.set_pipelining(False)
        ctx.set_stream(0)
    for d_o in outs:
        assert _encoding(ctx, d_o.cpu().numpy().view(np.uint64)) == want, "pipelined"


def test_segmented_msm_four_segments(ctx):
    ks, ss = _edge_case(256, 0x5E6)
    bases = ctx.bases_from_scalars(1, ks)
    off = [0, 64, 128, 192, 256]
    got = ctx.msm_segments(bases, ss, off)
    for j in range(4):
        assert _encoding(ctx, got[j]) == _want(ks[off[j]:off[j + 1]], ss[off[j]:off[j + 1]]), "segment %d" % j


def test_uniform_scalars_2_14(ctx):
    n = 1 << 14
    r = o.SplitMix64(0x214)
    ks = [r.scalar() for _ in range(n)]
    ss = [r.scalar() for _ in range(n)]
    bases = ctx.bases_from_scalars(1, ks)
    assert _encoding(ctx, ctx.msm(bases, ss)) == _want(ks, ss)
