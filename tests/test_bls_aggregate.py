"""Aggregate BLS verification on the GPU (blsgpu_bls_fast_aggregate_verify_batch[_device]): one signature over one message by a subset of a
resident key set.  For both modes, 42 aggregates over a registry of 256 keys made as in test_bls_verify_batch_from_bytes_vs_oracle
(keys [sk_j] G, sig_i = (sum of the subset's sk_j) * H(m_i) through mul_batch): subsets of 1, 2, 64 and 200 keys, an empty subset with the
identity signature (holds) and with an honest one (does not), a subset with one index swapped after signing, a wrong message, a signature
that does not decode.  Every verdict against the C oracle's pairings of the ORACLE-summed keys, five entries against the Python oracle end
to end, the size-1 subsets against blsgpu_bls_verify_batch on the same keys' bytes, and the device form against the host form."""
import numpy as np
import pytest

from oracle import bls12_381_ref as o

import g_sum_points as gp
from g_ntt_points import G

pytestmark = pytest.mark.gpu

NKEYS = 256


@pytest.fixture(scope="module")
def ctx():
    import bls12_381_amd as b
    return b.default_context()


def _scalar_bytes(vals):
    return np.stack([np.frombuffer((int(v) % o.R_ORDER).to_bytes(32, "little"), dtype=np.uint8) for v in vals])


def _oracle_affine(group, xy, inf):
    """(n, 12 | 24) u64 affine wire + flags -> oracle affine triples"""
    f = o.fp_from_mont_limbs
    out = []
    for row, i in zip(xy, inf):
        r = [int(v) for v in row]
        if i:
            out.append(o.G1_IDENTITY_AFF if group == 1 else o.G2_IDENTITY_AFF)
        elif group == 1:
            out.append((f(r[:6]), f(r[6:]), False))
        else:
            out.append(((f(r[:6]), f(r[6:12])), (f(r[12:18]), f(r[18:])), False))
    return out


@pytest.mark.parametrize("mode", [0, 1])
def test_fast_aggregate_verify_vs_oracle(ctx, mode):
    import torch
    from oracle import h2c_ref as h
    from oracle import c_oracle
    c_oracle.build()
    dev = torch.device("cuda", 0)
    gk, gs = (1, 2) if mode == 0 else (2, 1)                                 # group of the keys / of the signatures
    dst = b"BLS_SIG_BLS12381G%d_XMD:SHA-256_SSWU_RO_POP_" % gs
    rs = np.random.RandomState(1200 + mode)
    sks = [int.from_bytes(rs.randint(0, 256, size=32, dtype=np.uint8).tobytes(), "little") >> 3 for _ in range(NKEYS)]
    kxy, kinf = ctx.bases_from_scalars(gk, _scalar_bytes(sks)).download()
    # the subsets: sizes 1, 2, 64, 200, then the special entries
    sizes = [1] * 10 + [2] * 8 + [64] * 8 + [200] * 6
    subsets = [sorted(int(k) for k in rs.choice(NKEYS, size=s, replace=False)) for s in sizes]
    E_ID, E_HONEST, SWAP, WRONG_MSG, BAD_SIG, REPEAT = 32, 33, 34, 35, 36, 37
    subsets += [[], [], list(subsets[20]), list(subsets[11]), list(subsets[12]), [7, 7, 9]]     # a key may sign twice: 2 sk_7 + sk_9
    subsets += [sorted(int(k) for k in rs.choice(NKEYS, size=s, replace=False)) for s in (1, 2, 64, 200)]
    n = len(subsets)
    assert n == 42
    msgs = [bytes(rs.randint(0, 256, size=int(rs.randint(0, 80)), dtype=np.uint8)) for _ in range(n)]
    secret = [sum(sks[k] for k in s) % o.R_ORDER for s in subsets]
    secret[E_HONEST] = 5
    hxy, hinf = ctx.batch_normalize(gs, ctx.hash_to_curve(gs, msgs, dst))
    sig_xy, sig_inf = ctx.batch_normalize(gs, ctx.mul_batch(gs, hxy, hinf, _scalar_bytes(secret)))
    assert sig_inf[E_ID] == 1 and sig_inf.sum() == 1                         # the empty sum of secrets signs with the identity
    sig_b = ctx.points_to_bytes(gs, sig_xy, sig_inf, compressed=True).copy()
    msgs[WRONG_MSG] = msgs[WRONG_MSG] + b"!"
    other = next(k for k in range(NKEYS) if k not in subsets[SWAP])
    subsets[SWAP][3] = other
    for bit in range(8, 64):
        cand = sig_b[BAD_SIG].copy(); cand[bit // 8 + 1] ^= 1 << (bit % 8)
        if not ctx.points_from_bytes(gs, cand[None, :], compressed=True, checked=True)[2][0]:
            sig_b[BAD_SIG] = cand
            break
    expect = np.ones(n, dtype=np.uint8)
    expect[[E_HONEST, SWAP, WRONG_MSG]] = 0
    expect[BAD_SIG] = 3
    # the call: the registry resident on the device, everything else from the host
    d_kxy = torch.from_numpy(kxy.view(np.int64)).to(dev)
    d_kinf = torch.from_numpy(kinf).to(dev)
    got = ctx.bls_fast_aggregate_verify(mode, d_kxy.data_ptr(), d_kinf.data_ptr(), NKEYS, subsets, sig_b, msgs, dst)
    assert got.tolist() == expect.tolist()
    # every verdict: the C oracle's pairings of the oracle-summed keys
    keys_o = _oracle_affine(gk, kxy, kinf)
    from_aff = o.g1_from_affine if gk == 1 else o.g2_from_affine
    grp = G[gk]
    apk = [grp.to_affine(grp.sum(from_aff(keys_o[k]) for k in s)) for s in subsets]
    assert apk[E_ID][2] and apk[E_HONEST][2]
    axy, ainf = gp.wire_points(gk, apk)
    sxy, sinf, sok = ctx.points_from_bytes(gs, sig_b, compressed=True, checked=True)
    hm = ctx.batch_normalize(gs, ctx.hash_to_curve(gs, msgs, dst))
    gen1 = np.tile(gp.wire_points(1, [o.G1_GEN])[0][0], (n, 1)); gen2 = np.tile(gp.wire_points(2, [o.G2_GEN])[0][0], (n, 1)); z = np.zeros(n, dtype=np.uint8)
    if mode == 0:
        lhs = c_oracle.pairing_batch(0, axy, ainf, hm[0], hm[1])[0]; rhs = c_oracle.pairing_batch(0, gen1, z, sxy, sinf)[0]
    else:
        lhs = c_oracle.pairing_batch(0, sxy, sinf, gen2, z)[0]; rhs = c_oracle.pairing_batch(0, hm[0], hm[1], axy, ainf)[0]
    want_all = np.where(sok == 0, 3, (lhs == rhs).all(axis=1).astype(np.uint8)).astype(np.uint8)
    assert np.array_equal(got, want_all) and (sok == 0).sum() == 1 and 2 not in got
    # five entries end to end by the Python oracle: decode, hash, sum, pair
    dec = o.g2_from_compressed if mode == 0 else o.g1_from_compressed
    for i in (0, 12, E_ID, SWAP, WRONG_MSG):
        sg = dec(sig_b[i].tobytes())
        if mode == 0:
            want = int(o.pairing(apk[i], o.g2_to_affine(h.g2_hash_to_curve(msgs[i], dst))) == o.pairing(o.G1_GEN, sg))
        else:
            want = int(o.pairing(sg, o.G2_GEN) == o.pairing(o.g1_to_affine(h.g1_hash_to_curve(msgs[i], dst)), apk[i]))
        assert got[i] == want, (i, want)
    assert dec(sig_b[BAD_SIG].tobytes()) is None
    # subsets of one key: the verdicts of the bulk verifier on that key's bytes
    ones = [i for i, s in enumerate(subsets) if len(s) == 1]
    assert len(ones) == 11
    pk_b = ctx.points_to_bytes(gk, kxy[[subsets[i][0] for i in ones]], kinf[[subsets[i][0] for i in ones]], compressed=True)
    assert ctx.bls_verify_batch(mode, pk_b, sig_b[ones], [msgs[i] for i in ones], dst).tolist() == got[ones].tolist()
    # the device form: the same verdicts
    koff = np.zeros(n + 1, dtype=np.uint64); koff[1:] = np.cumsum([len(s) for s in subsets])
    idx = np.array([k for s in subsets for k in s], dtype=np.uint32)
    moff = np.zeros(n + 1, dtype=np.uint64); moff[1:] = np.cumsum([len(m) for m in msgs])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    d_idx, d_koff, d_sig, d_msgs, d_moff, d_dst = t(idx), t(koff), t(sig_b), t(np.frombuffer(b"".join(msgs), dtype=np.uint8)), t(moff), t(np.frombuffer(dst, dtype=np.uint8))
    d_v = torch.full((n,), 9, dtype=torch.uint8, device=dev)
    ctx.bls_fast_aggregate_verify_device(mode, d_kxy.data_ptr(), d_kinf.data_ptr(), NKEYS, d_idx.data_ptr(), d_koff.data_ptr(), len(idx), d_sig.data_ptr(), d_msgs.data_ptr(),
                                         d_moff.data_ptr(), n, d_dst.data_ptr(), len(dst), d_v.data_ptr())
    ctx.synchronize()
    assert d_v.cpu().numpy().tolist() == got.tolist()
    # the verdicts are n bytes at ANY address: a slice of a larger buffer at an odd offset, as blsgpu_bls_verify_batch_device takes it
    d_big = torch.full((n + 16,), 9, dtype=torch.uint8, device=dev)
    for shift in (3, 5):
        ctx.bls_fast_aggregate_verify_device(mode, d_kxy.data_ptr(), d_kinf.data_ptr(), NKEYS, d_idx.data_ptr(), d_koff.data_ptr(), len(idx), d_sig.data_ptr(), d_msgs.data_ptr(),
                                             d_moff.data_ptr(), n, d_dst.data_ptr(), len(dst), d_big.data_ptr() + shift)
        ctx.synchronize()
        big = d_big.cpu().numpy()
        assert big[shift:shift + n].tolist() == got.tolist() and (big[:shift] == 9).all() and (big[shift + n:] == 9).all()
        d_big.fill_(9)
    one_off = np.concatenate([[0], np.cumsum([len(msgs[i]) for i in ones])]).astype(np.uint64)
    d_pk1, d_sig1, d_msg1, d_off1 = t(pk_b), t(sig_b[ones]), t(np.frombuffer(b"".join(msgs[i] for i in ones), dtype=np.uint8)), t(one_off)
    ctx.bls_verify_batch_device(mode, d_pk1.data_ptr(), d_sig1.data_ptr(), d_msg1.data_ptr(), d_off1.data_ptr(), len(ones), d_dst.data_ptr(), len(dst), d_big.data_ptr() + 3)
    ctx.synchronize()
    assert d_big.cpu().numpy()[3:3 + len(ones)].tolist() == got[ones].tolist()
    # an index outside the registry: refused by the host form, flagged by the device form
    import bls12_381_amd as b
    with pytest.raises(b.BlsGpuError, match="outside the point set"):
        ctx.bls_fast_aggregate_verify(mode, d_kxy.data_ptr(), d_kinf.data_ptr(), NKEYS, [[0, NKEYS]] + subsets[1:], sig_b, msgs, dst)
    assert ctx.bls_fast_aggregate_verify(mode, d_kxy.data_ptr(), d_kinf.data_ptr(), NKEYS, [], sig_b[:0], [], dst).shape == (0,)
