"""Scalars at the edges of the MSM kernels' recoding and decompositions, shared by tests/test_msm_segments.py (on the GPU) and
tests/test_simt_msm.py (the same kernels emulated on the host).  Test infrastructure only: the product never imports this file."""
from oracle import bls12_381_ref as o


def carry_values():
    """scalars whose 4-bit signed recoding carries through long runs and across the window groups of plain mode (bits 64, 128, 192)
    and of the GLV / psi sub-scalars, plus the top of the range [2^254, r): reduced mod r"""
    rr = o.R_ORDER
    v = []
    for m in range(1, 64):
        t = 1 << (4 * m)
        v += [t - 1, t - 8, t - 9, t, t + 1, int("8" * m, 16), int("9" * m, 16)]
    for b in (64, 128, 192):
        for lo in (0x8, 0x9, 0xF):
            for hi in (0x0, 0x7, 0x8, 0x9, 0xF):
                v.append((lo << (b - 4)) | (hi << b))
        v += [(1 << b) - 1 + (0x8 << b), int("8" * (b // 4), 16) + (0x9 << b), int("9" * (b // 4 + 1), 16), int("F" * (b // 4 + 2), 16),
              (0x8 << (b - 4)) + (1 << (b - 4)) - 1, ((1 << 8) - 1) << (b - 4)]
    for top in (4, 5, 6, 7):
        t = top << 252
        v += [t, t + 1, t + int("8" * 63, 16), t + int("9" * 63, 16), t + (1 << 252) - 1, t + (0x8 << 248), t + (0xF << 188) + (0x9 << 192)]
    v += [rr - 1, rr - 8, rr - 9, rr - (1 << 128), (1 << 254) + (1 << 128) - 1]
    return sorted({x % rr for x in v})


def boundary_values(group):
    """the branch values of the GLV (G1) / psi (G2) split of tests/decomp_model.py"""
    import decomp_model
    return decomp_model.glv_candidates() if group == 1 else decomp_model.gls_candidates()
