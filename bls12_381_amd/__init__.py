"""bls12_381_amd -- MI355X-native multi-scalar multiplication and batched pairings for BLS12-381.

Host-side mirror of the zkcrypto/bls12_381 types for the accelerated hot path (see api.py); all compute
runs in hand-written HIP kernels for gfx950 behind the C ABI of include/bls12_381_hip.h.
"""
from ._lib import BlsGpuError, LIB_PATH, load  # noqa: F401
from .api import (  # noqa: F401
    Context, Scalar, G1Affine, G1Projective, G2Affine, G2Projective, Gt, MillerLoopResult, G2Prepared, Bls12,
    ResidentBases, pairing, multi_miller_loop, multi_miller_loop_many, msm_g1, msm_g2, default_context, Group, GroupBases, PreparedG2Table, UNPREPARED, FR_GENERATOR,
    FR_SCAN_SUM, FR_SCAN_PRODUCT, FR_SCAN_HORNER, FR_FRAC_MAX_COLS, FR_FRAC_TILE, FR_ORDER_NATURAL, FR_ORDER_BITREV, FR_POSEIDON_AUTO, FR_POSEIDON_DENSE, FR_POSEIDON_SPARSE, FrMatrix, FrSumcheck, FrPoseidon, fr_limbs_to_int,
    FR_EXPR_ADD, FR_EXPR_SUB, FR_EXPR_MUL, FR_EXPR_MAD, FR_EXPR_MOV, FrExpr, fr_expr_assemble, fr_expr_operand,
    FR_LOOKUP_LDS_ROWS, FR_LOOKUP_MISS, FrLookup, FrEdwards, FrEdwardsBases, KZG_FORM_COEFFS, KZG_FORM_EVALS, KzgCellVerifier, KzgMultiproof,
)
