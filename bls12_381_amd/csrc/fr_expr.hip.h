// fr_expr.hip.h -- Fr expression programs (blsgpu_fr_expr_eval*): a small straight-line program, validated once on the host
// (fr_expr_plan.h: frx_prog_build), interpreted per row on the device.  One pass: every column operand is read where it is used, every
// intermediate lives in the lane's register file, only the last instruction's dst goes back to memory -- the row-wise evaluation of a
// constraint expression on an extended coset domain (the quotient's numerator times 1 / Z_H) without one launch, one pass over HBM and
// one temporary per +, - and * of it.
//
// The arithmetic is scalar.hip.h's fr_add / fr_sub / fr_mul (scalar.rs:414-503): canonical in, canonical out, so a row's result is
// limb-identical to the same expression composed from blsgpu_fr_op whatever route got there.
//
// Layout.
//   rows        lane l of workgroup g takes the rows g * block * chunk + e * block + l, e < chunk: consecutive lanes on consecutive rows,
//               so a column operand is two 16-byte global loads per lane, coalesced apart from the wrap of a rotation.  A column of
//               length 1 (a challenge in device memory) is one address for the whole wavefront.  No column passes through LDS.
//   decode      every lane runs the same instruction: the image is read at addresses that depend on the instruction counter alone and
//               the words go through readfirstlane, so the decode, the operand kinds and the op are wave-uniform (scalar registers, no
//               divergence); `#pragma unroll 1` keeps ONE copy of the product in the code.
//   registers   in LDS, not in VGPRs (a dynamically indexed array of eight-word values in VGPRs becomes scratch): two planes of 16-byte
//               halves per register, address ((reg * 2 + half) * block + lane) * 16, so the lanes of a wavefront read and write
//               consecutive 16-byte words (ds_read_b128 / ds_write_b128 without a bank conflict).  A lane touches its own slots only:
//               there is no barrier in the kernel.  block * n_regs * 32 bytes: 64 KB at eight registers, two workgroups per CU.
//               The validation guarantees that no register is read before the SAME row wrote it, so nothing depends on stale LDS.
#pragma once
#include "scalar.hip.h"
#include "fr_expr_plan.h"

namespace bls {

DEV u32* frx_reg_addr(u32* lds, u32 reg, unsigned block, unsigned lane) { return lds + ((size_t)reg * 2 * block + lane) * 4; }
DEV Fr frx_reg_load(const u32* slot, unsigned block) {
  const uint4 a = *reinterpret_cast<const uint4*>(slot), b = *reinterpret_cast<const uint4*>(slot + (size_t)block * 4);
  Fr r; r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w; r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
  return r;
}
DEV void frx_reg_store(u32* slot, unsigned block, const Fr& v) {
  *reinterpret_cast<uint4*>(slot) = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
  *reinterpret_cast<uint4*>(slot + (size_t)block * 4) = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}

// operand word w (wave-uniform) for this lane's row: col_j[(row + rot * 2^log_stride) mod 2^log_len_j] in 64-bit signed arithmetic (a
// two's-complement AND is the mathematical mod of a power of two), a register of the lane, or a constant of the image
DEV Fr frx_operand(u32 w, const u32* __restrict__ prog, const FrxCols& cols, int64_t row, int log_stride, int log_n, const u32* lds, unsigned block, unsigned lane) {
  const u32 kind = frx_kind(w), idx = frx_index(w);
  if (kind == FRX_COL) {
#if defined(FRX_FAULT) && FRX_FAULT == 1
    const int64_t rot = -(int64_t)frx_rot(w);
#else
    const int64_t rot = frx_rot(w);
#endif
#if defined(FRX_FAULT) && FRX_FAULT == 2
    const int log_len = log_n;
#else
    const int log_len = cols.log_len[idx];
    (void)log_n;
#endif
    const int64_t at = (row + rot * ((int64_t)1 << log_stride)) & (((int64_t)1 << log_len) - 1);
    return fr_load(cols.p[idx] + (size_t)at * 8);
  }
  if (kind == FRX_CONST) return fr_load(prog + FRX_CONST_OFF + idx * 8);
  return frx_reg_load(frx_reg_addr(const_cast<u32*>(lds), idx, block, lane), block);
}

// One tile of blockDim.x * chunk rows per workgroup (fr_expr_plan.h: fr_expr_plan); dynamic LDS: blockDim.x * n_regs * 32 bytes.
// prog: the image of frx_prog_build; cols: the pointers and log-lengths of the columns the program reads (the others are never looked
// at); out: 2^log_n scalars that overlap no column read.
__global__ void __launch_bounds__(FRX_BLOCK, 2) k_frx_eval(const u32* __restrict__ prog, const FrxCols cols, int log_n, int log_stride, unsigned chunk, u32* __restrict__ out) {
  BLS_DYN_LDS(lds);
  const size_t rows = (size_t)1 << log_n;
  const unsigned block = blockDim.x, lane = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * block * chunk;
  const u32 n_instr = __builtin_amdgcn_readfirstlane(prog[0]);
#pragma unroll 1
  for (unsigned e = 0; e < chunk; e++) {
    const size_t row = base + (size_t)e * block + lane;
    if (row >= rows) break;
    Fr res = fr_zero();
#pragma unroll 1
    for (u32 i = 0; i < n_instr; i++) {
      const u32* ins = prog + FRX_CODE_OFF + 3 * i;
      const u32 w0 = __builtin_amdgcn_readfirstlane(ins[0]), wa = __builtin_amdgcn_readfirstlane(ins[1]), wb = __builtin_amdgcn_readfirstlane(ins[2]);
      const u32 op = frx_op(w0);
      u32* dst = frx_reg_addr(lds, frx_dst(w0), block, lane);
      const Fr a = frx_operand(wa, prog, cols, (int64_t)row, log_stride, log_n, lds, block, lane);
      if (op == FRX_MOV) {
        res = a;
      } else {
        const Fr b = frx_operand(wb, prog, cols, (int64_t)row, log_stride, log_n, lds, block, lane);
        if (op == FRX_MUL || op == FRX_MAD) {
          res = fr_mul(a, b);
#if !(defined(FRX_FAULT) && FRX_FAULT == 4)
          if (op == FRX_MAD) res = fr_add(frx_reg_load(dst, block), res);
#endif
        } else if (op == FRX_ADD) {
          res = fr_add(a, b);
        } else {
#if defined(FRX_FAULT) && FRX_FAULT == 3
          res = fr_sub(b, a);
#else
          res = fr_sub(a, b);
#endif
        }
      }
#if defined(FRX_FAULT) && FRX_FAULT == 5
      if (e == 0)                                      // the lane's later rows then read the first row's registers
#endif
      frx_reg_store(dst, block, res);
    }
    fr_store(out + row * 8, res);
  }
}

}  // namespace bls
