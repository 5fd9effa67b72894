// kzg.hip.h -- the data movement of amortised KZG openings (blsgpu_kzg_multiproof_*, blsgpu_kzg_cells*): everything between the Fr
// transforms, the segmented MSM and the group transforms that the circulant route (FK20) is made of.  kzg_plan.h holds the index maps,
// the order of the stages and the launch shapes; api_msm.hip launches from it.  Nothing here does field arithmetic except the one
// conversion that gives the wire form of 1 (the Z of an affine SRS point, the Y of an identity record).
//
// A scalar is 32 bytes (two 16-byte words), a projective wire point 144 bytes (nine): every kernel moves whole 16-byte words, so all
// arrays must be 16-byte aligned.  Sizes are count * 2n scalars at most (2^28) and count * 2c points (2^24): indices are 64-bit.
// -DKZG_FAULT=n seeds one fault for tests/test_simt_kzg.py (1: the transposition writes element (t, m) where (m, t) belongs, 2: the zero
// padding of c^_t one slot short, 3: natural numbering of the proofs and cells where the bit-reversed one is asked).
#pragma once
#include "convert.hip.h"
#include "kzg_plan.h"

#ifndef KZG_FAULT
#define KZG_FAULT 0
#endif

namespace bls {

constexpr int KZG_PQ = 9;                                    // 16-byte words of a projective G1 wire point

DEV void kzg_copy_scalar(uint4* dst, const uint4* src) { const uint4 a = src[0], b = src[1]; dst[0] = a; dst[1] = b; }
DEV void kzg_zero_scalar(uint4* dst) { dst[0] = make_uint4(0, 0, 0, 0); dst[1] = make_uint4(0, 0, 0, 0); }
// (0 : 1 : 0), the reference's `identity()`
DEV void kzg_identity_point(uint4* dst) {
  u32 one[12];
  fe_to_ref(fe_one(), one);
#pragma unroll
  for (int q = 0; q < KZG_PQ; q++) dst[q] = q >= 3 && q < 6 ? make_uint4(one[4 * (q - 3)], one[4 * (q - 3) + 1], one[4 * (q - 3) + 2], one[4 * (q - 3) + 3]) : make_uint4(0, 0, 0, 0);
}

// create: S^[t][j] (l vectors of 2c projective points) from the SRS prefix in affine wire form; a lane per point
__global__ void __launch_bounds__(256) k_kzg_srs_rows(const uint4* __restrict__ xy, const uint8_t* __restrict__ inf, uint4* __restrict__ out, int log_c, int log_l) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ((size_t)2 << (log_c + log_l))) return;
  const size_t t = g >> (log_c + 1), j = g & (((size_t)2 << log_c) - 1);
  const int64_t s = kzg_srs_slot(t, j, log_c, log_l);
  uint4* o = out + g * KZG_PQ;
  if (s < 0 || inf[s]) { kzg_identity_point(o); return; }
  u32 one[12];
  fe_to_ref(fe_one(), one);
  const uint4* p = xy + (size_t)s * 6;
#pragma unroll
  for (int q = 0; q < 6; q++) o[q] = p[q];
#pragma unroll
  for (int q = 0; q < 3; q++) o[6 + q] = make_uint4(one[4 * q], one[4 * q + 1], one[4 * q + 2], one[4 * q + 3]);
}

// out[v][i] = in[v][src(i)] over `vecs` vectors of 2^log_v points; a lane per point.  mode 0: src = i; 1: src = bitrev(i, log_v);
// 2: the transposition [t][m] -> [m][t] of create (log_v = log_l + log_c + 1, i = m l + t, src = t 2c + m)
__global__ void __launch_bounds__(256) k_kzg_point_permute(const uint4* __restrict__ in, uint4* __restrict__ out, size_t vecs, int log_v, int mode, int log_c, int log_l) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (vecs << log_v)) return;
  const size_t v = g >> log_v, i = g & (((size_t)1 << log_v) - 1);
  size_t s = i;
#if KZG_FAULT != 3
  if (mode == 1) s = (size_t)kzg_bitrev(i, log_v);
#endif
  if (mode == 2) s = (size_t)kzg_transposed_src(i >> log_l, i & (((size_t)1 << log_l) - 1), log_c);
  const uint4* p = in + ((v << log_v) + s) * KZG_PQ;
  uint4* o = out + g * KZG_PQ;
#pragma unroll
  for (int q = 0; q < KZG_PQ; q++) o[q] = p[q];
}

// identity records over points [first, first + 2^log_cnt) of every vector of 2^log_v points; a lane per record
__global__ void __launch_bounds__(256) k_kzg_identity_fill(uint4* __restrict__ pts, size_t vecs, int log_v, size_t first, int log_cnt) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (vecs << log_cnt)) return;
  const size_t v = g >> log_cnt, i = g & (((size_t)1 << log_cnt) - 1);
  kzg_identity_point(pts + ((v << log_v) + first + i) * KZG_PQ);
}

// out[v][j] = j < 2^log_in ? in[v][brev ? bitrev(j, log_in) : j] : 0 for rows of 2^log_out >= 2^log_in scalars; a lane per scalar of out.
// The copy of an evaluation-form input into scratch (log_out = log_in) and the zero extension of the cells (log_out = log_in + 1).
__global__ void __launch_bounds__(256) k_kzg_scalar_copy(const uint4* __restrict__ in, uint4* __restrict__ out, size_t rows, int log_in, int log_out, int brev) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (rows << log_out)) return;
  const size_t v = g >> log_out, j = g & (((size_t)1 << log_out) - 1);
  if (j >> log_in) { kzg_zero_scalar(out + g * 2); return; }
  const size_t s = brev ? (size_t)kzg_bitrev(j, log_in) : j;
  kzg_copy_scalar(out + g * 2, in + ((v << log_in) + s) * 2);
}

// the rows c^_t: out[(v l + t) 2c + j] from the coefficients p_v; a lane per scalar of out
__global__ void __launch_bounds__(256) k_kzg_coeff_rows(const uint4* __restrict__ p, uint4* __restrict__ out, size_t count, int log_c, int log_l) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int log_n = log_c + log_l;
  if (g >= (count << (log_n + 1))) return;
  const size_t v = g >> (log_n + 1), t = (g >> (log_c + 1)) & (((size_t)1 << log_l) - 1), j = g & (((size_t)2 << log_c) - 1);
  int64_t s = kzg_coeff_slot(t, j, log_c, log_l);
#if KZG_FAULT == 2
  if (j == ((size_t)1 << log_c) + 1 && log_c > 0) s = (int64_t)t;         // the last zero holds p[t]
#endif
  if (s < 0) { kzg_zero_scalar(out + g * 2); return; }
  kzg_copy_scalar(out + g * 2, p + ((v << log_n) + (size_t)s) * 2);
}

// offsets[s] = s l (s <= nseg) and base_first[s] = (s mod 2c) l of the Toeplitz MSM; a lane per segment
__global__ void __launch_bounds__(256) k_kzg_segments(u32* __restrict__ offsets, u32* __restrict__ base_first, size_t nseg, int log_c, int log_l) {
  const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s > nseg) return;
  offsets[s] = kzg_seg_offset(s, log_l);
  if (s < nseg) base_first[s] = kzg_seg_base_first(s, log_c, log_l);
}

// The tiled transposition through LDS: `vecs` matrices of R = 2^log_r rows x C = 2^log_cc columns of scalars, out[v][col][row] =
// in[v][row'][col'] with (row', col') = (row, col), or their bit reversals when brev is set (the bit-reversed cell numbering).  A
// workgroup of T x T lanes owns one tile: lane (y, x) reads source element (r0 + y, c0 + x) -- consecutive lanes, consecutive columns --
// and writes target element (c0 + y, r0 + x) -- consecutive lanes, consecutive rows; rows and columns past the matrix edge are skipped,
// so R and C shorter than, equal to and longer than a tile all work.  The tile is padded to T + 1 columns of 16-byte words.
template <int T>
__global__ void __launch_bounds__(T * T) k_kzg_transpose(const uint4* __restrict__ in, uint4* __restrict__ out, size_t vecs, int log_r, int log_cc, int brev) {
  __shared__ uint4 tile[2][T][T + 1];
  const size_t R = (size_t)1 << log_r, C = (size_t)1 << log_cc;
  const size_t tiles_r = (R + T - 1) / T, tiles_c = (C + T - 1) / T;
  size_t b = blockIdx.x;
  const size_t tc = b % tiles_c; b /= tiles_c;
  const size_t tr = b % tiles_r; b /= tiles_r;
  const size_t v = b;
  const unsigned y = threadIdx.x / T, x = threadIdx.x % T;
#if KZG_FAULT == 3
  brev = 0;
#endif
  if (v < vecs) {
    const size_t r = tr * T + y, cc = tc * T + x;
    if (r < R && cc < C) {
      const size_t sr = brev ? (size_t)kzg_bitrev(r, log_r) : r, sc = brev ? (size_t)kzg_bitrev(cc, log_cc) : cc;
      const uint4* p = in + ((v << (log_r + log_cc)) + (sr << log_cc) + sc) * 2;
      tile[0][y][x] = p[0]; tile[1][y][x] = p[1];
    }
  }
  __syncthreads();
  if (v < vecs) {
    const size_t cc = tc * T + y, r = tr * T + x;
    if (r < R && cc < C) {
#if KZG_FAULT == 1
      uint4* o = out + ((v << (log_r + log_cc)) + ((r << log_cc) + cc)) * 2;
#else
      uint4* o = out + ((v << (log_r + log_cc)) + (cc << log_r) + r) * 2;
#endif
      o[0] = tile[0][x][y]; o[1] = tile[1][x][y];
    }
  }
}

}  // namespace bls
