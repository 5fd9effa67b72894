// api_fr.hip -- the scalar field Fr: element-wise vector operations, the transforms, scans and batch inversion, Lagrange coefficients, fraction
// scans, evaluation-form openings, sparse products, Poseidon, expression programs, lookup tables, multilinear folds and sumcheck, KZG cell recovery.
#define BLS_TU_NAME "api_fr.hip"
#include "host.h"
#include "fr.hip.h"
#include "fr_plan.h"
#include "fr_scan.hip.h"
#include "fr_frac.hip.h"
#include "fr_bary.hip.h"
#include "fr_spmv.hip.h"
#include "fr_mle.hip.h"
#include "fr_poseidon.hip.h"
#include "fr_edwards.hip.h"
#include "fr_expr.hip.h"
#include "fr_lookup.hip.h"
#include "fr_lagrange.hip.h"
#include "kzg_recover.hip.h"

using namespace bls;

// ---------------------------------------------------------------------------------------------------
// scalar field Fr: element-wise vector operations and the radix-2 transform (fr.hip.h)
// ---------------------------------------------------------------------------------------------------
static int fr_op_check(blsgpu_ctx* c, int op, const void* a, const void* b, size_t n, const void* out) {
  if (!c || (n && (!a || !out))) return bad("fr_op: NULL argument");
  if (op < 0 || op > 6) return bad("fr_op: unknown op");
  if (op <= 2 && n && !b) return bad("fr_op: binary op needs b");
  return BLSGPU_OK;
}
extern "C" int blsgpu_fr_op_device(blsgpu_ctx* c, int op, const void* a, const void* b, size_t n, void* out, void* nonzero_flags) { CTX_CLAIM(c);
  if (int rc = fr_op_check(c, op, a, b, n, out)) return rc;
  if (!n) return BLSGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  KLAUNCH(k_fr_op, dim3(nblk(n, 256)), dim3(256), 0, c->stream, op, (const u32*)a, op <= 2 ? (const u32*)b : (const u32*)nullptr, (u32*)out,
                     (uint8_t*)nonzero_flags, n);
  LAUNCHCHK();
  return BLSGPU_OK;
}
extern "C" int blsgpu_fr_op(blsgpu_ctx* c, int op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out, uint8_t* nonzero_flags) { CTX_CLAIM(c);
  if (int rc = fr_op_check(c, op, a, b, n, out)) return rc;
  if (!n) return BLSGPU_OK;
  HostCall h(c);
  void* da = h.in(c->io_a, a, n * 32);
  void* db = h.in(c->io_b, op <= 2 ? b : nullptr, n * 32);
  void* o = h.out(c->io_out, out, n * 32);
  void* f = (op == 4 && nonzero_flags) ? h.out(c->flags_a, nonzero_flags, n) : nullptr;
  if (h.rc) return h.rc;
  return h.finish(blsgpu_fr_op_device(c, op, da, db, n, o, f));
}
// `Scalar::to_bytes` / `from_bytes` / `from_bytes_wide` over vectors (scalar.rs:284-296, :256-280, :300-331; k_fr_convert)
static int fr_convert_device(blsgpu_ctx* c, int op, const void* in, size_t n, void* out, void* ok) {
  if (!c || (n && (!in || !out))) return bad("fr conversion: NULL argument");
  if (!n) return BLSGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  KLAUNCH(k_fr_convert, dim3(nblk(n, 256)), dim3(256), 0, c->stream, op, (const u32*)in, (u32*)out, (uint8_t*)ok, n);
  LAUNCHCHK();
  return BLSGPU_OK;
}
static int fr_convert_host(blsgpu_ctx* c, int op, const void* in, size_t n, void* out, uint8_t* ok) {
  if (!c || (n && (!in || !out))) return bad("fr conversion: NULL argument");
  if (!n) return BLSGPU_OK;
  HostCall h(c);
  void* di = h.in(c->io_a, in, n * (op == 2 ? 64 : 32));
  void* o = h.out(c->io_out, out, n * 32);
  void* f = ok ? h.out(c->flags_a, ok, n) : nullptr;
  if (h.rc) return h.rc;
  return h.finish(fr_convert_device(c, op, di, n, o, f));
}
extern "C" int blsgpu_fr_to_bytes_device(blsgpu_ctx* c, const void* scalars, size_t n, void* bytes, void* ok) { CTX_CLAIM(c); return fr_convert_device(c, 0, scalars, n, bytes, ok); }
extern "C" int blsgpu_fr_from_bytes_device(blsgpu_ctx* c, const void* bytes, size_t n, void* scalars, void* ok) { CTX_CLAIM(c); return fr_convert_device(c, 1, bytes, n, scalars, ok); }
extern "C" int blsgpu_fr_from_bytes_wide_device(blsgpu_ctx* c, const void* bytes, size_t n, void* scalars) { CTX_CLAIM(c); return fr_convert_device(c, 2, bytes, n, scalars, nullptr); }
extern "C" int blsgpu_fr_to_bytes(blsgpu_ctx* c, const uint64_t* scalars, size_t n, uint8_t* bytes, uint8_t* ok) { CTX_CLAIM(c); return fr_convert_host(c, 0, scalars, n, bytes, ok); }
extern "C" int blsgpu_fr_from_bytes(blsgpu_ctx* c, const uint8_t* bytes, size_t n, uint64_t* scalars, uint8_t* ok) { CTX_CLAIM(c); return fr_convert_host(c, 1, bytes, n, scalars, ok); }
extern "C" int blsgpu_fr_from_bytes_wide(blsgpu_ctx* c, const uint8_t* bytes, size_t n, uint64_t* scalars) { CTX_CLAIM(c); return fr_convert_host(c, 2, bytes, n, scalars, nullptr); }
// in-place transform of 2^log_n scalars in device memory (natural order in and out)
static int fr_ntt_check(blsgpu_ctx* c, const void* data, int log_n) {
  if (!c || !data) return bad("fr_ntt: NULL argument");
  if (log_n < 0 || log_n > 28) return bad("fr_ntt: log_n must be in [0, 28]");
  return BLSGPU_OK;
}
// the twiddle tables of (log_n, direction), built on first use and awaited by every user; fr_tw[dir] is reserved by the caller
// (declared in host.h: the group transforms of api_msm.hip read the same tables)
int fr_twiddles_ready(blsgpu_ctx* c, int log_n, int dir) {
  hipStream_t st = c->stream;
  const size_t half = ((size_t)1 << log_n) >> 1;
  if (c->fr_tw_log[dir] != log_n) {
    KLAUNCH(k_fr_twiddles, dim3(nblk((half + FR_TW_RUN - 1) / FR_TW_RUN, 256)), dim3(256), 0, st, c->fr_tw[dir].as<u32>(), log_n, dir);
    if (log_n > 1) KLAUNCH(k_fr_tw_levels, dim3(nblk(half, 256)), dim3(256), 0, st, c->fr_tw[dir].as<u32>(), log_n);
    LAUNCHCHK();
    c->fr_tw_log[dir] = log_n;
    HIPCHK(hipEventRecord(c->ev_fr[dir], st));
  }
  HIPCHK(hipStreamWaitEvent(st, c->ev_fr[dir], 0));
  return BLSGPU_OK;
}
// n^-1 (pre-scaled like the twiddles) in fr_ninv, likewise
int fr_ninv_ready(blsgpu_ctx* c, int log_n) {
  hipStream_t st = c->stream;
  if (c->fr_ninv_log != log_n) {
    KLAUNCH(k_fr_ninv, dim3(1), dim3(64), 0, st, c->fr_ninv.as<u32>(), log_n); c->fr_ninv_log = log_n;
    HIPCHK(hipEventRecord(c->ev_fr[2], st));
  }
  HIPCHK(hipStreamWaitEvent(st, c->ev_fr[2], 0));
  return BLSGPU_OK;
}
// k_fr_cols needs 144 KB of dynamic LDS per workgroup (gfx950 has 160 KB per CU): asked for once per context
static void fr_cols_probe(blsgpu_ctx* c) {
  if (c->fr_cols_ok >= 0) return;
  int lds_max = 0;
  const size_t want = ((size_t)9 << FR_COLS_LOG) * 4;
  c->fr_cols_ok = 0;
  if (c->fr_cols_want && hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, c->device) == hipSuccess && (size_t)lds_max >= want &&
      hipFuncSetAttribute((const void*)k_fr_cols<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)want) == hipSuccess &&
      hipFuncSetAttribute((const void*)k_fr_cols<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)want) == hipSuccess)
    c->fr_cols_ok = 1;
  (void)hipGetLastError();
}
extern "C" int blsgpu_fr_ntt_device(blsgpu_ctx* c, void* d_data, int log_n, int inverse) { CTX_CLAIM(c);
  if (int rc = fr_ntt_check(c, d_data, log_n)) return rc;
  if (log_n == 0) return BLSGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const int dir = inverse ? 1 : 0;
  const size_t n = (size_t)1 << log_n;
  if (c->fr_tw[dir].reserve(n * 32) || c->fr_tmp.reserve(n * 32) || c->fr_ninv.reserve(64)) { g_err = "hipMalloc(fr scratch) failed"; return BLSGPU_ERR_HIP; }
  if (int rc = fr_twiddles_ready(c, log_n, dir)) return rc;
  u32* data = (u32*)d_data;
  u32* tmp = c->fr_tmp.as<u32>();
  const u32* tw = c->fr_tw[dir].as<u32>();
  const int tl = log_n < FR_TILE_LOG ? log_n : FR_TILE_LOG;
  int lh = log_n - 1;                                   // log2 of the current half-span
  // The tile kernel permutes, so it cannot run in place.  With global passes the first one moves the data to the
  // scratch buffer (the rest run there in place) and the tile kernel brings the result home; a transform that fits
  // one tile goes through the scratch buffer and is copied back.
  const u32* src = data;
  u32* cur = lh >= tl ? tmp : data;
  // round 5: the top log_n - tl stages on column tiles in LDS (k_fr_cols), at most ten stages per pass over the data; needs 144 KB of
  // dynamic LDS per workgroup (gfx950 has 160 KB per CU) -- the stage-pair passes below remain for a device that refuses it and as the
  // A/B twin (BLSGPU_NTT_IMPL=stage)
  fr_cols_probe(c);
  // Measured on MI355X (tools/ntt_time.py): tiles of 2^11 elements, at most seven stages per pass, 512 lanes per workgroup (two workgroups
  // per CU overlap their load / barrier / store phases): 2.52-2.55 ms at 2^24 and 11.2 ms at 2^26 against 2.85-2.91 / 12.2-12.4 ms for the
  // stage-pair passes (-11 % / -10 %); at 2^20 and 2^22 the two are equal within the run-to-run spread (0.155-0.17 / 0.60-0.66 ms): the
  // vector sits in the 256 MB Infinity Cache, a stage-pair pass is 19 us, and every variant costs 7-9 us per stage -- the butterflies'
  // ~375 instructions per multiplication, not the passes over the data, are what the transform pays for.  Below 2^20 the stage-pair
  // passes stay.  BLSGPU_NTT_COLS="tile log2,stages per pass,lanes" overrides the shape for experiments.
  if (c->fr_cols_ok && lh >= tl && (log_n >= 20 || c->fr_cols_want == 2)) {
    int tlog = 11, dmax = 7, block = 512;
    static_assert(FR_COLS_LOG == FR_COLS_LOG_MAX, "limits.h and fr.hip.h disagree on the largest column tile");
    if (c->diag.ntt_cols[0]) { tlog = c->diag.ntt_cols[0]; dmax = c->diag.ntt_cols[1]; block = c->diag.ntt_cols[2]; }
    const int m = lh + 1 - tl, passes = (m + dmax - 1) / dmax;
    for (int ps = 0; ps < passes; ps++) {
      const int d = (lh + 1 - tl + (passes - ps) - 1) / (passes - ps);      // the remaining stages split evenly over the remaining passes
      const int ls = lh - d + 1;
      const int lk = tlog - d < ls ? tlog - d : ls;
      KLAUNCH(k_fr_cols<false>, dim3((unsigned)(n >> (d + lk))), dim3(block), ((size_t)9 << (d + lk)) * 4, st, src, cur, tw, lh, d, lk, (const u32*)nullptr, log_n);
      src = cur; lh -= d;
    }
  }
  while (lh - 1 >= tl) {                                // two stages per pass over the data
    KLAUNCH(k_fr_stage2<false>, dim3(nblk(n / 4, 256)), dim3(256), 0, st, src, cur, tw, log_n, lh, n / 4, (const u32*)nullptr);
    src = cur; lh -= 2;
  }
  if (lh >= tl) { KLAUNCH(k_fr_stage1<false>, dim3(nblk(n / 2, 256)), dim3(256), 0, st, src, cur, tw, log_n, lh, n / 2, (const u32*)nullptr); src = cur; lh--; }
  LAUNCHCHK();
  const u32* scale = nullptr;
  if (inverse) {
    if (int rc = fr_ninv_ready(c, log_n)) return rc;
    scale = c->fr_ninv.as<u32>();
  }
  u32* dst = src == data ? tmp : data;
  KLAUNCH(k_fr_tile<false>, dim3((unsigned)(n >> tl)), dim3(256), ((size_t)9 << tl) * 4, st, src, dst, tw, log_n, tl, scale, n, (const u32*)nullptr, (const u32*)nullptr);
  LAUNCHCHK();
  if (dst != data) HIPCHK(hipMemcpyAsync(data, tmp, n * 32, hipMemcpyDeviceToDevice, st));
  return BLSGPU_OK;
}
extern "C" int blsgpu_fr_ntt(blsgpu_ctx* c, uint64_t* data, int log_n, int inverse) { CTX_CLAIM(c);
  if (int rc = fr_ntt_check(c, data, log_n)) return rc;
  HostCall h(c);
  void* d = h.inout(c->io_a, data, ((size_t)1 << log_n) * 32);
  if (h.rc) return h.rc;
  return h.finish(blsgpu_fr_ntt_device(c, d, log_n, inverse));
}
// ---- k independent transforms in one call, optionally on a coset (fr_plan.h decides the launches) ----------------------------------------
// every argument check of both forms: before any staging, reservation or launch
static int fr_ntt_many_check(blsgpu_ctx* c, const void* data, int log_n, size_t k, const uint64_t* coset) {
  if (!c || (k && !data)) return bad("fr_ntt_many: NULL argument");
  if (log_n < 0 || log_n > 28) return bad("fr_ntt_many: log_n must be in [0, 28]");
  if (k > (((size_t)1 << 28) >> log_n)) return bad("fr_ntt_many: k * 2^log_n must not exceed 2^28");
  if (coset) {
    if (!(coset[0] | coset[1] | coset[2] | coset[3])) return bad("fr_ntt_many: the coset shift must not be zero");
    bool below = false;                              // the limbs as an integer against r, from the top word down
    for (int i = 7; i >= 0; i--) {
      const u32 w = (u32)(coset[i >> 1] >> (32 * (i & 1)));
      if (w != FR_MOD_C.w[i]) { below = w < FR_MOD_C.w[i]; break; }
    }
    if (!below) return bad("fr_ntt_many: the coset shift is not a canonical Scalar (limbs >= r)");
  }
  return BLSGPU_OK;
}
extern "C" int blsgpu_fr_ntt_many_device(blsgpu_ctx* c, void* d_data, int log_n, size_t k, int inverse, const uint64_t* coset) { CTX_CLAIM(c);
  if (int rc = fr_ntt_many_check(c, d_data, log_n, k, coset)) return rc;
  if (!k || log_n == 0) return BLSGPU_OK;             // the plan has no step for these (fr_plan.h): nothing to set up either
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const int dir = inverse ? 1 : 0;
  const size_t n = (size_t)1 << log_n;
  fr_cols_probe(c);
  FrColsShape shape;
  if (c->diag.ntt_cols[0]) { shape.tlog = c->diag.ntt_cols[0]; shape.dmax = c->diag.ntt_cols[1]; shape.block = c->diag.ntt_cols[2]; }
  // the column-tile passes where the single transform takes them: per-vector size from 2^20 (api_fr.hip above), or forced
  const FrPlan plan = fr_plan_many(log_n, k, inverse != 0, coset != nullptr, c->fr_cols_ok && (log_n >= 20 || c->fr_cols_want == 2), shape);
  if (c->fr_tw[dir].reserve(n * 32) || c->fr_ninv.reserve(64) || (plan.needs_tmp && c->fr_tmp.reserve(plan.total * 32)) || (coset && c->fr_cs[dir].reserve(n * 32))) {
    g_err = "hipMalloc(fr scratch) failed"; return BLSGPU_ERR_HIP;
  }
  if (int rc = fr_twiddles_ready(c, log_n, dir)) return rc;
  const u32* cs = nullptr;
  if (coset) {
    if (c->fr_cs_log[dir] != log_n || memcmp(c->fr_cs_g[dir], coset, 32)) {
      FrArg g;
      for (int i = 0; i < 8; i++) g.w[i] = (u32)(coset[i >> 1] >> (32 * (i & 1)));
      KLAUNCH(k_fr_coset_table, dim3(nblk((n + FR_TW_RUN - 1) / FR_TW_RUN, 256)), dim3(256), 0, st, c->fr_cs[dir].as<u32>(), g, log_n, dir);
      LAUNCHCHK();
      c->fr_cs_log[dir] = log_n; memcpy(c->fr_cs_g[dir], coset, 32);
      HIPCHK(hipEventRecord(c->ev_fr_cs[dir], st));
    }
    HIPCHK(hipStreamWaitEvent(st, c->ev_fr_cs[dir], 0));
    cs = c->fr_cs[dir].as<u32>();
  }
  const u32* scale = nullptr;
  if (inverse && !coset) {
    if (int rc = fr_ninv_ready(c, log_n)) return rc;
    scale = c->fr_ninv.as<u32>();
  }
  u32* buf[2] = {(u32*)d_data, c->fr_tmp.as<u32>()};
  const u32* tw = c->fr_tw[dir].as<u32>();
  for (int i = 0; i < plan.n_steps; i++) {
    const FrStep& s = plan.step[i];
    const u32* src = buf[s.src];
    u32* dst = buf[s.dst];
    switch (s.kernel) {
      case FR_K_COLS:
        if (s.coset_in) KLAUNCH(k_fr_cols<true>, dim3(s.grid), dim3(s.block), s.lds, st, src, dst, tw, s.lh, s.d, s.lk, cs, log_n);
        else KLAUNCH(k_fr_cols<false>, dim3(s.grid), dim3(s.block), s.lds, st, src, dst, tw, s.lh, s.d, s.lk, (const u32*)nullptr, log_n);
        break;
      case FR_K_STAGE2:
        if (s.coset_in) KLAUNCH(k_fr_stage2<true>, dim3(s.grid), dim3(s.block), s.lds, st, src, dst, tw, log_n, s.lh, plan.total / 4, cs);
        else KLAUNCH(k_fr_stage2<false>, dim3(s.grid), dim3(s.block), s.lds, st, src, dst, tw, log_n, s.lh, plan.total / 4, (const u32*)nullptr);
        break;
      case FR_K_STAGE1:
        if (s.coset_in) KLAUNCH(k_fr_stage1<true>, dim3(s.grid), dim3(s.block), s.lds, st, src, dst, tw, log_n, s.lh, plan.total / 2, cs);
        else KLAUNCH(k_fr_stage1<false>, dim3(s.grid), dim3(s.block), s.lds, st, src, dst, tw, log_n, s.lh, plan.total / 2, (const u32*)nullptr);
        break;
      default:
        KLAUNCH(k_fr_tile<true>, dim3(s.grid), dim3(s.block), s.lds, st, src, dst, tw, log_n, s.d, scale, plan.total, s.coset_in ? cs : (const u32*)nullptr,
                s.coset_out ? cs : (const u32*)nullptr);
        break;
    }
  }
  LAUNCHCHK();
  return BLSGPU_OK;
}
extern "C" int blsgpu_fr_ntt_many(blsgpu_ctx* c, uint64_t* data, int log_n, size_t k, int inverse, const uint64_t* coset) { CTX_CLAIM(c);
  if (int rc = fr_ntt_many_check(c, data, log_n, k, coset)) return rc;
  if (!k) return BLSGPU_OK;
  HostCall h(c);
  void* d = h.inout(c->io_a, data, (k << log_n) * 32);
  if (h.rc) return h.rc;
  return h.finish(blsgpu_fr_ntt_many_device(c, d, log_n, k, inverse, coset));
}

// ---- recurrences along a vector: segmented scans and batch inversion (fr_scan.hip.h; fr_scan_plan.h decides the launches) -----------------
// every argument check of both forms, before anything is staged, reserved or launched.  *work: there is something to do.
static int fr_scan_check(blsgpu_ctx* c, int op, int exclusive, const void* in, size_t len, size_t k, const void* points, const void* out, bool device, bool* work) {
  *work = false;
  if (!c) return bad("fr_scan_many: NULL context");
  if (op < BLSGPU_FR_SCAN_SUM || op > BLSGPU_FR_SCAN_HORNER) return bad("fr_scan_many: unknown op");
  if (op == BLSGPU_FR_SCAN_HORNER && exclusive) return bad("fr_scan_many: exclusive is not defined for HORNER");
  if (len && k > FRS_MAX_TOTAL / len) return bad("fr_scan_many: k * len must not exceed 2^28");
  if (!len || !k) return BLSGPU_OK;
  if (!in || !out) return bad("fr_scan_many: NULL data pointer");
  if (op == BLSGPU_FR_SCAN_HORNER && !points) return bad("fr_scan_many: HORNER needs points (k scalars)");
  if (device && ((((uintptr_t)in | (uintptr_t)out) & 15) || (op == BLSGPU_FR_SCAN_HORNER && ((uintptr_t)points & 15))))
    return bad("fr_scan_many_device: device pointers must be 16-byte aligned");
  if (in != out && ranges_overlap(in, len * k * 32, out, len * k * 32)) return bad("fr_scan_many: in and out overlap partially (out == in is the in-place form)");
  *work = true;
  return BLSGPU_OK;
}
// the scan and inversion kernels' dynamic LDS (lds_grant, host.h): asked for by both entry points
static int frs_lds_probe(blsgpu_ctx* c) {
  return lds_grant(&c->frs_lds_ready, frs_lds_bytes(FrScanShape()),
                   {(const void*)k_frs_tile<FRS_SUM>, (const void*)k_frs_tile<FRS_PRODUCT>, (const void*)k_frs_tile<FRS_HORNER>, (const void*)k_frs_invert});
}
// the five scratch buffers of a scan-shaped plan (scans and fraction scans): recs[] records of `rec` bytes each, the carries one scalar
static bool frs_scratch_reserve(blsgpu_ctx* c, const size_t* recs, size_t rec) {
  return !(c->frs_agg[0].reserve(recs[FRS_BUF_AGG0] * rec) || c->frs_agg[1].reserve(recs[FRS_BUF_AGG1] * rec) ||
           c->frs_carry[0].reserve(recs[FRS_BUF_CARRY0] * 32) || c->frs_carry[1].reserve(recs[FRS_BUF_CARRY1] * 32) ||
           c->frs_lane.reserve(recs[FRS_BUF_LANE] * rec));
}
// a step's src / dst / carry among them: FRS_BUF_AGG0 .. FRS_BUF_CARRY1, FRS_BUF_NONE = no buffer
static u32* frs_buf(blsgpu_ctx* c, int i) { return i < 0 ? nullptr : (i < 2 ? c->frs_agg[i] : c->frs_carry[i - 2]).as<u32>(); }
// one step of the scan's own kinds (the tile kernel in its three modes, the aggregate kernel in its two): every step of a scan, the
// tail of a fraction scan, whose SCAN pass runs on `out` in place
template <int OP>
static void frs_step(blsgpu_ctx* c, const FrScanStep& s, int exclusive, const u32* in, u32* out, const u32* points, size_t len, size_t k, unsigned chunk) {
  u32* dst = frs_buf(c, s.dst);
  const u32* carry = frs_buf(c, s.carry);
  switch (s.kernel) {
    case FRS_K_SINGLE: case FRS_K_REDUCE: case FRS_K_SCAN:
      KLAUNCH(k_frs_tile<OP>, dim3(s.grid), dim3(s.block), s.lds, c->stream, s.kernel, exclusive, in, out, points, len, k, chunk, dst, carry, c->frs_lane.as<u32>());
      break;
    default:
      KLAUNCH(k_frs_agg<OP>, dim3(s.grid), dim3(s.block), s.lds, c->stream, s.kernel, (const u32*)frs_buf(c, s.src), s.items, chunk, s.kernel == FRS_K_AGG_REDUCE ? dst : (u32*)nullptr,
              carry, s.kernel == FRS_K_AGG_SCAN ? dst : (u32*)nullptr);
      break;
  }
}
template <int OP>
static int fr_scan_launch(blsgpu_ctx* c, const FrScanPlan& plan, int exclusive, const u32* in, size_t len, size_t k, const u32* points, u32* out) {
  for (int i = 0; i < plan.n_steps; i++) frs_step<OP>(c, plan.step[i], exclusive, in, out, points, len, k, FrScanShape().chunk);
  LAUNCHCHK();
  return BLSGPU_OK;
}
extern "C" int blsgpu_fr_scan_many_device(blsgpu_ctx* c, int op, int exclusive, const void* d_in, size_t len, size_t k, const void* d_points, void* d_out) { CTX_CLAIM(c);
  bool work;
  if (int rc = fr_scan_check(c, op, exclusive, d_in, len, k, d_points, d_out, true, &work)) return rc;
  if (!work) return BLSGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  if (int rc = frs_lds_probe(c)) return rc;
  const FrScanPlan plan = fr_scan_plan(len, k);
  if (plan.n_steps < 0) return bad("fr_scan_many: k * len must not exceed 2^28");
  const size_t rec = (size_t)frs_rec_words(op) * 4;
  if (!frs_scratch_reserve(c, plan.recs, rec)) { g_err = "hipMalloc(fr scan scratch) failed"; return BLSGPU_ERR_HIP; }
  const u32* in = (const u32*)d_in; const u32* pts = (const u32*)d_points; u32* out = (u32*)d_out;
  const int ex = exclusive ? 1 : 0;
  if (op == BLSGPU_FR_SCAN_SUM) return fr_scan_launch<FRS_SUM>(c, plan, ex, in, len, k, pts, out);
  if (op == BLSGPU_FR_SCAN_PRODUCT) return fr_scan_launch<FRS_PRODUCT>(c, plan, ex, in, len, k, pts, out);
  return fr_scan_launch<FRS_HORNER>(c, plan, 0, in, len, k, pts, out);
}
extern "C" int blsgpu_fr_scan_many(blsgpu_ctx* c, int op, int exclusive, const uint64_t* values, size_t len, size_t k, const uint64_t* points, uint64_t* out) { CTX_CLAIM(c);
  bool work;
  if (int rc = fr_scan_check(c, op, exclusive, values, len, k, points, out, false, &work)) return rc;
  if (!work) return BLSGPU_OK;
  HostCall h(c);
  void* di = h.in(c->io_a, values, len * k * 32);
  void* dp = h.in(c->io_b, op == BLSGPU_FR_SCAN_HORNER ? points : nullptr, k * 32);
  void* o = h.out(c->io_out, out, len * k * 32);
  if (h.rc) return h.rc;
  return h.finish(blsgpu_fr_scan_many_device(c, op, exclusive, di, len, k, dp, o));
}
static int fr_batch_invert_check(blsgpu_ctx* c, const void* in, size_t n, const void* out, bool device, bool* work) {
  *work = false;
  if (!c) return bad("fr_batch_invert: NULL context");
  if (n > FRS_MAX_TOTAL) return bad("fr_batch_invert: n must not exceed 2^28");
  if (!n) return BLSGPU_OK;
  if (!in || !out) return bad("fr_batch_invert: NULL data pointer");
  if (device && (((uintptr_t)in | (uintptr_t)out) & 15)) return bad("fr_batch_invert_device: device pointers must be 16-byte aligned");
  if (in != out && ranges_overlap(in, n * 32, out, n * 32)) return bad("fr_batch_invert: in and out overlap partially (out == in is the in-place form)");
  *work = true;
  return BLSGPU_OK;
}
extern "C" int blsgpu_fr_batch_invert_device(blsgpu_ctx* c, const void* d_in, size_t n, void* d_out, void* d_nonzero_flags) { CTX_CLAIM(c);
  bool work;
  if (int rc = fr_batch_invert_check(c, d_in, n, d_out, true, &work)) return rc;
  if (!work) return BLSGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  if (int rc = frs_lds_probe(c)) return rc;
  const FrScanPlan plan = fr_invert_plan(n);
  for (int i = 0; i < plan.n_steps; i++) {
    const FrScanStep& s = plan.step[i];
    KLAUNCH(k_frs_invert, dim3(s.grid), dim3(s.block), s.lds, c->stream, (const u32*)d_in, (u32*)d_out, (uint8_t*)d_nonzero_flags, n, (unsigned)FrScanShape().chunk);
  }
  LAUNCHCHK();
  return BLSGPU_OK;
}
extern "C" int blsgpu_fr_batch_invert(blsgpu_ctx* c, const uint64_t* values, size_t n, uint64_t* out, uint8_t* nonzero_flags) { CTX_CLAIM(c);
  bool work;
  if (int rc = fr_batch_invert_check(c, values, n, out, false, &work)) return rc;
  if (!work) return BLSGPU_OK;
  HostCall h(c);
  void* di = h.in(c->io_a, values, n * 32);
  void* o = h.out(c->io_out, out, n * 32);
  void* f = nonzero_flags ? h.out(c->flags_a, nonzero_flags, n) : nullptr;
  if (h.rc) return h.rc;
  return h.finish(blsgpu_fr_batch_invert_device(c, di, n, o, f));
}

// ---- Lagrange coefficients at arbitrary nodes (fr_lagrange.hip.h; fr_lagrange_plan.h decides the launch) ------------------------------
// ONE launch on the context's stream, a function of (nseg, total) alone; scratch of its own.  The caller has run flg_check.
int fr_lagrange_launch(blsgpu_ctx* c, const void* d_nodes, const void* d_offsets, size_t nseg, size_t total, const void* d_points, const void* d_values, void* d_lambda, void* d_y,
                       void* d_flags) {
  if (!nseg) return BLSGPU_OK;
  const FlgPlan plan = flg_plan(nseg, total, d_lambda != nullptr, c->diag.flg_shape);
  if (!plan.ok) return bad("fr_lagrange_segments: the sizes are out of range");
  HIPCHK(hipSetDevice(c->device));
  if (c->flg_pre.reserve(plan.pre_bytes + 16) || c->flg_work.reserve(plan.work_bytes + 16)) { g_err = "hipMalloc(fr lagrange scratch) failed"; return BLSGPU_ERR_HIP; }
  if (plan.shape == FLG_SHAPE_BLOCK)
    KLAUNCH((k_flg_segments<FLG_R, true>), dim3(plan.grid), dim3(plan.block), plan.lds, c->stream, (const u32*)d_nodes, (const u32*)d_offsets, (u32)nseg, (u32)total,
            (const u32*)d_points, (const u32*)d_values, (u32*)d_lambda, (u32*)d_y, (uint8_t*)d_flags, c->flg_work.as<u32>(), c->flg_pre.as<u32>(), plan.team, plan.tile, c->status_word);
  else
    KLAUNCH((k_flg_segments<FLG_R, false>), dim3(plan.grid), dim3(plan.block), plan.lds, c->stream, (const u32*)d_nodes, (const u32*)d_offsets, (u32)nseg, (u32)total,
            (const u32*)d_points, (const u32*)d_values, (u32*)d_lambda, (u32*)d_y, (uint8_t*)d_flags, c->flg_work.as<u32>(), c->flg_pre.as<u32>(), plan.team, plan.tile, c->status_word);
  LAUNCHCHK();
  return BLSGPU_OK;
}
static FlgArgs flg_args(const void* nodes, const void* offsets, size_t nseg, size_t total, const void* points, const void* values, const void* lambda, const void* y,
                        const void* flags, bool device) {
  FlgArgs a;
  a.nodes = nodes; a.offsets = offsets; a.nseg = nseg; a.total = total; a.points = points; a.values = values; a.lambda = lambda; a.y = y; a.flags = flags; a.device = device;
  return a;
}
extern "C" int blsgpu_fr_lagrange_segments_device(blsgpu_ctx* c, const void* d_nodes, const void* d_offsets, size_t nseg, size_t total, const void* d_points, const void* d_values,
                                                  void* d_lambda, void* d_y, void* d_distinct_flags) { CTX_CLAIM(c);
  if (!c) return bad("fr_lagrange_segments: NULL context");
  if (const char* why = flg_check(flg_args(d_nodes, d_offsets, nseg, total, d_points, d_values, d_lambda, d_y, d_distinct_flags, true))) return bad(why);
  return fr_lagrange_launch(c, d_nodes, d_offsets, nseg, total, d_points, d_values, d_lambda, d_y, d_distinct_flags);
}
extern "C" int blsgpu_fr_lagrange_segments(blsgpu_ctx* c, const uint64_t* nodes, const uint32_t* offsets, size_t nseg, const uint64_t* points, const uint64_t* values,
                                           uint64_t* lambda, uint64_t* y, uint8_t* distinct_flags) { CTX_CLAIM(c);
  if (!c) return bad("fr_lagrange_segments: NULL context");
  if (nseg > FLG_MAX_SEGS) return bad("fr_lagrange_segments: nseg must not exceed 2^27");
  if (nseg && !offsets) return bad("fr_lagrange_segments: NULL offsets with segments to do");
  const size_t total = nseg ? offsets[nseg] : 0;
  if (const char* why = flg_check(flg_args(nodes, offsets, nseg, total, points, values, lambda, y, distinct_flags, false))) return bad(why);
  if (const char* why = flg_check_host(offsets, nseg, total)) return bad(why);
  if (!nseg) return BLSGPU_OK;
  HostCall h(c);
  void* dn = h.in(c->io_a, nodes, total * 32);
  void* dv = h.in(c->io_b, values, total * 32);
  void* doff = h.in(c->io_e, offsets, (nseg + 1) * 4);
  void* dp = h.in(c->io_f, points, nseg * 32);
  // lambda and y share the output staging: total scalars, then nseg
  u32* o = (u32*)h.out(c->io_out, nullptr, (total + nseg) * 32);
  void* f = distinct_flags ? h.out(c->flags_a, distinct_flags, nseg) : nullptr;
  if (h.rc) return h.rc;
  if (lambda && total) h.back[h.nback++] = {lambda, o, total * 32};
  if (y) h.back[h.nback++] = {y, o + total * 8, nseg * 32};
  return h.finish(fr_lagrange_launch(c, dn, doff, nseg, total, dp, dv, lambda ? (void*)o : nullptr, y ? (void*)(o + total * 8) : nullptr, f));
}

// ---- fraction scans: permutation grand products and logUp sums (fr_frac.hip.h; fr_frac_plan.h decides the launches) -----------------------
// every argument check of the four forms, before anything is staged, reserved or launched.  xa / xb: num_a / num_b (grand product) or
// mult / nothing (fraction sum).  *work: there is something to do.
static int fr_frac_check(blsgpu_ctx* c, int op, int exclusive, int cols, const void* xa, const void* xb, const void* da, const void* db, size_t pitch, const void* chal, size_t len,
                         size_t k, const void* out, const void* flags, bool device, bool* work) {
  *work = false;
  if (!c) return bad("fr_frac: NULL context");
  if (cols < 1 || cols > FRF_MAX_COLS) return bad("fr_frac: c must be in [1, 8]");
  if (exclusive != 0 && exclusive != 1) return bad("fr_frac: exclusive must be 0 or 1");
  if (len && k > FRS_MAX_TOTAL / len) return bad("fr_frac: k * len must not exceed 2^28");
  if (!len || !k) return BLSGPU_OK;
  const size_t total = len * k;
  if (pitch < total) return bad("fr_frac: pitch must be at least k * len");
  if (pitch > FRS_MAX_TOTAL || (size_t)(cols - 1) * pitch + total > FRS_MAX_TOTAL) return bad("fr_frac: (c - 1) * pitch + k * len must not exceed 2^28");
  if ((op == FRF_GRAND_PRODUCT && !xa) || !da || !chal || !out) return bad("fr_frac: NULL pointer (num_a, den_a, challenges and out are required)");
  if (device && (((uintptr_t)xa | (uintptr_t)xb | (uintptr_t)da | (uintptr_t)db | (uintptr_t)chal | (uintptr_t)out) & 15)) return bad("fr_frac: device pointers must be 16-byte aligned");
  const size_t set = ((size_t)(cols - 1) * pitch + total) * 32, data = total * 32;
  const void* ins[5] = {xa, xb, da, db, chal};
  for (int i = 0; i < 5; i++) {
    if (!ins[i]) continue;
    const size_t bytes = i == 4 ? 64 : set;
    if (ranges_overlap(out, data, ins[i], bytes)) return bad("fr_frac: out overlaps an input (there is no in-place form)");
    if (flags && ranges_overlap(flags, total, ins[i], bytes)) return bad("fr_frac: nonzero_flags overlaps an input");
  }
  if (flags && ranges_overlap(flags, total, out, data)) return bad("fr_frac: nonzero_flags overlaps out");
  *work = true;
  return BLSGPU_OK;
}
template <int OP>
static int fr_frac_launch(blsgpu_ctx* c, const FrFracPlan& plan, int exclusive, int cols, const u32* xa, const u32* xb, const u32* da, const u32* db, size_t pitch, const u32* chal,
                          size_t len, size_t k, u32* out, uint8_t* flags) {
  constexpr int SOP = frf_scan_op(OP);
  const unsigned chunk = (unsigned)plan.shape.chunk;
  for (int i = 0; i < plan.n_steps; i++) {
    const FrScanStep& s = plan.step[i];
    if (s.kernel == FRF_K_FRONT)
      KLAUNCH(k_frf_front<OP>, dim3(s.grid), dim3(s.block), s.lds, c->stream, s.src, exclusive, cols, xa, xb, da, db, pitch, chal, len, k, chunk, out, flags, frs_buf(c, s.dst),
              c->frs_lane.as<u32>());
    else frs_step<SOP>(c, s, exclusive, out, out, nullptr, len, k, chunk);
  }
  LAUNCHCHK();
  return BLSGPU_OK;
}
static int fr_frac_device(blsgpu_ctx* c, int op, int exclusive, int cols, const void* xa, const void* xb, const void* da, const void* db, size_t pitch, const void* chal, size_t len,
                          size_t k, void* out, void* flags) {
  bool work;
  if (int rc = fr_frac_check(c, op, exclusive, cols, xa, xb, da, db, pitch, chal, len, k, out, flags, true, &work)) return rc;
  if (!work) return BLSGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  const FrFracPlan plan = fr_frac_plan(op, cols, len, k, pitch);
  if (plan.n_steps < 0) return bad("fr_frac: a size is out of range");
  const size_t rec = (size_t)frs_rec_words(frf_scan_op(op)) * 4;
  if (!frs_scratch_reserve(c, plan.recs, rec)) { g_err = "hipMalloc(fr frac scratch) failed"; return BLSGPU_ERR_HIP; }
  if (op == FRF_GRAND_PRODUCT)
    return fr_frac_launch<FRF_GRAND_PRODUCT>(c, plan, exclusive, cols, (const u32*)xa, (const u32*)xb, (const u32*)da, (const u32*)db, pitch, (const u32*)chal, len, k, (u32*)out, (uint8_t*)flags);
  return fr_frac_launch<FRF_FRAC_SUM>(c, plan, exclusive, cols, (const u32*)xa, (const u32*)nullptr, (const u32*)da, (const u32*)db, pitch, (const u32*)chal, len, k, (u32*)out, (uint8_t*)flags);
}
// packed sets (pitch = k * len).  A set passed twice (num_a == den_a) is staged once, so the device sees the alias too.
static int fr_frac_host(blsgpu_ctx* c, int op, int exclusive, int cols, const uint64_t* xa, const uint64_t* xb, const uint64_t* da, const uint64_t* db, const uint64_t* chal, size_t len,
                        size_t k, uint64_t* out, uint8_t* flags) {
  bool work;
  const size_t pitch = len && k <= FRS_MAX_TOTAL / len ? len * k : 0;        // an overflowing product is refused by the check before pitch is looked at
  if (int rc = fr_frac_check(c, op, exclusive, cols, xa, xb, da, db, pitch, chal, len, k, out, flags, false, &work)) return rc;
  if (!work) return BLSGPU_OK;
  HostCall h(c);
  const size_t set = (size_t)cols * pitch * 32;
  const void* src[4] = {xa, xb, da, db};
  DevBuf* stage[4] = {&c->io_a, &c->io_b, &c->io_e, &c->io_f};
  void* dev[4] = {nullptr, nullptr, nullptr, nullptr};
  for (int i = 0; i < 4; i++) {
    for (int j = 0; j < i && !dev[i]; j++) if (src[i] && src[j] == src[i]) dev[i] = dev[j];
    if (!dev[i]) dev[i] = h.in(*stage[i], src[i], set);
  }
  void* dc = h.in(c->flags_b, chal, 64);
  void* o = h.out(c->io_out, out, pitch * 32);
  void* f = flags ? h.out(c->flags_a, flags, pitch) : nullptr;
  if (h.rc) return h.rc;
  return h.finish(fr_frac_device(c, op, exclusive, cols, dev[0], dev[1], dev[2], dev[3], pitch, dc, len, k, o, f));
}
extern "C" int blsgpu_fr_grand_product_device(blsgpu_ctx* c, int exclusive, int cols, const void* d_num_a, const void* d_num_b, const void* d_den_a, const void* d_den_b, size_t pitch,
                                              const void* d_challenges, size_t len, size_t k, void* d_out, void* d_nonzero_flags) { CTX_CLAIM(c);
  return fr_frac_device(c, FRF_GRAND_PRODUCT, exclusive, cols, d_num_a, d_num_b, d_den_a, d_den_b, pitch, d_challenges, len, k, d_out, d_nonzero_flags);
}
extern "C" int blsgpu_fr_frac_sum_device(blsgpu_ctx* c, int exclusive, int cols, const void* d_mult, const void* d_den_a, const void* d_den_b, size_t pitch, const void* d_challenges,
                                         size_t len, size_t k, void* d_out, void* d_nonzero_flags) { CTX_CLAIM(c);
  return fr_frac_device(c, FRF_FRAC_SUM, exclusive, cols, d_mult, nullptr, d_den_a, d_den_b, pitch, d_challenges, len, k, d_out, d_nonzero_flags);
}
extern "C" int blsgpu_fr_grand_product(blsgpu_ctx* c, int exclusive, int cols, const uint64_t* num_a, const uint64_t* num_b, const uint64_t* den_a, const uint64_t* den_b,
                                       const uint64_t* challenges, size_t len, size_t k, uint64_t* out, uint8_t* nonzero_flags) { CTX_CLAIM(c);
  return fr_frac_host(c, FRF_GRAND_PRODUCT, exclusive, cols, num_a, num_b, den_a, den_b, challenges, len, k, out, nonzero_flags);
}
extern "C" int blsgpu_fr_frac_sum(blsgpu_ctx* c, int exclusive, int cols, const uint64_t* mult, const uint64_t* den_a, const uint64_t* den_b, const uint64_t* challenges, size_t len,
                                  size_t k, uint64_t* out, uint8_t* nonzero_flags) { CTX_CLAIM(c);
  return fr_frac_host(c, FRF_FRAC_SUM, exclusive, cols, mult, nullptr, den_a, den_b, challenges, len, k, out, nonzero_flags);
}

// ---- polynomials in evaluation form: value at a point and the opening's quotient (fr_bary.hip.h; fr_bary_plan.h decides the launches) ------
// every argument check of the four forms, before anything is staged, reserved or launched.  *work: there is something to do.
static int fr_bary_check(blsgpu_ctx* c, bool open, const void* evals, int log_n, size_t k, const void* points, int order, const void* y, const void* q, bool device, bool* work) {
  *work = false;
  if (!c) return bad("fr_bary: NULL context");
  if (log_n < 0 || log_n > 28) return bad("fr_bary: log_n must be in [0, 28]");
  if (k > (FRB_MAX_TOTAL >> log_n)) return bad("fr_bary: k * 2^log_n must not exceed 2^28");
  if (order != BLSGPU_FR_ORDER_NATURAL && order != BLSGPU_FR_ORDER_BITREV) return bad("fr_bary: unknown order");
  if (!k) return BLSGPU_OK;
  if (!evals || !points || !y || (open && !q)) return bad("fr_bary: NULL pointer");
  if (device && (((uintptr_t)evals | (uintptr_t)points | (uintptr_t)y | (uintptr_t)q) & 15)) return bad("fr_bary: device pointers must be 16-byte aligned");
  const size_t data = (k << log_n) * 32, small = k * 32;
  if (ranges_overlap(y, small, evals, data) || ranges_overlap(y, small, points, small)) return bad("fr_bary: y overlaps evals or points");
  if (open && (ranges_overlap(q, data, evals, data) || ranges_overlap(q, data, points, small) || ranges_overlap(q, data, y, small)))
    return bad("fr_bary: q overlaps evals, points or y (there is no in-place form)");
  *work = true;
  return BLSGPU_OK;
}
template <bool OPEN>
static int fr_bary_launch(blsgpu_ctx* c, const FrBaryPlan& plan, const u32* evals, int log_n, size_t k, const u32* points, int order, u32* y, u32* q) {
  hipStream_t st = c->stream;
  const unsigned chunk = FrBaryShape().chunk;
  const u32* tw = c->fr_tw[0].as<u32>();
  u32* buf[2] = {c->frb_rec.as<u32>(), c->frb_rowrec.as<u32>()};
  for (int i = 0; i < plan.n_steps; i++) {
    const FrBaryStep& s = plan.step[i];
    u32* src = s.src >= 0 ? buf[s.src] : nullptr;
    u32* dst = s.dst >= 0 ? buf[s.dst] : nullptr;
    switch (s.kernel) {
      case FRB_K_ROWS: case FRB_K_TILE:
        KLAUNCH(k_frb_tile<OPEN>, dim3(s.grid), dim3(s.block), s.lds, st, s.kernel, evals, points, tw, log_n, k, order, chunk, y, q, dst);
        break;
      case FRB_K_ROW:
        KLAUNCH(k_frb_row<OPEN>, dim3(s.grid), dim3(s.block), s.lds, st, (const u32*)src, ((size_t)1 << log_n) / plan.tile, (unsigned)plan.tile, points, log_n, k, y, q, dst);
        break;
      default:
        KLAUNCH(k_frb_quot, dim3(s.grid), dim3(s.block), s.lds, st, evals, (const u32*)src, log_n, k, chunk, q);
        break;
    }
  }
  LAUNCHCHK();
  return BLSGPU_OK;
}
static int fr_bary_device(blsgpu_ctx* c, bool open, const void* d_evals, int log_n, size_t k, const void* d_points, int order, void* d_y, void* d_q) {
  bool work;
  if (int rc = fr_bary_check(c, open, d_evals, log_n, k, d_points, order, d_y, d_q, true, &work)) return rc;
  if (!work) return BLSGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  if (int rc = lds_grant(&c->frb_lds_ready, frb_lds_bytes(FrBaryShape()), {(const void*)k_frb_tile<false>, (const void*)k_frb_tile<true>})) return rc;
  const FrBaryPlan plan = fr_bary_plan(log_n, k, open);
  if (plan.n_steps < 0) return bad("fr_bary: k * 2^log_n must not exceed 2^28");
  if (c->frb_rec.reserve(plan.recs[FRB_BUF_REC] * FRB_REC_WORDS * 4) || c->frb_rowrec.reserve(plan.recs[FRB_BUF_ROWREC] * FRB_ROWREC_WORDS * 4) ||
      (log_n && c->fr_tw[0].reserve(((size_t)1 << log_n) * 32))) {
    g_err = "hipMalloc(fr bary scratch) failed"; return BLSGPU_ERR_HIP;
  }
  if (log_n) if (int rc = fr_twiddles_ready(c, log_n, 0)) return rc;      // D[i]: the transform's forward table (no level at log_n = 0)
  if (open) return fr_bary_launch<true>(c, plan, (const u32*)d_evals, log_n, k, (const u32*)d_points, order, (u32*)d_y, (u32*)d_q);
  return fr_bary_launch<false>(c, plan, (const u32*)d_evals, log_n, k, (const u32*)d_points, order, (u32*)d_y, (u32*)nullptr);
}
static int fr_bary_host(blsgpu_ctx* c, bool open, const uint64_t* evals, int log_n, size_t k, const uint64_t* points, int order, uint64_t* y, uint64_t* q) {
  bool work;
  if (int rc = fr_bary_check(c, open, evals, log_n, k, points, order, y, q, false, &work)) return rc;
  if (!work) return BLSGPU_OK;
  HostCall h(c);
  const size_t data = (k << log_n) * 32;
  void* de = h.in(c->io_a, evals, data);
  void* dp = h.in(c->io_b, points, k * 32);
  void* dy = h.out(c->io_out, y, k * 32);
  void* dq = open ? h.out(c->io_e, q, data) : nullptr;
  if (h.rc) return h.rc;
  return h.finish(fr_bary_device(c, open, de, log_n, k, dp, order, dy, dq));
}
extern "C" int blsgpu_fr_bary_eval_many_device(blsgpu_ctx* c, const void* d_evals, int log_n, size_t k, const void* d_points, int order, void* d_y) { CTX_CLAIM(c);
  return fr_bary_device(c, false, d_evals, log_n, k, d_points, order, d_y, nullptr);
}
extern "C" int blsgpu_fr_bary_open_many_device(blsgpu_ctx* c, const void* d_evals, int log_n, size_t k, const void* d_points, int order, void* d_y, void* d_q) { CTX_CLAIM(c);
  return fr_bary_device(c, true, d_evals, log_n, k, d_points, order, d_y, d_q);
}
extern "C" int blsgpu_fr_bary_eval_many(blsgpu_ctx* c, const uint64_t* evals, int log_n, size_t k, const uint64_t* points, int order, uint64_t* y) { CTX_CLAIM(c);
  return fr_bary_host(c, false, evals, log_n, k, points, order, y, nullptr);
}
extern "C" int blsgpu_fr_bary_open_many(blsgpu_ctx* c, const uint64_t* evals, int log_n, size_t k, const uint64_t* points, int order, uint64_t* y, uint64_t* q) { CTX_CLAIM(c);
  return fr_bary_host(c, true, evals, log_n, k, points, order, y, q);
}

// ---- sparse matrix-vector products: a resident CSR matrix times k vectors (fr_spmv.hip.h; fr_spmv_plan.h decides the launches) ------------
// The whole structure is checked ONCE, before a handle exists: the product kernels gather x[col] and index out[row] on trust.
// `what` names the first offender.  Returns true for a valid matrix.
static bool frm_validate_host(size_t n_rows, size_t n_cols, const uint32_t* row_ptr, const uint32_t* col, const uint32_t* val_words, std::string* what) {
  char buf[160];
  if (row_ptr[0] != 0) { *what = "fr_matrix: row_ptr[0] must be 0"; return false; }
  for (size_t i = 0; i < n_rows; i++)
    if (row_ptr[i] > row_ptr[i + 1]) { snprintf(buf, sizeof buf, "fr_matrix: row_ptr decreases at row %zu", i); *what = buf; return false; }
  const size_t nnz = row_ptr[n_rows];
  if (nnz > FRSP_MAX) { *what = "fr_matrix: row_ptr[n_rows] (the number of non-zeros) must not exceed 2^28"; return false; }
  if (nnz && (!col || !val_words)) { *what = "fr_matrix: NULL col / val with non-zeros to read"; return false; }
  for (size_t p = 0; p < nnz; p++)
    if (col[p] >= n_cols) { snprintf(buf, sizeof buf, "fr_matrix: col[%zu] = %u is not below n_cols", p, (unsigned)col[p]); *what = buf; return false; }
  for (size_t p = 0; p < nnz; p++) {
    const uint32_t* w = val_words + p * 8;
    bool lt = false;
    for (int i = 7; i >= 0; i--) { if (w[i] != FR_MOD_C.w[i]) { lt = w[i] < FR_MOD_C.w[i]; break; } }
    if (!lt) { snprintf(buf, sizeof buf, "fr_matrix: val[%zu] is not a canonical Scalar (limbs >= r)", p); *what = buf; return false; }
  }
  return true;
}
static void frm_drop(blsgpu_fr_matrix* m) {
  if (!m) return;
  if (m->row_ptr) hipFree(m->row_ptr);
  if (m->col) hipFree(m->col);
  if (m->val) hipFree(m->val);
  if (m->tile_row) hipFree(m->tile_row);
  if (m->flag) hipFree(m->flag);
  delete m;
}
static int frm_sizes_check(blsgpu_ctx* c, size_t n_rows, size_t n_cols, const void* row_ptr, blsgpu_fr_matrix** out) {
  if (out) *out = nullptr;
  if (!c || !out || !row_ptr) return bad("fr_matrix: NULL argument");
  if (n_rows > FRSP_MAX || n_cols > FRSP_MAX) return bad("fr_matrix: n_rows and n_cols must not exceed 2^28");
  return BLSGPU_OK;
}
static int frm_alloc(blsgpu_ctx* c, blsgpu_fr_matrix* m) {
  const size_t tiles = frsp_tiles(m->nnz);
  HIPCHK(hipMalloc((void**)&m->row_ptr, (m->n_rows + 1) * 4));
  HIPCHK(hipMalloc((void**)&m->col, (m->nnz ? m->nnz : 1) * 4));
  HIPCHK(hipMalloc((void**)&m->val, (m->nnz ? m->nnz : 1) * 32));
  HIPCHK(hipMalloc((void**)&m->tile_row, (tiles + 1) * 4));
  HIPCHK(hipMalloc((void**)&m->flag, 16));
  HIPCHK(hipMemsetAsync(m->flag, 0, 16, c->stream));
  return BLSGPU_OK;
}
// the resident form of a validated matrix whose row_ptr / col / val are already in m's own buffers: fold 2^5 into the values, find the
// tiles' first rows, note whether a row is empty.  Synchronises (upload is a setup call).
static int frm_prepare(blsgpu_ctx* c, blsgpu_fr_matrix* m) {
  const size_t tiles = frsp_tiles(m->nnz);
  size_t span = m->nnz > m->n_rows ? m->nnz : m->n_rows;
  if (tiles + 1 > span) span = tiles + 1;
  if (m->n_rows) {
    KLAUNCH(k_frsp_prepare, dim3(nblk(span, 256)), dim3(256), 0, c->stream, (const u32*)m->row_ptr, (const u32*)m->val, m->val, m->tile_row, m->flag, m->n_rows, m->nnz, tiles,
            (unsigned)(FrSpmvShape().block * FrSpmvShape().chunk));
    LAUNCHCHK();
  }
  u32 flag[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(flag, m->flag, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  m->has_empty = flag[1] != 0;
  return BLSGPU_OK;
}
extern "C" int blsgpu_fr_matrix_upload(blsgpu_ctx* c, size_t n_rows, size_t n_cols, const uint32_t* row_ptr, const uint32_t* col, const uint64_t* val, blsgpu_fr_matrix** out) { CTX_CLAIM(c);
  if (int rc = frm_sizes_check(c, n_rows, n_cols, row_ptr, out)) return rc;
  std::string what;
  if (!frm_validate_host(n_rows, n_cols, row_ptr, col, (const uint32_t*)val, &what)) { g_err = what; return BLSGPU_ERR_ARG; }
  HIPCHK(hipSetDevice(c->device));
  blsgpu_fr_matrix* m = new blsgpu_fr_matrix();
  m->device = c->device; m->n_rows = n_rows; m->n_cols = n_cols; m->nnz = row_ptr[n_rows];
  int rc = frm_alloc(c, m);
  if (!rc) rc = staged_upload(c, m->row_ptr, row_ptr, (n_rows + 1) * 4);
  if (!rc && m->nnz) rc = staged_upload(c, m->col, col, m->nnz * 4);
  if (!rc && m->nnz) rc = staged_upload(c, m->val, val, m->nnz * 32);
  if (!rc) rc = frm_prepare(c, m);
  if (rc) { (void)hipStreamSynchronize(c->stream); frm_drop(m); return rc; }
  *out = m;
  return BLSGPU_OK;
}
extern "C" int blsgpu_fr_matrix_from_device(blsgpu_ctx* c, size_t n_rows, size_t n_cols, const void* d_row_ptr, const void* d_col, const void* d_val, blsgpu_fr_matrix** out) { CTX_CLAIM(c);
  if (int rc = frm_sizes_check(c, n_rows, n_cols, d_row_ptr, out)) return rc;
  if ((((uintptr_t)d_row_ptr | (uintptr_t)d_col) & 3) || ((uintptr_t)d_val & 15)) return bad("fr_matrix_from_device: d_val must be 16-byte aligned, d_row_ptr and d_col 4-byte aligned");
  HIPCHK(hipSetDevice(c->device));
  u32 ends[2] = {0, 0};                          // row_ptr[0], row_ptr[n_rows]: the latter IS the number of non-zeros
  HIPCHK(hipMemcpyAsync(&ends[0], d_row_ptr, 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(&ends[1], (const u32*)d_row_ptr + n_rows, 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (ends[0] != 0) return bad("fr_matrix: row_ptr[0] must be 0");
  const size_t nnz = ends[1];
  if (nnz > FRSP_MAX) return bad("fr_matrix: row_ptr[n_rows] (the number of non-zeros) must not exceed 2^28");
  if (nnz && (!d_col || !d_val)) return bad("fr_matrix: NULL col / val with non-zeros to read");
  blsgpu_fr_matrix* m = new blsgpu_fr_matrix();
  m->device = c->device; m->n_rows = n_rows; m->n_cols = n_cols; m->nnz = nnz;
  auto build = [&]() -> int {
    if (int rc = frm_alloc(c, m)) return rc;
    const size_t span = nnz > n_rows ? nnz : n_rows;
    u32 flag = 0;
    if (span) {
      KLAUNCH(k_frsp_validate, dim3(nblk(span, 256)), dim3(256), 0, c->stream, (const u32*)d_row_ptr, (const u32*)d_col, (const u32*)d_val, n_rows, n_cols, nnz, m->flag);
      LAUNCHCHK();
      HIPCHK(hipMemcpyAsync(&flag, m->flag, 4, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
    }
    if (flag) {                                  // refused: fetch the arrays to NAME the first offender (the slow path of a call that fails anyway)
      std::vector<uint32_t> rp(n_rows + 1), cl(nnz), vl(nnz * 8);
      HIPCHK(hipMemcpy(rp.data(), d_row_ptr, (n_rows + 1) * 4, hipMemcpyDeviceToHost));
      if (nnz) { HIPCHK(hipMemcpy(cl.data(), d_col, nnz * 4, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(vl.data(), d_val, nnz * 32, hipMemcpyDeviceToHost)); }
      std::string what;
      if (frm_validate_host(n_rows, n_cols, rp.data(), cl.data(), vl.data(), &what)) what = "fr_matrix: the matrix did not pass the device check";
      g_err = what;
      return BLSGPU_ERR_ARG;
    }
    HIPCHK(hipMemcpyAsync(m->row_ptr, d_row_ptr, (n_rows + 1) * 4, hipMemcpyDeviceToDevice, c->stream));
    if (nnz) {
      HIPCHK(hipMemcpyAsync(m->col, d_col, nnz * 4, hipMemcpyDeviceToDevice, c->stream));
      HIPCHK(hipMemcpyAsync(m->val, d_val, nnz * 32, hipMemcpyDeviceToDevice, c->stream));
    }
    return frm_prepare(c, m);
  };
  if (int rc = build()) { (void)hipStreamSynchronize(c->stream); frm_drop(m); return rc; }
  *out = m;
  return BLSGPU_OK;
}
extern "C" size_t blsgpu_fr_matrix_rows(const blsgpu_fr_matrix* m) { return m ? m->n_rows : 0; }
extern "C" size_t blsgpu_fr_matrix_cols(const blsgpu_fr_matrix* m) { return m ? m->n_cols : 0; }
extern "C" size_t blsgpu_fr_matrix_nnz(const blsgpu_fr_matrix* m) { return m ? m->nnz : 0; }
extern "C" void blsgpu_fr_matrix_free(blsgpu_fr_matrix* m) {
  if (!m) return;
  handle_quiesce(m->device);               // an asynchronous product may still be reading the matrix
  frm_drop(m);
}
// every argument check of both product forms, before anything is staged, reserved or launched.  *work: there is something to do.
static int fr_spmv_check(blsgpu_ctx* c, const blsgpu_fr_matrix* m, const void* x, size_t k, const void* out, bool device, bool* work) {
  *work = false;
  if (!c) return bad("fr_spmv: NULL context");
  if (!m) return bad("fr_spmv: NULL matrix");
  if (m->device != c->device) return bad("fr_spmv: the matrix lives on another device than the context");
  const size_t big = m->n_rows > m->n_cols ? m->n_rows : m->n_cols;
  if (big && k > FRSP_MAX / big) return bad("fr_spmv: k * max(n_rows, n_cols) must not exceed 2^28");
  if (!k || !m->n_rows) return BLSGPU_OK;
  if (!out || (m->n_cols && !x)) return bad("fr_spmv: NULL x / out with work to do");
  if (device && (((uintptr_t)x | (uintptr_t)out) & 15)) return bad("fr_spmv_device: device pointers must be 16-byte aligned");
  const size_t x_bytes = k * m->n_cols * 32, out_bytes = k * m->n_rows * 32;
  // The second clause only preserves a quirk of the test this replaces: a matrix without columns gathers nothing, so its x is an empty
  // range and overlaps nothing, but a non-NULL x strictly inside out has always been refused.
  const bool empty_x_inside = !x_bytes && (uintptr_t)x > (uintptr_t)out && (uintptr_t)x < (uintptr_t)out + out_bytes;
  if (ranges_overlap(x, x_bytes, out, out_bytes) || empty_x_inside) return bad("fr_spmv: out overlaps x (the gather would race with the stores)");
  *work = true;
  return BLSGPU_OK;
}
extern "C" int blsgpu_fr_spmv_device(blsgpu_ctx* c, const blsgpu_fr_matrix* m, const void* d_x, size_t k, void* d_out) { CTX_CLAIM(c);
  bool work;
  if (int rc = fr_spmv_check(c, m, d_x, k, d_out, true, &work)) return rc;
  if (!work) return BLSGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  const FrSpmvShape shape;
  if (int rc = lds_grant(&c->frsp_lds_ready, frsp_lds_bytes(shape), {(const void*)k_frsp_tile})) return rc;
  const FrSpmvPlan plan = fr_spmv_plan(m->n_rows, m->nnz, k, m->has_empty, shape);
  if (c->frsp_head.reserve(plan.rec_scalars * 32) || c->frsp_tail.reserve(plan.rec_scalars * 32) || c->frsp_meta.reserve(plan.meta_words * 4)) {
    g_err = "hipMalloc(fr spmv scratch) failed"; return BLSGPU_ERR_HIP;
  }
  hipStream_t st = c->stream;
  const u32* x = (const u32*)d_x; u32* out = (u32*)d_out;
  for (int i = 0; i < plan.n_steps; i++) {
    const FrSpmvStep& s = plan.step[i];
    switch (s.kernel) {
      case FRSP_K_FILL:
        HIPCHK(hipMemsetAsync(out, 0, s.items * 32, st));
        break;
      case FRSP_K_TILE:
        KLAUNCH(k_frsp_tile, dim3(s.grid), dim3(s.block), s.lds, st, (const u32*)m->row_ptr, (const u32*)m->col, (const u32*)m->val, (const u32*)m->tile_row, m->n_rows, m->n_cols, m->nnz,
                x, out, k, (unsigned)shape.chunk, c->frsp_head.as<u32>(), c->frsp_tail.as<u32>(), c->frsp_meta.as<u32>());
        break;
      default:
        KLAUNCH(k_frsp_fixup, dim3(s.grid), dim3(s.block), s.lds, st, (const u32*)m->row_ptr, (const u32*)c->frsp_head.as<u32>(), (const u32*)c->frsp_tail.as<u32>(),
                (const u32*)c->frsp_meta.as<u32>(), s.items, m->n_rows, k, (unsigned)plan.tile, out);
        break;
    }
  }
  LAUNCHCHK();
  return BLSGPU_OK;
}
extern "C" int blsgpu_fr_spmv(blsgpu_ctx* c, const blsgpu_fr_matrix* m, const uint64_t* x, size_t k, uint64_t* out) { CTX_CLAIM(c);
  bool work;
  if (int rc = fr_spmv_check(c, m, x, k, out, false, &work)) return rc;
  if (!work) return BLSGPU_OK;
  HostCall h(c);
  void* dx = h.in(c->io_a, x, k * m->n_cols * 32);
  void* o = h.out(c->io_out, out, k * m->n_rows * 32);
  if (h.rc) return h.rc;
  if (!dx) { if (!h.reserve(c->io_a, 16)) return h.rc; dx = c->io_a.p; }      // n_cols == 0: nothing is gathered, but the device form wants a pointer
  return h.finish(blsgpu_fr_spmv_device(c, m, dx, k, o));
}

// ---- Poseidon over Fr: permutations, hashes, Merkle trees (fr_poseidon.hip.h; fr_poseidon_plan.h validates, derives and plans) ------------
extern "C" int blsgpu_fr_poseidon_create(blsgpu_ctx* c, int t, int r_full, int r_partial, const uint64_t* round_constants, const uint64_t* mds, int form, blsgpu_fr_poseidon** out) { CTX_CLAIM(c);
  if (out) *out = nullptr;
  if (!c || !out) return bad("fr_poseidon: NULL context / out");
  FrPoseidonHost h;
  const std::string what = fr_poseidon_build(t, r_full, r_partial, round_constants, mds, form, &h);
  if (!what.empty()) { g_err = what; return BLSGPU_ERR_ARG; }
  HIPCHK(hipSetDevice(c->device));
  blsgpu_fr_poseidon* p = new blsgpu_fr_poseidon();
  p->device = c->device; p->t = t; p->r_full = r_full; p->r_partial = r_partial; p->form = h.form; p->args = h.args; p->products = h.products;
  const hipError_t e = device_image(&p->image, h.image.data(), h.image.size() * 4);
  if (e != hipSuccess) { delete p; return fail("fr_poseidon: upload of the constant image", e, __LINE__); }
  *out = p;
  return BLSGPU_OK;
}
extern "C" int blsgpu_fr_poseidon_width(const blsgpu_fr_poseidon* p) { return p ? p->t : 0; }
extern "C" int blsgpu_fr_poseidon_rounds_full(const blsgpu_fr_poseidon* p) { return p ? p->r_full : 0; }
extern "C" int blsgpu_fr_poseidon_rounds_partial(const blsgpu_fr_poseidon* p) { return p ? p->r_partial : 0; }
extern "C" int blsgpu_fr_poseidon_form(const blsgpu_fr_poseidon* p) { return p ? p->form : 0; }
extern "C" size_t blsgpu_fr_poseidon_products(const blsgpu_fr_poseidon* p) { return p ? p->products : 0; }
extern "C" void blsgpu_fr_poseidon_free(blsgpu_fr_poseidon* p) {
  if (!p) return;
  handle_quiesce(p->device);               // an asynchronous call may still be reading the image
  if (p->image) hipFree(p->image);
  delete p;
}
static int frp_handle_check(blsgpu_ctx* c, const blsgpu_fr_poseidon* p) {
  if (!c) return bad("fr_poseidon: NULL context");
  if (!p) return bad("fr_poseidon: NULL handle");
  if (p->device != c->device) return bad("fr_poseidon: the handle lives on another device than the context");
  return BLSGPU_OK;
}
static int frp_tag_check(const uint64_t* tag, FrArg* out) {
  if (!tag) return bad("fr_poseidon: NULL tag");
  if (!frp_below_r(tag)) return bad("fr_poseidon: tag is not a canonical Scalar (limbs >= r)");
  for (int w = 0; w < 4; w++) { out->w[2 * w] = (u32)tag[w]; out->w[2 * w + 1] = (u32)(tag[w] >> 32); }
  return BLSGPU_OK;
}
// every argument check of permute / hash_many in both forms, before anything is staged or launched.  *work: there is something to do.
static int frp_many_check(blsgpu_ctx* c, const blsgpu_fr_poseidon* p, bool hash, const uint64_t* tag, FrArg* tg, const void* in, size_t n, const void* out, bool device, bool* work) {
  *work = false;
  if (int rc = frp_handle_check(c, p)) return rc;
  if (hash) if (int rc = frp_tag_check(tag, tg)) return rc;
  if (n > FRP_MAX_TOTAL / (size_t)p->t) return bad("fr_poseidon: n * t must not exceed 2^28");
  if (!n) return BLSGPU_OK;
  if (!in || !out) return bad("fr_poseidon: NULL pointer with work to do");
  if (device && (((uintptr_t)in | (uintptr_t)out) & 15)) return bad("fr_poseidon: device pointers must be 16-byte aligned");
  const size_t in_bytes = n * (size_t)(hash ? p->t - 1 : p->t) * 32, out_bytes = n * (size_t)(hash ? 1 : p->t) * 32;
  if (!(!hash && in == out) && ranges_overlap(in, in_bytes, out, out_bytes))
    return bad(hash ? "fr_poseidon_hash_many: out overlaps the inputs" : "fr_poseidon_permute: out overlaps the states (only out == states, the in-place form, is allowed)");
  *work = true;
  return BLSGPU_OK;
}
// one step of a plan on the kernels of the handle's width and form
template <int T, bool SP>
static void frp_launch_step(hipStream_t st, const blsgpu_fr_poseidon* p, const FrPoseidonStep& s, const FrArg& tag, const u32* src, u32* dst, u32* roots) {
  const dim3 grid(s.grid), block(s.block);
  switch (s.kernel) {
    case FRP_K_PERMUTE: KLAUNCH((k_frp_permute<T, SP>), grid, block, 0, st, p->args, (const u32*)p->image, src, dst, s.items); break;
    default: KLAUNCH((k_frp_hash<T, SP>), grid, block, 0, st, p->args, (const u32*)p->image, tag, src, dst, roots, s.items); break;      // HASH, LEVEL
  }
}
static int frp_run_plan(blsgpu_ctx* c, const blsgpu_fr_poseidon* p, const FrPoseidonPlan& plan, const FrArg& tag, const u32* in, u32* out, u32* nodes) {
  hipStream_t st = c->stream;
  for (int i = 0; i < plan.n_steps; i++) {
    const FrPoseidonStep& s = plan.step[i];
    if (s.kernel == FRP_K_COPY) { HIPCHK(hipMemcpyAsync(out, in, s.items * 32, hipMemcpyDeviceToDevice, st)); continue; }
    const u32* src = (s.src == FRP_BUF_IN ? in : (const u32*)nodes) + s.src_off * 8;
    u32* dst = (s.dst == FRP_BUF_OUT ? out : nodes) + s.dst_off * 8;
    u32* roots = s.roots && s.dst != FRP_BUF_OUT ? out : nullptr;      // the roots next to the nodes array
#define FRP_CASE(T) case T: if (p->form == FRP_FORM_SPARSE) frp_launch_step<T, true>(st, p, s, tag, src, dst, roots); else frp_launch_step<T, false>(st, p, s, tag, src, dst, roots); break;
    switch (p->t) { FRP_CASE(2) FRP_CASE(3) FRP_CASE(4) FRP_CASE(5) FRP_CASE(9) FRP_CASE(12) default: return bad("fr_poseidon: no kernel for this width"); }
#undef FRP_CASE
  }
  LAUNCHCHK();
  return BLSGPU_OK;
}
static int frp_many_device(blsgpu_ctx* c, const blsgpu_fr_poseidon* p, bool hash, const uint64_t* tag, const void* d_in, size_t n, void* d_out) {
  bool work; FrArg tg = {};
  if (int rc = frp_many_check(c, p, hash, tag, &tg, d_in, n, d_out, true, &work)) return rc;
  if (!work) return BLSGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  const FrPoseidonPlan plan = fr_poseidon_many_plan(hash ? FRP_K_HASH : FRP_K_PERMUTE, p->t, n);
  if (plan.n_steps < 0) return bad("fr_poseidon: n * t must not exceed 2^28");
  return frp_run_plan(c, p, plan, tg, (const u32*)d_in, (u32*)d_out, nullptr);
}
static int frp_many_host(blsgpu_ctx* c, const blsgpu_fr_poseidon* p, bool hash, const uint64_t* tag, const uint64_t* in, size_t n, uint64_t* out) {
  bool work; FrArg tg = {};
  if (int rc = frp_many_check(c, p, hash, tag, &tg, in, n, out, false, &work)) return rc;
  if (!work) return BLSGPU_OK;
  HostCall h(c);
  void* di = h.in(c->io_a, in, n * (size_t)(hash ? p->t - 1 : p->t) * 32);
  void* dout = h.out(c->io_out, out, n * (size_t)(hash ? 1 : p->t) * 32);
  if (h.rc) return h.rc;
  return h.finish(frp_many_device(c, p, hash, tag, di, n, dout));
}
extern "C" int blsgpu_fr_poseidon_permute_device(blsgpu_ctx* c, const blsgpu_fr_poseidon* p, const void* d_states, size_t n, void* d_out) { CTX_CLAIM(c);
  return frp_many_device(c, p, false, nullptr, d_states, n, d_out);
}
extern "C" int blsgpu_fr_poseidon_permute(blsgpu_ctx* c, const blsgpu_fr_poseidon* p, const uint64_t* states, size_t n, uint64_t* out) { CTX_CLAIM(c);
  return frp_many_host(c, p, false, nullptr, states, n, out);
}
extern "C" int blsgpu_fr_poseidon_hash_many_device(blsgpu_ctx* c, const blsgpu_fr_poseidon* p, const uint64_t tag[4], const void* d_inputs, size_t n, void* d_out) { CTX_CLAIM(c);
  return frp_many_device(c, p, true, tag, d_inputs, n, d_out);
}
extern "C" int blsgpu_fr_poseidon_hash_many(blsgpu_ctx* c, const blsgpu_fr_poseidon* p, const uint64_t tag[4], const uint64_t* inputs, size_t n, uint64_t* out) { CTX_CLAIM(c);
  return frp_many_host(c, p, true, tag, inputs, n, out);
}
// every argument check of merkle in both forms; *plan: the launches (n_steps == 0: nothing to do)
static int frp_merkle_check(blsgpu_ctx* c, const blsgpu_fr_poseidon* p, const uint64_t* tag, FrArg* tg, const void* leaves, int height, size_t k, const void* nodes, const void* roots,
                            bool device, FrPoseidonPlan* plan) {
  plan->n_steps = 0;
  if (int rc = frp_handle_check(c, p)) return rc;
  if (int rc = frp_tag_check(tag, tg)) return rc;
  if (height < 0 || height > 28) return bad("fr_poseidon_merkle: height must be in [0, 28]");
  *plan = fr_poseidon_merkle_plan(p->t, height, k, nodes != nullptr);
  if (plan->n_steps < 0) { plan->n_steps = 0; return bad("fr_poseidon_merkle: k * (t-1)^height and the node count must not exceed 2^28"); }
  if (!k) return BLSGPU_OK;
  if (!leaves || !roots) { plan->n_steps = 0; return bad("fr_poseidon_merkle: NULL leaves / roots with work to do"); }
  if (device && (((uintptr_t)leaves | (uintptr_t)nodes | (uintptr_t)roots) & 15)) { plan->n_steps = 0; return bad("fr_poseidon_merkle: device pointers must be 16-byte aligned"); }
  const size_t lb = plan->leaves * 32, nb = plan->node_count * 32, rb = k * 32;
  if (ranges_overlap(leaves, lb, roots, rb) || ranges_overlap(leaves, lb, nodes, nb) || ranges_overlap(nodes, nb, roots, rb)) {
    plan->n_steps = 0;
    return bad("fr_poseidon_merkle: leaves, nodes and roots must not overlap");
  }
  return BLSGPU_OK;
}
static int frp_merkle_device(blsgpu_ctx* c, const blsgpu_fr_poseidon* p, const uint64_t* tag, const void* d_leaves, int height, size_t k, void* d_nodes, void* d_roots) {
  FrPoseidonPlan plan; FrArg tg = {};
  if (int rc = frp_merkle_check(c, p, tag, &tg, d_leaves, height, k, d_nodes, d_roots, true, &plan)) return rc;
  if (!plan.n_steps) return BLSGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  u32* nodes = (u32*)d_nodes;
  if (!nodes && plan.scratch) {
    if (c->frp_nodes.reserve(plan.scratch * 32)) { g_err = "hipMalloc(fr poseidon scratch) failed"; return BLSGPU_ERR_HIP; }
    nodes = c->frp_nodes.as<u32>();
  }
  return frp_run_plan(c, p, plan, tg, (const u32*)d_leaves, (u32*)d_roots, nodes);
}
extern "C" int blsgpu_fr_poseidon_merkle_device(blsgpu_ctx* c, const blsgpu_fr_poseidon* p, const uint64_t tag[4], const void* d_leaves, int height, size_t k, void* d_nodes, void* d_roots) { CTX_CLAIM(c);
  return frp_merkle_device(c, p, tag, d_leaves, height, k, d_nodes, d_roots);
}
extern "C" int blsgpu_fr_poseidon_merkle(blsgpu_ctx* c, const blsgpu_fr_poseidon* p, const uint64_t tag[4], const uint64_t* leaves, int height, size_t k, uint64_t* nodes, uint64_t* roots) { CTX_CLAIM(c);
  FrPoseidonPlan plan; FrArg tg = {};
  if (int rc = frp_merkle_check(c, p, tag, &tg, leaves, height, k, nodes, roots, false, &plan)) return rc;
  if (!plan.n_steps) return BLSGPU_OK;
  HostCall h(c);
  void* dl = h.in(c->io_a, leaves, plan.leaves * 32);
  void* dn = nodes && plan.node_count ? h.out(c->io_e, nodes, plan.node_count * 32) : nullptr;
  void* dr = h.out(c->io_out, roots, k * 32);
  if (h.rc) return h.rc;
  return h.finish(frp_merkle_device(c, p, tag, dl, height, k, dn, dr));
}

// ---- twisted Edwards groups over Fr: checks, normalisation, products, fixed-base tables, segmented MSMs (fr_edwards.hip.h; fr_edwards_plan.h
// holds the limits, every argument check, the recoding, the table layout and the plans) ---------------------------------------------------------
static EdArgs fred_kargs(const uint32_t* a, const uint32_t* d) {
  EdArgs k;
  for (int i = 0; i < 8; i++) { k.a.w[i] = a[i]; k.d.w[i] = d[i]; }
  return k;
}
extern "C" int blsgpu_fr_edwards_create(blsgpu_ctx* c, const uint64_t a[4], const uint64_t d[4], blsgpu_fr_edwards** out) { CTX_CLAIM(c);
  if (out) *out = nullptr;
  if (!c || !out) return bad("fr_edwards_create: NULL context / out");
  FredCurve cv;
  if (const char* what = fred_curve_check(a, d, &cv)) return bad(what);
  blsgpu_fr_edwards* e = new blsgpu_fr_edwards();
  e->device = c->device; e->complete = cv.complete;
  for (int w = 0; w < 4; w++) { e->a[2 * w] = (u32)a[w]; e->a[2 * w + 1] = (u32)(a[w] >> 32); e->d[2 * w] = (u32)d[w]; e->d[2 * w + 1] = (u32)(d[w] >> 32); }
  for (int w = 0; w < 4; w++) { e->a64[w] = a[w]; e->d64[w] = d[w]; }
  *out = e;
  return BLSGPU_OK;
}
extern "C" int blsgpu_fr_edwards_complete(const blsgpu_fr_edwards* e) { return e ? e->complete : 0; }
extern "C" void blsgpu_fr_edwards_free(blsgpu_fr_edwards* e) {
  if (!e) return;
  handle_quiesce(e->device);               // the rule of every handle's free; the constants themselves travel by value
  delete e;
}
static int fred_handle_check(blsgpu_ctx* c, const blsgpu_fr_edwards* e) {
  if (!c) return bad("fr_edwards: NULL context");
  if (!e) return bad("fr_edwards: NULL curve");
  if (e->device != c->device) return bad("fr_edwards: the curve was created for another device than the context");
  return BLSGPU_OK;
}
// a host form's verdict: the sticky word of a synchronous call means a scalar with a bit at or above `bits`
static int fred_finish(HostCall& h, int core_rc) {
  const int rc = h.finish(core_rc);
  if (rc == BLSGPU_ERR_ARG && h.status_host) g_err = "fr_edwards: a scalar has a bit set at or above `bits` (the value of that output is unspecified)";
  return rc;
}

extern "C" int blsgpu_fr_edwards_check_device(blsgpu_ctx* c, const blsgpu_fr_edwards* e, const void* d_xy, size_t n, void* d_ok) { CTX_CLAIM(c);
  if (int rc = fred_handle_check(c, e)) return rc;
  if (const char* what = fred_check_args(d_xy, n, d_ok, true)) return bad(what);
  if (!n) return BLSGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  const FredLaunch l = fred_points_launch(n);
  KLAUNCH(k_fred_check, dim3(l.grid), dim3(l.block), 0, c->stream, fred_kargs(e->a, e->d), (const u32*)d_xy, n, (uint8_t*)d_ok);
  LAUNCHCHK();
  return BLSGPU_OK;
}
extern "C" int blsgpu_fr_edwards_check(blsgpu_ctx* c, const blsgpu_fr_edwards* e, const uint64_t* xy, size_t n, uint8_t* ok) { CTX_CLAIM(c);
  if (int rc = fred_handle_check(c, e)) return rc;
  if (const char* what = fred_check_args(xy, n, ok, false)) return bad(what);
  if (!n) return BLSGPU_OK;
  HostCall h(c);
  void* dx = h.in(c->io_a, xy, n * 64);
  void* dk = h.out(c->flags_a, ok, n);
  if (h.rc) return h.rc;
  return h.finish(blsgpu_fr_edwards_check_device(c, e, dx, n, dk));
}

extern "C" int blsgpu_fr_edwards_normalize_device(blsgpu_ctx* c, const blsgpu_fr_edwards* e, const void* d_xyz, size_t n, void* d_xy, void* d_ok) { CTX_CLAIM(c);
  if (int rc = fred_handle_check(c, e)) return rc;
  if (const char* what = fred_normalize_args(d_xyz, n, d_xy, d_ok, true)) return bad(what);
  if (!n) return BLSGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  const FredLaunch l = fred_points_launch(n);
  KLAUNCH(k_fred_normalize<false>, dim3(l.grid), dim3(l.block), l.lds, c->stream, fred_kargs(e->a, e->d), (const u32*)d_xyz, n, (u32*)d_xy, (uint8_t*)d_ok);
  LAUNCHCHK();
  return BLSGPU_OK;
}
extern "C" int blsgpu_fr_edwards_normalize(blsgpu_ctx* c, const blsgpu_fr_edwards* e, const uint64_t* xyz, size_t n, uint64_t* xy, uint8_t* ok) { CTX_CLAIM(c);
  if (int rc = fred_handle_check(c, e)) return rc;
  if (const char* what = fred_normalize_args(xyz, n, xy, ok, false)) return bad(what);
  if (!n) return BLSGPU_OK;
  HostCall h(c);
  void* di = h.in(c->io_a, xyz, n * 96);
  void* dx = h.out(c->io_out, xy, n * 64);
  void* dk = ok ? h.out(c->flags_a, ok, n) : nullptr;
  if (h.rc) return h.rc;
  return h.finish(blsgpu_fr_edwards_normalize_device(c, e, di, n, dx, dk));
}

extern "C" int blsgpu_fr_edwards_mul_batch_device(blsgpu_ctx* c, const blsgpu_fr_edwards* e, const void* d_xy, const void* d_scalars, int bits, size_t n, void* d_out_xyz) { CTX_CLAIM(c);
  if (int rc = fred_handle_check(c, e)) return rc;
  if (const char* what = fred_mul_args(d_xy, d_scalars, bits, n, d_out_xyz, true)) return bad(what);
  if (!n) return BLSGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  const FredMulPlan p = fred_mul_plan(n, bits);
  if (!p.ok) return bad("fr_edwards_mul_batch: no plan for these sizes");
  KLAUNCH(k_fred_mul, dim3(p.mul.grid), dim3(p.mul.block), p.mul.lds, c->stream, fred_kargs(e->a, e->d), (const u32*)d_xy, (const u32*)d_scalars, bits, n, (u32*)d_out_xyz,
          c->status_word);
  LAUNCHCHK();
  return BLSGPU_OK;
}
extern "C" int blsgpu_fr_edwards_mul_batch(blsgpu_ctx* c, const blsgpu_fr_edwards* e, const uint64_t* xy, const uint8_t* scalars, int bits, size_t n, uint64_t* out_xyz) { CTX_CLAIM(c);
  if (int rc = fred_handle_check(c, e)) return rc;
  if (const char* what = fred_mul_args(xy, scalars, bits, n, out_xyz, false)) return bad(what);
  if (!n) return BLSGPU_OK;
  HostCall h(c);
  h.report_status();
  void* dx = h.in(c->io_a, xy, n * 64);
  void* ds = h.in(c->io_b, scalars, n * 32);
  void* dout = h.out(c->io_out, out_xyz, n * 96);
  if (h.rc) return h.rc;
  return fred_finish(h, blsgpu_fr_edwards_mul_batch_device(c, e, dx, ds, bits, n, dout));
}

// the table of n bases at d_xy (device memory), built and normalised on the device; synchronises (a setup call) and reads the flag back
static int fred_bases_build(blsgpu_ctx* c, const blsgpu_fr_edwards* e, const void* d_xy, const FredTablePlan& p, blsgpu_fr_edwards_bases** out) {
  HIPCHK(hipSetDevice(c->device));
  blsgpu_fr_edwards_bases* t = new blsgpu_fr_edwards_bases();
  t->device = c->device; t->bits = p.bits; t->window = p.window; t->W = p.W; t->H = p.H; t->n = p.n;
  for (int i = 0; i < 8; i++) { t->a[i] = e->a[i]; t->d[i] = e->d[i]; }
  auto build = [&]() -> int {
    HIPCHK(hipMalloc((void**)&t->table, p.bytes + 16));                   // the last 16 bytes: the flag of the build
    u32* flag = t->table + p.entries * FRED_ENTRY_WORDS;
    HIPCHK(hipMemsetAsync(flag, 0, 16, c->stream));
    const EdArgs k = fred_kargs(e->a, e->d);
    KLAUNCH(k_fred_table_build, dim3(p.build.grid), dim3(p.build.block), 0, c->stream, k, (const u32*)d_xy, p.n, p.window, p.W, p.H, t->table, flag);
    KLAUNCH(k_fred_normalize<true>, dim3(p.norm.grid), dim3(p.norm.block), p.norm.lds, c->stream, k, (const u32*)t->table, p.entries, t->table, (uint8_t*)nullptr);
    LAUNCHCHK();
    u32 bad_base = 0;
    HIPCHK(hipMemcpyAsync(&bad_base, flag, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (bad_base) return bad("fr_edwards_bases: a base is not a point of the curve (or has limbs >= r)");
    return BLSGPU_OK;
  };
  if (int rc = build()) { (void)hipStreamSynchronize(c->stream); if (t->table) hipFree(t->table); delete t; return rc; }
  *out = t;
  return BLSGPU_OK;
}
static int fred_bases_check(blsgpu_ctx* c, const blsgpu_fr_edwards* e, const void* xy, size_t n, int bits, int window, bool device, blsgpu_fr_edwards_bases** out, FredTablePlan* p) {
  if (out) *out = nullptr;
  if (int rc = fred_handle_check(c, e)) return rc;
  if (!out) return bad("fr_edwards_bases: NULL out");
  if (!xy) return bad("fr_edwards_bases: NULL xy");
  *p = fred_table_plan(n, bits, window);
  if (!p->ok) return bad(p->why);
  if (device && fred_misaligned(xy)) return bad("fr_edwards_bases_from_device: d_xy must be 16-byte aligned");
  return BLSGPU_OK;
}
extern "C" int blsgpu_fr_edwards_bases_from_device(blsgpu_ctx* c, const blsgpu_fr_edwards* e, const void* d_xy, size_t n, int bits, int window, blsgpu_fr_edwards_bases** out) { CTX_CLAIM(c);
  FredTablePlan p;
  if (int rc = fred_bases_check(c, e, d_xy, n, bits, window, true, out, &p)) return rc;
  return fred_bases_build(c, e, d_xy, p, out);
}
extern "C" int blsgpu_fr_edwards_bases_create(blsgpu_ctx* c, const blsgpu_fr_edwards* e, const uint64_t* xy, size_t n, int bits, int window, blsgpu_fr_edwards_bases** out) { CTX_CLAIM(c);
  FredTablePlan p;
  if (int rc = fred_bases_check(c, e, xy, n, bits, window, false, out, &p)) return rc;
  FredCurve cv;
  cv.a = fred_fe(e->a64); cv.d = fred_fe(e->d64);
  for (size_t i = 0; i < n; i++)
    if (!fred_on_curve(cv, xy + 8 * i)) {
      char buf[128];
      snprintf(buf, sizeof buf, "fr_edwards_bases_create: base %zu is not a point of the curve (or has limbs >= r)", i);
      g_err = buf;
      return BLSGPU_ERR_ARG;
    }
  HostCall h(c);
  void* dx = h.in(c->io_a, xy, n * 64);
  if (h.rc) return h.rc;
  return fred_bases_build(c, e, dx, p, out);
}
extern "C" size_t blsgpu_fr_edwards_bases_len(const blsgpu_fr_edwards_bases* t) { return t ? t->n : 0; }
extern "C" void blsgpu_fr_edwards_bases_free(blsgpu_fr_edwards_bases* t) {
  if (!t) return;
  handle_quiesce(t->device);               // an asynchronous MSM may still be reading the table
  if (t->table) hipFree(t->table);
  delete t;
}

static int fred_msm_check(blsgpu_ctx* c, const blsgpu_fr_edwards_bases* t, const void* base_first, const void* offsets, const void* scalars, size_t k, size_t total, const void* out,
                          bool device) {
  if (!c) return bad("fr_edwards_msm_segments: NULL context");
  if (!t) return bad("fr_edwards_msm_segments: NULL table");
  if (t->device != c->device) return bad("fr_edwards_msm_segments: the table lives on another device than the context");
  FredMsmArgs a;
  a.nbases = t->n; a.base_first = base_first; a.offsets = offsets; a.scalars = scalars; a.k = k; a.total = total; a.out = out; a.device = device;
  if (const char* what = fred_msm_args(a)) return bad(what);
  return BLSGPU_OK;
}
extern "C" int blsgpu_fr_edwards_msm_segments_device(blsgpu_ctx* c, const blsgpu_fr_edwards_bases* t, const void* d_base_first, const void* d_offsets, const void* d_scalars, size_t k,
                                                     size_t total, void* d_out_xyz) { CTX_CLAIM(c);
  if (int rc = fred_msm_check(c, t, d_base_first, d_offsets, d_scalars, k, total, d_out_xyz, true)) return rc;
  if (!k) return BLSGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  const FredMsmPlan p = fred_msm_plan(k, total);
  if (!p.ok) return bad("fr_edwards_msm_segments: no plan for these sizes");
  if (c->fred_off.reserve(p.off_bytes) || c->fred_part.reserve(p.part_bytes + 16) || c->fred_meta.reserve(p.meta_bytes + 16)) {
    g_err = "hipMalloc(fr edwards msm scratch) failed"; return BLSGPU_ERR_HIP;
  }
  hipStream_t st = c->stream;
  unsigned long long* off = c->fred_off.as<unsigned long long>();
  EdMsmArgs m;
  m.c = fred_kargs(t->a, t->d); m.table = t->table; m.nbases = (u32)t->n; m.bits = t->bits; m.window = t->window; m.W = t->W; m.H = t->H;
  KLAUNCH(k_fred_msm_prep, dim3(p.prep.grid), dim3(p.prep.block), 0, st, (const u32*)d_offsets, (const u32*)d_base_first, k, (u32)total, t->n, off, c->status_word);
  if (p.chunks.grid)
    KLAUNCH(k_fred_msm_chunks, dim3(p.chunks.grid), dim3(p.chunks.block), p.chunks.lds, st, m, (const u32*)d_base_first, (const u32*)d_scalars, (const unsigned long long*)off, (u32)k,
            (u32)total, p.cut.terms, (u32*)d_out_xyz, c->fred_part.as<u32>(), c->fred_meta.as<u32>(), c->status_word);
  KLAUNCH(k_fred_msm_combine, dim3(p.combine.grid), dim3(p.combine.block), p.combine.lds, st, m.c, (const unsigned long long*)off, (u32)k, (u32)total, p.cut.chunk, p.cut.nchunks,
          (const u32*)c->fred_part.as<u32>(), (const u32*)c->fred_meta.as<u32>(), (u32*)d_out_xyz);
  LAUNCHCHK();
  return BLSGPU_OK;
}
extern "C" int blsgpu_fr_edwards_msm_segments(blsgpu_ctx* c, const blsgpu_fr_edwards_bases* t, const uint32_t* base_first, const uint32_t* offsets, const uint8_t* scalars, size_t k,
                                              uint64_t* out_xyz) { CTX_CLAIM(c);
  if (int rc = fred_msm_check(c, t, base_first, offsets, nullptr, k, 0, out_xyz, false)) return rc;
  if (!k) return BLSGPU_OK;
  size_t total = 0;
  if (const char* what = fred_msm_args_host(offsets, base_first, k, t->n, &total)) return bad(what);
  if (int rc = fred_msm_check(c, t, base_first, offsets, scalars, k, total, out_xyz, false)) return rc;
  HostCall h(c);
  h.report_status();
  void* doff = h.in(c->io_a, offsets, (k + 1) * 4);
  void* dbf = h.in(c->io_b, base_first, k * 4);
  void* ds = total ? h.in(c->io_e, scalars, total * 32) : nullptr;
  void* dout = h.out(c->io_out, out_xyz, k * 96);
  if (h.rc) return h.rc;
  if (!ds) { if (!h.reserve(c->io_e, 16)) return h.rc; ds = c->io_e.p; }      // no term: nothing is read, but the device form wants a pointer
  return fred_finish(h, blsgpu_fr_edwards_msm_segments_device(c, t, dbf, doff, ds, k, total, dout));
}

// ---- expression programs: gate and quotient columns in one pass (fr_expr.hip.h; fr_expr_plan.h validates, builds the image and plans) ------
extern "C" int blsgpu_fr_expr_create(blsgpu_ctx* c, int n_cols, int n_regs, int n_consts, const uint64_t* consts, size_t n_instr, const uint32_t* code, blsgpu_fr_expr** out) { CTX_CLAIM(c);
  if (out) *out = nullptr;
  if (!c || !out) return bad("fr_expr: NULL context / out");
  FrxProg prog; FrxInfo info;
  if (const char* what = frx_prog_build(n_cols, n_regs, n_consts, consts, n_instr, code, &prog, &info)) return bad(what);
  HIPCHK(hipSetDevice(c->device));
  blsgpu_fr_expr* e = new blsgpu_fr_expr();
  e->device = c->device; e->info = info;
  const hipError_t err = device_image(&e->image, prog.w, sizeof(FrxProg));
  if (err != hipSuccess) { delete e; return fail("fr_expr: upload of the program image", err, __LINE__); }
  *out = e;
  return BLSGPU_OK;
}
extern "C" int blsgpu_fr_expr_cols(const blsgpu_fr_expr* e) { return e ? e->info.n_cols : 0; }
extern "C" int blsgpu_fr_expr_regs(const blsgpu_fr_expr* e) { return e ? e->info.n_regs : 0; }
extern "C" size_t blsgpu_fr_expr_instructions(const blsgpu_fr_expr* e) { return e ? e->info.n_instr : 0; }
extern "C" size_t blsgpu_fr_expr_products(const blsgpu_fr_expr* e) { return e ? e->info.products : 0; }
extern "C" uint32_t blsgpu_fr_expr_cols_read(const blsgpu_fr_expr* e) { return e ? e->info.cols_read : 0; }
extern "C" void blsgpu_fr_expr_free(blsgpu_fr_expr* e) {
  if (!e) return;
  handle_quiesce(e->device);               // an asynchronous evaluation may still be reading the image
  if (e->image) hipFree(e->image);
  delete e;
}
// every argument check of both forms, before anything is staged or launched; fills the kernel's column argument from the columns the
// program reads (the others stay NULL / 0: the kernel never looks at them)
static int fr_expr_check(blsgpu_ctx* c, const blsgpu_fr_expr* e, const void* const* cols, const uint8_t* col_log_len, int log_n, int log_stride, const void* out, bool device, FrxCols* k) {
  if (!c) return bad("fr_expr_eval: NULL context");
  if (!e) return bad("fr_expr_eval: NULL handle");
  if (e->device != c->device) return bad("fr_expr_eval: the handle lives on another device than the context");
  if (!cols || !out) return bad("fr_expr_eval: NULL cols / out");
  if (log_n < 0 || log_n > FRX_MAX_LOG_N) return bad("fr_expr_eval: log_n must be in [0, 28]");
  if (log_stride < 0 || log_stride > log_n) return bad("fr_expr_eval: log_stride must be in [0, log_n]");
  if (device && ((uintptr_t)out & 15)) return bad("fr_expr_eval: device pointers must be 16-byte aligned");
  for (int j = 0; j < FRX_MAX_COLS; j++) { k->p[j] = nullptr; k->log_len[j] = 0; }
  const size_t out_bytes = (size_t)32 << log_n;
  for (int j = 0; j < e->info.n_cols; j++) {
    if (!((e->info.cols_read >> j) & 1u)) continue;
    const int ll = col_log_len ? (int)col_log_len[j] : log_n;
    if (ll > log_n) return bad("fr_expr_eval: a column is longer than 2^log_n (col_log_len[j] must not exceed log_n)");
    if (!cols[j]) return bad("fr_expr_eval: NULL pointer of a column the program reads");
    if (device && ((uintptr_t)cols[j] & 15)) return bad("fr_expr_eval: device pointers must be 16-byte aligned");
    if (ranges_overlap(out, out_bytes, cols[j], (size_t)32 << ll)) return bad("fr_expr_eval: out overlaps a column the program reads (there is no in-place form)");
    k->p[j] = (const uint32_t*)cols[j]; k->log_len[j] = (uint32_t)ll;
  }
  return BLSGPU_OK;
}
static int fr_expr_launch(blsgpu_ctx* c, const blsgpu_fr_expr* e, const FrxCols& k, int log_n, int log_stride, void* d_out) {
  HIPCHK(hipSetDevice(c->device));
  const FrExprPlan plan = fr_expr_plan(log_n, e->info.n_regs);
  if (!plan.ok) return bad("fr_expr_eval: log_n is out of range");
  KLAUNCH(k_frx_eval, dim3(plan.grid), dim3(plan.block), plan.lds, c->stream, (const u32*)e->image, k, log_n, log_stride, plan.chunk, (u32*)d_out);
  LAUNCHCHK();
  return BLSGPU_OK;
}
extern "C" int blsgpu_fr_expr_eval_device(blsgpu_ctx* c, const blsgpu_fr_expr* e, const void* const* d_cols, const uint8_t* col_log_len, int log_n, int log_stride, void* d_out) { CTX_CLAIM(c);
  FrxCols k;
  if (int rc = fr_expr_check(c, e, d_cols, col_log_len, log_n, log_stride, d_out, true, &k)) return rc;
  return fr_expr_launch(c, e, k, log_n, log_stride, d_out);
}
// the columns the program reads are staged end to end in ONE buffer (each a multiple of 32 bytes, so every one stays 16-byte aligned); a
// host pointer passed for several columns of one length is staged once, so the device sees the alias too
extern "C" int blsgpu_fr_expr_eval(blsgpu_ctx* c, const blsgpu_fr_expr* e, const uint64_t* const* cols, const uint8_t* col_log_len, int log_n, int log_stride, uint64_t* out) { CTX_CLAIM(c);
  FrxCols k;
  if (int rc = fr_expr_check(c, e, (const void* const*)cols, col_log_len, log_n, log_stride, out, false, &k)) return rc;
  HostCall h(c);
  size_t off[FRX_MAX_COLS] = {}, total = 0;
  for (int j = 0; j < e->info.n_cols; j++) {
    if (!k.p[j]) continue;
    int same = -1;
    for (int i = 0; i < j && same < 0; i++) if (k.p[i] == k.p[j] && k.log_len[i] == k.log_len[j]) same = i;
    if (same >= 0) { off[j] = off[same]; continue; }
    off[j] = total; total += (size_t)32 << k.log_len[j];
  }
  if (!h.reserve(c->io_a, total)) return h.rc;
  size_t done = 0;
  for (int j = 0; j < e->info.n_cols && !h.rc; j++) {
    if (!k.p[j]) continue;
    if (off[j] == done) { h.rc = staged_upload(c, (char*)c->io_a.p + off[j], k.p[j], (size_t)32 << k.log_len[j]); done += (size_t)32 << k.log_len[j]; }
  }
  void* o = h.out(c->io_out, out, (size_t)32 << log_n);
  if (h.rc) return h.rc;
  for (int j = 0; j < e->info.n_cols; j++) if (k.p[j]) k.p[j] = (const uint32_t*)((const char*)c->io_a.p + off[j]);
  return h.finish(fr_expr_launch(c, e, k, log_n, log_stride, o));
}

// ---- lookup tables: logUp multiplicities and row indices in one call (fr_lookup.hip.h; fr_lookup_plan.h checks, sizes and plans) -----------
static void frl_release(blsgpu_fr_lookup* h) {
  if (h->keys) hipFree(h->keys);
  if (h->slot) hipFree(h->slot);
  if (h->counters) hipFree(h->counters);
  delete h;
}
// the handle of a table whose columns are in device memory: its own row-major copy of the keys, the slot array, the counters.  Ends
// with the stream synchronised (a setup call: `distinct` comes back, and the caller's buffer is free again).
static int frl_build(blsgpu_ctx* c, int cols, const void* d_t, size_t pitch, size_t rows, blsgpu_fr_lookup** out) {
  HIPCHK(hipSetDevice(c->device));
  const FrLookupPlan plan = fr_lookup_plan(rows, 0);
  if (!plan.ok) return bad("fr_lookup: rows must be in [1, 2^24]");
  blsgpu_fr_lookup* h = new blsgpu_fr_lookup();
  h->device = c->device; h->c = cols; h->rows = rows; h->slots = plan.slots;
  hipStream_t st = c->stream;
  u32 distinct = 0;
  hipError_t err = hipMalloc((void**)&h->keys, rows * (size_t)cols * 32);
  if (err == hipSuccess) err = hipMalloc((void**)&h->slot, plan.slots * 4);
  if (err == hipSuccess) err = hipMalloc((void**)&h->counters, rows * 4);
  if (err == hipSuccess) err = hipMemsetAsync(h->slot, 0, plan.slots * 4, st);
  if (err == hipSuccess) err = hipMemsetAsync(h->counters, 0, 4, st);        // counters[0] doubles as the `distinct` word of the build
  if (err == hipSuccess) {
    KLAUNCH(k_frl_build, dim3(plan.build_grid), dim3(plan.block), 0, st, (const u32*)d_t, pitch, (u32)rows, cols, h->keys, h->slot, (u32)(plan.slots - 1), h->counters);
    err = hipGetLastError();
  }
  if (err == hipSuccess) err = hipMemcpyAsync(&distinct, h->counters, 4, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err != hipSuccess) { frl_release(h); return fail("fr_lookup: building the table", err, __LINE__); }
  h->distinct = distinct;
  *out = h;
  return BLSGPU_OK;
}
extern "C" int blsgpu_fr_lookup_from_device(blsgpu_ctx* c, int cols, const void* d_t, size_t pitch, size_t rows, blsgpu_fr_lookup** out) { CTX_CLAIM(c);
  if (out) *out = nullptr;
  if (!c || !out) return bad("fr_lookup: NULL context / out");
  if (const char* what = frl_table_check(cols, d_t, pitch, rows, true)) return bad(what);
  return frl_build(c, cols, d_t, pitch, rows, out);
}
extern "C" int blsgpu_fr_lookup_create(blsgpu_ctx* c, int cols, const uint64_t* t, size_t rows, blsgpu_fr_lookup** out) { CTX_CLAIM(c);
  if (out) *out = nullptr;
  if (!c || !out) return bad("fr_lookup: NULL context / out");
  if (const char* what = frl_table_check(cols, t, rows, rows, false)) return bad(what);
  HostCall h(c);
  void* dt = h.in(c->io_a, t, (size_t)cols * rows * 32);
  if (h.rc) return h.rc;
  return frl_build(c, cols, dt, rows, rows, out);
}
extern "C" int blsgpu_fr_lookup_cols(const blsgpu_fr_lookup* h) { return h ? h->c : 0; }
extern "C" size_t blsgpu_fr_lookup_rows(const blsgpu_fr_lookup* h) { return h ? h->rows : 0; }
extern "C" size_t blsgpu_fr_lookup_distinct(const blsgpu_fr_lookup* h) { return h ? h->distinct : 0; }
extern "C" size_t blsgpu_fr_lookup_slots(const blsgpu_fr_lookup* h) { return h ? h->slots : 0; }
extern "C" void blsgpu_fr_lookup_free(blsgpu_fr_lookup* h) {
  if (!h) return;
  handle_quiesce(h->device);               // an asynchronous count may still be using the table
  frl_release(h);
}
// every argument check of both count forms, before anything is staged or launched
static int frl_count_check_all(blsgpu_ctx* c, const blsgpu_fr_lookup* h, const void* f, size_t pitch, size_t n, int negate, const void* mult, const void* index, const void* missing, bool device) {
  if (!c) return bad("fr_lookup_count: NULL context");
  if (!h) return bad("fr_lookup_count: NULL handle");
  if (h->device != c->device) return bad("fr_lookup_count: the handle lives on another device than the context");
  FrlCountArgs a;
  a.c = h->c; a.rows = h->rows; a.f = f; a.pitch = pitch; a.n = n; a.negate = negate; a.mult = mult; a.index = index; a.missing = missing; a.device = device;
  if (const char* what = frl_count_check(a)) return bad(what);
  return BLSGPU_OK;
}
static int frl_count_launch(blsgpu_ctx* c, const blsgpu_fr_lookup* h, const void* d_f, size_t pitch, size_t n, int negate, void* d_mult, void* d_index, void* d_missing) {
  HIPCHK(hipSetDevice(c->device));
  const FrLookupPlan plan = fr_lookup_plan(h->rows, n);
  if (!plan.ok) return bad("fr_lookup_count: a size is out of range");
  hipStream_t st = c->stream;
  if (d_missing) HIPCHK(hipMemsetAsync(d_missing, 0, 8, st));
  if (d_mult) HIPCHK(hipMemsetAsync(h->counters, 0, h->rows * 4, st));
  u32* counters = d_mult ? h->counters : nullptr;
  if (plan.count_grid && (d_mult || d_index || d_missing)) {
    const u32 mask = (u32)(h->slots - 1);
    if (plan.lds_path)
      KLAUNCH(k_frl_count<true>, dim3(plan.count_grid), dim3(plan.block), plan.count_lds, st, (const u32*)d_f, pitch, n, h->c, (const u32*)h->keys, (const u32*)h->slot, mask, (u32)h->rows,
              plan.iters, counters, (u32*)d_index, (unsigned long long*)d_missing);
    else
      KLAUNCH(k_frl_count<false>, dim3(plan.count_grid), dim3(plan.block), plan.count_lds, st, (const u32*)d_f, pitch, n, h->c, (const u32*)h->keys, (const u32*)h->slot, mask, (u32)h->rows,
              plan.iters, counters, (u32*)d_index, (unsigned long long*)d_missing);
  }
  if (d_mult) KLAUNCH(k_frl_finish, dim3(plan.finish_grid), dim3(plan.block), 0, st, (const u32*)h->counters, (u32)h->rows, negate, (u32*)d_mult);
  LAUNCHCHK();
  return BLSGPU_OK;
}
extern "C" int blsgpu_fr_lookup_count_device(blsgpu_ctx* c, const blsgpu_fr_lookup* h, const void* d_f, size_t pitch, size_t n, int negate, void* d_mult, void* d_index, void* d_missing) { CTX_CLAIM(c);
  if (int rc = frl_count_check_all(c, h, d_f, pitch, n, negate, d_mult, d_index, d_missing, true)) return rc;
  return frl_count_launch(c, h, d_f, pitch, n, negate, d_mult, d_index, d_missing);
}
extern "C" int blsgpu_fr_lookup_count(blsgpu_ctx* c, const blsgpu_fr_lookup* h, const uint64_t* f, size_t n, int negate, uint64_t* mult, uint32_t* index, uint64_t* missing) { CTX_CLAIM(c);
  if (int rc = frl_count_check_all(c, h, f, n, n, negate, mult, index, missing, false)) return rc;
  HostCall hc(c);
  void* df = hc.in(c->io_a, f, (size_t)h->c * n * 32);
  void* dm = mult ? hc.out(c->io_out, mult, h->rows * 32) : nullptr;
  void* di = index ? hc.out(c->io_b, index, n * 4) : nullptr;
  void* ds = missing ? hc.out(c->flags_a, missing, 8) : nullptr;
  if (hc.rc) return hc.rc;
  return hc.finish(frl_count_launch(c, h, df, n, n, negate, dm, di, ds));
}

// ---- multilinear tables: folds, eq tables, evaluation, sumcheck rounds (fr_mle.hip.h; fr_mle_plan.h decides the launches) -----------------
// the footprint (k - 1) * pitch + len scalars of k tables; false when it does not fit 2^28 (64-bit overflow included)
static bool frmle_footprint(size_t k, size_t pitch, size_t len, size_t* scalars) {
  *scalars = 0;
  if (!k) return true;
  if (k > FRM_MAX_TOTAL || pitch > FRM_MAX_TOTAL || len > FRM_MAX_TOTAL) return false;
  const size_t f = (k - 1) * pitch + len;           // both factors <= 2^28: no overflow
  *scalars = f;
  return f <= FRM_MAX_TOTAL;
}
// walks a plan: in / out are the caller's buffers with the caller's pitches, r the call's own challenge, point the challenges of an eval
static int frmle_launch(blsgpu_ctx* c, const FrMlePlan& plan, const u32* in, size_t pitch_in, u32* out, size_t pitch_out, const u32* r, const u32* point, size_t k,
                        const FrmProg* prog) {
  hipStream_t st = c->stream;
  const FrMleShape shape;
  u32* buf[4] = {const_cast<u32*>(in), out, c->frm_scratch.as<u32>(), c->frm_rec.as<u32>()};
  for (int i = 0; i < plan.n_steps; i++) {
    const FrMleStep& s = plan.step[i];
    u32* src = s.src >= 0 ? buf[s.src] : nullptr;
    u32* dst = s.dst >= 0 ? buf[s.dst] : nullptr;
    const size_t pi = s.pitch_in ? s.pitch_in : pitch_in, po = s.pitch_out ? s.pitch_out : pitch_out;
    switch (s.kernel) {
      case FRM_K_FOLD:
        KLAUNCH(k_frm_fold, dim3(s.grid), dim3(s.block), s.lds, st, (const u32*)src, pi, dst, po, s.m - 1, s.items, s.var >= 0 ? point + (size_t)s.var * 8 : r);
        break;
      case FRM_K_EQ:
        KLAUNCH(k_frm_eq, dim3(s.grid), dim3(s.block), s.lds, st, point, s.m, frm_eq_lo(s.m, shape), dst);
        break;
      case FRM_K_COPY:
        HIPCHK(hipMemcpy2DAsync(dst, po * 32, src, pi * 32, 32, s.items, hipMemcpyDeviceToDevice, st));
        break;
      case FRM_K_ROUND:
        KLAUNCH(k_frm_round<false>, dim3(s.grid), dim3(s.block), s.lds, st, src, pi, s.items, (unsigned)k, (unsigned)shape.chunk, *prog, (const u32*)nullptr, dst);
        break;
      case FRM_K_ROUND_FUSED:
        KLAUNCH(k_frm_round<true>, dim3(s.grid), dim3(s.block), s.lds, st, src, pi, s.items, (unsigned)k, (unsigned)shape.chunk, *prog, r, dst);
        break;
      default:
        KLAUNCH(k_frm_round_finish, dim3(s.grid), dim3(s.block), s.lds, st, (const u32*)src, s.items, prog->deg + 1, dst);
        break;
    }
  }
  LAUNCHCHK();
  return BLSGPU_OK;
}
// every argument check of both fold forms, before anything is staged, reserved or launched.  *work: there is something to do.
static int fr_mle_fold_check(blsgpu_ctx* c, const void* in, size_t pitch_in, int m, size_t k, const void* r, const void* out, size_t pitch_out, bool device, bool* work) {
  *work = false;
  if (!c) return bad("fr_mle_fold: NULL context");
  if (m < 1 || m > FRM_MAX_M) return bad("fr_mle_fold: m must be in [1, 28]");
  const size_t n = (size_t)1 << m, h = n >> 1;
  if (pitch_in < n || pitch_out < h) return bad("fr_mle_fold: a pitch is smaller than its table (pitch_in >= 2^m, pitch_out >= 2^(m-1))");
  size_t fin, fout;
  if (!frmle_footprint(k, pitch_in, n, &fin) || !frmle_footprint(k, pitch_out, h, &fout)) return bad("fr_mle_fold: (k - 1) * pitch + 2^m must not exceed 2^28");
  if (!k) return BLSGPU_OK;
  if (!in || !out || !r) return bad("fr_mle_fold: NULL tables / r / out with work to do");
  if (device && (((uintptr_t)in | (uintptr_t)out | (uintptr_t)r) & 15)) return bad("fr_mle_fold_device: device pointers must be 16-byte aligned");
  if (!(in == out && pitch_in == pitch_out) && ranges_overlap(in, fin * 32, out, fout * 32))
    return bad("fr_mle_fold: in and out overlap (d_out == d_in with equal pitches is the in-place form)");
  if (device && ranges_overlap(r, 32, out, fout * 32)) return bad("fr_mle_fold: the challenge lies inside the output");
  *work = true;
  return BLSGPU_OK;
}
extern "C" int blsgpu_fr_mle_fold_device(blsgpu_ctx* c, const void* d_in, size_t pitch_in, int m, size_t k, const void* d_r, void* d_out, size_t pitch_out) { CTX_CLAIM(c);
  bool work;
  if (int rc = fr_mle_fold_check(c, d_in, pitch_in, m, k, d_r, d_out, pitch_out, true, &work)) return rc;
  if (!work) return BLSGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  return frmle_launch(c, fr_mle_fold_plan(m, k), (const u32*)d_in, pitch_in, (u32*)d_out, pitch_out, (const u32*)d_r, nullptr, k, nullptr);
}
extern "C" int blsgpu_fr_mle_fold(blsgpu_ctx* c, const uint64_t* tables, int m, size_t k, const uint64_t* r, uint64_t* out) { CTX_CLAIM(c);
  bool work;
  const size_t n = m >= 1 && m <= FRM_MAX_M ? (size_t)1 << m : 2;
  if (int rc = fr_mle_fold_check(c, tables, n, m, k, r, out, n / 2, false, &work)) return rc;
  if (!work) return BLSGPU_OK;
  HostCall h(c);
  void* di = h.in(c->io_a, tables, k * n * 32);
  void* dr = h.in(c->io_b, r, 32);
  void* o = h.out(c->io_out, out, k * (n / 2) * 32);
  if (h.rc) return h.rc;
  return h.finish(blsgpu_fr_mle_fold_device(c, di, n, m, k, dr, o, n / 2));
}
static int fr_eq_table_check(blsgpu_ctx* c, const void* point, int m, const void* out, bool device) {
  if (!c) return bad("fr_eq_table: NULL context");
  if (m < 0 || m > FRM_MAX_M) return bad("fr_eq_table: m must be in [0, 28]");
  if (!out || (m && !point)) return bad("fr_eq_table: NULL point / out");
  if (device && (((uintptr_t)point | (uintptr_t)out) & 15)) return bad("fr_eq_table_device: device pointers must be 16-byte aligned");
  if (device && m && ranges_overlap(point, (size_t)m * 32, out, (size_t)32 << m)) return bad("fr_eq_table: the point lies inside the output");
  return BLSGPU_OK;
}
extern "C" int blsgpu_fr_eq_table_device(blsgpu_ctx* c, const void* d_point, int m, void* d_out) { CTX_CLAIM(c);
  if (int rc = fr_eq_table_check(c, d_point, m, d_out, true)) return rc;
  HIPCHK(hipSetDevice(c->device));
  return frmle_launch(c, fr_eq_table_plan(m), nullptr, 0, (u32*)d_out, 0, nullptr, (const u32*)d_point, 1, nullptr);
}
extern "C" int blsgpu_fr_eq_table(blsgpu_ctx* c, const uint64_t* point, int m, uint64_t* out) { CTX_CLAIM(c);
  if (int rc = fr_eq_table_check(c, point, m, out, false)) return rc;
  HostCall h(c);
  void* dp = h.in(c->io_a, m ? point : nullptr, (size_t)m * 32);
  void* o = h.out(c->io_out, out, ((size_t)1 << m) * 32);
  if (h.rc) return h.rc;
  return h.finish(blsgpu_fr_eq_table_device(c, dp, m, o));
}
static int fr_mle_eval_check(blsgpu_ctx* c, const void* tables, size_t pitch, int m, size_t k, const void* point, const void* out, bool device, bool* work) {
  *work = false;
  if (!c) return bad("fr_mle_eval: NULL context");
  if (m < 0 || m > FRM_MAX_M) return bad("fr_mle_eval: m must be in [0, 28]");
  const size_t n = (size_t)1 << m;
  if (pitch < n) return bad("fr_mle_eval: pitch is smaller than a table (pitch >= 2^m)");
  size_t foot;
  if (!frmle_footprint(k, pitch, n, &foot)) return bad("fr_mle_eval: (k - 1) * pitch + 2^m must not exceed 2^28");
  if (!k) return BLSGPU_OK;
  if (!tables || !out || (m && !point)) return bad("fr_mle_eval: NULL tables / point / out with work to do");
  if (device && (((uintptr_t)tables | (uintptr_t)out | (uintptr_t)point) & 15)) return bad("fr_mle_eval_device: device pointers must be 16-byte aligned");
  if (device && ranges_overlap(tables, foot * 32, out, k * 32)) return bad("fr_mle_eval: out overlaps the tables (they are not written)");
  if (device && m && ranges_overlap(point, (size_t)m * 32, out, k * 32)) return bad("fr_mle_eval: out overlaps the point");
  *work = true;
  return BLSGPU_OK;
}
extern "C" int blsgpu_fr_mle_eval_device(blsgpu_ctx* c, const void* d_tables, size_t pitch, int m, size_t k, const void* d_point, void* d_out) { CTX_CLAIM(c);
  bool work;
  if (int rc = fr_mle_eval_check(c, d_tables, pitch, m, k, d_point, d_out, true, &work)) return rc;
  if (!work) return BLSGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  const FrMlePlan plan = fr_mle_eval_plan(m, k);
  if (c->frm_scratch.reserve(plan.scratch * 32)) { g_err = "hipMalloc(fr mle scratch) failed"; return BLSGPU_ERR_HIP; }
  return frmle_launch(c, plan, (const u32*)d_tables, pitch, (u32*)d_out, 1, nullptr, (const u32*)d_point, k, nullptr);
}
extern "C" int blsgpu_fr_mle_eval(blsgpu_ctx* c, const uint64_t* tables, int m, size_t k, const uint64_t* point, uint64_t* out) { CTX_CLAIM(c);
  bool work;
  const size_t n = m >= 0 && m <= FRM_MAX_M ? (size_t)1 << m : 1;
  if (int rc = fr_mle_eval_check(c, tables, n, m, k, point, out, false, &work)) return rc;
  if (!work) return BLSGPU_OK;
  HostCall h(c);
  void* dt = h.in(c->io_a, tables, k * n * 32);
  void* dp = h.in(c->io_b, m ? point : nullptr, (size_t)m * 32);
  void* o = h.out(c->io_out, out, k * 32);
  if (h.rc) return h.rc;
  return h.finish(blsgpu_fr_mle_eval_device(c, dt, n, m, k, dp, o));
}
// every argument check of a round, before anything is reserved or launched; *prog: the kernels' form of the program
static int fr_sumcheck_round_check(blsgpu_ctx* c, const void* tables, size_t pitch, int m, size_t k, size_t n_terms, const uint32_t* term_ptr, const uint8_t* term_tab,
                                   const uint64_t* coef, const void* r_prev, const void* evals, FrmProg* prog) {
  if (!c) return bad("fr_sumcheck_round: NULL context");
  if (const char* why = frm_prog_build(k, n_terms, term_ptr, term_tab, coef, prog)) return bad(why);
  if (m > FRM_MAX_M || m < (r_prev ? 2 : 1)) return bad(r_prev ? "fr_sumcheck_round: m must be in [2, 28] when a challenge is folded in first" : "fr_sumcheck_round: m must be in [1, 28]");
  const size_t n = (size_t)1 << m;
  if (pitch < n) return bad("fr_sumcheck_round: pitch is smaller than a table (pitch >= 2^m)");
  size_t foot;
  if (!frmle_footprint(k, pitch, n, &foot)) return bad("fr_sumcheck_round: (k - 1) * pitch + 2^m must not exceed 2^28");
  if (!tables || !evals) return bad("fr_sumcheck_round: NULL tables / evals");
  if (((uintptr_t)tables | (uintptr_t)evals | (uintptr_t)r_prev) & 15) return bad("fr_sumcheck_round_device: device pointers must be 16-byte aligned");
  const size_t eval_bytes = (size_t)(prog->deg + 1) * 32;
  if (ranges_overlap(tables, foot * 32, evals, eval_bytes)) return bad("fr_sumcheck_round: evals overlaps the tables");
  if (r_prev && ranges_overlap(tables, foot * 32, r_prev, 32)) return bad("fr_sumcheck_round: the challenge lies inside the tables, which the fold writes");
  if (r_prev && ranges_overlap(evals, eval_bytes, r_prev, 32)) return bad("fr_sumcheck_round: the challenge lies inside evals");
  return BLSGPU_OK;
}
extern "C" int blsgpu_fr_sumcheck_round_device(blsgpu_ctx* c, void* d_tables, size_t pitch, int m, size_t k, size_t n_terms, const uint32_t* term_ptr, const uint8_t* term_tab,
                                               const uint64_t* coef, const void* d_r_prev, void* d_evals) { CTX_CLAIM(c);
  FrmProg prog;
  if (int rc = fr_sumcheck_round_check(c, d_tables, pitch, m, k, n_terms, term_ptr, term_tab, coef, d_r_prev, d_evals, &prog)) return rc;
  HIPCHK(hipSetDevice(c->device));
  if (int rc = lds_grant(&c->frm_lds_ready, frm_round_lds_bytes(FrMleShape(), FRM_MAX_K), {(const void*)k_frm_round<false>, (const void*)k_frm_round<true>})) return rc;
  const FrMlePlan plan = fr_sumcheck_round_plan(m, k, (int)prog.deg, d_r_prev != nullptr);
  if (plan.n_steps < 0) return bad("fr_sumcheck_round: the shape is out of range");
  if (c->frm_rec.reserve(plan.recs * (prog.deg + 1) * 32)) { g_err = "hipMalloc(fr sumcheck records) failed"; return BLSGPU_ERR_HIP; }
  return frmle_launch(c, plan, (const u32*)d_tables, pitch, (u32*)d_evals, 0, (const u32*)d_r_prev, nullptr, k, &prog);
}

// the handle: its own copy of the tables (the rounds consume them), the program validated once
static void frsc_drop(blsgpu_fr_sumcheck* s) {
  if (!s) return;
  if (s->tables) hipFree(s->tables);
  if (s->small) hipFree(s->small);
  delete s;
}
static int frsc_check(blsgpu_ctx* c, const void* tables, size_t pitch, int m, size_t k, size_t n_terms, const uint32_t* term_ptr, const uint8_t* term_tab, const uint64_t* coef,
                      blsgpu_fr_sumcheck** out, bool device, FrmProg* prog) {
  if (out) *out = nullptr;
  if (!c || !out) return bad("fr_sumcheck_begin: NULL context / out");
  if (const char* why = frm_prog_build(k, n_terms, term_ptr, term_tab, coef, prog)) return bad(why);
  if (m < 1 || m > FRM_MAX_M) return bad("fr_sumcheck_begin: m must be in [1, 28]");
  const size_t n = (size_t)1 << m;
  if (pitch < n) return bad("fr_sumcheck_begin: pitch is smaller than a table (pitch >= 2^m)");
  size_t foot;
  if (!frmle_footprint(k, pitch, n, &foot) || k * n > FRM_MAX_TOTAL) return bad("fr_sumcheck_begin: (k - 1) * pitch + 2^m and k * 2^m must not exceed 2^28");
  if (!tables) return bad("fr_sumcheck_begin: NULL tables");
  if (device && ((uintptr_t)tables & 15)) return bad("fr_sumcheck_begin_device: device pointers must be 16-byte aligned");
  return BLSGPU_OK;
}
static int frsc_make(blsgpu_ctx* c, int m, size_t k, size_t n_terms, const uint32_t* term_ptr, const uint8_t* term_tab, const uint64_t* coef, const FrmProg& prog,
                     blsgpu_fr_sumcheck** out) {
  blsgpu_fr_sumcheck* s = new blsgpu_fr_sumcheck();
  s->device = c->device; s->m = m; s->k = k; s->pitch = (size_t)1 << m; s->vars_left = m; s->deg = (int)prog.deg; s->n_terms = n_terms;
  memcpy(s->term_ptr, term_ptr, (n_terms + 1) * 4);
  memcpy(s->term_tab, term_tab, term_ptr[n_terms]);
  memcpy(s->coef, coef, n_terms * 32);
  if (hipMalloc((void**)&s->tables, k * s->pitch * 32) != hipSuccess || hipMalloc((void**)&s->small, (1 + FRM_MAX_EVALS) * 32) != hipSuccess) {
    (void)hipGetLastError(); frsc_drop(s); g_err = "hipMalloc(fr sumcheck tables) failed"; return BLSGPU_ERR_HIP;
  }
  *out = s;
  return BLSGPU_OK;
}
extern "C" int blsgpu_fr_sumcheck_begin(blsgpu_ctx* c, const uint64_t* tables, int m, size_t k, size_t n_terms, const uint32_t* term_ptr, const uint8_t* term_tab,
                                        const uint64_t* coef, blsgpu_fr_sumcheck** out) { CTX_CLAIM(c);
  FrmProg prog;
  if (int rc = frsc_check(c, tables, m >= 1 && m <= FRM_MAX_M ? (size_t)1 << m : 0, m, k, n_terms, term_ptr, term_tab, coef, out, false, &prog)) return rc;
  HIPCHK(hipSetDevice(c->device));
  blsgpu_fr_sumcheck* s = nullptr;
  if (int rc = frsc_make(c, m, k, n_terms, term_ptr, term_tab, coef, prog, &s)) return rc;
  int rc = staged_upload(c, s->tables, tables, k * s->pitch * 32);
  if (rc) { (void)hipStreamSynchronize(c->stream); frsc_drop(s); return rc; }
  *out = s;
  return BLSGPU_OK;
}
extern "C" int blsgpu_fr_sumcheck_begin_device(blsgpu_ctx* c, const void* d_tables, size_t pitch, int m, size_t k, size_t n_terms, const uint32_t* term_ptr,
                                               const uint8_t* term_tab, const uint64_t* coef, blsgpu_fr_sumcheck** out) { CTX_CLAIM(c);
  FrmProg prog;
  if (int rc = frsc_check(c, d_tables, pitch, m, k, n_terms, term_ptr, term_tab, coef, out, true, &prog)) return rc;
  HIPCHK(hipSetDevice(c->device));
  blsgpu_fr_sumcheck* s = nullptr;
  if (int rc = frsc_make(c, m, k, n_terms, term_ptr, term_tab, coef, prog, &s)) return rc;
  hipError_t e = hipMemcpy2DAsync(s->tables, s->pitch * 32, d_tables, pitch * 32, s->pitch * 32, k, hipMemcpyDeviceToDevice, c->stream);
  if (e != hipSuccess) { frsc_drop(s); return fail("hipMemcpy2DAsync(fr sumcheck tables)", e, __LINE__); }
  *out = s;
  return BLSGPU_OK;
}
extern "C" int blsgpu_fr_sumcheck_vars_left(const blsgpu_fr_sumcheck* s) { return s ? s->vars_left : 0; }
extern "C" int blsgpu_fr_sumcheck_degree(const blsgpu_fr_sumcheck* s) { return s ? s->deg : 0; }
extern "C" int blsgpu_fr_sumcheck_round(blsgpu_ctx* c, blsgpu_fr_sumcheck* s, const uint64_t* r_prev, uint64_t* evals) { CTX_CLAIM(c);
  if (!c || !s || !evals) return bad("fr_sumcheck_round: NULL context / handle / evals");
  if (s->device != c->device) return bad("fr_sumcheck_round: the handle lives on another device than the context");
  if (!s->vars_left) return bad("fr_sumcheck_round: the sumcheck is finished");
  if (!s->started && r_prev) return bad("fr_sumcheck_round: the first round takes no challenge (r_prev must be NULL)");
  if (s->started && !r_prev) return bad("fr_sumcheck_round: every round after the first needs the previous round's challenge");
  if (s->started && s->vars_left == 1) return bad("fr_sumcheck_round: one variable is left: blsgpu_fr_sumcheck_finish takes the last challenge");
  HIPCHK(hipSetDevice(c->device));
  if (r_prev) HIPCHK(hipMemcpyAsync(s->small, r_prev, 32, hipMemcpyHostToDevice, c->stream));
  if (int rc = blsgpu_fr_sumcheck_round_device(c, s->tables, s->pitch, s->vars_left, s->k, s->n_terms, s->term_ptr, s->term_tab, s->coef, r_prev ? s->small : nullptr, s->small + 8))
    return rc;
  HIPCHK(hipMemcpyAsync(evals, s->small + 8, (size_t)(s->deg + 1) * 32, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (r_prev) s->vars_left--;
  s->started = true;
  return BLSGPU_OK;
}
extern "C" int blsgpu_fr_sumcheck_finish(blsgpu_ctx* c, blsgpu_fr_sumcheck* s, const uint64_t* r_last, uint64_t* values) { CTX_CLAIM(c);
  if (!c || !s || !r_last || !values) return bad("fr_sumcheck_finish: NULL context / handle / r_last / values");
  if (s->device != c->device) return bad("fr_sumcheck_finish: the handle lives on another device than the context");
  if (!s->started || s->vars_left != 1) return bad("fr_sumcheck_finish: rounds are left (finish takes the LAST challenge, when one variable is left)");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(s->small, r_last, 32, hipMemcpyHostToDevice, c->stream));
  if (int rc = blsgpu_fr_mle_fold_device(c, s->tables, s->pitch, 1, s->k, s->small, s->tables, s->pitch)) return rc;
  HIPCHK(hipMemcpy2DAsync(values, 32, s->tables, s->pitch * 32, 32, s->k, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  s->vars_left = 0;
  return BLSGPU_OK;
}
extern "C" void blsgpu_fr_sumcheck_free(blsgpu_fr_sumcheck* s) {
  if (!s) return;
  handle_quiesce(s->device);               // work queued on a stream may still use the tables
  frsc_drop(s);
}

// ---- KZG cell recovery (kzg_recover.hip.h; kzg_recover_plan.h holds the mathematics, the checks, the maps, the scratch layout and the launch shapes) ------
static KzgrArgs kzgr_args(const void* col, const void* offsets, size_t count, size_t m, const void* cells, int log_n, int log_l, int order, const void* polys, const void* out_cells,
                          const void* ok, bool device) {
  KzgrArgs a;
  a.col = col; a.offsets = offsets; a.count = count; a.m = m; a.cells = cells; a.log_n = log_n; a.log_l = log_l; a.order = order;
  a.polys = polys; a.out_cells = out_cells; a.ok = ok; a.device = device;
  return a;
}
static int kzg_recover_device(blsgpu_ctx* c, const void* d_col, const void* d_offsets, size_t count, size_t m, const void* d_cells, int log_n, int log_l, int order, void* d_polys,
                              void* d_out_cells, void* d_ok) {
  if (!c) return bad("kzg_recover: ctx is NULL");
  if (const char* why = kzgr_check(kzgr_args(d_col, d_offsets, count, m, d_cells, log_n, log_l, order, d_polys, d_out_cells, d_ok, true))) return bad(why);
  if (!count) return BLSGPU_OK;
  const KzgrPlan p = kzgr_plan(log_n, log_l, count, m, d_polys == nullptr);
  if (!p.ok) return bad("kzg_recover: the plan refuses the shape");
  HIPCHK(hipSetDevice(c->device));
  if (c->kzgr.reserve(p.bytes) || c->kzgr_roots.reserve(p.roots_bytes)) { g_err = "hipMalloc(kzg_recover scratch) failed"; return BLSGPU_ERR_HIP; }
  hipStream_t st = c->stream;
  uint8_t* base = c->kzgr.as<uint8_t>();
  u32* eff = (u32*)(base + p.eff); uint8_t* mis = base + p.mis;
  int* slot = (int*)(base + p.slot);
  u32 *status = (u32*)(base + p.status), *upper = (u32*)(base + p.upper);
  u32 *zd = (u32*)(base + p.zd), *zc = (u32*)(base + p.zc), *work = (u32*)(base + p.work);
  u32 *rootd = (u32*)(c->kzgr_roots.as<uint8_t>() + p.rootd), *rootc = (u32*)(c->kzgr_roots.as<uint8_t>() + p.rootc);
  uint4* coef = d_polys ? (uint4*)d_polys : (uint4*)(base + p.coef);
  KLAUNCH(k_kzg_rec_offsets, dim3(p.offsets_grid), dim3(KZGR_BLOCK), 0, st, (const u32*)d_offsets, (u32)count, (u32)m, eff, mis);
  KLAUNCH(k_kzg_rec_slots, dim3(p.slots_grid), dim3(KZGR_BLOCK), 0, st, (const u32*)eff, (const uint8_t*)mis, (const u32*)d_col, p.log_c, slot, status, upper, c->status_word);
  if (c->kzgr_roots_log_c != p.log_c || c->kzgr_roots_log_l != log_l) {      // the tables of another shape (cached as the transform caches its coset tables)
    FrArg g;
    for (int i = 0; i < 8; i++) g.w[i] = (u32)(KZGR_GEN_MONT[i >> 1] >> (32 * (i & 1)));
    KLAUNCH(k_kzg_rec_roots, dim3(p.roots_grid), dim3(KZGR_BLOCK), 0, st, rootd, rootc, g, p.log_c, log_l);
    LAUNCHCHK();
    c->kzgr_roots_log_c = p.log_c; c->kzgr_roots_log_l = log_l;
    HIPCHK(hipEventRecord(c->ev_kzgr_roots, st));
  }
  HIPCHK(hipStreamWaitEvent(st, c->ev_kzgr_roots, 0));
  KLAUNCH(k_kzg_rec_vanish, dim3(p.vanish_grid), dim3(KZGR_BLOCK), 0, st, (const int*)slot, (const u32*)status, (const u32*)rootd, (const u32*)rootc, p.log_c, order, p.vanish_per_poly,
          KZGR_ROOT_TILE, zd, zc);
  LAUNCHCHK();
  if (int rc = blsgpu_fr_batch_invert_device(c, zc, p.tables, zc, nullptr)) return rc;
  KLAUNCH(k_kzg_rec_scatter<KZGR_TILE>, dim3(p.scatter_grid), dim3(p.scatter_block), 0, st, (const int*)slot, (const uint4*)d_cells, (const u32*)zd, count, p.log_c, log_l, order,
          (uint4*)work);
  LAUNCHCHK();
  if (int rc = blsgpu_fr_ntt_many_device(c, work, log_n + 1, count, 1, nullptr)) return rc;
  if (int rc = blsgpu_fr_ntt_many_device(c, work, log_n + 1, count, 0, KZGR_GEN_MONT)) return rc;
  KLAUNCH(k_kzg_rec_scale, dim3(p.scale_grid), dim3(KZGR_BLOCK), 0, st, work, (const u32*)zc, (size_t)p.scalars, log_n, p.log_c);
  LAUNCHCHK();
  if (int rc = blsgpu_fr_ntt_many_device(c, work, log_n + 1, count, 1, KZGR_GEN_MONT)) return rc;
  KLAUNCH(k_kzg_rec_check, dim3(p.finish_grid), dim3(KZGR_BLOCK), 0, st, (const u32*)work, log_n, p.finish_per_poly, upper);
  KLAUNCH(k_kzg_rec_finish, dim3(p.finish_grid), dim3(KZGR_BLOCK), 0, st, (const uint4*)work, (const u32*)status, (const u32*)upper, log_n, p.finish_per_poly, coef, (uint8_t*)d_ok);
  LAUNCHCHK();
  // the coefficients of a failed polynomial are zero by now, so its cells are too
  if (d_out_cells) return blsgpu_kzg_cells_device(c, coef, log_n, log_l, count, KZG_FORM_COEFFS, order, d_out_cells);
  return BLSGPU_OK;
}
extern "C" int blsgpu_kzg_recover_device(blsgpu_ctx* c, const void* col, const void* offsets, size_t count, size_t m, const void* cells, int log_n, int log_l, int order, void* polys,
                                         void* out_cells, void* ok) { CTX_CLAIM(c);
  return kzg_recover_device(c, col, offsets, count, m, cells, log_n, log_l, order, polys, out_cells, ok); }
extern "C" int blsgpu_kzg_recover(blsgpu_ctx* c, const uint32_t* col, const uint32_t* offsets, size_t count, const uint64_t* cells, int log_n, int log_l, int order, uint64_t* polys,
                                  uint64_t* out_cells, uint8_t* ok) { CTX_CLAIM(c);
  if (!c) return bad("kzg_recover: ctx is NULL");
  if (count > ((size_t)1 << KZGR_MAX_LOG_TOTAL)) return bad("kzg_recover: count * 2n must not exceed 2^28");
  if (count && !offsets) return bad("kzg_recover: NULL offsets or ok with polynomials to recover");
  const size_t m = count ? offsets[count] : 0;
  if (const char* why = kzgr_check(kzgr_args(col, offsets, count, m, cells, log_n, log_l, order, polys, out_cells, ok, false))) return bad(why);
  if (const char* why = kzgr_check_host(offsets, count, col, log_n, log_l)) return bad(why);
  if (!count) return BLSGPU_OK;
  HostCall h(c);
  // the two u32 arrays share one staging buffer (each piece at a 256-byte boundary)
  const size_t o_off = (m * 4 + 255) / 256 * 256, words = o_off + (count + 1) * 4;
  void* dcells = h.in(c->io_a, cells, (m << log_l) * 32);
  uint8_t* wf = nullptr;
  if (h.reserve(c->io_f, words)) {
    wf = c->io_f.as<uint8_t>();
    if (!h.rc && m) h.rc = staged_upload(c, wf, col, m * 4);
    if (!h.rc) h.rc = staged_upload(c, wf + o_off, offsets, (count + 1) * 4);
  }
  void* dp = polys ? h.out(c->io_out, polys, (count << log_n) * 32) : nullptr;
  void* dc = out_cells ? h.out(c->io_b, out_cells, (count << log_n) * 64) : nullptr;
  void* dk = h.out(c->flags_b, ok, count);
  if (h.rc) return h.rc;
  return h.finish(kzg_recover_device(c, wf, wf + o_off, count, m, dcells, log_n, log_l, order, dp, dc, dk));
}
