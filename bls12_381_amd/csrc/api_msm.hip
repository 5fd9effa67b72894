// api_msm.hip -- resident bases, multi-scalar multiplication, batched variable-base multiplication, sums and batch_normalize.
#define BLS_TU_NAME "api_msm.hip"
#include "host.h"
#include "abi_kernels.hip.h"
#include "mulbatch.hip.h"
#include "msm_seg.hip.h"
#include "msm_plan.h"
#include "gntt.hip.h"
#include "gsum.hip.h"
#include "lagrange_combine.hip.h"
#include "kzg.hip.h"
#include "kzg_verify.hip.h"

// ---------------------------------------------------------------------------------------------------
// bases
// ---------------------------------------------------------------------------------------------------
// G1 bases also keep their images under the GLV endomorphism next to them (2x the resident memory; see k_glv_decompose);
// G2 bases keep P, psi(P), psi^2(P), psi^3(P) interleaved in a second array (5x the resident memory; see k_gls_decompose)
static void bases_drop(blsgpu_bases* b) {        // error paths of the constructors: nothing queued can still matter
  if (b->rec) hipFree(b->rec);
  if (b->endo) hipFree(b->endo);
  if (b->table) hipFree(b->table);
  if (b->ev_ready) hipEventDestroy(b->ev_ready);
  delete b;
}
static int bases_make_endo(blsgpu_ctx* c, blsgpu_bases* b, bool trusted) {
  if (!b->n) { b->subgroup = 1; return BLSGPU_OK; }
  // G2 sets with 4 n beyond the sort's 24-bit indices never take the split: no images, plain windows (exact for any curve
  // point), so there is nothing to test either
  if (b->group == 2 && b->n > ((size_t)1 << 22)) { b->subgroup = trusted ? 1 : (c->assume_subgroup ? 2 : 3); return BLSGPU_OK; }
  if (trusted) b->subgroup = 1;
  else if (c->assume_subgroup) b->subgroup = 2;
  else {
    // one pass of the reference's own subgroup test over the set (G1 ~2 k, G2 ~6 k field multiplications per point, once per
    // upload): the result decides on the host whether images are built, so this synchronises the context's stream
    u32 nbad = 0;
    HIPCHK(hipMemsetAsync(c->d_status + 1, 0, 4, c->stream));
    if (b->group == 1) KLAUNCH(k_bases_subgroup_check<FpPolicy>, dim3(nblk(b->n, 128)), dim3(128), 0, c->stream, b->rec, b->n, c->d_status + 1);
    else KLAUNCH(k_bases_subgroup_check<Fp2Policy>, dim3(nblk(b->n, 128)), dim3(128), 0, c->stream, b->rec, b->n, c->d_status + 1);
    LAUNCHCHK();
    HIPCHK(hipMemcpyAsync(&nbad, c->d_status + 1, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (nbad) { b->subgroup = 0; return BLSGPU_OK; }
    b->subgroup = 1;
  }
  // the images are an accelerator, not a requirement: without memory for them the MSM runs on plain 256-bit windows
  const size_t bytes = (b->group == 1 ? b->n * Store<FpPolicy>::AFF_WORDS : 4 * b->n * Store<Fp2Policy>::AFF_WORDS) * 4;
  if (hipMalloc((void**)&b->endo, bytes) != hipSuccess) { (void)hipGetLastError(); b->endo = nullptr; return BLSGPU_OK; }
  if (b->group == 1) KLAUNCH(k_bases_endo, dim3(nblk(b->n, 256)), dim3(256), 0, c->stream, b->rec, b->endo, b->n);
  else KLAUNCH(k_bases_endo_g2, dim3(nblk(b->n, 256)), dim3(256), 0, c->stream, b->rec, b->endo, b->n);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipEventRecord(b->ev_ready, c->stream);     // MSMs on another stream (blsgpu_set_stream) wait for the records and images
  if (e != hipSuccess) { hipFree(b->endo); b->endo = nullptr; return fail("k_bases_endo", e, __LINE__); }
  return BLSGPU_OK;
}
// oneshot: the set serves exactly one MSM (blsgpu_g{1,2}_msm_host / *_msm_bytes).  The subgroup test costs ~2 k (G1) / ~6 k (G2)
// field multiplications per point -- several times the MSM it would speed up (2^20 G1 points: 23 ms of test for a 3 ms MSM) -- so
// unless the caller vouches for the set it is NOT tested and keeps no images: the call runs on plain 256-bit windows, which are the
// complete-formula bucket method and exact for every curve point (state 3).  Resident uploads amortise the test over their MSMs.
template <class F>
static int bases_import(blsgpu_ctx* c, const void* d_xy, const void* d_inf, size_t n, blsgpu_bases** out, bool oneshot = false, bool trusted = false) {
  blsgpu_bases* b = new blsgpu_bases();
  b->group = GroupTag<F>::id; b->n = n; b->device = c->device;
  size_t bytes = (n ? n : 1) * Store<F>::AFF_WORDS * 4;
  if (hipEventCreateWithFlags(&b->ev_ready, hipEventDisableTiming) != hipSuccess) { delete b; g_err = "hipEventCreate(bases) failed"; return BLSGPU_ERR_HIP; }
  if (hipMalloc((void**)&b->rec, bytes) != hipSuccess) { bases_drop(b); g_err = "hipMalloc(bases) failed"; return BLSGPU_ERR_HIP; }
  if (n) {
    KLAUNCH(k_bases_import<F>, dim3(nblk(n, 256)), dim3(256), 0, c->stream, (const u32*)d_xy, (const uint8_t*)d_inf, b->rec, n);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(b->ev_ready, c->stream);
    if (e != hipSuccess) { bases_drop(b); return fail("k_bases_import", e, __LINE__); }
  }
  if (oneshot && !c->assume_subgroup) { b->subgroup = 3; *out = b; return BLSGPU_OK; }
  if (int rc = bases_make_endo(c, b, trusted)) { bases_drop(b); return rc; }      // trusted: in the subgroup by construction (the transform of an SRS)
  *out = b;
  return BLSGPU_OK;
}
static int bases_check(const char* msg, blsgpu_ctx* c, const void* xy, size_t n, blsgpu_bases** out) { return (!c || !out || (n && !xy)) ? bad(msg) : BLSGPU_OK; }
template <class F>
static int bases_upload(blsgpu_ctx* c, const uint64_t* xy, const uint8_t* inf, size_t n, blsgpu_bases** out, bool oneshot = false) {
  if (int rc = bases_check("bases_upload: NULL argument", c, xy, n, out)) return rc;
  HostCall h(c);
  void* dxy = h.in(c->io_a, xy, n * 2 * Wire<F>::WORDS * 4);
  void* dinf = h.in(c->flags_a, inf, n);
  if (h.rc) return h.rc;
  return h.finish(bases_import<F>(c, dxy, dinf, n, out, oneshot));
}
extern "C" int blsgpu_g1_bases_upload(blsgpu_ctx* c, const uint64_t* xy, const uint8_t* inf, size_t n, blsgpu_bases** out) { CTX_CLAIM(c); return bases_upload<FpPolicy>(c, xy, inf, n, out); }
extern "C" int blsgpu_g2_bases_upload(blsgpu_ctx* c, const uint64_t* xy, const uint8_t* inf, size_t n, blsgpu_bases** out) { CTX_CLAIM(c); return bases_upload<Fp2Policy>(c, xy, inf, n, out); }
extern "C" int blsgpu_g1_bases_from_device(blsgpu_ctx* c, const void* xy, const void* inf, size_t n, blsgpu_bases** out) { CTX_CLAIM(c);
  if (int rc = bases_check("bases_from_device: NULL argument", c, xy, n, out)) return rc;
  HIPCHK(hipSetDevice(c->device));
  return bases_import<FpPolicy>(c, xy, inf, n, out);
}
extern "C" int blsgpu_g2_bases_from_device(blsgpu_ctx* c, const void* xy, const void* inf, size_t n, blsgpu_bases** out) { CTX_CLAIM(c);
  if (int rc = bases_check("bases_from_device: NULL argument", c, xy, n, out)) return rc;
  HIPCHK(hipSetDevice(c->device));
  return bases_import<Fp2Policy>(c, xy, inf, n, out);
}
// [k_i]G for n one-byte-per-limb scalars already on the device; the fixed-base table of the group is built first when this call needs it
// (*fb_built: marked ready by the caller once the call has synchronised)
static int bases_from_scalars_core(blsgpu_ctx* c, int group, const void* d_scalars, size_t n, blsgpu_bases** out, bool* fb_built) {
  blsgpu_bases* b = new blsgpu_bases();
  b->group = group; b->n = n; b->device = c->device;
  size_t words = group == 1 ? Store<FpPolicy>::AFF_WORDS : Store<Fp2Policy>::AFF_WORDS;
  if (hipEventCreateWithFlags(&b->ev_ready, hipEventDisableTiming) != hipSuccess) { delete b; g_err = "hipEventCreate(bases) failed"; return BLSGPU_ERR_HIP; }
  if (hipMalloc((void**)&b->rec, (n ? n : 1) * words * 4) != hipSuccess) { bases_drop(b); g_err = "hipMalloc(bases) failed"; return BLSGPU_ERR_HIP; }
  bool fb_built_now = false;
  if (n) {
    // below a few thousand multiples the double-and-add kernel is as fast as building the comb table would be
    const bool comb = n >= 4096 || c->fb_ready[group - 1];
    if (comb && !c->fb_ready[group - 1]) {
      // table[w * 256 + d] = [d * 2^(8 w)] G: 8 192 scalars with one non-zero byte each, through the double-and-add kernel, once per context
      DevBuf& tb = c->fb_table[group - 1];
      std::vector<uint8_t> one_byte((size_t)8192 * 32, 0);
      for (int w = 0; w < 32; w++) for (int d = 0; d < 256; d++) one_byte[((size_t)w * 256 + d) * 32 + w] = (uint8_t)d;
      // staged through a buffer of its own: io_c is the scratch of the asynchronous multi_miller_loop_many_device, whose partial products
      // may still be in flight on another stream (blsgpu_set_stream)
      if (tb.reserve((size_t)8192 * words * 4) || c->fb_stage.reserve((size_t)8192 * 32)) { bases_drop(b); g_err = "hipMalloc(fixed-base table) failed"; return BLSGPU_ERR_HIP; }
      hipError_t e = hipMemcpyAsync(c->fb_stage.p, one_byte.data(), one_byte.size(), hipMemcpyHostToDevice, c->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(c->stream);                 // `one_byte` lives on this frame
      if (e != hipSuccess) { bases_drop(b); return fail("fixed-base table upload", e, __LINE__); }
      if (group == 1) KLAUNCH(k_bases_from_scalars<FpPolicy>, dim3(nblk(8192, 256)), dim3(256), 0, c->stream, c->fb_stage.as<u32>(), tb.as<u32>(), (size_t)8192);
      else KLAUNCH(k_bases_from_scalars<Fp2Policy>, dim3(nblk(8192, 256)), dim3(256), 0, c->stream, c->fb_stage.as<u32>(), tb.as<u32>(), (size_t)8192);
      e = hipGetLastError();
      if (e == hipSuccess) e = hipEventRecord(c->ev_fb[group - 1], c->stream);
      if (e != hipSuccess) { bases_drop(b); return fail("fixed-base table build", e, __LINE__); }
      fb_built_now = true;                 // marked ready only once the build is known to have run (the synchronisation at the end of this call)
    }
    if (comb) {
      hipError_t e = hipStreamWaitEvent(c->stream, c->ev_fb[group - 1], 0);
      if (e != hipSuccess) { bases_drop(b); return fail("fixed-base table wait", e, __LINE__); }
      if (group == 1) KLAUNCH(k_fixed_base<FpPolicy>, dim3(nblk(n, 256)), dim3(256), 0, c->stream, (const u32*)d_scalars, c->fb_table[0].as<u32>(), b->rec, n);
      else KLAUNCH(k_fixed_base<Fp2Policy>, dim3(nblk(n, 256)), dim3(256), 0, c->stream, (const u32*)d_scalars, c->fb_table[1].as<u32>(), b->rec, n);
    } else if (group == 1) KLAUNCH(k_bases_from_scalars<FpPolicy>, dim3(nblk(n, 256)), dim3(256), 0, c->stream, (const u32*)d_scalars, b->rec, n);
    else KLAUNCH(k_bases_from_scalars<Fp2Policy>, dim3(nblk(n, 256)), dim3(256), 0, c->stream, (const u32*)d_scalars, b->rec, n);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(b->ev_ready, c->stream);
    if (e != hipSuccess) { bases_drop(b); return fail("k_bases_from_scalars", e, __LINE__); }
  }
  if (int rc = bases_make_endo(c, b, true)) { bases_drop(b); return rc; }      // [k]G lies in the subgroup by construction
  *fb_built = fb_built_now;
  *out = b;
  return BLSGPU_OK;
}
extern "C" int blsgpu_bases_from_scalars(blsgpu_ctx* c, int group, const uint8_t* scalars, size_t n, blsgpu_bases** out) { CTX_CLAIM(c);
  if (!c || !out || (n && !scalars) || (group != 1 && group != 2)) return bad("bases_from_scalars: bad argument");
  HostCall h(c);
  void* ds = h.in(c->io_a, scalars, n * 32);
  if (h.rc) return h.rc;
  blsgpu_bases* b = nullptr;
  bool fb_built = false;
  int rc = h.finish(bases_from_scalars_core(c, group, ds, n, &b, &fb_built));
  if (rc) { if (b) bases_drop(b); return rc; }        // (a table built in this call stays unmarked: rebuilt next time)
  if (fb_built) c->fb_ready[group - 1] = true;
  *out = b;
  return BLSGPU_OK;
}
extern "C" size_t blsgpu_bases_len(const blsgpu_bases* b) { return b ? b->n : 0; }
extern "C" int blsgpu_bases_subgroup_state(const blsgpu_bases* b) { return b ? b->subgroup : 0; }
extern "C" int blsgpu_set_assume_subgroup(blsgpu_ctx* c, int on) { CTX_CLAIM(c); if (!c) return bad("ctx is NULL"); c->assume_subgroup = on != 0; return BLSGPU_OK; }
extern "C" void blsgpu_bases_free(blsgpu_bases* b) {
  if (!b) return;
  hipSetDevice(b->device);
  hipDeviceSynchronize();                  // an asynchronous MSM may still be reading the records
  bases_drop(b);
}
template <class F>
static int bases_precompute(blsgpu_ctx* c, blsgpu_bases* b, int cw) {
  const int nwin = (256 + cw - 1) / cw;
  if ((size_t)nwin * b->n > ((size_t)1 << 24)) return bad("bases_precompute: n * windows must not exceed 2^24");
  if (b->table) { HIPCHK(hipFree(b->table)); b->table = nullptr; b->table_c = 0; }
  size_t bytes = (size_t)nwin * (b->n ? b->n : 1) * Store<F>::AFF_WORDS * 4;
  HIPCHK(hipMalloc((void**)&b->table, bytes));
  if (b->n) {
    KLAUNCH(k_bases_precompute<F>, dim3(nblk(b->n, 256)), dim3(256), 0, c->stream, b->rec, b->table, b->n, cw, nwin);
    LAUNCHCHK();
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  b->table_c = cw; b->table_w = nwin;
  return BLSGPU_OK;
}
extern "C" int blsgpu_bases_precompute(blsgpu_ctx* c, blsgpu_bases* b, int window_bits) { CTX_CLAIM(c);
  if (!c || !b) return bad("bases_precompute: NULL argument");
  if (window_bits == 0) window_bits = 20;
  if (window_bits < 9 || window_bits > 21) return bad("bases_precompute: window must be in [9, 21]");
  HIPCHK(hipSetDevice(c->device));
  return b->group == 1 ? bases_precompute<FpPolicy>(c, b, window_bits) : bases_precompute<Fp2Policy>(c, b, window_bits);
}

template <class F>
static int bases_export(blsgpu_ctx* c, const blsgpu_bases* b, size_t first, size_t count, void* d_xy, void* d_inf) {
  KLAUNCH(k_bases_export<F>, dim3(nblk(count, 256)), dim3(256), 0, c->stream, b->rec + first * Store<F>::AFF_WORDS, (u32*)d_xy, (uint8_t*)d_inf, count);
  LAUNCHCHK();
  return BLSGPU_OK;
}
extern "C" int blsgpu_bases_download(blsgpu_ctx* c, const blsgpu_bases* b, size_t first, size_t count, uint64_t* xy, uint8_t* inf) { CTX_CLAIM(c);
  if (!c || !b || (count && !xy) || first > b->n || count > b->n - first) return bad("bases_download: bad argument");
  if (b->device != c->device) return bad("bases_download: bases live on another device than the context");
  if (!count) return BLSGPU_OK;
  HostCall h(c);
  void* dxy = h.out(c->io_out, xy, count * 2 * (b->group == 1 ? Wire<FpPolicy>::WORDS : Wire<Fp2Policy>::WORDS) * 4);
  void* dinf = h.out(c->flags_b, inf, count);
  if (h.rc) return h.rc;
  return h.finish(b->group == 1 ? bases_export<FpPolicy>(c, b, first, count, dxy, dinf) : bases_export<Fp2Policy>(c, b, first, count, dxy, dinf));
}

// ---------------------------------------------------------------------------------------------------
// MSM
// ---------------------------------------------------------------------------------------------------
// The shape of a call, the sizes of its scratch and the schedule of its bucket reduction are plain host code (msm_plan.h); what the
// plan restates from the device headers is held to them here.
static_assert(MSMP_TEAM == TEAM && MSMP_SORT_MAX_COUNTERS == SORT_MAX_COUNTERS && MSMP_TREE_JOBS_MAX == TREE_JOBS_MAX, "msm_plan.h restates team.hip.h / msm.hip.h");
static_assert(MSMP_CTRL_WORDS == 4 + 2 * ITEM_BINS && MSMP_ITEM_BYTES == sizeof(ItemDesc) && MSMP_HEAVY_BYTES == sizeof(uint4), "msm_plan.h restates msm.hip.h");
static_assert(MSMP_MAX_LEVELS == sizeof(blsgpu_ctx::Slot::ev_lvl) / sizeof(hipEvent_t), "one event per reduction level");
#define TEAM_LDS(threads) ((size_t)team_lds_words<F>(threads) * 4)

template <class F>
static int msm_check(blsgpu_ctx* c, const blsgpu_bases* bases, size_t first, const void* scalars, size_t n, const void* out) {
  if (!c || !bases || !out || (n && !scalars)) return bad("msm: NULL argument");
  if (bases->group != GroupTag<F>::id) return bad("msm: bases belong to the other group");
  if (first > bases->n || n > bases->n - first) return bad("msm: range exceeds the resident bases");
  if (bases->device != c->device) return bad("msm: bases live on another device than the context");
  if (n > ((size_t)1 << 27)) return bad("msm: n too large for one call (shard the input)");
  return BLSGPU_OK;
}
// the slot's buffers at the sizes of the plan, in a fixed order.  ft: the stream the sort runs on (a fresh counter buffer is cleared
// there); st: the caller's stream
static int msm_reserve(blsgpu_ctx::Slot& sl, const MsmSizes& z, hipStream_t ft, hipStream_t st) {
  int bad_alloc = 0;
  bad_alloc |= sl.ent.reserve(z.ent);
  bad_alloc |= sl.sorted.reserve(z.sorted);
  const bool fresh = sl.hist.cap < z.hist;
  bad_alloc |= sl.hist.reserve(z.hist);
  if (fresh && !bad_alloc) HIPCHK(hipMemsetAsync(sl.hist.p, 0, sl.hist.cap, ft));      // the sort keeps its counters zeroed between calls
  bad_alloc |= sl.cursor.reserve(z.cursor);
  bad_alloc |= sl.glv.reserve(z.glv);
  bad_alloc |= sl.offs.reserve(z.offs);
  bad_alloc |= sl.bsum.reserve(z.bsum);
  bad_alloc |= sl.items.reserve(z.items);
  bad_alloc |= sl.heavy.reserve(z.heavy);
  bad_alloc |= sl.ctrl.reserve(z.ctrl);
  // (re)allocation frees memory: make sure nothing of this slot is in flight
  const bool grow = sl.buckets.cap < z.buckets || sl.lvlR[0].cap < z.lvlR || sl.lvlT.cap < z.lvlT || sl.wacc[0].cap < z.wacc || sl.wsums.cap < z.wsums;
  if (grow) { HIPCHK(hipStreamSynchronize(sl.tail)); HIPCHK(hipStreamSynchronize(sl.tail2)); HIPCHK(hipStreamSynchronize(st)); }
  bad_alloc |= sl.buckets.reserve(z.buckets);
  bad_alloc |= sl.lvlR[0].reserve(z.lvlR); bad_alloc |= sl.lvlR[1].reserve(z.lvlR); bad_alloc |= sl.lvlT.reserve(z.lvlT);
  bad_alloc |= sl.tsum[0].reserve(z.tsum); bad_alloc |= sl.tsum[1].reserve(z.tsum);
  bad_alloc |= sl.wacc[0].reserve(z.wacc); bad_alloc |= sl.wacc[1].reserve(z.wacc);
  bad_alloc |= sl.wsums.reserve(z.wsums);
  bad_alloc |= sl.result.reserve(z.result);
  if (bad_alloc) { g_err = "hipMalloc(msm scratch) failed"; return BLSGPU_ERR_HIP; }
  return BLSGPU_OK;
}

// phase marks of blsgpu_set_profiling
static inline void msm_mark(blsgpu_ctx* c, int i, hipStream_t stream) { if (c->profiling) hipEventRecord(c->ev[i], stream); }

// 1'-3'. the two-level counting sort (LDS atomics; see msm.hip.h) on ft, behind the decomposition of the scalars where the call has one.
// stride: the resident bases' count (the index of a table entry is window * stride + i)
static int msm_sort_fast(blsgpu_ctx* c, blsgpu_ctx::Slot& sl, const MsmShape& s, const void* d_scalars, u32 stride, hipStream_t ft) {
  // fixed layout: [MAX] counts (kept zero between calls) | [MAX+1] bases | [MAX] cursors
  u32* ghist = sl.hist.as<u32>();
  u32* gbase = ghist + SORT_MAX_COUNTERS;
  u32* gcur = gbase + SORT_MAX_COUNTERS + 1;
  if (sl.hist_dirty) { HIPCHK(hipMemsetAsync(ghist, 0, (size_t)SORT_MAX_COUNTERS * 4, ft)); sl.hist_dirty = false; }
  const unsigned tiles = nblk(s.ns, SORT_TILE);
  const int n = (int)s.n, ns = (int)s.ns, nc = s.nc, sform = c->scalar_form;
  const u32* sort_in = (const u32*)d_scalars;
  if (s.glv) {
    KLAUNCH(k_glv_decompose, dim3(nblk(s.n, 256)), dim3(256), 0, ft, (const u32*)d_scalars, sl.glv.as<u32>(), n, c->status_word, sform);
    sort_in = sl.glv.as<u32>();
    KLAUNCH(k_sort_hist<4>, dim3(tiles), dim3(SORT_THREADS), (size_t)nc * 4, ft, sort_in, ghist, ns, s.cw, s.nwin, s.fine_bits, s.ncoarse, 0, c->status_word);
  } else if (s.gls) {
    KLAUNCH(k_gls_decompose, dim3(nblk(s.n, 256)), dim3(256), 0, ft, (const u32*)d_scalars, sl.glv.as<u32>(), n, c->status_word, sform);
    sort_in = sl.glv.as<u32>();
    KLAUNCH(k_sort_hist<2>, dim3(tiles), dim3(SORT_THREADS), (size_t)nc * 4, ft, sort_in, ghist, ns, s.cw, s.nwin, s.fine_bits, s.ncoarse, 0, c->status_word);
  } else {
    KLAUNCH(k_sort_hist<8>, dim3(tiles), dim3(SORT_THREADS), (size_t)nc * 4, ft, sort_in, ghist, ns, s.cw, s.nwin, s.fine_bits, s.ncoarse, s.merged ? 1 : 0, c->status_word);
  }
  LAUNCHCHK();
  msm_mark(c, 1, ft);
  KLAUNCH(k_sort_scan, dim3(1), dim3(1024), 0, ft, ghist, gbase, gcur, nc, sl.ctrl.as<u32>(), 4 + 2 * ITEM_BINS);
  LAUNCHCHK();
  msm_mark(c, 2, ft);
  if (s.glv)
    KLAUNCH(k_sort_scatter<4>, dim3(tiles), dim3(SORT_THREADS), (size_t)nc * 8, ft, sort_in, gbase, gcur, sl.ent.as<u32>(), ns, s.cw, s.nwin, s.fine_bits, s.ncoarse, 0, (u32)0);
  else if (s.gls)
    KLAUNCH(k_sort_scatter<2>, dim3(tiles), dim3(SORT_THREADS), (size_t)nc * 8, ft, sort_in, gbase, gcur, sl.ent.as<u32>(), ns, s.cw, s.nwin, s.fine_bits, s.ncoarse, 0, (u32)0);
  else
    KLAUNCH(k_sort_scatter<8>, dim3(tiles), dim3(SORT_THREADS), (size_t)nc * 8, ft, sort_in, gbase, gcur, sl.ent.as<u32>(), ns, s.cw, s.nwin,
                       s.fine_bits, s.ncoarse, s.merged ? 1 : 0, stride);
  KLAUNCH(k_sort_fine, dim3(nc), dim3(256), 0, ft, sl.ent.as<u32>(), gbase, sl.sorted.as<u32>(), sl.offs.as<u32>(), s.fine_bits, nc);
  LAUNCHCHK();
  msm_mark(c, 3, ft);
  return BLSGPU_OK;
}
// 1.-3. the fallback beyond the counting sort's reach (more than 2^24 sort scalars; BLSGPU_FORCE_SLOW_SORT): global atomics, on ft
static int msm_sort_fallback(blsgpu_ctx* c, blsgpu_ctx::Slot& sl, const MsmShape& s, const void* d_scalars, hipStream_t ft) {
  const int n = (int)s.n, nb = (int)s.nb;
  // 1. digits + histogram
  sl.hist_dirty = true;
  HIPCHK(hipMemsetAsync(sl.hist.p, 0, s.nb * 4, ft));
  HIPCHK(hipMemsetAsync(sl.ctrl.p, 0, (4 + 2 * ITEM_BINS) * 4, ft));
  KLAUNCH(k_msm_digits, dim3(nblk(s.n, 256)), dim3(256), 0, ft, (const u32*)d_scalars, sl.ent.as<u32>(), sl.cursor.as<u32>(), sl.hist.as<u32>(), n, s.cw, s.nwin, c->status_word);
  LAUNCHCHK();
  msm_mark(c, 1, ft);
  // 2. scan
  const unsigned sb = nblk(s.nb, 1024);
  KLAUNCH(k_scan_block_sums, dim3(sb), dim3(256), 0, ft, sl.hist.as<u32>(), sl.bsum.as<u32>(), nb);
  KLAUNCH(k_scan_top, dim3(1), dim3(1024), 0, ft, sl.bsum.as<u32>(), (int)sb);
  KLAUNCH(k_scan_apply, dim3(sb), dim3(256), 0, ft, sl.hist.as<u32>(), sl.bsum.as<u32>(), sl.offs.as<u32>(), nb);
  LAUNCHCHK();
  msm_mark(c, 2, ft);
  // 3. scatter
  KLAUNCH(k_msm_scatter, dim3(nblk(s.total, 256)), dim3(256), 0, ft, sl.ent.as<u32>(), sl.cursor.as<u32>(), sl.offs.as<u32>(), sl.sorted.as<u32>(), n, s.total);
  LAUNCHCHK();
  msm_mark(c, 3, ft);
  return BLSGPU_OK;
}


// 4.-5. work items on ft, then the bucket accumulation and the fold of cut buckets on as: records [0, nb) of sl.buckets end as the bucket sums
template <class F>
static int msm_accumulate(blsgpu_ctx* c, const blsgpu_bases* bases, size_t first, blsgpu_ctx::Slot& sl, const MsmShape& s, hipStream_t ft, hipStream_t as) {
  const int nb = (int)s.nb;
  u32* ctrl = sl.ctrl.as<u32>();
  u32* bins = ctrl + 4;
  u32* bcur = ctrl + 4 + ITEM_BINS;
  // 4. work items
  KLAUNCH(k_item_count, dim3(nblk(s.nb, ITEM_BLOCK_BUCKETS)), dim3(256), 0, ft, sl.offs.as<u32>(), bins, ctrl, nb, s.cap);
  KLAUNCH(k_item_scan, dim3(1), dim3(256), 0, ft, bins, ctrl, s.cap);
  KLAUNCH(k_item_fill, dim3(nblk(s.nb, ITEM_BLOCK_BUCKETS)), dim3(256), 0, ft, sl.offs.as<u32>(), bins, bcur, ctrl, sl.items.as<ItemDesc>(),
                     sl.heavy.as<uint4>(), nb, s.cap);
  LAUNCHCHK();
  msm_mark(c, 4, ft);
  if (as != ft) { HIPCHK(hipEventRecord(sl.ev_front, ft)); HIPCHK(hipStreamWaitEvent(as, sl.ev_front, 0)); }
  // the records (and images) may have been written on another stream than this call's (blsgpu_set_stream after the upload)
  if (!bases->ready_seen) {
    if (hipEventQuery(bases->ev_ready) == hipSuccess) bases->ready_seen = true;
    else HIPCHK(hipStreamWaitEvent(as, bases->ev_ready, 0));
  }
  // 5. accumulate (grid covers the worst-case item count; surplus lanes exit on ctrl[2])
  // timing events are not free in a pipelined run (two records cost ~0.05-0.1 ms of queue time per MSM): sample every N-th launch
  const bool time_this = c->acc_timing && (c->acc_tick++ % (unsigned)c->acc_timing) == 0;
  if (time_this) { acc_harvest(c, false); if (sl.k_pending) { hipEventSynchronize(sl.ev_k1); acc_harvest(c, false); } hipEventRecord(sl.ev_k0, as); }
  u32* records = sl.buckets.as<u32>();
  const u32* base_rec = (s.merged ? bases->table : bases->rec) + first * Store<F>::AFF_WORDS;
  if constexpr (GroupTag<F>::id == 2)
    KLAUNCH(k_msm_accumulate_g2pair, dim3(nblk(2 * s.max_items, BLS_G2ACC_BLOCK)), dim3(BLS_G2ACC_BLOCK), 0, as, s.gls ? bases->endo + 4 * first * Store<F>::AFF_WORDS : base_rec,
                       sl.sorted.as<u32>(), sl.items.as<ItemDesc>(), ctrl, records);
  else
    KLAUNCH(k_msm_accumulate<F>, dim3(nblk(s.max_items, BLS_ACC_BLOCK)), dim3(BLS_ACC_BLOCK), 0, as, base_rec, s.glv ? bases->endo + first * Store<F>::AFF_WORDS : (const u32*)nullptr,
                       s.glv ? (u32)s.n : 0xffffffffu, sl.sorted.as<u32>(), sl.items.as<ItemDesc>(), ctrl, records);
  if (time_this) { hipEventRecord(sl.ev_k1, as); sl.k_pending = true; }
  // the fold of cut buckets (almost always a no-op) stays on the accumulation stream: as the first kernel of the tail it made
  // the next accumulation start ~90 us earlier, inside the previous call's bottom reduction level, and the pipelined rate FELL
  // by 2.6 % (A/B on one box, twice: 3.57 vs 3.66*10^8 scalar-muls/s)
  const u32 heavy_small_blocks = (u32)nblk(s.nb, 256);
  KLAUNCH(k_msm_heavy<F>, dim3(heavy_small_blocks + HEAVY_BIG_BLOCKS), dim3(256), 0, as, sl.heavy.as<uint4>(), ctrl, records, (u32)s.nb, heavy_small_blocks);
  LAUNCHCHK();
  return BLSGPU_OK;
}

// the rows of the Horner table: the T sum of level l for every bucket set, in wacc[0]
template <class F> static u32* msm_horner_row(blsgpu_ctx::Slot& sl, int nseg, int level) { return sl.wacc[0].as<u32>() + (size_t)level * nseg * Store<F>::PROJ_WORDS; }
// one pass of every unfinished T tree, on t2: a single multi-job launch when all of them fit the team form
template <class F>
static int msm_tree_step(blsgpu_ctx::Slot& sl, int nseg, const MsmTreeStep& step, hipStream_t t2) {
  constexpr int PW = Store<F>::PROJ_WORDS;
  auto in = [&](const MsmTreePass& p) -> const u32* { return (p.src < 0 ? sl.lvlT.as<u32>() : sl.tsum[p.src].as<u32>()) + p.off * PW; };
  auto out = [&](const MsmTreePass& p) -> u32* { return p.to_horner ? msm_horner_row<F>(sl, nseg, p.level) : sl.tsum[p.pp].as<u32>() + p.off * PW; };
  for (int i = 0; i < step.npass; i++) {
    const MsmTreePass& p = step.pass[i];
    if (!p.multi) KLAUNCH(k_tree_sum<F>, dim3(nblk((size_t)nseg * p.TG, 256)), dim3(256), 0, t2, in(p), out(p), nseg, p.n, p.TM);
  }
  TreeJobs J;
  msm_tree_jobs(J, nseg, step, in, out);
  if (J.njobs) KLAUNCH(k_tree_sum_team_multi<F>, dim3(step.multi_grid), dim3(MSMP_BLOCK), TEAM_LDS(256), t2, J);
  LAUNCHCHK();
  return BLSGPU_OK;
}
// 6. per-window weighted sums  wsum = sum_b (b + 1) * bucket_b  by the schedule of msm_plan.h: the levels on tt, the T trees on t2;
// sl.wsums ends as one record per bucket set
template <class F>
static int msm_reduce(blsgpu_ctx::Slot& sl, const MsmReduction& red, hipStream_t tt, hipStream_t t2) {
  constexpr int PW = Store<F>::PROJ_WORDS;
  const int nseg = red.nseg;
  const u32* records = sl.buckets.as<u32>();
  const u32* E = records;
  for (int l = 0; l < red.levels; l++) {
    const MsmLevel& L = red.level[l];
    u32* Rout = sl.lvlR[l & 1].as<u32>();
    u32* Tout = L.to_horner ? msm_horner_row<F>(sl, nseg, l) : sl.lvlT.as<u32>() + L.toff * PW;
    // team2: the two running sums of a chain (R and T) advance on two teams / two lanes, T one step behind R: M + 1 dependent
    // additions per level instead of 2 M
    if (L.form == MSM_FORM_TEAM2)
      KLAUNCH(k_wsum_level_team2<F>, dim3(L.grid), dim3(MSMP_BLOCK),
                         TEAM_LDS(256) + (size_t)(256 / TEAM / 2) * 3 * TeamTraits<F>::WORDS * 4, tt, E, Rout, Tout, nseg, L.n, L.M, L.off);
    else if (L.form == MSM_FORM_TEAM)
      KLAUNCH(k_wsum_level_team<F>, dim3(L.grid), dim3(MSMP_BLOCK), TEAM_LDS(256), tt, E, Rout, Tout, nseg, L.n, L.M, L.off);
    else if constexpr (GroupTag<F>::id == 2)
      KLAUNCH(k_wsum_level_g2pair, dim3(L.grid), dim3(MSMP_BLOCK), 0, tt, E, Rout, Tout, nseg, L.n, L.M, L.off);
    else
      KLAUNCH(k_wsum_level_pair, dim3(nblk(L.lanes, BLS_WSUM_BLOCK)), dim3(BLS_WSUM_BLOCK), 0, tt, E, Rout, Tout, nseg, L.n, L.M, L.off);
    LAUNCHCHK();
    // sum the G T-records of each window down to one -- on the second tail stream: the next level needs only Rout.  Level l
    // needs log8(G_l) passes; after every level ONE launch carries the next pass of every tree that still has one (the T
    // trees of different levels are independent), so the trees finish while the R chain is still running.
    if (L.G > 1 && t2 != tt) { HIPCHK(hipEventRecord(sl.ev_lvl[l], tt)); HIPCHK(hipStreamWaitEvent(t2, sl.ev_lvl[l], 0)); }
    if (int rc = msm_tree_step<F>(sl, nseg, red.step[l], t2)) return rc;
    E = Rout;
  }
  for (int t = red.levels; t < red.nsteps; t++)              // passes that are left when the last level has run
    if (int rc = msm_tree_step<F>(sl, nseg, red.step[t], t2)) return rc;
  if (t2 != tt) { HIPCHK(hipEventRecord(sl.ev_tree, t2)); HIPCHK(hipStreamWaitEvent(tt, sl.ev_tree, 0)); }
  if (red.levels == 0) {
    // a single bucket per window (c = 1): the bucket itself is the window sum
    HIPCHK(hipMemcpyAsync(sl.wsums.p, records, (size_t)nseg * PW * 4, hipMemcpyDeviceToDevice, tt));
    return BLSGPU_OK;
  }
  // Horner over the levels: acc_L = T_L ; acc_l = T_l + M_l * acc_{l+1}
  u32* accbuf = sl.wacc[1].as<u32>();
  HIPCHK(hipMemcpyAsync(accbuf, msm_horner_row<F>(sl, nseg, red.levels - 1), (size_t)nseg * PW * 4, hipMemcpyDeviceToDevice, tt));
  for (int l = red.levels - 2; l >= 0; l--) {
    KLAUNCH(k_shift_add_team<F>, dim3(nblk((size_t)nseg * TEAM, 256)), dim3(256), TEAM_LDS(256), tt, accbuf, msm_horner_row<F>(sl, nseg, l), accbuf, nseg, red.level[l].shift);
    LAUNCHCHK();
  }
  HIPCHK(hipMemcpyAsync(sl.wsums.p, accbuf, (size_t)nseg * PW * 4, hipMemcpyDeviceToDevice, tt));
  return BLSGPU_OK;
}
// 7. combine the window sums and export the result, on tt
template <class F>
static int msm_combine(blsgpu_ctx::Slot& sl, const MsmShape& s, void* d_out_wire, hipStream_t tt) {
  KLAUNCH(k_msm_combine_team<F>, dim3(1), dim3(TEAM), TEAM_LDS(TEAM), tt, sl.wsums.as<u32>(), sl.result.as<u32>(), s.nseg, s.cw);
  LAUNCHCHK();
  KLAUNCH(k_proj_export<F>, dim3(1), dim3(256), 0, tt, sl.result.as<u32>(), (u32*)d_out_wire, (size_t)1);
  LAUNCHCHK();
  return BLSGPU_OK;
}


template <class F>
static int msm_device(blsgpu_ctx* c, const blsgpu_bases* bases, size_t first, const void* d_scalars, size_t n, void* d_out_wire) {
  if (int rc = msm_check<F>(c, bases, first, d_scalars, n, d_out_wire)) return rc;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  constexpr int PW = Store<F>::PROJ_WORDS;
  if (c->result.reserve(PW * 4)) { g_err = "hipMalloc failed"; return BLSGPU_ERR_HIP; }
  if (n == 0) {
    if (blsgpu_join(c) != BLSGPU_OK) return BLSGPU_ERR_HIP;
    KLAUNCH(k_store_identity<F>, dim3(1), dim3(64), 0, st, c->result.as<u32>());
    LAUNCHCHK();
    KLAUNCH(k_proj_export<F>, dim3(1), dim3(256), 0, st, c->result.as<u32>(), (u32*)d_out_wire, (size_t)1);
    LAUNCHCHK();
    return BLSGPU_OK;
  }
  // the whole configuration is validated BEFORE a slot is taken or anything is enqueued
  const MsmShape s = msm_shape(GroupTag<F>::id, n, bases->table ? bases->table_c : 0, bases->endo != nullptr, c->no_glv, c->force_slow_sort, c->msm_c, c->item_cap);
  if (s.refusal) return bad(s.refusal);
  const MsmReduction red = msm_reduction(s.nseg, s.nbw);
  if (red.refusal) return bad(red.refusal);
  const MsmSizes z = msm_sizes(s, PW, c->scalar_form == SCALAR_MONT);
  blsgpu_ctx::Slot& sl = c->slot[c->next_slot];
  c->next_slot = (c->next_slot + 1) % NSLOT;
  // One call at a time (no pipelining): front, accumulation and tail run on the caller's stream -- every cross-stream
  // dependency costs a barrier packet and 20-90 us of idle time between the phases (kernel trace of a single call), and there is
  // nothing to overlap with.  Only the T tree sums keep their side stream.  Pipelined calls use the slot's own streams, and
  // accumulate on the library's own: front(i+1) must not queue behind accumulate(i).
  const bool single = !c->pipelining;
  const hipStream_t ft = single ? st : sl.front, as = single ? st : c->acc_stream, tt = single ? st : sl.tail, t2 = sl.tail2;
  // every buffer of this slot may still be in use by the call that used it last (NSLOT calls ago)
  if (sl.tail_pending) { HIPCHK(hipStreamWaitEvent(ft, sl.ev_tail, 0)); HIPCHK(hipStreamWaitEvent(st, sl.ev_tail, 0)); }
  if (int rc = msm_reserve(sl, z, ft, st)) return rc;
  // the front stream starts after whatever produced the scalars on the caller's stream
  if (ft != st) { HIPCHK(hipEventRecord(sl.ev_in, st)); HIPCHK(hipStreamWaitEvent(ft, sl.ev_in, 0)); }

  // ---- front: the sorted entry list and the bucket offsets ----------------------------------------------------------------------------
  msm_mark(c, 0, ft);
  if (c->scalar_form == SCALAR_MONT && !s.glv && !s.gls) {       // no decomposition kernel touches the scalars: reduce them first
    KLAUNCH(k_scalars_from_mont, dim3(nblk(n, 256)), dim3(256), 0, ft, (const u32*)d_scalars, sl.glv.as<u32>(), (int)n, c->status_word);
    LAUNCHCHK();
    d_scalars = sl.glv.p;
  }
  if (int rc = s.fast_sort ? msm_sort_fast(c, sl, s, d_scalars, (u32)bases->n, ft) : msm_sort_fallback(c, sl, s, d_scalars, ft)) return rc;
  // ---- accumulate, reduce, combine: all windows of the call at once (cutting a single call into a high and a low window group whose
  // tails overlap was measured in round 4 and is slower, tools/experiments/msm_window_groups.patch) -------------------------------------
  if (int rc = msm_accumulate<F>(c, bases, first, sl, s, ft, as)) return rc;
  msm_mark(c, 5, as);
  if (tt != as) { HIPCHK(hipEventRecord(sl.ev_acc, as)); HIPCHK(hipStreamWaitEvent(tt, sl.ev_acc, 0)); }
  if (int rc = msm_reduce<F>(sl, red, tt, t2)) return rc;
  msm_mark(c, 6, tt);
  if (int rc = msm_combine<F>(sl, s, d_out_wire, tt)) return rc;
  msm_mark(c, 7, tt);
  // ---- bookkeeping ---------------------------------------------------------------------------------------------------------------------
  HIPCHK(hipEventRecord(sl.ev_tail, tt));
  sl.tail_pending = true;
  sl.seq = ++c->msm_calls;
  if (c->profiling) {
    HIPCHK(hipStreamSynchronize(tt));
    HIPCHK(hipStreamSynchronize(st));
    for (int i = 0; i < 7; i++) hipEventElapsedTime(&c->phase_ms[i], c->ev[i], c->ev[i + 1]);
    hipEventElapsedTime(&c->phase_ms[7], c->ev[0], c->ev[7]);
  }
  return BLSGPU_OK;
}

template <class F>
static int msm_host(blsgpu_ctx* c, const blsgpu_bases* bases, size_t first, const uint8_t* scalars, size_t n, uint64_t* out) {
  if (int rc = msm_check<F>(c, bases, first, scalars, n, out)) return rc;
  HostCall h(c);
  h.report_status();
  void* s = h.in(c->io_b, scalars, n * 32);
  void* o = h.out(c->io_out, out, 3 * Wire<F>::WORDS * 4);
  if (h.rc) return h.rc;
  int rc = msm_device<F>(c, bases, first, s, n, o);
  return h.finish(rc ? rc : blsgpu_join(c));
}
extern "C" int blsgpu_g1_msm(blsgpu_ctx* c, const blsgpu_bases* b, size_t first, const uint8_t* s, size_t n, uint64_t* out) { CTX_CLAIM(c); return msm_host<FpPolicy>(c, b, first, s, n, out); }
extern "C" int blsgpu_g2_msm(blsgpu_ctx* c, const blsgpu_bases* b, size_t first, const uint8_t* s, size_t n, uint64_t* out) { CTX_CLAIM(c); return msm_host<Fp2Policy>(c, b, first, s, n, out); }
extern "C" int blsgpu_g1_msm_device(blsgpu_ctx* c, const blsgpu_bases* b, size_t first, const void* s, size_t n, void* out) { CTX_CLAIM(c); return msm_device<FpPolicy>(c, b, first, s, n, out); }
extern "C" int blsgpu_g2_msm_device(blsgpu_ctx* c, const blsgpu_bases* b, size_t first, const void* s, size_t n, void* out) { CTX_CLAIM(c); return msm_device<Fp2Policy>(c, b, first, s, n, out); }
// the same four with the scalars as `&[Scalar]` memory holds them: four u64 Montgomery limbs each (scalar.rs:23-27); `Scalar::to_bytes`
// (:284-296) runs on the device, fused into the decomposition kernels
extern "C" int blsgpu_g1_msm_mont(blsgpu_ctx* c, const blsgpu_bases* b, size_t first, const uint64_t* s, size_t n, uint64_t* out) { CTX_CLAIM(c);
  ScalarFormScope f(c, SCALAR_MONT); return msm_host<FpPolicy>(c, b, first, (const uint8_t*)s, n, out); }
extern "C" int blsgpu_g2_msm_mont(blsgpu_ctx* c, const blsgpu_bases* b, size_t first, const uint64_t* s, size_t n, uint64_t* out) { CTX_CLAIM(c);
  ScalarFormScope f(c, SCALAR_MONT); return msm_host<Fp2Policy>(c, b, first, (const uint8_t*)s, n, out); }
extern "C" int blsgpu_g1_msm_mont_device(blsgpu_ctx* c, const blsgpu_bases* b, size_t first, const void* s, size_t n, void* out) { CTX_CLAIM(c);
  ScalarFormScope f(c, SCALAR_MONT); return msm_device<FpPolicy>(c, b, first, s, n, out); }
extern "C" int blsgpu_g2_msm_mont_device(blsgpu_ctx* c, const blsgpu_bases* b, size_t first, const void* s, size_t n, void* out) { CTX_CLAIM(c);
  ScalarFormScope f(c, SCALAR_MONT); return msm_device<Fp2Policy>(c, b, first, s, n, out); }
// k MSMs over the SAME resident bases (e.g. commitments to k polynomials under one SRS): scalars of call j at
// d_scalars + j * n * 32, result j at d_out + j * 3 * WORDS * 4.  The calls go through the pipeline slots, so the sort,
// accumulation and tail of consecutive MSMs overlap; results are ordered on the context's stream on return.
template <class F>
static int msm_many_check(blsgpu_ctx* c, const blsgpu_bases* bases, size_t first, const void* scalars, size_t n, size_t k, const void* out) {
  if (!c || !bases || (k && (!out || (n && !scalars)))) return bad("msm_many: NULL argument");
  return k ? msm_check<F>(c, bases, first, scalars, n, out) : BLSGPU_OK;
}
template <class F>
static int msm_many_device(blsgpu_ctx* c, const blsgpu_bases* bases, size_t first, const void* d_scalars, size_t n, size_t k, void* d_out) {
  if (int rc = msm_many_check<F>(c, bases, first, d_scalars, n, k, d_out)) return rc;
  const bool was = c->pipelining;
  c->pipelining = true;
  int rc = BLSGPU_OK;
  for (size_t j = 0; j < k && rc == BLSGPU_OK; j++)
    rc = msm_device<F>(c, bases, first, (const uint8_t*)d_scalars + j * n * 32, n, (uint8_t*)d_out + j * 3 * Wire<F>::WORDS * 4);
  c->pipelining = was;
  int rj = blsgpu_join(c);
  return rc ? rc : rj;
}
extern "C" int blsgpu_g1_msm_many_device(blsgpu_ctx* c, const blsgpu_bases* b, size_t first, const void* s, size_t n, size_t k, void* out) { CTX_CLAIM(c); return msm_many_device<FpPolicy>(c, b, first, s, n, k, out); }
extern "C" int blsgpu_g2_msm_many_device(blsgpu_ctx* c, const blsgpu_bases* b, size_t first, const void* s, size_t n, size_t k, void* out) { CTX_CLAIM(c); return msm_many_device<Fp2Policy>(c, b, first, s, n, k, out); }
template <class F>
static int msm_many_host(blsgpu_ctx* c, const blsgpu_bases* bases, size_t first, const uint8_t* scalars, size_t n, size_t k, uint64_t* out) {
  if (int rc = msm_many_check<F>(c, bases, first, scalars, n, k, out)) return rc;
  if (!k) return BLSGPU_OK;
  HostCall h(c);
  h.report_status();
  void* s = h.in(c->io_b, scalars, n * k * 32);
  void* o = h.out(c->io_out, out, k * 3 * Wire<F>::WORDS * 4);
  if (h.rc) return h.rc;
  return h.finish(msm_many_device<F>(c, bases, first, s, n, k, o));
}
extern "C" int blsgpu_g1_msm_many(blsgpu_ctx* c, const blsgpu_bases* b, size_t first, const uint8_t* s, size_t n, size_t k, uint64_t* out) { CTX_CLAIM(c); return msm_many_host<FpPolicy>(c, b, first, s, n, k, out); }
extern "C" int blsgpu_g2_msm_many(blsgpu_ctx* c, const blsgpu_bases* b, size_t first, const uint8_t* s, size_t n, size_t k, uint64_t* out) { CTX_CLAIM(c); return msm_many_host<Fp2Policy>(c, b, first, s, n, k, out); }

// k independent small MSMs, segment j = scalars [offsets[j], offsets[j+1]) over bases [base_first[j], base_first[j] + len_j)
// (msm_seg.hip.h): two launches per batch of segments on the context's stream, scratch of their own (a pipelined msm_device still
// in flight keeps its slot buffers), no slot of the MSM pipeline.
static_assert(BLSGPU_SEG_LEN_MAX == SEG_LEN_MAX, "include/bls12_381_hip.h and limits.h disagree on the segment length limit");
constexpr size_t SEG_K_MAX = (size_t)1 << 27;
constexpr size_t SEG_BATCH_BYTES = (size_t)64 << 20;     // window sums of one batch of segments
template <class F>
static int msm_segments_check(blsgpu_ctx* c, const blsgpu_bases* bases, const void* offsets, const void* scalars, size_t k, size_t total, const void* out) {
  if (!c || !bases || (k && (!offsets || !out)) || (total && !scalars)) return bad("msm_segments: NULL argument");
  if (bases->group != GroupTag<F>::id) return bad("msm_segments: bases belong to the other group");
  if (bases->device != c->device) return bad("msm_segments: bases live on another device than the context");
  if (total > ((size_t)1 << 27)) return bad("msm_segments: more than 2^27 scalars in one call");
  if (k > SEG_K_MAX) return bad("msm_segments: more than 2^27 segments in one call");
  return BLSGPU_OK;
}
template <class F, int MODE, class FK>
static int msm_segments_launch(blsgpu_ctx* c, const blsgpu_bases* bases, const u32* bf, const u32* off, const u32* s, size_t k, size_t total, u32* out) {
  typedef SegCfg<FK, MODE> C;
  constexpr int PW = Store<F>::PROJ_WORDS, WW = Wire<F>::WORDS;
  const size_t per_seg = (size_t)C::NWIN * PW * 4;
  size_t batch = SEG_BATCH_BYTES / per_seg;
  if (batch > k) batch = k;
  if (c->seg_wsum.reserve(batch * per_seg) || c->seg_rec.reserve(batch * PW * 4)) { g_err = "hipMalloc(msm_segments scratch) failed"; return BLSGPU_ERR_HIP; }
  for (size_t s0 = 0; s0 < k; s0 += batch) {
    const u32 nb = (u32)(k - s0 < batch ? k - s0 : batch);
    KLAUNCH((k_msm_seg_accumulate<FK, MODE>), dim3(nb * C::NGRP), dim3(SEG_THREADS), 0, c->stream, bases->rec, bases->endo, bases->n, bf, off, s,
            (u32)s0, (u32)total, c->scalar_form, c->status_word, c->seg_wsum.as<u32>());
    KLAUNCH((k_msm_seg_combine<FK, C::NWIN>), dim3(nblk((size_t)nb * C::LPA, 256)), dim3(256), 0, c->stream, c->seg_wsum.as<u32>(), c->seg_rec.as<u32>(), nb);
    KLAUNCH(k_proj_export<F>, dim3(nblk(nb, 256)), dim3(256), 0, c->stream, c->seg_rec.as<u32>(), out + s0 * 3 * WW, (size_t)nb);
    LAUNCHCHK();
  }
  return BLSGPU_OK;
}
template <class F>
static int msm_segments_device(blsgpu_ctx* c, const blsgpu_bases* bases, const void* d_bf, const void* d_off, const void* d_s, size_t k, size_t total, void* d_out) {
  if (int rc = msm_segments_check<F>(c, bases, d_off, d_s, k, total, d_out)) return rc;
  if (!k) return BLSGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  // the records (and images) may have been written on another stream than this call's (blsgpu_set_stream after the upload)
  if (!bases->ready_seen) {
    if (hipEventQuery(bases->ev_ready) == hipSuccess) bases->ready_seen = true;
    else HIPCHK(hipStreamWaitEvent(c->stream, bases->ev_ready, 0));
  }
  // the endomorphism split only for sets in the subgroup (tested or vouched for) whose images are resident, as in msm_device
  const bool split = (bases->subgroup == 1 || bases->subgroup == 2) && bases->endo && !c->no_glv;
  const u32 *bf = (const u32*)d_bf, *off = (const u32*)d_off, *s = (const u32*)d_s;
  u32* out = (u32*)d_out;
  if constexpr (GroupTag<F>::id == 1)
    return split ? msm_segments_launch<F, SEG_GLV, FpPolicy>(c, bases, bf, off, s, k, total, out) : msm_segments_launch<F, SEG_PLAIN, FpPolicy>(c, bases, bf, off, s, k, total, out);
  else
    return split ? msm_segments_launch<F, SEG_GLS, Fp2PairPolicy>(c, bases, bf, off, s, k, total, out) : msm_segments_launch<F, SEG_PLAIN, Fp2PairPolicy>(c, bases, bf, off, s, k, total, out);
}
template <class F>
static int msm_segments_host(blsgpu_ctx* c, const blsgpu_bases* bases, const uint32_t* base_first, const uint32_t* offsets, const uint8_t* scalars, size_t k, uint64_t* out) {
  if (!offsets && k) return bad("msm_segments: NULL argument");
  const size_t total = k ? offsets[k] : 0;
  if (int rc = msm_segments_check<F>(c, bases, offsets, scalars, k, total, out)) return rc;
  if (!k) return BLSGPU_OK;
  // everything is checked before anything is staged: the kernel's own checks are the device form's
  for (size_t j = 0; j < k; j++) {
    if (offsets[j + 1] < offsets[j]) return bad("msm_segments: offsets decrease");
    const size_t len = offsets[j + 1] - offsets[j];
    if (len > SEG_LEN_MAX) return bad("msm_segments: a segment is longer than BLSGPU_SEG_LEN_MAX");
    const size_t first = base_first ? base_first[j] : offsets[j];
    if (first + len > bases->n) return bad("msm_segments: a segment's bases exceed the resident set");
  }
  ScalarFormScope bytes_form(c, SCALAR_BYTES);        // the host form's scalars ARE `Scalar::to_bytes()` output, whatever the context's setting
  HostCall h(c);
  h.report_status();
  void* doff = h.in(c->io_a, offsets, (k + 1) * 4);
  void* dbf = h.in(c->io_e, base_first, k * 4);
  void* ds = h.in(c->io_b, scalars, total * 32);
  void* o = h.out(c->io_out, out, k * 3 * Wire<F>::WORDS * 4);
  if (h.rc) return h.rc;
  return h.finish(msm_segments_device<F>(c, bases, dbf, doff, ds, k, total, o));
}
extern "C" int blsgpu_g1_msm_segments(blsgpu_ctx* c, const blsgpu_bases* b, const uint32_t* bf, const uint32_t* off, const uint8_t* s, size_t k, uint64_t* out) { CTX_CLAIM(c);
  return msm_segments_host<FpPolicy>(c, b, bf, off, s, k, out); }
extern "C" int blsgpu_g2_msm_segments(blsgpu_ctx* c, const blsgpu_bases* b, const uint32_t* bf, const uint32_t* off, const uint8_t* s, size_t k, uint64_t* out) { CTX_CLAIM(c);
  return msm_segments_host<Fp2Policy>(c, b, bf, off, s, k, out); }
extern "C" int blsgpu_g1_msm_segments_device(blsgpu_ctx* c, const blsgpu_bases* b, const void* bf, const void* off, const void* s, size_t k, size_t total, void* out) { CTX_CLAIM(c);
  return msm_segments_device<FpPolicy>(c, b, bf, off, s, k, total, out); }
extern "C" int blsgpu_g2_msm_segments_device(blsgpu_ctx* c, const blsgpu_bases* b, const void* bf, const void* off, const void* s, size_t k, size_t total, void* out) { CTX_CLAIM(c);
  return msm_segments_device<Fp2Policy>(c, b, bf, off, s, k, total, out); }
// Repeated one-shot MSMs over the SAME base array (a drop-in caller that passes its SRS slice on every call: the reference's surface
// has no place for a resident handle).  Opt-in (blsgpu_set_bases_cache): a base array is recognised by its length and a fingerprint of
// 64 evenly spaced points -- the caller promises not to change an array it passes again.  First sight: the one-shot path as always.
// Second sight: the set is uploaded as RESIDENT bases (subgroup test, endomorphism images) and kept; from then on a call only moves its
// scalars, i.e. it runs on the headline path (bases resident, 32 B per scalar over PCIe).
// every word of the array, four host threads (blsgpu_set_bases_cache_verify): ~100 MB at memory speed for 2^20 G1 points
static uint64_t bases_full_hash(const uint64_t* xy, const uint8_t* inf, size_t n, size_t words) {
  constexpr int T = 4;
  uint64_t part[T];
  auto run = [&](int t) {
    const size_t lo = n * (size_t)t / T, hi = n * (size_t)(t + 1) / T;
    uint64_t a = 0x9e3779b97f4a7c15ull ^ (uint64_t)t, b = 0xc2b2ae3d27d4eb4full;
    for (size_t i = lo * words; i < hi * words; i++) { a = (a ^ xy[i]) * 0xff51afd7ed558ccdull; a ^= a >> 29; b += a; }
    if (inf) for (size_t i = lo; i < hi; i++) { b = (b ^ inf[i]) * 0x100000001b3ull; }
    part[t] = a ^ (b * 0x9e3779b97f4a7c15ull);
  };
  std::vector<std::thread> th;
  try { for (int t = 1; t < T; t++) th.emplace_back(run, t); } catch (...) { for (auto& x : th) x.join(); th.clear(); for (int t = 1; t < T; t++) run(t); }
  run(0);
  for (auto& x : th) x.join();
  uint64_t h = 1469598103934665603ull ^ (uint64_t)n;
  for (int t = 0; t < T; t++) { h ^= part[t]; h *= 1099511628211ull; }
  return h;
}
static uint64_t bases_fingerprint(const uint64_t* xy, const uint8_t* inf, size_t n, size_t words) {
  uint64_t h = 1469598103934665603ull ^ (uint64_t)n;
  const size_t step = n > 64 ? n / 64 : 1;
  for (size_t i = 0; i < n; i += step) {
    for (size_t k = 0; k < words; k++) { h ^= xy[i * words + k]; h *= 1099511628211ull; }
    h ^= inf ? inf[i] : 0; h *= 1099511628211ull;
  }
  for (size_t k = 0; k < words && n; k++) { h ^= xy[(n - 1) * words + k]; h *= 1099511628211ull; }
  return h;
}
template <class F>
static int msm_oneshot(blsgpu_ctx* c, const uint64_t* xy, const uint8_t* inf, const uint8_t* s, size_t n, uint64_t* out) {
  if (c && c->bcache_cap > 0 && n >= 1024 && xy) {
    constexpr size_t W = 2 * Wire<F>::WORDS / 2;            // u64 per affine point
    const uint64_t fp = c->bcache_verify ? bases_full_hash(xy, inf, n, W) : bases_fingerprint(xy, inf, n, W);
    blsgpu_ctx::BasesCacheEntry* hit = nullptr;
    for (auto& e : c->bcache) if (e.group == GroupTag<F>::id && e.n == n && e.fp == fp) hit = &e;
    if (hit) {
      hit->last = ++c->bcache_tick;
      if (!hit->b) {                                          // second sight: make it resident
        int rc = bases_upload<F>(c, xy, inf, n, &hit->b, false);
        if (rc) { hit->b = nullptr; return rc; }
      }
      return msm_host<F>(c, hit->b, 0, s, n, out);
    }
    if ((int)c->bcache.size() >= c->bcache_cap) {             // evict the least recently used entry
      size_t lru = 0;
      for (size_t k = 1; k < c->bcache.size(); k++) if (c->bcache[k].last < c->bcache[lru].last) lru = k;
      if (c->bcache[lru].b) blsgpu_bases_free(c->bcache[lru].b);
      c->bcache.erase(c->bcache.begin() + (long)lru);
    }
    c->bcache.push_back({GroupTag<F>::id, n, fp, nullptr, ++c->bcache_tick});
  }
  blsgpu_bases* b = nullptr;
  int rc = bases_upload<F>(c, xy, inf, n, &b, true);
  if (rc) return rc;
  rc = msm_host<F>(c, b, 0, s, n, out);
  blsgpu_bases_free(b);
  return rc;
}
extern "C" int blsgpu_set_bases_cache_verify(blsgpu_ctx* c, int on) { CTX_CLAIM(c);
  if (!c) return bad("ctx is NULL");
  if ((on != 0) != c->bcache_verify) {                 // fingerprints of the two kinds do not compare: start over
    for (auto& e : c->bcache) if (e.b) blsgpu_bases_free(e.b);
    c->bcache.clear();
  }
  c->bcache_verify = on != 0;
  return BLSGPU_OK;
}
extern "C" int blsgpu_set_bases_cache(blsgpu_ctx* c, int entries) { CTX_CLAIM(c);
  if (!c || entries < 0 || entries > 8) return bad("set_bases_cache: entries must be in [0, 8]");
  HIPCHK(hipSetDevice(c->device));
  c->bcache_cap = entries;
  while ((int)c->bcache.size() > entries) { if (c->bcache.back().b) blsgpu_bases_free(c->bcache.back().b); c->bcache.pop_back(); }
  return BLSGPU_OK;
}
extern "C" int blsgpu_g1_msm_host(blsgpu_ctx* c, const uint64_t* xy, const uint8_t* inf, const uint8_t* s, size_t n, uint64_t* out) { CTX_CLAIM(c); return msm_oneshot<FpPolicy>(c, xy, inf, s, n, out); }
extern "C" int blsgpu_g2_msm_host(blsgpu_ctx* c, const uint64_t* xy, const uint8_t* inf, const uint8_t* s, size_t n, uint64_t* out) { CTX_CLAIM(c); return msm_oneshot<Fp2Policy>(c, xy, inf, s, n, out); }

// ---------------------------------------------------------------------------------------------------
// batched variable-base scalar multiplication (mulbatch.hip.h): out[i] = [s_i] P_i, N in -> N out
// ---------------------------------------------------------------------------------------------------
static int mul_batch_check(blsgpu_ctx* c, const void* xy, const void* scalars, size_t n, const void* out) { return (!c || (n && (!xy || !scalars || !out))) ? bad("mul_batch: NULL argument") : BLSGPU_OK; }
template <class F>
static int mul_batch_device(blsgpu_ctx* c, const void* d_xy, const void* d_inf, const void* d_scalars, size_t n, void* d_out) {
  if (int rc = mul_batch_check(c, d_xy, d_scalars, n, d_out)) return rc;
  if (!n) return BLSGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  if constexpr (MbIO<F>::LANES == 1) {
    // G1 points the caller vouches for (blsgpu_set_assume_subgroup): the endomorphism split halves the doublings, as in the MSM
    if (c->assume_subgroup && !c->no_glv) {
      KLAUNCH(k_mul_batch_glv, dim3(nblk(n, 256)), dim3(256), 0, c->stream, (const u32*)d_xy, (const uint8_t*)d_inf, (const u32*)d_scalars, (u32*)d_out, n, c->status_word, c->scalar_form);
      LAUNCHCHK();
      return BLSGPU_OK;
    }
  }
  if constexpr (MbIO<F>::LANES == 2) {
    if (c->assume_subgroup && !c->no_glv) {         // G2 points the caller vouches for: the four-dimensional psi split
      KLAUNCH(k_mul_batch_gls, dim3(nblk(n * 2, 256)), dim3(256), 0, c->stream, (const u32*)d_xy, (const uint8_t*)d_inf, (const u32*)d_scalars, (u32*)d_out, n, c->status_word, c->scalar_form);
      LAUNCHCHK();
      return BLSGPU_OK;
    }
  }
  KLAUNCH(k_mul_batch<F>, dim3(nblk(n * MbIO<F>::LANES, 256)), dim3(256), 0, c->stream, (const u32*)d_xy, (const uint8_t*)d_inf, (const u32*)d_scalars,
                     (u32*)d_out, n, c->status_word, c->scalar_form);
  LAUNCHCHK();
  return BLSGPU_OK;
}
template <class F>
static int mul_batch_host(blsgpu_ctx* c, const uint64_t* xy, const uint8_t* inf, const uint8_t* scalars, size_t n, uint64_t* out) {
  if (int rc = mul_batch_check(c, xy, scalars, n, out)) return rc;
  if (!n) return BLSGPU_OK;
  constexpr size_t WB = MbIO<F>::WW * 4;
  HostCall h(c);
  h.report_status();
  void* dxy = h.in(c->io_a, xy, n * 2 * WB);
  void* ds = h.in(c->io_b, scalars, n * 32);
  void* dinf = h.in(c->flags_a, inf, n);
  void* o = h.out(c->io_out, out, n * 3 * WB);
  if (h.rc) return h.rc;
  return h.finish(mul_batch_device<F>(c, dxy, dinf, ds, n, o));
}
extern "C" int blsgpu_g1_mul_batch(blsgpu_ctx* c, const uint64_t* xy, const uint8_t* inf, const uint8_t* s, size_t n, uint64_t* out) { CTX_CLAIM(c); return mul_batch_host<FpPolicy>(c, xy, inf, s, n, out); }
extern "C" int blsgpu_g2_mul_batch(blsgpu_ctx* c, const uint64_t* xy, const uint8_t* inf, const uint8_t* s, size_t n, uint64_t* out) { CTX_CLAIM(c); return mul_batch_host<Fp2PairPolicy>(c, xy, inf, s, n, out); }
extern "C" int blsgpu_g1_mul_batch_device(blsgpu_ctx* c, const void* xy, const void* inf, const void* s, size_t n, void* out) { CTX_CLAIM(c); return mul_batch_device<FpPolicy>(c, xy, inf, s, n, out); }
extern "C" int blsgpu_g2_mul_batch_device(blsgpu_ctx* c, const void* xy, const void* inf, const void* s, size_t n, void* out) { CTX_CLAIM(c); return mul_batch_device<Fp2PairPolicy>(c, xy, inf, s, n, out); }
// `&G1Affine * &Scalar` over slices with the scalars as Montgomery limbs (g1.rs:556-594 calls `Scalar::to_bytes` per product)
extern "C" int blsgpu_g1_mul_batch_mont(blsgpu_ctx* c, const uint64_t* xy, const uint8_t* inf, const uint64_t* s, size_t n, uint64_t* out) { CTX_CLAIM(c);
  ScalarFormScope f(c, SCALAR_MONT); return mul_batch_host<FpPolicy>(c, xy, inf, (const uint8_t*)s, n, out); }
extern "C" int blsgpu_g2_mul_batch_mont(blsgpu_ctx* c, const uint64_t* xy, const uint8_t* inf, const uint64_t* s, size_t n, uint64_t* out) { CTX_CLAIM(c);
  ScalarFormScope f(c, SCALAR_MONT); return mul_batch_host<Fp2PairPolicy>(c, xy, inf, (const uint8_t*)s, n, out); }
extern "C" int blsgpu_g1_mul_batch_mont_device(blsgpu_ctx* c, const void* xy, const void* inf, const void* s, size_t n, void* out) { CTX_CLAIM(c);
  ScalarFormScope f(c, SCALAR_MONT); return mul_batch_device<FpPolicy>(c, xy, inf, s, n, out); }
extern "C" int blsgpu_g2_mul_batch_mont_device(blsgpu_ctx* c, const void* xy, const void* inf, const void* s, size_t n, void* out) { CTX_CLAIM(c);
  ScalarFormScope f(c, SCALAR_MONT); return mul_batch_device<Fp2PairPolicy>(c, xy, inf, s, n, out); }

// ---------------------------------------------------------------------------------------------------
// group transforms (gntt.hip.h; gntt_plan.h decides the launches): k vectors of 2^log_n projective wire points, in place
// ---------------------------------------------------------------------------------------------------
// every argument check of both forms: before any staging, reservation or launch
static int g_ntt_check(blsgpu_ctx* c, const void* xyz, int log_n, size_t k, bool device) {
  if (!c || (k && !xyz)) return bad("g_ntt_many: NULL argument");
  if (log_n < 0 || log_n > GNTT_MAX_LOG) return bad("g_ntt_many: log_n must be in [0, 24]");
  if (k > (((size_t)1 << GNTT_MAX_LOG) >> log_n)) return bad("g_ntt_many: k * 2^log_n must not exceed 2^24");
  if (device && ((uintptr_t)xyz & 15)) return bad("g_ntt_many_device: d_xyz must be 16-byte aligned");
  return BLSGPU_OK;
}
template <class LaneS, class TeamS>
static int g_ntt_many_device(blsgpu_ctx* c, void* d_xyz, int log_n, size_t k, int inverse) {
  if (int rc = g_ntt_check(c, d_xyz, log_n, k, true)) return rc;
  const GnPlan plan = gntt_plan_many(LaneS::GROUP, log_n, k, c->diag.gntt_team_max);
  if (!plan.n_steps) return BLSGPU_OK;                 // k == 0 or log_n == 0: nothing to set up either
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const int dir = inverse ? 1 : 0;
  // the tables are the Fr transform's own (api_fr.hip), cached per (log_n, direction); the points are transformed in place, so the
  // call shares no scratch with an MSM in flight
  if (c->fr_tw[dir].reserve(((size_t)1 << log_n) * 32) || c->fr_ninv.reserve(64)) { g_err = "hipMalloc(fr scratch) failed"; return BLSGPU_ERR_HIP; }
  if (int rc = fr_twiddles_ready(c, log_n, dir)) return rc;
  const u32* ninv = nullptr;
  if (inverse) {
    if (int rc = fr_ninv_ready(c, log_n)) return rc;
    ninv = c->fr_ninv.as<u32>();
  }
  const u32* tw = c->fr_tw[dir].as<u32>();
  u32* x = (u32*)d_xyz;
  for (int i = 0; i < plan.n_steps; i++) {
    const GnStep& s = plan.step[i];
    if (s.kernel == GN_K_PERMUTE) KLAUNCH(k_gntt_permute<LaneS::IO::WW>, dim3(s.grid), dim3(s.block), s.lds, st, x, log_n, plan.total);
    else if (s.shape == GN_TEAM) KLAUNCH(k_gntt_stage<TeamS>, dim3(s.grid), dim3(s.block), s.lds, st, x, tw, s.stage ? nullptr : ninv, s.stage, plan.butterflies);
    else KLAUNCH(k_gntt_stage<LaneS>, dim3(s.grid), dim3(s.block), s.lds, st, x, tw, s.stage ? nullptr : ninv, s.stage, plan.butterflies);
  }
  LAUNCHCHK();
  return BLSGPU_OK;
}
template <class LaneS, class TeamS>
static int g_ntt_many_host(blsgpu_ctx* c, uint64_t* xyz, int log_n, size_t k, int inverse) {
  if (int rc = g_ntt_check(c, xyz, log_n, k, false)) return rc;
  if (!k) return BLSGPU_OK;
  HostCall h(c);
  void* d = h.inout(c->io_a, xyz, (k << log_n) * 3 * LaneS::IO::WW * 4);
  if (h.rc) return h.rc;
  return h.finish(g_ntt_many_device<LaneS, TeamS>(c, d, log_n, k, inverse));
}
extern "C" int blsgpu_g1_ntt_many(blsgpu_ctx* c, uint64_t* xyz, int log_n, size_t k, int inverse) { CTX_CLAIM(c); return g_ntt_many_host<GnG1Lane, GnG1Team>(c, xyz, log_n, k, inverse); }
extern "C" int blsgpu_g2_ntt_many(blsgpu_ctx* c, uint64_t* xyz, int log_n, size_t k, int inverse) { CTX_CLAIM(c); return g_ntt_many_host<GnG2Lane, GnG2Team>(c, xyz, log_n, k, inverse); }
extern "C" int blsgpu_g1_ntt_many_device(blsgpu_ctx* c, void* d_xyz, int log_n, size_t k, int inverse) { CTX_CLAIM(c); return g_ntt_many_device<GnG1Lane, GnG1Team>(c, d_xyz, log_n, k, inverse); }
extern "C" int blsgpu_g2_ntt_many_device(blsgpu_ctx* c, void* d_xyz, int log_n, size_t k, int inverse) { CTX_CLAIM(c); return g_ntt_many_device<GnG2Lane, GnG2Team>(c, d_xyz, log_n, k, inverse); }

// ---------------------------------------------------------------------------------------------------
// group helpers
// ---------------------------------------------------------------------------------------------------
// device-pointer variant: wire-format partials in device memory -> wire-format sum in device memory, asynchronous
static int sum_check(const char* msg, blsgpu_ctx* c, const void* xyz, size_t n, const void* out) { return (!c || !out || (n && !xyz)) ? bad(msg) : BLSGPU_OK; }
template <class F>
static int proj_sum_device(blsgpu_ctx* c, const void* d_xyz, size_t n, void* d_out) {
  if (int rc = sum_check("sum_device: NULL argument", c, d_xyz, n, d_out)) return rc;
  HIPCHK(hipSetDevice(c->device));
  constexpr int PW = Store<F>::PROJ_WORDS;
  // (a fold queued on the fold stream must not share scratch with calls on the main stream: nothing orders the two)
  DevBuf& recs = c->on_fold_stream ? c->fold_c : c->io_c;
  DevBuf& res = c->on_fold_stream ? c->fold_result : c->result;
  if (recs.reserve((n ? n : 1) * PW * 4) || res.reserve(PW * 4)) { g_err = "hipMalloc failed"; return BLSGPU_ERR_HIP; }
  if (n) KLAUNCH(k_proj_import<F>, dim3(nblk(n, 256)), dim3(256), 0, c->stream, (const u32*)d_xyz, recs.as<u32>(), n);
  KLAUNCH(k_proj_sum_team<F>, dim3(1), dim3(TEAM), TEAM_LDS(TEAM), c->stream, recs.as<u32>(), res.as<u32>(), n);
  KLAUNCH(k_proj_export<F>, dim3(1), dim3(256), 0, c->stream, res.as<u32>(), (u32*)d_out, (size_t)1);
  LAUNCHCHK();
  return BLSGPU_OK;
}
template <class F>
static int proj_sum(blsgpu_ctx* c, const uint64_t* xyz, size_t n, uint64_t* out) {
  if (int rc = sum_check("sum: NULL argument", c, xyz, n, out)) return rc;
  constexpr int WW = Wire<F>::WORDS;
  HostCall h(c);
  void* dxyz = h.in(c->io_a, xyz, n * 3 * WW * 4);
  void* o = h.out(c->io_out, out, 3 * WW * 4);
  if (h.rc) return h.rc;
  return h.finish(proj_sum_device<F>(c, dxyz, n, o));
}
extern "C" int blsgpu_g1_sum_device(blsgpu_ctx* c, const void* xyz, size_t n, void* out) { CTX_CLAIM(c); return proj_sum_device<FpPolicy>(c, xyz, n, out); }
extern "C" int blsgpu_g2_sum_device(blsgpu_ctx* c, const void* xyz, size_t n, void* out) { CTX_CLAIM(c); return proj_sum_device<Fp2Policy>(c, xyz, n, out); }
extern "C" int blsgpu_g1_sum(blsgpu_ctx* c, const uint64_t* xyz, size_t n, uint64_t* out) { CTX_CLAIM(c); return proj_sum<FpPolicy>(c, xyz, n, out); }
extern "C" int blsgpu_g2_sum(blsgpu_ctx* c, const uint64_t* xyz, size_t n, uint64_t* out) { CTX_CLAIM(c); return proj_sum<Fp2Policy>(c, xyz, n, out); }

// segmented, gathered sums (gsum.hip.h): the launches of gsum_plan.h on the context's stream, asynchronous
template <class F>
static int sum_segments_device(blsgpu_ctx* c, const void* d_xy, const void* d_inf, size_t npoints, const void* d_idx, const void* d_offsets, size_t nseg, size_t total,
                               void* d_out) {
  if (!c) return bad("sum_segments: ctx is NULL");
  GsumArgs a;
  a.group = GroupTag<F>::id; a.xy = d_xy; a.inf = d_inf; a.npoints = npoints; a.idx = d_idx; a.offsets = d_offsets; a.nseg = nseg; a.total = total; a.out = d_out; a.device = true;
  if (const char* why = gsum_check(a)) return bad(why);
  if (!nseg) return BLSGPU_OK;
  const GsumPlan plan = gsum_plan(a.group, nseg, total);
  if (!plan.ok) return bad("sum_segments: the sizes are out of range");
  HIPCHK(hipSetDevice(c->device));
  if (c->gsum_part.reserve(plan.part_bytes + 16) || c->gsum_meta.reserve(plan.meta_bytes + 16)) { g_err = "hipMalloc failed"; return BLSGPU_ERR_HIP; }
  const unsigned long long* off = (const unsigned long long*)d_offsets;
  if (plan.chunks_grid)
    KLAUNCH(k_gsum_chunks<F>, dim3(plan.chunks_grid), dim3(plan.block), plan.lds, c->stream, (const u32*)d_xy, (const uint8_t*)d_inf, (u32)npoints, (const u32*)d_idx, off,
            (u32)nseg, (u32)total, plan.terms, (u32*)d_out, c->gsum_part.as<u32>(), c->gsum_meta.as<u32>(), c->status_word);
  KLAUNCH(k_gsum_combine<F>, dim3(plan.combine_grid), dim3(plan.block), plan.lds, c->stream, off, (u32)nseg, (u32)total, plan.chunk, plan.nchunks,
          (const u32*)c->gsum_part.as<u32>(), (const u32*)c->gsum_meta.as<u32>(), (u32*)d_out);
  LAUNCHCHK();
  return BLSGPU_OK;
}
template <class F>
static int sum_segments(blsgpu_ctx* c, const uint64_t* xy, const uint8_t* inf, size_t npoints, const uint32_t* idx, const uint64_t* offsets, size_t nseg, size_t total,
                        uint64_t* out) {
  if (!c) return bad("sum_segments: ctx is NULL");
  GsumArgs a;
  a.group = GroupTag<F>::id; a.xy = xy; a.inf = inf; a.npoints = npoints; a.idx = idx; a.offsets = offsets; a.nseg = nseg; a.total = total; a.out = out;
  if (const char* why = gsum_check(a)) return bad(why);
  if (const char* why = gsum_check_host(offsets, nseg, total, idx, npoints)) return bad(why);
  if (!nseg) return BLSGPU_OK;
  constexpr int WW = Wire<F>::WORDS;
  HostCall h(c);
  // (without idx only the first `total` points can be named)
  const size_t used = total ? (idx ? npoints : total) : 0;
  void* dxy = h.in(c->io_a, xy, used * 2 * WW * 4);
  void* dinf = h.in(c->flags_a, inf, used);
  void* didx = total ? h.in(c->io_b, idx, total * 4) : nullptr;
  void* doff = h.in(c->io_e, offsets, (nseg + 1) * 8);
  void* o = h.out(c->io_out, out, nseg * 3 * WW * 4);
  if (h.rc) return h.rc;
  return h.finish(sum_segments_device<F>(c, dxy, dinf, used, didx, doff, nseg, total, o));
}
extern "C" int blsgpu_g1_sum_segments_device(blsgpu_ctx* c, const void* xy, const void* inf, size_t npoints, const void* idx, const void* offsets, size_t nseg, size_t total,
                                             void* out) { CTX_CLAIM(c); return sum_segments_device<FpPolicy>(c, xy, inf, npoints, idx, offsets, nseg, total, out); }
extern "C" int blsgpu_g2_sum_segments_device(blsgpu_ctx* c, const void* xy, const void* inf, size_t npoints, const void* idx, const void* offsets, size_t nseg, size_t total,
                                             void* out) { CTX_CLAIM(c); return sum_segments_device<Fp2Policy>(c, xy, inf, npoints, idx, offsets, nseg, total, out); }
extern "C" int blsgpu_g1_sum_segments(blsgpu_ctx* c, const uint64_t* xy, const uint8_t* inf, size_t npoints, const uint32_t* idx, const uint64_t* offsets, size_t nseg,
                                      size_t total, uint64_t* out) { CTX_CLAIM(c); return sum_segments<FpPolicy>(c, xy, inf, npoints, idx, offsets, nseg, total, out); }
extern "C" int blsgpu_g2_sum_segments(blsgpu_ctx* c, const uint64_t* xy, const uint8_t* inf, size_t npoints, const uint32_t* idx, const uint64_t* offsets, size_t nseg,
                                      size_t total, uint64_t* out) { CTX_CLAIM(c); return sum_segments<Fp2Policy>(c, xy, inf, npoints, idx, offsets, nseg, total, out); }

// interpolation in the exponent: out[s] = sum_i lambda_i P_i over segment s, lambda the Lagrange coefficients of the segment's nodes at
// its point.  Three stages on the context's stream, no synchronisation: the coefficients into scratch (fr_lagrange.hip.h, launched by
// api_fr.hip), the products lambda_i P_i (mulbatch.hip.h: exact for every curve point, the endomorphism split only under
// assume_subgroup), the segment sums (lagrange_combine.hip.h).  F: the group; FM: the policy mul_batch runs it under.
template <class F, class FM>
static int lagrange_combine_device(blsgpu_ctx* c, const void* d_xy, const void* d_inf, const void* d_nodes, const void* d_offsets, size_t nseg, size_t total, const void* d_points,
                                   void* d_out, void* d_flags) {
  if (!c) return bad("lagrange_combine: ctx is NULL");
  FlgcArgs a;
  a.group = GroupTag<F>::id; a.xy = d_xy; a.inf = d_inf; a.nodes = d_nodes; a.offsets = d_offsets; a.nseg = nseg; a.total = total; a.points = d_points; a.out = d_out;
  a.flags = d_flags; a.device = true;
  if (const char* why = flgc_check(a)) return bad(why);
  if (!nseg) return BLSGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  constexpr int WW = Wire<F>::WORDS, PW = Store<F>::PROJ_WORDS;
  if (c->flg_lambda.reserve(total * 32 + 16) || c->flg_prod.reserve(total * 3 * WW * 4 + 16)) { g_err = "hipMalloc(lagrange_combine scratch) failed"; return BLSGPU_ERR_HIP; }
  // a segment that breaks the offsets contract writes no coefficient: its shares, and those no segment covers, are multiplied by 0
  if (total) HIPCHK(hipMemsetAsync(c->flg_lambda.p, 0, total * 32, c->stream));
  if (int rc = fr_lagrange_launch(c, d_nodes, d_offsets, nseg, total, d_points, nullptr, c->flg_lambda.p, nullptr, d_flags)) return rc;
  {
    ScalarFormScope mont(c, SCALAR_MONT);               // the coefficients are Montgomery limbs whatever the context's setting
    if (int rc = mul_batch_device<FM>(c, d_xy, d_inf, c->flg_lambda.p, total, c->flg_prod.p)) return rc;
  }
  const unsigned block = flgc_block(a.group, nseg, total);
  KLAUNCH(k_flg_point_sums<F>, dim3((unsigned)nseg), dim3(block), (size_t)block * PW * 4, c->stream, (const u32*)c->flg_prod.as<u32>(), (const u32*)d_offsets, (u32)nseg, (u32)total,
          (u32*)d_out);
  LAUNCHCHK();
  return BLSGPU_OK;
}
template <class F, class FM>
static int lagrange_combine(blsgpu_ctx* c, const uint64_t* xy, const uint8_t* inf, const uint64_t* nodes, const uint32_t* offsets, size_t nseg, const uint64_t* points,
                            uint64_t* out, uint8_t* flags) {
  if (!c) return bad("lagrange_combine: ctx is NULL");
  if (nseg > FLG_MAX_SEGS) return bad("fr_lagrange_segments: nseg must not exceed 2^27");
  if (nseg && !offsets) return bad("fr_lagrange_segments: NULL offsets with segments to do");
  const size_t total = nseg ? offsets[nseg] : 0;
  FlgcArgs a;
  a.group = GroupTag<F>::id; a.xy = xy; a.inf = inf; a.nodes = nodes; a.offsets = offsets; a.nseg = nseg; a.total = total; a.points = points; a.out = out; a.flags = flags;
  if (const char* why = flgc_check(a)) return bad(why);
  if (const char* why = flg_check_host(offsets, nseg, total)) return bad(why);
  if (!nseg) return BLSGPU_OK;
  constexpr int WW = Wire<F>::WORDS;
  HostCall h(c);
  h.report_status();
  void* dxy = h.in(c->io_a, xy, total * 2 * WW * 4);
  void* dinf = h.in(c->flags_a, inf, total);
  void* dn = h.in(c->io_b, nodes, total * 32);
  void* doff = h.in(c->io_e, offsets, (nseg + 1) * 4);
  void* dp = h.in(c->io_f, points, nseg * 32);
  void* o = h.out(c->io_out, out, nseg * 3 * WW * 4);
  void* f = flags ? h.out(c->flags_b, flags, nseg) : nullptr;
  if (h.rc) return h.rc;
  return h.finish(lagrange_combine_device<F, FM>(c, dxy, dinf, dn, doff, nseg, total, dp, o, f));
}
extern "C" int blsgpu_g1_lagrange_combine_device(blsgpu_ctx* c, const void* xy, const void* inf, const void* nodes, const void* offsets, size_t nseg, size_t total,
                                                 const void* points, void* out, void* flags) { CTX_CLAIM(c);
  return lagrange_combine_device<FpPolicy, FpPolicy>(c, xy, inf, nodes, offsets, nseg, total, points, out, flags); }
extern "C" int blsgpu_g2_lagrange_combine_device(blsgpu_ctx* c, const void* xy, const void* inf, const void* nodes, const void* offsets, size_t nseg, size_t total,
                                                 const void* points, void* out, void* flags) { CTX_CLAIM(c);
  return lagrange_combine_device<Fp2Policy, Fp2PairPolicy>(c, xy, inf, nodes, offsets, nseg, total, points, out, flags); }
extern "C" int blsgpu_g1_lagrange_combine(blsgpu_ctx* c, const uint64_t* xy, const uint8_t* inf, const uint64_t* nodes, const uint32_t* offsets, size_t nseg,
                                          const uint64_t* points, uint64_t* out, uint8_t* flags) { CTX_CLAIM(c);
  return lagrange_combine<FpPolicy, FpPolicy>(c, xy, inf, nodes, offsets, nseg, points, out, flags); }
extern "C" int blsgpu_g2_lagrange_combine(blsgpu_ctx* c, const uint64_t* xy, const uint8_t* inf, const uint64_t* nodes, const uint32_t* offsets, size_t nseg,
                                          const uint64_t* points, uint64_t* out, uint8_t* flags) { CTX_CLAIM(c);
  return lagrange_combine<Fp2Policy, Fp2PairPolicy>(c, xy, inf, nodes, offsets, nseg, points, out, flags); }

// device core: projective wire records in device memory -> affine wire coordinates + infinity bytes in device memory (asynchronous)
// (the host forms take no infinity array when the caller does not want one: inf_ok = true)
static int normalize_check(blsgpu_ctx* c, const void* xyz, size_t n, const void* xy, bool inf_ok) { return (!c || (n && (!xyz || !xy || !inf_ok))) ? bad("batch_normalize: NULL argument") : BLSGPU_OK; }
template <class F>
static int batch_normalize_device(blsgpu_ctx* c, const void* d_xyz, size_t n, void* d_xy, void* d_inf) {
  if (int rc = normalize_check(c, d_xyz, n, d_xy, d_inf != nullptr)) return rc;
  if (!n) return BLSGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  constexpr int PW = Store<F>::PROJ_WORDS;
  if (c->io_c.reserve(n * PW * 4) || c->io_d.reserve(n * Store<F>::EL * 4)) { g_err = "hipMalloc failed"; return BLSGPU_ERR_HIP; }
  KLAUNCH(k_proj_import<F>, dim3(nblk(n, 256)), dim3(256), 0, c->stream, (const u32*)d_xyz, c->io_c.as<u32>(), n);
  if (n >= 4096) {
    const int K = normalize_k(n);
    size_t T = (n + K - 1) / K;
    KLAUNCH(k_batch_normalize<F>, dim3(nblk(T, 256)), dim3(256), 0, c->stream, c->io_c.as<u32>(), c->io_d.as<u32>(), (u32*)d_xy, (uint8_t*)d_inf, n, T, K);
  } else {
    KLAUNCH(k_proj_to_affine<F>, dim3(nblk(n, 256)), dim3(256), 0, c->stream, c->io_c.as<u32>(), (u32*)d_xy, (uint8_t*)d_inf, n);
  }
  LAUNCHCHK();
  return BLSGPU_OK;
}
template <class F>
static int batch_normalize(blsgpu_ctx* c, const uint64_t* xyz, size_t n, uint64_t* xy, uint8_t* inf) {
  if (int rc = normalize_check(c, xyz, n, xy, true)) return rc;
  if (!n) return BLSGPU_OK;
  constexpr int WW = Wire<F>::WORDS;
  HostCall h(c);
  void* dxyz = h.in(c->io_a, xyz, n * 3 * WW * 4);
  void* dxy = h.out(c->io_out, xy, n * 2 * WW * 4);
  void* dinf = h.out(c->flags_b, inf, n);
  if (h.rc) return h.rc;
  return h.finish(batch_normalize_device<F>(c, dxyz, n, dxy, dinf));
}
extern "C" int blsgpu_g1_batch_normalize_device(blsgpu_ctx* c, const void* xyz, size_t n, void* xy, void* inf) { CTX_CLAIM(c); return batch_normalize_device<FpPolicy>(c, xyz, n, xy, inf); }
extern "C" int blsgpu_g2_batch_normalize_device(blsgpu_ctx* c, const void* xyz, size_t n, void* xy, void* inf) { CTX_CLAIM(c); return batch_normalize_device<Fp2Policy>(c, xyz, n, xy, inf); }
extern "C" int blsgpu_g1_batch_normalize(blsgpu_ctx* c, const uint64_t* xyz, size_t n, uint64_t* xy, uint8_t* inf) { CTX_CLAIM(c); return batch_normalize<FpPolicy>(c, xyz, n, xy, inf); }
extern "C" int blsgpu_g2_batch_normalize(blsgpu_ctx* c, const uint64_t* xyz, size_t n, uint64_t* xy, uint8_t* inf) { CTX_CLAIM(c); return batch_normalize<Fp2Policy>(c, xyz, n, xy, inf); }

// ---------------------------------------------------------------------------------------------------
// amortised KZG openings (kzg.hip.h; kzg_plan.h holds the checks, the index maps and the launch shapes): every cell proof of many
// polynomials by the circulant route -- Fr transforms (api_fr.hip, through the public entry point), ONE segmented MSM over the
// handle's own bases, two group transforms -- and the cells themselves
// ---------------------------------------------------------------------------------------------------
namespace {
struct KzgTmp {                      // device memory of blsgpu_kzg_multiproof_create, freed when the call has synchronised
  void* p[4] = {nullptr, nullptr, nullptr, nullptr};
  ~KzgTmp() { for (void* q : p) if (q) hipFree(q); }
};
}  // namespace
extern "C" int blsgpu_kzg_multiproof_create(blsgpu_ctx* c, const blsgpu_bases* srs, int log_n, int log_l, blsgpu_kzg_multiproof** out) { CTX_CLAIM(c);
  if (!c) return bad("kzg_multiproof_create: ctx is NULL");
  KzgCreateArgs a;
  a.srs_given = srs != nullptr; a.out_given = out != nullptr; a.log_n = log_n; a.log_l = log_l;
  if (srs) { a.srs_group = srs->group; a.srs_len = srs->n; a.srs_subgroup = srs->subgroup; }
  if (const char* why = kzg_check_create(a)) return bad(why);
  if (srs->device != c->device) return bad("kzg_multiproof_create: the SRS lives on another device than the context");
  const KzgCreatePlan plan = kzg_plan_create(log_n, log_l);
  HIPCHK(hipSetDevice(c->device));
  blsgpu_kzg_multiproof* h = new blsgpu_kzg_multiproof();
  h->device = c->device; h->log_n = log_n; h->log_l = log_l;
  if (!plan.msm) { *out = h; return BLSGPU_OK; }                 // c = 1: every proof is the identity, nothing is resident
  KzgTmp tmp;
  if (hipMalloc(&tmp.p[0], plan.xy_bytes) != hipSuccess || hipMalloc(&tmp.p[1], plan.inf_bytes) != hipSuccess || hipMalloc(&tmp.p[2], plan.point_bytes) != hipSuccess ||
      hipMalloc(&tmp.p[3], plan.point_bytes) != hipSuccess) { (void)hipGetLastError(); delete h; g_err = "hipMalloc(kzg_multiproof_create) failed"; return BLSGPU_ERR_HIP; }
  auto run = [&]() -> int {
    if (!srs->ready_seen) {
      if (hipEventQuery(srs->ev_ready) == hipSuccess) srs->ready_seen = true;
      else HIPCHK(hipStreamWaitEvent(c->stream, srs->ev_ready, 0));
    }
    // the prefix in wire form -> S^ [t][j] -> X^ = its l transforms of size 2c -> [m][t] -> affine -> a base set with its images
    if (int rc = bases_export<FpPolicy>(c, srs, 0, plan.n, tmp.p[0], tmp.p[1])) return rc;
    KLAUNCH(k_kzg_srs_rows, dim3(plan.gather_grid), dim3(KZG_BLOCK), 0, c->stream, (const uint4*)tmp.p[0], (const uint8_t*)tmp.p[1], (uint4*)tmp.p[2], plan.log_c, log_l);
    LAUNCHCHK();
    if (int rc = g_ntt_many_device<GnG1Lane, GnG1Team>(c, tmp.p[2], plan.log_c + 1, plan.l, 0)) return rc;
    KLAUNCH(k_kzg_point_permute, dim3(plan.permute_grid), dim3(KZG_BLOCK), 0, c->stream, (const uint4*)tmp.p[2], (uint4*)tmp.p[3], (size_t)1, log_n + 1, 2, plan.log_c, log_l);
    LAUNCHCHK();
    if (int rc = batch_normalize_device<FpPolicy>(c, tmp.p[3], plan.points, tmp.p[0], tmp.p[1])) return rc;
    if (int rc = bases_import<FpPolicy>(c, tmp.p[0], tmp.p[1], plan.points, &h->xhat, false, true)) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));                     // a setup call: the temporaries go, and the handle keeps no reference to the SRS
    return BLSGPU_OK;
  };
  if (int rc = run()) {
    (void)hipStreamSynchronize(c->stream);
    if (h->xhat) bases_drop(h->xhat);
    delete h;
    return rc;
  }
  *out = h;
  return BLSGPU_OK;
}
extern "C" int blsgpu_kzg_multiproof_log_n(const blsgpu_kzg_multiproof* h) { return h ? h->log_n : -1; }
extern "C" int blsgpu_kzg_multiproof_log_l(const blsgpu_kzg_multiproof* h) { return h ? h->log_l : -1; }
extern "C" size_t blsgpu_kzg_multiproof_cells(const blsgpu_kzg_multiproof* h) { return h ? (size_t)2 << (h->log_n - h->log_l) : 0; }
extern "C" void blsgpu_kzg_multiproof_free(blsgpu_kzg_multiproof* h) {
  if (!h) return;
  if (h->xhat) blsgpu_bases_free(h->xhat);                       // waits for the device: an asynchronous call may still be reading the bases
  delete h;
}
// the coefficients of `count` polynomials as the later stages read them: the caller's array (FORM_COEFFS), or a copy in scratch that went
// through the inverse transform (FORM_EVALS: bit-reversed on the way for ORDER_BITREV); the caller's array is never written
static int kzg_coeffs(blsgpu_ctx* c, const void* d_polys, int log_n, size_t count, int form, int order, unsigned copy_grid, size_t coeff_bytes, const uint4** coeffs) {
  *coeffs = (const uint4*)d_polys;
  if (form != KZG_FORM_EVALS) return BLSGPU_OK;
  if (c->kzg_coeff.reserve(coeff_bytes)) { g_err = "hipMalloc(kzg scratch) failed"; return BLSGPU_ERR_HIP; }
  KLAUNCH(k_kzg_scalar_copy, dim3(copy_grid), dim3(KZG_BLOCK), 0, c->stream, (const uint4*)d_polys, c->kzg_coeff.as<uint4>(), count, log_n, log_n, order == KZG_ORDER_BITREV ? 1 : 0);
  LAUNCHCHK();
  if (int rc = blsgpu_fr_ntt_many_device(c, c->kzg_coeff.p, log_n, count, 1, nullptr)) return rc;
  *coeffs = c->kzg_coeff.as<uint4>();
  return BLSGPU_OK;
}
static int kzg_proofs_device(blsgpu_ctx* c, const blsgpu_kzg_multiproof* h, const void* d_polys, size_t count, int form, int order, void* d_out) {
  if (!c) return bad("kzg_multiproof_proofs: ctx is NULL");
  KzgProofsArgs a;
  a.handle_given = h != nullptr; a.polys = d_polys; a.count = count; a.form = form; a.order = order; a.out = d_out; a.device = true;
  if (h) { a.log_n = h->log_n; a.log_l = h->log_l; }
  if (const char* why = kzg_check_proofs(a)) return bad(why);
  if (h->device != c->device) return bad("kzg_multiproof_proofs: the handle lives on another device than the context");
  if (!count) return BLSGPU_OK;
  const KzgPlan p = kzg_plan_proofs(h->log_n, h->log_l, count, form);
  if (!p.ok) return bad("kzg_multiproof_proofs: the plan refuses the shape");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const int log_v = p.log_c + 1;                                 // a polynomial's 2c proofs
  if (!p.msm) {                                                  // c = 1: two identities per polynomial
    KLAUNCH(k_kzg_identity_fill, dim3(p.fill_grid), dim3(KZG_BLOCK), 0, st, (uint4*)d_out, count, log_v, (size_t)0, log_v);
    LAUNCHCHK();
    return BLSGPU_OK;
  }
  if (c->kzg_rows.reserve(p.rows_bytes) || c->kzg_seg.reserve(p.seg_bytes) || c->kzg_pts.reserve(p.point_bytes) || c->kzg_off.reserve(p.offset_bytes + p.base_first_bytes)) {
    g_err = "hipMalloc(kzg scratch) failed"; return BLSGPU_ERR_HIP;
  }
  const uint4* coeffs = nullptr;
  if (int rc = kzg_coeffs(c, d_polys, p.log_n, count, form, order, p.copy_grid, p.coeff_bytes, &coeffs)) return rc;
  uint4 *rows = c->kzg_rows.as<uint4>(), *seg = c->kzg_seg.as<uint4>(), *pts = c->kzg_pts.as<uint4>();
  u32 *off = c->kzg_off.as<u32>(), *bf = off + p.points + 1;
  KLAUNCH(k_kzg_coeff_rows, dim3(p.rows_grid), dim3(KZG_BLOCK), 0, st, coeffs, rows, count, p.log_c, p.log_l);
  LAUNCHCHK();
  if (int rc = blsgpu_fr_ntt_many_device(c, rows, log_v, p.vectors, 0, nullptr)) return rc;
  KLAUNCH(k_kzg_transpose<KZG_TILE>, dim3(p.transpose.grid), dim3(p.transpose.block), 0, st, (const uint4*)rows, seg, count, p.log_l, log_v, 0);
  KLAUNCH(k_kzg_segments, dim3(p.seg_grid), dim3(KZG_BLOCK), 0, st, off, bf, (size_t)p.points, p.log_c, p.log_l);
  LAUNCHCHK();
  {
    ScalarFormScope mont(c, SCALAR_MONT);                        // the transform's output is Montgomery limbs whatever the context's setting
    if (int rc = msm_segments_device<FpPolicy>(c, h->xhat, bf, off, seg, p.points, p.scalars, pts)) return rc;
  }
  if (int rc = g_ntt_many_device<GnG1Lane, GnG1Team>(c, pts, log_v, count, 1)) return rc;
  KLAUNCH(k_kzg_identity_fill, dim3(p.fill_grid), dim3(KZG_BLOCK), 0, st, pts, count, log_v, (size_t)p.c, p.log_c);
  LAUNCHCHK();
  if (int rc = g_ntt_many_device<GnG1Lane, GnG1Team>(c, pts, log_v, count, 0)) return rc;
  KLAUNCH(k_kzg_point_permute, dim3(p.permute_grid), dim3(KZG_BLOCK), 0, st, (const uint4*)pts, (uint4*)d_out, count, log_v, order == KZG_ORDER_BITREV ? 1 : 0, p.log_c, p.log_l);
  LAUNCHCHK();
  return BLSGPU_OK;
}
static int kzg_cells_device(blsgpu_ctx* c, const void* d_polys, int log_n, int log_l, size_t count, int form, int order, void* d_cells) {
  if (!c) return bad("kzg_cells: ctx is NULL");
  KzgCellsArgs a;
  a.polys = d_polys; a.log_n = log_n; a.log_l = log_l; a.count = count; a.form = form; a.order = order; a.cells = d_cells; a.device = true;
  if (const char* why = kzg_check_cells(a)) return bad(why);
  if (!count) return BLSGPU_OK;
  const KzgCellsPlan p = kzg_plan_cells(log_n, log_l, count, form);
  if (!p.ok) return bad("kzg_cells: the plan refuses the shape");
  HIPCHK(hipSetDevice(c->device));
  if (c->kzg_rows.reserve(p.ext_bytes)) { g_err = "hipMalloc(kzg scratch) failed"; return BLSGPU_ERR_HIP; }
  const uint4* coeffs = nullptr;
  if (int rc = kzg_coeffs(c, d_polys, log_n, count, form, order, p.copy_grid, p.coeff_bytes, &coeffs)) return rc;
  uint4* ext = c->kzg_rows.as<uint4>();
  KLAUNCH(k_kzg_scalar_copy, dim3(p.extend_grid), dim3(KZG_BLOCK), 0, c->stream, coeffs, ext, count, log_n, log_n + 1, 0);
  LAUNCHCHK();
  if (int rc = blsgpu_fr_ntt_many_device(c, ext, log_n + 1, count, 0, nullptr)) return rc;
  KLAUNCH(k_kzg_transpose<KZG_TILE>, dim3(p.map.grid), dim3(p.map.block), 0, c->stream, (const uint4*)ext, (uint4*)d_cells, count, log_l, p.log_c + 1, order == KZG_ORDER_BITREV ? 1 : 0);
  LAUNCHCHK();
  return BLSGPU_OK;
}
extern "C" int blsgpu_kzg_multiproof_proofs_device(blsgpu_ctx* c, const blsgpu_kzg_multiproof* h, const void* polys, size_t count, int form, int order, void* out) { CTX_CLAIM(c);
  return kzg_proofs_device(c, h, polys, count, form, order, out); }
extern "C" int blsgpu_kzg_cells_device(blsgpu_ctx* c, const void* polys, int log_n, int log_l, size_t count, int form, int order, void* cells) { CTX_CLAIM(c);
  return kzg_cells_device(c, polys, log_n, log_l, count, form, order, cells); }
extern "C" int blsgpu_kzg_multiproof_proofs(blsgpu_ctx* c, const blsgpu_kzg_multiproof* hd, const uint64_t* polys, size_t count, int form, int order, uint64_t* out) { CTX_CLAIM(c);
  if (!c) return bad("kzg_multiproof_proofs: ctx is NULL");
  KzgProofsArgs a;
  a.handle_given = hd != nullptr; a.polys = polys; a.count = count; a.form = form; a.order = order; a.out = out;
  if (hd) { a.log_n = hd->log_n; a.log_l = hd->log_l; }
  if (const char* why = kzg_check_proofs(a)) return bad(why);
  if (!count) return BLSGPU_OK;
  HostCall h(c);
  h.report_status();
  void* dp = h.in(c->io_a, polys, (count << hd->log_n) * 32);
  void* o = h.out(c->io_out, out, (count << (hd->log_n - hd->log_l + 1)) * 144);
  if (h.rc) return h.rc;
  return h.finish(kzg_proofs_device(c, hd, dp, count, form, order, o));
}
extern "C" int blsgpu_kzg_cells(blsgpu_ctx* c, const uint64_t* polys, int log_n, int log_l, size_t count, int form, int order, uint64_t* cells) { CTX_CLAIM(c);
  if (!c) return bad("kzg_cells: ctx is NULL");
  KzgCellsArgs a;
  a.polys = polys; a.log_n = log_n; a.log_l = log_l; a.count = count; a.form = form; a.order = order; a.cells = cells;
  if (const char* why = kzg_check_cells(a)) return bad(why);
  if (!count) return BLSGPU_OK;
  HostCall h(c);
  void* dp = h.in(c->io_a, polys, (count << log_n) * 32);
  void* o = h.out(c->io_out, cells, (count << (log_n + 1)) * 32);
  if (h.rc) return h.rc;
  return h.finish(kzg_cells_device(c, dp, log_n, log_l, count, form, order, o));
}

// ---------------------------------------------------------------------------------------------------
// batched KZG cell-proof verification (kzg_verify.hip.h; kzg_verify_plan.h holds the checks, the maps, the fold's cut and the scratch
// layout): a random linear combination of all cells of a batch, decided by ONE two-term pairing product.  The chain joins the entry
// points that exist on the context's stream, as blsgpu_bls_verify_batch does for signatures; it never synchronises.
// ---------------------------------------------------------------------------------------------------
static void kzgv_drop(blsgpu_kzg_cell_verifier* h) {
  if (h->s) bases_drop(h->s);
  if (h->table) blsgpu_g2_prepared_free(h->table);
  if (h->roots) hipFree(h->roots);
  delete h;
}
extern "C" int blsgpu_kzg_cell_verifier_create(blsgpu_ctx* c, const blsgpu_bases* srs, int log_n, int log_l, const uint64_t* q_xy, const uint8_t* q_inf,
                                               blsgpu_kzg_cell_verifier** out) { CTX_CLAIM(c);
  if (!c) return bad("kzg_cell_verifier_create: ctx is NULL");
  KzgvCreateArgs a;
  a.srs_given = srs != nullptr; a.q_given = q_xy != nullptr; a.out_given = out != nullptr; a.log_n = log_n; a.log_l = log_l;
  if (srs) { a.srs_group = srs->group; a.srs_len = srs->n; a.srs_subgroup = srs->subgroup; }
  if (const char* why = kzgv_check_create(a)) return bad(why);
  if (srs->device != c->device) return bad("kzg_cell_verifier_create: the SRS lives on another device than the context");
  HIPCHK(hipSetDevice(c->device));
  const size_t l = (size_t)1 << log_l;
  blsgpu_kzg_cell_verifier* h = new blsgpu_kzg_cell_verifier();
  h->device = c->device; h->log_n = log_n; h->log_l = log_l;
  KzgTmp tmp;                                                    // S[0..l) in wire form with its flags; the two G2 points with theirs
  if (hipMalloc(&tmp.p[0], l * 96) != hipSuccess || hipMalloc(&tmp.p[1], l) != hipSuccess || hipMalloc(&tmp.p[2], 2 * 192) != hipSuccess || hipMalloc(&tmp.p[3], 16) != hipSuccess ||
      hipMalloc((void**)&h->roots, (size_t)(log_n + 1) * 32) != hipSuccess) {
    (void)hipGetLastError(); kzgv_drop(h); g_err = "hipMalloc(kzg_cell_verifier_create) failed"; return BLSGPU_ERR_HIP;
  }
  auto run = [&]() -> int {
    if (!srs->ready_seen) {
      if (hipEventQuery(srs->ev_ready) == hipSuccess) srs->ready_seen = true;
      else HIPCHK(hipStreamWaitEvent(c->stream, srs->ev_ready, 0));
    }
    if (int rc = bases_export<FpPolicy>(c, srs, 0, l, tmp.p[0], tmp.p[1])) return rc;
    // (a tested or vouched-for SRS needs no second subgroup test; an untested one -- state 3 -- gets the import's own)
    if (int rc = bases_import<FpPolicy>(c, tmp.p[0], tmp.p[1], l, &h->s, false, srs->subgroup == 1 || srs->subgroup == 2)) return rc;
    if (h->s->subgroup == 0) return bad("kzg_cell_verifier_create: the SRS holds a point outside the prime-order subgroup");
    HIPCHK(hipMemcpyAsync(tmp.p[2], q_xy, 192, hipMemcpyHostToDevice, c->stream));
    KLAUNCH(k_kzgv_table_points, dim3(1), dim3(64), 0, c->stream, (u32*)tmp.p[2], (uint8_t*)tmp.p[3], (q_inf && *q_inf) ? 1 : 0);
    KLAUNCH(k_kzgv_roots, dim3(1), dim3(64), 0, c->stream, h->roots, log_n);
    LAUNCHCHK();
    if (int rc = blsgpu_g2_prepare_device(c, tmp.p[2], tmp.p[3], 2, &h->table)) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));                     // a setup call: the temporaries go, and the handle keeps no reference to the SRS
    return BLSGPU_OK;
  };
  if (int rc = run()) {
    (void)hipStreamSynchronize(c->stream);
    kzgv_drop(h);
    return rc;
  }
  *out = h;
  return BLSGPU_OK;
}
extern "C" int blsgpu_kzg_cell_verifier_log_n(const blsgpu_kzg_cell_verifier* h) { return h ? h->log_n : -1; }
extern "C" int blsgpu_kzg_cell_verifier_log_l(const blsgpu_kzg_cell_verifier* h) { return h ? h->log_l : -1; }
extern "C" size_t blsgpu_kzg_cell_verifier_cells(const blsgpu_kzg_cell_verifier* h) { return h ? (size_t)2 << (h->log_n - h->log_l) : 0; }
extern "C" void blsgpu_kzg_cell_verifier_free(blsgpu_kzg_cell_verifier* h) {
  if (!h) return;
  handle_quiesce(h->device);                                     // an asynchronous call may still be reading the bases, the table or the roots
  if (h->s) blsgpu_bases_free(h->s);
  if (h->table) blsgpu_g2_prepared_free(h->table);
  if (h->roots) hipFree(h->roots);
  delete h;
}
static KzgvArgs kzgv_args(const blsgpu_kzg_cell_verifier* h, const void* commit_xy, const void* commit_inf, size_t ncommit, const void* row, const void* col, const void* cells,
                          const void* proof_xy, const void* proof_inf, const void* offsets, size_t nseg, size_t m, const void* r, int order, const void* verdict, const void* out_ab,
                          bool device) {
  KzgvArgs a;
  a.handle_given = h != nullptr;
  if (h) { a.log_n = h->log_n; a.log_l = h->log_l; }
  a.commit_xy = commit_xy; a.commit_inf = commit_inf; a.ncommit = ncommit; a.row = row; a.col = col; a.cells = cells; a.proof_xy = proof_xy; a.proof_inf = proof_inf;
  a.offsets = offsets; a.nseg = nseg; a.m = m; a.r = r; a.order = order; a.verdict = verdict; a.out_ab = out_ab; a.device = device;
  return a;
}
static int kzg_verify_device(blsgpu_ctx* c, const blsgpu_kzg_cell_verifier* h, const void* d_commit_xy, const void* d_commit_inf, size_t ncommit, const void* d_row,
                             const void* d_col, const void* d_cells, const void* d_proof_xy, const void* d_proof_inf, const void* d_offsets, size_t nseg, size_t m, const void* d_r,
                             int order, void* d_verdict, void* d_out_ab) {
  if (!c) return bad("kzg_verify_cells: ctx is NULL");
  const KzgvArgs a = kzgv_args(h, d_commit_xy, d_commit_inf, ncommit, d_row, d_col, d_cells, d_proof_xy, d_proof_inf, d_offsets, nseg, m, d_r, order, d_verdict, d_out_ab, true);
  if (const char* why = kzgv_check(a)) return bad(why);
  if (h->device != c->device) return bad("kzg_verify_cells: the handle lives on another device than the context");
  if (!nseg) return BLSGPU_OK;
  const KzgvPlan p = kzgv_plan(h->log_n, h->log_l, m, nseg);
  if (!p.ok) return bad("kzg_verify_cells: the plan refuses the shape");
  HIPCHK(hipSetDevice(c->device));
  if (c->kzgv.reserve(p.bytes)) { g_err = "hipMalloc(kzg_verify_cells scratch) failed"; return BLSGPU_ERR_HIP; }
  hipStream_t st = c->stream;
  uint8_t* base = c->kzgv.as<uint8_t>();
  const int log_n = p.log_n, log_l = p.log_l;
  u32* eff = (u32*)(base + p.eff);
  uint8_t *mis = base + p.mis, *badidx = base + p.badidx, *badf = base + p.bad, *isone = base + p.isone;
  u32 *scal = (u32*)(base + p.scal), *cellc = (u32*)(base + p.cellc), *agg = (u32*)(base + p.agg);
  // 1. the offsets every stage walks, the weights, the gather
  HIPCHK(hipMemsetAsync(badidx, 0, nseg, st));
  KLAUNCH(k_kzgv_offsets, dim3(p.scan_grid), dim3(KZGV_BLOCK), 0, st, (const u32*)d_offsets, (u32)nseg, (u32)m, log_l, eff, mis, (unsigned long long*)(base + p.off64),
          (u32*)(base + p.msm_off), (u32*)(base + p.base_first), c->status_word);
  if (m)
    KLAUNCH(k_kzgv_weights, dim3(p.weights_grid), dim3(KZGV_BLOCK), 0, st, (const u32*)eff, (u32)nseg, (u32)m, (const u32*)d_row, (const u32*)d_col, (u32)ncommit, (const u32*)d_r,
            (const u32*)h->roots, (const uint2*)d_commit_xy, (const uint8_t*)d_commit_inf, (const uint2*)d_proof_xy, (const uint8_t*)d_proof_inf, log_n, log_l, order, scal,
            (uint2*)(base + p.pxy), base + p.pinf, badidx, c->status_word);
  LAUNCHCHK();
  // 2. the 3 m products in ONE call; 3. their sums per batch and third (the products go through the normalisation the segment sums read)
  {
    ScalarFormScope mont(c, SCALAR_MONT);                        // the weights are Montgomery limbs whatever the context's setting
    if (int rc = mul_batch_device<FpPolicy>(c, base + p.pxy, base + p.pinf, scal, p.products, base + p.prod)) return rc;
  }
  if (int rc = batch_normalize_device<FpPolicy>(c, base + p.prod, p.products, base + p.pxy, base + p.pinf)) return rc;
  if (int rc = sum_segments_device<FpPolicy>(c, base + p.pxy, base + p.pinf, p.products, nullptr, base + p.off64, p.sums, p.products, base + p.sum)) return rc;
  // 4. the cells in natural coset order, inverse-transformed; 5. the fold
  if (m) {
    KLAUNCH(k_kzg_scalar_copy, dim3(p.copy_grid), dim3(KZG_BLOCK), 0, st, (const uint4*)d_cells, (uint4*)cellc, m, log_l, log_l, order == KZGV_ORDER_BITREV ? 1 : 0);
    LAUNCHCHK();
    if (int rc = blsgpu_fr_ntt_many_device(c, cellc, log_l, m, 1, nullptr)) return rc;
    KLAUNCH(k_kzgv_fold_chunks, dim3(p.fold_grid), dim3(KZGV_BLOCK), 0, st, (const u32*)eff, (u32)nseg, (u32)m, (const u32*)d_col, (const u32*)scal, (const u32*)cellc,
            (const u32*)h->roots, log_n, log_l, order, p.chunk, (u32)p.nchunks, agg, (u32*)(base + p.part));
  }
  KLAUNCH(k_kzgv_fold_combine, dim3(p.combine_grid), dim3(KZGV_BLOCK), 0, st, (const u32*)eff, (u32)nseg, log_l, p.chunk, (const u32*)(base + p.part), agg);
  LAUNCHCHK();
  // 6. sum_u agg[s][u] S[u]: one segment per batch over the handle's bases
  {
    ScalarFormScope mont(c, SCALAR_MONT);
    if (int rc = msm_segments_device<FpPolicy>(c, h->s, base + p.base_first, base + p.msm_off, agg, nseg, nseg << log_l, base + p.msm)) return rc;
  }
  // 7. (A_s, B_s) and the pairing terms; 8.-10. one two-term product per batch against {q, -G2}
  KLAUNCH(k_kzgv_finish, dim3(p.finish_grid), dim3(KZGV_BLOCK), 0, st, (const u32*)(base + p.sum), (const u32*)(base + p.msm), (const uint8_t*)mis, (const uint8_t*)badidx, (u32)nseg,
          (u32*)(base + p.ab), (u32*)d_out_ab, (u32*)(base + p.qidx), (unsigned long long*)(base + p.poff), badf);
  LAUNCHCHK();
  if (int rc = batch_normalize_device<FpPolicy>(c, base + p.ab, p.terms, base + p.abxy, base + p.abinf)) return rc;
  if (int rc = blsgpu_multi_miller_loop_prepared_many_device(c, base + p.abxy, base + p.abinf, nullptr, nullptr, base + p.qidx, h->table, base + p.poff, nseg, p.terms, 2, 1, base + p.gt))
    return rc;
  if (int rc = blsgpu_gt_is_identity_device(c, base + p.gt, nseg, isone)) return rc;
  KLAUNCH(k_kzgv_verdict, dim3(p.finish_grid), dim3(KZGV_BLOCK), 0, st, (const uint8_t*)isone, (const uint8_t*)badf, (u32)nseg, (uint8_t*)d_verdict);
  LAUNCHCHK();
  return BLSGPU_OK;
}
extern "C" int blsgpu_kzg_verify_cells_device(blsgpu_ctx* c, const blsgpu_kzg_cell_verifier* h, const void* commit_xy, const void* commit_inf, size_t ncommit, const void* row,
                                              const void* col, const void* cells, const void* proof_xy, const void* proof_inf, const void* offsets, size_t nseg, size_t m, const void* r,
                                              int order, void* verdict, void* out_ab) { CTX_CLAIM(c);
  return kzg_verify_device(c, h, commit_xy, commit_inf, ncommit, row, col, cells, proof_xy, proof_inf, offsets, nseg, m, r, order, verdict, out_ab); }
extern "C" int blsgpu_kzg_verify_cells(blsgpu_ctx* c, const blsgpu_kzg_cell_verifier* hd, const uint64_t* commit_xy, const uint8_t* commit_inf, size_t ncommit, const uint32_t* row,
                                       const uint32_t* col, const uint64_t* cells, const uint64_t* proof_xy, const uint8_t* proof_inf, const uint32_t* offsets, size_t nseg,
                                       const uint64_t* r, int order, uint8_t* verdict, uint64_t* out_ab) { CTX_CLAIM(c);
  if (!c) return bad("kzg_verify_cells: ctx is NULL");
  if (nseg > ((size_t)1 << KZGV_MAX_LOG_SEGS)) return bad("kzg_verify_cells: nseg must not exceed 2^24");
  if (nseg && !offsets) return bad("kzg_verify_cells: NULL offsets, challenges or verdicts with batches to check");
  const size_t m = nseg ? offsets[nseg] : 0;
  const KzgvArgs a = kzgv_args(hd, commit_xy, commit_inf, ncommit, row, col, cells, proof_xy, proof_inf, offsets, nseg, m, r, order, verdict, out_ab, false);
  if (const char* why = kzgv_check(a)) return bad(why);
  if (const char* why = kzgv_check_host(offsets, nseg, m, row, col, ncommit, hd->log_n, hd->log_l)) return bad(why);
  if (!nseg) return BLSGPU_OK;
  HostCall h(c);
  h.report_status();
  // nine inputs through the staging buffers: the u32 arrays share one, the flag arrays another (each piece at a 256-byte boundary)
  auto up = [](size_t x) { return (x + 255) / 256 * 256; };
  void* dcells = h.in(c->io_a, cells, (m << hd->log_l) * 32);
  void* dproof = h.in(c->io_b, proof_xy, m * 96);
  void* dcommit = h.in(c->io_e, commit_xy, ncommit * 96);
  const size_t o_row = up(nseg * 32), o_col = o_row + up(m * 4), o_off = o_col + up(m * 4), words = o_off + (nseg + 1) * 4;
  const size_t o_cinf = up(m), flags = o_cinf + ncommit;
  uint8_t *wf = nullptr, *ff = nullptr;
  if (h.reserve(c->io_f, words) && h.reserve(c->flags_a, flags)) {
    wf = c->io_f.as<uint8_t>(); ff = c->flags_a.as<uint8_t>();
    const struct { void* dst; const void* src; size_t bytes; } piece[6] = {{wf, r, nseg * 32}, {wf + o_row, row, m * 4}, {wf + o_col, col, m * 4}, {wf + o_off, offsets, (nseg + 1) * 4},
                                                                          {ff, proof_inf, m}, {ff + o_cinf, commit_inf, ncommit}};
    for (const auto& q : piece) if (!h.rc && q.bytes) h.rc = staged_upload(c, q.dst, q.src, q.bytes);
  }
  void* v = h.out(c->flags_b, verdict, nseg);
  void* ab = out_ab ? h.out(c->io_out, out_ab, nseg * 288) : nullptr;
  if (h.rc) return h.rc;
  return h.finish(kzg_verify_device(c, hd, dcommit, ff + o_cinf, ncommit, wf + o_row, wf + o_col, dcells, dproof, ff, wf + o_off, nseg, m, wf, order, v, ab));
}

// ---------------------------------------------------------------------------------------------------
// pairings
// MSM on the reference's public encodings (for a wrapper crate that cannot see limbs): bases as uncompressed
// bytes (`to_uncompressed`, decoded like `from_uncompressed_unchecked`), scalars as `Scalar::to_bytes`, result as the
// uncompressed bytes of the affine sum.  A composition of the entry points above.
template <int G>
static int msm_bytes(blsgpu_ctx* c, const uint8_t* bases, const uint8_t* scalars, size_t n, uint8_t* out) {
  constexpr int W = G == 1 ? 12 : 24, BYTES = G == 1 ? 96 : 192;
  if (!c || !out || (n && (!bases || !scalars))) return bad("msm_bytes: NULL argument");
  ScalarFormScope bytes_form(c, SCALAR_BYTES);        // this entry point's scalars ARE `Scalar::to_bytes()` output, whatever the context's setting
  std::vector<uint64_t> xy(n * W + 1), xyz(3 * W), axy(2 * W);
  std::vector<uint8_t> inf(n + 1), ok(n + 1);
  uint8_t ainf = 0;
  int rc = BLSGPU_OK;
  if (n) {
    rc = G == 1 ? blsgpu_g1_from_bytes_batch(c, bases, n, 0, 0, xy.data(), inf.data(), ok.data()) : blsgpu_g2_from_bytes_batch(c, bases, n, 0, 0, xy.data(), inf.data(), ok.data());
    if (rc) return rc;
    for (size_t i = 0; i < n; i++) if (!ok[i]) return bad("msm_bytes: a base is not a valid uncompressed encoding");
  }
  rc = G == 1 ? blsgpu_g1_msm_host(c, xy.data(), inf.data(), scalars, n, xyz.data()) : blsgpu_g2_msm_host(c, xy.data(), inf.data(), scalars, n, xyz.data());
  if (rc) return rc;
  rc = G == 1 ? blsgpu_g1_batch_normalize(c, xyz.data(), 1, axy.data(), &ainf) : blsgpu_g2_batch_normalize(c, xyz.data(), 1, axy.data(), &ainf);
  if (rc) return rc;
  (void)BYTES;
  return G == 1 ? blsgpu_g1_to_bytes_batch(c, axy.data(), &ainf, 1, 0, out) : blsgpu_g2_to_bytes_batch(c, axy.data(), &ainf, 1, 0, out);
}
extern "C" int blsgpu_g1_msm_bytes(blsgpu_ctx* c, const uint8_t* bases, const uint8_t* scalars, size_t n, uint8_t out[96]) { CTX_CLAIM(c); return msm_bytes<1>(c, bases, scalars, n, out); }
extern "C" int blsgpu_g2_msm_bytes(blsgpu_ctx* c, const uint8_t* bases, const uint8_t* scalars, size_t n, uint8_t out[192]) { CTX_CLAIM(c); return msm_bytes<2>(c, bases, scalars, n, out); }

#ifdef BLS_ACC_TRACE
// diagnostic build only: where the accumulation kernel writes its per-wavefront trace (4 words per wavefront; nullptr = off)
extern "C" int blsgpu_diag_set_acc_trace(void* device_words) {
  unsigned long long* p = (unsigned long long*)device_words;
  return hipMemcpyToSymbol(HIP_SYMBOL(bls::g_acc_trace), &p, sizeof(p)) == hipSuccess ? 0 : 1;
}
// sequence mode: 1 = every wavefront of every following launch appends its record (up to 2^18); 0 = back to one record per wavefront index
extern "C" int blsgpu_diag_set_acc_trace_seq(unsigned int on) {
  return hipMemcpyToSymbol(HIP_SYMBOL(bls::g_acc_seq), &on, sizeof(on)) == hipSuccess ? 0 : 1;
}
#endif
