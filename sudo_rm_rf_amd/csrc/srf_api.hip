// Plan + whole-forward orchestration behind the C ABI (include/sudormrf_hip.h).
//   srf_forward  <-  SuDORMRF.forward            improved_sudormrf.py:283-301
//                    GroupCommSudoRmRf.forward   groupcomm_sudormrf_v2.py:302-322
// One immutable plan per (config, batch, T): parameter indices in state_dict() order, workspace
// carve-up, GlobLN statistic slots.  The library allocates nothing on the device: the caller hands
// in one workspace buffer.  All launches go to the caller's stream; nothing synchronises.
#include <string.h>

#include <atomic>
#include <mutex>
#include <new>
#include <vector>

#include "srf_improved_walk.h"

// ---------------------------------------------------------------------------------------------
// error string / kernel mode
// ---------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
static std::atomic<int> g_kernel_mode{0};   // process-wide diagnostics switch (tests, bench A/B); per-thread override below

void srf_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
// per-thread override (srf_forward_train runs its GEMMs in exact fp32 by default, see srf_train.hip)
static thread_local int g_kernel_mode_override = -1;
int srf_kernel_mode() { return g_kernel_mode_override >= 0 ? g_kernel_mode_override : g_kernel_mode.load(std::memory_order_relaxed); }
int srf_kernel_mode_override(int mode) {
  const int prev = g_kernel_mode_override;
  g_kernel_mode_override = mode;
  return prev;
}
static std::atomic<int> g_debug_flags{0};   // process-wide diagnostics switch: kernel-variant A/B only, never set by the product path
int srf_debug_flags() { return g_debug_flags.load(std::memory_order_relaxed); }
extern "C" void srf_set_debug_flags(int f) { g_debug_flags.store(f, std::memory_order_relaxed); }

// ---- per-device caches (see srf_common.h) ----------------------------------------------------------
static std::mutex g_dev_mu;
static int g_dev_cus[SRF_MAX_DEVICES];
static long g_dev_occ[SRF_MAX_DEVICES][SRF_OCC_SLOTS];
static bool g_dev_occ_set[SRF_MAX_DEVICES][SRF_OCC_SLOTS];

int srf_current_device() {
  int dev = 0;
  return hipGetDevice(&dev) == hipSuccess ? dev : -1;
}
int srf_device_cus() {
  const int dev = srf_current_device();
  if (dev < 0 || dev >= SRF_MAX_DEVICES) return 256;
  std::lock_guard<std::mutex> lk(g_dev_mu);
  if (!g_dev_cus[dev]) {
    hipDeviceProp_t prop;
    g_dev_cus[dev] = hipGetDeviceProperties(&prop, dev) == hipSuccess ? prop.multiProcessorCount : 256;
  }
  return g_dev_cus[dev];
}
long srf_device_cached(int slot, long (*compute)(void*), void* arg) {
  const int dev = srf_current_device();
  if (dev < 0 || dev >= SRF_MAX_DEVICES || slot < 0 || slot >= SRF_OCC_SLOTS) return compute(arg);
  {
    std::lock_guard<std::mutex> lk(g_dev_mu);
    if (g_dev_occ_set[dev][slot]) return g_dev_occ[dev][slot];
  }
  // evaluated OUTSIDE the lock (compute may call srf_device_cus(), which takes it); two threads racing here compute the
  // same value for the same device
  const long v = compute(arg);
  std::lock_guard<std::mutex> lk(g_dev_mu);
  g_dev_occ[dev][slot] = v;
  g_dev_occ_set[dev][slot] = true;
  return v;
}

// ---- in-library HIP-event profiler: one event after every kernel launch on the caller's stream ------
struct ProfMark {
  const char* name;
  hipEvent_t ev;
  hipStream_t st;     // the stream the event was recorded on (timeline mode: launches of several streams in one list)
};
static bool g_prof = false;
static std::vector<ProfMark> g_marks;
static std::vector<hipEvent_t> g_pool;
static std::vector<float> g_ms;

static thread_local int g_prof_hold = 0;   // > 0: launches of a multi-launch operation are not marked one by one
bool srf_profiling() { return g_prof && g_prof_hold == 0; }
void srf_prof_hold(int delta) { g_prof_hold += delta; }
void srf_prof_mark(const char* name, hipStream_t st) {
  hipEvent_t ev;
  if (!g_pool.empty()) {
    ev = g_pool.back();
    g_pool.pop_back();
  } else if (hipEventCreate(&ev) != hipSuccess) {
    return;
  }
  (void)hipEventRecord(ev, st);
  g_marks.push_back(ProfMark{name, ev, st});
}

extern "C" int srf_profile_begin(void* stream) {
  for (auto& m : g_marks) g_pool.push_back(m.ev);
  g_marks.clear();
  g_ms.clear();
  g_prof = true;
  srf_prof_mark("begin", (hipStream_t)stream);
  return SRF_OK;
}

extern "C" int srf_profile_end(void* stream, int* count) {
  g_prof = false;
  SRF_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
  g_ms.assign(g_marks.size(), 0.f);
  for (size_t i = 1; i < g_marks.size(); ++i) {
    float ms = 0.f;
    SRF_CHECK_HIP(hipEventElapsedTime(&ms, g_marks[i - 1].ev, g_marks[i].ev));
    g_ms[i] = ms;
  }
  if (count) *count = g_marks.empty() ? 0 : (int)g_marks.size() - 1;
  return SRF_OK;
}

// Timeline view of the same marks (the forward AS TIMED runs on two streams, rocprofv3's kernel trace
// serialises them): mark i's completion time in ms since mark 0 ("begin") and the index of its stream in order of first
// appearance.  The caller synchronises the device before srf_profile_end when more than one stream was used.
extern "C" int srf_profile_timeline(int i, const char** name, float* t_ms, int* stream_index) {
  SRF_CHECK_ARG(i >= 0 && (size_t)(i + 1) < g_marks.size() && name && t_ms && stream_index, "srf_profile_timeline: bad index %d", i);
  float ms = 0.f;
  SRF_CHECK_HIP(hipEventElapsedTime(&ms, g_marks[0].ev, g_marks[i + 1].ev));
  int idx = 0;
  std::vector<hipStream_t> seen;
  for (size_t j = 1; j <= (size_t)(i + 1); ++j) {
    bool known = false;
    for (size_t k = 0; k < seen.size(); ++k)
      if (seen[k] == g_marks[j].st) {
        known = true;
        if (j == (size_t)(i + 1)) idx = (int)k;
      }
    if (!known) {
      if (j == (size_t)(i + 1)) idx = (int)seen.size();
      seen.push_back(g_marks[j].st);
    }
  }
  *name = g_marks[i + 1].name;
  *t_ms = ms;
  *stream_index = idx;
  return SRF_OK;
}

extern "C" int srf_profile_get(int i, const char** name, float* ms) {
  SRF_CHECK_ARG(i >= 0 && (size_t)(i + 1) < g_marks.size() && name && ms, "srf_profile_get: bad index %d", i);
  *name = g_marks[i + 1].name;
  *ms = g_ms[i + 1];
  return SRF_OK;
}

extern "C" const char* srf_last_error(void) { return g_err; }
extern "C" int srf_abi_version(void) { return SRF_ABI_VERSION; }
extern "C" void srf_set_kernel_mode(int mode) { g_kernel_mode.store((mode == 1 || mode == 2) ? mode : 0, std::memory_order_relaxed); }
extern "C" int srf_get_kernel_mode(void) { return g_kernel_mode.load(std::memory_order_relaxed); }

// Zero fill as a kernel of our own rather than hipMemsetAsync: the inference forward is replayed from a captured HIP graph
// for small batches (engine.py), and a graph made of kernel nodes only replayed correctly where one with memset nodes did
// not (NaN outputs after an unrelated host-synchronising copy, ROCm 7.0 runtime; tools/diag_graph.py).  16-byte granules.
__global__ __launch_bounds__(256) void srf_zero_kernel(uint4* __restrict__ p, size_t n16) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) p[i] = make_uint4(0, 0, 0, 0);
}
int srf_zero_launch(void* p, size_t bytes, hipStream_t st) {
  SRF_CHECK_ARG(srf_aligned16(p) && bytes % 16 == 0, "internal: zero fill needs 16-byte granules");
  const size_t n16 = bytes / 16;
  if (!n16) return SRF_OK;
  const size_t blocks = (n16 + 255) / 256;
  hipLaunchKernelGGL(srf_zero_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, st, (uint4*)p, n16);
  SRF_CHECK_LAUNCH("zero_fill", st);
  return SRF_OK;
}

// ---------------------------------------------------------------------------------------------
// decoder = transpose(weight) -> frame GEMM (K2) -> overlap-add + crop
// ---------------------------------------------------------------------------------------------
extern "C" size_t srf_decoder_scratch_floats(int Bt, int Ci, int Co, int K, int L) {
  const size_t M = (size_t)Co * K;
  // wt [M][Ci] | zero bias [M] | z [Bt][M][L]   (each section 64-float aligned)
  return srf_align_up(M * Ci, 64) + srf_align_up(M, 64) + srf_align_up((size_t)Bt * M * L, 64);
}

extern "C" int srf_decoder(const float* v, const float* w, float* out, int Bt, int Ci, int Co, int K,
                           int L, int T, float* scratch, void* stream) {
  return srf_decoder_impl(v, w, out, Bt, Ci, Co, K, L, T, scratch, nullptr, nullptr, 0, stream);
}
// post_stats / post_wav / post_mc: the callers' rescale (+ mixture consistency) folded into the overlap-add (srf_separate)
// in_prelu: a PReLU slope applied to v as the frame GEMM loads it (the causal model's mask_nl_class), NULL = none
// lens / frames: the ragged overlap-add (srf_original_forward_ragged); the transpose and the frame GEMM run over every column
int srf_decoder_impl(const float* v, const float* w, float* out, int Bt, int Ci, int Co, int K, int L, int T,
                     float* scratch, const float* post_stats, const float* post_wav, int post_mc, void* stream,
                     const float* in_prelu, const SrfFrames* lens, const SrfFrames* frames) {
  SRF_CHECK_ARG(v && w && out && scratch, "srf_decoder: null pointer");
  SRF_CHECK_ARG(Bt > 0 && Ci > 0 && Co > 0 && L > 0 && T > 0, "srf_decoder: bad sizes");
  SRF_CHECK_ARG(K >= 3 && (K & 1), "srf_decoder: kernel size must be odd (got %d)", K);
  SRF_CHECK_ARG(T <= (K / 2) * L, "srf_decoder: T=%d exceeds hop*L=%d", T, (K / 2) * L);
  SRF_CHECK_ARG(Co <= 65535 && Bt <= 65535, "srf_decoder: too many channels / batch");
  SRF_CHECK_ALIGNED16("srf_decoder", {"scratch", scratch});      // (zero-filled with 16-byte stores; checked before the first launch)
  hipStream_t st = (hipStream_t)stream;
  const int M = Co * K;
  float* wt = scratch;
  float* zb = wt + srf_align_up((size_t)M * Ci, 64);
  float* z = zb + srf_align_up((size_t)M, 64);
  int rc = srf_transpose_launch(w, wt, Ci, M, st);
  if (rc) return rc;
  rc = srf_zero_launch(zb, sizeof(float) * srf_align_up((size_t)M, 64), st);
  if (rc) return rc;
  const srf_norm act{nullptr, nullptr, nullptr, in_prelu};
  rc = srf_pw_conv(v, wt, zb, z, Bt, Ci, M, L, in_prelu ? &act : nullptr, nullptr, nullptr, 0, nullptr, 0, stream);
  if (rc) return rc;
  return srf_overlap_add_launch(z, out, Bt, Co, K, L, T, 1, post_stats, post_wav, post_mc, st, lens, frames);
}

// ---------------------------------------------------------------------------------------------
// plan
// ---------------------------------------------------------------------------------------------
// T padded up to a multiple of n_least_samples_req = h * 2^D, at least one (improved_sudormrf.py:244,303-314)
static long plan_padded_length(int T, int h, int D) {
  const long nls = (long)h << D;
  return (T < nls) ? nls : ((T / nls) + (T % nls ? 1 : 0)) * nls;
}
static int plan_fail(srf_plan* p, int rc) {
  delete p;
  return rc;
}

static int causal_plan_create(const srf_config* c, int batch, int T, srf_plan** out);
extern "C" int srf_plan_create(const srf_config* c, int batch, int T, srf_plan** out) {
  SRF_CHECK_ARG(c && out, "srf_plan_create: null pointer");
  *out = nullptr;
  SRF_CHECK_ARG(c->variant == SRF_VARIANT_IMPROVED || c->variant == SRF_VARIANT_GROUPCOMM || c->variant == SRF_VARIANT_CAUSAL,
                c->variant == SRF_VARIANT_ATTENTIVE      ? "srf_plan_create: variant %d (attentive) takes srf_attentive_plan_create"
                : c->variant == SRF_VARIANT_ATTENTIVE_V3 ? "srf_plan_create: variant %d (attentive v3) takes srf_attentive_v3_plan_create"
                : c->variant == SRF_VARIANT_ORIGINAL     ? "srf_plan_create: variant %d (original) takes srf_original_plan_create"
                                                         : "srf_plan_create: unknown variant %d",
                c->variant);
  if (c->variant == SRF_VARIANT_CAUSAL) return causal_plan_create(c, batch, T, out);
  SRF_CHECK_ARG(batch > 0 && T > 0, "srf_plan_create: batch and T must be positive");
  SRF_CHECK_ARG(c->out_channels > 0 && c->in_channels > 0 && c->num_blocks > 0 && c->enc_num_basis > 0 &&
                    c->num_sources > 0,
                "srf_plan_create: non-positive model dimension");
  SRF_CHECK_ARG(c->upsampling_depth >= 1 && c->upsampling_depth <= SRF_MAX_DEPTH,
                "srf_plan_create: upsampling_depth %d unsupported (1..%d)", c->upsampling_depth,
                SRF_MAX_DEPTH);
  SRF_CHECK_ARG(c->enc_kernel_size >= 3 && (c->enc_kernel_size & 1),
                "srf_plan_create: enc_kernel_size must be odd (the reference's mask multiply breaks "
                "for even sizes)");
  srf_plan* p = new (std::nothrow) srf_plan();
  SRF_CHECK_ARG(p != nullptr, "srf_plan_create: out of host memory");
  p->cfg = *c;
  const bool gc = c->variant == SRF_VARIANT_GROUPCOMM;
  const int G = gc ? c->group_size : 1;
  p->A = gc ? c->in_audio_channels : 1;
  if (G <= 0 || p->A <= 0) {
    srf_set_error("srf_plan_create: group_size / in_audio_channels must be positive");
    return plan_fail(p, SRF_EINVAL);
  }
  if (gc && (c->out_channels % G || c->in_channels % G)) {
    srf_set_error("srf_plan_create: channels (%d,%d) not divisible by group_size %d", c->out_channels,
                  c->in_channels, G);
    return plan_fail(p, SRF_EINVAL);
  }
  if (gc) {
    const int n = c->out_channels / G;
    if (!(n == 2 || n == 4 || n == 8 || n == 16 || n == 32)) {
      srf_set_error("srf_plan_create: out_channels/group_size = %d unsupported (2,4,8,16,32)", n);
      return plan_fail(p, SRF_EINVAL);
    }
  }
  const int D = c->upsampling_depth, U = c->num_blocks, K = c->enc_kernel_size;
  const int h = K / 2;
  const long Tp = plan_padded_length(T, h, D);
  p->Bt = batch;
  p->T = T;
  p->Tp = (int)Tp;
  p->L = (int)((Tp + 2 * h - K) / h + 1);
  p->SA = c->num_sources * p->A;
  p->Bg = batch * G;
  p->nB = c->out_channels / G;
  p->nC = c->in_channels / G;
  if (p->L % (1 << (D - 1)) != 0) {
    srf_set_error("srf_plan_create: internal: L=%d not divisible by 2^(D-1)", p->L);
    return plan_fail(p, SRF_EINVAL);
  }
  if ((long)p->Bg > 65535) {
    srf_set_error("srf_plan_create: batch*group_size=%d too large (max 65535 per call)", p->Bg);
    return plan_fail(p, SRF_EINVAL);
  }
  // ---- parameter indexing (state_dict order)
  p->p_block0 = SRF_P_FRONT;
  p->p_ublock_off = gc ? SRF_P_TAC : 0;
  p->p_block_stride = plan_block_params(D, gc);
  p->p_tail = p->p_block0 + U * p->p_block_stride;
  p->n_params = p->p_tail + SRF_P_TAIL;
  // ---- statistic slots: ln | per block: [tac] proj d0..d{D-1} merged (plan_slots)
  p->slots_per_block = D + 2 + (gc ? 1 : 0);
  p->n_slots = 1 + U * p->slots_per_block;
  // ---- workspace
  const size_t F = sizeof(float);
  const size_t L = p->L;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t o = off;
    off = srf_align_up(off + bytes, 256);
    return o;
  };
  p->stats_bytes = (size_t)p->n_slots * p->Bg * SRF_STAT_BUCKETS * 2 * sizeof(double);
  p->off_stats = take(p->stats_bytes);
  p->off_enc = take(F * batch * c->enc_num_basis * L);
  p->off_xa = take(F * batch * c->out_channels * L);
  p->off_xb = take(F * batch * c->out_channels * L);
  p->off_xq = gc ? take(F * batch * c->out_channels * L) : 0;
  p->off_xu = gc ? take(F * batch * c->out_channels * L) : 0;
  p->off_y1 = take(F * batch * c->in_channels * L);
  for (int k = 0; k < D; ++k) p->off_lv[k] = take(F * batch * c->in_channels * (L >> k));
  p->off_masked = take(F * batch * p->SA * c->enc_num_basis * L);
  p->off_dec = take(F * srf_decoder_scratch_floats(batch, p->SA * c->enc_num_basis, p->SA, K, p->L));
  p->fused_pyramid = srf_pyramid_supported(p->nC, p->L, D);   // (evaluated with the default debug flags)
  p->off_pyr = p->fused_pyramid ? take(srf_pyramid_scratch_bytes(p->Bg, p->nC, p->L, D)) : 0;
  // packed weights for the split-precision GEMM (only shapes the kernel supports)
  p->pk_of_param.assign(p->n_params, 0);
  plan_add_pack(p, &off, SRF_P_BOTTLENECK, c->out_channels, c->enc_num_basis);
  for (int i = 0; i < U; ++i) {
    plan_add_pack(p, &off, plan_p_proj(p, i), p->nC, p->nB);
    plan_add_pack(p, &off, plan_p_res(p, i), p->nB, p->nC);
  }
  plan_add_pack(p, &off, plan_p_mask(p), p->SA * c->enc_num_basis, c->out_channels);
  // decoder weights as MFMA fragments for the fused tail (K5); whether it runs is decided per forward
  p->off_wdpack = (p->SA * K <= 64 && p->pk_of_param[plan_p_mask(p)]) ? take(srf_mask_decode_pack_bytes(p->SA * c->enc_num_basis)) : 0;
  p->total_bytes = off;
  p->n_launches = 1 /*memset*/ + 2 + U * (D + 3 + (gc ? 2 : 0)) + 1 + 4;
  *out = p;
  return SRF_OK;
}

// ---- causal variant (CausalSuDORMRF, causal_improved_sudormrf_v3.py; parameter layout: srf_plan.h) ---------------------------
static int causal_plan_create(const srf_config* c, int batch, int T, srf_plan** out) {
  SRF_CHECK_ARG(batch > 0 && T > 0, "srf_plan_create: batch and T must be positive");
  SRF_CHECK_ARG(c->in_audio_channels > 0 && c->out_channels > 0 && c->in_channels > 0 && c->num_blocks > 0 &&
                    c->enc_num_basis > 0 && c->num_sources > 0,
                "srf_plan_create: non-positive model dimension (causal variant)");
  SRF_CHECK_ARG(c->group_size == 1, "srf_plan_create: the causal variant has no groups (group_size must be 1, got %d)",
                c->group_size);
  SRF_CHECK_ARG(c->upsampling_depth >= 1 && c->upsampling_depth <= SRF_MAX_DEPTH,
                "srf_plan_create: upsampling_depth %d unsupported (1..%d)", c->upsampling_depth, SRF_MAX_DEPTH);
  SRF_CHECK_ARG(c->enc_kernel_size >= 3 && (c->enc_kernel_size & 1),
                "srf_plan_create: enc_kernel_size must be odd for the causal variant (got %d)", c->enc_kernel_size);
  srf_plan* p = new (std::nothrow) srf_plan();
  SRF_CHECK_ARG(p != nullptr, "srf_plan_create: out of host memory");
  p->cfg = *c;
  const int D = c->upsampling_depth, U = c->num_blocks, K = c->enc_kernel_size, N = c->enc_num_basis;
  const int B = c->out_channels, Cc = c->in_channels;
  const int h = K / 2;
  const long Tp = plan_padded_length(T, h, D);
  if (Tp > (1L << 30)) {
    srf_set_error("srf_plan_create: T=%d too long", T);
    return plan_fail(p, SRF_EINVAL);
  }
  p->A = c->in_audio_channels;
  p->Bt = batch;
  p->T = T;
  p->Tp = (int)Tp;
  p->L = (int)(Tp / h);            // (T' + 2(K-1) - (2K-1)) / h + 1
  p->SA = c->num_sources * p->A;
  p->Bg = batch;
  p->nB = B;
  p->nC = Cc;
  if (batch > 65535) {
    srf_set_error("srf_plan_create: batch %d too large (max 65535 per call)", batch);
    return plan_fail(p, SRF_EINVAL);
  }
  const SrfCausalLayout lay = causal_layout(U, D);
  p->p_block0 = lay.block0, p->p_block_stride = lay.stride, p->p_tail = lay.tail, p->n_params = lay.n_params;
  p->p_ublock_off = 0;
  p->slots_per_block = 0;
  p->n_slots = 0;
  p->alpha.assign(U, 1.f);
  p->beta.assign(U, 1.f);
  const size_t F = sizeof(float), L = p->L;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t o = off;
    off = srf_align_up(off + (bytes ? bytes : 1), 256);
    return o;
  };
  p->stats_bytes = 0;
  p->off_stats = 0;
  p->off_enc = take(F * batch * N * L);
  p->off_xa = take(F * batch * B * L);
  p->off_xb = take(F * batch * B * L);
  p->off_xq = p->off_xu = 0;
  p->off_y1 = take(F * batch * Cc * L);
  p->off_merged = take(F * batch * Cc * L);
  for (int k = 0; k < D; ++k) p->off_lv[k] = take(F * batch * Cc * (L >> k));
  p->off_masked = take(F * batch * p->SA * N * L);
  p->off_dec = take(F * srf_decoder_scratch_floats(batch, p->SA * N, p->SA, K, p->L));
  p->fused_pyramid = srf_causal_pyramid_supported(Cc, p->L, D);
  p->off_pyr = 0;
  // the folded weights of every block (srf_causal_fold)
  p->off_fold_res = take(F * causal_fold_res_floats(B, Cc) * U);
  p->off_fold_proj = take(F * (size_t)Cc * B * U);
  p->pk_of_param.assign(p->n_params, 0);
  plan_add_pack(p, &off, SRF_PC_BOTTLENECK, B, N);
  for (int i = 0; i < U; ++i) {
    plan_add_pack(p, &off, causal_p_proj(lay, i), Cc, B);
    plan_add_pack(p, &off, causal_p_res(lay, i), B, Cc);
  }
  plan_add_pack(p, &off, causal_p_mask(lay), p->SA * N, B);
  p->off_wdpack = 0;
  p->total_bytes = off;
  p->n_launches = 3 /*fold, pack, encoder*/ + 1 + U * 3 + 1 + 4;
  *out = p;
  return SRF_OK;
}

extern "C" int srf_plan_set_block_scales(srf_plan* p, const float* alpha, const float* beta, int n) {
  SRF_CHECK_ARG(p && alpha && beta, "srf_plan_set_block_scales: null pointer");
  SRF_CHECK_ARG(p->cfg.variant == SRF_VARIANT_CAUSAL, "srf_plan_set_block_scales: causal plans only (variant %d)", p->cfg.variant);
  SRF_CHECK_ARG(n == p->cfg.num_blocks, "srf_plan_set_block_scales: expected %d blocks, got %d", p->cfg.num_blocks, n);
  for (int i = 0; i < n; ++i) SRF_CHECK_ARG(beta[i] != 0.f, "srf_plan_set_block_scales: beta[%d] is zero", i);
  p->alpha.assign(alpha, alpha + n);
  p->beta.assign(beta, beta + n);
  return SRF_OK;
}

extern "C" void srf_plan_destroy(srf_plan* p) { delete p; }
extern "C" size_t srf_plan_workspace_bytes(const srf_plan* p) { return p ? p->total_bytes : 0; }
extern "C" int srf_plan_num_params(const srf_plan* p) { return p ? p->n_params : 0; }
extern "C" int srf_plan_frames(const srf_plan* p) { return p ? p->L : 0; }
extern "C" int srf_plan_padded_length(const srf_plan* p) { return p ? p->Tp : 0; }
extern "C" int srf_plan_num_launches(const srf_plan* p) { return p ? p->n_launches : 0; }

// ---------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------
static int srf_forward_impl(const srf_plan* p, const float* const* P, int num_params, const float* wav, float* out,
                            void* workspace, size_t workspace_bytes, const float* wav_stats, int mixture_consistency,
                            void* stream);
extern "C" int srf_forward(const srf_plan* p, const float* const* P, int num_params, const float* wav,
                           float* out, void* workspace, size_t workspace_bytes, void* stream) {
  return srf_forward_impl(p, P, num_params, wav, out, workspace, workspace_bytes, nullptr, 0, stream);
}

// The reference's caller-side inference recipe as ONE pass (README.md:100-114, experiments/simple_whamr_evaluation.py:
// 142-148): stats = per-row {mean, unbiased std} of the raw mixture (srf_wav_stats), the encoder normalises on load, the
// decoder's overlap-add rescales the estimates with the mixture's statistics and -- mixture_consistency != 0, what the README
// prescribes for the GroupComm models -- applies mixture_consistency.apply against the normalised mixture.  wav: the RAW
// mixture [Bt, in_audio_channels, T]; stats: [Bt * in_audio_channels][2] device floats (written here).
extern "C" int srf_separate(const srf_plan* p, const float* const* P, int num_params, const float* wav, float* out,
                            float* stats, int mixture_consistency, void* workspace, size_t workspace_bytes, void* stream) {
  SRF_CHECK_ARG(p && wav && stats, "srf_separate: null pointer");
  SRF_CHECK_ARG(p->cfg.variant != SRF_VARIANT_CAUSAL, "srf_separate: not available for the causal variant (CausalSuDORMRF)");
  SRF_CHECK_ARG(p->A == 1, "srf_separate: the recipe is defined for single-channel mixtures (in_audio_channels = %d)", p->A);
  int rc = srf_wav_stats(wav, stats, p->Bt * p->A, p->T, stream);
  if (rc) return rc;
  return srf_forward_impl(p, P, num_params, wav, out, workspace, workspace_bytes, stats, mixture_consistency, stream);
}

// what the forward entry points (`who`) ask of their arguments (srf_internal.h); ptrs: none of the caller's pointers is null
int forward_check_args(const char* who, bool ptrs, const srf_plan* p, const float* const* P, int num_params, const void* workspace,
                       size_t workspace_bytes) {
  SRF_CHECK_ARG(ptrs, "%s: null pointer", who);
  SRF_CHECK_ARG(num_params == p->n_params, "%s: expected %d parameter tensors, got %d", who, p->n_params, num_params);
  if (workspace_bytes < p->total_bytes) {
    srf_set_error("%s: workspace too small (%zu < %zu bytes)", who, workspace_bytes, p->total_bytes);
    return SRF_EWORKSPACE;
  }
  SRF_CHECK_ARG((((size_t)workspace) & 255) == 0, "%s: workspace must be 256-byte aligned", who);
  for (int i = 0; i < num_params; ++i) SRF_CHECK_ARG(P[i] != nullptr, "%s: parameter %d is null", who, i);
  return SRF_OK;
}

// The Improved / GroupComm inference forward: srf_forward, srf_separate (wav_stats), srf_forward_ragged (rg) and
// srf_separate_ragged (both).  It is improved_walk (srf_improved_walk.h, which also has the ragged invariant) over the plan's
// workspace -- two alternating stream buffers, one set of block tensors -- with the statistics cleared by a launch, the plan's
// packed images behind step helpers that pick the ragged twins, and srf_improved_tail.
static int forward_walk(const srf_plan* p, const float* const* P, const float* wav, float* out, void* workspace,
                        const float* wav_stats, int mixture_consistency, const Ragged* rg, void* stream) {
  const srf_config& c = p->cfg;
  const bool gc = c.variant == SRF_VARIANT_GROUPCOMM;
  const int N = c.enc_num_basis, Bt = p->Bt, L = p->L, nB = p->nB, nC = p->nC;
  char* ws = (char*)workspace;
  int rc = srf_zero_launch(ws + p->off_stats, p->stats_bytes, (hipStream_t)stream);
  if (rc) return rc;
  // A ragged batch runs what plan_ragged_now has made sure the uniform forward would choose here -- the packed weights, the fused
  // pyramid, the pair at the head and after every block (Improved) or the pre-add form (GroupComm), the fused tail -- whatever
  // the "at least as many tiles as CUs" gates of the pair and of the 256 x 128 GEMM say: it has no other kernel to go to.
  const bool use_pack = rg || plan_use_pack(p);
  if (use_pack) {
    rc = plan_pack_weights(p, [&](int param) { return P[param]; }, ws, stream);
    if (rc) return rc;
  }
  auto packed = [&](int param) { return plan_packed(p, ws, use_pack, param); };
  auto conv = [&](int rows_per_example, const float* x, const float* w, int param, const float* bias, float* y, int rows, int Cin,
                  int Cout, const srf_norm* in_norm, const float* residual, double* out_sums) {
    return imp_conv(rg, rows_per_example, x, w, packed(param), bias, y, rows, Cin, Cout, L, in_norm, residual, out_sums, stream);
  };
  auto pair = [&](const float* x, int param1, const float* bias1, float* y, const srf_norm* in_norm, const float* residual, int param2,
                  const float* bias2, float* y2, double* out_sums2, int Cin1, int Cmid, int Cout2) {
    return imp_pair(rg, x, packed(param1), bias1, y, in_norm, residual, packed(param2), bias2, y2, out_sums2, Bt, Cin1, Cmid, Cout2, L,
                    stream);
  };
  // Round 5: a 1x1 conv with 256 output channels and the proj_1x1 that consumes its output run as ONE launch, the 256-channel
  // tensor handed over in registers (srf_pwconv_x3f.hip): bottleneck -> proj_1x1 of block 0, res_conv of block i -> proj_1x1 of
  // block i + 1.  Needs the fused pyramid (its merged tensor has a buffer of its own: the pair kernel writes y1 while it reads the
  // merged tensor), and the head pair only runs where the block pairs do.  Debug flag 1 = separate launches.
  const bool fused = rg || plan_fused_pyramid_now(p);
  const int i_proj = plan_p_proj(p, 0), i_res = plan_p_res(p, 0);
  const bool pair_res = !gc && (rg || (use_pack && fused && packed(i_proj) && packed(i_res) && srf_pw_conv_pair_supported(Bt, nC, nB, nC, L)));
  const bool pair_head = pair_res && (rg || (packed(SRF_P_BOTTLENECK) && srf_pw_conv_pair_supported(Bt, N, nB, nC, L)));

  // merged: on y1 (dead once every level exists), or -- fused: pass 2 re-reads y1 with halos -- in the unused level-0 buffer
  SrfImpAddrs a{};
  a.stats = (double*)(ws + p->off_stats);
  a.enc = (float*)(ws + p->off_enc);
  a.x[0] = ws + p->off_xa, a.x[1] = ws + p->off_xb, a.blk = ws;
  a.o_y1 = p->off_y1, a.o_merged = fused ? p->off_lv[0] : p->off_y1, a.o_q = p->off_xq, a.o_u = p->off_xu;
  for (int k = 0; k < c.upsampling_depth; ++k) a.o_lv[k] = p->off_lv[k];
  a.lv_mask = fused ? 0u : ~0u;
  a.pyr = ws + p->off_pyr;
  rc = improved_walk(p, P, wav, a, conv, pair, pair_head, pair_res, fused, rg, wav_stats, stream);
  if (rc) return rc;
  return srf_improved_tail(p, P, a.x_in(c.num_blocks), out, workspace, use_pack, wav_stats, wav, mixture_consistency, rg, stream);
}

// ---- mask estimation + decoder of the Improved / GroupComm / attentive (v2, v3) walks      improved_sudormrf.py:295-301
// cur: the separation module's output; the encoder output is where the walk left it (off_enc); rg as in forward_walk
int srf_improved_tail(const srf_plan* p, const float* const* P, const float* cur, float* out, void* workspace, bool use_pack,
                      const float* wav_stats, const float* wav, int mixture_consistency, const Ragged* rg, void* stream) {
  const srf_config& c = p->cfg;
  const int N = c.enc_num_basis, K = c.enc_kernel_size, Bt = p->Bt, L = p->L;
  char* ws = (char*)workspace;
  hipStream_t st = (hipStream_t)stream;
  const SrfTail<const float> t = plan_tail(p, P);
  const void* mask_packed = plan_packed(p, ws, use_pack, plan_p_mask(p));
  const float* enc = (const float*)(ws + p->off_enc);
  float* masked = (float*)(ws + p->off_masked);
  int rc;
  // K5: mask GEMM and decoder contraction in ONE launch -- the [Bt, S N, L] masked tensor (the largest of the forward) never
  // reaches HBM; the GEMM leaves per-256-channel partial decoder frames (in the masked tensor's workspace region, <= 1/4 of
  // it) and the overlap-add sums them.  Only where the 256 x 128 GEMM would have run the mask conv anyway.  (Ragged: the
  // uniform GEMM over every column -- the block stream is unspecified past an example's end, and so are the partial frames it
  // makes there -- then the ragged overlap-add.)
  // (The attentive model's ragged walk has no gate on the tail: where its plan does not run the fused launch, it takes the
  // unfused path below with the ragged overlap-add.)
  if ((rg && c.variant != SRF_VARIANT_ATTENTIVE) || plan_fused_tail_now(p, use_pack)) {
    const int M = p->SA * K, nparts = (p->SA * N + 255) / 256;
    rc = srf_mask_decode_pack(t.dec_w, ws + p->off_wdpack, p->SA * N, M, st);
    if (rc) return rc;
    rc = srf_mask_decode(cur, t.mask_w, mask_packed, t.mask_b, t.mask_prelu, enc, N, ws + p->off_wdpack, masked, Bt, c.out_channels,
                         p->SA * N, L, M, st);
    if (rc) return rc;
    return imp_overlap_add(rg, masked, out, Bt, p->SA, K, L, p->T, nparts, wav_stats, wav, mixture_consistency, st);
  }
  srf_norm pre{nullptr, nullptr, nullptr, t.mask_prelu};
  rc = srf_pw_conv_packed(cur, t.mask_w, mask_packed, t.mask_b, masked, Bt, c.out_channels, p->SA * N, L, &pre, nullptr, nullptr, 1,
                          enc, N, stream);
  if (rc) return rc;
  // (ragged: the mask GEMM and the decoder's frame GEMM run over every column -- columns are independent in both -- and the
  // overlap-add reads the example's own frames, as in the original model's ragged walk)
  return srf_decoder_impl(masked, t.dec_w, out, Bt, p->SA * N, p->SA, K, L, p->T, (float*)(ws + p->off_dec), wav_stats, wav,
                          mixture_consistency, stream, nullptr, rg ? &rg->lens_t : nullptr, rg ? &rg->frames_t : nullptr);
}

static int causal_forward(const srf_plan* p, const float* const* P, const float* wav, float* out, void* workspace, void* stream);
static int srf_forward_impl(const srf_plan* p, const float* const* P, int num_params, const float* wav, float* out,
                            void* workspace, size_t workspace_bytes, const float* wav_stats, int mixture_consistency,
                            void* stream) {
  // The inference forward is what the engine runs as two sub-batches on two streams: its GEMMs take the half-CU blocks of
  // srf_pwconv_x3p.hip so that the other stream's kernels can co-reside (srf_pwconv.hip, srf_pw_256_launch).
  const SrfPairedScope paired_for_this_call;
  const int rc = forward_check_args("srf_forward", p && P && wav && out && workspace, p, P, num_params, workspace, workspace_bytes);
  if (rc) return rc;
  // profiler: intervals run from mark to mark, so without this one the first kernel's interval would also hold the
  // host-side gap since the previous forward
  if (srf_profiling()) srf_prof_mark("(gap)", (hipStream_t)stream);
  if (p->cfg.variant == SRF_VARIANT_CAUSAL) return causal_forward(p, P, wav, out, workspace, stream);
  if (p->cfg.variant == SRF_VARIANT_ATTENTIVE)
    return srf_attentive_forward(p, P, wav, out, workspace, wav_stats, mixture_consistency, stream);
  if (p->cfg.variant == SRF_VARIANT_ATTENTIVE_V3)
    return srf_attentive_v3_forward(p, P, wav, out, workspace, wav_stats, mixture_consistency, stream);
  if (p->cfg.variant == SRF_VARIANT_ORIGINAL)
    return srf_original_forward(p, P, wav, out, workspace, wav_stats, mixture_consistency, stream);
  return forward_walk(p, P, wav, out, workspace, wav_stats, mixture_consistency, nullptr, stream);
}

// ---- the by-value table of every ragged entry point (srf_internal.h)
int srf_frames_table(const char* what, const int* frames, int groups, int L, SrfFrames* out) {
  SRF_CHECK_ARG(frames != nullptr, "%s: null frames table", what);
  SRF_CHECK_ARG(groups >= 1 && groups <= SRF_RAGGED_MAX_BATCH, "%s: a ragged batch holds 1..%d examples (got %d)", what,
                SRF_RAGGED_MAX_BATCH, groups);
  for (int g = 0; g < SRF_RAGGED_MAX_BATCH; ++g) out->n[g] = 0;
  for (int g = 0; g < groups; ++g) {
    SRF_CHECK_ARG(frames[g] >= 1 && frames[g] <= L, "%s: example %d has %d frames (allowed: 1..%d)", what, g, frames[g], L);
    out->n[g] = frames[g];
  }
  return SRF_OK;
}

// ---------------------------------------------------------------------------------------------
// ragged forward: unequal-length examples in one set of launches (include/sudormrf_hip.h, "Ragged forms")
// ---------------------------------------------------------------------------------------------
// It IS the uniform walk (forward_walk above) with a frames table: plan_ragged_now is the gate -- whether the uniform forward of
// this plan, now, runs exactly the kernels that have ragged twins -- and the walk's step helpers pick the twins.
static bool plan_ragged_now(const srf_plan* p, const char** why) {
  const srf_config& c = p->cfg;
  const int D = c.upsampling_depth, U = c.num_blocks, N = c.enc_num_basis;
  auto no = [&](const char* w) {
    if (why) *why = w;
    return false;
  };
  const bool gc = c.variant == SRF_VARIANT_GROUPCOMM;
  if (c.variant == SRF_VARIANT_CAUSAL) return no("the causal model has no ragged kernels (per-example calls)");
  if (c.variant == SRF_VARIANT_ATTENTIVE || c.variant == SRF_VARIANT_ATTENTIVE_V3) return no("the attentive model has no ragged kernels (per-example calls)");
  if (c.variant == SRF_VARIANT_ORIGINAL) return no("the original model has no ragged kernels (per-example calls)");
  if (p->A != 1 || c.enc_kernel_size != 21) return no("the ragged encoder is the one-channel K = 21 kernel");
  if (gc && (c.group_size != 16 || p->nB != 16))
    return no("GroupComm: the ragged TAC is the MFMA kernel (group_size = 16, out_channels = 256)");
  if (gc && !(srf_pw_small_ragged_supported(p->nB, p->nC, p->L) && srf_pw_small_ragged_supported(p->nC, p->nB, p->L)))
    return no("GroupComm: in_channels / 16 is not a shape the thin conv's ragged forms take in both directions");
  if (p->Bt > SRF_RAGGED_MAX_BATCH) return no("the batch exceeds SRF_RAGGED_MAX_BATCH");
  if (!plan_use_pack(p)) return no("the forward does not run the packed 256 x 128 GEMMs (kernel mode / debug flags / shapes)");
  if (!plan_fused_pyramid_now(p) || srf_dbg(SRF_DBG_PYR_NO_REG) || !srf_pyramid_reg_supported(p->L, D))
    return no("the forward does not run the register-resident fused pyramid at this length");
  if (gc) {
    // what the uniform GroupComm forward must be running: the MFMA TAC, the fused pre-add, the packed bottleneck, the fused tail
    if (srf_dbg(SRF_DBG_TAC_ONE_STEP_PER_LANE | SRF_DBG_TAC_VALU | SRF_DBG_TAC_GENERIC | SRF_DBG_TAC_LANES_4TILES) ||
        (long)c.out_channels * p->L * 4 >= (1L << 31))
      return no("GroupComm: the forward does not run the MFMA TAC (debug flags / length)");
    if (!p->pk_of_param[SRF_P_BOTTLENECK] || !p->pk_of_param[plan_p_mask(p)] || !srf_x3w_shape_supported(N, c.out_channels, p->L) ||
        (long)p->Bt * ((p->L + 127) / 128) < 8)
      return no("bottleneck / mask conv shapes outside the 256 x 128 GEMM, or too few tiles for it");
    if (!plan_fused_tail_now(p, true))
      return no("the forward does not run the fused mask + decoder tail at this size (small launches)");
    return true;
  }
  if (!p->pk_of_param[SRF_P_BOTTLENECK] || !p->pk_of_param[plan_p_mask(p)]) return no("bottleneck / mask conv shapes outside the 256 x 128 GEMM");
  for (int i = 0; i < U; ++i)
    if (!p->pk_of_param[plan_p_proj(p, i)] || !p->pk_of_param[plan_p_res(p, i)]) return no("block conv shapes outside the 256 x 128 GEMM");
  if (!srf_pw_conv_pair_ragged_supported(N, p->nB, p->nC, p->L) || !srf_pw_conv_pair_ragged_supported(p->nC, p->nB, p->nC, p->L))
    return no("channel counts outside the fused conv pair (needs out_channels = 256)");
  if (!srf_x3w_shape_supported(p->nC, p->nB, p->L) || (long)p->Bt * ((p->L + 127) / 128) < 8)
    return no("too few tiles for the 256 x 128 GEMM");
  if (!plan_fused_tail_now(p, true)) return no("the forward does not run the fused mask + decoder tail at this size (small launches)");
  return true;
}
extern "C" int srf_plan_ragged_supported(const srf_plan* p) { return p && plan_ragged_now(p, nullptr) ? 1 : 0; }
extern "C" size_t srf_plan_ragged_workspace_bytes(const srf_plan* p) { return p && plan_ragged_now(p, nullptr) ? p->total_bytes : 0; }

// What srf_forward_ragged and srf_separate_ragged (`who`) share: the gate, the argument checks and every example's own padded
// length, as its batch-1 plan would have it -- all refusals BEFORE the first launch (a length the pyramid takes is on its 16- /
// 32-frame chunk grid: the "multiple of 4 frames" the GEMMs' ragged forms ask for is implied)
static int ragged_prepare(const char* who, const srf_plan* p, const float* const* P, int num_params, const int* lengths,
                          const void* workspace, size_t workspace_bytes, Ragged* rg) {
  const char* why = "";
  SRF_CHECK_ARG(plan_ragged_now(p, &why), "%s: plan not supported%s: %s", who,
                p->cfg.variant == SRF_VARIANT_IMPROVED ? "" : " (ragged kernels exist for the Improved model and for GroupComm with 16 groups of 16 channels)",
                why);
  int rc = forward_check_args(who, true /* checked by the caller: the gate comes first */, p, P, num_params, workspace, workspace_bytes);
  if (rc) return rc;
  const int D = p->cfg.upsampling_depth, h = p->cfg.enc_kernel_size / 2;
  rg->lengths = lengths;
  for (int b = 0; b < p->Bt; ++b) {
    SRF_CHECK_ARG(lengths[b] >= 1 && lengths[b] <= p->T, "%s: example %d has length %d (allowed: 1..%d)", who, b, lengths[b], p->T);
    rg->frames[b] = (int)(plan_padded_length(lengths[b], h, D) / h);
    SRF_CHECK_ARG(srf_pyramid_ragged_frames_ok(rg->frames[b], p->L, D),
                  "%s: example %d (length %d = %d frames) is too short for the fused pyramid or off its chunk grid", who, b,
                  lengths[b], rg->frames[b]);
  }
  rc = srf_frames_table(who, lengths, p->Bt, p->T, &rg->lens_t);
  if (rc) return rc;
  return srf_frames_table(who, rg->frames, p->Bt, p->L, &rg->frames_t);
}

extern "C" int srf_forward_ragged(const srf_plan* p, const float* const* P, int num_params, const float* wav, const int* lengths,
                                  float* out, void* workspace, size_t workspace_bytes, void* stream) {
  SRF_CHECK_ARG(p && P && wav && lengths && out && workspace, "srf_forward_ragged: null pointer");
  Ragged rg;
  const int rc = ragged_prepare("srf_forward_ragged", p, P, num_params, lengths, workspace, workspace_bytes, &rg);
  if (rc) return rc;
  if (srf_profiling()) srf_prof_mark("(gap)", (hipStream_t)stream);
  // no normalisation on load, no mixture consistency: the caller's business here (srf_separate_ragged folds both in).  (Not under
  // srf_pw_prefer_paired: the ragged forward runs on one stream.)
  return forward_walk(p, P, wav, out, workspace, nullptr, 0, &rg, stream);
}

// srf_separate over a ragged batch: srf_forward_ragged with a statistics launch over every row's own samples in front, the
// normalisation in the ragged encoder's load and the rescale (+ mixture consistency) in the ragged overlap-add's store.  wav: the
// RAW padded mixture; nothing at or past lengths[b] is read by any of the three.
extern "C" int srf_separate_ragged(const srf_plan* p, const float* const* P, int num_params, const float* wav, const int* lengths,
                                   float* out, float* stats, int mixture_consistency, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  SRF_CHECK_ARG(p && P && wav && lengths && out && stats && workspace, "srf_separate_ragged: null pointer");
  Ragged rg;
  int rc = ragged_prepare("srf_separate_ragged", p, P, num_params, lengths, workspace, workspace_bytes, &rg);
  if (rc) return rc;
  if (srf_profiling()) srf_prof_mark("(gap)", (hipStream_t)stream);
  rc = srf_wav_stats_ragged_launch(wav, rg.lens_t, stats, p->Bt, p->T, (hipStream_t)stream);
  if (rc) return rc;
  return forward_walk(p, P, wav, out, workspace, stats, mixture_consistency, &rg, stream);
}

extern "C" int srf_debug_fetch(const srf_plan* p, const void* workspace, int what, float* dst,
                               size_t dst_floats, void* stream) {
  SRF_CHECK_ARG(p && workspace && dst, "srf_debug_fetch: null pointer");
  const srf_config& c = p->cfg;
  const char* ws = (const char*)workspace;
  size_t off = 0, n = 0;
  if (what == 0) {
    off = p->off_enc;
    n = (size_t)p->Bt * c.enc_num_basis * p->L;
  } else if (what == 3 && c.variant == SRF_VARIANT_ORIGINAL) {      // the mask logits before the softmax
    off = p->off_orig_z;
    n = (size_t)p->Bt * p->SA * c.enc_num_basis * p->L;
  } else if (what == 1) {
    // (the original model's blocks write their output over their input)
    off = (c.num_blocks % 2 == 0 || c.variant == SRF_VARIANT_ORIGINAL) ? p->off_xa : p->off_xb;
    n = (size_t)p->Bt * c.out_channels * p->L;
  } else if (what == 2) {
    // the fused tail (K5) never materialises the masked tensor: its workspace region holds partial decoder frames
    if (plan_fused_tail_now(p, plan_use_pack(p))) {
      srf_set_error("srf_debug_fetch: the masked tensor is not materialised at this shape (mask GEMM and decoder run fused); "
                    "set debug flag 32768 to run the tail unfused");
      return SRF_EINVAL;
    }
    off = p->off_masked;
    n = (size_t)p->Bt * p->SA * c.enc_num_basis * p->L;
  } else {
    srf_set_error("srf_debug_fetch: unknown selector %d", what);
    return SRF_EINVAL;
  }
  SRF_CHECK_ARG(dst_floats >= n, "srf_debug_fetch: destination too small (%zu < %zu)", dst_floats, n);
  SRF_CHECK_HIP(hipMemcpyAsync(dst, ws + off, n * sizeof(float), hipMemcpyDeviceToDevice,
                               (hipStream_t)stream));
  return SRF_OK;
}

// ---------------------------------------------------------------------------------------------
// causal forward (CausalSuDORMRF.forward): encoder -> bottleneck -> U x [proj_1x1 -> fused causal pyramid -> res_conv with
// skipinit_gain * alpha folded into its weights, + residual] -> PReLU + mask conv -> PReLU folded into the decoder's load.
// ---------------------------------------------------------------------------------------------
// (srf_plan.h) entries of the one launch: per block res_conv weight, res_conv bias, then proj_1x1 weight where beta != 1
int srf_causal_fold(const srf_plan* p, const float* const* P, float* fold_res, float* fold_proj, SrfCausalFolded* out, hipStream_t st) {
  const int U = p->cfg.num_blocks, B = p->nB, Cc = p->nC;
  const SrfCausalLayout lay = causal_layout(p);
  std::vector<const float*> src, scale;
  std::vector<float*> dst;
  std::vector<long> n;
  std::vector<float> h;
  auto add = [&](const float* from, float* to, long count, const float* dscale, float hscale) {
    src.push_back(from), dst.push_back(to), n.push_back(count), scale.push_back(dscale), h.push_back(hscale);
  };
  out->wproj.assign(U, nullptr), out->wres.assign(U, nullptr), out->bres.assign(U, nullptr);
  for (int i = 0; i < U; ++i) {
    const SrfCausalBlock<const float> b = causal_block<const float>(lay, P, i);
    float* rw = fold_res + (size_t)i * causal_fold_res_floats(B, Cc);
    float* rb = rw + srf_align_up((size_t)B * Cc, 64);
    add(b.res_w, rw, (long)B * Cc, b.gain, p->alpha[i]);
    add(b.res_b, rb, (long)B, b.gain, p->alpha[i]);
    out->wres[i] = rw;
    out->bres[i] = rb;
    out->wproj[i] = b.proj_w;
    if (p->beta[i] != 1.f) {
      float* pw = fold_proj + (size_t)i * Cc * B;
      add(b.proj_w, pw, (long)Cc * B, nullptr, 1.f / p->beta[i]);
      out->wproj[i] = pw;
    }
  }
  return srf_causal_scale_many(src.data(), dst.data(), n.data(), scale.data(), h.data(), (int)src.size(), st);
}

static int causal_forward(const srf_plan* p, const float* const* P, const float* wav, float* out, void* workspace, void* stream) {
  const srf_config& c = p->cfg;
  const int D = c.upsampling_depth, U = c.num_blocks, N = c.enc_num_basis, K = c.enc_kernel_size;
  const int Bt = p->Bt, L = p->L, B = p->nB, Cc = p->nC;
  char* ws = (char*)workspace;
  hipStream_t st = (hipStream_t)stream;
  auto fptr = [&](size_t o) { return (float*)(ws + o); };
  const SrfCausalLayout lay = causal_layout(p);
  SrfCausalFolded w;
  int rc = srf_causal_fold(p, P, fptr(p->off_fold_res), fptr(p->off_fold_proj), &w, st);
  if (rc) return rc;
  // ---- split-bf16 weight images of the packed shapes (kernel mode 0), from the folded copies where there are any
  const bool use_pack = plan_use_pack(p);
  auto source_of = [&](int param) -> const float* {
    const SrfBlockParam q = plan_block_param(lay.block0, lay.stride, lay.tail, param);
    if (q.block >= 0 && q.rel == SRF_PC_PROJ) return w.wproj[q.block];
    if (q.block >= 0 && q.rel == causal_u_level(D)) return w.wres[q.block];
    return P[param];
  };
  if (use_pack) {
    rc = plan_pack_weights(p, source_of, ws, stream);
    if (rc) return rc;
  }
  auto packed = [&](int param) { return plan_packed(p, ws, use_pack, param); };
  // ---- front end: causal encoder, bottleneck (no norm)
  const SrfCausalFront<const float> f = causal_front<const float>(P);
  float* enc = fptr(p->off_enc);
  rc = srf_causal_encoder(wav, f.enc_w, enc, Bt, p->A, p->T, N, K, L, stream);
  if (rc) return rc;
  float* cur = fptr(p->off_xa);
  float* nxt = fptr(p->off_xb);
  float* y1 = fptr(p->off_y1);
  float* merged = fptr(p->off_merged);
  rc = srf_pw_conv_packed(enc, f.bott_w, packed(SRF_PC_BOTTLENECK), f.bott_b, cur, Bt, N, B, L, nullptr, nullptr, nullptr, 0, nullptr, 0,
                          stream);
  if (rc) return rc;
  // ---- separation module.  res_conv of block i + proj_1x1 of block i + 1 as one launch where the pair kernel takes the
  // shape (its no-prologue form: residual required), as in the Improved forward
  const bool fused = plan_fused_pyramid_now(p);
  const bool pair = use_pack && !srf_dbg(SRF_DBG_NO_PAIRS) && srf_pw_conv_pair_supported(Bt, Cc, B, Cc, L);
  bool y1_ready = false;
  for (int i = 0; i < U; ++i) {
    const SrfCausalBlock<const float> b = causal_block<const float>(lay, P, i);
    if (!y1_ready) {
      rc = srf_pw_conv_packed(cur, w.wproj[i], packed(b.i_proj), b.proj_b, y1, Bt, B, Cc, L, nullptr, nullptr, nullptr, 0, nullptr, 0,
                              stream);
      if (rc) return rc;
    }
    y1_ready = false;
    if (fused) {
      rc = srf_causal_pyramid(y1, merged, b.proj_prelu, b.lv_w, b.lv_b, b.lv_prelu, Bt, Cc, L, D, stream);
      if (rc) return rc;
    } else {
      const float* levels[SRF_MAX_DEPTH];
      for (int k = 0; k < D; ++k) {
        float* dk = fptr(p->off_lv[k]);
        rc = srf_causal_dwconv(k == 0 ? y1 : levels[k - 1], b.lv_w[k], b.lv_b[k], k == 0 ? b.proj_prelu : nullptr, b.lv_prelu[k], dk,
                               Bt, Cc, k == 0 ? L : (L >> (k - 1)), k == 0 ? 1 : 2, stream);
        if (rc) return rc;
        levels[k] = dk;
      }
      rc = srf_causal_merge(levels, D, merged, Bt, Cc, L, stream);
      if (rc) return rc;
    }
    if (pair && i + 1 < U && packed(b.i_res) && packed(causal_p_proj(lay, i + 1))) {
      const SrfCausalBlock<const float> nb = causal_block<const float>(lay, P, i + 1);
      rc = srf_pw_conv_pair(merged, packed(b.i_res), w.bres[i], nxt, nullptr, cur, packed(nb.i_proj), nb.proj_b, y1, nullptr, Bt, Cc,
                            B, Cc, L, stream);
      y1_ready = true;
    } else {
      rc = srf_pw_conv_packed(merged, w.wres[i], packed(b.i_res), w.bres[i], nxt, Bt, Cc, B, L, nullptr, cur, nullptr, 0, nullptr, 0,
                              stream);
    }
    if (rc) return rc;
    float* t = cur;
    cur = nxt;
    nxt = t;
  }
  // ---- mask_net (PReLU on load + 1x1) -> mask_nl_class PReLU on the decoder frame GEMM's load -> overlap-add + crop
  const SrfCausalTail<const float> t = causal_tail<const float>(lay, P);
  float* masks = fptr(p->off_masked);
  {
    srf_norm pre{nullptr, nullptr, nullptr, t.mask_prelu};
    rc = srf_pw_conv_packed(cur, t.mask_w, packed(causal_p_mask(lay)), t.mask_b, masks, Bt, B, p->SA * N, L, &pre, nullptr, nullptr, 0,
                            nullptr, 0, stream);
    if (rc) return rc;
  }
  return srf_decoder_impl(masks, t.dec_w, out, Bt, p->SA * N, p->SA, K, L, p->T, fptr(p->off_dec), nullptr, nullptr, 0, stream,
                          t.out_prelu);
}
