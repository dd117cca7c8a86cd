// Training step, device side: forward that keeps what the backward needs, and the backward
// of the whole SuDoRM-RF graph (improved_sudormrf.py:283-301 / groupcomm_sudormrf_v2.py:302-322 under autograd), as sequences of the
// per-kernel entry points of this library.  The reference gets the same result from torch autograd over ~1.8 k
// ATen nodes (run_improved_sudormrf.py:167-172: rec = model(x); l = clamp(loss(rec, clean)); l.backward()).
//
//   srf_forward_train : the inference forward's walk (improved_walk, srf_improved_walk.h: encoder -> bottleneck -> U x [proj,
//                       pyramid, res_conv], every GlobLN folded into its neighbours) over `saved`, which keeps what the
//                       backward reads: GlobLN statistics, encoder output, the residual stream x_0..x_U, per block y1, the
//                       D pre-norm levels (written on the side by the fused pyramid, or per level) and the merged tensor;
//                       then its own tail: the mask pre-activation m, the masked encoding v, the decoder.
//   srf_backward      : walks the graph in reverse; parameter gradients are ACCUMULATED into `grads` (same
//                       order / shapes as the parameters; the caller zeroes them, like optimizer.zero_grad()).
//                       In stages over one BwdWalk: tail (decoder, mask, mask_net), U x block (res_conv, the pyramid,
//                       proj_1x1, GroupComm: TAC), front (bottleneck, the deferred parameter sums, encoder).  How a
//                       block's pyramid runs -- which kernel form per level -- is a table (PyrBwdPath) filled before
//                       the first launch, from the shape, the kernel mode, the debug flags and the forward's record;
//                       a backward that cannot follow its forward is refused there, with `grads` untouched.
// GroupComm: each block is preceded by TAC (MLP + TAC_norm + residual, groupcomm_sudormrf_v2.py:356-384) and the
// U-ConvBlock runs on the (batch x group)-folded tensor with channels / G (:388-418); `saved` additionally keeps the
// TAC MLP output q and the block input u = x + GlobLN(q).
#include <map>
#include <memory>
#include <mutex>

#include "srf_improved_walk.h"

// Round 6: levels 1 and 0 of a block's pyramid backward and proj_1x1's norm backward run on the fused-head kernels
// (srf_backward.hip: srf_bwd_l1h_kernel, srf_bwd_l0p_kernel), which re-compute d_0 from y1 -- so srf_forward_train does not WRITE
// d_0 either.  The forward decides from the plan, the kernel mode and the debug flags, and RECORDS what it did (below); the
// backward follows that record, not the mode / flags of its own time: a forward that left d_0 out gets the head (or SRF_EINVAL
// when the head cannot run now), a forward that wrote d_0 gets the head or the row kernels, whichever the backward's own
// settings and shapes allow.  Every buffer involved is a 256-byte-aligned slice of saved / scratch.
static bool train_fused_head(const srf_plan* p) {
  return p->cfg.upsampling_depth > 1 && srf_bwd_level0_proj_ok(p->L, nullptr, 0);
}

// What a srf_forward_train did to its `saved` buffer, for the srf_backward that reads it: whether d_0 was left out,
// and the kernel mode / debug flags the forward ran under (for the error message).  Host-side, keyed by (device, address) like
// the packed3 format table (srf_pwconv.hip), so the backward needs no read of device memory.  A forward replaces every record
// its `saved` extent overlaps (the allocator re-uses addresses); at most kTrainRecMax records are kept, the oldest goes first.
struct TrainRec {
  size_t bytes;
  unsigned long long seq;
  bool skip_d0;
  int mode, flags;
};
static std::mutex g_trec_mu;
static std::map<unsigned long long, TrainRec> g_trec;     // key: device << 56 | address (ordered: range queries)
static unsigned long long g_trec_seq = 0;
static const size_t kTrainRecMax = 1024;
static unsigned long long train_rec_key(const void* p) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  return ((unsigned long long)dev << 56) | ((unsigned long long)(size_t)p & ((1ull << 56) - 1));
}
// valid = false: only drop what the extent overlaps (a forward that failed leaves no record behind)
static void train_rec_put(const void* saved, size_t bytes, bool valid, bool skip_d0, int mode, int flags) {
  const unsigned long long k0 = train_rec_key(saved), k1 = k0 + bytes;
  std::lock_guard<std::mutex> lk(g_trec_mu);
  auto it = g_trec.lower_bound(k0);
  if (it != g_trec.begin()) {
    auto prev = std::prev(it);
    if (prev->first + prev->second.bytes > k0) it = prev;
  }
  while (it != g_trec.end() && it->first < k1) it = g_trec.erase(it);
  if (!valid) return;
  if (g_trec.size() >= kTrainRecMax) {
    auto oldest = g_trec.begin();
    for (auto j = g_trec.begin(); j != g_trec.end(); ++j)
      if (j->second.seq < oldest->second.seq) oldest = j;
    g_trec.erase(oldest);
  }
  g_trec[k0] = TrainRec{bytes, ++g_trec_seq, skip_d0, mode, flags};
}
static bool train_rec_get(const void* saved, TrainRec* out) {
  std::lock_guard<std::mutex> lk(g_trec_mu);
  const auto it = g_trec.find(train_rec_key(saved));
  if (it == g_trec.end()) return false;
  *out = it->second;
  return true;
}

struct TrainLayout {
  size_t stats, enc, x0, x_stride, blk0, blk_stride, y1, lv[SRF_MAX_DEPTH], merged, q, u, m, v, total;
};

static TrainLayout train_layout(const srf_plan* p) {
  TrainLayout t;
  const srf_config& c = p->cfg;
  const size_t F = sizeof(float), L = p->L, Bt = p->Bt;
  const int D = c.upsampling_depth, U = c.num_blocks;
  SrfCarve all, blk;      // (blk: one block's slices, offsets relative to the block's start)
  t.stats = all.take(p->stats_bytes);
  t.enc = all.take(F * Bt * c.enc_num_basis * L);
  t.x_stride = srf_align_up(F * Bt * c.out_channels * L, 256);
  t.x0 = all.take(t.x_stride * (U + 1));
  t.y1 = blk.take(F * Bt * c.in_channels * L);
  for (int k = 0; k < SRF_MAX_DEPTH; ++k) t.lv[k] = k < D ? blk.take(F * Bt * c.in_channels * (L >> k)) : 0;
  t.merged = blk.take(F * Bt * c.in_channels * L);
  const bool gc = c.variant == SRF_VARIANT_GROUPCOMM;
  t.q = gc ? blk.take(F * Bt * c.out_channels * L) : 0;
  t.u = gc ? blk.take(F * Bt * c.out_channels * L) : 0;
  t.blk_stride = blk.off;
  t.blk0 = all.take(blk.off * U);
  t.m = all.take(F * Bt * p->SA * c.enc_num_basis * L);
  t.v = all.take(F * Bt * p->SA * c.enc_num_basis * L);
  t.total = all.off;
  return t;
}

struct ScratchLayout {
  size_t dec, gv, genc, gxa, gxb, gf, go, gd, gn[SRF_MAX_DEPTH], gu[SRF_MAX_DEPTH], frames, wt, zeros, wdpad, wg,
      gln, gln2, dw, gq, gxm, tac, pk3, pkT, arena, arena_bytes, gln_slice, dw_slice, total;
  int dec_rows;
};

static ScratchLayout scratch_layout(const srf_plan* p) {
  ScratchLayout s;
  const srf_config& c = p->cfg;
  const size_t F = sizeof(float), L = p->L, Bt = p->Bt;
  const int D = c.upsampling_depth, K = c.enc_kernel_size, N = c.enc_num_basis, B = c.out_channels, C = c.in_channels;
  const int SAN = p->SA * N;
  SrfCarve all;
  s.dec = all.take(F * srf_decoder_scratch_floats(p->Bt, SAN, p->SA, K, p->L));
  s.gv = all.take(F * Bt * SAN * L);
  s.genc = all.take(F * Bt * N * L);
  s.gxa = all.take(F * Bt * B * L);
  s.gxb = all.take(F * Bt * B * L);
  s.gf = all.take(F * Bt * C * L);
  s.go = all.take(F * Bt * C * L);
  s.gd = all.take(F * Bt * C * L);
  for (int k = 0; k < SRF_MAX_DEPTH; ++k) {
    s.gn[k] = (k >= 1 && k < D) ? all.take(F * Bt * C * (L >> k)) : 0;
    s.gu[k] = (k >= 1 && k < D) ? all.take(F * Bt * C * (L >> k)) : 0;   // gradient w.r.t. normalised level k from level k+1
  }
  s.dec_rows = (p->SA * K + 63) / 64 * 64;
  const size_t enc_rows = (size_t)p->A * K;
  s.frames = all.take(F * Bt * L * (s.dec_rows > (int)enc_rows ? s.dec_rows : enc_rows));
  s.wt = all.take(F * std::max({(size_t)B * N, (size_t)B * C, (size_t)B * SAN}));
  s.zeros = all.take(F * std::max({C, SAN, N}));
  s.wdpad = all.take(F * (size_t)SAN * s.dec_rows);
  size_t wg = 0;
  auto wgmax = [&](int cout, int cin) {
    const size_t b = srf_pw_wgrad_scratch_bytes(p->Bt, cout, cin, p->L);
    if (b > wg) wg = b;
  };
  wgmax(B, N);
  wgmax(SAN, B);
  wgmax(SAN, s.dec_rows);
  wgmax(N, (int)enc_rows);
  {
    const size_t b1 = srf_pw_wgrad_scratch_bytes(p->Bg, p->nC, p->nB, p->L), b2 = srf_pw_wgrad_scratch_bytes(p->Bg, p->nB, p->nC, p->L);
    if (b1 > wg) wg = b1;
    if (b2 > wg) wg = b2;
  }
  s.wg = all.take(wg);
  s.gln = all.take(std::max({srf_gln_bwd_scratch_bytes(p->Bg, p->nC), srf_gln_bwd_scratch_bytes(p->Bt, N),
                              srf_gln_bwd_scratch_bytes(p->Bg, p->nB)}));
  s.gln2 = all.take(srf_gln_bwd_scratch_bytes(p->Bg, p->nC));   // the pyramid's norms alternate between gln and gln2
  s.dw = all.take(srf_dwconv5_bwd_scratch_bytes(p->Bg, p->nC));
  const bool gc = c.variant == SRF_VARIANT_GROUPCOMM;
  s.gq = gc ? all.take(F * Bt * B * L) : 0;
  s.gxm = gc ? all.take(F * Bt * B * L) : 0;
  s.tac = gc ? all.take(srf_tac_bwd_scratch_bytes(p->Bt, c.group_size, p->nB, p->L)) : 0;
  // per-call scratch slices of the blocks' norm / depthwise-conv backwards (zeroed once per backward; their parameter-gradient
  // reductions are deferred to one batched flush: srf_backward.hip, SrfDeferCtx): per block D + 2 norm slices and D conv slices
  s.gln_slice = srf_align_up(srf_gln_bwd_scratch_bytes(p->Bg, p->nC), 256);
  s.dw_slice = srf_align_up(srf_dwconv5_bwd_scratch_bytes(p->Bg, p->nC), 256);
  s.arena_bytes = (size_t)c.num_blocks * ((size_t)(D + 2) * s.gln_slice + (size_t)D * s.dw_slice);
  s.arena = all.take(s.arena_bytes);
  // two-part images of the TRANSPOSED weights for the backward's data-gradient GEMMs (packed once per backward)
  {
    size_t pk = srf_align_up(srf_packed_pw_weight_bytes(B, SAN), 256) + srf_align_up(srf_packed_pw_weight_bytes(N, B), 256);
    pk += (size_t)c.num_blocks * (srf_align_up(srf_packed_pw_weight_bytes(p->nC, p->nB), 256) + srf_align_up(srf_packed_pw_weight_bytes(p->nB, p->nC), 256));
    s.pkT = all.take(pk);
  }
  // three-part weight images of the forward's 1x1 convolutions (packed once per step by srf_forward_train)
  {
    size_t pk = srf_align_up(srf_packed3_pw_weight_bytes(B, N), 256) + srf_align_up(srf_packed3_pw_weight_bytes(SAN, B), 256);
    pk += (size_t)c.num_blocks * (srf_align_up(srf_packed3_pw_weight_bytes(p->nC, p->nB), 256) + srf_align_up(srf_packed3_pw_weight_bytes(p->nB, p->nC), 256));
    s.pk3 = all.take(pk);
  }
  s.total = all.off;
  return s;
}

static int train_check(const srf_plan* p, const char* who) {
  if (p->cfg.variant == SRF_VARIANT_GROUPCOMM) {
    const int n = p->nB, G = p->cfg.group_size;
    const bool n_ok = n == 2 || n == 4 || n == 8 || n == 16, g_ok = G == 2 || G == 4 || G == 8 || G == 16;
    if (!n_ok || !g_ok) {
      srf_set_error("%s: TAC backward supports out_channels/group_size in {2,4,8,16} and group_size in {2,4,8,16} "
                    "(got %d, %d)", who, n, G);
      return SRF_EINVAL;
    }
  }
  if (p->L % 4 != 0) {
    srf_set_error("%s: L=%d must be a multiple of 4", who, p->L);
    return SRF_EINVAL;
  }
  return SRF_OK;
}

// The entry points of this file train the Improved and GroupComm models.  The plans of every other family are refused before
// anything is launched, with where that family trains: the causal and the original model through entry points of their own
// (srf_causal_train.hip, srf_original_train.hip), the attentive models nowhere (inference forward only).  A null plan is refused too.  The two
// size queries return 0 with the same message in srf_last_error().
static bool other_family_refused(const srf_plan* p, const char* who) {
  if (!p) {
    srf_set_error("%s: null plan", who);
    return true;
  }
  if (p->cfg.variant == SRF_VARIANT_ATTENTIVE) {
    srf_set_error("%s: not available for the attentive variant (attentive SuDORMRF v2 has an inference forward only)", who);
    return true;
  }
  if (p->cfg.variant == SRF_VARIANT_ATTENTIVE_V3) {
    srf_set_error("%s: not available for the attentive v3 variant (attentive SuDORMRF v3 has an inference forward only)", who);
    return true;
  }
  if (p->cfg.variant == SRF_VARIANT_ORIGINAL) {
    srf_set_error("%s: not available for the original variant (the original SuDORMRF trains through srf_original_forward_train / "
                  "srf_original_backward)", who);
    return true;
  }
  if (p->cfg.variant != SRF_VARIANT_CAUSAL) return false;
  srf_set_error("%s: not available for the causal variant (CausalSuDORMRF trains through srf_causal_forward_train / "
                "srf_causal_backward)", who);
  return true;
}
extern "C" size_t srf_train_saved_bytes(const srf_plan* p) {
  return !other_family_refused(p, "srf_train_saved_bytes") ? train_layout(p).total : 0;
}
extern "C" size_t srf_train_scratch_bytes(const srf_plan* p) {
  return !other_family_refused(p, "srf_train_scratch_bytes") ? scratch_layout(p).total : 0;
}

int srf_train_entry_check(const char* who, const srf_plan* p, const float* const* P, float* const* G, int num_params,
                          int null_grad_tail, std::initializer_list<const void*> others, const SrfTrainBuffers& b) {
  bool all = p && P && b.saved && b.scratch;
  for (const void* o : others) all = all && o;
  SRF_CHECK_ARG(all, "%s: null pointer", who);
  SRF_CHECK_ARG(num_params == p->n_params, "%s: expected %d parameter tensors, got %d", who, p->n_params, num_params);
  for (int i = 0; i < num_params; ++i) {
    SRF_CHECK_ARG(P[i], "%s: parameter %d is null", who, i);
    SRF_CHECK_ARG(!G || G[i] || i >= num_params - null_grad_tail, "%s: gradient %d is null", who, i);
  }
  SRF_CHECK_ARG(b.saved_bytes >= b.saved_need, "%s: saved buffer too small (%zu bytes, needs %zu)", who, b.saved_bytes, b.saved_need);
  SRF_CHECK_ARG(b.scratch_bytes >= b.scratch_need, "%s: scratch buffer too small (%zu bytes, needs %zu)", who, b.scratch_bytes,
                b.scratch_need);
  SRF_CHECK_ARG(((((size_t)b.saved) | ((size_t)b.scratch)) & 255) == 0, "%s: saved and scratch must be 256-byte aligned", who);
  return SRF_OK;
}

// The training forward's walk and tail.  split_tail: the exact class was srf_forward_train's own choice;  *skip_d0_out: d_0 was
// left out (srf_forward_train records it for the backward).
static int forward_train_impl(const srf_plan* p, const float* const* P, int num_params, const float* wav, float* out,
                              void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes, bool split_tail, bool* skip_d0_out,
                              void* stream) {
  const TrainLayout t = train_layout(p);
  const ScratchLayout s = scratch_layout(p);
  int rc = srf_train_entry_check("srf_forward_train", p, P, nullptr, num_params, 0, {wav, out},
                                 {saved, saved_bytes, t.total, scratch, scratch_bytes, s.total});
  if (!rc) rc = train_check(p, "srf_forward_train");
  if (rc) return rc;
  const srf_config& c = p->cfg;
  const int D = c.upsampling_depth, U = c.num_blocks, N = c.enc_num_basis, K = c.enc_kernel_size;
  const int Bt = p->Bt, L = p->L, B = c.out_channels;
  char *sv = (char*)saved, *sc = (char*)scratch;
  double* stats = (double*)(sv + t.stats);
  SRF_CHECK_HIP(hipMemsetAsync(stats, 0, p->stats_bytes, (hipStream_t)stream));
  const bool gc = c.variant == SRF_VARIANT_GROUPCOMM;
  const int Bg = p->Bg, nB = p->nB, nC = p->nC;
  // the exact-class images of the 1x1 weights (SrfPackQueue::add3), split and laid out once per step, here
  SrfPackQueue pk{sc + s.pk3};
  std::vector<const void*> image(p->n_params, nullptr);      // parameter index -> its packed image (NULL: none)
  const SrfTail<const float> tl = plan_tail(p, P);
  const int i_mask = plan_p_mask(p), i_proj = plan_p_proj(p, 0), i_res = plan_p_res(p, 0);
  image[SRF_P_BOTTLENECK] = pk.add3(P[SRF_P_BOTTLENECK], B, N);
  for (int i = 0; i < U; ++i) {
    image[plan_p_proj(p, i)] = pk.add3(P[plan_p_proj(p, i)], nC, nB);
    image[plan_p_res(p, i)] = pk.add3(P[plan_p_res(p, i)], nB, nC);
  }
  image[i_mask] = pk.add3(tl.mask_w, p->SA * N, B);
  rc = pk.pack3(stream);
  if (rc) return rc;
  auto conv = [&](int, const float* x, const float* w, int param, const float* bias, float* y, int rows, int Cin, int Cout,
                  const srf_norm* in_norm, const float* residual, double* out_sums) {
    return srf_pw_conv_packed3(x, w, image[param], bias, y, rows, Cin, Cout, L, in_norm, residual, out_sums, stream);
  };
  auto pair = [&](const float* x, int param1, const float* bias1, float* y, const srf_norm* in_norm, const float* residual, int param2,
                  const float* bias2, float* y2, double* out_sums2, int Cin1, int Cmid, int Cout2) {
    return srf_pw_conv_pair_packed3(x, image[param1], bias1, y, in_norm, residual, image[param2], bias2, y2, out_sums2, Bt, Cin1, Cmid,
                                    Cout2, L, stream);
  };
  // Round 5: like srf_forward, the B = 256 Improved models run bottleneck + proj_1x1(0) and res_conv(i) + proj_1x1(i + 1) as ONE
  // launch each (srf_pwconv_x3f.hip on the two-fp16-part images: outputs bit-identical to the two launches), each where its own two
  // images and its shape allow (every block's images have one shape: block 0's stand for all).  Debug flag 1 = without.
  const bool pair_head = !gc && image[SRF_P_BOTTLENECK] && image[i_proj] && srf_pw_conv_pair_packed3_supported(Bt, N, B, nC, L);
  const bool pair_block = !gc && image[i_res] && image[i_proj] && srf_pw_conv_pair_packed3_supported(Bg, nC, nB, nC, L);
  // fused pyramid with level outputs (register-resident kernels only); its scratch lives in the backward's gradient
  // buffers gf | go | gd, idle during the forward.  SRF_DBG_PYR_PER_LEVEL (as in srf_forward) selects the per-level kernels.
  // Not plan_fused_pyramid_now(p): p->fused_pyramid was decided under the flags of the plan's creation and also admits the
  // LDS kernels; this test needs the register kernels, under the flags of this call.
  const bool fused_pyr = !srf_dbg(SRF_DBG_PYR_PER_LEVEL | SRF_DBG_PYR_NO_REG | SRF_DBG_PYR_PASS1_NONPERSISTENT) && srf_kernel_mode() != 1 &&
                         srf_pyramid_supported(nC, L, D) && srf_pyramid_reg_supported(L, D) &&
                         srf_pyramid_scratch_bytes(Bg, nC, L, D) <= (s.gd + sizeof(float) * Bt * c.in_channels * L) - s.gf;
  const bool skip_d0 = fused_pyr && train_fused_head(p);     // (the backward re-computes d_0: nothing reads it)
  *skip_d0_out = skip_d0;
  SrfImpAddrs a{};
  a.stats = stats;
  a.enc = (float*)(sv + t.enc);
  a.x[0] = a.x[1] = sv + t.x0, a.x_stride = t.x_stride;
  a.blk = sv + t.blk0, a.blk_stride = t.blk_stride;
  a.o_y1 = t.y1, a.o_merged = t.merged, a.o_q = t.q, a.o_u = t.u;
  for (int k = 0; k < D; ++k) a.o_lv[k] = t.lv[k];
  a.lv_mask = skip_d0 ? ~1u : ~0u;
  a.pyr = sc + s.gf;
  rc = improved_walk(p, P, wav, a, conv, pair, pair_head, pair_block, fused_pyr, nullptr, nullptr, stream);
  if (rc) return rc;

  float* m = (float*)(sv + t.m);
  float* v = (float*)(sv + t.v);
  {
    srf_norm pre{nullptr, nullptr, nullptr, tl.mask_prelu};
    rc = srf_pw_conv_packed3(a.x_in(U), tl.mask_w, image[i_mask], tl.mask_b, m, Bt, B, p->SA * N, L, &pre, nullptr, nullptr, stream);
    if (rc) return rc;
  }
  rc = srf_mask_apply(m, a.enc, v, Bt, p->SA, N, L, stream);
  if (rc) return rc;
  // The decoder's frame GEMM (S N -> S K rows) is the LAST linear map of the forward: nothing downstream amplifies the 2^-17
  // rounding of the split-bf16 GEMM (the loss is smooth in the estimates), unlike the early layers' (srf_train_fwd_exact) -- so when
  // the exact class was this function's own choice it runs on the split kernel (round 6: 292 -> 130 us at cfg 2, 4 x that at N = 2048)
  // instead of the exact-fp32 MFMA kernel the thin output (42 rows) would otherwise fall to.
  const SrfKernelModeScope split_class(split_tail, 0);
  return srf_decoder(v, tl.dec_w, out, Bt, p->SA * N, p->SA, K, L, p->T, (float*)(sc + s.dec), stream);
}

// The 1x1 convolutions run in the exact-fp32 class where srf_train_fwd_exact() says so (srf_plan.h has the reasons).  What the
// forward did to `saved` is recorded for the backward, under the kernel mode and the debug flags of the call.
extern "C" int srf_forward_train(const srf_plan* p, const float* const* P, int num_params, const float* wav, float* out,
                                 void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes, void* stream) {
  if (other_family_refused(p, "srf_forward_train")) return SRF_EINVAL;
  const int mode = srf_kernel_mode(), flags = srf_debug_flags();
  const bool exact = srf_train_fwd_exact();
  bool skip_d0 = false;
  int rc;
  {
    const SrfKernelModeScope exact_class(exact, 2);
    rc = forward_train_impl(p, P, num_params, wav, out, saved, saved_bytes, scratch, scratch_bytes, exact, &skip_d0, stream);
  }
  if (saved) train_rec_put(saved, saved_bytes, rc == SRF_OK, skip_d0, mode, flags);
  return rc;
}

// ---- srf_backward: the graph in reverse, in stages over one walk state (as the forwards of srf_api.hip) ----------------------

// How one block's pyramid backward runs, level by level, decided ONCE per backward and before any device work.  Level k's conv
// backward can also produce the COMPLETE gradient w.r.t. its (normalised) input -- its own input gradient + the merge part -- and
// the reduce pass of that input's GlobLN backward (the input tensor is in its registers); and it can evaluate the apply pass of
// its OWN level's norm on load.  Where the row kernels serve every level that is one conv kernel per level, g_d never written.
enum PyrBwdForm {
  PYR_BWD_SEQ,          // norm backward (reduce unless pre-reduced, apply into the g_d buffer), then the conv backward on the chunked kernels
  PYR_BWD_ROW,          // the same two calls; the conv's row kernel also reduces the norm of the level below
  PYR_BWD_ROW_ONLOAD,   // norm: reduce only (if at all); the row kernel applies it on load
  PYR_BWD_HEAD1,        // level 1 on the fused-head kernel: as ROW_ONLOAD with conv 1's input re-computed from y1 (d_0 is not read)
  PYR_BWD_HEAD0,        // level 0 + proj_1x1's norm as the fused head (two passes over {G_0, y1}); g_y1 lands in the g_d buffer
};
struct PyrBwdPath {
  PyrBwdForm form[SRF_MAX_DEPTH];
  bool pre[SRF_MAX_DEPTH];    // level k's incoming gradient arrives complete in ONE buffer, its norm's reduce pass done (by level k + 1)
  bool proj_pre;              // ... and proj_1x1's norm (by level 0; without the head)
};

// The path is a function of L, D, the kernel mode and debug flags of NOW, where `saved` and `scratch` lie (every operand is a
// 256-byte-aligned slice of one of the two: the predicates get the two bases) and of the forward that filled `saved`: levels 1
// and 0 follow its record; no record -- a buffer no srf_forward_train of this process filled, or one evicted from the table -- is
// taken as "d_0 may be missing".  d_0 left out: the fused head must run, whatever the mode / flags say now.  This is the ONE place
// where a backward that cannot follow its forward is refused: nothing has been launched, `grads` is untouched.
static int pyr_bwd_path(const srf_plan* p, const void* saved, const void* scratch, const char* who, PyrBwdPath* path) {
  const int D = p->cfg.upsampling_depth, L = p->L;
  TrainRec rec{};
  const bool known = train_rec_get(saved, &rec);
  const bool d0_missing = D > 1 && (!known || rec.skip_d0);
  auto head_lost = [&](const char* where) {
    if (known)
      srf_set_error("%s: the srf_forward_train that filled `saved` left d_0 out for the fused backward head (kernel mode %d, debug "
                    "flags 0x%x), but the head cannot run %s under kernel mode %d / debug flags 0x%x -- run the backward under the "
                    "forward's settings", who, rec.mode, (unsigned)rec.flags, where, srf_kernel_mode(), (unsigned)srf_debug_flags());
    else
      srf_set_error("%s: no srf_forward_train of this process filled `saved` (%p): d_0 may be missing, and the fused backward head "
                    "that re-computes it cannot run %s under kernel mode %d / debug flags 0x%x", who, saved, where, srf_kernel_mode(),
                    (unsigned)srf_debug_flags());
    return SRF_EINVAL;
  };
  if (d0_missing) {
    if (!srf_bwd_level0_proj_shape_ok(L, nullptr, 0)) return head_lost("at level 0 (L)");
    if (!srf_dwconv5_bwd_rowwise_ok(L, 2, nullptr, 0)) return head_lost("at level 1 (the row kernels)");
  }
  const void* base[2] = {saved, scratch};
  bool head = d0_missing || train_fused_head(p);   // (re-computes d_0: needed when the forward left it out, harmless otherwise)
  bool pre = false;
  for (int k = D - 1; k >= 0; --k) {
    path->pre[k] = pre;
    if (k == 0 && head) {     // (head still set: level 1 ran on the head kernel, so G_0 is complete and norm 0 reduced)
      if (pre && srf_bwd_level0_proj_shape_ok(L, base, 2)) {
        path->form[0] = PYR_BWD_HEAD0;
        break;
      }
      if (d0_missing) return head_lost("at level 0");
    }
    const bool rows = srf_dwconv5_bwd_rowwise_ok(k ? L >> (k - 1) : L, k ? 2 : 1, base, 2);
    // apply-on-load needs the level's gradient in one buffer: pre-reduced, or the deepest level's (only the merge part)
    const bool on_load = rows && (pre || k == D - 1);
    if (k == 1 && head && !on_load) {
      if (d0_missing) return head_lost("at level 1 (the row kernels)");
      head = false;           // d_0 is in `saved`: levels 1 and 0 on the conv kernels
    }
    path->form[k] = (k == 1 && head) ? PYR_BWD_HEAD1 : on_load ? PYR_BWD_ROW_ONLOAD : rows ? PYR_BWD_ROW : PYR_BWD_SEQ;
    pre = rows;
  }
  path->proj_pre = pre;
  return SRF_OK;
}

// One backward: what its stages share, and the stages
struct BwdWalk {
  const srf_plan* p;
  const float* const* P;      // parameters, and their gradients (accumulated into)
  float* const* G;
  const TrainLayout t;
  const ScratchLayout s;
  const char* sv;
  char* sc;
  hipStream_t st;
  SrfBwdCtx* ctx;
  const int D, U, N, K, Bt, L, B, SA, SAN, Bg, nB, nC;
  PyrBwdPath path;
  const void *pkT_mask, *pkT_bott;              // packed images of the TRANSPOSED weights (NULL: none)
  std::vector<const void*> pkT_res, pkT_proj;
  float *gx, *gx_other;       // gradient w.r.t. the residual stream x_i (ping-pong)
  float *go, *gd;             // a block's g_o / g_y1 and its g_d buffer (they swap roles after a block that ran the fused head)
  bool gf_ready;              // block i's g_f was produced by block i + 1's data-gradient pair

  BwdWalk(const srf_plan* p, const float* const* P, float* const* G, const void* saved, void* scratch, void* stream, SrfBwdCtx* ctx)
      : p(p), P(P), G(G), t(train_layout(p)), s(scratch_layout(p)), sv((const char*)saved), sc((char*)scratch),
        st((hipStream_t)stream), ctx(ctx), D(p->cfg.upsampling_depth), U(p->cfg.num_blocks), N(p->cfg.enc_num_basis),
        K(p->cfg.enc_kernel_size), Bt(p->Bt), L(p->L), B(p->cfg.out_channels), SA(p->SA), SAN(p->SA * N), Bg(p->Bg), nB(p->nB),
        nC(p->nC), gx(fp(s.gxa)), gx_other(fp(s.gxb)), go(fp(s.go)), gd(fp(s.gd)), gf_ready(false) {}
  float* fp(size_t o) const { return (float*)(sc + o); }
  double* stats() const { return (double*)(sv + t.stats); }      // (the slot of ln is the first)
  const float* xbuf(int i) const { return (const float*)(sv + t.x0 + t.x_stride * i); }
  const float* enc() const { return (const float*)(sv + t.enc); }
  const char* blk(int i) const { return sv + t.blk0 + t.blk_stride * i; }
  // g = W^T g_in (+ skip) of a 1x1 conv with forward weight w [cin][cout]
  int data_grad(const float* g_in, const float* w, const void* pkT, float* g, int batch, int cin, int cout, const float* skip) const {
    return srf_pw_data_grad(g_in, w, pkT, fp(s.wt), fp(s.zeros), g, batch, cin, cout, L, skip, st);
  }
  int pack_weights();
  int tail(const float* grad_out);
  int block(int i);
  int block_pyramid(int i);
  int block_tac(int i);
  int front(const float* wav, float* grad_wav);
};

// The data-gradient GEMMs g_x = W^T g run on the 256 x 128 split-bf16 kernel with the TRANSPOSED weights pre-split into its
// stage images, all of them in one launch here (shapes / launches that kernel does not take keep the transposed fp32 copy
// `wt` and the 128 x 128 kernels).
int BwdWalk::pack_weights() {
  SrfPackQueue pk{sc + s.pkT};
  auto packT = [&](const float* w, int cout_d, int cin_d) {   // w: forward weight [cin_d][cout_d]
    return pk.add(w, srf_kernel_mode() == 0 ? srf_packed_pw_weight_bytes(cout_d, cin_d) : 0, cout_d, cin_d);
  };
  pkT_mask = packT(plan_tail(p, P).mask_w, B, SAN);
  pkT_bott = packT(plan_front(P).bott_w, N, B);
  pkT_res.assign(U, nullptr);
  pkT_proj.assign(U, nullptr);
  for (int i = 0; i < U; ++i) {
    const SrfBlock<const float> b = plan_block(p, P, i);
    pkT_res[i] = packT(b.res_w, nC, nB);               // res_conv: forward [nB][nC], gradient GEMM nB -> nC
    pkT_proj[i] = packT(b.proj_w, nB, nC);             // proj_1x1: forward [nC][nB], gradient GEMM nC -> nB
  }
  return pk.packT(st);
}

// Decoder, mask, mask_net: grad_out -> gx = gradient w.r.t. x_U; leaves the mask path's g_enc in s.genc
int BwdWalk::tail(const float* grad_out) {
  const SrfTail<const float> tl = plan_tail(p, P);
  const SrfTail<float> gtl = plan_tail(p, G);
  const float *m = (const float*)(sv + t.m), *v = (const float*)(sv + t.v);
  const int h = K / 2;
  void* wg = sc + s.wg;
  // ---- decoder: out = overlap_add(W_d^T v)                       improved_sudormrf.py:272-279,300
  float* frames = fp(s.frames);
  int rc = srf_frames_gather(grad_out, frames, Bt, SA, p->T, K, h, h, L, s.dec_rows, st);
  if (rc) return rc;
  rc = srf_pw_wgrad_cols(v, frames, nullptr, Bt, s.dec_rows, SAN, L, gtl.dec_w, SA * K, nullptr, 1, wg, st);
  if (rc) return rc;
  float* wdpad = fp(s.wdpad);
  SRF_CHECK_HIP(hipMemsetAsync(wdpad, 0, sizeof(float) * (size_t)SAN * s.dec_rows, st));
  SRF_CHECK_HIP(hipMemcpy2DAsync(wdpad, sizeof(float) * s.dec_rows, tl.dec_w, sizeof(float) * SA * K,
                                 sizeof(float) * SA * K, SAN, hipMemcpyDeviceToDevice, st));
  float* gv = fp(s.gv);
  rc = srf_pw_conv(frames, wdpad, fp(s.zeros), gv, Bt, s.dec_rows, SAN, L, nullptr, nullptr, nullptr, 0, nullptr, 0, st);
  if (rc) return rc;
  // ---- mask: v = relu(m) * enc                                  :296-298
  rc = srf_mask_bwd(gv, m, enc(), gv, fp(s.genc), 0, Bt, SA, N, L, st);   // gv now holds g_m
  if (rc) return rc;
  // ---- mask_net: m = W_m PReLU(x_U) + b_m                       :268-269,295
  srf_norm pre{nullptr, nullptr, nullptr, tl.mask_prelu};
  rc = srf_pw_wgrad(gv, xbuf(U), &pre, Bt, B, SAN, L, gtl.mask_w, gtl.mask_b, 1, wg, st);
  if (rc) return rc;
  rc = data_grad(gv, tl.mask_w, pkT_mask, gx, Bt, SAN, B, nullptr);
  if (rc) return rc;
  return srf_prelu_bwd(gx, xbuf(U), tl.mask_prelu, gx, gtl.mask_prelu, (long)Bt * B * L, st);
}

// Block i's pyramid: g_f (in s.gf) -> go = g_y1: final_norm, merge, the D levels as the path table says, proj_1x1's norm.
// Norm slices of the block's arena: 0 final_norm, D - k level k (the order they run in), D + 1 proj_1x1's norm -- a conv kernel
// reads its own level's slice (reduced) and writes the next one.
int BwdWalk::block_pyramid(int i) {
  const SrfBlock<const float> b = plan_block(p, P, i);
  const SrfBlock<float> g = plan_block(p, G, i);
  const SrfSlots sl = plan_slots(p, stats(), i);
  const float* y1 = (const float*)(blk(i) + t.y1);
  const float* merged = (const float*)(blk(i) + t.merged);
  char* gln_sl = sc + s.arena + (size_t)i * ((size_t)(D + 2) * s.gln_slice + (size_t)D * s.dw_slice);   // D + 2 norm slices,
  char* dw_sl = gln_sl + (size_t)(D + 2) * s.gln_slice;                                                 // then D conv slices
  float* gn[SRF_MAX_DEPTH];       // the merge part of the gradient w.r.t. the normalised level k
  gn[0] = fp(s.gf);
  for (int k = 1; k < D; ++k) gn[k] = fp(s.gn[k]);
  const srf_norm fn{sl.merged, b.fin_g, b.fin_be, b.fin_prelu}, pn{sl.proj, b.proj_g, b.proj_be, b.proj_prelu};
  srf_bwd_ctx_merge_sink(ctx, gn, D);  // the merge backward rides on the norm's apply pass (the levels' pair sums of its output)
  int rc = srf_gln_bwd_impl(gn[0], nullptr, merged, &fn, Bg, nC, L, gn[0], 0, g.fin_g, g.fin_be, g.fin_prelu, gln_sl, 0, st, ctx);
  if (rc) return rc;                                       // gf now holds g_merged = g_n_0 (merge part)
  if (!srf_bwd_ctx_merge_taken(ctx)) {
    rc = srf_merge_bwd(gn[0], gn, D, (long)Bg * nC, L, st);
    if (rc) return rc;
  }
  const float* g_o = go;      // where level 0's conv leaves the gradient w.r.t. o = PReLU(GlobLN(y1))
  for (int k = D - 1; k >= 0; --k) {
    const PyrBwdForm form = path.form[k];
    const bool pre = path.pre[k], on_load = form == PYR_BWD_ROW_ONLOAD || form == PYR_BWD_HEAD1;
    const float* dk = (const float*)(blk(i) + t.lv[k]);
    const srf_norm nk{sl.level[k], b.lv_g[k], b.lv_be[k], nullptr};
    // gradient w.r.t. the normalised level k: merge part (gn[k]) + what level k + 1's conv sent down (pre: already their sum)
    const float* gu_in = (k < D - 1) ? (k == 0 ? go : fp(s.gu[k])) : nullptr;
    const float* gout1 = pre ? gu_in : gn[k];
    const float* gout2 = pre ? nullptr : gu_in;
    char* cur_sl = gln_sl + (size_t)(D - k) * s.gln_slice;
    char* next_sl = cur_sl + s.gln_slice;
    if (form == PYR_BWD_HEAD0) {      // (neither d_0 nor g_o travels; the two norms' parameter sums: recorded for the batched flush)
      rc = srf_bwd_ctx_gln_params(ctx, &nk, cur_sl, Bg, nC, g.lv_g[0], g.lv_be[0], nullptr, st);
      if (rc) return rc;
      rc = srf_bwd_level0_proj(gout1, y1, &pn, &nk, b.lv_w[0], b.lv_b[0], cur_sl, next_sl, dw_sl, g.lv_w[0], g.lv_b[0], gd, Bg, nC, L, st,
                               ctx);
      if (rc) return rc;
      std::swap(go, gd);      // g_y1 sits in the former g_d buffer: the two swap roles for the rest of the backward
      return srf_bwd_ctx_gln_params(ctx, &pn, next_sl, Bg, nC, g.proj_g, g.proj_be, g.proj_prelu, st);
    }
    // the conv's input: the normalised level k - 1 (stride 2), at level 0 o = PReLU(GlobLN(y1)); its gradient goes to g_u[k - 1],
    // at levels 1 and 0 to `go` -- but apply-on-load at level 0 reads G_0 from `go` (with halos) while the same kernel writes its
    // input gradient: that one goes to the g_d buffer, which the on-load form leaves unused
    const srf_norm in = k ? srf_norm{sl.level[k - 1], b.lv_g[k - 1], b.lv_be[k - 1], nullptr} : pn;
    const float* src = k ? (const float*)(blk(i) + t.lv[k - 1]) : y1;
    float* gin = k > 1 ? fp(s.gu[k - 1]) : (k == 0 && on_load && pre) ? gd : go;
    const float* gadd = k > 0 ? gn[k - 1] : nullptr;
    if (k == 0) g_o = gin;
    rc = srf_gln_bwd_impl(gout1, gout2, dk, &nk, Bg, nC, L >> k, gd, 0, g.lv_g[k], g.lv_be[k], nullptr, cur_sl,
                          (pre ? 1 : 0) | (on_load ? 2 : 0), st, ctx);
    if (rc) return rc;
    if (form == PYR_BWD_HEAD1)
      rc = srf_bwd_level1_head(gout1, dk, &nk, cur_sl, y1, &pn, &in, b.lv_w[0], b.lv_b[0], b.lv_w[k], gadd, gin, next_sl,
                               dw_sl + (size_t)k * s.dw_slice, g.lv_w[k], g.lv_b[k], Bg, nC, L, st, ctx);
    else
      rc = srf_dwconv5_bwd_impl(on_load ? gout1 : gd, src, &in, b.lv_w[k], Bg, nC, k ? L >> (k - 1) : L, k ? 2 : 1, gin, g.lv_w[k],
                                g.lv_b[k], dw_sl + (size_t)k * s.dw_slice, gadd, next_sl, on_load ? dk : nullptr, on_load ? &nk : nullptr,
                                on_load ? cur_sl : nullptr, st, ctx);
    if (rc) return rc;
  }
  // proj_1x1: y1 = W_p xin + b_p, o = PReLU(GlobLN(y1))
  return srf_gln_bwd_impl(g_o, nullptr, y1, &pn, Bg, nC, L, go, 0, g.proj_g, g.proj_be, g.proj_prelu, gln_sl + (size_t)(D + 1) * s.gln_slice,
                          path.proj_pre ? 1 : 0, st, ctx);   // go = g_y1
}

// GroupComm: gx = g_u.  u = x + GlobLN_(b,g)(q), q = TAC_MLP(x):  g_x = g_u + MLP^T(GlobLN^T(g_u))
int BwdWalk::block_tac(int i) {
  const SrfBlock<const float> b = plan_block(p, P, i);
  const SrfBlock<float> g = plan_block(p, G, i);
  const float* q = (const float*)(blk(i) + t.q);
  float *gq = fp(s.gq), *gxm = fp(s.gxm);
  srf_norm tn{plan_slots(p, stats(), i).tac, b.tac_g, b.tac_b, nullptr};
  int rc = srf_gln_bwd(gx, nullptr, q, &tn, Bg, nB, L, gq, 0, g.tac_g, g.tac_b, nullptr, sc + s.gln, st);
  if (rc) return rc;
  rc = srf_tac_bwd(xbuf(i), gq, b.tac, g.tac, Bt, p->cfg.group_size, nB, 3 * nB, L, gxm, sc + s.tac, st);
  if (rc) return rc;
  return srf_accumulate_launch(gx, gxm, (long)Bt * B * L, st);
}

// Block i, U-ConvBlock :198-220 (GroupComm: on the folded tensor, preceded by TAC): gx = g_x(i + 1) -> g_x(i)
int BwdWalk::block(int i) {
  const bool gc = p->cfg.variant == SRF_VARIANT_GROUPCOMM;
  const SrfBlock<const float> b = plan_block(p, P, i);
  const SrfBlock<float> g = plan_block(p, G, i);
  const float* merged = (const float*)(blk(i) + t.merged);
  const float* xin = gc ? (const float*)(blk(i) + t.u) : xbuf(i);   // the U-ConvBlock's input
  float *zeros = fp(s.zeros), *gf = fp(s.gf);
  void* wg = sc + s.wg;
  // res_conv: x_{i+1} = W_r PReLU(GlobLN(merged)) + b_r + xin
  srf_norm fn{plan_slots(p, stats(), i).merged, b.fin_g, b.fin_be, b.fin_prelu};
  int rc = srf_pw_wgrad(gx, merged, &fn, Bg, nC, nB, L, g.res_w, g.res_b, 1, wg, st);
  if (rc) return rc;
  if (!gf_ready) {        // (else: block i + 1's data-gradient pair below already left g_f = W_r^T g_x here)
    rc = data_grad(gx, b.res_w, pkT_res[i], gf, Bg, nB, nC, nullptr);
    if (rc) return rc;
  }
  gf_ready = false;
  srf_bwd_ctx_defer(ctx, true);     // the block's norm / conv backwards leave their parameter-gradient reductions to the batched flush
  rc = block_pyramid(i);
  srf_bwd_ctx_defer(ctx, false);
  if (rc) return rc;
  rc = srf_pw_wgrad(go, xin, nullptr, Bg, nB, nC, L, g.proj_w, g.proj_b, 1, wg, st);
  if (rc) return rc;
  // Data gradients back to back (round 5; srf_pwconv_x3f.hip, no prologue): g_x(i) = W_p^T g_y1 + g_x(i + 1) -- the block's
  // input gradient, skip included -- and, from registers, block i - 1's g_f = W_r^T g_x(i): one launch, bit-identical to the
  // two it replaces (the B = 256 Improved models, launches of at least one tile per CU; debug flag 1 = without).
  if (i > 0 && !gc && pkT_proj[i] && pkT_res[i - 1] && srf_pw_conv_pair_supported(Bg, nC, nB, nC, L) &&
      srf_pw_packed_only(pkT_proj[i], go, Bg, nC, nB, L) && srf_pw_packed_only(pkT_res[i - 1], gx, Bg, nB, nC, L)) {
    rc = srf_pw_conv_pair(go, pkT_proj[i], zeros, gx_other, nullptr, gx, pkT_res[i - 1], zeros, gf, nullptr, Bg, nC, nB, nC, L, st);
    gf_ready = true;
  } else {
    rc = data_grad(go, b.proj_w, pkT_proj[i], gx_other, Bg, nC, nB, gx);   // + skip
  }
  if (rc) return rc;
  std::swap(gx, gx_other);
  return gc ? block_tac(i) : SRF_OK;
}

// Bottleneck, the blocks' deferred reductions, encoder weight, and on request the input waveform
int BwdWalk::front(const float* wav, float* grad_wav) {
  const SrfFront<const float> f = plan_front(P);
  const SrfFront<float> gf_ = plan_front(G);
  const int h = K / 2;
  void* wg = sc + s.wg;
  float *genc = fp(s.genc), *gv = fp(s.gv), *frames = fp(s.frames);
  // ---- bottleneck: x_0 = W_b GlobLN(enc) + b_b                  :256-259,292
  srf_norm ln{stats(), f.ln_g, f.ln_b, nullptr};
  int rc = srf_pw_wgrad(gx, enc(), &ln, Bt, N, B, L, gf_.bott_w, gf_.bott_b, 1, wg, st);
  if (rc) return rc;
  // g_ln into the (now free) gv buffer, then GlobLN backward accumulated onto the mask path's g_enc
  rc = data_grad(gx, f.bott_w, pkT_bott, gv, Bt, B, N, nullptr);
  if (rc) return rc;
  rc = srf_gln_bwd(gv, nullptr, enc(), &ln, Bt, N, L, genc, 1, gf_.ln_g, gf_.ln_b, nullptr, sc + s.gln, st);
  if (rc) return rc;
  // ---- the blocks' deferred parameter-gradient reductions, batched
  rc = srf_bwd_ctx_flush(ctx, st);
  if (rc) return rc;
  // ---- encoder weight                                           :247-251,286
  rc = srf_frames_gather(wav, frames, Bt, p->A, p->T, K, h, h, L, p->A * K, st);
  if (rc) return rc;
  rc = srf_pw_wgrad(genc, frames, nullptr, Bt, p->A * K, N, L, gf_.enc_w, nullptr, 1, wg, st);
  if (rc || !grad_wav) return rc;
  // ---- input waveform: g_wav[b,a,t] = sum_{n,l,k: h l + k - h = t} W_e[n,a,k] g_enc[b,n,l]   (the decoder's arithmetic with
  // the encoder's weight [N, A, K] in ConvTranspose1d layout; its scratch fits the forward decoder's: N <= S A N, A <= S A)
  return srf_decoder(genc, f.enc_w, grad_wav, Bt, N, p->A, K, L, p->T, fp(s.dec), st);
}

static int backward_impl(const srf_plan* p, const float* const* P, float* const* G, int num_params, const float* wav,
                         const float* grad_out, const void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes,
                         float* grad_wav, void* stream) {
  const char* who = grad_wav ? "srf_backward_wav" : "srf_backward";
  if (other_family_refused(p, who)) return SRF_EINVAL;
  // (freed on every exit path: a backward that fails half-way leaves nothing behind)
  const std::unique_ptr<SrfBwdCtx, void (*)(SrfBwdCtx*)> ctx(srf_bwd_ctx_new(), srf_bwd_ctx_free);
  BwdWalk w(p, P, G, saved, scratch, stream, ctx.get());
  int rc = srf_train_entry_check(who, p, P, G, num_params, 0, {G, wav, grad_out},
                                 {saved, saved_bytes, w.t.total, scratch, scratch_bytes, w.s.total});
  if (!rc) rc = train_check(p, who);
  if (!rc) rc = pyr_bwd_path(p, saved, scratch, who, &w.path);
  if (rc) return rc;
  SRF_CHECK_HIP(hipMemsetAsync(w.fp(w.s.zeros), 0, sizeof(float) * std::max({p->cfg.in_channels, w.SAN, w.N}), w.st));
  // the blocks' norm / conv backwards get one scratch slice per call (statistic buckets zeroed here, once)
  // (the WHOLE arena, 75 MB at cfg 2 / 170 MB at cfg 4 = 0.1 % of a step, not just the fp64 buckets at the head of each norm slice
  // -- the chunked fallback kernels (debug flags 1<<29 / 1<<30, rows beyond the row kernels' limits) accumulate
  // their row partials with atomicAdd and rely on zeroed slices)
  SRF_CHECK_HIP(hipMemsetAsync(w.sc + w.s.arena, 0, w.s.arena_bytes, w.st));
  rc = w.pack_weights();
  if (!rc) rc = w.tail(grad_out);
  for (int i = w.U - 1; i >= 0 && !rc; --i) rc = w.block(i);
  return rc ? rc : w.front(wav, grad_wav);
}

extern "C" int srf_backward(const srf_plan* p, const float* const* P, float* const* G, int num_params, const float* wav,
                            const float* grad_out, const void* saved, size_t saved_bytes, void* scratch,
                            size_t scratch_bytes, void* stream) {
  return backward_impl(p, P, G, num_params, wav, grad_out, saved, saved_bytes, scratch, scratch_bytes, nullptr, stream);
}
// ... and the gradient w.r.t. the input waveform on top (ABI 15; the reference's autograd produces it when the caller's
// mixture requires grad, improved_sudormrf.py:283-301 is plain ATen): grad_wav [Bt, in_audio_channels, T] (overwritten) =
// the encoder's transposed convolution (:247-251,286; the right zero-pad of :303-314 is a crop) of the gradient w.r.t.
// the encoder output, which the backward forms anyway (mask path + GlobLN path).
extern "C" int srf_backward_wav(const srf_plan* p, const float* const* P, float* const* G, int num_params, const float* wav,
                                const float* grad_out, const void* saved, size_t saved_bytes, void* scratch,
                                size_t scratch_bytes, float* grad_wav, void* stream) {
  SRF_CHECK_ARG(grad_wav, "srf_backward_wav: null grad_wav");
  return backward_impl(p, P, G, num_params, wav, grad_out, saved, saved_bytes, scratch, scratch_bytes, grad_wav, stream);
}
