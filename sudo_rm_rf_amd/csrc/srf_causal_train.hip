// Causal SuDoRM-RF (v3) training step, device side: srf_causal_forward_train keeps what the backward
// needs, srf_causal_backward turns d loss / d output into every parameter gradient -- torch autograd over the reference's
// CausalSuDORMRF.forward (causal_improved_sudormrf_v3.py), as sequences of this library's per-kernel entry points.  Opt-in: the
// general training entry points (srf_train.hip) keep refusing causal plans.
//   saved   : encoder output | residual stream x_0 .. x_U | per block: proj_1x1's pre-activation u, the D pre-activations d_k of
//             the pyramid, merged | mask_net's output m (pre mask_nl_class).  Pre-activations, because a PReLU slope may be zero
//             or negative and the sign of the activated value then no longer tells the branch.
//   grads   : WRITTEN (not accumulated into), same order and shapes as the parameters.
#include "srf_plan.h"

namespace {

struct CTrainLayout {
  size_t enc, x0, x_stride, blk0, blk_stride, u, lv[SRF_MAX_DEPTH], merged, m, total;
};

CTrainLayout ctrain_layout(const srf_plan* p) {
  CTrainLayout t{};
  const srf_config& c = p->cfg;
  const size_t F = sizeof(float), L = p->L, Bt = p->Bt;
  const int D = c.upsampling_depth, U = c.num_blocks;
  SrfCarve all, blk;      // (blk: one block's slices, offsets relative to the block's start)
  t.enc = all.take(F * Bt * c.enc_num_basis * L);
  t.x_stride = srf_align_up(F * Bt * c.out_channels * L, 256);
  t.x0 = all.take(t.x_stride * (U + 1));
  t.u = blk.take(F * Bt * c.in_channels * L);
  for (int k = 0; k < D; ++k) t.lv[k] = blk.take(F * Bt * c.in_channels * (L >> k));
  t.merged = blk.take(F * Bt * c.in_channels * L);
  t.blk_stride = blk.off;
  t.blk0 = all.take(blk.off * U);
  t.m = all.take(F * Bt * p->SA * c.enc_num_basis * L);
  t.total = all.off;
  return t;
}

struct CScratchLayout {
  size_t dec, gv, genc, gxa, gxb, gm, gu, gd[SRF_MAX_DEPTH], frames, wt, zeros, wdpad, wg, pyr, fold_res, fold_proj, encw, pk3,
      pkT, total;
  size_t zero_floats;
  int dec_rows;
};

CScratchLayout cscratch_layout(const srf_plan* p) {
  CScratchLayout s{};
  const srf_config& c = p->cfg;
  const size_t F = sizeof(float), L = p->L, Bt = p->Bt;
  const int D = c.upsampling_depth, U = c.num_blocks, K = c.enc_kernel_size, N = c.enc_num_basis, B = c.out_channels,
            C = c.in_channels;
  const int SAN = p->SA * N;
  SrfCarve all{0, /*min_one=*/true};
  s.dec = all.take(F * srf_decoder_scratch_floats(p->Bt, SAN, p->SA, K, p->L));
  s.gv = all.take(F * Bt * SAN * L);
  s.genc = all.take(F * Bt * N * L);
  s.gxa = all.take(F * Bt * B * L);
  s.gxb = all.take(F * Bt * B * L);
  s.gm = all.take(F * Bt * C * L);
  s.gu = all.take(F * Bt * C * L);
  for (int k = 0; k < D; ++k) s.gd[k] = all.take(F * Bt * C * (L >> k));
  s.dec_rows = (p->SA * K + 63) / 64 * 64;
  const size_t enc_rows = (size_t)p->A * K;
  s.frames = all.take(F * Bt * L * std::max((size_t)s.dec_rows, enc_rows));
  s.wt = all.take(F * std::max({(size_t)B * N, (size_t)B * C, (size_t)B * SAN}));
  s.zero_floats = std::max({C, SAN, N, B});
  s.zeros = all.take(F * s.zero_floats);
  s.wdpad = all.take(F * (size_t)SAN * s.dec_rows);
  size_t wg = 0;
  auto wgmax = [&](int cout, int cin) { wg = std::max(wg, srf_pw_wgrad_scratch_bytes(p->Bt, cout, cin, p->L)); };
  wgmax(B, N);
  wgmax(SAN, B);
  wgmax(SAN, s.dec_rows);
  wgmax(N, (int)enc_rows);
  wgmax(C, B);
  wgmax(B, C);
  s.wg = all.take(wg);
  s.pyr = all.take(std::max({srf_causal_pyramid_bwd_scratch_bytes(p->Bt, C, p->L, D), srf_causal_dwconv_bwd_scratch_bytes(p->Bt, C, p->L),
                              F * srf_causal_prelu_bwd_scratch_floats()}));
  s.fold_res = all.take(F * causal_fold_res_floats(B, C) * U);
  s.fold_proj = all.take(F * (size_t)C * B * U);
  s.encw = all.take(F * (size_t)N * enc_rows);
  {
    size_t pk = srf_align_up(srf_packed3_pw_weight_bytes(B, N), 256) + srf_align_up(srf_packed3_pw_weight_bytes(SAN, B), 256);
    pk += (size_t)U * srf_align_up(srf_packed3_pw_weight_bytes(C, B), 256);
    s.pk3 = all.take(pk);
  }
  {
    size_t pk = srf_align_up(srf_packed_pw_weight_bytes(B, SAN), 256) + srf_align_up(srf_packed_pw_weight_bytes(N, B), 256);
    pk += (size_t)U * (srf_align_up(srf_packed_pw_weight_bytes(C, B), 256) + srf_align_up(srf_packed_pw_weight_bytes(B, C), 256));
    s.pkT = all.take(pk);
  }
  s.total = all.off;
  return s;
}

bool causal_plan(const srf_plan* p, const char* who) {
  if (p && p->cfg.variant == SRF_VARIANT_CAUSAL) return true;
  srf_set_error("%s: %s", who, p ? "causal plans only (the other models train through srf_forward_train / srf_backward)" : "null plan");
  return false;
}

int ctrain_check(const srf_plan* p, const char* who) {
  if (p->L % 4 != 0) {      // (the weight-gradient GEMM's limit; only D = 1 models can miss it)
    srf_set_error("%s: L=%d must be a multiple of 4", who, p->L);
    return SRF_EINVAL;
  }
  return SRF_OK;
}

int cforward_train_impl(const srf_plan* p, const float* const* P, const float* wav, float* out, void* saved, void* scratch,
                        bool split_tail, void* stream) {
  const CTrainLayout t = ctrain_layout(p);
  const CScratchLayout s = cscratch_layout(p);
  const srf_config& c = p->cfg;
  const int D = c.upsampling_depth, U = c.num_blocks, N = c.enc_num_basis, K = c.enc_kernel_size;
  const int Bt = p->Bt, L = p->L, B = p->nB, Cc = p->nC, SAN = p->SA * N;
  char* sv = (char*)saved;
  char* sc = (char*)scratch;
  hipStream_t st = (hipStream_t)stream;
  auto xbuf = [&](int i) { return (float*)(sv + t.x0 + t.x_stride * i); };
  const SrfCausalLayout lay = causal_layout(p);
  const SrfCausalFront<const float> f = causal_front<const float>(P);
  const SrfCausalTail<const float> tl = causal_tail<const float>(lay, P);
  SrfCausalFolded w;
  int rc = srf_causal_fold(p, P, (float*)(sc + s.fold_res), (float*)(sc + s.fold_proj), &w, st);
  if (rc) return rc;
  // the exact-class images of the 1x1 weights the 256 x 128 GEMM takes, as srf_forward_train packs them (SrfPackQueue::add3)
  SrfPackQueue pk{sc + s.pk3};
  const void* pk_bott = pk.add3(f.bott_w, B, N);
  const void* pk_mask = pk.add3(tl.mask_w, SAN, B);
  std::vector<const void*> pk_proj(U, nullptr);
  for (int i = 0; i < U; ++i) pk_proj[i] = pk.add3(w.wproj[i], Cc, B);
  rc = pk.pack3(stream);
  if (rc) return rc;
  float* enc = (float*)(sv + t.enc);
  rc = srf_causal_encoder(wav, f.enc_w, enc, Bt, p->A, p->T, N, K, L, stream);
  if (rc) return rc;
  rc = srf_pw_conv_packed3(enc, f.bott_w, pk_bott, f.bott_b, xbuf(0), Bt, N, B, L, nullptr, nullptr, nullptr, stream);
  if (rc) return rc;
  for (int i = 0; i < U; ++i) {
    const SrfCausalBlock<const float> b = causal_block<const float>(lay, P, i);
    char* blk = sv + t.blk0 + t.blk_stride * i;
    float* u = (float*)(blk + t.u);
    float* merged = (float*)(blk + t.merged);
    rc = srf_pw_conv_packed3(xbuf(i), w.wproj[i], pk_proj[i], b.proj_b, u, Bt, B, Cc, L, nullptr, nullptr, nullptr, stream);
    if (rc) return rc;
    // the per-level kernels with the activation moved to the consumer's load: d_k is stored BEFORE its PReLU
    const float* dv[SRF_MAX_DEPTH];
    for (int k = 0; k < D; ++k) {
      float* dk = (float*)(blk + t.lv[k]);
      rc = srf_causal_dwconv(k == 0 ? u : dv[k - 1], b.lv_w[k], b.lv_b[k], k == 0 ? b.proj_prelu : b.lv_prelu[k - 1], nullptr, dk, Bt,
                             Cc, k == 0 ? L : (L >> (k - 1)), k == 0 ? 1 : 2, stream);
      if (rc) return rc;
      dv[k] = dk;
    }
    rc = srf_causal_merge_act(dv, b.lv_prelu, D, merged, Bt, Cc, L, st);
    if (rc) return rc;
    rc = srf_pw_conv_packed3(merged, w.wres[i], nullptr, w.bres[i], xbuf(i + 1), Bt, Cc, B, L, nullptr, xbuf(i), nullptr, stream);
    if (rc) return rc;
  }
  float* m = (float*)(sv + t.m);
  {
    srf_norm pre{nullptr, nullptr, nullptr, tl.mask_prelu};
    rc = srf_pw_conv_packed3(xbuf(U), tl.mask_w, pk_mask, tl.mask_b, m, Bt, B, SAN, L, &pre, nullptr, nullptr, stream);
    if (rc) return rc;
  }
  float* v = (float*)(sc + s.gv);
  rc = srf_prelu_apply(m, tl.out_prelu, v, (long)Bt * SAN * L, stream);
  if (rc) return rc;
  // the decoder's frame GEMM is the last linear map: on the split kernel when the exact class was this call's own choice
  const SrfKernelModeScope split_class(split_tail, 0);
  return srf_decoder(v, tl.dec_w, out, Bt, SAN, p->SA, K, L, p->T, (float*)(sc + s.dec), stream);
}

}  // namespace

extern "C" size_t srf_causal_train_saved_bytes(const srf_plan* p) {
  return causal_plan(p, "srf_causal_train_saved_bytes") ? ctrain_layout(p).total : 0;
}
extern "C" size_t srf_causal_train_scratch_bytes(const srf_plan* p) {
  return causal_plan(p, "srf_causal_train_scratch_bytes") ? cscratch_layout(p).total : 0;
}

extern "C" int srf_causal_forward_train(const srf_plan* p, const float* const* P, int num_params, const float* wav, float* out,
                                        void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes, void* stream) {
  if (!causal_plan(p, "srf_causal_forward_train")) return SRF_EINVAL;
  int rc = srf_train_entry_check("srf_causal_forward_train", p, P, nullptr, num_params, 0, {wav, out},
                                 {saved, saved_bytes, ctrain_layout(p).total, scratch, scratch_bytes, cscratch_layout(p).total});
  if (!rc) rc = ctrain_check(p, "srf_causal_forward_train");
  if (rc) return rc;
  const bool exact = srf_train_fwd_exact();
  const SrfKernelModeScope exact_class(exact, 2);
  if (srf_profiling()) srf_prof_mark("(gap)", (hipStream_t)stream);
  return cforward_train_impl(p, P, wav, out, saved, scratch, exact, stream);
}

extern "C" int srf_causal_backward(const srf_plan* p, const float* const* P, float* const* G, int num_params, const float* wav,
                                   const float* grad_out, const void* saved, size_t saved_bytes, void* scratch,
                                   size_t scratch_bytes, void* stream) {
  if (!causal_plan(p, "srf_causal_backward")) return SRF_EINVAL;
  const CTrainLayout t = ctrain_layout(p);
  const CScratchLayout s = cscratch_layout(p);
  int rc = srf_train_entry_check("srf_causal_backward", p, P, G, num_params, 0, {G, wav, grad_out},
                                 {saved, saved_bytes, t.total, scratch, scratch_bytes, s.total});
  if (!rc) rc = ctrain_check(p, "srf_causal_backward");
  if (rc) return rc;
  const srf_config& c = p->cfg;
  const int D = c.upsampling_depth, U = c.num_blocks, N = c.enc_num_basis, K = c.enc_kernel_size, h = K / 2;
  const int Bt = p->Bt, L = p->L, B = p->nB, C = p->nC, SA = p->SA, SAN = p->SA * N;
  const char* sv = (const char*)saved;
  char* sc = (char*)scratch;
  hipStream_t st = (hipStream_t)stream;
  auto xbuf = [&](int i) { return (const float*)(sv + t.x0 + t.x_stride * i); };
  auto fp = [&](size_t o) { return (float*)(sc + o); };
  const float* enc = (const float*)(sv + t.enc);
  const float* m = (const float*)(sv + t.m);
  float* zeros = fp(s.zeros);
  float* wt = fp(s.wt);
  void* wg = sc + s.wg;
  const SrfCausalLayout lay = causal_layout(p);
  const SrfCausalFront<const float> f = causal_front<const float>(P);
  const SrfCausalFront<float> gf = causal_front<float>(G);
  const SrfCausalTail<const float> tl = causal_tail<const float>(lay, P);
  const SrfCausalTail<float> gtl = causal_tail<float>(lay, G);
  if (srf_profiling()) srf_prof_mark("(gap)", st);
  SRF_CHECK_HIP(hipMemsetAsync(zeros, 0, sizeof(float) * s.zero_floats, st));
  // the weight-gradient GEMMs of this call fold their partial sums in a fixed order: two backwards of one step give equal bits
  const SrfWgradOrderedScope ordered_for_this_call;
  SrfCausalFolded w;
  rc = srf_causal_fold(p, P, fp(s.fold_res), fp(s.fold_proj), &w, st);
  if (rc) return rc;
  // transposed weights of the data-gradient GEMMs, pre-split for the 256 x 128 kernel where it takes the shape
  SrfPackQueue pk{sc + s.pkT};
  auto packT = [&](const float* wf, int cout_d, int cin_d) {   // wf: forward weight [cin_d][cout_d]
    return pk.add(wf, srf_kernel_mode() == 0 ? srf_packed_pw_weight_bytes(cout_d, cin_d) : 0, cout_d, cin_d);
  };
  const void* pkT_mask = packT(tl.mask_w, B, SAN);
  const void* pkT_bott = packT(f.bott_w, N, B);
  std::vector<const void*> pkT_res(U, nullptr), pkT_proj(U, nullptr);
  for (int i = 0; i < U; ++i) {
    pkT_res[i] = packT(w.wres[i], C, B);
    pkT_proj[i] = packT(w.wproj[i], B, C);
  }
  rc = pk.packT(st);
  if (rc) return rc;
  // g_x = W^T g (+ residual): cin_d -> cout_d, w the forward weight [cin_d][cout_d]
  // Where no packed image serves the launch the GEMM would fall to the kernels that split fp32 into two bf16 parts on the fly (16
  // mantissa bits per operand); those launches, and the decoder's frame GEMM below, run in the exact-fp32 class instead (kernel
  // mode 2 for this thread, as the training forward does and as srf_original_backward does for the same launches).  Measured on
  // causal_tiny with a batch that falls silent half-way: mask_net.0's slope gradient, one sum of 3104 terms that cancels to 6e-4
  // of their size, carried 1.0e-5 of absolute error from the two GEMMs that feed it (4.4e-4 of its value, 2.3e-2) against 4.7e-7
  // in the exact class.  Launches the 256 x 128 kernel serves from a packed image keep it, and so does every launch of more than
  // 2^28 multiply-adds: below that a GEMM's time is its launch (microseconds in either class), above it the exact-fp32 MFMA kernel
  // costs 2.5 x the split one (the 16-block bench step: 18 such launches, 39.9 -> 41.0 ms when they were moved too).
  auto small_gemm = [&](int cin_d, int cout_d) { return (long)Bt * L * cin_d * cout_d <= (1L << 28); };
  auto data_grad = [&](const float* g, const float* w, const void* pk, float* y, int cin_d, int cout_d, const float* residual) -> int {
    const bool on_the_fly = small_gemm(cin_d, cout_d) && !srf_pw_packed_only(pk, g, Bt, cin_d, cout_d, L);
    const SrfKernelModeScope exact(on_the_fly && srf_kernel_mode() == 0, 2);
    return srf_pw_data_grad(g, w, pk, wt, zeros, y, Bt, cin_d, cout_d, L, residual, st);
  };
  // ---- decoder: out = overlap_add(W_d^T PReLU_c(m))
  float* frames = fp(s.frames);
  float* gv = fp(s.gv);
  rc = srf_frames_gather(grad_out, frames, Bt, SA, p->T, K, h, h, L, s.dec_rows, stream);
  if (rc) return rc;
  rc = srf_prelu_apply(m, tl.out_prelu, gv, (long)Bt * SAN * L, stream);     // v, re-computed
  if (rc) return rc;
  rc = srf_pw_wgrad_cols(gv, frames, nullptr, Bt, s.dec_rows, SAN, L, gtl.dec_w, SA * K, nullptr, 0, wg, stream);
  if (rc) return rc;
  float* wdpad = fp(s.wdpad);
  SRF_CHECK_HIP(hipMemsetAsync(wdpad, 0, sizeof(float) * (size_t)SAN * s.dec_rows, st));
  SRF_CHECK_HIP(hipMemcpy2DAsync(wdpad, sizeof(float) * s.dec_rows, tl.dec_w, sizeof(float) * SA * K, sizeof(float) * SA * K, SAN,
                                 hipMemcpyDeviceToDevice, st));
  {
    const SrfKernelModeScope exact(small_gemm(s.dec_rows, SAN) && srf_kernel_mode() == 0, 2);
    rc = srf_pw_conv(frames, wdpad, zeros, gv, Bt, s.dec_rows, SAN, L, nullptr, nullptr, nullptr, 0, nullptr, 0, stream);
  }
  if (rc) return rc;
  // ---- mask_nl_class, mask_net
  rc = srf_causal_prelu_bwd(gv, m, tl.out_prelu, gv, gtl.out_prelu, (long)Bt * SAN * L, fp(s.pyr), st);      // gv = g_m
  if (rc) return rc;
  float* gx = fp(s.gxa);
  float* gx_other = fp(s.gxb);
  {
    srf_norm pre{nullptr, nullptr, nullptr, tl.mask_prelu};
    rc = srf_pw_wgrad(gv, xbuf(U), &pre, Bt, B, SAN, L, gtl.mask_w, gtl.mask_b, 0, wg, stream);
    if (rc) return rc;
    rc = data_grad(gv, tl.mask_w, pkT_mask, gx, SAN, B, nullptr);
    if (rc) return rc;
    rc = srf_causal_prelu_bwd(gx, xbuf(U), tl.mask_prelu, gx, gtl.mask_prelu, (long)Bt * B * L, fp(s.pyr), st);
    if (rc) return rc;
  }
  // ---- blocks in reverse
  const bool fused = srf_kernel_mode() != 1 && !srf_dbg(SRF_DBG_PYR_PER_LEVEL) && srf_causal_pyramid_bwd_supported(C, L, D);
  float* gm = fp(s.gm);
  float* gu = fp(s.gu);
  std::vector<float*> g_dw(U), g_db(U), g_gain(U);
  std::vector<const float*> p_w(U), p_b(U), p_gain(U);
  std::vector<const float*> bsrc, bscale;
  std::vector<float*> bdst;
  std::vector<long> bn;
  std::vector<float> bh;
  for (int i = U - 1; i >= 0; --i) {
    const SrfCausalBlock<const float> b = causal_block<const float>(lay, P, i);
    const SrfCausalBlock<float> g = causal_block<float>(lay, G, i);
    const char* blk = sv + t.blk0 + t.blk_stride * i;
    const float* u = (const float*)(blk + t.u);
    const float* merged = (const float*)(blk + t.merged);
    // res_conv in its folded form: dW_f, db_f now (scaled to dW_r, db_r and reduced to d gain after the loop), g_M = W_f^T g_x'
    rc = srf_pw_wgrad(gx, merged, nullptr, Bt, C, B, L, g.res_w, g.res_b, 0, wg, stream);
    if (rc) return rc;
    g_dw[i] = g.res_w; g_db[i] = g.res_b; g_gain[i] = g.gain;
    p_w[i] = b.res_w; p_b[i] = b.res_b; p_gain[i] = b.gain;
    rc = data_grad(gx, w.wres[i], pkT_res[i], gm, B, C, nullptr);
    if (rc) return rc;
    const float* dv[SRF_MAX_DEPTH];
    for (int k = 0; k < D; ++k) dv[k] = (const float*)(blk + t.lv[k]);
    if (fused) {
      rc = srf_causal_pyramid_bwd(gm, u, dv, b.proj_prelu, b.lv_w, b.lv_prelu, gu, g.lv_w, g.lv_b, g.lv_prelu, g.proj_prelu, Bt, C, L,
                                  D, sc + s.pyr, stream);
      if (rc) return rc;
    } else {
      for (int k = D - 1; k >= 0; --k) {
        rc = srf_causal_dwconv_bwd(gm, k, k < D - 1 ? fp(s.gd[k + 1]) : nullptr, k < D - 1 ? b.lv_w[k + 1] : nullptr, 2, dv[k],
                                   b.lv_prelu[k], k == 0 ? u : dv[k - 1], k == 0 ? b.proj_prelu : b.lv_prelu[k - 1], k == 0 ? 1 : 2,
                                   fp(s.gd[k]), g.lv_w[k], g.lv_b[k], g.lv_prelu[k], Bt, C, L >> k, sc + s.pyr, stream);
        if (rc) return rc;
      }
      rc = srf_causal_dwconv_bwd(nullptr, 0, fp(s.gd[0]), b.lv_w[0], 1, u, b.proj_prelu, nullptr, nullptr, 1, gu, nullptr, nullptr,
                                 g.proj_prelu, Bt, C, L, sc + s.pyr, stream);
      if (rc) return rc;
    }
    // proj_1x1 (its weight ran as W_p / beta): dW_p = gu x^T / beta, db_p, g_x = g_x' + W_p^T gu / beta
    rc = srf_pw_wgrad(gu, xbuf(i), nullptr, Bt, B, C, L, g.proj_w, g.proj_b, 0, wg, stream);
    if (rc) return rc;
    if (p->beta[i] != 1.f) {
      bsrc.push_back(g.proj_w); bdst.push_back(g.proj_w); bn.push_back((long)C * B); bscale.push_back(nullptr); bh.push_back(1.f / p->beta[i]);
    }
    rc = data_grad(gu, w.wproj[i], pkT_proj[i], gx_other, C, B, gx);
    if (rc) return rc;
    float* tmp = gx;
    gx = gx_other;
    gx_other = tmp;
  }
  // ---- bottleneck, encoder
  float* genc = fp(s.genc);
  rc = srf_pw_wgrad(gx, enc, nullptr, Bt, N, B, L, gf.bott_w, gf.bott_b, 0, wg, stream);
  if (rc) return rc;
  rc = data_grad(gx, f.bott_w, pkT_bott, genc, B, N, nullptr);
  if (rc) return rc;
  rc = srf_frames_gather(wav, frames, Bt, p->A, p->T, K, h, 2 * h, L, p->A * K, stream);
  if (rc) return rc;
  rc = srf_pw_wgrad(genc, frames, nullptr, Bt, p->A * K, N, L, fp(s.encw), nullptr, 0, wg, stream);
  if (rc) return rc;
  rc = srf_causal_enc_scatter(fp(s.encw), gf.enc_w, N, p->A, K, st);
  if (rc) return rc;
  // ---- every block's skipinit_gain / res_conv gradients and the 1 / beta of the proj_1x1 weight gradients
  std::vector<float> alpha(p->alpha.begin(), p->alpha.end());
  rc = srf_causal_gain_fold(g_dw.data(), g_db.data(), p_w.data(), p_b.data(), p_gain.data(), g_gain.data(), alpha.data(), B * C, B, U, st);
  if (rc) return rc;
  if (!bsrc.empty()) rc = srf_causal_scale_many(bsrc.data(), bdst.data(), bn.data(), bscale.data(), bh.data(), (int)bsrc.size(), st);
  return rc;
}
