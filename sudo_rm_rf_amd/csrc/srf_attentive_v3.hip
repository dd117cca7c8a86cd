// Attentive SuDoRM-RF v3 (attentive_sudormrf_v3.py): the Improved model's front end and tail around blocks that fold the
// depthwise pyramid from the deepest level up with D - 1 ConditionalTransformerLayers ("attentive resamplers") instead of an
// upsample-and-add.  Plan constructor and the inference walk; every kernel is an existing entry point except srf_gln_apply_stats
// (srf_attention.hip).  Inference only, single stream.  Parameter and slot layout: srf_plan.h.
//
// One block (AttentiveUConvBlock.forward); level k has L_k positions, L_0 = L, L_{k+1} = ceil(L_k / 2):
//   y1  = proj_1x1.conv(x)                                    srf_pw_conv_packed   (+ statistics of proj_1x1.norm)
//   d_k = spp_dw[k].conv(norm(d_{k-1})), k = 0 .. D - 1       srf_dwconv5          (+ statistics of spp_dw[k].norm)
//   v   = d_{D-1} with its lazy GlobLN; for r = 0 .. D - 2, q = d_{D-2-r} with its lazy GlobLN (Lq = L_{D-2-r}, Lk = L_{D-1-r}):
//     vp = norm(v) + pe_r[:Lk]                                srf_posenc_apply
//     kv = [K; V]_proj(vp)                                    srf_pw_conv_packed, ONE conv over the concatenated [2 H d, C] weight
//     qp = Q_proj(norm(q))                                    srf_pw_conv_packed   (norm on load)
//     o  = softmax(qp^T k / sqrt(d)) v per head               srf_mha_forward(Lq, Lk)
//     qn = norm(q)                                            srf_gln_apply_stats  (no statistics: O_proj's residual is a raw pointer)
//     y  = O_proj(o) + qn                                     srf_pw_conv_packed   (residual, + statistics of out_mha_norm)
//     f  = ffn.conv(out_mha_norm(y))                          srf_pw_conv_packed   (norm on load, + statistics of ffn.norm)
//     z  = PReLU(ffn.norm(f)) + out_mha_norm(y)               srf_gln_apply2_add   (+ statistics of out_norm; into q's buffer)
//     v  = z with out_norm as its lazy GlobLN
//   e   = norm(v)                                             srf_gln_apply_stats  (+ statistics of final_norm: a GlobLN on a GlobLN)
//   x'  = res_conv(PReLU(final_norm(e))) + x                  srf_pw_conv_packed
// D = 1 has no resampler: v = d_0 goes straight to the last two steps.
#include <vector>
#include "srf_mha.h"
#include "srf_plan.h"

static long att3_gcd(long a, long b) { return b ? att3_gcd(b, a % b) : a; }

// parameter index of resampler r's first tensor (mha.Q_proj.weight) in block i
static inline int att3_p_base(const srf_plan* p, int i, int r) {
  return plan_p_proj(p, i) + plan_block_params(p->cfg.upsampling_depth, false) + r * SRF_PA_COUNT;
}

extern "C" int srf_attentive_v3_plan_create(const srf_config* base, int n_heads, int att_dims, int batch, int T, srf_plan** out) {
  SRF_CHECK_ARG(base && out, "srf_attentive_v3_plan_create: null pointer");
  *out = nullptr;
  const srf_config& c = *base;
  SRF_CHECK_ARG(batch > 0 && T > 0, "srf_attentive_v3_plan_create: batch and T must be positive");
  SRF_CHECK_ARG(c.out_channels > 0 && c.in_channels > 0 && c.num_blocks > 0 && c.enc_num_basis > 0 && c.num_sources > 0,
                "srf_attentive_v3_plan_create: non-positive model dimension");
  SRF_CHECK_ARG(c.in_audio_channels == 1 && c.group_size == 1,
                "srf_attentive_v3_plan_create: in_audio_channels and group_size must be 1 (got %d, %d)", c.in_audio_channels,
                c.group_size);
  SRF_CHECK_ARG(n_heads >= 1 && att_dims >= 1, "srf_attentive_v3_plan_create: n_heads = %d and att_dims = %d must be positive",
                n_heads, att_dims);
  SRF_CHECK_ARG(c.upsampling_depth >= 1 && c.upsampling_depth <= SRF_MAX_DEPTH,
                "srf_attentive_v3_plan_create: upsampling_depth %d unsupported (1..%d)", c.upsampling_depth, SRF_MAX_DEPTH);
  SRF_CHECK_ARG(c.enc_kernel_size >= 3 && (c.enc_kernel_size & 1),
                "srf_attentive_v3_plan_create: enc_kernel_size must be odd (got %d)", c.enc_kernel_size);
  const int D = c.upsampling_depth, U = c.num_blocks, K = c.enc_kernel_size, N = c.enc_num_basis, h = K / 2;
  // pad_to_appropriate_length: up to a multiple of lcm(K / 2, 2^D) -- only when T is not one already
  const long lcm = (long)h * (1L << D) / att3_gcd(h, 1L << D);
  const long Tp = T % lcm ? T + lcm - T % lcm : T;
  SRF_CHECK_ARG(Tp <= (1L << 30), "srf_attentive_v3_plan_create: T = %d too long", T);
  const long L = (Tp + 2 * h - K) / h + 1;
  // the strided convolutions' own arithmetic (kernel 5, padding 2, stride 2): ceil halving, no divisibility asked
  long lv[SRF_MAX_DEPTH];
  lv[0] = L;
  for (int k = 1; k < D; ++k) lv[k] = (lv[k - 1] - 1) / 2 + 1;
  for (int k = 0; k < D; ++k)
    SRF_CHECK_ARG(lv[k] >= 1, "srf_attentive_v3_plan_create: T = %d leaves level %d with %ld positions (needs >= 1)", T, k, lv[k]);
  if (D >= 2)
    SRF_CHECK_ARG(lv[1] <= SRF_ATT_MAX_LEN,
                  "srf_attentive_v3_plan_create: T = %d gives %ld positions on level 1; the position table of the answering side "
                  "holds %d", T, lv[1], SRF_ATT_MAX_LEN);
  SRF_CHECK_ARG(batch <= 65535, "srf_attentive_v3_plan_create: batch %d too large (max 65535 per call)", batch);
  srf_plan* p = new (std::nothrow) srf_plan();
  SRF_CHECK_ARG(p != nullptr, "srf_attentive_v3_plan_create: out of host memory");
  p->cfg = c;
  p->cfg.variant = SRF_VARIANT_ATTENTIVE_V3;
  p->A = 1;
  p->Bt = p->Bg = batch;
  p->T = T;
  p->Tp = (int)Tp;
  p->L = (int)L;
  p->SA = c.num_sources;
  p->nB = c.out_channels;
  p->nC = c.in_channels;
  p->att_heads = n_heads;
  p->att_dims = att_dims;
  for (int k = 0; k < D; ++k) p->att_lv[k] = (int)lv[k];
  p->att_len = (int)lv[D - 1];
  const int C = c.in_channels, HD = n_heads * att_dims, R = D - 1;
  // ---- parameters and statistic slots (srf_plan.h)
  p->p_block0 = SRF_P_FRONT;
  p->p_ublock_off = 0;
  p->p_block_stride = plan_v3_block_params(D);
  p->p_tail = p->p_block0 + U * p->p_block_stride;
  p->n_params = p->p_tail + SRF_P_TAIL;
  p->slots_per_block = plan_v3_slots_per_block(D);
  p->n_slots = 1 + U * p->slots_per_block;
  const size_t F = sizeof(float);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t o = off;
    off = srf_align_up(off + bytes, 256);
    return o;
  };
  p->stats_bytes = (size_t)p->n_slots * batch * SRF_STAT_BUCKETS * 2 * sizeof(double);
  p->off_stats = take(p->stats_bytes);
  p->off_enc = take(F * batch * N * L);
  p->off_xa = take(F * batch * c.out_channels * L);
  p->off_xb = take(F * batch * c.out_channels * L);
  p->off_y1 = take(F * batch * C * L);
  for (int k = 0; k < D; ++k) p->off_lv[k] = take(F * batch * C * lv[k]);
  p->off_masked = take(F * batch * p->SA * N * L);
  p->off_dec = take(F * srf_decoder_scratch_floats(batch, p->SA * N, p->SA, K, p->L));
  if (R > 0) {
    // the resamplers' activations, sized for the shallowest pair (asking side: level 0, answering side: level 1)
    p->off_att_x = take(F * batch * C * lv[1]);
    p->off_att_qkv = take(F * batch * 2 * HD * lv[1]);
    p->off_att_q = take(F * batch * HD * lv[0]);
    p->off_att_o = take(F * batch * HD * lv[0]);
    p->off_att_qn = take(F * batch * C * lv[0]);
    p->off_att_y = take(F * batch * C * lv[0]);
    p->off_att_f = take(F * batch * C * lv[0]);
    // per (block, resampler): [2 H d, C] weight | [2 H d] bias   (each section 64-float aligned)
    p->off_att_wqkv = take(F * U * R * (srf_align_up((size_t)2 * HD * C, 64) + srf_align_up((size_t)2 * HD, 64)));
  }
  p->fused_pyramid = 0;
  p->off_pyr = 0;
  // packed (split-bf16) images for the 256 x 128 GEMM, where it takes the shape; the K/V image hangs on K_proj.weight's index
  p->pk_of_param.assign(p->n_params, 0);
  plan_add_pack(p, &off, SRF_P_BOTTLENECK, c.out_channels, N);
  for (int i = 0; i < U; ++i) {
    plan_add_pack(p, &off, plan_p_proj(p, i), C, c.out_channels);
    plan_add_pack(p, &off, plan_p_res(p, i), c.out_channels, C);
    for (int r = 0; r < R; ++r) {
      plan_add_pack(p, &off, att3_p_base(p, i, r) + SRF_PA_Q, HD, C);
      plan_add_pack(p, &off, att3_p_base(p, i, r) + SRF_PA_K, 2 * HD, C);
      plan_add_pack(p, &off, att3_p_base(p, i, r) + SRF_PA_O, C, HD);
      plan_add_pack(p, &off, att3_p_base(p, i, r) + SRF_PA_FFN, C, C);
    }
  }
  plan_add_pack(p, &off, plan_p_mask(p), p->SA * N, c.out_channels);
  p->off_wdpack = (p->SA * K <= 64 && p->pk_of_param[plan_p_mask(p)]) ? take(srf_mask_decode_pack_bytes(p->SA * N)) : 0;
  p->total_bytes = off;
  p->n_launches = 1 /*zero*/ + (4 * U * R + 47) / 48 /*concat*/ + 1 /*pack*/ + 2 + U * (D + 3 + 8 * R) + 1 + 4;
  *out = p;
  return SRF_OK;
}

int srf_attentive_v3_forward(const srf_plan* p, const float* const* P, const float* wav, float* out, void* workspace,
                             const float* wav_stats, int mixture_consistency, void* stream) {
  const srf_config& c = p->cfg;
  const int D = c.upsampling_depth, U = c.num_blocks, N = c.enc_num_basis, K = c.enc_kernel_size, R = D - 1;
  const int Bt = p->Bt, L = p->L, nB = p->nB, C = p->nC, H = p->att_heads, d = p->att_dims, HD = H * d;
  const int* lv_len = p->att_lv;
  char* ws = (char*)workspace;
  hipStream_t st = (hipStream_t)stream;
  auto fptr = [&](size_t o) { return (float*)(ws + o); };
  double* stats = (double*)(ws + p->off_stats);
  const size_t each = (size_t)Bt * SRF_STAT_BUCKETS * 2;
  int rc = srf_zero_launch(stats, p->stats_bytes, st);
  if (rc) return rc;

  // ---- K / V weights and biases of every resampler side by side, so that the two projections of the answering side are one
  // convolution
  const size_t wkv_floats = srf_align_up((size_t)2 * HD * C, 64), res_floats = wkv_floats + srf_align_up((size_t)2 * HD, 64);
  std::vector<const float*> wkv((size_t)U * R), bkv((size_t)U * R);
  if (R > 0) {
    std::vector<const float*> src, scale;
    std::vector<float*> dst;
    std::vector<long> n;
    std::vector<float> one;
    for (int i = 0; i < U; ++i)
      for (int r = 0; r < R; ++r) {
        const float* const* A = P + att3_p_base(p, i, r);
        float* w = fptr(p->off_att_wqkv) + ((size_t)i * R + r) * res_floats;
        float* b = w + wkv_floats;
        for (int t = 0; t < 2; ++t) {
          src.push_back(A[SRF_PA_K + 2 * t]), dst.push_back(w + (size_t)t * HD * C), n.push_back((long)HD * C);
          src.push_back(A[SRF_PA_K + 2 * t + 1]), dst.push_back(b + (size_t)t * HD), n.push_back((long)HD);
        }
        wkv[(size_t)i * R + r] = w;
        bkv[(size_t)i * R + r] = b;
      }
    scale.assign(src.size(), nullptr);
    one.assign(src.size(), 1.f);
    rc = srf_causal_scale_many(src.data(), dst.data(), n.data(), scale.data(), one.data(), (int)src.size(), st);
    if (rc) return rc;
  }
  const bool use_pack = plan_use_pack(p);
  if (use_pack) {
    // the image on K_proj.weight's index is that of the concatenated K/V weight
    auto source_of = [&](int param) -> const float* {
      const SrfBlockParam q = plan_block_param(p->p_block0, p->p_block_stride, p->p_tail, param);
      const int a = q.rel - plan_block_params(D, false);
      return q.block >= 0 && a >= 0 && a % SRF_PA_COUNT == SRF_PA_K ? wkv[(size_t)q.block * R + a / SRF_PA_COUNT] : P[param];
    };
    rc = plan_pack_weights(p, source_of, ws, stream);
    if (rc) return rc;
  }
  auto conv = [&](const float* x, const float* w, int param, const float* bias, float* y, int Cin, int Cout, int len,
                  const srf_norm* in_norm, const float* residual, double* out_sums) {
    return srf_pw_conv_packed(x, w, plan_packed(p, ws, use_pack, param), bias, y, Bt, Cin, Cout, len, in_norm, residual, out_sums, 0,
                              nullptr, 0, stream);
  };

  // ---- front end: encoder (+ ln statistics), ln folded into the bottleneck GEMM's operand load
  const SrfFront<const float> f = plan_front(P);
  float* enc = fptr(p->off_enc);
  rc = srf_encoder_impl(wav, f.enc_w, enc, stats, Bt, 1, p->T, N, K, L, wav_stats, stream);
  if (rc) return rc;
  float* cur = fptr(p->off_xa);
  float* nxt = fptr(p->off_xb);
  float* y1 = fptr(p->off_y1);
  {
    const srf_norm ln{stats, f.ln_g, f.ln_b, nullptr};
    rc = conv(enc, f.bott_w, SRF_P_BOTTLENECK, f.bott_b, cur, N, nB, L, &ln, nullptr, nullptr);
    if (rc) return rc;
  }

  // ---- separation module
  float *vp = fptr(p->off_att_x), *kv = fptr(p->off_att_qkv), *qp = fptr(p->off_att_q), *ao = fptr(p->off_att_o),
        *qn = fptr(p->off_att_qn), *ay = fptr(p->off_att_y), *af = fptr(p->off_att_f);
  const float q_normalizer = (float)(1.0 / sqrt((double)d));
  for (int i = 0; i < U; ++i) {
    const SrfBlock<const float> b = plan_block(p, P, i);
    const SrfSlots s = plan_slots(p, stats, i);   // (s.merged: the slot of final_norm; the resamplers' three each follow it)
    rc = conv(cur, b.proj_w, b.i_proj, b.proj_b, y1, nB, C, L, nullptr, nullptr, s.proj);
    if (rc) return rc;
    float* levels[SRF_MAX_DEPTH];
    srf_norm norms[SRF_MAX_DEPTH];
    for (int k = 0; k < D; ++k) {
      const srf_norm in = k == 0 ? srf_norm{s.proj, b.proj_g, b.proj_be, b.proj_prelu} : norms[k - 1];
      float* lv = fptr(p->off_lv[k]);
      rc = srf_dwconv5(k == 0 ? y1 : levels[k - 1], b.lv_w[k], b.lv_b[k], lv, Bt, C, k == 0 ? L : lv_len[k - 1], k == 0 ? 1 : 2, &in,
                       s.level[k], stream);
      if (rc) return rc;
      levels[k] = lv;
      norms[k] = srf_norm{s.level[k], b.lv_g[k], b.lv_be[k], nullptr};
    }
    // ---- the attentive resamplers, deepest pair first; v: the answering tensor and its lazy norm
    const float* v = levels[D - 1];
    srf_norm vnorm = norms[D - 1];
    for (int r = 0; r < R; ++r) {
      const int ql = D - 2 - r, Lq = lv_len[ql], Lk = lv_len[ql + 1];
      const int pa = att3_p_base(p, i, r);
      const float* const* A = P + pa;
      double *s_mha = s.merged + (1 + 3 * r) * each, *s_ffn = s_mha + each, *s_out = s_ffn + each;
      rc = srf_posenc_apply(v, &vnorm, A[SRF_PA_PE], vp, Bt, C, Lk, SRF_ATT_MAX_LEN, stream);
      if (rc) return rc;
      rc = conv(vp, wkv[(size_t)i * R + r], pa + SRF_PA_K, bkv[(size_t)i * R + r], kv, C, 2 * HD, Lk, nullptr, nullptr, nullptr);
      if (rc) return rc;
      rc = conv(levels[ql], A[SRF_PA_Q], pa + SRF_PA_Q, A[SRF_PA_Q + 1], qp, C, HD, Lq, &norms[ql], nullptr, nullptr);
      if (rc) return rc;
      const long s2 = (long)2 * HD * Lk, s1 = (long)HD * Lq;
      const MhaArgs att{qp, kv, kv + (size_t)HD * Lk, ao, s1, s2, s2, s1, H, d, Lq, Lk, q_normalizer};
      rc = srf_mha_forward(0, att, Bt, nullptr, nullptr, nullptr, st);
      if (rc) return rc;
      rc = srf_gln_apply_stats(levels[ql], &norms[ql], qn, nullptr, Bt, C, Lq, stream);
      if (rc) return rc;
      rc = conv(ao, A[SRF_PA_O], pa + SRF_PA_O, A[SRF_PA_O + 1], ay, HD, C, Lq, nullptr, qn, s_mha);
      if (rc) return rc;
      const srf_norm mha_norm{s_mha, A[SRF_PA_MHA_NORM], A[SRF_PA_MHA_NORM + 1], nullptr};
      rc = conv(ay, A[SRF_PA_FFN], pa + SRF_PA_FFN, A[SRF_PA_FFN + 1], af, C, C, Lq, &mha_norm, nullptr, s_ffn);
      if (rc) return rc;
      const srf_norm ffn_norm{s_ffn, A[SRF_PA_FFN_NORM], A[SRF_PA_FFN_NORM + 1], A[SRF_PA_FFN_PRELU]};
      float* z = levels[ql];                  // (the asking level is dead: Q_proj and qn have read it)
      rc = srf_gln_apply2_add(af, &ffn_norm, ay, &mha_norm, z, s_out, Bt, C, Lq, stream);
      if (rc) return rc;
      v = z;
      vnorm = srf_norm{s_out, A[SRF_PA_OUT_NORM], A[SRF_PA_OUT_NORM + 1], nullptr};
    }
    // ---- final_norm over the NORMALISED tensor (into y1: dead once level 0 exists), + PReLU folded into res_conv, + residual
    rc = srf_gln_apply_stats(v, &vnorm, y1, s.merged, Bt, C, L, stream);
    if (rc) return rc;
    const srf_norm fn{s.merged, b.fin_g, b.fin_be, b.fin_prelu};
    rc = conv(y1, b.res_w, b.i_res, b.res_b, nxt, C, nB, L, &fn, cur, nullptr);
    if (rc) return rc;
    float* t = cur;
    cur = nxt;
    nxt = t;
  }

  // ---- mask estimation + decoder: the Improved walk's tail
  return srf_improved_tail(p, P, cur, out, workspace, use_pack, wav_stats, wav, mixture_consistency, nullptr, stream);
}
