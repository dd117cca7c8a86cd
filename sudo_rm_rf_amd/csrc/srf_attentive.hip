// Attentive SuDoRM-RF v2 (attentive_sudormrf_v2.py): the Improved model with a TransformerLayer on the deepest level of every
// U-block.  Plan constructor and the inference walk; every kernel is an existing entry point except the attention and its two
// glue kernels (srf_attention.hip).  Inference only, single stream.
//
// One block (AttentiveUConvBlock.forward), a = level D - 1 of the depthwise pyramid with its lazy GlobLN:
//   y1 = proj_1x1.conv(x)                                     srf_pw_conv_packed   (+ statistics of proj_1x1.norm)
//   d_k = spp_dw[k].conv(norm(d_{k-1})), k = 0 .. D - 1       srf_dwconv5          (per-level path: the fused pyramid cannot
//                                                                                   hand out its deepest level)
//   xp  = GlobLN(d_{D-1}) + pe[:Ld]                           srf_posenc_apply
//   qkv = [Q; K; V]_proj(xp)                                  srf_pw_conv_packed, ONE conv over the concatenated [3 H d, C] weight
//   o   = softmax(q k^T / sqrt(d)) v per head                 srf_mha_attention
//   y   = O_proj(o) + xp                                      srf_pw_conv_packed   (residual, + statistics of out_mha_norm)
//   f   = ffn.conv(out_mha_norm(y))                           srf_pw_conv_packed   (norm on load, + statistics of ffn.norm)
//   z   = PReLU(ffn.norm(f)) + out_mha_norm(y)                srf_gln_apply2_add   (+ statistics of out_norm)
//   merged = upsample-and-add of norm_k(d_k), k < D - 1, and out_norm(z)      srf_merge (z takes level D - 1's place and buffer)
//   x' = res_conv(PReLU(final_norm(merged))) + x              srf_pw_conv_packed
// Front end and tail are those of the Improved walk (srf_api.hip, forward_walk) without the fused conv pairs.
#include <vector>
#include "srf_mha.h"
#include "srf_plan.h"

static long att_gcd(long a, long b) { return b ? att_gcd(b, a % b) : a; }

static inline int att_p_base(const srf_plan* p, int i) { return plan_p_proj(p, i) + plan_block_params(p->cfg.upsampling_depth, false); }

extern "C" int srf_attentive_plan_create(const srf_config* base, int n_heads, int att_dims, int batch, int T, srf_plan** out) {
  SRF_CHECK_ARG(base && out, "srf_attentive_plan_create: null pointer");
  *out = nullptr;
  const srf_config& c = *base;
  SRF_CHECK_ARG(batch > 0 && T > 0, "srf_attentive_plan_create: batch and T must be positive");
  SRF_CHECK_ARG(c.out_channels > 0 && c.in_channels > 0 && c.num_blocks > 0 && c.enc_num_basis > 0 && c.num_sources > 0,
                "srf_attentive_plan_create: non-positive model dimension");
  SRF_CHECK_ARG(c.in_audio_channels == 1 && c.group_size == 1,
                "srf_attentive_plan_create: in_audio_channels and group_size must be 1 (got %d, %d)", c.in_audio_channels, c.group_size);
  SRF_CHECK_ARG(n_heads >= 1 && att_dims >= 1, "srf_attentive_plan_create: n_heads = %d and att_dims = %d must be positive", n_heads,
                att_dims);
  SRF_CHECK_ARG(c.upsampling_depth >= 2,
                "srf_attentive_plan_create: upsampling_depth = %d: the attentive block needs at least 2 levels (the reference's depth-1 "
                "block applies spp_dw[0] twice)", c.upsampling_depth);
  SRF_CHECK_ARG(c.upsampling_depth <= SRF_MAX_DEPTH, "srf_attentive_plan_create: upsampling_depth %d unsupported (2..%d)",
                c.upsampling_depth, SRF_MAX_DEPTH);
  SRF_CHECK_ARG(c.enc_kernel_size >= 3 && (c.enc_kernel_size & 1), "srf_attentive_plan_create: enc_kernel_size must be odd (got %d)",
                c.enc_kernel_size);
  const int D = c.upsampling_depth, U = c.num_blocks, K = c.enc_kernel_size, N = c.enc_num_basis, h = K / 2;
  // pad_to_appropriate_length: up to a multiple of lcm(K / 2, 2^D) -- only when T is not one already
  const long lcm = (long)h * (1L << D) / att_gcd(h, 1L << D);
  const long Tp = T % lcm ? T + lcm - T % lcm : T;
  SRF_CHECK_ARG(Tp <= (1L << 30), "srf_attentive_plan_create: T = %d too long", T);
  const long L = (Tp + 2 * h - K) / h + 1;
  SRF_CHECK_ARG(L % (1L << (D - 1)) == 0,
                "srf_attentive_plan_create: enc_kernel_size = %d, upsampling_depth = %d: %ld frames are not a multiple of 2^(D-1) (the "
                "reference's upsample-and-add fails there too)", K, D, L);
  const long Ld = L >> (D - 1);
  SRF_CHECK_ARG(Ld >= 1, "srf_attentive_plan_create: T = %d leaves the deepest level (Ld) with %ld positions (needs >= 1)", T, Ld);
  SRF_CHECK_ARG(Ld <= SRF_ATT_MAX_LEN,
                "srf_attentive_plan_create: T = %d gives Ld = %ld positions on the deepest level; the position table holds %d", T, Ld,
                SRF_ATT_MAX_LEN);
  SRF_CHECK_ARG(batch <= 65535, "srf_attentive_plan_create: batch %d too large (max 65535 per call)", batch);
  srf_plan* p = new (std::nothrow) srf_plan();
  SRF_CHECK_ARG(p != nullptr, "srf_attentive_plan_create: out of host memory");
  p->cfg = c;
  p->cfg.variant = SRF_VARIANT_ATTENTIVE;
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
  p->att_len = (int)Ld;
  const int C = c.in_channels, HD = n_heads * att_dims;
  // ---- parameters: the Improved layout with SRF_PA_COUNT more tensors per block
  p->p_block0 = SRF_P_FRONT;
  p->p_ublock_off = 0;
  p->p_block_stride = plan_block_params(D, false) + SRF_PA_COUNT;
  p->p_tail = p->p_block0 + U * p->p_block_stride;
  p->n_params = p->p_tail + SRF_P_TAIL;
  // ---- statistic slots: the Improved block's (plan_slots), then out_mha_norm, ffn.norm, out_norm
  p->slots_per_block = D + 2 + 3;
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
  for (int k = 0; k < D; ++k) p->off_lv[k] = take(F * batch * C * (L >> k));
  p->off_masked = take(F * batch * p->SA * N * L);
  p->off_dec = take(F * srf_decoder_scratch_floats(batch, p->SA * N, p->SA, K, p->L));
  p->off_att_x = take(F * batch * C * Ld);
  p->off_att_qkv = take(F * batch * 3 * HD * Ld);
  p->off_att_o = take(F * batch * HD * Ld);
  p->off_att_y = take(F * batch * C * Ld);
  p->off_att_f = take(F * batch * C * Ld);
  // per block: [3 H d, C] weight | [3 H d] bias   (each section 64-float aligned)
  p->off_att_wqkv = take(F * U * (srf_align_up((size_t)3 * HD * C, 64) + srf_align_up((size_t)3 * HD, 64)));
  p->fused_pyramid = 0;
  p->off_pyr = 0;
  // packed (split-bf16) images for the 256 x 128 GEMM, where it takes the shape; the Q/K/V image hangs on Q_proj.weight's index
  p->pk_of_param.assign(p->n_params, 0);
  plan_add_pack(p, &off, SRF_P_BOTTLENECK, c.out_channels, N);
  for (int i = 0; i < U; ++i) {
    plan_add_pack(p, &off, plan_p_proj(p, i), C, c.out_channels);
    plan_add_pack(p, &off, plan_p_res(p, i), c.out_channels, C);
    plan_add_pack(p, &off, att_p_base(p, i) + SRF_PA_Q, 3 * HD, C);
    plan_add_pack(p, &off, att_p_base(p, i) + SRF_PA_O, C, HD);
    plan_add_pack(p, &off, att_p_base(p, i) + SRF_PA_FFN, C, C);
  }
  plan_add_pack(p, &off, plan_p_mask(p), p->SA * N, c.out_channels);
  p->off_wdpack = (p->SA * K <= 64 && p->pk_of_param[plan_p_mask(p)]) ? take(srf_mask_decode_pack_bytes(p->SA * N)) : 0;
  p->total_bytes = off;
  p->n_launches = 1 /*zero*/ + (6 * U + 47) / 48 /*concat*/ + 1 /*pack*/ + 2 + U * (D + 9) + 1 + 4;
  *out = p;
  return SRF_OK;
}

int srf_attentive_forward(const srf_plan* p, const float* const* P, const float* wav, float* out, void* workspace,
                          const float* wav_stats, int mixture_consistency, void* stream) {
  const srf_config& c = p->cfg;
  const int D = c.upsampling_depth, U = c.num_blocks, N = c.enc_num_basis, K = c.enc_kernel_size;
  const int Bt = p->Bt, L = p->L, nB = p->nB, C = p->nC, H = p->att_heads, d = p->att_dims, HD = H * d, Ld = p->att_len;
  char* ws = (char*)workspace;
  hipStream_t st = (hipStream_t)stream;
  auto fptr = [&](size_t o) { return (float*)(ws + o); };
  double* stats = (double*)(ws + p->off_stats);
  const size_t each = (size_t)Bt * SRF_STAT_BUCKETS * 2;
  int rc = srf_zero_launch(stats, p->stats_bytes, st);
  if (rc) return rc;

  // ---- Q / K / V weights and biases of every block side by side, so that the three projections are one convolution
  const size_t wq_floats = srf_align_up((size_t)3 * HD * C, 64), blk_floats = wq_floats + srf_align_up((size_t)3 * HD, 64);
  std::vector<const float*> wqkv(U), bqkv(U);
  {
    std::vector<const float*> src, scale;
    std::vector<float*> dst;
    std::vector<long> n;
    std::vector<float> one;
    for (int i = 0; i < U; ++i) {
      const float* const* A = P + att_p_base(p, i);
      float* w = fptr(p->off_att_wqkv) + (size_t)i * blk_floats;
      float* bq = w + wq_floats;
      for (int t = 0; t < 3; ++t) {
        src.push_back(A[SRF_PA_Q + 2 * t]), dst.push_back(w + (size_t)t * HD * C), n.push_back((long)HD * C);
        src.push_back(A[SRF_PA_Q + 2 * t + 1]), dst.push_back(bq + (size_t)t * HD), n.push_back((long)HD);
      }
      wqkv[i] = w;
      bqkv[i] = bq;
    }
    scale.assign(src.size(), nullptr);
    one.assign(src.size(), 1.f);
    rc = srf_causal_scale_many(src.data(), dst.data(), n.data(), scale.data(), one.data(), (int)src.size(), st);
    if (rc) return rc;
  }
  const bool use_pack = plan_use_pack(p);
  if (use_pack) {
    // the image on Q_proj.weight's index is that of the concatenated Q/K/V weight
    auto source_of = [&](int param) -> const float* {
      const SrfBlockParam q = plan_block_param(p->p_block0, p->p_block_stride, p->p_tail, param);
      return q.block >= 0 && q.rel == plan_block_params(D, false) + SRF_PA_Q ? wqkv[q.block] : P[param];
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
  float *xp = fptr(p->off_att_x), *qkv = fptr(p->off_att_qkv), *ao = fptr(p->off_att_o), *ay = fptr(p->off_att_y),
        *af = fptr(p->off_att_f);
  const float q_normalizer = (float)(1.0 / sqrt((double)d));
  for (int i = 0; i < U; ++i) {
    const SrfBlock<const float> b = plan_block(p, P, i);
    const SrfSlots s = plan_slots(p, stats, i);
    double *s_mha = s.merged + each, *s_ffn = s.merged + 2 * each, *s_out = s.merged + 3 * each;
    const int pa = att_p_base(p, i);
    const float* const* A = P + pa;
    rc = conv(cur, b.proj_w, b.i_proj, b.proj_b, y1, nB, C, L, nullptr, nullptr, s.proj);
    if (rc) return rc;
    // the pyramid level by level; the deepest one stays un-merged until the transformer layer has replaced it
    const float* levels[SRF_MAX_DEPTH];
    srf_norm norms[SRF_MAX_DEPTH];
    for (int k = 0; k < D; ++k) {
      const srf_norm in = k == 0 ? srf_norm{s.proj, b.proj_g, b.proj_be, b.proj_prelu} : norms[k - 1];
      float* lv = fptr(p->off_lv[k]);
      rc = srf_dwconv5(k == 0 ? y1 : levels[k - 1], b.lv_w[k], b.lv_b[k], lv, Bt, C, k == 0 ? L : L >> (k - 1), k == 0 ? 1 : 2, &in,
                       s.level[k], stream);
      if (rc) return rc;
      levels[k] = lv;
      norms[k] = srf_norm{s.level[k], b.lv_g[k], b.lv_be[k], nullptr};
    }
    // ---- TransformerLayer on level D - 1
    rc = srf_posenc_apply(levels[D - 1], &norms[D - 1], A[SRF_PA_PE], xp, Bt, C, Ld, SRF_ATT_MAX_LEN, stream);
    if (rc) return rc;
    rc = conv(xp, wqkv[i], pa + SRF_PA_Q, bqkv[i], qkv, C, 3 * HD, Ld, nullptr, nullptr, nullptr);
    if (rc) return rc;
    const long s3 = (long)3 * HD * Ld;
    const MhaArgs att{qkv, qkv + (size_t)HD * Ld, qkv + (size_t)2 * HD * Ld, ao, s3, s3, s3, (long)HD * Ld, H, d, Ld, Ld, q_normalizer};
    rc = srf_mha_forward(0, att, Bt, nullptr, nullptr, nullptr, st);
    if (rc) return rc;
    rc = conv(ao, A[SRF_PA_O], pa + SRF_PA_O, A[SRF_PA_O + 1], ay, HD, C, Ld, nullptr, xp, s_mha);
    if (rc) return rc;
    const srf_norm mha_norm{s_mha, A[SRF_PA_MHA_NORM], A[SRF_PA_MHA_NORM + 1], nullptr};
    rc = conv(ay, A[SRF_PA_FFN], pa + SRF_PA_FFN, A[SRF_PA_FFN + 1], af, C, C, Ld, &mha_norm, nullptr, s_ffn);
    if (rc) return rc;
    const srf_norm ffn_norm{s_ffn, A[SRF_PA_FFN_NORM], A[SRF_PA_FFN_NORM + 1], A[SRF_PA_FFN_PRELU]};
    float* z = fptr(p->off_lv[D - 1]);      // (level D - 1 is dead since srf_posenc_apply)
    rc = srf_gln_apply2_add(af, &ffn_norm, ay, &mha_norm, z, s_out, Bt, C, Ld, stream);
    if (rc) return rc;
    norms[D - 1] = srf_norm{s_out, A[SRF_PA_OUT_NORM], A[SRF_PA_OUT_NORM + 1], nullptr};
    // ---- upsample-and-add (into y1: dead once level 0 exists), final_norm + PReLU folded into res_conv, + residual
    rc = srf_merge(levels, norms, D, y1, Bt, C, L, s.merged, stream);
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
