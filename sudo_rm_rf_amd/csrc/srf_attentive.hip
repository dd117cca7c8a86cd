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
// A ragged batch (opt-in: srf_attentive_forward_ragged / srf_attentive_separate_ragged) is the SAME walk
// with a Ragged: every step picks its ragged twin with example b's own frames[b] >> k columns at level k, and every 1x1
// convolution goes through att_conv_ragged, which decides per launch.
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

// One 1x1 convolution of the ragged walk, decided PER LAUNCH: (1) the 256 x 128 packed ragged GEMM where its gate, its built
// forms, its statistics table and its "at least 8 tiles" pass; (2) the 128 x 128 ragged GEMM where its gate passes; (3) what
// neither takes (Cin % 64 != 0, a row stride off the grid of 4): the uniform GEMM over every column without out_sums -- columns
// are independent, no consumer reads past an example's end -- with srf_gln_stats_ragged for the statistics it should leave behind
// and srf_sums_scale_ragged (into `rsums`) in front of a norm on load.
static int att_conv_ragged(const float* x, const float* w, const void* w_packed, const float* bias, float* y, int Bt, int Cin, int Cout,
                           int len, const srf_norm* in_norm, const float* residual, double* out_sums, const int* frames, double* rsums,
                           void* stream) {
  const int pro = in_norm ? (in_norm->sums ? (in_norm->prelu ? 2 : 1) : (in_norm->prelu ? 3 : 0)) : 0;
  const bool packed_form = pro != 3 && (pro == 2) == (residual != nullptr) && !(pro == 2 && out_sums);
  if (w_packed && packed_form && srf_x3w_supported(Bt, pro) && (long)Bt * ((Cout + 255) / 256) * ((len + 127) / 128) >= 8 &&
      srf_pw_conv_packed_ragged_supported(Bt, Cin, Cout, len, frames))
    return srf_pw_conv_packed_ragged(x, w, w_packed, bias, y, Bt, Cin, Cout, len, in_norm, residual, out_sums, 0, nullptr, 0, frames,
                                     stream);
  if (srf_pw_conv_ragged_supported(Bt, Cin, Cout, len, frames))
    return srf_pw_conv_ragged(x, w, bias, y, Bt, Cin, Cout, len, in_norm, residual, out_sums, frames, stream);
  srf_norm scaled;
  if (in_norm && in_norm->sums) {
    const int rc = srf_sums_scale_ragged(in_norm->sums, rsums, Bt, len, frames, stream);
    if (rc) return rc;
    scaled = *in_norm;
    scaled.sums = rsums;
    in_norm = &scaled;
  }
  const int rc = srf_pw_conv_packed(x, w, w_packed, bias, y, Bt, Cin, Cout, len, in_norm, residual, nullptr, 0, nullptr, 0, stream);
  if (rc || !out_sums) return rc;
  return srf_gln_stats_ragged(y, out_sums, Bt, Cout, len, frames, stream);
}

int srf_attentive_forward(const srf_plan* p, const float* const* P, const float* wav, float* out, void* workspace,
                          const float* wav_stats, int mixture_consistency, void* stream, const Ragged* rg) {
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
  // ragged: example b's own columns at level k (its frames are a multiple of 2^(D-1): K = 21, see the gate)
  std::vector<int> fr_lv(rg ? (size_t)D * Bt : 0);
  for (int k = 0; rg && k < D; ++k)
    for (int e = 0; e < Bt; ++e) fr_lv[(size_t)k * Bt + e] = rg->frames[e] >> k;
  const int *fr0 = rg ? fr_lv.data() : nullptr, *frd = rg ? fr_lv.data() + (size_t)(D - 1) * Bt : nullptr;
  // the scaled sums a uniform GEMM's norm on load takes (att_conv_ragged): one statistics slot at the start of the masked tensor's
  // region, which is dead until the tail (the gate has made sure it is large enough)
  double* rsums = (double*)(ws + p->off_masked);
  // fr: the ragged batch's table at the conv's level (fr0 or frd; NULL in the uniform walk)
  auto conv = [&](const float* x, const float* w, int param, const float* bias, float* y, int Cin, int Cout, int len, const int* fr,
                  const srf_norm* in_norm, const float* residual, double* out_sums) {
    const void* packed = plan_packed(p, ws, use_pack, param);
    if (rg) return att_conv_ragged(x, w, packed, bias, y, Bt, Cin, Cout, len, in_norm, residual, out_sums, fr, rsums, stream);
    return srf_pw_conv_packed(x, w, packed, bias, y, Bt, Cin, Cout, len, in_norm, residual, out_sums, 0, nullptr, 0, stream);
  };

  // ---- front end: encoder (+ ln statistics), ln folded into the bottleneck GEMM's operand load
  const SrfFront<const float> f = plan_front(P);
  float* enc = fptr(p->off_enc);
  rc = rg ? srf_encoder_ragged_impl(wav, f.enc_w, enc, stats, Bt, 1, p->T, N, K, L, rg->lengths, rg->frames, wav_stats, stream)
          : srf_encoder_impl(wav, f.enc_w, enc, stats, Bt, 1, p->T, N, K, L, wav_stats, stream);
  if (rc) return rc;
  float* cur = fptr(p->off_xa);
  float* nxt = fptr(p->off_xb);
  float* y1 = fptr(p->off_y1);
  {
    const srf_norm ln{stats, f.ln_g, f.ln_b, nullptr};
    rc = conv(enc, f.bott_w, SRF_P_BOTTLENECK, f.bott_b, cur, N, nB, L, fr0, &ln, nullptr, nullptr);
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
    rc = conv(cur, b.proj_w, b.i_proj, b.proj_b, y1, nB, C, L, fr0, nullptr, nullptr, s.proj);
    if (rc) return rc;
    // the pyramid level by level; the deepest one stays un-merged until the transformer layer has replaced it
    const float* levels[SRF_MAX_DEPTH];
    srf_norm norms[SRF_MAX_DEPTH];
    for (int k = 0; k < D; ++k) {
      const srf_norm in = k == 0 ? srf_norm{s.proj, b.proj_g, b.proj_be, b.proj_prelu} : norms[k - 1];
      float* lv = fptr(p->off_lv[k]);
      const float* src = k == 0 ? y1 : levels[k - 1];
      const int Lin = k == 0 ? L : L >> (k - 1), stride = k == 0 ? 1 : 2;
      rc = rg ? srf_dwconv5_ragged(src, b.lv_w[k], b.lv_b[k], lv, Bt, C, Lin, stride, &in, s.level[k],
                                   fr_lv.data() + (size_t)(k == 0 ? 0 : k - 1) * Bt, stream)
              : srf_dwconv5(src, b.lv_w[k], b.lv_b[k], lv, Bt, C, Lin, stride, &in, s.level[k], stream);
      if (rc) return rc;
      levels[k] = lv;
      norms[k] = srf_norm{s.level[k], b.lv_g[k], b.lv_be[k], nullptr};
    }
    // ---- TransformerLayer on level D - 1
    rc = rg ? srf_posenc_apply_ragged(levels[D - 1], &norms[D - 1], A[SRF_PA_PE], xp, Bt, C, Ld, SRF_ATT_MAX_LEN, frd, stream)
            : srf_posenc_apply(levels[D - 1], &norms[D - 1], A[SRF_PA_PE], xp, Bt, C, Ld, SRF_ATT_MAX_LEN, stream);
    if (rc) return rc;
    rc = conv(xp, wqkv[i], pa + SRF_PA_Q, bqkv[i], qkv, C, 3 * HD, Ld, frd, nullptr, nullptr, nullptr);
    if (rc) return rc;
    const long s3 = (long)3 * HD * Ld;
    const MhaArgs att{qkv, qkv + (size_t)HD * Ld, qkv + (size_t)2 * HD * Ld, ao, s3, s3, s3, (long)HD * Ld, H, d, Ld, Ld, q_normalizer};
    rc = srf_mha_forward(rg ? SRF_MHA_RAGGED : 0, att, Bt, nullptr, frd, frd, st);
    if (rc) return rc;
    rc = conv(ao, A[SRF_PA_O], pa + SRF_PA_O, A[SRF_PA_O + 1], ay, HD, C, Ld, frd, nullptr, xp, s_mha);
    if (rc) return rc;
    const srf_norm mha_norm{s_mha, A[SRF_PA_MHA_NORM], A[SRF_PA_MHA_NORM + 1], nullptr};
    rc = conv(ay, A[SRF_PA_FFN], pa + SRF_PA_FFN, A[SRF_PA_FFN + 1], af, C, C, Ld, frd, &mha_norm, nullptr, s_ffn);
    if (rc) return rc;
    const srf_norm ffn_norm{s_ffn, A[SRF_PA_FFN_NORM], A[SRF_PA_FFN_NORM + 1], A[SRF_PA_FFN_PRELU]};
    float* z = fptr(p->off_lv[D - 1]);      // (level D - 1 is dead since srf_posenc_apply)
    rc = rg ? srf_gln_apply2_add_ragged(af, &ffn_norm, ay, &mha_norm, z, s_out, Bt, C, Ld, frd, stream)
            : srf_gln_apply2_add(af, &ffn_norm, ay, &mha_norm, z, s_out, Bt, C, Ld, stream);
    if (rc) return rc;
    norms[D - 1] = srf_norm{s_out, A[SRF_PA_OUT_NORM], A[SRF_PA_OUT_NORM + 1], nullptr};
    // ---- upsample-and-add (into y1: dead once level 0 exists), final_norm + PReLU folded into res_conv, + residual
    rc = rg ? srf_merge_ragged(levels, norms, D, y1, Bt, C, L, s.merged, fr0, stream)
            : srf_merge(levels, norms, D, y1, Bt, C, L, s.merged, stream);
    if (rc) return rc;
    const srf_norm fn{s.merged, b.fin_g, b.fin_be, b.fin_prelu};
    rc = conv(y1, b.res_w, b.i_res, b.res_b, nxt, C, nB, L, fr0, &fn, cur, nullptr);
    if (rc) return rc;
    float* t = cur;
    cur = nxt;
    nxt = t;
  }

  // ---- mask estimation + decoder: the Improved walk's tail
  return srf_improved_tail(p, P, cur, out, workspace, use_pack, wav_stats, wav, mixture_consistency, rg, stream);
}

// ---------------------------------------------------------------------------------------------
// ragged forward (opt-in: srf_plan_ragged_supported / srf_forward_ragged / srf_separate_ragged keep refusing an attentive plan)
// ---------------------------------------------------------------------------------------------
// The gate.  There is none on the GEMM shapes (att_conv_ragged has a path for every launch) and none on the tail.  With K = 21 the
// hop is 10, an example's own padded length is a multiple of lcm(10, 2^D) = 5 * 2^D, so its frame count is a multiple of 2^(D-1):
// what the merge needs; no length inside 1..T is refused for its grid.
static bool att_ragged_now(const srf_plan* p, const char** why) {
  auto no = [&](const char* w) {
    if (why) *why = w;
    return false;
  };
  if (p->cfg.variant != SRF_VARIANT_ATTENTIVE) return no("not a plan of srf_attentive_plan_create");
  if (p->A != 1 || p->cfg.enc_kernel_size != 21) return no("the ragged encoder is the one-channel K = 21 kernel");
  if (srf_kernel_mode() == 1) return no("kernel mode 1 (generic kernels only) has no ragged encoder");
  if (p->Bt > SRF_RAGGED_MAX_BATCH) return no("the batch exceeds SRF_RAGGED_MAX_BATCH");
  // (the walk keeps one statistics slot of scaled sums in the masked tensor's region while the blocks run)
  if ((size_t)p->SA * p->cfg.enc_num_basis * p->L * sizeof(float) < SRF_STAT_BUCKETS * 2 * sizeof(double))
    return no("the model is too small (sources x basis x frames < 256)");
  return true;
}
extern "C" int srf_attentive_ragged_supported(const srf_plan* p) { return p && att_ragged_now(p, nullptr) ? 1 : 0; }
extern "C" size_t srf_attentive_ragged_workspace_bytes(const srf_plan* p) { return p && att_ragged_now(p, nullptr) ? p->total_bytes : 0; }

// What the two entry points (`who`) share: the gate, the argument checks and every example's own padded length, as its batch-1
// plan would have it -- all refusals BEFORE the first launch
static int att_ragged_prepare(const char* who, const srf_plan* p, const float* const* P, int num_params, const int* lengths,
                              const void* workspace, size_t workspace_bytes, Ragged* rg) {
  const char* why = "";
  SRF_CHECK_ARG(att_ragged_now(p, &why), "%s: plan not supported by the attentive model's ragged forward: %s", who, why);
  int rc = forward_check_args(who, true /* checked by the caller */, p, P, num_params, workspace, workspace_bytes);
  if (rc) return rc;
  const int D = p->cfg.upsampling_depth, h = p->cfg.enc_kernel_size / 2;
  const long lcm = (long)h * (1L << D) / att_gcd(h, 1L << D);
  rg->lengths = lengths;
  for (int b = 0; b < p->Bt; ++b) {
    SRF_CHECK_ARG(lengths[b] >= 1 && lengths[b] <= p->T, "%s: example %d has length %d (allowed: 1..%d)", who, b, lengths[b], p->T);
    const long Tp = lengths[b] % lcm ? lengths[b] + lcm - lengths[b] % lcm : lengths[b];   // the example alone, padded by the model's rule
    rg->frames[b] = (int)(Tp / h);
    SRF_CHECK_ARG(rg->frames[b] <= p->L && rg->frames[b] % (1 << (D - 1)) == 0,
                  "%s: example %d (length %d = %d frames) is off the grid of 2^(D-1) frames or longer than the plan", who, b, lengths[b],
                  rg->frames[b]);
  }
  rc = srf_frames_table(who, lengths, p->Bt, p->T, &rg->lens_t);
  if (rc) return rc;
  return srf_frames_table(who, rg->frames, p->Bt, p->L, &rg->frames_t);
}

extern "C" int srf_attentive_forward_ragged(const srf_plan* p, const float* const* P, int num_params, const float* wav, const int* lengths,
                                            float* out, void* workspace, size_t workspace_bytes, void* stream) {
  SRF_CHECK_ARG(p && P && wav && lengths && out && workspace, "srf_attentive_forward_ragged: null pointer");
  Ragged rg;
  const int rc = att_ragged_prepare("srf_attentive_forward_ragged", p, P, num_params, lengths, workspace, workspace_bytes, &rg);
  if (rc) return rc;
  if (srf_profiling()) srf_prof_mark("(gap)", (hipStream_t)stream);
  return srf_attentive_forward(p, P, wav, out, workspace, nullptr, 0, stream, &rg);
}

// srf_separate over a ragged batch: the ragged forward with a statistics launch over every row's own samples in front, the
// normalisation in the ragged encoder's load and the rescale (+ mixture consistency) in the ragged overlap-add.  wav: the RAW padded
// mixture; nothing at or past lengths[b] is read by any of the three.
extern "C" int srf_attentive_separate_ragged(const srf_plan* p, const float* const* P, int num_params, const float* wav,
                                             const int* lengths, float* out, float* stats, int mixture_consistency, void* workspace,
                                             size_t workspace_bytes, void* stream) {
  SRF_CHECK_ARG(p && P && wav && lengths && out && stats && workspace, "srf_attentive_separate_ragged: null pointer");
  Ragged rg;
  int rc = att_ragged_prepare("srf_attentive_separate_ragged", p, P, num_params, lengths, workspace, workspace_bytes, &rg);
  if (rc) return rc;
  if (srf_profiling()) srf_prof_mark("(gap)", (hipStream_t)stream);
  rc = srf_wav_stats_ragged_launch(wav, rg.lens_t, stats, p->Bt, p->T, (hipStream_t)stream);
  if (rc) return rc;
  return srf_attentive_forward(p, P, wav, out, workspace, stats, mixture_consistency, stream, &rg);
}
