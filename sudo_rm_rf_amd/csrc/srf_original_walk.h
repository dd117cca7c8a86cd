// The original SuDoRM-RF's ONE forward walk (orig_walk) and its step helpers, for its two callers: srf_original_forward
// (srf_original.hip: inference and ragged) and srf_original_forward_train (srf_original_train.hip).  Each caller keeps its own
// addresses, pack and conv beside its own layout.
#pragma once
#include "srf_plan.h"

// ---- the steps of the walk, one per kernel family: the uniform entry point, or -- rg != NULL, srf_original_forward_ragged --
// its ragged twin with the batch's tables.  Every per-launch refusal stays with the entry point.
static inline int orig_encoder(const Ragged* rg, const float* wav, const float* w, const float* bias, float* enc, double* sums, int Bt, int T,
                        int N, int K, int L, const float* wav_stats, void* stream) {
  return rg ? srf_encoder_bias_relu_ragged(wav, w, bias, enc, sums, Bt, T, N, K, L, rg->lengths, rg->frames, wav_stats, stream)
            : srf_encoder_bias_relu(wav, w, bias, enc, sums, Bt, T, N, K, L, wav_stats, stream);
}
// ragged: always the 256 x 128 kernel (the gate has made sure every conv of the model has a packed image and a shape it takes)
static inline int orig_conv(const Ragged* rg, const float* x, const float* w, const void* w_packed, const float* bias, float* y, int Bt, int Cin,
                     int Cout, int L, const srf_norm* in_norm, double* out_sums, void* stream) {
  return rg ? srf_pw_conv_packed_ragged(x, w, w_packed, bias, y, Bt, Cin, Cout, L, in_norm, nullptr, out_sums, 0, nullptr, 0, rg->frames,
                                        stream)
            : srf_pw_conv_packed(x, w, w_packed, bias, y, Bt, Cin, Cout, L, in_norm, nullptr, out_sums, 0, nullptr, 0, stream);
}
static inline int orig_gln(const Ragged* rg, const float* x, const srf_norm* norm, const float* slopes, const float* add, float* y,
                    double* out_sums, int Bt, int C, int L, void* stream) {
  return rg ? srf_gln_apply_c_ragged(x, norm, slopes, add, y, out_sums, Bt, C, L, rg->frames, stream)
            : srf_gln_apply_c(x, norm, slopes, add, y, out_sums, Bt, C, L, stream);
}
// the fused pyramid over the materialised activation: no norm on load
static inline int orig_pyramid(const Ragged* rg, const float* act, float* merged, const SrfOrigBlock& b, int Bt, int C, int L, int D,
                        void* scratch, double* out_sums, void* stream) {
  return rg ? srf_pyramid_ragged(act, merged, nullptr, b.lv_w, b.lv_b, b.lv_g, b.lv_be, Bt, C, L, D, scratch, out_sums, rg->frames, stream)
            : srf_pyramid(act, merged, nullptr, b.lv_w, b.lv_b, b.lv_g, b.lv_be, Bt, C, L, D, scratch, out_sums, stream);
}
static inline int orig_softmax(const Ragged* rg, const float* z, const float* enc, float* v, int Bt, int S, int N, int L, void* stream) {
  return rg ? srf_softmax_mask_ragged(z, enc, v, Bt, S, N, L, rg->frames, stream) : srf_softmax_mask(z, enc, v, Bt, S, N, L, stream);
}
static inline int orig_bias(const Ragged* rg, float* out, const float* bias, const float* wav_stats, const float* wav, int mc, int Bt, int S,
                     int T, void* stream) {
  return rg ? srf_bias_rescale_ragged_launch(out, bias, wav_stats, wav, mc, Bt, S, T, rg->lens_t, stream)
            : srf_bias_rescale(out, bias, wav_stats, wav, mc, Bt, S, T, stream);
}

// THE walk of the original model's forward: srf_forward, srf_separate (wav_stats), srf_original_forward_ragged (rg),
// srf_original_separate_ragged (both) -- srf_original_forward, srf_original.hip -- and srf_original_forward_train.
// The callers differ in four things, and pass them:
//   a      where each tensor lives (srf_internal.h);
//   pack   pack(tz): packs the caller's weight images, the Toeplitz weight's among them -- after the two weight forms, before the
//          encoder;
//   conv   conv(x, w, parameter index of w, bias, y, Cin, Cout, in_norm, out_sums): a 1x1 convolution over the caller's image of w;
//   fused  whether the pyramid runs as the fused kernels (its result then has no raw levels: the training forward never does).
// The ragged forward keeps the layout -- [batch, C, L] with L the PLAN's frame count as row stride, the same workspace carve-up --
// and every kernel takes the example's own frame count L_b (its own length padded by THIS model's rule, lcm(hop, 2^D), over the
// hop) from a by-value table.  The invariants:
//   * every tensor whose GlobLN statistics are taken -- s, y1, the merged pyramid output m, g and g + x -- is exactly zero on
//     [L_b, L), so the sums come out right and only the count changes (C * L_b);
//   * a and e (srf_gln_apply_c's outputs, the pyramid's and conv_1x1_exp's inputs) are zero there too: the pyramid reads its
//     input with a halo only up to L_b, the GEMM is pointwise;
//   * the block stream x is written by srf_gln_apply_c, so it is zero there as well.  l1's output is the one block-stream tensor
//     the invariant does not rest on (only pointwise consumers read it: proj_1x1 and, below L_b, the residual add);
//   * the mask logits z are unspecified on [L_b, L): srf_softmax_mask reads neither them nor s there and stores v as exact
//     zeros, so the decoder's frame GEMM (unchanged, over every column) sees zeros and the ragged overlap-add reads the example's
//     own frames only; out is exactly 0 from the example's length on.
// srf_mask_weight_fill, srf_decoder_weight_expand, the mask GEMM / reshape_before_masks (the plain ragged GEMM) and the decoder's
// transpose + frame GEMM run over every column.
template <typename Pack, typename Conv>
static inline int orig_walk(const srf_plan* p, const float* const* P, const float* wav, float* out, const SrfOrigAddrs& a, Pack pack,
                            Conv conv, bool fused, const Ragged* rg, const float* wav_stats, int mixture_consistency, void* stream) {
  const srf_config& c = p->cfg;
  const int D = c.upsampling_depth, U = c.num_blocks, N = c.enc_num_basis, K = c.enc_kernel_size, S = c.num_sources;
  const int Bt = p->Bt, L = p->L, B = p->nB, C = p->nC;
  const SrfOrigFront f = orig_front(P);
  const SrfOrigTail t = orig_tail(p, P);
  int rc = srf_zero_launch(a.stats, p->stats_bytes, (hipStream_t)stream);
  if (rc) return rc;
  rc = srf_original_weight_forms(p, P, a.tz, a.wdec, stream);
  if (rc) return rc;
  rc = pack(a.tz);
  if (rc) return rc;

  // ---- front end: encoder with bias and ReLU (+ ln statistics), ln folded into l1's operand load
  rc = orig_encoder(rg, wav, f.enc_w, f.enc_b, a.enc, a.stats, Bt, p->T, N, K, L, wav_stats, stream);
  if (rc) return rc;
  {
    const srf_norm ln{a.stats, f.ln_g, f.ln_b, nullptr};
    rc = conv(a.enc, f.l1_w, SRF_PO_L1, f.l1_b, a.x_in(0), N, B, &ln, nullptr);
    if (rc) return rc;
  }

  // ---- separation module
  for (int i = 0; i < U; ++i) {
    const SrfOrigBlock b = orig_block(p, P, i);
    const SrfOrigSlots s = orig_slots(p, a.stats, i);
    float *x = a.x_in(i), *y1 = a.y1(i), *m = a.m(i), *g = a.g(i), *gx = a.gx(i);
    rc = conv(x, b.proj_w, b.i_proj, b.proj_b, y1, B, C, nullptr, s.proj);
    if (rc) return rc;
    const srf_norm pn{s.proj, b.proj_g, b.proj_be, nullptr};
    rc = orig_gln(rg, y1, &pn, b.proj_slope, nullptr, a.act, nullptr, Bt, C, L, stream);
    if (rc) return rc;
    // the pyramid, its result m (the inference forward: into y1, dead since a exists) with the statistics of final_norm: the
    // fused kernels where they take the shape, else level by level + merge (D = 1: the normalised level 0).  Either way level 0
    // reads the materialised activation as it is, no norm on load
    if (fused) {
      rc = orig_pyramid(rg, a.act, m, b, Bt, C, L, D, a.pyr, s.merged, stream);
    } else {
      float* lv[SRF_MAX_DEPTH];
      for (int k = 0; k < D; ++k) lv[k] = a.lv(i, k);
      rc = srf_pyramid_per_level(a.act, nullptr, lv, m, b.lv_w, b.lv_b, b.lv_g, b.lv_be, s.level, s.merged, Bt, C, L, D, stream);
    }
    if (rc) return rc;
    // final_norm + PReLU_c (into a's buffer)
    const srf_norm fn{s.merged, b.fin_g, b.fin_be, nullptr};
    rc = orig_gln(rg, m, &fn, b.fin_slope, nullptr, a.act, nullptr, Bt, C, L, stream);
    if (rc) return rc;
    rc = conv(a.act, b.exp_w, b.i_exp, b.exp_b, g, C, B, nullptr, s.exp);
    if (rc) return rc;
    // the residual goes in BEFORE module_act's norm
    const srf_norm en{s.exp, b.exp_g, b.exp_be, nullptr};
    rc = orig_gln(rg, g, &en, nullptr, x, gx, s.act, Bt, B, L, stream);
    if (rc) return rc;
    const srf_norm an{s.act, b.act_g, b.act_be, nullptr};
    rc = orig_gln(rg, gx, &an, b.act_slope, nullptr, a.x_out(i), nullptr, Bt, B, L, stream);
    if (rc) return rc;
  }

  // ---- masks: [reshape_before_masks,] the basis-axis convolution as a GEMM, softmax over the sources times the encoder output
  const float* xm = a.x_in(U);
  if (orig_has_reshape(p)) {
    rc = conv(xm, t.rs_w, t.i_rs, t.rs_b, a.xr, B, N, nullptr, nullptr);
    if (rc) return rc;
    xm = a.xr;
  }
  rc = conv(xm, a.tz, t.i_m, a.tz + orig_tz_bias_at(S, N), a.z, N, S * N, nullptr, nullptr);
  if (rc) return rc;
  rc = orig_softmax(rg, a.z, a.enc, a.masked, Bt, S, N, L, stream);
  if (rc) return rc;
  // ---- decoder: the frame GEMM + overlap-add over the block-diagonal weight, then the bias (+ the callers' recipe)
  rc = srf_decoder_impl(a.masked, a.wdec, out, Bt, S * N, S, K, L, p->T, a.dec, nullptr, nullptr, 0, stream, nullptr,
                        rg ? &rg->lens_t : nullptr, rg ? &rg->frames_t : nullptr);
  if (rc) return rc;
  return orig_bias(rg, out, t.dec_b, wav_stats, wav, mixture_consistency, Bt, S, p->T, stream);
}
