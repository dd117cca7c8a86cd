// The Improved / GroupComm model's ONE forward walk (improved_walk) and its step helpers, for its two callers: forward_walk
// (srf_api.hip: srf_forward, srf_separate and their ragged forms) and srf_forward_train (srf_train.hip).  Each caller keeps its own
// addresses, its way of clearing the statistics, its weight images and its tail beside its own layout.
#pragma once
#include "srf_plan.h"

// ---- the steps of the walk, one per kernel family: the uniform entry point, or -- rg != NULL, srf_forward_ragged -- its ragged
// twin with the batch's frame counts.  Every per-launch refusal stays with the entry point.
// (struct Ragged: srf_internal.h)
static inline int imp_encoder(const Ragged* rg, const float* wav, const float* w, float* enc, double* sums, int Bt, int A, int T, int N,
                              int K, int L, const float* wav_stats, void* stream) {
  return rg ? srf_encoder_ragged_impl(wav, w, enc, sums, Bt, A, T, N, K, L, rg->lengths, rg->frames, wav_stats, stream)
            : srf_encoder_impl(wav, w, enc, sums, Bt, A, T, N, K, L, wav_stats, stream);
}
// rows = examples * rows_per_example (GroupComm's per-group convs run over the folded rows).  Ragged: as in srf_pw_conv_packed
// the thin-shape kernel has precedence, everything else is the 256 x 128 kernel (rows_per_example = 1)
static inline int imp_conv(const Ragged* rg, int rows_per_example, const float* x, const float* w, const void* w_packed, const float* bias,
                           float* y, int rows, int Cin, int Cout, int L, const srf_norm* in_norm, const float* residual, double* out_sums,
                           void* stream) {
  if (!rg) return srf_pw_conv_packed(x, w, w_packed, bias, y, rows, Cin, Cout, L, in_norm, residual, out_sums, 0, nullptr, 0, stream);
  if (srf_pw_small_ragged_supported(Cin, Cout, L))
    return srf_pw_conv_small_ragged(x, w, bias, y, rows, Cin, Cout, L, in_norm, residual, out_sums, nullptr, nullptr, nullptr,
                                    rg->frames, rows_per_example, stream);
  return srf_pw_conv_packed_ragged(x, w, w_packed, bias, y, rows, Cin, Cout, L, in_norm, residual, out_sums, 0, nullptr, 0, rg->frames,
                                   stream);
}
static inline int imp_pair(const Ragged* rg, const float* x, const void* w1_packed, const float* bias1, float* y, const srf_norm* in_norm,
                           const float* residual, const void* w2_packed, const float* bias2, float* y2, double* out_sums2, int Bt, int Cin1,
                           int Cmid, int Cout2, int L, void* stream) {
  return rg ? srf_pw_conv_pair_ragged(x, w1_packed, bias1, y, in_norm, residual, w2_packed, bias2, y2, out_sums2, Bt, Cin1, Cmid, Cout2,
                                      L, rg->frames, stream)
            : srf_pw_conv_pair(x, w1_packed, bias1, y, in_norm, residual, w2_packed, bias2, y2, out_sums2, Bt, Cin1, Cmid, Cout2, L,
                               stream);
}
static inline int imp_tac(const Ragged* rg, const float* x, float* q, const float* const* params, int Bt, int G, int n, int H, int L,
                          double* out_sums, void* stream) {
  return rg ? srf_tac_ragged(x, q, params, Bt, G, n, H, L, out_sums, rg->frames, stream)
            : srf_tac(x, q, params, Bt, G, n, H, L, out_sums, stream);
}
// proj_1x1 with u = x + GlobLN(q) folded into its operand load (u is written for the block's residual as it goes)
static inline int imp_preadd(const Ragged* rg, int G, const float* x, const float* q, const srf_norm* qnorm, float* u, const float* w,
                             const float* bias, float* y, int Bg, int Cin, int Cout, int L, double* out_sums, void* stream) {
  return rg ? srf_pw_conv_small_ragged(x, w, bias, y, Bg, Cin, Cout, L, nullptr, nullptr, out_sums, q, qnorm, u, rg->frames, G, stream)
            : srf_pw_conv_preadd(x, q, qnorm, u, w, bias, y, Bg, Cin, Cout, L, out_sums, (hipStream_t)stream);
}
// the fused pyramid: two passes with every level kept on chip (srf_pyramid.hip), over G folded rows per example.  lv_out /
// lv_sums (both or neither, uniform only): the raw levels and their statistics on the side, as srf_pyramid_impl takes them
static inline int imp_pyramid(const Ragged* rg, int G, const float* y1, float* merged, const srf_norm* in_norm,
                              const SrfBlock<const float>& b, int Bg, int C, int L, int D, void* scratch, double* out_sums,
                              float* const* lv_out, double* const* lv_sums, void* stream) {
  return rg ? srf_pyramid_ragged_rows(y1, merged, in_norm, b.lv_w, b.lv_b, b.lv_g, b.lv_be, Bg, C, L, D, scratch, out_sums, rg->frames, G,
                                      stream)
            : srf_pyramid_impl(y1, merged, in_norm, b.lv_w, b.lv_b, b.lv_g, b.lv_be, Bg, C, L, D, scratch, out_sums, lv_out, lv_sums, stream);
}
// the ragged form reads the example's own frames only; its post-processing (wav_stats: srf_separate_ragged) stays on the example's
// own samples
static inline int imp_overlap_add(const Ragged* rg, const float* z, float* out, int Bt, int Co, int K, int L, int T, int nparts,
                                  const float* wav_stats, const float* wav, int mc, hipStream_t st) {
  return rg ? srf_overlap_add_launch(z, out, Bt, Co, K, L, T, nparts, wav_stats, wav, mc, st, &rg->lens_t, &rg->frames_t)
            : srf_overlap_add_launch(z, out, Bt, Co, K, L, T, nparts, wav_stats, wav, mc, st);
}

// THE walk of the Improved / GroupComm forward, from the encoder through the last block: srf_forward, srf_separate (wav_stats),
// srf_forward_ragged (rg), srf_separate_ragged (both) -- forward_walk, srf_api.hip -- and srf_forward_train.  It leaves the
// separation module's output at a.x_in(U).  The callers clear the statistics and pack their weight images before it, run their
// tail after it, and pass what else they differ in:
//   a           where each tensor lives, and which raw levels the fused pyramid writes on the side (srf_internal.h);
//   conv        conv(rows per example, x, w, parameter index of w, bias, y, rows, Cin, Cout, in_norm, residual, out_sums): a 1x1
//               convolution over the caller's image of w;
//   pair        pair(x, parameter index of w1, bias1, y, in_norm, residual, parameter index of w2, bias2, y2, out_sums2, Cin1, Cmid,
//               Cout2): a 256-channel 1x1 conv and the proj_1x1 that consumes its output as ONE launch (srf_pwconv_x3f.hip),
//               over the caller's images;
//   pair_head   bottleneck + proj_1x1 of block 0 run as a pair;  pair_block: res_conv of block i + proj_1x1 of block i + 1 do
//               (improved_sudormrf.py:292 -> :205, :220 -> :205; never GroupComm);
//   fused       the pyramid runs as the fused kernels (else: level by level + merge).
// The ragged forward keeps the layout -- [batch, C, L] with L the PLAN's frame count as row stride, the same workspace carve-up
// and two-buffer scheme -- and every kernel takes the example's own frame count L_b from a by-value table.  The invariant:
//   * a tensor whose GlobLN statistics are taken (enc, y1, merged; GroupComm: q) is exactly zero at columns >= L_b, so the
//     sums come out right and only the count changes (C * L_b);
//   * a tensor read with a halo (the wave by the encoder, y1 by the pyramid) is never read past the example's end;
//   * the block stream (x / u: pointwise consumers only) may hold anything there -- so may the partial decoder frames the
//     unchanged mask + decoder GEMM leaves at those columns: the ragged overlap-add never reads them.
template <typename Conv, typename Pair>
static inline int improved_walk(const srf_plan* p, const float* const* P, const float* wav, const SrfImpAddrs& a, Conv conv, Pair pair,
                                bool pair_head, bool pair_block, bool fused, const Ragged* rg, const float* wav_stats, void* stream) {
  const srf_config& c = p->cfg;
  const bool gc = c.variant == SRF_VARIANT_GROUPCOMM;
  const int G = gc ? c.group_size : 1;
  const int D = c.upsampling_depth, U = c.num_blocks, N = c.enc_num_basis, K = c.enc_kernel_size;
  const int Bt = p->Bt, L = p->L, Bg = p->Bg, nB = p->nB, nC = p->nC;
  int rc;

  // ---- front end: encoder (+ ln statistics; the slot of ln is the first), ln folded into the bottleneck GEMM's operand load
  const SrfFront<const float> f = plan_front(P);
  rc = imp_encoder(rg, wav, f.enc_w, a.enc, a.stats, Bt, p->A, p->T, N, K, L, wav_stats, stream);
  if (rc) return rc;
  bool y1_ready = false;      // proj_1x1 of the coming block has already been computed (with its statistics) by a pair launch
  {
    const srf_norm ln{a.stats, f.ln_g, f.ln_b, nullptr};
    if (pair_head) {
      const SrfBlock<const float> b0 = plan_block(p, P, 0);
      rc = pair(a.enc, SRF_P_BOTTLENECK, f.bott_b, a.x_in(0), &ln, nullptr, b0.i_proj, b0.proj_b, a.y1(0), plan_slots(p, a.stats, 0).proj,
                N, nB, nC);
      y1_ready = true;
    } else {
      rc = conv(1, a.enc, f.bott_w, SRF_P_BOTTLENECK, f.bott_b, a.x_in(0), Bt, N, c.out_channels, &ln, nullptr, nullptr);
    }
    if (rc) return rc;
  }

  // ---- separation module (GroupComm: every kernel of a block over the Bt * G folded rows, finding its example as row / G)
  for (int i = 0; i < U; ++i) {
    const SrfBlock<const float> b = plan_block(p, P, i);
    const SrfSlots s = plan_slots(p, a.stats, i);
    const float* xin = a.x_in(i);
    float *y1 = a.y1(i), *merged = a.merged(i);
    bool tac_norm_fused = false;
    if (gc) {
      // TAC (groupcomm_sudormrf_v2.py:356-384): q = TAC MLPs, u = x + GlobLN_(b,g)(q)
      float *q = a.q(i), *u = a.u(i);
      rc = imp_tac(rg, xin, q, b.tac, Bt, G, nB, 3 * nB, L, s.tac, stream);
      if (rc) return rc;
      const srf_norm tn{s.tac, b.tac_g, b.tac_b, nullptr};
      // u = x + GlobLN(q): folded into the proj conv's operand load where the thin-shape kernel runs it (it writes u for
      // the block's residual -- and the backward -- as it goes; bitwise the separate kernels' results); else its own kernel
      const void* al[4] = {xin, q, u, y1};
      tac_norm_fused = rg || srf_pw_conv_preadd_supported(nB, nC, L, al, 4);
      if (tac_norm_fused) {
        rc = imp_preadd(rg, G, xin, q, &tn, u, b.proj_w, b.proj_b, y1, Bg, nB, nC, L, s.proj, stream);
      } else {
        rc = srf_gln_apply_add(xin, q, u, &tn, Bg, nB, L, stream);
      }
      if (rc) return rc;
      xin = u;
    }
    // proj_1x1 conv (+ statistics for its GlobLN)            improved_sudormrf.py:205
    if (!tac_norm_fused && !y1_ready) {
      rc = conv(G, xin, b.proj_w, b.i_proj, b.proj_b, y1, Bg, nB, nC, nullptr, nullptr, s.proj);
      if (rc) return rc;
    }
    y1_ready = false;
    // depthwise pyramid + upsample/add (:206-216): the two fused passes -- with the raw levels d_k and their statistics written
    // on the side where the caller keeps them -- or D depthwise kernels + the merge kernel
    float* lv[SRF_MAX_DEPTH];
    for (int k = 0; k < D; ++k) lv[k] = a.lv(i, k);
    const srf_norm in{s.proj, b.proj_g, b.proj_be, b.proj_prelu};
    if (fused) {
      rc = imp_pyramid(rg, G, y1, merged, &in, b, Bg, nC, L, D, a.pyr, s.merged, a.lv_mask ? lv : nullptr, a.lv_mask ? s.level : nullptr,
                       stream);
    } else {
      rc = srf_pyramid_per_level(y1, &in, lv, merged, b.lv_w, b.lv_b, b.lv_g, b.lv_be, s.level, s.merged, Bg, nC, L, D, stream);
    }
    if (rc) return rc;
    // final_norm + PReLU folded into res_conv, + residual     :218-220
    const srf_norm fn{s.merged, b.fin_g, b.fin_be, b.fin_prelu};
    if (pair_block && i + 1 < U) {
      // res_conv of this block + proj_1x1 of the next one (into the next block's y1, its statistics into that block's first slot)
      const SrfBlock<const float> nb = plan_block(p, P, i + 1);
      rc = pair(merged, b.i_res, b.res_b, a.x_out(i), &fn, xin, nb.i_proj, nb.proj_b, a.y1(i + 1), plan_slots(p, a.stats, i + 1).proj, nC,
                nB, nC);
      y1_ready = true;
    } else {
      rc = conv(G, merged, b.res_w, b.i_res, b.res_b, a.x_out(i), Bg, nC, nB, &fn, xin, nullptr);
    }
    if (rc) return rc;
  }
  return SRF_OK;
}
