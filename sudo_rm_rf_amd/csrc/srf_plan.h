// The plan object behind the opaque srf_plan* of include/sudormrf_hip.h (shared by srf_api.hip and srf_train.hip).
#pragma once
#include <vector>
#include "srf_internal.h"

struct srf_plan {
  srf_config cfg;
  int Bt, T, Tp, L, A, SA;
  int Bg, nB, nC;  // folded batch (Bt*G), channels outside / inside the U-block per group
  int n_params, n_launches;
  // parameter indices
  int p_block0, p_block_stride, p_ublock_off, p_tail;
  // workspace offsets (bytes)
  size_t off_stats, stats_bytes, off_enc, off_xa, off_xb, off_xq, off_xu, off_y1, off_lv[SRF_MAX_DEPTH],
      off_masked, off_dec, off_pyr, off_wdpack, total_bytes;
  int fused_pyramid;
  int slots_per_block, n_slots;
  // pre-packed (split-bf16) weights of the 1x1 convolutions: param index -> workspace offset (0 = none)
  std::vector<int> pk_param, pk_cout, pk_cin;
  std::vector<size_t> pk_off;
  std::vector<size_t> pk_of_param;  // [n_params] offset or 0
  // causal variant (SRF_VARIANT_CAUSAL): UConvBlock's plain attributes alpha / beta per block (srf_plan_set_block_scales)
  // and the workspace copies of the weights they and skipinit_gain are folded into
  std::vector<float> alpha, beta;
  size_t off_fold_res, off_fold_proj, off_merged;
  // attentive variant (SRF_VARIANT_ATTENTIVE): the transformer layer's heads, head dimension and positions (L >> (D - 1)), its
  // activations x | qkv | o | y | f and the concatenated [3 H d, C] Q/K/V weights + biases of every block
  int att_heads = 0, att_dims = 0, att_len = 0;
  size_t off_att_x = 0, off_att_qkv = 0, off_att_o = 0, off_att_y = 0, off_att_f = 0, off_att_wqkv = 0;
};
// attentive blocks: the Improved block's tensors, then these (state_dict order of TransformerLayer)
enum { SRF_PA_Q = 0, SRF_PA_K = 2, SRF_PA_V = 4, SRF_PA_O = 6, SRF_PA_OUT_NORM = 8, SRF_PA_MHA_NORM = 10, SRF_PA_FFN = 12,
       SRF_PA_FFN_NORM = 14, SRF_PA_FFN_PRELU = 16, SRF_PA_PE = 17, SRF_PA_COUNT = 18 };

// ---- named views of the parameter table and of the GlobLN statistic slots (Improved / GroupComm layout; the causal variant
// has its own).  state_dict order:
//   front   encoder.weight | ln.{gamma, beta} | bottleneck.{weight, bias}
//   block   [GroupComm: the 11 TAC tensors, the last two TAC_norm.{gamma, beta}] | proj_1x1.conv.{weight, bias},
//           proj_1x1.norm.{gamma, beta}, proj_1x1.act.weight | D x {conv.weight, conv.bias, norm.gamma, norm.beta} |
//           final_norm.{gamma, beta}, final_act.weight | res_conv.{weight, bias}
//   tail    mask_net.0.weight (PReLU) | mask_net.1.{weight, bias} | decoder.weight
// slots     ln | per block: [GroupComm: TAC_norm] proj_1x1.norm, level 0 .. D-1, final_norm (the merged tensor)
// This is the ONE place that spells the layout out.  T = const float: the parameters; T = float: the backward's gradients.
enum { SRF_P_BOTTLENECK = 3, SRF_P_FRONT = 5, SRF_P_TAC = 11, SRF_P_TAIL = 4 };
// inside a U-ConvBlock's run of tensors: conv.weight of level k (k = D: final_norm.gamma)
static inline int plan_u_level(int k) { return 5 + 4 * k; }
static inline int plan_block_params(int D, bool gc) { return (gc ? SRF_P_TAC : 0) + plan_u_level(D) + 5; }
static inline int plan_p_proj(const srf_plan* p, int i) { return p->p_block0 + i * p->p_block_stride + p->p_ublock_off; }
static inline int plan_p_res(const srf_plan* p, int i) { return plan_p_proj(p, i) + plan_u_level(p->cfg.upsampling_depth) + 3; }
static inline int plan_p_mask(const srf_plan* p) { return p->p_tail + 1; }

template <typename T>
struct SrfFront {
  T *enc_w, *ln_g, *ln_b, *bott_w, *bott_b;
};
template <typename T>
struct SrfBlock {
  T* const* tac;   // GroupComm: the TAC sub-table as srf_tac / srf_tac_bwd take it (else null) and its norm
  T *tac_g, *tac_b;
  T *proj_w, *proj_b, *proj_g, *proj_be, *proj_prelu;
  T *lv_w[SRF_MAX_DEPTH], *lv_b[SRF_MAX_DEPTH], *lv_g[SRF_MAX_DEPTH], *lv_be[SRF_MAX_DEPTH];   // (as srf_pyramid* take them)
  T *fin_g, *fin_be, *fin_prelu;
  T *res_w, *res_b;
  int i_proj, i_res;   // parameter indices of the two packable weights (pk_of_param)
};
template <typename T>
struct SrfTail {
  T *mask_prelu, *mask_w, *mask_b, *dec_w;
};
struct SrfSlots {
  double *tac, *proj, *level[SRF_MAX_DEPTH], *merged;
};

template <typename T>
static inline SrfFront<T> plan_front(T* const* t) {
  return SrfFront<T>{t[0], t[1], t[2], t[SRF_P_BOTTLENECK], t[SRF_P_BOTTLENECK + 1]};
}
template <typename T>
static inline SrfBlock<T> plan_block(const srf_plan* p, T* const* t, int i) {
  const int D = p->cfg.upsampling_depth;
  SrfBlock<T> b{};
  b.i_proj = plan_p_proj(p, i);
  b.i_res = plan_p_res(p, i);
  if (p->p_ublock_off) {
    b.tac = t + b.i_proj - SRF_P_TAC;
    b.tac_g = b.tac[SRF_P_TAC - 2];
    b.tac_b = b.tac[SRF_P_TAC - 1];
  }
  T* const* u = t + b.i_proj;
  b.proj_w = u[0], b.proj_b = u[1], b.proj_g = u[2], b.proj_be = u[3], b.proj_prelu = u[4];
  for (int k = 0; k < D; ++k) {
    T* const* l = u + plan_u_level(k);
    b.lv_w[k] = l[0], b.lv_b[k] = l[1], b.lv_g[k] = l[2], b.lv_be[k] = l[3];
  }
  T* const* f = u + plan_u_level(D);
  b.fin_g = f[0], b.fin_be = f[1], b.fin_prelu = f[2], b.res_w = f[3], b.res_b = f[4];
  return b;
}
template <typename T>
static inline SrfTail<T> plan_tail(const srf_plan* p, T* const* t) {
  return SrfTail<T>{t[p->p_tail], t[plan_p_mask(p)], t[p->p_tail + 2], t[p->p_tail + 3]};
}
// stats: the zero-filled statistics region (one entry per FOLDED row and slot); the slot of ln is the first: `stats` itself
static inline SrfSlots plan_slots(const srf_plan* p, double* stats, int i) {
  const size_t each = (size_t)p->Bg * SRF_STAT_BUCKETS * 2;
  const bool gc = p->p_ublock_off != 0;
  double* s = stats + (1 + (size_t)i * p->slots_per_block) * each;
  SrfSlots v{};
  if (gc) v.tac = s, s += each;
  v.proj = s;
  for (int k = 0; k < p->cfg.upsampling_depth; ++k) v.level[k] = s + (1 + k) * each;
  v.merged = s + (1 + p->cfg.upsampling_depth) * each;
  return v;
}

// ---- dispatch decisions of a forward.  They depend on the kernel mode and the debug flags at CALL time, so they are
// functions of the plan, not fields of it.

// split + lay out every 1x1 weight for the 256 x 128 split-precision GEMMs at the start of the forward (kernel mode 0 only;
// SRF_DBG_NO_PACKED_WEIGHTS = without: the 128 x 128 kernels that split W on the fly)
static inline bool plan_use_pack(const srf_plan* p) {
  return srf_kernel_mode() == 0 && !srf_dbg(SRF_DBG_NO_PACKED_WEIGHTS) && !p->pk_param.empty();
}
// the blocks' depthwise pyramids run as the fused kernels (else: per-level kernels + merge)
static inline bool plan_fused_pyramid_now(const srf_plan* p) {
  return p->fused_pyramid && srf_kernel_mode() != 1 && !srf_dbg(SRF_DBG_PYR_PER_LEVEL);
}
// K5: mask GEMM and decoder contraction in ONE launch, the masked tensor never reaches memory.  Only where the 256 x 128 GEMM
// would have run the mask conv anyway (off_wdpack != 0 implies that the mask conv's weight has a packed image).
static inline bool plan_fused_tail_now(const srf_plan* p, bool use_pack) {
  const srf_config& c = p->cfg;
  return p->off_wdpack && use_pack && c.enc_num_basis % 8 == 0 &&
         srf_mask_decode_supported(p->Bt, c.out_channels, p->SA * c.enc_num_basis, p->L, p->SA * c.enc_kernel_size);
}
