// The plan object behind the opaque srf_plan* of include/sudormrf_hip.h (shared by srf_api.hip and srf_train.hip).
#pragma once
#include <algorithm>
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
  // attentive v3 (SRF_VARIANT_ATTENTIVE_V3): positions of every pyramid level (ceil halving) and, next to the fields above
  // (x: the answering level + its table, qkv: its [K; V] projection, wqkv: the concatenated [2 H d, C] K/V weights + biases
  // of every resampler), the asking side's Q projection and normalised copy
  int att_lv[SRF_MAX_DEPTH] = {};
  size_t off_att_q = 0, off_att_qn = 0;
  // original variant (SRF_VARIANT_ORIGINAL): the materialised activation a / e [C], conv_1x1_exp's output g and g + x with its
  // norm applied [B], reshape_before_masks' output [N], the mask logits z [S N], the Toeplitz mask weight + its row bias and the
  // block-diagonal decoder weight
  size_t off_orig_act = 0, off_orig_g = 0, off_orig_gx = 0, off_orig_xr = 0, off_orig_z = 0, off_orig_tz = 0, off_orig_wdec = 0;
};
// attentive blocks: the Improved block's tensors, then these (state_dict order of TransformerLayer)
enum { SRF_PA_Q = 0, SRF_PA_K = 2, SRF_PA_V = 4, SRF_PA_O = 6, SRF_PA_OUT_NORM = 8, SRF_PA_MHA_NORM = 10, SRF_PA_FFN = 12,
       SRF_PA_FFN_NORM = 14, SRF_PA_FFN_PRELU = 16, SRF_PA_PE = 17, SRF_PA_COUNT = 18 };

// attentive v3 blocks: the Improved block's tensors (final_norm.norm.{gamma, beta}, final_norm.act.weight where the Improved
// model has final_norm.{gamma, beta}, final_act.weight: the same places), then D - 1 groups of the SRF_PA_* tensors above,
// attentive_resamplers.0 .. D-2 (ConditionalTransformerLayer has TransformerLayer's state_dict).  Resampler r asks from level
// D - 2 - r and is answered by the result of resampler r - 1 (r = 0: by level D - 1).
// slots     ln | per block: proj_1x1.norm, level 0 .. D-1, final_norm (its input: the last out_norm's OUTPUT; D = 1: level 0's
//           norm's), then per resampler out_mha_norm, ffn.norm, out_norm
static inline int plan_v3_block_params(int D) { return 5 + 4 * D + 5 + (D - 1) * SRF_PA_COUNT; }
static inline int plan_v3_slots_per_block(int D) { return D + 2 + 3 * (D - 1); }

// ---- named views of the parameter table and of the GlobLN statistic slots (Improved / GroupComm layout, which the attentive
// variant extends; the causal variant's views follow below).  state_dict order:
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

// ---- causal variant (CausalSuDORMRF, causal_improved_sudormrf_v3.py).  state_dict order:
//   front   encoder.weight | bottleneck.{weight, bias}
//   block   skipinit_gain | proj_1x1.conv.{weight, bias}, proj_1x1.act.weight | D x spp_dw.k.{conv.weight, conv.bias, act.weight} |
//           res_conv.{weight, bias}
//   tail    mask_net.0.weight (PReLU) | mask_net.1.{weight, bias} | decoder.weight | mask_nl_class.weight (PReLU)
// The ONE place that spells this layout out, for the plan and for the streaming session (srf_stream is no srf_plan: both go through
// SrfCausalLayout).  The views take any table t with t[parameter index] -> T*.  T = const float: the parameters (an array of
// pointers, or SrfOffsetTable over the session's prepared weights); T = float: the backward's gradients; T = long: element counts.
enum { SRF_PC_BOTTLENECK = 1, SRF_PC_FRONT = 3, SRF_PC_PROJ = 1, SRF_PC_TAIL = 5 };
// inside a block's run of tensors: conv.weight of level k (k = D: res_conv.weight)
static inline int causal_u_level(int k) { return 4 + 3 * k; }
struct SrfCausalLayout { int block0, stride, tail, n_params, D; };
static inline SrfCausalLayout causal_layout(int U, int D) {
  SrfCausalLayout y{SRF_PC_FRONT, causal_u_level(D) + 2, 0, 0, D};
  y.tail = y.block0 + U * y.stride;
  y.n_params = y.tail + SRF_PC_TAIL;
  return y;
}
static inline SrfCausalLayout causal_layout(const srf_plan* p) { return causal_layout(p->cfg.num_blocks, p->cfg.upsampling_depth); }
static inline int causal_p_proj(const SrfCausalLayout& y, int i) { return y.block0 + i * y.stride + SRF_PC_PROJ; }
static inline int causal_p_res(const SrfCausalLayout& y, int i) { return y.block0 + i * y.stride + causal_u_level(y.D); }
static inline int causal_p_mask(const SrfCausalLayout& y) { return y.tail + 1; }
static inline int causal_p_dec(const SrfCausalLayout& y) { return y.tail + 3; }

template <typename T> struct SrfOffsetTable {   // entry p at base + off[p]
  T* base; const size_t* off;
  T* operator[](int p) const { return base + off[p]; }
};
template <typename T> struct SrfCausalFront { T *enc_w, *bott_w, *bott_b; };
template <typename T> struct SrfCausalTail { T *mask_prelu, *mask_w, *mask_b, *dec_w, *out_prelu; };
template <typename T> struct SrfCausalBlock {
  T *gain, *proj_w, *proj_b, *proj_prelu;
  T *lv_w[SRF_MAX_DEPTH], *lv_b[SRF_MAX_DEPTH], *lv_prelu[SRF_MAX_DEPTH];   // (as srf_causal_pyramid* take them)
  T *res_w, *res_b;
  int i_proj, i_res;   // parameter indices of the two packable weights (pk_of_param)
};
template <typename T, typename Tab> static inline SrfCausalFront<T> causal_front(const Tab& t) {
  return SrfCausalFront<T>{t[0], t[SRF_PC_BOTTLENECK], t[SRF_PC_BOTTLENECK + 1]};
}
template <typename T, typename Tab> static inline SrfCausalBlock<T> causal_block(const SrfCausalLayout& y, const Tab& t, int i) {
  SrfCausalBlock<T> b{};
  b.i_proj = causal_p_proj(y, i);
  b.i_res = causal_p_res(y, i);
  b.gain = t[b.i_proj - SRF_PC_PROJ];
  b.proj_w = t[b.i_proj], b.proj_b = t[b.i_proj + 1], b.proj_prelu = t[b.i_proj + 2];
  for (int k = 0; k < y.D; ++k) {
    const int l = b.i_proj - SRF_PC_PROJ + causal_u_level(k);
    b.lv_w[k] = t[l], b.lv_b[k] = t[l + 1], b.lv_prelu[k] = t[l + 2];
  }
  b.res_w = t[b.i_res], b.res_b = t[b.i_res + 1];
  return b;
}
template <typename T, typename Tab> static inline SrfCausalTail<T> causal_tail(const SrfCausalLayout& y, const Tab& t) {
  return SrfCausalTail<T>{t[y.tail], t[causal_p_mask(y)], t[y.tail + 2], t[causal_p_dec(y)], t[y.tail + 4]};
}
// one block's share of a fold region: res_conv weight * (skipinit_gain * alpha) [B][C] | its bias [B]   (each 64-float aligned)
static inline size_t causal_fold_res_floats(int B, int C) { return srf_align_up((size_t)B * C, 64) + srf_align_up((size_t)B, 64); }
// The weights a causal forward runs on, per block: res_conv weight and bias * (skipinit_gain * alpha) in fold_res (U x
// causal_fold_res_floats) and, where beta != 1, proj_1x1 weight / beta in fold_proj (U x [C][B]); else the parameter itself.
// One srf_causal_scale_many launch (srf_api.hip).
struct SrfCausalFolded { std::vector<const float*> wproj, wres, bres; };
int srf_causal_fold(const srf_plan* p, const float* const* P, float* fold_res, float* fold_proj, SrfCausalFolded* out, hipStream_t st);

// ---- original variant (SuDORMRF, sudormrf.py).  state_dict order:
//   front   encoder.0.{weight, bias} | ln.{weight, bias} | l1.{weight, bias}
//   block   proj_1x1.{conv.weight, conv.bias, norm.weight, norm.bias, act.weight [C]} | D x spp_dw.k.{conv.weight, conv.bias,
//           norm.weight, norm.bias} | conv_1x1_exp.{conv.weight, conv.bias, norm.weight, norm.bias} |
//           final_norm.{norm.weight, norm.bias, act.weight [C]} | module_act.{norm.weight, norm.bias, act.weight [B]}
//   tail    [B != N: reshape_before_masks.{weight, bias}] | m.{weight, bias} | decoder.{weight, bias} | ln_mask_in.{weight, bias}
// slots     ln | per block: proj_1x1.norm, level 0 .. D-1, final_norm (the merged tensor), conv_1x1_exp.norm, module_act.norm
// The ONE place that spells this layout out.
enum { SRF_PO_L1 = 4, SRF_PO_FRONT = 6, SRF_PO_TAIL = 6 };
static inline int orig_block_params(int D) { return 5 + 4 * D + 4 + 3 + 3; }
static inline int orig_slots_per_block(int D) { return D + 4; }
static inline int orig_p_proj(const srf_plan* p, int i) { return p->p_block0 + i * p->p_block_stride; }
static inline int orig_p_exp(const srf_plan* p, int i) { return orig_p_proj(p, i) + 5 + 4 * p->cfg.upsampling_depth; }
static inline bool orig_has_reshape(const srf_plan* p) { return p->cfg.out_channels != p->cfg.enc_num_basis; }
static inline int orig_p_reshape(const srf_plan* p) { return p->p_tail; }                       // (only where orig_has_reshape)
static inline int orig_p_mask(const srf_plan* p) { return p->p_tail + (orig_has_reshape(p) ? 2 : 0); }
// T = const float: the parameters; T = float: the training backward's gradients (same indices)
template <typename T> struct SrfOrigFrontT { T *enc_w, *enc_b, *ln_g, *ln_b, *l1_w, *l1_b; };
template <typename T> struct SrfOrigBlockT {
  T *proj_w, *proj_b, *proj_g, *proj_be, *proj_slope;
  T *lv_w[SRF_MAX_DEPTH], *lv_b[SRF_MAX_DEPTH], *lv_g[SRF_MAX_DEPTH], *lv_be[SRF_MAX_DEPTH];
  T *exp_w, *exp_b, *exp_g, *exp_be;
  T *fin_g, *fin_be, *fin_slope;
  T *act_g, *act_be, *act_slope;
  int i_proj, i_exp;   // parameter indices of the two packable weights (pk_of_param)
};
template <typename T> struct SrfOrigTailT { T *rs_w, *rs_b, *m_w, *m_b, *dec_w, *dec_b; int i_rs, i_m; };
using SrfOrigFront = SrfOrigFrontT<const float>;
using SrfOrigBlock = SrfOrigBlockT<const float>;
using SrfOrigTail = SrfOrigTailT<const float>;
struct SrfOrigSlots { double *proj, *level[SRF_MAX_DEPTH], *merged, *exp, *act; };
template <typename T> static inline SrfOrigFrontT<T> orig_front(T* const* t) {
  return SrfOrigFrontT<T>{t[0], t[1], t[2], t[3], t[SRF_PO_L1], t[SRF_PO_L1 + 1]};
}
template <typename T> static inline SrfOrigBlockT<T> orig_block(const srf_plan* p, T* const* t, int i) {
  const int D = p->cfg.upsampling_depth;
  SrfOrigBlockT<T> b{};
  b.i_proj = orig_p_proj(p, i);
  b.i_exp = orig_p_exp(p, i);
  T* const* u = t + b.i_proj;
  b.proj_w = u[0], b.proj_b = u[1], b.proj_g = u[2], b.proj_be = u[3], b.proj_slope = u[4];
  for (int k = 0; k < D; ++k) {
    T* const* l = u + 5 + 4 * k;
    b.lv_w[k] = l[0], b.lv_b[k] = l[1], b.lv_g[k] = l[2], b.lv_be[k] = l[3];
  }
  T* const* e = t + b.i_exp;
  b.exp_w = e[0], b.exp_b = e[1], b.exp_g = e[2], b.exp_be = e[3];
  b.fin_g = e[4], b.fin_be = e[5], b.fin_slope = e[6];
  b.act_g = e[7], b.act_be = e[8], b.act_slope = e[9];
  return b;
}
template <typename T> static inline SrfOrigTailT<T> orig_tail(const srf_plan* p, T* const* t) {
  SrfOrigTailT<T> v{};
  v.i_rs = orig_p_reshape(p);
  v.i_m = orig_p_mask(p);
  if (orig_has_reshape(p)) v.rs_w = t[v.i_rs], v.rs_b = t[v.i_rs + 1];
  v.m_w = t[v.i_m], v.m_b = t[v.i_m + 1], v.dec_w = t[v.i_m + 2], v.dec_b = t[v.i_m + 3];
  return v;
}
// the Toeplitz weight's region: tz [S N, N] | bias rows [S N]   (each section 64-float aligned; the same layout holds the two
// gradients in the backward).  orig_tz_bias_at: floats in front of the bias rows; orig_tz_floats: floats of the region
static inline size_t orig_tz_bias_at(int S, int N) { return srf_align_up((size_t)S * N * N, 64); }
static inline size_t orig_tz_floats(int S, int N) { return orig_tz_bias_at(S, N) + srf_align_up((size_t)S * N, 64); }
// pad_to_appropriate_length: T up to a multiple of lcm(hop, 2^D), only when it is not one already (the plan's Tp, and every
// example's own padded length in a ragged batch)
static inline long orig_gcd(long a, long b) { return b ? orig_gcd(b, a % b) : a; }
static inline long orig_padded_length(long T, int h, int D) {
  const long lcm = (long)h * (1L << D) / orig_gcd(h, 1L << D);
  return T % lcm ? T + lcm - T % lcm : T;
}
static inline SrfOrigSlots orig_slots(const srf_plan* p, double* stats, int i) {
  const size_t each = (size_t)p->Bg * SRF_STAT_BUCKETS * 2;
  const int D = p->cfg.upsampling_depth;
  double* s = stats + (1 + (size_t)i * p->slots_per_block) * each;
  SrfOrigSlots v{};
  v.proj = s;
  for (int k = 0; k < D; ++k) v.level[k] = s + (1 + k) * each;
  v.merged = s + (1 + D) * each, v.exp = s + (2 + D) * each, v.act = s + (3 + D) * each;
  return v;
}

// ---- the packed (split-bf16) weight images of a plan
// parameter index -> (block, index inside the block's run of tensors); block = -1 outside the blocks
struct SrfBlockParam { int block, rel; };
static inline SrfBlockParam plan_block_param(int block0, int stride, int tail, int param) {
  if (param < block0 || param >= tail) return SrfBlockParam{-1, 0};
  return SrfBlockParam{(param - block0) / stride, (param - block0) % stride};
}
// A packed image of parameter `param` ([cout, cin]) in the workspace, for the shapes the 256 x 128 GEMM supports
static inline void plan_add_pack(srf_plan* p, size_t* off, int param, int cout, int cin) {
  const size_t bytes = srf_packed_pw_weight_bytes(cout, cin);
  if (!bytes) return;
  const size_t o = *off;
  *off = srf_align_up(*off + bytes, 256);
  p->pk_param.push_back(param);
  p->pk_cout.push_back(cout);
  p->pk_cin.push_back(cin);
  p->pk_off.push_back(o);
  p->pk_of_param[param] = o;
}
static inline const void* plan_packed(const srf_plan* p, const char* ws, bool use_pack, int param) {
  return (use_pack && p->pk_of_param[param]) ? (const void*)(ws + p->pk_of_param[param]) : nullptr;
}
// split + lay out every packable 1x1 weight for the 256 x 128 split-precision GEMMs (srf_pwconv_x3w.hip / _x3p.hip), one launch
// per forward.  source(parameter index): the fp32 weight that goes into the image (the causal forward: its folded copies; the
// attentive one: its concatenated Q/K/V weights)
template <typename F>
static inline int plan_pack_weights(const srf_plan* p, F source, char* ws, void* stream) {
  std::vector<const float*> pw(p->pk_param.size());
  std::vector<void*> pd(p->pk_param.size());
  for (size_t i = 0; i < p->pk_param.size(); ++i) {
    pw[i] = source(p->pk_param[i]);
    pd[i] = ws + p->pk_off[i];
  }
  return srf_pack_pw_weights(pw.data(), pd.data(), p->pk_cout.data(), p->pk_cin.data(), (int)pw.size(), stream);
}

// weight images queued for ONE pack launch, carved from `at` in steps of 256 bytes (the training steps: their images live in
// `scratch`, which images there are depends on the kernel mode of the call)
struct SrfPackQueue {
  char* at;
  std::vector<const float*> w;
  std::vector<void*> d;
  std::vector<int> cout, cin;
  // bytes: the image's size, 0 = none wanted (returns null)
  const void* add(const float* weight, size_t bytes, int co, int ci) {
    if (!bytes) return nullptr;
    void* dst = at;
    at += srf_align_up(bytes, 256);
    w.push_back(weight), d.push_back(dst), cout.push_back(co), cin.push_back(ci);
    return dst;
  }
  // An image for a training forward: its exact-class 1x1 convolutions (kernel mode 2) run on the THREE-part split GEMM (six bf16
  // MFMAs per product block, 24-bit operands: srf_pwconv_x3w.hip NP 3) where the 256 x 128 kernel takes the launch, on weights
  // split and laid out once per step.  Debug flag 1 << 31: no image, the exact-fp32 MFMA kernel instead (A/B).
  const void* add3(const float* weight, int co, int ci) {
    const bool three = srf_kernel_mode() == 2 && !srf_dbg(SRF_DBG_TRAIN_FWD_EXACT_MFMA);
    return add(weight, three ? srf_packed3_pw_weight_bytes(co, ci) : 0, co, ci);
  }
  // the exact-class images of the training forward / the images of the TRANSPOSED weights of a backward's data-gradient GEMMs
  int pack3(void* stream) const {
    return w.empty() ? SRF_OK : srf_pack3_pw_weights(w.data(), d.data(), cout.data(), cin.data(), (int)w.size(), stream);
  }
  int packT(hipStream_t st) const {
    return w.empty() ? SRF_OK : srf_pack_pw_weights_transposed(w.data(), d.data(), cout.data(), cin.data(), (int)w.size(), st);
  }
};

// A training forward runs its 1x1 convolutions in the EXACT-fp32 CLASS (kernel mode 2: since round 3 the three-part split
// GEMM where the 256 x 128 kernel takes the launch, else the exact fp32 MFMA kernel) unless debug flag 1<<28 is set.
// The split-bf16 GEMMs are accurate to ~2^-17 of sum|terms| per output -- far inside the 1e-4 forward bar -- but
// the gradients of the first blocks' parameters are ill-conditioned with respect to exactly that rounding:
// injecting 2^-17 noise into the bottleneck GEMM's output alone moves d loss / d sm.0.proj_1x1.conv.weight by 5 %
// in an fp64 autograd experiment (2^-24 noise: 3e-6), and the HIP step reproduces both numbers against the
// reference's own gradients (tests/golden/train_*).  The backward GEMMs (data / weight gradients) stay split-bf16:
// with an exact forward every parameter gradient is within 2e-5 of the reference's.  (Ask before SrfKernelModeScope sets mode 2.)
static inline bool srf_train_fwd_exact() { return srf_kernel_mode() == 0 && !srf_dbg(SRF_DBG_TRAIN_FWD_SPLIT_BF16); }

// ---- what every training entry point refuses before its first launch (srf_train.hip), in this order: a null pointer (the
// plan, P, any of `others`: G, wav, out, grad_out), a wrong num_params, a null P[i], a null G[i] (G = NULL: a forward, no
// gradient table; the last null_grad_tail entries may be NULL: parameters the forward never reads), a `saved` or `scratch`
// smaller than needed, either of them off the 256-byte grid.  SRF_EINVAL with `who` in front of the reason.  The refusals of
// one family -- which plans it takes, its shape limits -- stay with the family.
struct SrfTrainBuffers {
  const void* saved;
  size_t saved_bytes, saved_need;
  const void* scratch;
  size_t scratch_bytes, scratch_need;
};
int srf_train_entry_check(const char* who, const srf_plan* p, const float* const* P, float* const* G, int num_params,
                          int null_grad_tail, std::initializer_list<const void*> others, const SrfTrainBuffers& b);

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
