// Softmax attention (srf_attention.hip, srf_attention_bwd.hip): the kernels' arguments, the readers of their trailing parameter
// pack, and the one host path of the forward, which the attentive walks (srf_attentive.hip, srf_attentive_v3.hip) call too.
#pragma once
#include "srf_internal.h"

typedef float srf_f32x16 __attribute__((ext_vector_type(16)));
#define SRF_MHA_GEN_T 16   // generic (VALU) kernels, channels per lane: d <= 64 * 16

struct MhaArgs {
  const float *q, *k, *v;
  float* o;
  long qs, ks, vs, os;   // example strides (floats)
  int H, d, Lq, Lk;
  float scale;
};

struct MhaBwdArgs {
  const float *q, *k, *v, *go, *lse, *delta;   // lse, delta: [Bt, H, Lq] contiguous
  float *gq, *gk, *gv;
  long qs, ks, vs, gos, gqs, gks, gvs;          // example strides (floats)
  int H, d, Lq, Lk;
  float scale;
};

// The attention kernels' trailing parameter pack: [float* lse] [SrfFrames q_len, SrfFrames k_len].  Without the tables the row
// stride is the edge (the uniform instantiations: their arguments and code stay what they were); with them example b's own
// counts are, read once from the launch arguments into scalar registers.  Without lse nothing is stored (never evaluated).
template <int I, typename T, typename... X>
__device__ __forceinline__ const auto& srf_mha_pack_at(const T& t, const X&... x) {
  if constexpr (I == 0) return t;
  else return srf_mha_pack_at<I - 1>(x...);
}
template <typename... X>
__device__ __forceinline__ int srf_mha_qlen(int b, int L, const X&... x) {
  if constexpr (sizeof...(X) >= 2) return srf_mha_pack_at<sizeof...(X) - 2>(x...).n[b];
  else return L;
}
template <typename... X>
__device__ __forceinline__ int srf_mha_klen(int b, int L, const X&... x) {
  if constexpr (sizeof...(X) >= 2) return srf_mha_pack_at<sizeof...(X) - 1>(x...).n[b];
  else return L;
}
template <typename... X>
__device__ __forceinline__ void srf_mha_store_lse(size_t at, float v, const X&... x) {
  if constexpr (sizeof...(X) & 1) srf_mha_pack_at<0>(x...)[at] = v;
}

// ---- srf_attention.hip
// The one host path of the forward, behind the four public entries: q, k, v, o with an example stride per operand (the walks
// pass thirds or halves of one projection), lse [Bt, H, Lq] contiguous.  form picks the instantiation and the profiler names;
// SRF_MHA_RAGGED with both tables NULL still runs the ragged kernels (NULL = every example full on that side).
enum { SRF_MHA_LSE = 1, SRF_MHA_RAGGED = 2 };
int srf_mha_forward(int form, const MhaArgs& a, int Bt, float* lse, const int* q_lengths, const int* k_lengths, hipStream_t st);
// the two tables of a ragged call (one per side), checked against the row strides; fn names the caller in the error string
int srf_mha_ragged_tables(const char* fn, int Bt, int Lq, int Lk, const int* q_lengths, const int* k_lengths, SrfFrames* qf,
                          SrfFrames* kf);
