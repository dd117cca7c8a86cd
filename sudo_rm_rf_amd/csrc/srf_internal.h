// Library-internal entry points: every non-static function that one .hip defines and another calls is declared here, once
// (those that take PwArgs / PwPairArgs: srf_pw.h; PyrRegArgs: srf_pyr.h; MhaArgs: srf_mha.h).  The defining file includes this header too, so the
// compiler checks each definition against the declaration its callers see.  The public extern "C" functions come from
// include/sudormrf_hip.h (through srf_common.h) and are never re-declared.
#pragma once
#include "srf_common.h"

// ---- causal model: shared by the whole-sequence kernels (srf_causal.hip) and the streaming ones (srf_causal_stream.hip);
// "bit-identical under any chunking" rests on both reading the same taps
#define SRF_CAUSAL_TAPS 11   // live taps of the k = 21 depthwise convs (21 - 21 // 2)
#define SRF_CAUSAL_KW 21     // weight row stride of those convs

// ---- ragged forms (srf_*_ragged): the frame count of every example of the batch, handed to the kernels BY VALUE next to their
// uniform twins' arguments (no upload, no synchronisation; the table caps the batch at SRF_RAGGED_MAX_BATCH)
struct SrfFrames {
  int n[SRF_RAGGED_MAX_BATCH];
};
// A kernel template takes the table(s) as a trailing parameter PACK: empty in the uniform instantiations (their arguments and
// their code stay what they were), one SrfFrames (encoder: two -- samples, frames) in the ragged ones.
__device__ __forceinline__ int srf_frames_of(int) { return 0; }    // (uniform: never evaluated)
__device__ __forceinline__ int srf_frames2_of(int) { return 0; }
template <typename... R>
__device__ __forceinline__ int srf_frames_of(int g, const SrfFrames& f, const R&...) { return f.n[g]; }
__device__ __forceinline__ int srf_frames2_of(int g, const SrfFrames&, const SrfFrames& f2) { return f2.n[g]; }
// Kernels that run over FOLDED rows (GroupComm: batch x groups) take (SrfFrames, int rows_per_example): the table stays one
// entry per example and row r (wave-uniform) belongs to example r / rows_per_example (the Improved model passes 1)
__device__ __forceinline__ int srf_frames_of(int row, const SrfFrames& f, int rows_per_example) { return f.n[row / rows_per_example]; }
// checks frames[0 .. groups) against the row stride L and fills the table; `what` names the caller in the error string
int srf_frames_table(const char* what, const int* frames, int groups, int L, SrfFrames* out);

// ---- srf_elementwise.hip
int srf_transpose_launch(const float* w, float* wt, int Ci, int M, hipStream_t st);
// stats: null = plain overlap-add; else [Bt][2] {mean, std} of the raw mixture `wav` [Bt][T] (mc: also mixture consistency)
// lens / frames (both or neither): the ragged form -- frames of example b at or past frames[b] count as zero and are never
// read, samples at or past lens[b] are written as exact 0; with stats (srf_separate_ragged) the example's own samples are
// rescaled (mc: + mixture consistency) and wav is read on [0, lens[b]) only
int srf_overlap_add_launch(const float* z, float* out, int Bt, int Co, int K, int L, int T, int nparts, const float* stats,
                           const float* wav, int mc, hipStream_t st, const SrfFrames* lens = nullptr,
                           const SrfFrames* frames = nullptr);
// per-row {mean, unbiased std} over lens.n[r] samples of a padded [rows, T] tensor; `lens` already checked against T
int srf_wav_stats_ragged_launch(const float* wav, const SrfFrames& lens, float* stats, int rows, int T, hipStream_t st);

// ---- srf_api.hip: what the attentive models' walks (srf_attentive.hip, srf_attentive_v3.hip) share with forward_walk
int srf_zero_launch(void* p, size_t bytes, hipStream_t st);
// post_stats / post_wav / post_mc: the callers' rescale (+ mixture consistency) folded into the overlap-add (srf_separate)
int srf_decoder_impl(const float* v, const float* w, float* out, int Bt, int Ci, int Co, int K, int L, int T, float* scratch,
                     const float* post_stats, const float* post_wav, int post_mc, void* stream, const float* in_prelu = nullptr,
                     const SrfFrames* lens = nullptr, const SrfFrames* frames = nullptr);   // (both or neither: the ragged overlap-add)

struct srf_plan;
// what srf_forward / srf_separate, srf_forward_ragged and the original model's ragged entries (`who`, in front of every reason) ask
// of their arguments, in this order: ptrs (none of the caller's pointers is null), num_params, the workspace's size
// (SRF_EWORKSPACE) and its 256-byte alignment, no null P[i]
int forward_check_args(const char* who, bool ptrs, const srf_plan* p, const float* const* P, int num_params, const void* workspace,
                       size_t workspace_bytes);

// ---- srf_attentive.hip (softmax attention, which its walk and the next one call: srf_mha.h)
struct Ragged;
// rg: NULL = the uniform forward; else the ragged batch of srf_attentive_forward_ragged / srf_attentive_separate_ragged
int srf_attentive_forward(const srf_plan* p, const float* const* P, const float* wav, float* out, void* workspace,
                          const float* wav_stats, int mixture_consistency, void* stream, const Ragged* rg = nullptr);
// ---- srf_attentive_v3.hip
int srf_attentive_v3_forward(const srf_plan* p, const float* const* P, const float* wav, float* out, void* workspace,
                             const float* wav_stats, int mixture_consistency, void* stream);
// A ragged batch as the walks carry it (forward_walk in srf_api.hip, srf_original_forward): NULL = the uniform call
struct Ragged {
  const int* lengths;                 // samples per example (host, the caller's)
  int frames[SRF_RAGGED_MAX_BATCH];   // frames per example: its own padded length / hop, as its batch-1 plan would have it
  SrfFrames lens_t, frames_t;         // the same two by value, for the overlap-add
};
// ---- srf_original.hip
// Where the original model's ONE forward walk keeps its tensors.  Block i reads the block stream at x + i * x_stride and writes
// it one stride further; its own tensors lie at blk + i * blk_stride + the o_* byte offsets.  The inference forward overwrites one
// set block after block (both strides 0, m on y1: the plan's workspace); the training forward keeps every block's (`saved`, the
// rest in `scratch`: srf_original_train.hip).
struct SrfOrigAddrs {
  double* stats;
  float* enc;
  char *x, *blk;
  size_t x_stride, blk_stride;
  size_t o_y1, o_m, o_g, o_gx, o_lv[SRF_MAX_DEPTH];
  float *act, *xr, *z, *masked, *dec, *tz, *wdec;   // act: a, then e; xr: only with reshape_before_masks; dec: the decoder's scratch
  void* pyr;                                         // the fused pyramid's scratch (NULL where the pyramid never runs fused)
  float* x_in(int i) const { return (float*)(x + x_stride * i); }
  float* x_out(int i) const { return (float*)(x + x_stride * (i + 1)); }
  float* y1(int i) const { return (float*)(blk + blk_stride * i + o_y1); }
  float* m(int i) const { return (float*)(blk + blk_stride * i + o_m); }
  float* g(int i) const { return (float*)(blk + blk_stride * i + o_g); }
  float* gx(int i) const { return (float*)(blk + blk_stride * i + o_gx); }
  float* lv(int i, int k) const { return (float*)(blk + blk_stride * i + o_lv[k]); }
};
// Where the Improved / GroupComm model's ONE forward walk (srf_improved_walk.h) keeps its tensors.  Block i reads the block stream
// at x[i & 1] + i * x_stride and writes it at x[(i + 1) & 1] + (i + 1) * x_stride; its own tensors lie at blk + i * blk_stride + the
// o_* byte offsets.  The inference forward alternates two stream buffers and overwrites one set of block tensors (both strides 0,
// merged on y1 unless the pyramid runs fused: the plan's workspace); the training forward keeps every block's (x[0] = x[1], `saved`).
struct SrfImpAddrs {
  double* stats;
  float* enc;
  char *x[2], *blk;
  size_t x_stride, blk_stride;
  size_t o_y1, o_merged, o_q, o_u, o_lv[SRF_MAX_DEPTH];   // q, u: GroupComm only
  unsigned lv_mask;   // bit k: the raw level d_k has a place (none: the fused pyramid writes no levels; all, all but d_0: it does)
  void* pyr;          // the fused pyramid's scratch
  float* x_in(int i) const { return (float*)(x[i & 1] + x_stride * i); }
  float* x_out(int i) const { return x_in(i + 1); }
  float* y1(int i) const { return (float*)(blk + blk_stride * i + o_y1); }
  float* merged(int i) const { return (float*)(blk + blk_stride * i + o_merged); }
  float* q(int i) const { return (float*)(blk + blk_stride * i + o_q); }
  float* u(int i) const { return (float*)(blk + blk_stride * i + o_u); }
  float* lv(int i, int k) const { return (lv_mask >> k & 1) ? (float*)(blk + blk_stride * i + o_lv[k]) : nullptr; }
};
int srf_original_forward(const srf_plan* p, const float* const* P, const float* wav, float* out, void* workspace,
                         const float* wav_stats, int mixture_consistency, void* stream, const Ragged* rg = nullptr);
// srf_bias_rescale_ragged's launch alone, from a table the caller has checked (the walk: srf_original_walk.h)
int srf_bias_rescale_ragged_launch(float* out, const float* bias, const float* stats, const float* wav, int mc, int Bt, int S, int T,
                                   const SrfFrames& lens, void* stream);
// m.{weight, bias} as the [S N, N] GEMM weight + its bias rows (tz: orig_tz_floats of srf_plan.h, the rows at orig_tz_bias_at) and
// decoder.weight as the block-diagonal one (wdec): two launches, at the start of the walk and of srf_original_backward
int srf_original_weight_forms(const srf_plan* p, const float* const* P, float* tz, float* wdec, void* stream);
// the Improved walk's mask + decoder tail (srf_api.hip), shared with the attentive walks; rg: forward_walk's ragged batch, else NULL
int srf_improved_tail(const srf_plan* p, const float* const* P, const float* cur, float* out, void* workspace, bool use_pack,
                      const float* wav_stats, const float* wav, int mixture_consistency, const Ragged* rg, void* stream);

// ---- srf_encoder.hip
int srf_encoder_impl(const float* wav, const float* w, float* out, double* sums, int Bt, int A, int T, int N, int K, int L,
                     const float* in_stats, void* stream);
int srf_encoder_ragged_impl(const float* wav, const float* w, float* out, double* sums, int Bt, int A, int T, int N, int K, int L,
                            const int* lengths, const int* frames, const float* in_stats, void* stream);

// ---- srf_causal.hip: srf_forward folds every block's scales with as few launches as possible
int srf_causal_scale_many(const float* const* src, float* const* dst, const long* n, const float* const* dscale,
                          const float* hscale, int count, hipStream_t st);

// ---- srf_causal_bwd.hip: what the causal training step (srf_causal_train.hip) needs besides the public kernels
int srf_causal_merge_act(const float* const* d, const float* const* prelu, int D, float* y, int Bt, int C, int L, hipStream_t st);
int srf_causal_gain_fold(float* const* dw, float* const* db, const float* const* w, const float* const* b,
                         const float* const* gain, float* const* dgain, const float* alpha, int nw, int nb, int count,
                         hipStream_t st);
int srf_causal_enc_scatter(const float* src, float* dst, int N, int A, int K, hipStream_t st);
// gx = gout * (x > 0 ? 1 : slope) (may alias gout), dslope[0] = sum gout min(x, 0), WRITTEN, block partials added in block order;
// scratch: srf_causal_prelu_bwd_scratch_floats() floats
size_t srf_causal_prelu_bwd_scratch_floats();
int srf_causal_prelu_bwd(const float* gout, const float* x, const float* slope, float* gx, float* dslope, long n, float* scratch,
                         hipStream_t st);

// ---- srf_dwconv.hip: the per-level pyramid of the Improved and the original model's inference and training forwards
// (w, bias, gamma, beta: the level arrays of a block view of srf_plan.h; lv_sums, merged_sums: its statistic slots)
int srf_pyramid_per_level(const float* x, const srf_norm* in_norm, float* const* lv, float* merged, const float* const* w,
                          const float* const* bias, const float* const* gamma, const float* const* beta, double* const* lv_sums,
                          double* merged_sums, int Bg, int nC, int L, int D, void* stream);

// ---- srf_pyramid.hip / srf_pyramid_reg.hip
bool srf_pyramid_reg_supported(int L, int D);
// lv_out / lv_sums (both or neither; register-resident kernels only): the training forward's extra outputs
int srf_pyramid_impl(const float* y1, float* merged, const srf_norm* in_norm, const float* const* w,
                     const float* const* bias, const float* const* gamma, const float* const* beta, int groups, int C,
                     int L, int D, void* scratch, double* out_sums, float* const* lv_out, double* const* lv_sums,
                     void* stream);

// ---- srf_pwconv.hip
void srf_pw_prefer_paired(bool on);   // the paired-block form of the 256 x 128 GEMM for this thread's launches
struct SrfPairedScope {               // ... for the launches of one call, on every path out of it
  SrfPairedScope() { srf_pw_prefer_paired(true); }
  ~SrfPairedScope() { srf_pw_prefer_paired(false); }
};
bool srf_pw_conv_preadd_supported(int Cin, int Cout, int L, const void* const* ptrs, int nptrs);
int srf_pw_conv_preadd(const float* x, const float* q, const srf_norm* qnorm, float* u, const float* w, const float* bias,
                       float* y, int Bt, int Cin, int Cout, int L, double* out_sums, hipStream_t st);
// K5 (srf_forward's tail): mask GEMM + decoder contraction in one launch
bool srf_mask_decode_supported(int Bt, int Cin, int Cout, int L, int M);
size_t srf_mask_decode_pack_bytes(int Cout);
int srf_mask_decode_pack(const float* wd, void* dst, int Ci, int M, hipStream_t st);
// zpart[Bt][ceil(Cout / 256)][M][L] = per-256-channel partial sums of Wd^T (relu(W prelu(x) + bias) * mul)
int srf_mask_decode(const float* x, const float* w, const void* w_packed, const float* bias, const float* prelu,
                    const float* mul, int mul_channels, const void* wd_packed, float* zpart, int Bt, int Cin, int Cout, int L,
                    int M, hipStream_t st);
int srf_pack_pw_weights_transposed(const float* const* w, void* const* packed, const int* Cout, const int* Cin, int n,
                                   hipStream_t st);
bool srf_pw_packed_only(const void* w_packed, const float* x, int Bt, int Cin, int Cout, int L);
// srf_pack3_pw_weights / srf_pw_conv_packed3 of THIS thread take the three-bf16-part form (24 mantissa bits, what debug flag
// 16384 selects process-wide) while on; returns the previous setting
bool srf_train_three_parts_override(bool on);
struct SrfThreePartsScope {           // ... on until the scope ends, then the previous setting is back
  const bool prev;
  SrfThreePartsScope() : prev(srf_train_three_parts_override(true)) {}
  ~SrfThreePartsScope() { srf_train_three_parts_override(prev); }
};
// A backward's data-gradient GEMM gx = W^T g (+ skip), Cin -> Cout, W the FORWARD weight [Cin][Cout]: from the packed image
// of W^T where that serves the whole launch (srf_pw_packed_only), else from its fp32 transpose, made in `wt` first
int srf_pw_data_grad(const float* g, const float* w, const void* wT_packed, float* wt, const float* zero_bias, float* gx, int Bt,
                     int Cin, int Cout, int L, const float* skip, hipStream_t st);

// ---- srf_pwconv_x3w.hip (the 256 x 128 kernel), _x3p.hip (its paired-block form), _x3f.hip (the fused pair), _small.hip
bool srf_x3w_supported(int Bt, int pro);
bool srf_x3w_shape_supported(int Cin, int Cout, int L);
size_t srf_x3w_packed_bytes(int Cout, int Cin);
int srf_x3w_pack_launch(const float* const* w, char* const* dst, const int* Cout, const int* Cin, int n, hipStream_t st);
int srf_x3w_pack2_launch(const float* const* w, char* const* dst, char* const* dst16, const int* Cout, const int* Cin, int n,
                         hipStream_t st);
size_t srf_x3w_dec_pack_bytes(int Ci);
int srf_x3w_pack_dec_launch(const float* w, void* dst, int Ci, int M, hipStream_t st);
int srf_x3w_pack_f16_launch(const float* const* w, char* const* dst, const int* Cout, const int* Cin, int n, hipStream_t st,
                            char* const* dst16);
size_t srf_x3w_packed3_bytes(int Cout, int Cin);
int srf_x3w_pack3_launch(const float* const* w, char* const* dst, const int* Cout, const int* Cin, int n, hipStream_t st);
size_t srf_x3p_packed_bytes(int Cout, int Cin);
bool srf_x3f_supported(int Bt, int K1, int C2, int L);
bool srf_pw_small_supported(int Cin, int Cout, int L);
bool srf_pw_small_ragged_supported(int Cin, int Cout, int L);   // the shapes its ragged forms are built for

// ---- srf_pwconv_wgrad.hip: this thread's weight-gradient GEMMs fold their partial sums in a fixed order (no atomic split)
void srf_pw_wgrad_ordered(bool on);
struct SrfWgradOrderedScope {         // ... for the weight-gradient GEMMs of one call, on every path out of it
  SrfWgradOrderedScope() { srf_pw_wgrad_ordered(true); }
  ~SrfWgradOrderedScope() { srf_pw_wgrad_ordered(false); }
};

// ---- srf_backward.hip
int srf_accumulate_launch(float* dst, const float* src, long n, hipStream_t st);
// What one srf_backward call carries across its kernel-level calls -- the deferred parameter-gradient reductions and the
// "merge backward rides on the next GlobLN apply" request (an explicit object; NULL = neither)
struct SrfBwdCtx;
SrfBwdCtx* srf_bwd_ctx_new();
void srf_bwd_ctx_free(SrfBwdCtx* c);
void srf_bwd_ctx_defer(SrfBwdCtx* c, bool on);
void srf_bwd_ctx_merge_sink(SrfBwdCtx* c, float* const* levels, int D);
bool srf_bwd_ctx_merge_taken(const SrfBwdCtx* c);
int srf_bwd_ctx_flush(SrfBwdCtx* c, hipStream_t st);
int srf_gln_bwd_impl(const float* gout, const float* gout2, const float* x, const srf_norm* norm, int groups, int C,
                     int L, float* gx, int accumulate_gx, float* dgamma, float* dbeta, float* dslope, void* scratch,
                     int mode, void* stream, SrfBwdCtx* ctx);
// one norm's parameter sums from the row partials of its scratch slice: recorded for the flush when the context defers, else now
int srf_bwd_ctx_gln_params(SrfBwdCtx* ctx, const srf_norm* norm, void* scratch, int groups, int C, float* dgamma, float* dbeta,
                           float* dslope, hipStream_t st);
// the kernel form a srf_dwconv5_bwd_impl call takes: the chunked kernels (scalar / float4), the row kernel, the row kernel with
// the input norm's reduce pass fused in (what apply-on-load needs)
enum SrfDwBwdForm { SRF_DW_BWD_CHUNKED, SRF_DW_BWD_CHUNKED_FAST, SRF_DW_BWD_ROW, SRF_DW_BWD_ROW_FUSED };
SrfDwBwdForm srf_dwconv5_bwd_form(int Lin, int stride, bool aligned, bool fuse_asked);
bool srf_dwconv5_bwd_rowwise_ok(int Lin, int stride, const void* const* ptrs, int nptrs);
int srf_dwconv5_bwd_impl(const float* gd, const float* xin, const srf_norm* in_norm, const float* w, int groups, int C,
                         int Lin, int stride, float* gin, float* dw, float* dbias, void* scratch, const float* gadd,
                         void* gln_scratch, const float* ax, const srf_norm* anorm, const void* a_scratch, void* stream,
                         SrfBwdCtx* ctx);
bool srf_bwd_level0_proj_ok(int L, const void* const* ptrs, int nptrs);
bool srf_bwd_level0_proj_shape_ok(int L, const void* const* ptrs, int nptrs);
int srf_bwd_level0_proj(const float* G0, const float* y1, const srf_norm* pn, const srf_norm* n0, const float* w0, const float* b0,
                        const void* n0_scratch, void* pn_scratch, void* dw_scratch, float* dw, float* dbias, float* gy1,
                        int groups, int C, int L, void* stream, SrfBwdCtx* ctx);
int srf_bwd_level1_head(const float* G1, const float* d1, const srf_norm* n1, const void* n1_scratch, const float* y1,
                        const srf_norm* pn, const srf_norm* n0, const float* w0, const float* b0, const float* w1, const float* gadd,
                        float* G0, void* n0_scratch, void* dw_scratch, float* dw1, float* db1, int groups, int C, int L,
                        void* stream, SrfBwdCtx* ctx);
