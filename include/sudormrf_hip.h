/*
 * sudormrf_hip.h -- C ABI of libsudormrf_hip.so, the MI355X (gfx950) hot path of
 * SuDoRM-RF (Improved SuDORMRF, GroupComm SuDoRM-RF v2, Causal SuDORMRF v3 and attentive SuDORMRF v2 / v3) inference forward.
 *
 * Boundary replaced (reference is pure PyTorch, paths relative to
 * /root/reference/sudo_rm_rf/dnn/):
 *   srf_forward            <- SuDORMRF.forward            models/improved_sudormrf.py:283-301
 *                             GroupCommSudoRmRf.forward   models/groupcomm_sudormrf_v2.py:302-322
 *   srf_encoder            <- self.encoder (nn.Conv1d)    models/improved_sudormrf.py:247-251,286
 *                             + pad_to_appropriate_length :303-314 (folded into bounds checks)
 *   srf_gln_stats/_apply   <- GlobLN.forward              models/improved_sudormrf.py:30-47
 *   srf_pw_conv            <- nn.Conv1d(kernel_size=1) sites :256-259 (bottleneck), :174 (proj_1x1),
 *                             :196,:220 (res_conv + residual), :268-269,:295-298 (mask_net + ReLU + *s)
 *                             with the neighbouring GlobLN / PReLU folded into prologue / epilogue
 *   srf_dwconv5            <- DilatedConvNorm.conv (depthwise k=5, stride 1|2) :152-153,:206-211
 *   srf_merge              <- Upsample(x2 nearest) + add loop          :190-194,:214-216
 *   srf_decoder            <- self.decoder (nn.ConvTranspose1d)        :272-279,:300 + crop :316-318
 *   srf_tac                <- TAC.forward                 models/groupcomm_sudormrf_v2.py:356-377
 *   srf_gln_apply_add      <- TAC_norm + residual add     models/groupcomm_sudormrf_v2.py:378-382
 *   srf_mixture_consistency<- mixture_consistency.apply   experiments/utils/mixture_consistency.py:14-36
 *   srf_wav_normalize / srf_wav_denormalize <- the callers' normalise / rescale lines   README.md:100-114
 *   srf_pit_sisdr_*        <- PITLossWrapper(PairwiseNegSDR("sisdr")) fwd/bwd        losses/sisdr.py:254-311,426-458
 *   srf_perm_inv_sisdr     <- PermInvariantSISDR.forward (validation metric)        losses/sisdr.py:66-196
 *   srf_forward (causal)   <- CausalSuDORMRF.forward      models/causal_improved_sudormrf_v3.py (ABI 16)
 *   srf_forward (attentive)<- SuDORMRF.forward             models/attentive_sudormrf_v2.py (srf_attentive_plan_create, below)
 *   srf_forward (att. v3)  <- SuDORMRF.forward             models/attentive_sudormrf_v3.py (srf_attentive_v3_plan_create, below)
 *   srf_forward (original) <- SuDORMRF.forward             models/sudormrf.py (srf_original_plan_create, below)
 *   srf_mha_attention      <- MHAttentionLayer.forward: softmax(q k^T / sqrt(d)) v per head, between its four Linear layers
 *   srf_mha_attention_lse / _bwd <- the same under autograd: forward that keeps the log-sum-exp, and its gradient
 *   srf_mha_attention_ragged / _lse_ragged / _bwd_ragged <- the three with one query and one key length per example
 *   srf_stream_*           <- the same model run chunk by chunk with device-side state (ABI 17; row-table push: ABI 19)
 *   srf_zeroref_snr_*      <- PermInvariantSNRwithZeroRefs fwd/bwd (FUSS training loss)  losses/snr.py:13-142 (ABI 18)
 *   srf_stab_sisdr         <- StabilizedPermInvSISDRMetric.forward (FUSS validation)    losses/sisdr.py:460-576
 *   srf_fuss_augment       <- online_augment + mixture normalisation   experiments/run_fuss_separation.py:195-243
 *   srf_causal_encoder     <- its encoder (ScaledWSConv1d, 2K-1 taps of which K are live)
 *   srf_causal_dwconv / _merge / _pyramid <- UConvBlock's causal k = 21 depthwise pyramid + upsample/add
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous fp32 (or fp64 for GlobLN sums) owned by the
 *     caller; the library allocates nothing on the device; global state = a thread-local error string,
 *     the kernel-mode switch and the (off by default) profiler;
 *   - activations are [batch, channel, time] contiguous, exactly as the reference's tensors;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); all work is asynchronous
 *     on that stream, nothing synchronises;
 *   - return value: 0 on success, a negative SRF_E* code otherwise (srf_last_error() has the text);
 *     nothing throws across the ABI;
 *   - GlobLN statistics travel as fp64 {sum, sum_of_squares} pairs ("sums",
 *     [groups][SRF_STAT_BUCKETS][2]); producers ACCUMULATE into them (atomics), so the caller zeroes
 *     them first (srf_forward does it itself).
 */
#ifndef SUDORMRF_HIP_H
#define SUDORMRF_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRF_ABI_VERSION 19

/* GlobLN statistics layout: "sums" = fp64 [groups][SRF_STAT_BUCKETS][2] {sum, sum of squares}; the
 * statistic of a group is the total over its buckets (producers spread their atomics over buckets). */
#define SRF_STAT_BUCKETS 64

#define SRF_OK 0
#define SRF_EINVAL (-1)   /* bad argument / unsupported shape */
#define SRF_EHIP (-2)     /* a HIP runtime call or kernel launch failed */
#define SRF_EWORKSPACE (-3) /* workspace too small */

#define SRF_VARIANT_IMPROVED 0
#define SRF_VARIANT_GROUPCOMM 1
#define SRF_VARIANT_CAUSAL 2      /* CausalSuDORMRF (causal_improved_sudormrf_v3.py), ABI 16; trains through srf_causal_* only */

/* Constructor arguments of the reference models, same meaning
 * (improved_sudormrf.py:224-231, groupcomm_sudormrf_v2.py:232-241, causal_improved_sudormrf_v3.py CausalSuDORMRF).
 * Causal: in_audio_channels is used (A), group_size must be 1. */
typedef struct srf_config {
  int variant;           /* SRF_VARIANT_* */
  int in_audio_channels; /* 1 for Improved; A for GroupComm and Causal */
  int out_channels;      /* B */
  int in_channels;       /* C */
  int num_blocks;        /* U */
  int upsampling_depth;  /* D */
  int enc_kernel_size;   /* K (odd) */
  int enc_num_basis;     /* N */
  int num_sources;       /* S */
  int group_size;        /* G (1 for Improved) */
} srf_config;

/* "Apply GlobLN (+ optional PReLU) to this tensor when it is loaded". */
typedef struct srf_norm {
  const double* sums;  /* [groups][SRF_STAT_BUCKETS][2] over (channel,time); NULL = no normalisation */
  const float* gamma;  /* [channels] */
  const float* beta;   /* [channels] */
  const float* prelu;  /* [1] shared slope, or NULL = no activation */
} srf_norm;

typedef struct srf_plan srf_plan;

int srf_abi_version(void);
const char* srf_last_error(void);

/* Kernel-variant switch for A/B measurements:
 *   0 = fast paths where the shape allows (default); 1x1 convs run as split-precision MFMA GEMMs
 *       (each fp32 operand = bf16 hi + bf16 lo, three bf16 MFMAs per product block, fp32 accumulate);
 *   1 = force the generic (shape-agnostic, scalar-load, fp32 FMA) kernels everywhere;
 *   2 = fast paths, but 1x1 convs on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32). */
void srf_set_kernel_mode(int mode);
int srf_get_kernel_mode(void);
/* In-library profiler (bench.py): between begin/end every kernel launched through this library is
 * followed by a HIP event on the caller's stream; end() synchronises the stream and get(i) returns
 * the kernel family name and the elapsed ms between the previous event and launch i's event
 * (i.e. that launch's duration including its launch gap).  Not thread-safe; off by default. */
int srf_profile_begin(void* stream);
int srf_profile_end(void* stream, int* count);
int srf_profile_get(int i, const char** name, float* ms);
/* The same marks as a timeline: completion time of launch i in ms since srf_profile_begin and the index (order of first
 * appearance) of the stream it ran on -- for forwards whose sub-batches run on several streams (synchronise the device before
 * srf_profile_end); tools/two_stream_events.py. */
int srf_profile_timeline(int i, const char** name, float* t_ms, int* stream_index);

/* ---- SRF_DIAGNOSTICS -----------------------------------------------------------------------------------------------------
 * NOT part of the drop-in surface: process-wide switches between kernel variants for A/B measurements and bisection
 * (tools/, bench.py --debug-flags, a handful of tests).  They act on every thread's subsequent launches; a caller that does
 * not define SRF_DIAGNOSTICS before including this header does not see them.  Default 0 = the shipped paths.
 * One bit per switch: enum srf_debug_flag below.  The VALUES are frozen (bench.py --debug-flags and tools/gpu_ab.sh take
 * numbers on their command lines); sudo_rm_rf_amd.ops.DebugFlag mirrors the names without the SRF_DBG_ prefix. */
#ifdef SRF_DIAGNOSTICS
enum srf_debug_flag {
  /* srf_forward WITHOUT the fused conv pairs (round 5: res_conv / bottleneck + the next proj_1x1 in one launch) */
  SRF_DBG_NO_PAIRS = 1,
  /* 256 x 128 GEMMs: no m-tile groups (round 2's tile order); paired-block form: plain cache policy */
  SRF_DBG_GEMM_NO_MGROUPS = 2,
  /* without the 256 x 128 GEMM (128 x 128 kernels) */
  SRF_DBG_NO_GEMM_256 = 4,
  /* WITHOUT pre-packed weights (srf_forward packs by default) */
  SRF_DBG_NO_PACKED_WEIGHTS = 8,
  /* per-level depthwise + merge kernels instead of the fused pyramid (inference and training) */
  SRF_DBG_PYR_PER_LEVEL = 16,
  /* LDS pyramid kernels (with PYR_NO_REG): the block-per-row kernel instead of the wave-per-tile one */
  SRF_DBG_PYR_NO_LDS_TILES = 32,
  /* LDS pyramid kernels instead of the register ones */
  SRF_DBG_PYR_NO_REG = 64,
  /* non-persistent pyramid pass 1 */
  SRF_DBG_PYR_PASS1_NONPERSISTENT = 128,
  /* leftover GEMM tiles as whole tiles (no quarter tiles) */
  SRF_DBG_GEMM_WHOLE_TAIL_TILES = 256,
  /* quarter tiles last */
  SRF_DBG_GEMM_QUARTER_TILES_LAST = 512,
  /* TAC forward with one time step per lane */
  SRF_DBG_TAC_ONE_STEP_PER_LANE = 1024,
  /* one-tile-per-block 128 x 128 GEMM everywhere (also: no 64 x 64 tiles for small launches) */
  SRF_DBG_GEMM_128_ONE_TILE_PER_BLOCK = 2048,
  /* weight-gradient GEMM: round 3's block -> (tile, partial) mapping (every XCD re-reads its rows through its own L2) */
  SRF_DBG_WGRAD_NO_XCD_MAP = 4096,
  /* swap the two forms of the 256 x 128 GEMM: srf_forward / srf_separate run the one-block-per-CU kernel (srf_pwconv_x3w.hip),
   * every other caller the paired-block kernel (srf_pwconv_x3p.hip) -- default: the paired form inside the forward only */
  SRF_DBG_GEMM_256_SWAP_FORMS = 8192,
  /* training forward: three bf16 parts per operand (6 MFMAs, round 3) instead of two fp16 parts (3 MFMAs, round 4).
   * Range of the two-fp16-part form: an operand at or beyond 65520 makes its outputs non-finite (fp16 ends at 65504); an
   * activation tensor whose level as a whole is below 1e-2 leaves the 2e-6 accuracy class (relative error 1.6e-5 at 1e-3, ten
   * times more per decade below: fp16's normal numbers end at 6.1e-5, its subnormals at 6e-8).  The three-part form has fp32's
   * exponent range and neither limit. */
  SRF_DBG_TRAIN_BF16X3 = 16384,
  /* WITHOUT the fused tail: mask GEMM -> masked tensor -> decoder frame GEMM -> overlap-add as separate launches */
  SRF_DBG_NO_FUSED_TAIL = 32768,
  /* srf_backward WITHOUT the fused head of the blocks' pyramid backward (round 6: level 0 + proj_1x1's norm as two passes
   * over {G_0, y1}): the level-0 conv kernel + the norm's apply pass of rounds 3-5 (set it around BOTH calls: a forward
   * run without it leaves d_0 out of `saved`, and its backward then takes the head whatever the flag says) */
  SRF_DBG_BWD_NO_FUSED_HEAD = 1 << 16,
  /* pyramid pass 1 on a grid of co-resident wavefronts, several rows each (rounds 2-5) -- default since round 6: one row
   * per wavefront */
  SRF_DBG_PYR_PASS1_ROWS_PER_WAVE = 1 << 17,
  /* weight-gradient GEMM WITHOUT the wide tile (round 6: 256 x 128 / 128 x 256, one block per CU): the 128 x 128 kernel;
   * small-channel form on a fixed 1024 blocks (rounds 3-5) instead of one resident round */
  SRF_DBG_WGRAD_NO_WIDE_TILE = 1 << 18,
  /* weight-gradient GEMM, 128 x 128 kernel: the masked form for full shapes too (rounds 3-5) */
  SRF_DBG_WGRAD_128_MASKED = 1 << 19,
  /* weight-gradient GEMM, wide tile: 800-column time chunks (several per block) instead of one long chunk per block */
  SRF_DBG_WGRAD_SHORT_CHUNKS = 1 << 20,
  /* fused conv pair on persistent blocks (2 per CU, several tiles each) whatever the launch size -- default: one tile per block */
  SRF_DBG_PAIR_PERSISTENT = 1 << 21,
  /* TAC forward / backward on the VALU kernels instead of the MFMA forms (n = 16, G = 16) */
  SRF_DBG_TAC_VALU = 1 << 22,
  /* fused conv pair with every counted wait of its DMA pipeline as a full drain (bisection aid, same results) */
  SRF_DBG_PAIR_FULL_DRAIN = 1 << 23,
  /* TAC forward on the generic kernel (no lane-per-time-step form) */
  SRF_DBG_TAC_GENERIC = 1 << 24,
  /* weight-gradient partials folded by one chain per output (rounds 3-4) instead of four groups per output (round 5) */
  SRF_DBG_WGRAD_ONE_CHAIN_FOLD = 1 << 25,
  /* TAC forward: the lane-per-time-step form with four tiles per block */
  SRF_DBG_TAC_LANES_4TILES = 1 << 26,
  /* 64-bit pointer loads in the 128 x 128 GEMM (no buffer loads) */
  SRF_DBG_GEMM_128_POINTER_LOADS = 1 << 27,
  /* training forward on the split-bf16 GEMMs (faster; gradients then differ from the reference by ~3e-3) */
  SRF_DBG_TRAIN_FWD_SPLIT_BF16 = 1 << 28,
  /* chunked depthwise-backward kernels and no backward fusion */
  SRF_DBG_BWD_DW_CHUNKED = 1 << 29,
  /* scalar GlobLN-backward kernels and no backward fusion */
  SRF_DBG_BWD_GLN_SCALAR = 1 << 30,
  /* training forward on the exact-fp32 MFMA kernel instead of the three-part split GEMM.  Bit 31 of an int: INT_MIN */
  SRF_DBG_TRAIN_FWD_EXACT_MFMA = -2147483647 - 1
};
void srf_set_debug_flags(int flags);
#endif

/* ---- whole-model path ---------------------------------------------------------------------- */
int srf_plan_create(const srf_config* cfg, int batch, int T, srf_plan** out);
void srf_plan_destroy(srf_plan* plan);
size_t srf_plan_workspace_bytes(const srf_plan* plan);
int srf_plan_num_params(const srf_plan* plan);    /* tensors in state_dict() order */
int srf_plan_frames(const srf_plan* plan);        /* L */
int srf_plan_padded_length(const srf_plan* plan); /* T' */
int srf_plan_num_launches(const srf_plan* plan);  /* kernel launches per forward (informational) */

/* params: host array of num_params device pointers in the reference's state_dict() order
 * (causal: DESIGN.md §11).  wav: [batch, in_audio_channels, T].  out: [batch, S*in_audio, T].
 * Causal plans: skipinit_gain (a device scalar per block) is folded into res_conv inside the forward, never read by the
 * host; srf_forward_train / srf_backward[_wav], their buffer sizes and srf_separate refuse causal plans with SRF_EINVAL --
 * the causal model trains through the opt-in srf_causal_forward_train / srf_causal_backward below. */
int srf_forward(const srf_plan* plan, const float* const* params, int num_params,
                const float* wav, float* out, void* workspace, size_t workspace_bytes, void* stream);

/* Ragged-batch forward (additive to ABI 19): ONE set of launches over utterances of unequal length.  wav: [batch, 1, T] padded
 * rows, lengths: HOST array [batch], 1 <= lengths[b] <= T (T = the plan's: no example has to be that long, so a caller keeps
 * one plan per length bucket).  out[b, :, :lengths[b]] is what srf_forward on a batch-1 plan of length lengths[b] returns
 * for wav[b, :, :lengths[b]] alone (each example is padded to ITS OWN multiple of (K/2) 2^D, its GlobLNs run over its own
 * frames); out[b, :, lengths[b]:] is exactly 0; wav[b, :, lengths[b]:] is never read and may hold anything, NaN included.
 * The lengths reach the kernels by value in the launch arguments (see "Ragged forms" below): nothing is uploaded or
 * synchronised, and a ragged batch is capped at SRF_RAGGED_MAX_BATCH = 128 examples.
 * srf_plan_ragged_supported: 1 for an Improved plan (one audio channel, K = 21, out_channels = 256, batch <= 128) whose
 * uniform forward, under the current kernel mode, runs the packed 256 x 128 GEMMs, the register-resident fused pyramid and
 * the fused mask + decoder tail; 1 for a GroupComm plan with one audio channel, K = 21, group_size = 16, out_channels = 256,
 * in_channels = 512 (the thin conv's ragged forms: 16 <-> 32 channels per group), batch <= 128, whose uniform forward runs
 * the packed bottleneck GEMM, the MFMA TAC, the fused pre-add, the register-resident pyramid and the fused tail; every other
 * GroupComm plan and causal plans: 0.  The ragged forward runs the fused conv pair and the 256 x 128
 * kernel whatever the uniform forward's "at least as many tiles as CUs" gates say; plans too small for the fused tail are
 * not supported (run those examples one by one).  GroupComm launch sequence: encoder, bottleneck GEMM, per block TAC ->
 * pre-add proj_1x1 -> pyramid (16 folded rows per example) -> res_conv, then the unchanged mask + decoder GEMM and the ragged
 * overlap-add (srf_tac_ragged, srf_pw_conv_small_ragged, srf_pyramid_ragged_rows below).
 * srf_plan_ragged_workspace_bytes: the workspace the ragged call needs (0 = not supported); srf_plan_workspace_bytes is
 * unchanged.  Refused with SRF_EINVAL BEFORE anything is launched, srf_last_error() naming the example: an unsupported plan,
 * a length outside 1..T, an example whose padded length the fused pyramid does not take as a row length of its own
 * (srf_pyramid_ragged_frames_ok: shorter than 8 * 2^(D-1) frames, or off the kernels' chunk grid). */
int srf_plan_ragged_supported(const srf_plan* plan);
size_t srf_plan_ragged_workspace_bytes(const srf_plan* plan);
int srf_forward_ragged(const srf_plan* plan, const float* const* params, int num_params, const float* wav,
                       const int* lengths /* host, [batch] */, float* out, void* workspace, size_t workspace_bytes,
                       void* stream);

/* The whole caller-side inference recipe in ONE forward (README.md:100-114): per-example {mean,
 * unbiased std} of the RAW mixture (written to `stats`, [batch][2] device floats), normalisation folded into the encoder's
 * load, "estimates * std + mean" and -- mixture_consistency != 0, as the README prescribes for the GroupComm models --
 * mixture_consistency.apply against the normalised mixture folded into the decoder's overlap-add.  Single-channel
 * mixtures (in_audio_channels = 1).  Same buffers and rules as srf_forward. */
int srf_separate(const srf_plan* plan, const float* const* params, int num_params, const float* wav, float* out,
                 float* stats, int mixture_consistency, void* workspace, size_t workspace_bytes, void* stream);

/* srf_separate over a ragged batch (additive to ABI 19): srf_forward_ragged with the recipe folded in, every step over the
 * example's OWN samples.  wav: the RAW padded mixture [batch, 1, T]; lengths: HOST array [batch]; stats: [batch][2] device
 * floats, WRITTEN: {mean, unbiased std} of wav[b, 0, :lengths[b]] (one srf_wav_stats_ragged launch in front of the forward).
 * The ragged encoder normalises on load -- the zero padding past lengths[b] is that of the NORMALISED signal -- and the
 * ragged overlap-add stores est * std + mean and, mixture_consistency != 0, the correction against the mixture re-normalised
 * from the raw row, for t < lengths[b]; out[b, :, lengths[b]:] is exactly 0, and wav[b, :, lengths[b]:] is never read, by
 * the mixture-consistency step either.  Same gate (srf_plan_ragged_supported), workspace and length rules as
 * srf_forward_ragged; refused with SRF_EINVAL BEFORE anything is launched, srf_last_error() naming the example: an
 * unsupported plan (causal plans included), a length outside 1..T, a length the pyramid does not take, a null pointer.
 * Placement: workspace 256-byte aligned; wav, out and stats at any float-aligned address. */
int srf_separate_ragged(const srf_plan* plan, const float* const* params, int num_params, const float* wav,
                        const int* lengths /* host, [batch] */, float* out, float* stats /* [batch][2], written */,
                        int mixture_consistency, void* workspace, size_t workspace_bytes, void* stream);

/* The ragged forward of the ORIGINAL model (plans of srf_original_plan_create; additive to ABI 19).
 * Opt-in through entry points of its own: srf_plan_ragged_supported stays 0 for such a plan and srf_forward_ragged /
 * srf_separate_ragged keep refusing it.  Same contract as the two above: out[b, :, :lengths[b]] is what srf_forward (resp.
 * srf_separate) on a batch-1 plan of length lengths[b] returns for row b alone -- the row padded to ITS OWN multiple of
 * lcm(K / 2, 2^D), this model's rule, every GroupNorm over its own frames --, out[b, :, lengths[b]:] is exactly 0 and
 * wav[b, :, lengths[b]:] is never read.  srf_original_separate_ragged: stats [batch][2] receives {mean, unbiased std} per row.
 * srf_original_ragged_supported: 1 only for an original plan with K = 21, batch <= SRF_RAGGED_MAX_BATCH, num_sources <= 16, under
 * kernel mode 0 with packed weights on, whose 1x1 convolutions -- l1, proj_1x1, conv_1x1_exp, reshape_before_masks where present,
 * the mask GEMM N -> S N -- all are shapes of the 256 x 128 GEMM (Cin % 64 == 0, Cin >= 128, Cout >= 192) within its 32-bit reach
 * and with at least 8 tiles, and whose frame count the register-resident fused pyramid takes.  (The README recipe, B 256 / C 512
 * / N 512, passes; out_channels = 128 does not: conv_1x1_exp then has 128 < 192 output rows.)
 * srf_original_ragged_workspace_bytes: the workspace the ragged call needs (0 = not supported).
 * Refused with SRF_EINVAL BEFORE anything is launched, srf_last_error() containing "original" and naming the example: a plan
 * the gate does not take (plans of other variants included), a length outside 1..T, a row whose own frame count the pyramid
 * does not take (srf_pyramid_ragged_frames_ok: at D <= 4 the lengths off the 16-frame chunk grid; at D = 5 every length of at
 * least 1280 samples passes).  Placement as srf_forward_ragged. */
int srf_original_ragged_supported(const srf_plan* plan);
size_t srf_original_ragged_workspace_bytes(const srf_plan* plan);
int srf_original_forward_ragged(const srf_plan* plan, const float* const* params, int num_params, const float* wav,
                                const int* lengths /* host, [batch] */, float* out, void* workspace, size_t workspace_bytes,
                                void* stream);
int srf_original_separate_ragged(const srf_plan* plan, const float* const* params, int num_params, const float* wav,
                                 const int* lengths /* host, [batch] */, float* out, float* stats /* [batch][2], written */,
                                 int mixture_consistency, void* workspace, size_t workspace_bytes, void* stream);

/* Causal plans only: the per-block plain attributes alpha / beta of UConvBlock (both 1.0 as the reference constructs them,
 * the default of a new plan).  srf_forward computes res_conv(.) * skipinit_gain * alpha[i] + x and proj_1x1(x / beta[i]).
 * alpha, beta: host arrays of n = num_blocks floats.  Call before the plan's first forward. */
int srf_plan_set_block_scales(srf_plan* plan, const float* alpha, const float* beta, int n);

/* Copy an intermediate of the LAST srf_forward on this workspace into dst (for parity tests).
 * what: 0 = encoder output [Bt,N,L], 1 = separation-module output [Bt,B,L], 2 = masked [Bt,S*A*N,L]
 * (causal plans: 2 = mask_net output before mask_nl_class).
 * 2 fails (SRF_EINVAL) at shapes whose forward runs the mask GEMM fused with the decoder (launches with at least as many
 * 256 x 128 tiles as the GPU has CUs): the masked tensor then never exists in memory. */
int srf_debug_fetch(const srf_plan* plan, const void* workspace, int what, float* dst, size_t dst_floats,
                    void* stream);

/* ---- per-kernel entry points (unit parity + building blocks) -------------------------------- */

/* Operand placement.  Every device pointer below must be aligned for its element type (float: 4 bytes, double: 8).
 * Outputs and scratch need NO initialisation (every element an entry point documents as written is written; nothing is
 * read before it is written); only what is documented as "+=" / ACCUMULATED must hold the caller's running value
 * (zero for a fresh sum).  Nothing is read or written outside the extents given.  What a base that is element aligned
 * but NOT 16-byte aligned does (a view such as x[..., a:b] of a [1, 1, T] signal, a parameter carved out of a flat
 * buffer) is, per entry point -- the same table as tests/placement.py PLACEMENT, which the GPU suite runs:
 *   any address   every float operand of srf_encoder, srf_gln_stats, srf_gln_apply(_add), srf_conv1d,
 *                 srf_mixture_consistency(_magsq), srf_mask_apply, srf_mask_bwd, srf_frames_gather, srf_wav_normalize,
 *                 srf_wav_stats, srf_wav_denormalize, srf_causal_encoder, srf_causal_dwconv, srf_causal_merge,
 *                 srf_causal_stream_pyramid, srf_causal_scale, srf_prelu_apply, srf_clip_adam_step's tensors, the PIT /
 *                 permutation-invariant SI-SDR inputs; every bias / gamma / beta / PReLU slope / depthwise or TAC weight
 *                 of every entry point; every out_sums (accumulated one double at a time).
 *   falls back    the result is the same to rounding, a slower kernel serves the call:
 *                 srf_pw_conv / _packed / _packed3: x, w, y, residual, mul -> the scalar kernel (pw_conv_generic); w_packed /
 *                   w_packed3 -> the kernels that split the fp32 weight themselves;
 *                 srf_dwconv5: x, y -> dwconv5_generic;  srf_merge: levels, y -> merge_generic;
 *                 srf_decoder: v -> the scalar frame GEMM (out: any address);
 *                 srf_tac: x, q -> the VALU kernels;  srf_causal_pyramid: y1 -> scalar loads;
 *                 srf_pw_wgrad*: dw, scratch -> the scalar fold of the partial sums;
 *                 srf_gln_bwd: gout, gout2, x, gx;  srf_merge_bwd: g_merged, g_levels (the chain of pair sums);
 *                 srf_dwconv5_bwd: gd, xin, gin;  srf_prelu_bwd: gout, x, gx;
 *                 the zero-reference SNR / stabilized SI-SDR / FUSS augmentation rows (16-byte loads only when T % 4 == 0 and
 *                 the bases are on the grid).
 *   refused       SRF_EINVAL before anything is launched, srf_last_error() names the operand ("operand 'x' is not 16-byte
 *                 aligned"): every GlobLN statistics INPUT (srf_norm.sums: read as pairs of doubles);
 *                 srf_pack_pw_weights / srf_pack3_pw_weights: packed;  srf_pw_conv_pair / _pair_packed3: x, y, y2,
 *                 residual, both packed images;  srf_pyramid: y1, merged, scratch;  srf_decoder: scratch;
 *                 srf_pw_wgrad*: g, x;  srf_gln_bwd: scratch;  srf_tac_bwd: x, go, gx, scratch.
 *   256 bytes     the whole-model buffers (workspace, saved, train scratch) and the stream session's weights_buf / state /
 *                 workspace, as stated with those entry points; wav and out of srf_forward / srf_separate / srf_forward_train /
 *                 srf_stream_push / srf_stream_push_rows, and out_tail of srf_stream_flush / srf_stream_flush_rows: any
 *                 address. */

/* out[b,n,l] = sum_{a,k} w[n,a,k] * xpad[b,a,h*l+k-h], h=K/2; samples outside [0,T) are zero, so the
 * reference's right zero-padding is implicit in L.  sums (nullable): [Bt][SRF_STAT_BUCKETS][2] += {sum, sumsq}. */
int srf_encoder(const float* wav, const float* w, float* out, double* sums,
                int Bt, int A, int T, int N, int K, int L, void* stream);

/* ---- Ragged forms: one launch over examples of unequal length (additive; SRF_ABI_VERSION unchanged) ----
 * A ragged form takes its uniform twin's arguments plus HOST tables with one entry per example.  The layout does not change:
 * T and L stay the row strides of [Bt, ., T] / [Bt, ., L] tensors; example b is lengths[b] <= T samples and frames[b] <= L
 * frames long.  Everything at or past an example's end is treated as the zero padding its own batch-1 call would see:
 * it is never read (it may hold anything, NaN included), statistics count the example's own elements only, and outputs
 * that carry statistics are stored as exact zeros from the example's end to the row stride.  The tables reach the kernels BY
 * VALUE in the launch arguments -- no upload, no synchronisation -- which caps a ragged batch at SRF_RAGGED_MAX_BATCH examples;
 * larger batches, out-of-range entries and lengths a kernel cannot take are refused (SRF_EINVAL, the message names the
 * example) before anything is launched.  The profiler names of the ragged kernels carry the suffix "_ragged".
 * Kernels that run over FOLDED rows (GroupComm folds its groups into the batch: rows = examples * rows_per_example) keep
 * the table at ONE ENTRY PER EXAMPLE and find a row's example as row / rows_per_example: srf_pyramid_ragged_rows,
 * srf_pw_conv_small_ragged. */
#define SRF_RAGGED_MAX_BATCH 128
/* srf_encoder over a ragged batch (A = 1, K = 21 only: the shape of the published Improved models).  Requires
 * lengths[b] <= (K/2) * frames[b]; frames[b] = padded length / hop of example b (srf_plan_padded_length of a batch-1 plan). */
int srf_encoder_ragged(const float* wav, const float* w, float* out, double* sums, int Bt, int A, int T, int N, int K, int L,
                       const int* lengths, const int* frames, void* stream);
/* A test and building-block entry (srf_separate_ragged reaches the same kernel internally; nothing else in the library calls
 * this one).  The same with the caller-side normalisation folded into the load: in_stats [Bt][2] {mean, std} per row (srf_wav_stats_ragged);
 * the kernel sees (x - mean) / (std + 1e-9) on [0, lengths[b]) and zeros past it.  in_stats: any float-aligned address. */
int srf_encoder_ragged_stats(const float* wav, const float* w, float* out, double* sums, int Bt, int A, int T, int N, int K,
                             int L, const int* lengths, const int* frames, const float* in_stats, void* stream);
/* stats[r] = {mean, unbiased std} of wav[r, :lengths[r]] for the rows of a padded [rows, T] tensor (T = the row stride;
 * rows <= SRF_RAGGED_MAX_BATCH, 1 <= lengths[r] <= T, lengths on the HOST).  The arithmetic of srf_wav_stats: fp64 mean, then
 * the fp64 sum of squared deviations over max(lengths[r] - 1, 1); one block per row and a fixed reduction order, so a row's
 * two numbers are the same bits whatever the other rows hold.  Nothing at or past lengths[r] is read.  wav, stats: any
 * float-aligned address. */
int srf_wav_stats_ragged(const float* wav, const int* lengths /* host */, float* stats, int rows, int T, void* stream);
/* The padded batch from the caller's separate utterance buffers, in one launch: rows = HOST array of `batch` DEVICE pointers,
 * utterance b = lengths[b] floats at rows[b].  wav[b, 0, :lengths[b]] receives them bit for bit; wav[b, 0, lengths[b]:] is NOT
 * written (no ragged entry point reads it).  The pointers travel by value in the launch arguments, as the lengths do
 * (batch <= SRF_RAGGED_MAX_BATCH).  Refused before the launch: a null entry of rows (the message names the example), a
 * length outside 1..T.  Sources and wav: any float-aligned address (4-byte copies); a source must not overlap wav. */
int srf_wav_gather_ragged(const float* const* rows /* host array of device pointers */, const int* lengths /* host */,
                          float* wav /* [batch, 1, T] */, int batch, int T, void* stream);
/* The original model's own kernels over a ragged batch (their uniform twins: "Original SuDoRM-RF" below; additive to ABI 19).
 * srf_gln_apply_c_ragged: group g is frames[g] columns long (frames[g] % 4 == 0).  x and add are not read at columns >=
 *   frames[g]; y is exact 0 on [frames[g], length); the GlobLN count is channels * frames[g]; out_sums run over the group's own
 *   columns.  With frames[g] == length for every g, y is bit for bit srf_gln_apply_c's.  Any float-aligned address.
 * srf_encoder_bias_relu_ragged (K = 21 only, not under kernel mode 1): samples at or past lengths[b] are never read (with
 *   in_stats the zero padding is that of the normalised signal); frames at or past frames[b] are stored as exact 0 -- relu(bias)
 *   is not zero -- and the sums run over the example's own frames.  Requires lengths[b] <= (K/2) * frames[b].
 * srf_softmax_mask_ragged: z and enc are not read at columns >= frames[b] (z may hold anything there, NaN included); v is
 *   exact 0 there.  v may be z.
 * srf_bias_rescale_ragged: t < lengths[b]: as srf_bias_rescale; t >= lengths[b]: exactly 0.f, and wav is never read there. */
int srf_gln_apply_c_ragged(const float* x, const srf_norm* norm, const float* slopes, const float* add, float* y,
                           double* out_sums, int groups, int channels, int length, const int* frames, void* stream);
int srf_encoder_bias_relu_ragged(const float* wav, const float* w, const float* bias, float* out, double* sums, int Bt, int T,
                                 int N, int K, int L, const int* lengths, const int* frames, const float* in_stats, void* stream);
int srf_softmax_mask_ragged(const float* z, const float* enc, float* v, int Bt, int S, int N, int L, const int* frames,
                            void* stream);
int srf_bias_rescale_ragged(float* out, const float* bias, const float* stats, const float* wav, int mc, int Bt, int S, int T,
                            const int* lengths, void* stream);

/* sums[g][bucket][0..1] += {sum, sumsq} of x[g, :, :] (x: [groups, channels*length]). */
int srf_gln_stats(const float* x, double* sums, int groups, long per_group, void* stream);
/* y = gamma_c * (x - mu_g) / sqrt(var_g + 1e-8) + beta_c, then optional PReLU. */
int srf_gln_apply(const float* x, float* y, const srf_norm* norm, int groups, int channels, int length,
                  void* stream);
/* y = x + GlobLN(q)  (TAC_norm + residual). */
int srf_gln_apply_add(const float* x, const float* q, float* y, const srf_norm* norm, int groups,
                      int channels, int length, void* stream);

/* 1x1 convolution y[b,m,l] = bias[m] + sum_k w[m,k] * f(x[b,k,l])  (+ residual[b,m,l]),
 * f = in_norm (GlobLN and/or PReLU on load; NULL = identity).
 * epilogue_mask != 0:  y = relu(y) * mul[b, m % mul_channels, l]   (mask_nl_class + "* s.unsqueeze(1)").
 * out_sums (nullable): [Bt][SRF_STAT_BUCKETS][2] += {sum, sumsq} of the stored y. */
int srf_pw_conv(const float* x, const float* w, const float* bias, float* y,
                int Bt, int Cin, int Cout, int L, const srf_norm* in_norm, const float* residual,
                double* out_sums, int epilogue_mask, const float* mul, int mul_channels, void* stream);

/* Pre-packed weights for the split-precision GEMM (kernel mode 0): the fp32 weight [Cout,Cin] is split
 * into bf16 hi/lo and laid out tile-by-tile ONCE (srf_forward does it at the start of every forward for
 * all its 1x1 convolutions, in one launch).  srf_packed_pw_weight_bytes() = 0 when the shape does not
 * qualify (needs Cin % 64 == 0, Cout >= 192); srf_pw_conv_packed() with w_packed = NULL (or a
 * non-qualifying shape / mode) is exactly srf_pw_conv().  packed buffers: 16-B aligned device memory.
 * Round 4: a packed buffer holds TWO layouts of the same bf16 parts, written by the one pack launch -- the image of the
 * one-block-per-CU kernel (srf_pwconv_x3w.hip: what srf_pw_conv_packed runs) and the image of the paired-block kernel
 * (srf_pwconv_x3p.hip: two co-resident blocks per CU, bit-identical outputs, what srf_forward / srf_separate run for their
 * proj_1x1 / res_conv / bottleneck GEMMs so that a caller's second stream can share the CUs); srf_packed_pw_weight_bytes
 * covers both.  Always size the buffer with that function. */
size_t srf_packed_pw_weight_bytes(int Cout, int Cin);
int srf_pack_pw_weights(const float* const* w, void* const* packed, const int* Cout, const int* Cin, int n,
                        void* stream);
int srf_pw_conv_packed(const float* x, const float* w, const void* w_packed, const float* bias, float* y,
                       int Bt, int Cin, int Cout, int L, const srf_norm* in_norm, const float* residual,
                       double* out_sums, int epilogue_mask, const float* mul, int mul_channels, void* stream);

/* Round 5: TWO 1x1 convolutions back to back in ONE launch (csrc/srf_pwconv_x3f.hip) -- a conv with Cmid = 256 output channels
 * and the conv that consumes its output, the 256-channel tensor handed over in registers (it is still written to y: it is the
 * model's residual stream):
 *     y  = W1 f(x) + bias1 (+ residual)     f = in_norm: GlobLN (bottleneck, improved_sudormrf.py:292: no residual),
 *                                           GlobLN + PReLU (res_conv, :218-220: residual required), or NULL: no prologue,
 *                                           residual required (the backward's data-gradient pair W_proj^T g + skip, W_res^T of it)
 *     y2 = W2 y + bias2,  out_sums2 (nullable) += {sum, sumsq} of y2          (proj_1x1 of the next block, :205)
 * Results are BIT-IDENTICAL to srf_pw_conv_packed(x -> y) followed by srf_pw_conv_packed(y -> y2) (statistics: to rounding).
 * w1_packed / w2_packed: buffers of srf_pack_pw_weights for [Cmid, Cin1] / [Cout2, Cmid].  srf_pw_conv_pair_supported: the
 * shapes served (Cmid = 256, Cin1 % 64 == 0, 128 <= Cin1 <= 512, Cout2 % 128 == 0, Cout2 <= 512, L % 4 == 0, at least as
 * many 128-column tiles as CUs) under the default kernel mode; srf_forward uses the pair wherever this says 1. */
int srf_pw_conv_pair_supported(int Bt, int Cin1, int Cmid, int Cout2, int L);
int srf_pw_conv_pair(const float* x, const void* w1_packed, const float* bias1, float* y, const srf_norm* in_norm,
                     const float* residual, const void* w2_packed, const float* bias2, float* y2, double* out_sums2,
                     int Bt, int Cin1, int Cmid, int Cout2, int L, void* stream);

/* The ragged forms of the two (see "Ragged forms" above; frames[b] % 4 == 0).  Columns are independent in a 1x1 convolution, so
 * nothing is masked on load.  What an output holds past an example's end: exact zeros where the launch accumulates statistics
 * (srf_pw_conv_packed_ragged with out_sums, and y2 of the pair), unspecified otherwise (y of the pair and the residual form:
 * the model's block stream, which only pointwise consumers read).  The prologue's GlobLN counts Cin * frames[b] values.
 * Both always run their 256 x 128 kernels, whatever the "at least as many tiles as CUs" gates of their uniform twins say -- a
 * ragged batch has no other kernel to go to: the packed images are required, shapes outside those kernels' limits are refused
 * (srf_pw_conv_pair_ragged_supported; srf_packed_pw_weight_bytes != 0 and Cin >= 128 for the single conv, at least 8 tiles).
 *   srf_pw_conv_packed_ragged  forms: no prologue or GlobLN, no residual (out_sums allowed); GlobLN + PReLU with residual
 *                              (no out_sums).  No mask epilogue.  Every tile is computed.
 *   srf_pw_conv_pair_ragged    forms: GlobLN (no residual), GlobLN + PReLU (residual required).  One 128-column tile per
 *                              block; a tile that starts at or past its example's end stores its zeros of y2 and returns
 *                              before any load or MFMA -- this is where a ragged batch does less work than a padded one. */
int srf_pw_conv_packed_ragged(const float* x, const float* w, const void* w_packed, const float* bias, float* y,
                              int Bt, int Cin, int Cout, int L, const srf_norm* in_norm, const float* residual,
                              double* out_sums, int epilogue_mask, const float* mul, int mul_channels, const int* frames,
                              void* stream);
/* GroupComm's per-group convolutions over a ragged batch (the thin-shape kernel; 16 -> 32 and 32 -> 16 channels, L % 4 == 0,
 * frames[b] % 4 == 0; srf_pw_conv_small_ragged_supported).  x, y, residual, pre_q, pre_u: [rows, channels, L] with
 * rows = examples * rows_per_example; frames: one entry per EXAMPLE.  Two forms:
 *   pre-add (proj_1x1)   pre_q, pre_norm {sums, gamma, beta}, pre_u and out_sums given; no in_norm, no residual.
 *                        u = x + GlobLN(pre_q) with count Cin * frames, written to pre_u for the example's own columns only
 *                        (unspecified past them: the block's residual); y = W u + bias stored as exact 0 from the example's
 *                        end to L; out_sums over the example's own columns.  A wavefront wholly past the end stores its zeros
 *                        without loading anything.
 *   residual (res_conv)  in_norm {sums, gamma, beta, prelu} (count Cin * frames) and residual given; no out_sums, no pre_*.
 *                        y is written for the example's own columns only (the block stream). */
int srf_pw_conv_small_ragged_supported(int Cin, int Cout, int L);
int srf_pw_conv_small_ragged(const float* x, const float* w, const float* bias, float* y, int rows, int Cin, int Cout, int L,
                             const srf_norm* in_norm, const float* residual, double* out_sums, const float* pre_q,
                             const srf_norm* pre_norm, float* pre_u, const int* frames, int rows_per_example, void* stream);
int srf_pw_conv_pair_ragged_supported(int Cin1, int Cmid, int Cout2, int L);
int srf_pw_conv_pair_ragged(const float* x, const void* w1_packed, const float* bias1, float* y, const srf_norm* in_norm,
                            const float* residual, const void* w2_packed, const float* bias2, float* y2, double* out_sums2,
                            int Bt, int Cin1, int Cmid, int Cout2, int L, const int* frames, void* stream);

/* The same GEMM in the exact-fp32 class for the training forward.  Round 4 (default): TWO FP16 parts per operand (22 mantissa
 * bits, three MFMAs per product block, the inference kernel's speed; range: |operand| < 65520 -- beyond it, and for NaN / inf operands,
 * the affected outputs are non-finite (round 5: no silent clamp), the remedy is flag 16384).  Debug flag 16384:
 * round 3's form, THREE bf16 parts per operand (h + m + l = 24 mantissa bits) and six MFMAs per product block: results in
 * the exact-fp32 class (what srf_forward_train needs: the two-part kernel's 2^-17 representation error is amplified by the
 * early layers' gradients) at ~1.6 x the two-part kernel's time.  Weights packed by srf_pack3_pw_weights (bytes:
 * srf_packed3_pw_weight_bytes, 0 = shape not taken).  No mask epilogue; residual only together with a GlobLN + PReLU
 * prologue (the res_conv form).  w_packed3 = NULL or a shape / launch size the kernel does not take: exactly srf_pw_conv. */
size_t srf_packed3_pw_weight_bytes(int Cout, int Cin);
int srf_pack3_pw_weights(const float* const* w, void* const* packed, const int* Cout, const int* Cin, int n, void* stream);
/* The library remembers, per (device, address), in which of the two forms a packed3 image was written (so that a launch under
 * the other setting of flag 16384 is refused instead of reading a foreign layout).  A pack replaces every record its extent
 * overlaps; srf_pack3_forget drops the record of a buffer the caller frees or re-uses for other data (ABI 15). */
void srf_pack3_forget(const void* packed);
int srf_pw_conv_packed3(const float* x, const float* w, const void* w_packed3, const float* bias, float* y, int Bt, int Cin,
                        int Cout, int L, const srf_norm* in_norm, const float* residual, double* out_sums, void* stream);
/* The fused pair of the training forward (ABI 14): srf_pw_conv_pair on the two-fp16-part images -- y and y2 BIT-IDENTICAL to
 * srf_pw_conv_packed3(x -> y) followed by srf_pw_conv_packed3(y -> y2, out_sums2).  w1_packed3 / w2_packed3: buffers written by
 * srf_pack3_pw_weights in this process under the default (fp16) form -- it keeps the paired-block layout of the same parts in
 * the buffer's second half.  in_norm required (GlobLN: no residual; GlobLN + PReLU: residual required). */
int srf_pw_conv_pair_packed3_supported(int Bt, int Cin1, int Cmid, int Cout2, int L);
int srf_pw_conv_pair_packed3(const float* x, const void* w1_packed3, const float* bias1, float* y, const srf_norm* in_norm,
                             const float* residual, const void* w2_packed3, const float* bias2, float* y2, double* out_sums2,
                             int Bt, int Cin1, int Cmid, int Cout2, int L, void* stream);

/* Depthwise k=5, padding 2: y[r,j] = bias[c] + sum_k w[c,k] * f(x[r, stride*j+k-2]), r=(b,c), zero
 * outside AFTER f (the reference pads the normalised tensor).  x: [Bt,C,Lin], y: [Bt,C,Lout],
 * Lout = (Lin-1)/stride + 1. */
int srf_dwconv5(const float* x, const float* w, const float* bias, float* y,
                int Bt, int C, int Lin, int stride, const srf_norm* in_norm, double* out_sums,
                void* stream);

/* General Conv1d (round 6, ABI 15): any kernel size / stride / dilation / zero padding / groups, weights [Cout, Cin/groups, K]
 * (nn.Conv1d layout), bias nullable; y: [Bt, Cout, Lout], Lout = (Lin + 2 padding - dilation (K - 1) - 1) / stride + 1.
 * Not on the model's path (that builds kSize 1 and depthwise k = 5 only): it serves the reference's building blocks
 * ConvNormAct / DilatedConvNorm (improved_sudormrf.py:50-73,:138-159) when a user instantiates them with other shapes.
 * out_sums (nullable): [Bt][SRF_STAT_BUCKETS][2] += {sum, sumsq} of y. */
int srf_conv1d(const float* x, const float* w, const float* bias, float* y, int Bt, int Cin, int Cout, int Lin, int K,
               int stride, int padding, int dilation, int groups, double* out_sums, void* stream);

/* Bottom-up nearest-x2 upsample-and-add of D normalised levels:
 * y[b,c,j] = n_0[j] + (n_1[j>>1] + (... + n_{D-1}[j>>(D-1)])),  n_k = GlobLN_k(levels[k]).
 * levels[k]: [Bt,C,L>>k]; norms[k] describes level k (prelu ignored). */
int srf_merge(const float* const* levels, const srf_norm* norms, int D, float* y,
              int Bt, int C, int L, double* out_sums, void* stream);

/* Fused depthwise pyramid of one U-ConvBlock (all D depthwise convs + their GlobLNs + the upsample/add
 * merge) in two passes over y1: y1 [groups,C,L] = proj_1x1 conv output (in_norm = its GlobLN + PReLU,
 * applied on load) -> merged [groups,C,L] (+ out_sums for final_norm).  w/bias/gamma/beta: D pointers
 * each (spp_dw[k].conv.weight/.bias, spp_dw[k].norm.gamma/.beta).  Equivalent to D x srf_dwconv5 +
 * srf_merge but moves 3 C*L instead of 7.75 C*L through HBM.  srf_pyramid_supported() tells whether
 * the shape qualifies (L % (4*2^(D-1)) == 0, L >> (D-1) >= 8, row fits LDS).  merged must NOT alias y1
 * (pass 2 re-reads y1 with halos while other wavefronts write merged). */
int srf_pyramid_supported(int C, int L, int D);
size_t srf_pyramid_scratch_bytes(int groups, int C, int L, int D);
int srf_pyramid(const float* y1, float* merged, const srf_norm* in_norm, const float* const* w,
                const float* const* bias, const float* const* gamma, const float* const* beta, int groups,
                int C, int L, int D, void* scratch, double* out_sums, void* stream);

/* srf_pyramid over a ragged batch (register-resident kernels only: L % 16 == 0 for D <= 5, L % 32 == 0 for D = 6).  y1 must be
 * finite inside every example (what lies past frames[g] is not read); merged is written over the whole row stride, exact zeros
 * from frames[g] on; out_sums and every level's GlobLN count the example's own C * (frames[g] >> k) values.
 * srf_pyramid_ragged_frames_ok: whether one example may be `frames` long -- frames <= L, a multiple of 2^(D-1) and of the
 * kernels' chunk (16 / 32), at least 4 chunks and 8 positions on the deepest level (the finalize step needs distinct edges).
 * Scratch: srf_pyramid_scratch_bytes(groups, C, L, D), as for srf_pyramid. */
int srf_pyramid_ragged_frames_ok(int frames, int L, int D);
int srf_pyramid_ragged(const float* y1, float* merged, const srf_norm* in_norm, const float* const* w,
                       const float* const* bias, const float* const* gamma, const float* const* beta, int groups,
                       int C, int L, int D, void* scratch, double* out_sums, const int* frames, void* stream);
/* The same over folded rows: groups = examples * groups_per_example, every group a GlobLN group of its own with C channels
 * (GroupComm: C = in_channels / G), frames: one entry per EXAMPLE.  srf_pyramid_ragged is groups_per_example = 1. */
int srf_pyramid_ragged_rows(const float* y1, float* merged, const srf_norm* in_norm, const float* const* w,
                            const float* const* bias, const float* const* gamma, const float* const* beta, int groups,
                            int C, int L, int D, void* scratch, double* out_sums, const int* frames, int groups_per_example,
                            void* stream);

/* ---- Causal SuDORMRF (ABI 16; causal_improved_sudormrf_v3.py) ----
 * srf_causal_encoder: out[b,n,l] = sum_{a, k<K} w[n,a,k] * x[b,a, h*l+k-2h], h = K/2, w: [N, A, 2K-1] (the stored
 *   ScaledWSConv1d weight; taps K..2K-2 are masked in the reference and never read here).  Samples outside [0,T) are 0.
 * srf_causal_dwconv: one spp_dw level, y[r,j] = PReLU_out(bias[c] + sum_{k<=10} w[c,k] * f(x[r, stride*j-10+k])),
 *   r = (b,c), w: [C,1,21] (taps 11..20 never read), f = PReLU_in (in_prelu: [1] slope, NULL = identity), zero left of 0
 *   after f; out_prelu NULL = no activation.  x: [Bt,C,Lin], y: [Bt,C,(Lin-1)/stride+1], y must not alias x.
 * srf_causal_merge: y[r,j] = l_0[j] + (l_1[j>>1] + (... + l_{D-1}[j>>(D-1)])), levels[k]: [Bt,C,L>>k].
 * srf_causal_pyramid: the whole pyramid of one UConvBlock in ONE launch: levels = D x srf_causal_dwconv (level 0 from y1
 *   with in_prelu = proj_1x1's PReLU, stride 1; level k from level k-1, stride 2; each with its own bias and PReLU), then
 *   srf_causal_merge -- bit-identical to that sequence, but y1 is read once and merged written once.  w / bias / prelu:
 *   D pointers each (spp_dw[k].conv.weight / .bias, spp_dw[k].act.weight).  merged must NOT alias y1.
 *   srf_causal_pyramid_supported: the shapes it takes (1 <= D <= 8, L % 2^(D-1) == 0). */
int srf_causal_encoder(const float* wav, const float* w, float* out, int Bt, int A, int T, int N, int K, int L, void* stream);
int srf_causal_dwconv(const float* x, const float* w, const float* bias, const float* in_prelu, const float* out_prelu,
                      float* y, int Bt, int C, int Lin, int stride, void* stream);
int srf_causal_merge(const float* const* levels, int D, float* y, int Bt, int C, int L, void* stream);
int srf_causal_pyramid_supported(int C, int L, int D);
int srf_causal_pyramid(const float* y1, float* merged, const float* in_prelu, const float* const* w,
                       const float* const* bias, const float* const* prelu, int Bt, int C, int L, int D, void* stream);
/* dst = src * dscale[0] * hscale (dscale: a DEVICE scalar, NULL = 1) -- the skipinit_gain * alpha / 1 / beta folding.
 * srf_prelu_apply: y = PReLU_a(x), slope[0] on the device (a stand-alone nn.PReLU).  n elements, y may alias x. */
int srf_causal_scale(const float* src, float* dst, long n, const float* dscale, float hscale, void* stream);
int srf_prelu_apply(const float* x, const float* slope, float* y, long n, void* stream);

/* ---- Training the causal model (opt-in, additive to ABI 19) ----
 * srf_causal_forward_train: the forward of srf_forward for a causal plan with its 1x1 convolutions in the exact-fp32 class
 *   (as srf_forward_train, under the same diagnostics switches), keeping in `saved`: encoder output, residual stream
 *   x_0..x_U, per block proj_1x1's PRE-activation u, the D PRE-activations d_k of the pyramid and merged, and mask_net's output.
 * srf_causal_backward: grad_out [Bt, S*A, T] -> every parameter gradient, WRITTEN to grads[i] (same order and shapes as params,
 *   the masked taps of the encoder / depthwise weights as 0); skipinit_gain is read on the device; alpha / beta of
 *   srf_plan_set_block_scales are honoured.  No gradient w.r.t. wav.
 * saved / scratch: 256-byte aligned, srf_causal_train_saved_bytes / _scratch_bytes (0 for a non-causal plan); `saved` stays
 *   untouched between the two calls, `scratch` may be reused in between.  Caller's stream, no host synchronisation; refusals
 *   (non-causal plan, null pointer, wrong num_params, short or misaligned buffer, L % 4 != 0) return SRF_EINVAL before the
 *   first launch.
 * Kernel level.  u = proj_1x1's pre-activation, d_k = level k's, a_k = PReLU_k(d_k) (a_p = PReLU_p(u)), live taps t = 0..10:
 * srf_causal_dwconv_bwd: ONE level.  G[i] = pairwise-tree sum of g_pool[i * 2^shift .. (i + 1) * 2^shift) (g_pool NULL: 0)
 *     + sum_t w_next[c, t] g_next[n], n = i + 10 - t (next_stride 1) or (i + 10 - t) / 2 where even (next_stride 2), n < Lnext
 *     (g_next NULL: none; Lnext = Lout / next_stride);   gd = G * (d > 0 ? 1 : slope)  -- an exact 0 takes the slope, as torch;
 *   dslope[0] = sum G min(d, 0);  with xin (the conv's input BEFORE its PReLU in_slope, [Bt, C, Lout * stride]):
 *   dbias[c] = sum gd, dw[c, t] = sum_j gd[j] PReLU(xin[stride j - 10 + t]) (0 left of the row), dw[c, 11..20] = 0.
 *   xin NULL (proj_1x1's PReLU: d = u, g_next = gd_0, next_stride 1): dw, dbias NULL.  Outputs are written; gd aliases no input.
 * srf_causal_pyramid_bwd: all D levels and proj_1x1's PReLU of one block in one launch + the finalize launches: g_merged, u, gu
 *   [Bt, C, L], d[k] [Bt, C, L >> k]; w / prelu: spp_dw[k].conv.weight / .act.weight, in_prelu: proj_1x1.act.weight; dw[k]
 *   [C, 21], dbias[k] [C], dslope[k] [1], dslope_in [1].  gu is BIT-IDENTICAL to the D + 1 srf_causal_dwconv_bwd calls.  Tiles of
 *   srf_causal_pyramid_bwd_tile() level-0 frames; _supported: 1 <= D <= 8, L % 2^(D-1) == 0.
 * scratch (any float-aligned address): srf_causal_dwconv_bwd_scratch_bytes / srf_causal_pyramid_bwd_scratch_bytes: one record of
 *   partial sums per (row, chunk or tile), added in index order by the finalize launch -- no atomics, same inputs same bits. */
size_t srf_causal_train_saved_bytes(const srf_plan* plan);
size_t srf_causal_train_scratch_bytes(const srf_plan* plan);
int srf_causal_forward_train(const srf_plan* plan, const float* const* params, int num_params, const float* wav, float* out,
                             void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes, void* stream);
int srf_causal_backward(const srf_plan* plan, const float* const* params, float* const* grads, int num_params, const float* wav,
                        const float* grad_out, const void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes,
                        void* stream);
size_t srf_causal_dwconv_bwd_scratch_bytes(int Bt, int C, int Lout);
int srf_causal_dwconv_bwd(const float* g_pool, int shift, const float* g_next, const float* w_next, int next_stride,
                          const float* d, const float* slope, const float* xin, const float* in_slope, int stride, float* gd,
                          float* dw, float* dbias, float* dslope, int Bt, int C, int Lout, void* scratch, void* stream);
int srf_causal_pyramid_bwd_tile(void);
int srf_causal_pyramid_bwd_supported(int C, int L, int D);
size_t srf_causal_pyramid_bwd_scratch_bytes(int Bt, int C, int L, int D);
int srf_causal_pyramid_bwd(const float* g_merged, const float* u, const float* const* d, const float* in_prelu,
                           const float* const* w, const float* const* prelu, float* gu, float* const* dw, float* const* dbias,
                           float* const* dslope, float* dslope_in, int Bt, int C, int L, int D, void* scratch, void* stream);

/* ---- Streaming inference for the causal model (ABI 17) ----
 * A session serves `batch` independent streams of one causal config.  A push takes the next n samples of every stream,
 * n a positive multiple of the granule g = h * 2^(D-1) (h = K/2) and at most max_chunk_samples, and returns n separated
 * samples delayed by h: a push that covers samples [pos, pos + n) returns those at [pos - h, pos + n - h).  After a reset the
 * first h returned samples lie at negative time; the caller drops them.  Feeding zeros up to the reference's padded length T'
 * and then srf_stream_flush reproduces srf_forward on the whole signal.  The same samples under ANY chunk schedule give the
 * same bits: no kernel choice or accumulation order depends on n.
 * Caller-owned device buffers, 256-byte aligned; the library allocates nothing and a push never synchronises:
 *   weights_buf  srf_stream_weights_bytes    snapshot made by srf_stream_prepare (skipinit_gain * alpha folded into res_conv
 *                                            on the device, 1/beta into proj_1x1, decoder weight transposed).  Call it again
 *                                            only when the parameters changed.
 *   state        srf_stream_state_bytes =    4 * (align64(batch*A*2h) + align64(U*D*batch*C*10) + align64(batch*S*A*(h+1)))
 *                                            floats: encoder history | the last 10 inputs of every depthwise level | the
 *                                            pending overlap-add tail.  srf_stream_reset zeroes it (row = -1: every stream).
 *   workspace    srf_stream_workspace_bytes  activations of one push.
 * wav: [batch, A, n]; out: [batch, S*A, n]; out_tail: [batch, S*A, h] (the pending samples; the state is left unchanged).
 * srf_stream_num_launches: kernels per push (3 U + 5), all of the families stream_encoder / stream_pw / stream_pyramid /
 * stream_ola.  Every refusal (non-causal config, n <= 0, n % g != 0, n > max_chunk_samples, small or misaligned buffers, row
 * out of range) returns SRF_EINVAL before anything is launched.
 * srf_causal_stream_pyramid: one block's pyramid for a chunk of Lc frames (Lc % 2^(D-1) == 0): y1 / merged [Bt,C,Lc], state:
 * D pointers to [Bt,C,10] holding the last 10 inputs of each level (level 0: after proj_1x1's PReLU), read and then
 * rolled.  Chunk after chunk it is bit-identical to srf_causal_pyramid on the whole sequence.
 *
 * Independent streams (ABI 19).  srf_stream_push runs the session's `batch` streams in lock-step.  srf_stream_push_rows serves
 * ANY subset of them in one push, each with its own number of granules: rows[j] = {slot, n} is a HOST array of m rows,
 * slot = the stream's index in the state (0 .. batch - 1), n = its samples in this push.  Packed operands, with
 * frames_j = n_j / h and col0_j = the sum of the frames of the rows before j:
 *   wav   row j is a contiguous [A, n_j] block at float offset A * h * col0_j
 *   out   row j is a contiguous [S*A, n_j] block at float offset S*A * h * col0_j
 * (for equal n these are the [m, A, n] / [m, S*A, n] tensors of srf_stream_push).  The state layout is the one above, addressed
 * by slot; slots that are not listed are neither read nor written.  The rows travel to the encoder, pyramid and overlap-add
 * kernels as a kernel argument, SRF_STREAM_ROWS_PER_LAUNCH at a time: there is no device-side table, and a push still allocates
 * nothing on the device, copies nothing and never synchronises.  Those three kernels go out once per group of rows, the 1x1
 * GEMMs once over all columns: srf_stream_push_rows_num_launches(s, m) = 2 U + 3 + ceil(m / 128) * (U + 2) (= 3 U + 5 up to 128
 * rows), same four families.  Every stream gets bit for bit what a batch-1 session of its own would have returned.
 * Refused with SRF_EINVAL before anything is launched: m < 1 or m > batch, a slot outside 0 .. batch - 1, the same slot twice
 * (two rows would race on one state), n_j <= 0, n_j % g != 0, n_j > max_chunk_samples, a small or misaligned buffer, a null
 * pointer.  The session's workspace is large enough for any accepted push.
 * srf_stream_flush_rows: out_tail [m, S*A, h] = the pending samples of slots[0 .. m) (a HOST array); the state is unchanged. */
#define SRF_STREAM_ROWS_PER_LAUNCH 128
typedef struct srf_stream srf_stream;
typedef struct { int slot; int n; } srf_stream_row;
int srf_stream_create(const srf_config* cfg, int batch, int max_chunk_samples, srf_stream** out);
void srf_stream_destroy(srf_stream* s);
int srf_stream_granule(const srf_stream* s);
int srf_stream_delay(const srf_stream* s);
size_t srf_stream_state_bytes(const srf_stream* s);
size_t srf_stream_weights_bytes(const srf_stream* s);
size_t srf_stream_workspace_bytes(const srf_stream* s);
int srf_stream_num_launches(const srf_stream* s);
int srf_stream_set_block_scales(srf_stream* s, const float* alpha, const float* beta, int n);
int srf_stream_prepare(const srf_stream* s, const float* const* params, int num_params, void* weights_buf, void* stream);
int srf_stream_reset(const srf_stream* s, void* state, int row, void* stream);
int srf_stream_push(const srf_stream* s, const void* weights_buf, void* state, const float* wav, int n, float* out,
                    void* workspace, size_t workspace_bytes, void* stream);
int srf_stream_flush(const srf_stream* s, const void* state, float* out_tail, void* stream);
int srf_stream_push_rows(const srf_stream* s, const void* weights_buf, void* state, const srf_stream_row* rows, int m,
                         const float* wav, float* out, void* workspace, size_t workspace_bytes, void* stream);
int srf_stream_flush_rows(const srf_stream* s, const void* state, const int* slots, int m, float* out_tail, void* stream);
int srf_stream_push_rows_num_launches(const srf_stream* s, int m);
int srf_causal_stream_pyramid(const float* y1, float* merged, float* const* state, const float* in_prelu,
                              const float* const* w, const float* const* bias, const float* const* prelu, int Bt, int C, int Lc,
                              int D, void* stream);

/* Transposed conv synthesis + crop: out[b,o,t] = sum_{ci,l,k: h*l+k-h=t} v[b,ci,l]*w[ci,o,k], t<T.
 * v: [Bt,Ci,L], w: [Ci,Co,K] (ConvTranspose1d layout), out: [Bt,Co,T].
 * scratch: device buffer of srf_decoder_scratch_floats() floats, 16-byte aligned (the decoder zero-fills a part of it with
 * 16-byte stores; an unaligned scratch is rejected with SRF_EINVAL). */
size_t srf_decoder_scratch_floats(int Bt, int Ci, int Co, int K, int L);
int srf_decoder(const float* v, const float* w, float* out, int Bt, int Ci, int Co, int K, int L, int T,
                float* scratch, void* stream);

/* TAC up to (not including) TAC_norm: q[b,g,:,l] = PReLU(Wo [z_g ; PReLU(Wm mean_g z_g + bm)] + bo),
 * z_g = PReLU(Wi x[b,g,:,l] + bi).  x,q: [Bt,G,n,L].  params: the 9 TAC tensors in state_dict order
 * (TAC_input.0.weight/.bias, TAC_input.1.weight, TAC_mean.0.weight/.bias, TAC_mean.1.weight,
 * TAC_output.0.weight/.bias, TAC_output.1.weight).  out_sums: [Bt*G][SRF_STAT_BUCKETS][2]. */
int srf_tac(const float* x, float* q, const float* const* params, int Bt, int G, int n, int H, int L,
            double* out_sums, void* stream);
/* srf_tac over a ragged batch: the MFMA kernel only (n = 16, H = 48, G = 16, 16-byte aligned x / q; anything else is refused
 * before a launch).  TAC is pointwise in time, so x past an example's end is never interpreted (it may hold NaN); q is stored
 * as exact 0 from frames[b] to L -- per column: a 32-column tile may straddle the end -- and out_sums run over the example's
 * own columns (the consumer's count is n * frames[b]).  A tile wholly past the end stores zeros without loads or MFMAs. */
int srf_tac_ragged(const float* x, float* q, const float* const* params, int Bt, int G, int n, int H, int L,
                   double* out_sums, const int* frames /* host, [Bt] */, void* stream);

/* pr + w * (mix - sum_s pr), uniform weights (w = 1/S).  pr,out: [Bt,S,T], mix: [Bt,1,T]. */
int srf_mixture_consistency(const float* pr, const float* mix, float* out, int Bt, int S, int T,
                            void* stream);

/* The 'magsq' variant (mixture_consistency.py:26-28): w[b,s] = mean_t pr[b,s]^2 / (sum_s mean_t pr[b,s]^2 + 1e-9).
 * work: Bt*S floats of device scratch (receives the per-source energies). */
int srf_mixture_consistency_magsq(const float* pr, const float* mix, float* out, int Bt, int S, int T, float* work,
                                  void* stream);

/* Caller-side pre/post-processing that every user of the reference wraps around model() (README.md:100-114,
 * experiments/simple_whamr_evaluation.py:142-148):
 *   srf_wav_normalize:   out = (wav - mean) / (std + 1e-9) per row, std unbiased (torch.std default);
 *                        stats[row] = {mean, std}.  wav,out: [rows,T].
 *   srf_wav_denormalize: out = est * std + mean; with mix_norm != NULL additionally
 *                        mixture_consistency.apply(out, mix_norm) (uniform), as the README prescribes for the
 *                        GroupComm models.  est,out: [Bt,S,T]; stats: [Bt][2]; mix_norm: [Bt,1,T]. */
int srf_wav_normalize(const float* wav, float* out, float* stats, int rows, int T, void* stream);
int srf_wav_stats(const float* wav, float* stats, int rows, int T, void* stream);   /* the statistics alone */
int srf_wav_denormalize(const float* est, const float* stats, const float* mix_norm, float* out, int Bt, int S,
                        int T, void* stream);

/* ---- training loss: clamp(PITLossWrapper(PairwiseNegSDR("sisdr"), pit_from='pw_mtx'), +-clamp)
 * reference: losses/sisdr.py:426-458 (pairwise SI-SDR), :254-311,:342-387 (PIT), runner clamp
 * experiments/run_improved_sudormrf.py:169-171.  est, tgt, grad_est: [Bt,S,T]; S <= 9 -- the reference's own limit
 * (sisdr.py:275); 1..4 sources on the streaming kernels, 5..9 on the generic ones (S! permutations per example).
 *   work  : srf_pit_sisdr_work_bytes(Bt,S) bytes, 8-byte aligned, written by _forward and read by _backward;
 *   pw    : optional [Bt,S,S] pairwise losses (estimate, target);
 *   loss  : 2 floats {clamp(batch mean), raw batch mean}; clamp <= 0 disables the clamp;
 *   srf_pit_sisdr_match: [Bt,S] int32, the estimate matched with target j (best permutation);
 *   _backward: grad_est = upstream[0] * d loss[0] / d est (zero when the raw mean is outside +-clamp);
 *              upstream is a DEVICE scalar (NULL = 1), so an autograd chain never synchronises. */
size_t srf_pit_sisdr_work_bytes(int Bt, int S);
int srf_pit_sisdr_forward(const float* est, const float* tgt, int Bt, int S, int T, float clamp, void* work,
                          float* pw, float* loss, void* stream);
/* The other PairwiseNegSDR configurations (losses/sisdr.py:418-424,440-458): sdr_type 0 = "sisdr", 1 = "sdsdr",
 * 2 = "snr"; zero_mean / take_log as the constructor flags.  srf_pit_sisdr_forward == (0, 1, 1).  Same work buffer,
 * srf_pit_sisdr_match / _backward apply unchanged. */
int srf_pit_sdr_forward(const float* est, const float* tgt, int Bt, int S, int T, float clamp, int sdr_type,
                        int zero_mean, int take_log, void* work, float* pw, float* loss, void* stream);
int srf_pit_sisdr_match(const void* work, int Bt, int S, int* match_out, void* stream);
int srf_pit_sisdr_backward(const float* est, const float* tgt, int Bt, int S, int T, float clamp, const void* work,
                           const float* loss, const float* upstream, float* grad_est, void* stream);

/* ---- validation metric of the runners: PermInvariantSISDR.forward (losses/sisdr.py:66-196; constructed at
 * experiments/run_improved_sudormrf.py:82-85, called :201-205).  pr, tgt: [Bt,S,T], mix: [Bt,1,T] or NULL; S <= 9.
 *   best      [Bt]    max over permutations (itertools order) of the source-mean SI-SNR in dB, eps as the class
 *                     places it: s = <p,t>/(<t,t>+eps) t, 10 log10(<s,s>/(<p-s,p-s>+eps));
 *   best_perm [Bt]    index of that permutation in itertools.permutations(range(S)) (first maximum);
 *   base      [Bt*S]  optional (needs mix): SI-SNR of the mixture against every target -- the class subtracts
 *                     mean(base) over batch AND sources from `best` when improvement=True;
 *   zero_mean         subtract the time mean of every signal first (perform_zero_mean);
 *   work              srf_perm_inv_sisdr_work_bytes(Bt,S) bytes, 8-byte aligned. */
size_t srf_perm_inv_sisdr_work_bytes(int Bt, int S);
int srf_perm_inv_sisdr(const float* pr, const float* tgt, const float* mix, int Bt, int S, int T, int zero_mean,
                       double eps, void* work, float* best, int* best_perm, float* base, void* stream);
/* The class as a TRAINING loss (experiments/run_sudormrf.py:56-62,125-128 constructs it with backward_loss=True): the gradient of
 * `best` w.r.t. the estimates with the class's own eps placement, from the `work` and `best_perm` the forward call above left
 * (same Bt, S, T, zero_mean, eps): grad_pr[b] = upstream[b] * d best[b] / d pr[b]; upstream: [Bt] on the device; grad_pr
 * [Bt,S,T], every element written, must not be pr or tgt.  The improvement baseline does not depend on the estimates. */
int srf_perm_inv_sisdr_backward(const float* pr, const float* tgt, int Bt, int S, int T, int zero_mean, double eps,
                                const void* work, const int* best_perm, const float* upstream, float* grad_pr, void* stream);

/* ---- The FUSS recipe (ABI 18; experiments/run_fuss_separation.py) ----
 * Training loss PermInvariantSNRwithZeroRefs (losses/snr.py:13-142): up to 4 sources of which any number may be silent.
 * Per example, with M = |sum_j t_j|^2, P_j = |t_j|^2, active_j = [10 log10(P_j / (M + eps)) >= threshold_db],
 * n_act = sum_j active_j and stab_j = thresh (active_j ? P_j : M):
 *   term(i, j) = 10 active_j log10((P_j + eps) / (|e_i - t_j|^2 + stab_j + eps) + eps)
 *   values[b]  = max over permutations (itertools order, first maximum) of n_act sum_j term(perm(j), j)
 *   loss[0]    = -mean_b values[b];  best_perm[b] = index of the maximising permutation in itertools.permutations(range(S)).
 * est, tgt, grad_est: [Bt,S,T] float32; zero_mean subtracts every row's time mean first.  S = 1..4 ONLY: S > 4 is refused
 * with SRF_EINVAL and a message naming the limit before anything is launched (FUSS's maximum; the sums of one example live
 * in registers).  Any T >= 1; rows are read with 16-byte loads when T % 4 == 0 and the bases are 16-byte aligned.
 *   work: srf_zeroref_snr_work_bytes(Bt,S,T) bytes, 8-byte aligned, written by _forward and read by _backward.  Every block
 *         of the streaming pass writes its partial sums there and the finalize launch adds them in block order: the same
 *         inputs give the same bits on every run.  No allocation, no memset, no host synchronisation; 2 launches.
 *   _backward (1 launch): grad_est is OVERWRITTEN completely; an estimate matched with an inactive target gets exact zeros.
 *         upstream is a DEVICE pointer (NULL = 1): upstream_per_example == 0 -> one scalar, grad = upstream[0] d loss[0] / d est;
 *         != 0 -> [Bt], grad of example b = upstream[b] d values[b] / d est. */
size_t srf_zeroref_snr_work_bytes(int Bt, int S, int T);
int srf_zeroref_snr_forward(const float* est, const float* tgt, int Bt, int S, int T, int zero_mean, float threshold_db,
                            float thresh, float eps, void* work, float* values, int* best_perm, float* loss, void* stream);
int srf_zeroref_snr_backward(const float* est, const float* tgt, int Bt, int S, int T, const void* work,
                             const float* upstream, int upstream_per_example, float* grad_est, void* stream);
/* Validation metric StabilizedPermInvSISDRMetric.forward (losses/sisdr.py:460-576), fewer targets than estimates allowed:
 * pr [Bt,pr_rows,T], tgt [Bt,n_act,T], 1 <= n_act <= n_est <= 4; pr_rows == n_est, or n_est == 1 and the pr_rows <= 4 rows are
 * summed into the one estimate (single_source).  rho^2(i,j) = <p_i,t_j>^2 / (|p_i|^2 |t_j|^2 + eps);
 * value(i,j) = 10 log10((rho^2 + eps) / (1 - rho^2 + eps)); values[b] = max over itertools.permutations(range(n_est), r = n_act)
 * (first maximum; best_perm[b] = its index) of the mean over the targets; improvement != 0 subtracts the batch-and-source mean
 * of value(sum of the targets, t_j).  work: srf_stab_sisdr_work_bytes(Bt,T), 8-byte aligned.  2 launches, deterministic. */
size_t srf_stab_sisdr_work_bytes(int Bt, int T);
int srf_stab_sisdr(const float* pr, const float* tgt, int Bt, int pr_rows, int n_est, int n_act, int T, int zero_mean,
                   int improvement, double eps, void* work, float* values, int* best_perm, void* stream);
/* online_augment (run_fuss_separation.py:195-215) and the loop's mixture normalisation (:237-243):
 *   out[b,k] = clean[src_b[src_s[k]][b], src_s[k]] * gain[b,k];  mix[b] = (m - mean(m)) / (std(m) + eps), m = sum_k out[b,k],
 * std unbiased; stats[b] = {mean, std} of m.  clean, out: [B,S,T] (out must not alias clean), mix: [B,T]; src_b [S][B] and
 * src_s [S] int32, gain [B][S] float32, all on the device; S <= 4; scratch: srf_fuss_augment_scratch_bytes(B,T), 8-byte
 * aligned.  2 launches, deterministic. */
size_t srf_fuss_augment_scratch_bytes(int B, int T);
int srf_fuss_augment(const float* clean, const int* src_b, const int* src_s, const float* gain, int B, int S, int T, float eps,
                     float* out, float* mix, float* stats, void* scratch, void* stream);

/* ---- training step, backward kernels (one entry point per kernel for unit parity) ---- */

/* Weight / bias gradient of a pointwise conv y = W f(x) + bias (improved_sudormrf.py:174,196,256-259,268-269):
 *   dw[m,n] = sum_{b,l} g[b,m,l] * f(x[b,n,l]),  dbias[m] = sum_{b,l} g[b,m,l]
 * f = the forward's operand prologue (in_norm: GlobLN statistics of x + gamma/beta and/or PReLU slope; NULL = none).
 * g: [Bt,Cout,L], x: [Bt,Cin,L], dw: [Cout,Cin], dbias: [Cout] or NULL; accumulate != 0 adds to dw / dbias.
 * scratch: srf_pw_wgrad_scratch_bytes(...) bytes.  L % 4 == 0.
 * srf_pw_wgrad_cols: dw is [Cout, dw_cols] and only the first dw_cols <= Cin columns are produced (x rows beyond
 * them are padding, e.g. the decoder's 42 frame rows padded to 64 for the GEMM). */
size_t srf_pw_wgrad_scratch_bytes(int Bt, int Cout, int Cin, int L);
int srf_pw_wgrad(const float* g, const float* x, const srf_norm* in_norm, int Bt, int Cin, int Cout, int L, float* dw,
                 float* dbias, int accumulate, void* scratch, void* stream);
int srf_pw_wgrad_cols(const float* g, const float* x, const srf_norm* in_norm, int Bt, int Cin, int Cout, int L,
                      float* dw, int dw_cols, float* dbias, int accumulate, void* scratch, void* stream);
/* ... and with a row pitch of dw_ld floats (a column block of a wider matrix, e.g. the two halves of TAC_output) */
int srf_pw_wgrad_ld(const float* g, const float* x, const srf_norm* in_norm, int Bt, int Cin, int Cout, int L,
                    float* dw, int dw_cols, int dw_ld, float* dbias, int accumulate, void* scratch, void* stream);

/* TAC backward (groupcomm_sudormrf_v2.py:356-377 under autograd).  x, go, gx: [Bt,G,n,L]; go = gradient w.r.t. the
 * TAC MLP output (before TAC_norm); gx = gradient through the MLP only; params / grads: the 9 TAC tensors as in
 * srf_tac / same shapes, gradients ACCUMULATED into.  n in {2,4,8,16}, G in {2,4,8,16}, L % 4 == 0. */
size_t srf_tac_bwd_scratch_bytes(int Bt, int G, int n, int L);
int srf_tac_bwd(const float* x, const float* go, const float* const* params, float* const* grads, int Bt, int G, int n,
                int H, int L, float* gx, void* scratch, void* stream);

/* GlobLN (+PReLU when norm->prelu) backward (improved_sudormrf.py:30-47, PReLU of ConvNormAct :73 / NormAct :113).
 * gout (+ optional gout2, added on load): gradient w.r.t. the normalised (activated) tensor; x: the GlobLN input;
 * norm: {sums of x, gamma, beta, slope}.  gx (accumulate_gx != 0: added to).  dgamma, dbeta [C], dslope [1] are
 * ACCUMULATED into (NULL = skip).  scratch: srf_gln_bwd_scratch_bytes(groups, C). */
size_t srf_gln_bwd_scratch_bytes(int groups, int C);
int srf_gln_bwd(const float* gout, const float* gout2, const float* x, const srf_norm* norm, int groups, int C, int L,
                float* gx, int accumulate_gx, float* dgamma, float* dbeta, float* dslope, void* scratch, void* stream);

/* Merge backward (improved_sudormrf.py:214-216): g_levels[k][j] = sum of g_merged over the 2^k samples level k was
 * upsampled to, k = 1..D-1 ([rows, L >> k]); level 0's gradient IS g_merged (g_levels[0] is ignored). */
int srf_merge_bwd(const float* g_merged, float* const* g_levels, int D, long rows, int L, void* stream);

/* Depthwise k=5 conv backward (improved_sudormrf.py:138-159,178-189).  gd: [groups,C,Lout] gradient w.r.t. the conv
 * output; xin: [groups,C,Lin] the conv's PRE-prologue input, in_norm its prologue (NULL = identity); gin: gradient
 * w.r.t. the prologue's output (overwritten; NULL = skip); dw [C,5], dbias [C]: ACCUMULATED into (NULL = skip). */
size_t srf_dwconv5_bwd_scratch_bytes(int groups, int C);
int srf_dwconv5_bwd(const float* gd, const float* xin, const srf_norm* in_norm, const float* w, int groups, int C,
                    int Lin, int stride, float* gin, float* dw, float* dbias, void* scratch, void* stream);

/* Mask application v = relu(m) * enc (improved_sudormrf.py:296-298; the inference path fuses it into the mask GEMM)
 * and its backward: gm = gv * enc * [m > 0] (may alias gv), genc (+)= sum_s gv * relu(m).
 * m, v, gv, gm: [Bt, SA*N, L]; enc, genc: [Bt, N, L]. */
int srf_mask_apply(const float* m, const float* enc, float* v, int Bt, int SA, int N, int L, void* stream);
int srf_mask_bwd(const float* gv, const float* m, const float* enc, float* gm, float* genc, int accumulate_genc, int Bt,
                 int SA, int N, int L, void* stream);

/* Stand-alone PReLU backward (mask_net.0, improved_sudormrf.py:268): gx = gout * (x >= 0 ? 1 : a) (may alias gout),
 * dslope[0] += sum gout * x [x < 0] (NULL = skip). */
int srf_prelu_bwd(const float* gout, const float* x, const float* slope, float* gx, float* dslope, long n, void* stream);

/* out[b, r*K + k, l] = src[b, r, hop*l + k - pad] (0 outside [0,T); rows R*K..rows_out-1 are zero).  src: [Bt,R,T],
 * out: [Bt,rows_out,L].  Feeds the encoder's weight gradient and the decoder's backward (:247-251, :272-279). */
int srf_frames_gather(const float* src, float* out, int Bt, int R, int T, int K, int hop, int pad, int L, int rows_out,
                      void* stream);

/* ---- training step (both models; SURVEY.md §8b proposal: srf_forward_train / srf_backward) ----
 * srf_forward_train: the forward of srf_forward, un-fused where the backward needs an intermediate, keeping what
 *   the backward needs in `saved` (srf_train_saved_bytes: GlobLN statistics, encoder output, residual stream,
 *   per block y1 / D levels / merged, mask pre-activation, masked encoding).
 * srf_backward: grad_out [Bt, S, T] -> parameter gradients ACCUMULATED into grads[i] (same order and shapes as
 *   params; the caller zeroes them like optimizer.zero_grad()).  Reference: torch autograd over
 *   SuDORMRF.forward (improved_sudormrf.py:283-301), run_improved_sudormrf.py:167-172.
 * saved / scratch: 256-byte aligned device buffers of srf_train_saved_bytes / srf_train_scratch_bytes; `saved`
 *   must stay untouched between the two calls, `scratch` may be reused by anything in between.  srf_backward and
 *   srf_backward_wav refuse a `saved` or `scratch` off the 256-byte grid (SRF_EINVAL, "256-byte aligned"), as
 *   srf_forward_train does on the same two buffers; before the training entry points shared one entry check they did not look.
 * The backward follows what the srf_forward_train that filled `saved` did (recorded host-side per device and address),
 *   not the kernel mode / debug flags at its own call: when that forward left the level-0 depthwise output out (the fused
 *   backward head re-computes it) and the head cannot run under the current settings, it returns SRF_EINVAL naming both. */
size_t srf_train_saved_bytes(const srf_plan* plan);
size_t srf_train_scratch_bytes(const srf_plan* plan);
int srf_forward_train(const srf_plan* plan, const float* const* params, int num_params, const float* wav, float* out,
                      void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes, void* stream);
int srf_backward(const srf_plan* plan, const float* const* params, float* const* grads, int num_params,
                 const float* wav, const float* grad_out, const void* saved, size_t saved_bytes, void* scratch,
                 size_t scratch_bytes, void* stream);
/* srf_backward plus the gradient w.r.t. the INPUT waveform (ABI 15): grad_wav [Bt, in_audio_channels, T], overwritten --
 * what torch autograd over the reference's forward returns for a mixture that requires grad (improved_sudormrf.py:283-301;
 * the encoder's Conv1d :247-251 transposed, applied to the encoder-output gradient the backward forms anyway). */
int srf_backward_wav(const srf_plan* plan, const float* const* params, float* const* grads, int num_params,
                     const float* wav, const float* grad_out, const void* saved, size_t saved_bytes, void* scratch,
                     size_t scratch_bytes, float* grad_wav, void* stream);

/* On-GPU online remix augmentation of the training loop (experiments/run_improved_sudormrf.py:150-164): new source j
 * of example b = clean[src_b[j][b], src_s[j]] re-scaled to the energy of clean[b, j]; mix = normalize(sum_j),
 * out[:, j] = normalize(new source j), normalize = (x - mean)/(std + eps) with the unbiased std (:127-131).
 * clean, out: [B,S,T] (out must not alias clean), mix: [B,T], src_b: [S][B] and src_s: [S] int32 on the device,
 * S <= 4; scratch: srf_online_remix_scratch_bytes(B, S). */
size_t srf_online_remix_scratch_bytes(int B, int S);
int srf_online_remix(const float* clean, const int* src_b, const int* src_s, int B, int S, int T, float eps, float* mix,
                     float* out, void* scratch, void* stream);

/* Fused clip_grad_norm_ + Adam step over all parameters (run_improved_sudormrf.py:172-176; torch.optim.Adam without
 * amsgrad / weight decay).  tensors: device array of {float* p; const float* g; float* m; float* v; long n;};
 * chunks: device array of {int tensor, int chunk} covering every tensor in srf_opt_chunk_size()-element pieces;
 * buckets: SRF_STAT_BUCKETS doubles of device scratch; step: 1-based step count; max_norm <= 0: no clipping;
 * norm_out: optional device float receiving the total gradient norm before clipping. */
int srf_opt_chunk_size(void);
int srf_clip_adam_step(const void* tensors, const void* chunks, int n_chunks, double* buckets, float max_norm, float lr,
                       float beta1, float beta2, float eps, int step, float* norm_out, void* stream);

/* Input feeder.  Replaces, for this path, the reference's Dataset.__getitem__ + torch DataLoader
 * (dataset_loader/wham.py:171-226): a pool of host threads reads the WAV files of a batch in parallel -- mixture = stream
 * 0, then the sources; one crop start per example, shared by its files (:183-186,:201); float32 values exactly as
 * scipy.io.wavfile.read + torch.tensor(dtype=float32) give them; zero pad to time_samples (:157-166) -- straight into
 * CALLER-OWNED buffers (pinned host memory if the copy to the device is to be asynchronous):
 *   wave [batch][n_streams][time_samples] float32, len [batch][n_streams] int32 (valid samples of every stream: a source
 *   file may be shorter than its mixture), stat [batch][2] float32 = {mean, unbiased std} of the mixture over the range the
 *   reference normalises it on (the crop when it crops, else the whole file: it truncates after normalising, :183-191;
 *   only computed when the feeder was created with normalize != 0).
 * paths: n_items * n_streams file names, item-major.  augment: random crop start when a file is longer than time_samples
 * (splitmix64 of seed, epoch and item: reproducible, unlike the reference's time-seeded numpy generator).  shuffle /
 * drop_last: the DataLoader's (get_generator, :219-224).
 * srf_feeder_submit queues the next batch of the epoch (returns 1, queues nothing, when the epoch is exhausted);
 * srf_feeder_wait blocks until the OLDEST submitted batch is complete and hands its buffers back.  Any number of batches may
 * be in flight.  srf_wav_info / srf_wav_read: the reader on its own (RIFF/WAVE mono, PCM 8/16/24/32, IEEE float 32/64).
 * srf_feeder_create_sharded: the rank-aware form for one process per GPU (the reference feeds its DataParallel replicas
 * from ONE DataLoader and scatters each batch, wham.py:219-226 + run_improved_sudormrf.py:118): every rank builds the same
 * epoch order from (seed, epoch); a GLOBAL batch is batch * world consecutive items of it and this feeder delivers items
 * [rank * batch, (rank + 1) * batch) of every global batch -- disjoint across ranks, their concatenation in rank order is the
 * single-process batch of size batch * world, an epoch covers every item once over all ranks.  world > 1 requires drop_last.
 * normalize = 0 skips the mixture statistics (and the second read of files longer than time_samples they need).
 * srf_feeder_create = the same with normalize 1, rank 0, world 1.  srf_feeder_epoch_items: the items this rank delivers in
 * the current epoch, in order.  srf_feeder_read_example: one example synchronously in the calling thread (Dataset[i]). */
typedef struct srf_feeder srf_feeder;
int srf_wav_info(const char* path, int* rate, int* channels, int* bits, long* frames);
int srf_wav_read(const char* path, long start, long n, float* dst, long* frames);
int srf_feeder_create(const char* const* paths, int n_items, int n_streams, int time_samples, int batch, int n_threads,
                      int augment, int shuffle, int drop_last, unsigned long long seed, srf_feeder** out);
int srf_feeder_create_sharded(const char* const* paths, int n_items, int n_streams, int time_samples, int batch,
                              int n_threads, int augment, int shuffle, int drop_last, unsigned long long seed, int normalize,
                              int rank, int world, srf_feeder** out);
void srf_feeder_destroy(srf_feeder* f);
long srf_feeder_epoch_items(srf_feeder* f, int* items, long capacity);
int srf_feeder_read_example(const char* const* paths, int n_streams, int time_samples, long start, int augment, int normalize,
                            float* wave, int* len, float* stat);
long srf_feeder_batches_per_epoch(const srf_feeder* f);
long srf_feeder_item_frames(const srf_feeder* f, int item);
int srf_feeder_start_epoch(srf_feeder* f, int epoch);
int srf_feeder_submit(srf_feeder* f, float* wave, int* len, float* stat);
int srf_feeder_wait(srf_feeder* f, float** wave, int** len, float** stat, int* n_valid);
/* The Dataset's normalisation on a whole batch, on the device (wham.py:189-217): raw [B][n_streams][T] as delivered by the
 * feeder (len [B][n_streams]) -> mix [B][T], src [B][n_streams-1][T].  normalize = 0: copy; 1: every stream
 * (x - mean)/(std + eps) over ITS OWN valid samples (the mixture with `stat`), zero pad, then (x - mean_T)/(mix_std + eps)
 * with the population std of the padded mixture. */
int srf_feeder_normalize(const float* raw, const int* len, const float* stat, int B, int n_streams, int T, int normalize,
                         float eps, float* mix, float* src, void* stream);

/* ---- Attentive SuDoRM-RF v2 (additive to ABI 19; attentive_sudormrf_v2.py) ----
 * The Improved model with a TransformerLayer on the deepest level of every U-block.  Inference only.
 * srf_attentive_plan_create: base = the Improved model's fields (variant is ignored, in_audio_channels and group_size must be 1);
 *   n_heads / att_dims = the blocks' MHAttentionLayer (H heads of d channels).  The input is padded as the reference pads it, to
 *   a multiple of lcm(K / 2, 2^D) -- not the Improved model's (K / 2) 2^D.  The plan works with srf_forward, srf_separate,
 *   srf_plan_workspace_bytes / _num_params / _frames / _padded_length and the profiler.  Parameters in state_dict() order, per
 *   block: the Improved block's tensors, then mha.{Q,K,V,O}_proj.{weight, bias}, out_norm.{gamma, beta},
 *   out_mha_norm.{gamma, beta}, ffn.conv.{weight, bias}, ffn.norm.{gamma, beta}, ffn.act.weight, pos_enc.pe ([1, 5000, C], read
 *   on the device).  Refused before anything is launched (SRF_EINVAL, the message names the argument): upsampling_depth < 2,
 *   a deepest level of more than SRF_ATT_MAX_LEN or fewer than 1 positions, n_heads / att_dims < 1; srf_forward_train,
 *   srf_backward(_wav) and srf_forward_ragged / srf_separate_ragged refuse such a plan, srf_plan_ragged_supported is 0.
 * srf_mha_attention: softmax attention per (example, head).  q: [Bt, H d, Lq], k, v: [Bt, H d, Lk], o: [Bt, H d, Lq] (WRITTEN),
 *   channel h d + j belongs to head h; o[., h d + j, lq] = sum_lk softmax_lk(scale * <q[., h, lq], k[., h, lk]>) v[., h d + j, lk].
 *   q is scaled before the product, as the reference does.  Any float-aligned address; any Lq, Lk >= 1 (online softmax over key
 *   tiles, the score matrix never reaches memory).  Kernels: the exact-fp32 MFMA form for d % 16 == 0, 16 <= d <= 256
 *   (srf_mha_attention_mfma_supported, kernel modes 0 and 2; profiler name mha_attention_mfma), a VALU form for every other
 *   d <= 1024 (mha_attention_generic).
 * srf_mha_attention_lse: srf_mha_attention that also WRITES lse[Bt, H, Lq] = log sum_lk exp(score), the per-query log-sum-exp
 *   of the scaled scores.  o is bit-identical to srf_mha_attention's; profiler names mha_attention_lse_mfma / _generic.
 * srf_mha_attention_bwd: the gradient of srf_mha_attention.  q, k, v as above, o and lse as srf_mha_attention_lse wrote them for
 *   the same (q, k, v, scale), go: [Bt, H d, Lq] the gradient of o; gq [Bt, H d, Lq], gk, gv [Bt, H d, Lk] are WRITTEN in full
 *   (no accumulation).  P is recomputed from lse: no tensor of size Lq x Lk reaches memory.  workspace: at least
 *   srf_mha_attention_bwd_workspace_bytes(Bt, H, d, Lq, Lk) bytes of device memory at any float-aligned address, the caller's,
 *   contents irrelevant before and after.  Deterministic: no float atomics, every output element is summed by one wavefront in
 *   a fixed order.  Kernels: mha_attention_bwd_delta, then the exact-fp32 MFMA form where
 *   srf_mha_attention_bwd_mfma_supported(d) (the forward's predicate: d % 16 == 0, 16 <= d <= 256, kernel modes 0 and 2):
 *   mha_attention_bwd_dq_mfma + mha_attention_bwd_dkv_mfma (d <= 128) or + mha_attention_bwd_dv_mfma, mha_attention_bwd_dk_mfma
 *   (d > 128: one pass per output); a VALU form for every other d <= 1024 (mha_attention_bwd_dq_generic, _dkv_generic).
 *   Refused before the first launch (SRF_EINVAL, the message names the argument): a null pointer, the workspace included;
 *   sizes < 1; d > 1024 on the VALU form; more than 2^31 elements per example; Bt or H > 65535.  Any Lq, Lk >= 1, independent.
 * srf_mha_attention_ragged, srf_mha_attention_lse_ragged, srf_mha_attention_bwd_ragged (additive; SRF_ABI_VERSION unchanged): the
 *   three calls above over examples of unequal length.  Tensors, layout and workspace are the uniform calls': Lq and Lk stay
 *   the ROW STRIDES; example b owns q_lengths[b] <= Lq queries and k_lengths[b] <= Lk keys.  q_lengths / k_lengths: HOST int
 *   arrays of Bt entries (NULL = every example is full on that side), handed to the kernels by value in the launch arguments:
 *   nothing is uploaded, nothing synchronises, Bt <= SRF_RAGGED_MAX_BATCH.  Per example b:
 *     reads    nothing at queries >= q_lengths[b] (q, go, o, lse) and nothing at keys >= k_lengths[b] (k, v): may hold NaN;
 *     writes   o, lse and gq are exact 0.f at queries >= q_lengths[b] up to Lq, gk and gv exact 0.f at keys >= k_lengths[b] up
 *              to Lk; delta in the workspace is unspecified there;
 *     cost     a block whose whole tile lies at or past the owned side's length stores its zeros and returns before any load;
 *              the loop over the other side runs to that side's own length: work follows sum_b q_lengths[b] k_lengths[b];
 *     bits     inside the lengths, those of the uniform call on example b alone with Lq = q_lengths[b], Lk = k_lengths[b]
 *              (same arithmetic in the same order); deterministic, no float atomics, a masked position has P = 0 by selection.
 *   Dispatch is the uniform predicate (srf_mha_attention_mfma_supported(d) and the kernel mode); profiler names are the uniform
 *   ones + "_ragged".  Refused before the first launch (SRF_EINVAL, the message names the example and the argument): a length
 *   < 1 or above its row stride, Bt > SRF_RAGGED_MAX_BATCH, and everything the uniform call refuses.
 * srf_posenc_apply: x[b, c, l] = norm(a)[b, c, l] + pe[l, c] (norm nullable = identity; prelu ignored); pe: [max_len, C].
 * srf_posenc_apply_dropout: srf_posenc_apply under the PositionalEncoding's dropout (train() mode):
 *   x[b, c, l] = keep(i) ? (norm(a)[b, c, l] + pe[l, c]) * inv_keep : 0.f, i = (b C + c) L + l as a 64-bit index.
 *   keep(i) is a pure function of (seed, offset, i) -- not of the launch geometry, the tile or the device: word i & 3 of
 *   Philox4x32-10 with the key {lo32(seed), hi32(seed)} on the counter {lo32(i >> 2), hi32(i >> 2), lo32(offset), hi32(offset)}
 *   (multipliers 0xD2511F53, 0xCD9E8D57, key increments 0x9E3779B9, 0xBB67AE85), kept where word >= floor(p 2^32); the threshold
 *   is formed on the host in double and compared as a 64-bit number, so p = 1 drops everything.  inv_keep is the host's fp32
 *   1.f / (1.f - p); a dropped element is SELECTED 0.f, never multiplied (p = 1: exact zeros, no inf * 0).  p == 0 runs the plain
 *   kernel (profiler name posenc_apply, srf_posenc_apply's bits); otherwise posenc_apply_dropout.  Refused before the launch
 *   (SRF_EINVAL, the message names the argument): p outside [0, 1] or NaN, a null a / pe / x, and srf_posenc_apply's own limits.
 * srf_posenc_dropout_bwd: gn[i] = keep(i) ? gx[i] * inv_keep : 0.f over i < Bt C L, the mask RECOMPUTED from the forward's
 *   (p, seed, offset), never stored; gn may alias gx.  gn is the gradient w.r.t. norm(a) + pe, which srf_gln_bwd takes as gout.
 * srf_dropout_mask: keep[i] in {0, 1} for i < n, the same function as bytes (tests; a building block for other dropouts).
 * srf_gln_apply2_add: z = fnorm(f) + ynorm(y), each GlobLN (+ PReLU where its prelu is set) from its own statistics;
 *   out_sums (nullable) += {sum, sumsq} of z.  f, y, z: [groups, channels, length] at any float-aligned address. */
#define SRF_VARIANT_ATTENTIVE 3
#define SRF_ATT_MAX_LEN 5000
int srf_attentive_plan_create(const srf_config* base, int n_heads, int att_dims, int batch, int T, srf_plan** out);
int srf_mha_attention_mfma_supported(int d);
int srf_mha_attention(const float* q, const float* k, const float* v, float* o, int Bt, int H, int d, int Lq, int Lk, float scale,
                      void* stream);
int srf_mha_attention_lse(const float* q, const float* k, const float* v, float* o, float* lse, int Bt, int H, int d, int Lq, int Lk,
                          float scale, void* stream);
int srf_mha_attention_bwd_mfma_supported(int d);
size_t srf_mha_attention_bwd_workspace_bytes(int Bt, int H, int d, int Lq, int Lk);
int srf_mha_attention_bwd(const float* q, const float* k, const float* v, const float* o, const float* lse, const float* go,
                          float* gq, float* gk, float* gv, void* workspace, int Bt, int H, int d, int Lq, int Lk, float scale,
                          void* stream);
int srf_mha_attention_ragged(const float* q, const float* k, const float* v, float* o, int Bt, int H, int d, int Lq, int Lk,
                             const int* q_lengths, const int* k_lengths, float scale, void* stream);
int srf_mha_attention_lse_ragged(const float* q, const float* k, const float* v, float* o, float* lse, int Bt, int H, int d, int Lq,
                                 int Lk, const int* q_lengths, const int* k_lengths, float scale, void* stream);
int srf_mha_attention_bwd_ragged(const float* q, const float* k, const float* v, const float* o, const float* lse, const float* go,
                                 float* gq, float* gk, float* gv, void* workspace, int Bt, int H, int d, int Lq, int Lk,
                                 const int* q_lengths, const int* k_lengths, float scale, void* stream);
int srf_posenc_apply(const float* a, const srf_norm* norm, const float* pe, float* x, int Bt, int C, int L, int max_len,
                     void* stream);
int srf_posenc_apply_dropout(const float* a, const srf_norm* norm, const float* pe, float* x, int Bt, int C, int L, int max_len,
                             float p, unsigned long long seed, unsigned long long offset, void* stream);
int srf_posenc_dropout_bwd(const float* gx, float* gn, int Bt, int C, int L, float p, unsigned long long seed,
                           unsigned long long offset, void* stream);
int srf_dropout_mask(unsigned char* keep, long n, float p, unsigned long long seed, unsigned long long offset, void* stream);
int srf_gln_apply2_add(const float* f, const srf_norm* fnorm, const float* y, const srf_norm* ynorm, float* z, double* out_sums,
                       int groups, int channels, int length, void* stream);

/* ---- Attentive SuDoRM-RF v3 (additive to ABI 19; attentive_sudormrf_v3.py) ----
 * The Improved model's front end and tail around blocks WITHOUT an upsample-and-add: the depthwise pyramid's levels are folded
 * from the deepest up by D - 1 ConditionalTransformerLayers ("attentive resamplers": the shallower level asks, the deeper one --
 * with its own position table added -- answers), and final_norm sits on the last one's out_norm.  Inference only.
 * srf_attentive_v3_plan_create: arguments and padding (lcm(K / 2, 2^D)) as srf_attentive_plan_create.  Level k + 1 has
 *   ceil(L_k / 2) positions -- the strided convolution's own arithmetic; no divisibility is asked of the frame count -- and
 *   upsampling_depth = 1 is legal (no resampler: final_norm on spp_dw[0]'s GlobLN).  The plan works with srf_forward,
 *   srf_separate, srf_plan_workspace_bytes / _num_params / _frames / _padded_length and the profiler.  Parameters in state_dict()
 *   order, per block: the Improved block's tensors, then attentive_resamplers.0 .. D-2, each the 18 tensors listed for v2 above
 *   (resampler r asks from level D - 2 - r: resampler 0 serves the DEEPEST pair).  Refused before anything is launched
 *   (SRF_EINVAL, the message names the argument): more than SRF_ATT_MAX_LEN positions on level 1 (the table is added to the
 *   answering side), a level with fewer than 1 position, n_heads / att_dims < 1, in_audio_channels or group_size != 1,
 *   upsampling_depth > 8; srf_forward_train, srf_backward(_wav) and srf_forward_ragged / srf_separate_ragged refuse
 *   such a plan, srf_plan_ragged_supported is 0.
 * srf_gln_apply_stats: y = norm(x), a GlobLN (+ PReLU where norm->prelu is set) from norm->sums; out_sums (nullable) += {sum,
 *   sumsq} of the STORED y in the bucket scheme of every other statistics producer (the moments of an already-normalised tensor,
 *   which a second GlobLN on top needs and which do not follow from x's sums).  x, y: [groups, channels, length] at any
 *   float-aligned address, any length; x and y do not overlap. */
#define SRF_VARIANT_ATTENTIVE_V3 4
int srf_attentive_v3_plan_create(const srf_config* base, int n_heads, int att_dims, int batch, int T, srf_plan** out);
int srf_gln_apply_stats(const float* x, const srf_norm* norm, float* y, double* out_sums, int groups, int channels, int length,
                        void* stream);

/* ---- Attentive block on a ragged batch (additive to ABI 19) ----
 * The ragged forms of the kernels an AttentiveUConvBlock runs besides its GEMMs and the attention: the same kernel templates as
 * their uniform twins with the table behind their arguments (profiler names: the twin's + "_ragged").  Tensors keep the uniform
 * layout, the length argument stays the ROW STRIDE, and example (group) b brings its own count of columns in a HOST table of Bt
 * (groups) ints that travels by value in the launch arguments: no upload, no synchronisation, at most SRF_RAGGED_MAX_BATCH
 * entries.  Every example is treated as its own batch-1 call on its slice would treat it: a GlobLN applied on load counts
 * C * (its own columns), a convolution meets literal zeros at its own end, nothing is read at or past an example's end (it may
 * hold NaN), outputs are exact 0.f from the example's own end to the row stride, and out_sums (where the twin has them;
 * nullable, accumulated in the twin's bucket scheme) run over the example's own columns.  A row's output does not depend on any
 * other row's content, nor on its length while the launch stays on the same kernel (the float4 kernels below serve a launch whose
 * EVERY length lies on their grid; they pre-add a lane's four outputs in fp32 before the fp64 out_sums, the generic ones do not).
 * srf_dwconv5_ragged: in_frames[b] input columns under row stride Lin; for stride 2 Lin and every in_frames[b] are even.  The
 *   output row stride is srf_dwconv5's, the example's own outputs are in_frames[b] / stride.  The float4 kernels serve a launch
 *   whose Lin and every in_frames[b] are multiples of 4 * stride (and 16-byte aligned x, y), the generic kernel any other.
 * srf_merge_ragged: frames[b] level-0 columns, a multiple of 2^(D-1); level k has frames[b] >> k columns under row stride
 *   L >> k and its norm counts C * (frames[b] >> k).  The float4 kernel serves a launch whose L and every frames[b] are multiples
 *   of 4, the generic kernel any other.
 * srf_posenc_apply_ragged: the inference form (no dropout): x[b, c, l] = norm(a)[b, c, l] + pe[l, c] for l < frames[b], the
 *   norm counting C * frames[b]; neither a nor pe is read at l >= frames[b].
 * srf_gln_apply2_add_ragged, srf_gln_apply_ragged: any frames[g] >= 1 (dword accesses throughout); both need the statistics,
 *   gamma and beta of their norm(s).
 * srf_gln_stats_ragged: WRITES sums[g] ([SRF_STAT_BUCKETS][2], srf_gln_stats' layout; no zeroing needed) = {sum, sumsq} over
 *   x[g, :, :frames[g]].  Bucket k holds the rows c = k mod SRF_STAT_BUCKETS, added in a fixed order by the bucket's one block: no
 *   atomics, the same bits on every run, and a group's numbers do not depend on the other groups.
 * srf_sums_scale_ragged: out[g][*] = in[g][*] * (double) L / frames[g], not in place, one launch.  This is the copy a UNIFORM
 *   kernel's on-load norm takes (e.g. srf_pw_conv_packed on a ragged batch): with the count C * L it assumes, the scaled sums
 *   give the mean and variance of the example's own C * frames[g] elements.  Ragged kernels take the unscaled sums.
 * Refused before any launch (SRF_EINVAL, the message names the example): a null table, more than SRF_RAGGED_MAX_BATCH entries,
 *   an entry < 1 or above its row stride, an odd entry (or Lin) under stride 2, a frames[b] that is no multiple of 2^(D-1) in the
 *   merge, and everything the uniform twin refuses. */
int srf_dwconv5_ragged(const float* x, const float* w, const float* bias, float* y, int Bt, int C, int Lin, int stride,
                       const srf_norm* in_norm, double* out_sums, const int* in_frames, void* stream);
int srf_merge_ragged(const float* const* levels, const srf_norm* norms, int D, float* y, int Bt, int C, int L, double* out_sums,
                     const int* frames, void* stream);
int srf_posenc_apply_ragged(const float* a, const srf_norm* norm, const float* pe, float* x, int Bt, int C, int L, int max_len,
                            const int* frames, void* stream);
int srf_gln_apply2_add_ragged(const float* f, const srf_norm* fnorm, const float* y, const srf_norm* ynorm, float* z,
                              double* out_sums, int groups, int channels, int length, const int* frames, void* stream);
int srf_gln_apply_ragged(const float* x, float* y, const srf_norm* norm, int groups, int channels, int length, const int* frames,
                         void* stream);
int srf_gln_stats_ragged(const float* x, double* sums, int groups, int channels, int length, const int* frames, void* stream);
int srf_sums_scale_ragged(const double* in, double* out, int groups, int length, const int* frames, void* stream);
/* 1 where srf_pw_conv_packed_ragged takes (Bt, Cin, Cout, L) with these frames NOW -- the 256 x 128 kernel's shape and reach,
 * kernel mode 0, no debug flag that takes the kernel or the packed images away, 1 <= frames[b] <= L and frames[b] % 4 == 0 --
 * else 0 (no GPU needed; frames on the host).  Left to the call: the forms built, non-null pointers, the 16-byte alignment of x, y,
 * residual and the packed image.  For a caller with another path to take: the attentive block falls back to the uniform GEMM. */
int srf_pw_conv_packed_ragged_supported(int Bt, int Cin, int Cout, int L, const int* frames);

/* ---- Attentive v2 on a ragged batch: the whole model (additive to ABI 19) ----
 * srf_pw_conv_ragged: the ragged form of the 128 x 128 split-bf16 GEMM (profiler name pw_conv_bf16x3_ragged<PRO>), for the 1x1
 *   convolutions the 256 x 128 ragged GEMM does not take: Cout < 192 and lengths off the grid of 4.  It reads the fp32 weight (no
 *   packed image).  L stays the row stride; example b owns columns [0, frames[b]) for ANY 1 <= frames[b] <= L.  A 128-column
 *   tile that starts at or past frames[b] is skipped before any load: y is unspecified there.  In the tile that holds the
 *   example's end, columns >= frames[b] are stored as exact 0.f.  What x and residual hold at columns >= frames[b] (NaN
 *   included) reaches no own column and no statistic; out_sums (nullable, the uniform kernel's buckets) run over own columns;
 *   the norm on load counts Cin * frames[b] against own-column sums (no scaled copy).  Every prologue, with or without
 *   residual and out_sums; no mask epilogue.
 * srf_pw_conv_ragged_supported: 1 under kernel mode 0 for Cin % 64 == 0, Cout >= 32, L % 4 == 0, W and x within the 2 GB reach
 *   of 32-bit offsets, 1 <= Bt <= SRF_RAGGED_MAX_BATCH and every frames[b] in 1..L; else 0.  No GPU needed.
 *   srf_pw_conv_ragged refuses, before any launch and naming the example where there is one, everything the gate refuses, null
 *   pointers and x / w / y / residual / in_norm.sums off the 16-byte grid. */
int srf_pw_conv_ragged_supported(int Bt, int Cin, int Cout, int L, const int* frames);
int srf_pw_conv_ragged(const float* x, const float* w, const float* bias, float* y, int Bt, int Cin, int Cout, int L,
                       const srf_norm* in_norm, const float* residual, double* out_sums, const int* frames, void* stream);
/* The whole attentive v2 model over unequal-length examples in one set of launches.  Opt-in through entry points of its own:
 * srf_plan_ragged_supported stays 0 for an attentive plan and srf_forward_ragged / srf_separate_ragged keep refusing it.  Same
 * contract as those two: out[b, :, :lengths[b]] is what srf_forward (resp. srf_separate) gives for example b alone at its own
 * length (to rounding: the GEMM kernels differ), out[b, :, lengths[b]:] is exact 0, wav[b, :, lengths[b]:] is never read.
 * Every 1x1 convolution is decided per launch: the 256 x 128 packed ragged GEMM, else srf_pw_conv_ragged, else the uniform GEMM
 * over every column between srf_sums_scale_ragged and srf_gln_stats_ragged.
 * srf_attentive_ragged_supported: 1 for a plan of srf_attentive_plan_create with enc_kernel_size = 21 (one audio channel),
 *   batch <= SRF_RAGGED_MAX_BATCH, kernel mode != 1, num_sources * enc_num_basis * frames >= 256 (one slot of scaled sums lives at
 *   the start of the masked tensor's workspace region while the blocks run); with K = 21 every length in 1..T is taken.
 *   Attentive v3 plans: 0.
 * srf_attentive_ragged_workspace_bytes: the workspace the ragged call needs (0 = not supported).
 * Refused with SRF_EINVAL before anything is launched, srf_last_error() naming the example: a length outside 1..T. */
int srf_attentive_ragged_supported(const srf_plan* plan);
size_t srf_attentive_ragged_workspace_bytes(const srf_plan* plan);
int srf_attentive_forward_ragged(const srf_plan* plan, const float* const* params, int num_params, const float* wav,
                                 const int* lengths /* host */, float* out, void* workspace, size_t workspace_bytes, void* stream);
int srf_attentive_separate_ragged(const srf_plan* plan, const float* const* params, int num_params, const float* wav,
                                  const int* lengths /* host */, float* out, float* stats, int mixture_consistency, void* workspace,
                                  size_t workspace_bytes, void* stream);

/* ---- Original SuDoRM-RF (additive to ABI 19; sudormrf.py) ----
 * The model of the paper: an encoder WITH bias and ReLU, GroupNorm(1, C) everywhere (GlobLN's arithmetic), PReLU with one slope
 * PER CHANNEL, blocks whose residual is added before the last norm, a mask layer that is a convolution along the basis axis
 * (a [S N, N] Toeplitz GEMM) followed by a softmax over the sources (sigmoid for one source), and a grouped decoder with bias.
 * One stream; inference through srf_forward / srf_separate, training through the opt-in walk further below.
 * srf_original_plan_create: padding up to a multiple of lcm(K / 2, 2^D), only when T is not one already.  The plan works with
 *   srf_forward, srf_separate (decoder.bias is added before the rescale and mixture consistency), srf_plan_workspace_bytes /
 *   _num_params / _frames / _padded_length / _num_launches, srf_debug_fetch (1: always the separation module's output; 3: the
 *   pre-softmax mask logits [Bt, S N, L]) and the profiler.  Parameters in state_dict() order: encoder.0.{weight, bias},
 *   ln.{weight, bias}, l1.{weight, bias}; per block proj_1x1.{conv.weight, conv.bias, norm.weight, norm.bias, act.weight [C]},
 *   D x spp_dw.k.{conv.weight, conv.bias, norm.weight, norm.bias}, conv_1x1_exp.{conv.weight, conv.bias, norm.weight,
 *   norm.bias}, final_norm.{norm.weight, norm.bias, act.weight [C]}, module_act.{norm.weight, norm.bias, act.weight [B]};
 *   reshape_before_masks.{weight, bias} only when out_channels != enc_num_basis; m.{weight [S, 1, N + 1, 1], bias},
 *   decoder.{weight [S N, 1, K], bias [S]}, ln_mask_in.{weight, bias} (in the state_dict, never read).
 *   Refused before anything is launched (SRF_EINVAL, the message names the argument): odd enc_num_basis (the reference's own
 *   mask multiply fails there: the mask layer then has N + 1 rows), even or < 3 enc_kernel_size, in_audio_channels or group_size
 *   != 1, upsampling_depth outside 1..8, a frame count that is no multiple of 2^(D-1), num_sources above
 *   SRF_SOFTMAX_MASK_MAX_SOURCES, batch > 65535; srf_forward_train, srf_backward(_wav) and srf_forward_ragged /
 *   srf_separate_ragged refuse such a plan, srf_plan_ragged_supported is 0.
 * srf_gln_apply_c: y = norm(x), a GlobLN from norm->sums (norm->prelu is ignored), then PReLU with slopes[c] (nullable: none),
 *   then + add (nullable); out_sums (nullable) += {sum, sumsq} of the STORED y.  x, add, y: [groups, channels, length] at any
 *   float-aligned address, any length; y overlaps neither input.
 * srf_encoder_bias_relu: out = relu(bias[n] + srf_encoder's sum) for one audio channel and any odd K; sums of the stored out;
 *   in_stats (nullable): [Bt][2] {mean, std}, the row is normalised on load as in srf_separate.
 * srf_mask_weight_fill: tz [S N, N], tz[s N + i, n] = mw[s, n - i + N - N / 2] where that tap exists (0 .. N), else 0;
 *   bias_rows [S N] = mb[s] repeated N times.  N even.
 * srf_softmax_mask: v[b, s N + i, l] = p_s(z[b, :, i, l]) * enc[b, i, l]; p = softmax over the S sources (maximum subtracted),
 *   S = 1: the sigmoid.  v may be z.  1 <= S <= SRF_SOFTMAX_MASK_MAX_SOURCES.
 * srf_decoder_weight_expand: the grouped ConvTranspose1d weight w [S N, 1, K] as the block-diagonal wexp [S N, S, K] of an
 *   ungrouped one (zeros written).
 * srf_bias_rescale: out[b, s, t] = est[b, s, t] + bias[s], in place over out [Bt, S, T]; stats (nullable) [Bt][2] {mean, std}
 *   of the raw mixture wav [Bt, T]: then out = (est + bias) * std + mean and, mc != 0, mixture consistency against the
 *   mixture normalised on the fly, exactly as srf_separate's overlap-add does it. */
#define SRF_VARIANT_ORIGINAL 5
#define SRF_SOFTMAX_MASK_MAX_SOURCES 16
int srf_original_plan_create(const srf_config* cfg, int batch, int T, srf_plan** out);
int srf_gln_apply_c(const float* x, const srf_norm* norm, const float* slopes, const float* add, float* y, double* out_sums,
                    int groups, int channels, int length, void* stream);
int srf_encoder_bias_relu(const float* wav, const float* w, const float* bias, float* out, double* sums, int Bt, int T, int N,
                          int K, int L, const float* in_stats, void* stream);
int srf_mask_weight_fill(const float* mw, const float* mb, float* tz, float* bias_rows, int N, int S, void* stream);
int srf_softmax_mask(const float* z, const float* enc, float* v, int Bt, int S, int N, int L, void* stream);
int srf_decoder_weight_expand(const float* w, float* wexp, int N, int S, int K, void* stream);
int srf_bias_rescale(float* out, const float* bias, const float* stats, const float* wav, int mc, int Bt, int S, int T,
                     void* stream);

/* ---- Original SuDoRM-RF: opt-in training step (csrc/srf_original_train.hip; additive to ABI 19) ----
 * srf_original_forward_train is srf_forward's arithmetic for an original plan (the pyramid level by level, the 1x1 convolutions
 *   in the exact-fp32 class as srf_forward_train runs them) and keeps what the backward needs in `saved`: the GroupNorm
 *   statistics, the encoder output s, the block stream x_0 .. x_U, per block y1, the D raw levels, m, g and g + x, the mask GEMM's
 *   input where reshape_before_masks exists, the logits z.  The activations a and e are NOT saved: the backward re-computes each
 *   with one srf_gln_apply_c launch.
 * srf_original_backward: grad_out [Bt, S, T] -> every parameter gradient, ACCUMULATED into grads[i] (same order and shapes as
 *   params; the caller zeroes them).  Torch autograd over the reference's SuDORMRF.forward (sudormrf.py) -- there ln_mask_in.*
 *   receives no gradient: the last two entries of grads may be NULL and are never written.  No gradient w.r.t. wav.
 * saved / scratch: 256-byte aligned device buffers of srf_original_train_saved_bytes / _scratch_bytes (0 for any plan that is not
 *   SRF_VARIANT_ORIGINAL); `saved` stays untouched between the two calls, `scratch` may be reused in between.  Both calls refuse
 *   (SRF_EINVAL, before the first launch, naming the argument) any other plan, a parameter count that is not the plan's, a null
 *   parameter / gradient, and a short or misaligned buffer.  The general srf_forward_train / srf_backward keep refusing the plan.
 *
 * The kernels this model's backward has that no other has.  Every parameter gradient is ACCUMULATED into; every reduction
 * writes block partials and adds them in block order (no floating-point atomics): the same inputs give the same bits.
 * srf_gln_c_bwd: backward of srf_gln_apply_c, y = [PReLU_c](norm(x)) [+ add] (the addend's gradient is gout itself).  gout
 *   (+ optional gout2, added on load), x, gx: [groups, channels, length] at any float-aligned address, any length (16-byte
 *   accesses where gout, gout2, x and gx share their phase on the 16-byte grid).  norm: {sums of x, gamma, beta}; slopes
 *   [channels] or NULL (no activation).  With xh = (x - mean) rstd, v = gamma_c xh + beta_c, g' = gout (v >= 0 ? 1 : slope_c):
 *   gx (accumulate_gx != 0: added to) = rstd (gamma_c g' - mean(gamma g') - xh mean(gamma g' xh)), the means over the example;
 *   dgamma_c += sum g' xh, dbeta_c += sum g', dslope_c += sum gout v [v < 0] (each nullable; dslope ignored without slopes).
 *   Two launches (reduce, apply); v is re-computed.  scratch: srf_gln_c_bwd_scratch_bytes(groups, channels, length), float-aligned.
 * srf_softmax_mask_bwd: backward of srf_softmax_mask from the logits z and enc: p re-computed as the forward does (maximum
 *   subtracted, expf), gz_s = p_s (gv_s enc - sum_r p_r gv_r enc) (S = 1: gv enc p (1 - p)), gz may be gv;
 *   genc (accumulate_genc != 0: +=) sum_s gv_s p_s.  z, gv, gz: [Bt, S N, L]; enc, genc: [Bt, N, L].
 * srf_mask_weight_fold: the transpose of srf_mask_weight_fill: dmw[s, j] += sum_{i, n: n - i + N - N / 2 = j} dtz[s N + i, n],
 *   j = 0 .. N; dmb[s] += sum_i drow[s N + i].  dtz [S N, N], drow [S N].
 * srf_decoder_weight_contract: dw[c, k] += dwexp[c, c / N, k]: the diagonal blocks of the [S N, S, K] gradient of the
 *   block-diagonal decoder weight.
 * srf_decoder_bias_grad: dbias[s] += sum_{b, t} grad_out[b, s, t], grad_out [Bt, S, T]; scratch:
 *   srf_decoder_bias_grad_scratch_floats(S) floats.
 * srf_relu_gate: g[i] = s[i] > 0 ? g[i] : 0 in place, s the saved post-ReLU output; n elements. */
size_t srf_original_train_saved_bytes(const srf_plan* plan);
size_t srf_original_train_scratch_bytes(const srf_plan* plan);
int srf_original_forward_train(const srf_plan* plan, const float* const* params, int num_params, const float* wav, float* out,
                               void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes, void* stream);
int srf_original_backward(const srf_plan* plan, const float* const* params, float* const* grads, int num_params, const float* wav,
                          const float* grad_out, const void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes,
                          void* stream);
size_t srf_gln_c_bwd_scratch_bytes(int groups, int channels, int length);
int srf_gln_c_bwd(const float* gout, const float* gout2, const float* x, const srf_norm* norm, const float* slopes, int groups,
                  int channels, int length, float* gx, int accumulate_gx, float* dgamma, float* dbeta, float* dslope, void* scratch,
                  void* stream);
int srf_softmax_mask_bwd(const float* z, const float* enc, const float* gv, float* gz, float* genc, int accumulate_genc, int Bt,
                         int S, int N, int L, void* stream);
int srf_mask_weight_fold(const float* dtz, const float* drow, float* dmw, float* dmb, int N, int S, void* stream);
int srf_decoder_weight_contract(const float* dwexp, float* dw, int N, int S, int K, void* stream);
size_t srf_decoder_bias_grad_scratch_floats(int S);
int srf_decoder_bias_grad(const float* grad_out, float* dbias, int Bt, int S, int T, float* scratch, void* stream);
int srf_relu_gate(float* g, const float* s, long n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SUDORMRF_HIP_H */
