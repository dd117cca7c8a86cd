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
};

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
