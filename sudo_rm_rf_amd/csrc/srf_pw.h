// Shared pieces of the pointwise-conv GEMM kernels (srf_pwconv*.hip).
#pragma once
#include "srf_internal.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// 8 fp32 values -> their bf16 hi | lo parts (hi = bf16(v), lo = bf16(v - hi): 16 mantissa bits, three MFMAs per product block)
__device__ __forceinline__ void srf_split8(const float (&v)[8], bf16x8& hi, bf16x8& lo) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const __bf16 h = (__bf16)v[j];
    hi[j] = h;
    lo[j] = (__bf16)(v[j] - (float)h);
  }
}

// Byte offset of 16-byte chunk c (0..3) of row r in a [rows][32] bf16 image with 64-byte rows, XOR-swizzled.  The packed weight
// images (srf_x3w_pack_kernel) are written with it and read back by the x3w / x3p / x3f kernels: ONE function, or the format breaks.
__host__ __device__ __forceinline__ int srf_swz(int r, int c) { return r * 64 + ((c ^ ((r >> 2) & 3)) << 4); }

#define SRF_LDS(p) ((__attribute__((address_space(3))) void*)(p))   // a pointer into LDS as the DMA builtins want it

// 0 = identity, 1 = GlobLN, 2 = GlobLN + PReLU, 3 = PReLU only: the PRO template argument of every GEMM kernel
static inline int srf_pw_pro(const SrfNormDev& n) { return n.sums ? (n.prelu ? 2 : 1) : (n.prelu ? 3 : 0); }

struct PwArgs {
  const float* x;
  const float* w;
  const float* bias;
  float* y;
  const float* residual;
  double* out_sums;
  const float* mul;
  SrfNormDev nrm;
  double inv_count;
  int Cin, Cout, L, Bt;
  int mul_channels;
  int epi_mask;
  // srf_pwconv_small.hip only: the conv's input is u = x + GlobLN(pre_q) (GroupComm's TAC norm + residual,
  // groupcomm_sudormrf_v2.py:381-384, folded into this conv's load); u is also written to pre_u (the block's residual)
  const float* pre_q = nullptr;
  float* pre_u = nullptr;
  SrfNormDev pre_nrm = {nullptr, nullptr, nullptr, nullptr};
  double pre_inv_count = 0.0;
};


// Two 1x1 convolutions back to back in one launch (srf_pwconv_x3f.hip): y = W1 f(x) + b1 (+ residual) with Cout = 256, then
// y2 = W2 y + b2 and the statistics of y2.  wpack1 / wpack2: the paired-block image of the two weights (srf_x3p_packed_bytes).
struct PwPairArgs {
  // conv 1
  const float* x;
  const float* residual;
  const float* bias1;
  float* y;
  SrfNormDev nrm;
  double inv_count;
  const char* wpack1;
  // conv 2
  const char* wpack2;
  const float* bias2;
  float* y2;
  double* out_sums2;
  int K1, C2, L, Bt, nLt, total;
};

// ---- launchers of the GEMM files, called by the dispatch in srf_pwconv.hip (the rest of the cross-file surface: srf_internal.h)
int srf_pw_bf16x3_launch(const PwArgs& a, int pro, hipStream_t st);
// its ragged form (one tile per block, buffer loads; the caller has checked the table, the shape and the 32-bit reach)
int srf_pw_bf16x3_ragged_launch(const PwArgs& a, int pro, hipStream_t st, const SrfFrames& frames);
int srf_pw_w4_launch(const PwArgs& a, int pro, hipStream_t st);   // 64 x 64 tiles for small launches (srf_pwconv_w4.hip)
bool srf_pw_w4_wanted(const PwArgs& a);
// the 256 x 128 kernel (srf_pwconv_x3w.hip); frames: null = the uniform kernels, else its ragged form
int srf_pw_x3w_launch(const PwArgs& a, const char* wpack, int pro, hipStream_t st, const SrfFrames* frames = nullptr);
int srf_pw_x3p_launch(const PwArgs& a, const char* wpack, int pro, hipStream_t st);   // its paired-block form (srf_pwconv_x3p.hip)
bool srf_x3p_supported(const PwArgs& a, int pro);
// the thin-shape kernel (srf_pwconv_small.hip); frames: null = the uniform kernels, else its ragged forms over folded rows
// (a.Bt rows, rows_per_example of them per table entry)
int srf_pw_small_launch(const PwArgs& a, hipStream_t st, const SrfFrames* frames = nullptr, int rows_per_example = 1);
// the fused pair (srf_pwconv_x3f.hip); frames: null = the uniform kernels, else its ragged form (bf16 parts, pro 1 / 2)
int srf_pw_x3f_launch(const PwPairArgs& a, int pro, hipStream_t st, bool f16 = false, const SrfFrames* frames = nullptr);
// K5: mask GEMM + decoder contraction in one launch (srf_pwconv_x3w.hip, EPI 4)
int srf_pw_x3w_fused_tail_launch(const PwArgs& a, const char* wpack, const char* wdpack, float* zpart, int M, hipStream_t st);
int srf_pw_x3w3_launch(const PwArgs& a, const char* wpack3, int pro, hipStream_t st);   // three bf16 parts (training forward)
int srf_pw_x3w4_launch(const PwArgs& a, const char* wpack, int pro, hipStream_t st);    // two fp16 parts (training forward)

// Launch macros of the kernels that have a ragged form (template arguments ..., SrfFrames): SRF_FRAMES_ARG(the optional template
// arguments) is `, *frames` behind the kernel arguments when SrfFrames is the last of them, nothing otherwise
#define SRF_FRAMES_ARG(opt, ...) SRF_FRAMES_ARG_##__VA_ARGS__
#define SRF_FRAMES_ARG_
#define SRF_FRAMES_ARG_SrfFrames , *frames


// XCD-aware tile numbering: hardware places block id on XCD id%8; give each XCD a contiguous run of
// virtual ids so the Cout/BM blocks that share one X tile hit the same L2 (bijective for any total).
__device__ __forceinline__ int srf_xcd_remap(int id, int total) {
  const int xcd = id & 7, slot = id >> 3;
  const int qn = total >> 3, rn = total & 7;
  return (xcd < rn ? xcd * (qn + 1) : rn * (qn + 1) + (xcd - rn) * qn) + slot;
}

// Epilogue of a 32(row) x 64(time) strip held as two 32x32 MFMA accumulator tiles (accL | accR), staged
// through a wave-private LDS strip so that global traffic is row-contiguous 16-B per lane
// (4 rows x 256 B per wavefront instruction) instead of 4-B scattered stores:
//   C/D layout of v_mfma_f32_32x32x*: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
// bias / residual / ReLU*enc / {sum,sumsq} are applied on the float4 side.  `strip` = 32*SRF_EPI_PITCH
// floats, 16-B aligned, private to the calling wavefront (all 64 lanes must call).
// RAGGED (srf_pw_conv_ragged; `own` = the example's column count, any value in 1..L): after bias and residual -- which may have
// read anything past the example's end -- the components at columns >= own are SELECTED to exact 0.f, so the 16-byte stores stay
// whole, the straddling tile holds zeros up to its end and the statistics run over own columns only.
constexpr int SRF_EPI_PITCH = 68;

template <bool RAGGED = false>
__device__ __forceinline__ void srf_pw_epilogue_strip(const PwArgs& a, const f32x16& accL, const f32x16& accR,
                                                      float* strip, long b, int m_base, int l_base, int lane,
                                                      float& s, float& q, int own = 0) {
  const int col = lane & 31, kh = lane >> 5;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * kh;
    strip[row * SRF_EPI_PITCH + col] = accL[r];
    strip[row * SRF_EPI_PITCH + 32 + col] = accR[r];
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int c4 = (lane & 15) * 4;
  const int l = l_base + c4;
  const bool l_ok = l < a.L;  // L % 4 == 0 -> the whole float4 is in range
  const size_t lc = l_ok ? l : 0;
  const int mulC = a.mul_channels;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int row = i * 4 + (lane >> 4);
    const int m = m_base + row;
    const bool ok = l_ok && m < a.Cout;
    const int mc = m < a.Cout ? m : 0;  // clamped: loads stay unconditional (no branch, no vmcnt drain)
    float4 v = *reinterpret_cast<const float4*>(strip + row * SRF_EPI_PITCH + c4);
    const float bs = a.bias[mc];
    v.x += bs;
    v.y += bs;
    v.z += bs;
    v.w += bs;
    const size_t idx = ((size_t)b * a.Cout + mc) * a.L + lc;
    if (a.residual) {
      const float4 rv = *reinterpret_cast<const float4*>(a.residual + idx);
      v.x += rv.x;
      v.y += rv.y;
      v.z += rv.z;
      v.w += rv.w;
    }
    if (a.epi_mask & 1) {
      const float4 e = *reinterpret_cast<const float4*>(a.mul + ((size_t)b * mulC + (mc % mulC)) * a.L + lc);
      v.x = fmaxf(v.x, 0.f) * e.x;
      v.y = fmaxf(v.y, 0.f) * e.y;
      v.z = fmaxf(v.z, 0.f) * e.z;
      v.w = fmaxf(v.w, 0.f) * e.w;
    }
    if constexpr (RAGGED) {
      v.x = l + 0 < own ? v.x : 0.f;
      v.y = l + 1 < own ? v.y : 0.f;
      v.z = l + 2 < own ? v.z : 0.f;
      v.w = l + 3 < own ? v.w : 0.f;
    }
    if (ok) {
      *reinterpret_cast<float4*>(a.y + idx) = v;
      s += (v.x + v.y) + (v.z + v.w);
      q = fmaf(v.x, v.x, fmaf(v.y, v.y, fmaf(v.z, v.z, fmaf(v.w, v.w, q))));
    }
  }
}

// ---- 32 x 32 variant (one accumulator tile per call), shared by the persistent kernels ----
constexpr int SRF_EPI_PITCH_H = 36;

// one 32x32 accumulator tile -> rows x 128 B float4 stores (see srf_pw_epilogue_strip)
__device__ __forceinline__ void srf_pw_epilogue_half(const PwArgs& a, const f32x16& acc, float* strip, long b,
                                                     int m_base, int l_base, int lane, float& s, float& q) {
  const int col = lane & 31, kh = lane >> 5;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * kh;
    strip[row * SRF_EPI_PITCH_H + col] = acc[r];
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int c4 = (lane & 7) * 4;
  const int l = l_base + c4;
  const bool l_ok = l < a.L;
  const size_t lc = l_ok ? l : 0;
  const int mulC = a.mul_channels;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = i * 8 + (lane >> 3);
    const int m = m_base + row;
    const bool ok = l_ok && m < a.Cout;
    const int mc = m < a.Cout ? m : 0;
    float4 v = *reinterpret_cast<const float4*>(strip + row * SRF_EPI_PITCH_H + c4);
    const float bs = a.bias[mc];
    v.x += bs;
    v.y += bs;
    v.z += bs;
    v.w += bs;
    const size_t idx = ((size_t)b * a.Cout + mc) * a.L + lc;
    if (a.residual) {
      const float4 rv = *reinterpret_cast<const float4*>(a.residual + idx);
      v.x += rv.x;
      v.y += rv.y;
      v.z += rv.z;
      v.w += rv.w;
    }
    if (a.epi_mask & 1) {
      const float4 e = *reinterpret_cast<const float4*>(a.mul + ((size_t)b * mulC + (mc % mulC)) * a.L + lc);
      v.x = fmaxf(v.x, 0.f) * e.x;
      v.y = fmaxf(v.y, 0.f) * e.y;
      v.z = fmaxf(v.z, 0.f) * e.z;
      v.w = fmaxf(v.w, 0.f) * e.w;
    }
    if (ok) {
      *reinterpret_cast<float4*>(a.y + idx) = v;
      s += (v.x + v.y) + (v.z + v.w);
      q = fmaf(v.x, v.x, fmaf(v.y, v.y, fmaf(v.z, v.z, fmaf(v.w, v.w, q))));
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

