// Original SuDoRM-RF (sudormrf.py, the model of the paper): plan constructor, the inference and ragged forwards and the kernels
// it has that no other variant has.  Single stream.  THE forward walk, which the training forward runs too: srf_original_walk.h;
// the training step: srf_original_train.hip.  Parameter and slot layout: srf_plan.h.
//
//   s   = relu(encoder.0(wav))                                srf_encoder_bias_relu (+ statistics of ln)
//   x   = l1(ln(s))                                           srf_pw_conv_packed    (ln on load)
// One block (UBlock.forward); GroupNorm(1, C) is GlobLN's arithmetic, PReLU has one slope per channel:
//   y1  = proj_1x1.conv(x)                                    srf_pw_conv_packed    (+ statistics of proj_1x1.norm)
//   a   = PReLU_c(proj_1x1.norm(y1))                          srf_gln_apply_c       (materialised: no prologue takes a slope vector)
//   d_0 = spp_dw[0].conv(a); d_k = spp_dw[k].conv(norm(d_{k-1}))   srf_pyramid with NO input norm where it takes the shape
//   m   = upsample-and-add of norm_k(d_k)                     (+ statistics of final_norm; into y1); else srf_dwconv5 x D + srf_merge
//   e   = PReLU_c(final_norm(m))                              srf_gln_apply_c       (into a's buffer)
//   g   = conv_1x1_exp.conv(e)                                srf_pw_conv_packed    (+ statistics of conv_1x1_exp.norm)
//   gx  = conv_1x1_exp.norm(g) + x                            srf_gln_apply_c       (no slope, addend, + statistics of module_act.norm)
//   x'  = PReLU_c(module_act.norm(gx))                        srf_gln_apply_c       (over x: dead since the step before)
// Tail:
//   xr  = reshape_before_masks(x)                             srf_pw_conv_packed    (only when B != N)
//   z   = Tz xr + m.bias                                      srf_pw_conv_packed over the Toeplitz weight srf_mask_weight_fill wrote
//   v   = softmax_s(z) * s                                    srf_softmax_mask
//   out = decoder(v) + decoder.bias [rescale, mixture consistency]   srf_decoder_impl over the block-diagonal weight, srf_bias_rescale
//
// Ragged batches (opt-in: srf_original_forward_ragged / srf_original_separate_ragged): the SAME walk with a
// frames table.  L stays the row stride; example b has L_b = frames[b] columns (its own length padded to a multiple of
// lcm(hop, 2^D), over the hop) and len_b samples, and every kernel above runs as its ragged twin.  The invariants: with the walk.
#include <vector>
#include "srf_original_walk.h"

// ---------------------------------------------------------------------------------------------
// y = [PReLU_c](norm(x)) [+ add], out_sums += {sum, sumsq} of the stored y.  Bandwidth-bound: one block per (row = (g, c), chunk
// of GC_CHUNK positions).  VEC: x, add and y share their phase on the 16-byte grid (the walk's buffers always do), so a row
// chunk is a scalar head up to the grid, 16-byte loads and stores, and a scalar tail; else dwords throughout.
// ---------------------------------------------------------------------------------------------
constexpr int GC_CHUNK = 2048;

struct GlnCRow {
  float sc, sh, slope;
  bool act;
};
__device__ __forceinline__ float gln_c_one(float x, const GlnCRow& r) {
  float v = fmaf(x, r.sc, r.sh);
  if (r.act) v = srf_prelu(v, r.slope);
  return v;
}

// RAGGED (srf_gln_apply_c_ragged; FR = SrfFrames): `length` stays the row stride, group g is frames[g] columns long (a multiple
// of 4).  x and add are not read at columns >= frames[g], y is stored as exact 0 there, the GlobLN count is channels * frames[g]
// and out_sums run over the group's own columns; a (row, chunk) block wholly past the end stores its zeros and loads nothing.
// The end may cut a chunk anywhere: with a base off the 16-byte grid it falls inside one 16-byte group, which then goes
// element by element.
template <bool VEC, bool ADD, typename... FR>
__global__ __launch_bounds__(256) void srf_gln_apply_c_kernel(const float* __restrict__ x, SrfNormDev n, const float* __restrict__ slopes,
                                                              const float* __restrict__ add, float* __restrict__ y,
                                                              double* __restrict__ out_sums, double inv_count, int channels,
                                                              int length, int chunks, FR... fr) {
  constexpr bool RAGGED = sizeof...(FR) != 0;
  __shared__ double red[8];
  const long row = blockIdx.x / chunks;
  const int chunk = (int)(blockIdx.x - row * chunks);
  const int c = (int)(row % channels);
  const long g = row / channels;
  int own = 0;      // (RAGGED only) elements of this chunk inside the group's own columns: 1 .. cnt
  if constexpr (RAGGED) {
    const int Lg = srf_frames_of((int)g, fr...);
    const int cnt = min(GC_CHUNK, length - chunk * GC_CHUNK);
    own = min(cnt, Lg - chunk * GC_CHUNK);
    inv_count = 1.0 / ((double)channels * (double)Lg);
    if (own <= 0) {      // block-uniform: zeros, nothing loaded, nothing added to the statistics
      float* yp = y + (size_t)row * length + (size_t)chunk * GC_CHUNK;
      if constexpr (VEC) {
        const int head = min(cnt, (int)(((16 - ((size_t)yp & 15)) & 15) >> 2));
        const int nv = (cnt - head) >> 2, tail0 = head + 4 * nv;
        if ((int)threadIdx.x < head) yp[threadIdx.x] = 0.f;
        for (int i = threadIdx.x; i < nv; i += 256) *reinterpret_cast<float4*>(yp + head + 4 * i) = make_float4(0.f, 0.f, 0.f, 0.f);
        if ((int)threadIdx.x < cnt - tail0) yp[tail0 + threadIdx.x] = 0.f;
      } else {
        for (int i = threadIdx.x; i < cnt; i += 256) yp[i] = 0.f;
      }
      return;
    }
  }
  float mean, rstd;
  srf_finalize_stats(n.sums, g, inv_count, mean, rstd);
  GlnCRow r;
  r.sc = n.gamma[c] * rstd;
  r.sh = n.beta[c] - mean * r.sc;
  r.act = slopes != nullptr;
  r.slope = r.act ? slopes[c] : 1.f;
  const size_t base = (size_t)row * length + (size_t)chunk * GC_CHUNK;
  const int cnt = min(GC_CHUNK, length - chunk * GC_CHUNK);      // elements of this chunk: 1 .. GC_CHUNK
  const float* xp = x + base;
  const float* ap = ADD ? add + base : nullptr;
  float* yp = y + base;
  double ds = 0.0, dq = 0.0;
  auto one = [&](int i) {
    float v = gln_c_one(xp[i], r);
    if constexpr (ADD) v += ap[i];
    yp[i] = v;
    ds += (double)v;
    dq += (double)v * (double)v;
  };
  // (RAGGED) element i of the chunk: the group's own, or zero padding
  auto one_or_zero = [&](int i) {
    if (!RAGGED || i < own) one(i);
    else yp[i] = 0.f;
  };
  if constexpr (VEC) {
    const int head = min(cnt, (int)(((16 - ((size_t)xp & 15)) & 15) >> 2));      // dwords up to the 16-byte grid
    const int nv = (cnt - head) >> 2;
    const int tail0 = head + 4 * nv;
    if ((int)threadIdx.x < head) one_or_zero(threadIdx.x);
    for (int i = threadIdx.x; i < nv; i += 256) {
      if constexpr (RAGGED) {
        const int p = head + 4 * i;
        if (p >= own) {
          *reinterpret_cast<float4*>(yp + p) = make_float4(0.f, 0.f, 0.f, 0.f);
          continue;
        }
        if (p + 4 > own) {      // the one group the end cuts
          for (int e = 0; e < 4; ++e) one_or_zero(p + e);
          continue;
        }
      }
      const float4 a = *reinterpret_cast<const float4*>(xp + head + 4 * i);
      float4 o;
      o.x = gln_c_one(a.x, r), o.y = gln_c_one(a.y, r), o.z = gln_c_one(a.z, r), o.w = gln_c_one(a.w, r);
      if constexpr (ADD) {
        const float4 b = *reinterpret_cast<const float4*>(ap + head + 4 * i);
        o.x += b.x, o.y += b.y, o.z += b.z, o.w += b.w;
      }
      *reinterpret_cast<float4*>(yp + head + 4 * i) = o;
      ds += ((double)o.x + (double)o.y) + ((double)o.z + (double)o.w);
      dq += ((double)o.x * o.x + (double)o.y * o.y) + ((double)o.z * o.z + (double)o.w * o.w);
    }
    if ((int)threadIdx.x < cnt - tail0) one_or_zero(tail0 + threadIdx.x);
  } else {
    for (int i = threadIdx.x; i < cnt; i += 256) one_or_zero(i);
  }
  if (out_sums) srf_block_stats_atomic<4>(ds, dq, srf_stat_slot(out_sums, g, blockIdx.x), red);
}

// who: the entry point's name in its refusals; frames: NULL = the uniform call, else one entry per group (srf_gln_apply_c_ragged)
static int gln_apply_c_impl(const char* who, const float* x, const srf_norm* norm, const float* slopes, const float* add, float* y,
                            double* out_sums, int groups, int channels, int length, const int* frames, void* stream) {
  SRF_CHECK_ARG(x && y && norm && groups > 0 && channels > 0 && length > 0, "%s: bad arguments", who);
  SRF_CHECK_ARG(norm->sums && norm->gamma && norm->beta, "%s: the norm needs statistics, gamma and beta", who);
  SRF_CHECK_ARG((const void*)norm->sums != (const void*)out_sums, "%s: out_sums must not be norm.sums", who);
  {
    // y overlaps neither input: blocks of other rows would read what this one has already overwritten
    const size_t bytes = sizeof(float) * (size_t)groups * channels * length;
    auto overlaps = [&](const float* in) { return in && (const char*)y < (const char*)in + bytes && (const char*)in < (const char*)y + bytes; };
    SRF_CHECK_ARG(!overlaps(x) && !overlaps(add), "%s: y must not overlap x or add", who);
  }
  SRF_CHECK_ALIGNED16(who, {"norm.sums", norm->sums});
  SRF_CHECK_ARG((((size_t)x | (size_t)y | (size_t)add) & 3) == 0, "%s: x, add and y must be float-aligned", who);
  const int chunks = (length + GC_CHUNK - 1) / GC_CHUNK;
  const long blocks = (long)groups * channels * chunks;
  SRF_CHECK_ARG(blocks < (1L << 31), "%s: tensor too large", who);
  const bool vec = srf_kernel_mode() != 1 && (((size_t)x ^ (size_t)y) & 15) == 0 && (!add || (((size_t)x ^ (size_t)add) & 15) == 0);
  const SrfNormDev nd{norm->sums, norm->gamma, norm->beta, nullptr};
  const double inv = 1.0 / ((double)channels * (double)length);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks), blk(256);
  if (frames) {
    SrfFrames fr;
    const int rc = srf_frames_table(who, frames, groups, length, &fr);
    if (rc) return rc;
    for (int g = 0; g < groups; ++g)
      SRF_CHECK_ARG(frames[g] % 4 == 0, "%s: example %d has %d frames: not a multiple of 4", who, g, frames[g]);
    if (vec && add)
      hipLaunchKernelGGL((srf_gln_apply_c_kernel<true, true, SrfFrames>), grid, blk, 0, st, x, nd, slopes, add, y, out_sums, inv, channels, length, chunks, fr);
    else if (vec)
      hipLaunchKernelGGL((srf_gln_apply_c_kernel<true, false, SrfFrames>), grid, blk, 0, st, x, nd, slopes, add, y, out_sums, inv, channels, length, chunks, fr);
    else if (add)
      hipLaunchKernelGGL((srf_gln_apply_c_kernel<false, true, SrfFrames>), grid, blk, 0, st, x, nd, slopes, add, y, out_sums, inv, channels, length, chunks, fr);
    else
      hipLaunchKernelGGL((srf_gln_apply_c_kernel<false, false, SrfFrames>), grid, blk, 0, st, x, nd, slopes, add, y, out_sums, inv, channels, length, chunks, fr);
    SRF_CHECK_LAUNCH(vec ? "gln_apply_c_ragged" : "gln_apply_c_scalar_ragged", st);
    return SRF_OK;
  }
  if (vec && add)
    hipLaunchKernelGGL((srf_gln_apply_c_kernel<true, true>), grid, blk, 0, st, x, nd, slopes, add, y, out_sums, inv, channels, length, chunks);
  else if (vec)
    hipLaunchKernelGGL((srf_gln_apply_c_kernel<true, false>), grid, blk, 0, st, x, nd, slopes, add, y, out_sums, inv, channels, length, chunks);
  else if (add)
    hipLaunchKernelGGL((srf_gln_apply_c_kernel<false, true>), grid, blk, 0, st, x, nd, slopes, add, y, out_sums, inv, channels, length, chunks);
  else
    hipLaunchKernelGGL((srf_gln_apply_c_kernel<false, false>), grid, blk, 0, st, x, nd, slopes, add, y, out_sums, inv, channels, length, chunks);
  SRF_CHECK_LAUNCH(vec ? "gln_apply_c" : "gln_apply_c_scalar", st);
  return SRF_OK;
}
extern "C" int srf_gln_apply_c(const float* x, const srf_norm* norm, const float* slopes, const float* add, float* y, double* out_sums,
                               int groups, int channels, int length, void* stream) {
  return gln_apply_c_impl("srf_gln_apply_c", x, norm, slopes, add, y, out_sums, groups, channels, length, nullptr, stream);
}
extern "C" int srf_gln_apply_c_ragged(const float* x, const srf_norm* norm, const float* slopes, const float* add, float* y,
                                      double* out_sums, int groups, int channels, int length, const int* frames, void* stream) {
  SRF_CHECK_ARG(frames != nullptr, "srf_gln_apply_c_ragged: null frames table");
  return gln_apply_c_impl("srf_gln_apply_c_ragged", x, norm, slopes, add, y, out_sums, groups, channels, length, frames, stream);
}

// ---------------------------------------------------------------------------------------------
// Encoder with bias and ReLU: out[b, n, l] = relu(bias[n] + sum_k w[n, k] xpad[b, h l + k - h]), one audio channel, any odd K.
// A kernel of its own (the Improved encoder's instantiations keep their code).  64 frames per block, lane = frame, the basis
// function is wave-uniform: taps and bias are scalar operands.  KT = the compile-time K with the lane's window in registers;
// KT = 0: any K, the window read from LDS in the inner loop.  Statistics of the stored (post-ReLU) output.
// ---------------------------------------------------------------------------------------------
// RAGGED (srf_encoder_bias_relu_ragged; TABS = SrfFrames samples, SrfFrames frames; KT = 21 only): T and L stay the row strides,
// example b is lens[b] samples and frames[b] frames long.  Samples at or past lens[b] are never read -- with in_stats the padding
// is that of the NORMALISED signal, zero -- and frames at or past frames[b] are stored as exact 0: relu(bias) is not zero, and
// frame frames[b] would see the example's last H samples.  The statistics run over the example's own frames; a time tile
// wholly past the end stores its zeros without staging a window.
template <int KT, typename... TABS>
__global__ __launch_bounds__(256) void srf_encoder_bias_relu_kernel(const float* __restrict__ wav, const float* __restrict__ w,
                                                                    const float* __restrict__ bias, float* __restrict__ out,
                                                                    double* __restrict__ sums, int T, int N, int K, int L,
                                                                    const float* __restrict__ in_stats, TABS... tabs) {
  constexpr bool RAGGED = sizeof...(TABS) != 0;
  extern __shared__ __attribute__((aligned(16))) char eb_smem[];
  double* red = reinterpret_cast<double*>(eb_smem);        // 8 doubles
  float* win = reinterpret_cast<float*>(eb_smem + 64);     // [63 H + K]
  const int Kk = KT ? KT : K, H = Kk / 2;
  const int WIN = 63 * H + Kk;
  const int b = blockIdx.y;
  const int l0 = blockIdx.x * 64;
  const float* xb = wav + (size_t)b * T;
  const int Tb = RAGGED ? srf_frames_of(b, tabs...) : T;     // samples / frames of this example
  const int Lb = RAGGED ? srf_frames2_of(b, tabs...) : L;
  if constexpr (RAGGED) {
    if (l0 >= Lb) {   // block-uniform
      const int per = ((N + (int)gridDim.z - 1) / (int)gridDim.z + 3) & ~3;
      const int n_lo = blockIdx.z * per, n_hi = min(N, n_lo + per);
      const int l = l0 + (int)(threadIdx.x & 63);
      if (l < L)
        for (int n = n_lo + (int)(threadIdx.x >> 6); n < n_hi; n += 4) out[((size_t)b * N + n) * L + l] = 0.f;
      return;
    }
  }
  const float im = in_stats ? in_stats[2 * b] : 0.f, iden = in_stats ? in_stats[2 * b + 1] + 1e-9f : 1.f;
  for (int i = threadIdx.x; i < WIN; i += 256) {
    const long t = (long)H * l0 - H + i;
    win[i] = (t >= 0 && t < Tb) ? (in_stats ? (xb[t] - im) / iden : xb[t]) : 0.f;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l = l0 + lane;
  const int per = ((N + (int)gridDim.z - 1) / (int)gridDim.z + 3) & ~3;      // blockIdx.z: a slice of the basis
  const int n_lo = blockIdx.z * per, n_hi = min(N, n_lo + per);
  double ds = 0.0, dq = 0.0;
  if constexpr (KT != 0) {
    float xw[KT ? KT : 1];
#pragma unroll
    for (int k = 0; k < KT; ++k) xw[k] = win[H * lane + k];
    for (int n = n_lo + wave; n < n_hi; n += 4) {
      const float* wn = w + (size_t)n * KT;
      float acc = bias[n];
#pragma unroll
      for (int k = 0; k < KT; ++k) acc = fmaf(wn[k], xw[k], acc);
      acc = fmaxf(acc, 0.f);
      if constexpr (RAGGED) acc = l < Lb ? acc : 0.f;
      if (l < L) {
        out[((size_t)b * N + n) * L + l] = acc;
        ds += (double)acc;
        dq += (double)acc * (double)acc;
      }
    }
  } else {
    const float* xw = win + H * lane;
    for (int n = n_lo + wave; n < n_hi; n += 4) {
      const float* wn = w + (size_t)n * Kk;
      float acc = bias[n];
      for (int k = 0; k < Kk; ++k) acc = fmaf(wn[k], xw[k], acc);
      acc = fmaxf(acc, 0.f);
      if (l < L) {
        out[((size_t)b * N + n) * L + l] = acc;
        ds += (double)acc;
        dq += (double)acc * (double)acc;
      }
    }
  }
  if (sums) srf_block_stats_atomic<4>(ds, dq, srf_stat_slot(sums, b, blockIdx.x + blockIdx.z * gridDim.x), red);
}

extern "C" int srf_encoder_bias_relu(const float* wav, const float* w, const float* bias, float* out, double* sums, int Bt, int T,
                                     int N, int K, int L, const float* in_stats, void* stream) {
  SRF_CHECK_ARG(wav && w && bias && out, "srf_encoder_bias_relu: null pointer");
  SRF_CHECK_ARG(Bt > 0 && T > 0 && N > 0 && L > 0, "srf_encoder_bias_relu: bad sizes");
  SRF_CHECK_ARG(K >= 3 && (K & 1), "srf_encoder_bias_relu: enc_kernel_size must be odd and >= 3 (got %d)", K);
  SRF_CHECK_ARG(Bt <= 65535, "srf_encoder_bias_relu: batch %d too large for one launch", Bt);
  SRF_CHECK_ALIGNED16("srf_encoder_bias_relu", {"sums", sums});
  const int H = K / 2;
  const size_t lds = 64 + sizeof(float) * (size_t)(63 * H + K);
  SRF_CHECK_ARG(lds <= 64 * 1024, "srf_encoder_bias_relu: window does not fit LDS (K = %d)", K);
  hipStream_t st = (hipStream_t)stream;
  // basis slices per (time tile, example), as srf_encoder_impl: enough blocks for small batches, at least 16 functions each
  const long bxy = (long)((L + 63) / 64) * Bt, want = 32L * srf_device_cus();
  int nz = bxy >= want ? 1 : (int)((want + bxy - 1) / bxy);
  nz = nz > N / 16 ? (N / 16 > 0 ? N / 16 : 1) : nz;
  dim3 grid((L + 63) / 64, Bt, nz);
  if (K == 21 && srf_kernel_mode() != 1)
    hipLaunchKernelGGL(srf_encoder_bias_relu_kernel<21>, grid, dim3(256), lds, st, wav, w, bias, out, sums, T, N, K, L, in_stats);
  else
    hipLaunchKernelGGL(srf_encoder_bias_relu_kernel<0>, grid, dim3(256), lds, st, wav, w, bias, out, sums, T, N, K, L, in_stats);
  SRF_CHECK_LAUNCH("encoder_bias_relu", st);
  return SRF_OK;
}

// The ragged form exists for the register-window kernel (K = 21, the model's default; not under kernel mode 1).
extern "C" int srf_encoder_bias_relu_ragged(const float* wav, const float* w, const float* bias, float* out, double* sums, int Bt, int T,
                                            int N, int K, int L, const int* lengths, const int* frames, const float* in_stats,
                                            void* stream) {
  SRF_CHECK_ARG(wav && w && bias && out, "srf_encoder_bias_relu_ragged: null pointer");
  SRF_CHECK_ARG(Bt > 0 && T > 0 && N > 0 && L > 0, "srf_encoder_bias_relu_ragged: bad sizes");
  SRF_CHECK_ARG(K == 21 && srf_kernel_mode() != 1,
                "srf_encoder_bias_relu_ragged: only the K = 21 kernel has a ragged form (K=%d, kernel mode %d)", K, srf_kernel_mode());
  SRF_CHECK_ALIGNED16("srf_encoder_bias_relu_ragged", {"sums", sums});
  SrfFrames lens, fr;
  int rc = srf_frames_table("srf_encoder_bias_relu_ragged (lengths)", lengths, Bt, T, &lens);
  if (rc) return rc;
  rc = srf_frames_table("srf_encoder_bias_relu_ragged (frames)", frames, Bt, L, &fr);
  if (rc) return rc;
  for (int b = 0; b < Bt; ++b)
    SRF_CHECK_ARG((long)lengths[b] <= (long)(K / 2) * frames[b],
                  "srf_encoder_bias_relu_ragged: example %d: %d samples exceed hop * frames = %d", b, lengths[b], (K / 2) * frames[b]);
  const size_t lds = 64 + sizeof(float) * (size_t)(63 * (K / 2) + K);
  hipStream_t st = (hipStream_t)stream;
  const long bxy = (long)((L + 63) / 64) * Bt, want = 32L * srf_device_cus();      // (grid: as srf_encoder_bias_relu)
  int nz = bxy >= want ? 1 : (int)((want + bxy - 1) / bxy);
  nz = nz > N / 16 ? (N / 16 > 0 ? N / 16 : 1) : nz;
  dim3 grid((L + 63) / 64, Bt, nz);
  hipLaunchKernelGGL((srf_encoder_bias_relu_kernel<21, SrfFrames, SrfFrames>), grid, dim3(256), lds, st, wav, w, bias, out, sums, T, N, K,
                     L, in_stats, lens, fr);
  SRF_CHECK_LAUNCH("encoder_bias_relu_ragged", st);
  return SRF_OK;
}

// ---------------------------------------------------------------------------------------------
// The mask layer Conv2d(1 -> S, (N + 1, 1), padding (N - N / 2, 0)) as a GEMM weight: tz[s N + i, n] = mw[s, n - i + pad] where
// 0 <= n - i + pad <= N, else 0 (written); bias_rows[s N + i] = mb[s].  A copy: no arithmetic on the values.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void srf_mask_weight_fill_kernel(const float* __restrict__ mw, const float* __restrict__ mb,
                                                                   float* __restrict__ tz, float* __restrict__ bias_rows, int N, int S) {
  const size_t total = (size_t)S * N * N;
  const int pad = N - N / 2;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int n = (int)(idx % N);
    const size_t rowi = idx / N;              // s N + i
    const int i = (int)(rowi % N), s = (int)(rowi / N);
    const int j = n - i + pad;
    tz[idx] = (j >= 0 && j <= N) ? mw[(size_t)s * (N + 1) + j] : 0.f;
    if (n == 0) bias_rows[rowi] = mb[s];
  }
}

extern "C" int srf_mask_weight_fill(const float* mw, const float* mb, float* tz, float* bias_rows, int N, int S, void* stream) {
  SRF_CHECK_ARG(mw && mb && tz && bias_rows, "srf_mask_weight_fill: null pointer");
  SRF_CHECK_ARG(N >= 2 && N % 2 == 0, "srf_mask_weight_fill: enc_num_basis = %d must be even and positive", N);
  SRF_CHECK_ARG(S >= 1 && (long)S * N < (1L << 24), "srf_mask_weight_fill: num_sources = %d out of range", S);
  const size_t total = (size_t)S * N * N, blocks = (total + 255) / 256;
  hipLaunchKernelGGL(srf_mask_weight_fill_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream, mw,
                     mb, tz, bias_rows, N, S);
  SRF_CHECK_LAUNCH("mask_weight_fill", stream);
  return SRF_OK;
}

// ---------------------------------------------------------------------------------------------
// v[b, s N + i, l] = p_s(z[b, :, i, l]) * enc[b, i, l]: softmax over the S sources with the maximum subtracted, S = 1: sigmoid.
// One thread per (b, i, l), l fastest: every source's row is read and written coalesced; the S logits stay in registers (the
// loops run to the compile-time cap SMAX with a wave-uniform guard, so the array is never indexed dynamically; SMAX = 4 serves
// S <= 4, SMAX = 16 the rest).  The source planes are walked with one per-lane pointer, a plane at a time: 64-bit addresses
// throughout and no table of S plane offsets in scalar registers.  v may be z: a thread reads all of its S logits before it
// writes any.
// ---------------------------------------------------------------------------------------------
// RAGGED (srf_softmax_mask_ragged; FR = SrfFrames): z and enc are not read at columns >= frames[b] -- z comes out of the block
// stream through pointwise GEMMs and is unspecified there -- and v is stored as exact 0, so the decoder's frame GEMM sees zeros.
template <int SMAX, typename... FR>
__global__ __launch_bounds__(256) void srf_softmax_mask_kernel(const float* z, const float* __restrict__ enc, float* v, int S, int N,
                                                               int L, size_t per_example, size_t total, FR... fr) {
  constexpr bool RAGGED = sizeof...(FR) != 0;
  const size_t plane = (size_t)N * L;      // one source of one example
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const size_t b = idx / per_example, r = idx - b * per_example;      // r = i L + l
    const size_t at = b * S * plane + r;
    if constexpr (RAGGED) {
      if ((int)(r % (size_t)L) >= srf_frames_of((int)b, fr...)) {
        float* vp = v + at;
        for (int s = 0; s < S; ++s, vp += plane) *vp = 0.f;
        continue;
      }
    }
    const float e = enc[idx];
    float zv[SMAX];
    float mx = -__builtin_inff();
    const float* zp = z + at;
#pragma unroll
    for (int s = 0; s < SMAX; ++s) {
      zv[s] = -__builtin_inff();
      if (s < S) {
        zv[s] = *zp;
        zp += plane;
      }
      mx = fmaxf(mx, zv[s]);
    }
    if (S == 1) {
      v[at] = e / (1.f + expf(-zv[0]));
      continue;
    }
    float sum = 0.f;
#pragma unroll
    for (int s = 0; s < SMAX; ++s) {
      zv[s] = expf(zv[s] - mx);      // (a source past S: expf(-inf) = 0)
      sum += zv[s];
    }
    const float sc = e / sum;
    float* vp = v + at;
#pragma unroll
    for (int s = 0; s < SMAX; ++s)
      if (s < S) {
        *vp = zv[s] * sc;
        vp += plane;
      }
  }
}

extern "C" int srf_softmax_mask(const float* z, const float* enc, float* v, int Bt, int S, int N, int L, void* stream) {
  SRF_CHECK_ARG(z && enc && v, "srf_softmax_mask: null pointer");
  SRF_CHECK_ARG(Bt > 0 && N > 0 && L > 0, "srf_softmax_mask: bad sizes");
  SRF_CHECK_ARG(S >= 1 && S <= SRF_SOFTMAX_MASK_MAX_SOURCES, "srf_softmax_mask: num_sources = %d unsupported (1..%d)", S,
                SRF_SOFTMAX_MASK_MAX_SOURCES);
  SRF_CHECK_ARG((const void*)enc != (const void*)v, "srf_softmax_mask: v must not be enc");
  const size_t per = (size_t)N * L, total = per * Bt, blocks = (total + 255) / 256;
  const dim3 grid((unsigned)(blocks < (1u << 20) ? blocks : (1u << 20)));
  if (S <= 4)
    hipLaunchKernelGGL(srf_softmax_mask_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, z, enc, v, S, N, L, per, total);
  else
    hipLaunchKernelGGL((srf_softmax_mask_kernel<SRF_SOFTMAX_MASK_MAX_SOURCES>), grid, dim3(256), 0, (hipStream_t)stream, z, enc, v, S, N,
                       L, per, total);
  SRF_CHECK_LAUNCH("softmax_mask", stream);
  return SRF_OK;
}

extern "C" int srf_softmax_mask_ragged(const float* z, const float* enc, float* v, int Bt, int S, int N, int L, const int* frames,
                                       void* stream) {
  SRF_CHECK_ARG(z && enc && v, "srf_softmax_mask_ragged: null pointer");
  SRF_CHECK_ARG(Bt > 0 && N > 0 && L > 0, "srf_softmax_mask_ragged: bad sizes");
  SRF_CHECK_ARG(S >= 1 && S <= SRF_SOFTMAX_MASK_MAX_SOURCES, "srf_softmax_mask_ragged: num_sources = %d unsupported (1..%d)", S,
                SRF_SOFTMAX_MASK_MAX_SOURCES);
  SRF_CHECK_ARG((const void*)enc != (const void*)v, "srf_softmax_mask_ragged: v must not be enc");
  SrfFrames fr;
  const int rc = srf_frames_table("srf_softmax_mask_ragged", frames, Bt, L, &fr);
  if (rc) return rc;
  const size_t per = (size_t)N * L, total = per * Bt, blocks = (total + 255) / 256;
  const dim3 grid((unsigned)(blocks < (1u << 20) ? blocks : (1u << 20)));
  if (S <= 4)
    hipLaunchKernelGGL((srf_softmax_mask_kernel<4, SrfFrames>), grid, dim3(256), 0, (hipStream_t)stream, z, enc, v, S, N, L, per, total, fr);
  else
    hipLaunchKernelGGL((srf_softmax_mask_kernel<SRF_SOFTMAX_MASK_MAX_SOURCES, SrfFrames>), grid, dim3(256), 0, (hipStream_t)stream, z, enc,
                       v, S, N, L, per, total, fr);
  SRF_CHECK_LAUNCH("softmax_mask_ragged", stream);
  return SRF_OK;
}

// ---------------------------------------------------------------------------------------------
// Grouped ConvTranspose1d weight [S N, 1, K] -> block-diagonal [S N, S, K]: row c keeps its K taps in column group c / N, zeros
// elsewhere (written: the workspace holds anything).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void srf_decoder_weight_expand_kernel(const float* __restrict__ w, float* __restrict__ wexp, int N,
                                                                        int S, int K) {
  const size_t total = (size_t)S * N * S * K;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int k = (int)(idx % K);
    const size_t t = idx / K;
    const int s2 = (int)(t % S);
    const size_t c = t / S;
    wexp[idx] = (size_t)s2 == c / N ? w[c * K + k] : 0.f;
  }
}

extern "C" int srf_decoder_weight_expand(const float* w, float* wexp, int N, int S, int K, void* stream) {
  SRF_CHECK_ARG(w && wexp, "srf_decoder_weight_expand: null pointer");
  SRF_CHECK_ARG(N > 0 && S > 0 && K > 0 && (long)S * N < (1L << 24) && (long)S * K < (1L << 16), "srf_decoder_weight_expand: bad sizes");
  const size_t total = (size_t)S * N * S * K, blocks = (total + 255) / 256;
  hipLaunchKernelGGL(srf_decoder_weight_expand_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0,
                     (hipStream_t)stream, w, wexp, N, S, K);
  SRF_CHECK_LAUNCH("decoder_weight_expand", stream);
  return SRF_OK;
}

// ---------------------------------------------------------------------------------------------
// decoder.bias, then the callers' recipe exactly as the overlap-add's POST form has it (srf_elementwise.hip): est = out + bias[s];
// stats: est = est * std + mean; mc: + ((wav - mean) / (std + 1e-9) - sum_s est_s) / S.  One thread per (b, t), in place.
// ---------------------------------------------------------------------------------------------
// RAGGED (srf_bias_rescale_ragged; FR = SrfFrames samples): t >= lens[b] is stored as exactly 0 and wav is never read there.
template <bool POST, typename... FR>
__global__ __launch_bounds__(256) void srf_bias_rescale_kernel(float* __restrict__ out, const float* __restrict__ bias,
                                                               const float* __restrict__ stats, const float* __restrict__ wav, int mc,
                                                               int S, int T, FR... fr) {
  constexpr bool RAGGED = sizeof...(FR) != 0;
  const long b = blockIdx.y;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  if constexpr (RAGGED) {
    if (t >= srf_frames_of((int)b, fr...)) {
      float* ob = out + (size_t)b * S * T + t;
      for (int s = 0; s < S; ++s) ob[(size_t)s * T] = 0.f;
      return;
    }
  }
  float mean = 0.f, sd = 1.f;
  if constexpr (POST) {
    mean = stats[2 * b];
    sd = stats[2 * b + 1];
  }
  float* ob = out + (size_t)b * S * T + t;
  auto est = [&](int s) {
    const float a = ob[(size_t)s * T] + bias[s];
    return POST ? a * sd + mean : a;
  };
  float corr = 0.f;
  if (POST && mc) {
    float tot = 0.f;
    for (int s = 0; s < S; ++s) tot += est(s);
    corr = ((wav[b * (long)T + t] - mean) / (sd + 1e-9f) - tot) * (1.f / (float)S);
  }
  for (int s = 0; s < S; ++s) {
    const float v = est(s);
    ob[(size_t)s * T] = (POST && mc) ? v + corr : v;
  }
}

extern "C" int srf_bias_rescale(float* out, const float* bias, const float* stats, const float* wav, int mc, int Bt, int S, int T,
                                void* stream) {
  SRF_CHECK_ARG(out && bias && Bt > 0 && S > 0 && T > 0, "srf_bias_rescale: bad arguments");
  SRF_CHECK_ARG(Bt <= 65535, "srf_bias_rescale: batch %d too large for one launch", Bt);
  SRF_CHECK_ARG(!stats || !mc || wav, "srf_bias_rescale: mixture consistency needs the raw mixture");
  const dim3 grid((T + 255) / 256, Bt);
  if (stats)
    hipLaunchKernelGGL(srf_bias_rescale_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, out, bias, stats, wav, mc, S, T);
  else
    hipLaunchKernelGGL(srf_bias_rescale_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, out, bias, stats, wav, 0, S, T);
  SRF_CHECK_LAUNCH("bias_rescale", stream);
  return SRF_OK;
}

// the launch alone, from a table the caller has checked (the ragged walk's orig_bias: the one its overlap-add uses)
int srf_bias_rescale_ragged_launch(float* out, const float* bias, const float* stats, const float* wav, int mc, int Bt, int S, int T,
                                      const SrfFrames& lens, void* stream) {
  const dim3 grid((T + 255) / 256, Bt);
  if (stats)
    hipLaunchKernelGGL((srf_bias_rescale_kernel<true, SrfFrames>), grid, dim3(256), 0, (hipStream_t)stream, out, bias, stats, wav, mc, S, T,
                       lens);
  else
    hipLaunchKernelGGL((srf_bias_rescale_kernel<false, SrfFrames>), grid, dim3(256), 0, (hipStream_t)stream, out, bias, stats, wav, 0, S, T,
                       lens);
  SRF_CHECK_LAUNCH("bias_rescale_ragged", stream);
  return SRF_OK;
}
extern "C" int srf_bias_rescale_ragged(float* out, const float* bias, const float* stats, const float* wav, int mc, int Bt, int S, int T,
                                       const int* lengths, void* stream) {
  SRF_CHECK_ARG(out && bias && Bt > 0 && S > 0 && T > 0, "srf_bias_rescale_ragged: bad arguments");
  SRF_CHECK_ARG(!stats || !mc || wav, "srf_bias_rescale_ragged: mixture consistency needs the raw mixture");
  SrfFrames lens;
  const int rc = srf_frames_table("srf_bias_rescale_ragged", lengths, Bt, T, &lens);
  if (rc) return rc;
  return srf_bias_rescale_ragged_launch(out, bias, stats, wav, mc, Bt, S, T, lens, stream);
}

// ---------------------------------------------------------------------------------------------
// plan
// ---------------------------------------------------------------------------------------------
extern "C" int srf_original_plan_create(const srf_config* base, int batch, int T, srf_plan** out) {
  SRF_CHECK_ARG(base && out, "srf_original_plan_create: null pointer");
  *out = nullptr;
  const srf_config& c = *base;
  SRF_CHECK_ARG(batch > 0 && T > 0, "srf_original_plan_create: batch and T must be positive");
  SRF_CHECK_ARG(c.out_channels > 0 && c.in_channels > 0 && c.num_blocks > 0 && c.enc_num_basis > 0 && c.num_sources > 0,
                "srf_original_plan_create: non-positive model dimension");
  SRF_CHECK_ARG(c.in_audio_channels == 1 && c.group_size == 1,
                "srf_original_plan_create: in_audio_channels and group_size must be 1 (got %d, %d)", c.in_audio_channels, c.group_size);
  SRF_CHECK_ARG(c.enc_num_basis % 2 == 0,
                "srf_original_plan_create: enc_num_basis = %d is odd: the mask layer then has enc_num_basis + 1 rows (the reference's "
                "own mask multiply fails there)", c.enc_num_basis);
  SRF_CHECK_ARG(c.upsampling_depth >= 1 && c.upsampling_depth <= SRF_MAX_DEPTH,
                "srf_original_plan_create: upsampling_depth %d unsupported (1..%d)", c.upsampling_depth, SRF_MAX_DEPTH);
  SRF_CHECK_ARG(c.enc_kernel_size >= 3 && (c.enc_kernel_size & 1), "srf_original_plan_create: enc_kernel_size must be odd and >= 3 (got %d)",
                c.enc_kernel_size);
  SRF_CHECK_ARG(c.num_sources <= SRF_SOFTMAX_MASK_MAX_SOURCES,
                "srf_original_plan_create: num_sources = %d exceeds SRF_SOFTMAX_MASK_MAX_SOURCES = %d (srf_softmax_mask)", c.num_sources,
                SRF_SOFTMAX_MASK_MAX_SOURCES);
  const int D = c.upsampling_depth, U = c.num_blocks, K = c.enc_kernel_size, N = c.enc_num_basis, h = K / 2, S = c.num_sources;
  const int B = c.out_channels, C = c.in_channels;
  const long Tp = orig_padded_length(T, h, D);
  SRF_CHECK_ARG(Tp <= (1L << 30), "srf_original_plan_create: T = %d too long", T);
  const long L = (Tp + 2 * h - K) / h + 1;
  SRF_CHECK_ARG(L % (1L << (D - 1)) == 0,
                "srf_original_plan_create: enc_kernel_size = %d, upsampling_depth = %d: %ld frames are not a multiple of 2^(D-1) (the "
                "reference's upsample-and-add fails there too)", K, D, L);
  SRF_CHECK_ARG(batch <= 65535, "srf_original_plan_create: batch %d too large (max 65535 per call)", batch);
  // what the encoder's window and the overlap-add's frame tile ask of LDS (64 KB): refused here, not at their launches
  SRF_CHECK_ARG(64 + sizeof(float) * (size_t)(63 * h + K) <= 64 * 1024 && (long)c.num_sources * K <= 4096,
                "srf_original_plan_create: enc_kernel_size = %d (x num_sources = %d) exceeds the encoder's / overlap-add's LDS tiles", K,
                c.num_sources);
  srf_plan* p = new (std::nothrow) srf_plan();
  SRF_CHECK_ARG(p != nullptr, "srf_original_plan_create: out of host memory");
  p->cfg = c;
  p->cfg.variant = SRF_VARIANT_ORIGINAL;
  p->A = 1;
  p->Bt = p->Bg = batch;
  p->T = T;
  p->Tp = (int)Tp;
  p->L = (int)L;
  p->SA = S;
  p->nB = B;
  p->nC = C;
  p->p_block0 = SRF_PO_FRONT;
  p->p_ublock_off = 0;
  p->p_block_stride = orig_block_params(D);
  p->p_tail = p->p_block0 + U * p->p_block_stride;
  p->n_params = p->p_tail + (B != N ? 2 : 0) + SRF_PO_TAIL;
  p->slots_per_block = orig_slots_per_block(D);
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
  p->off_xa = take(F * batch * B * L);
  p->off_xb = p->off_xq = p->off_xu = 0;
  p->off_orig_g = take(F * batch * B * L);
  p->off_orig_gx = take(F * batch * B * L);
  p->off_y1 = take(F * batch * C * L);
  p->off_orig_act = take(F * batch * C * L);
  for (int k = 0; k < D; ++k) p->off_lv[k] = take(F * batch * C * (L >> k));
  p->off_orig_xr = B != N ? take(F * batch * N * L) : 0;
  p->off_orig_z = take(F * batch * S * N * L);
  p->off_masked = take(F * batch * S * N * L);
  p->off_dec = take(F * srf_decoder_scratch_floats(batch, S * N, S, K, p->L));
  p->off_orig_tz = take(F * orig_tz_floats(S, N));
  p->off_orig_wdec = take(F * (size_t)S * N * S * K);
  // the fused pyramid takes its input without a lazy norm (in_norm = NULL: the materialised activation as it is)
  p->fused_pyramid = srf_pyramid_supported(C, p->L, D);   // (evaluated with the default debug flags)
  p->off_pyr = p->fused_pyramid ? take(srf_pyramid_scratch_bytes(batch, C, p->L, D)) : 0;
  p->off_wdpack = 0;
  // packed (split-bf16) images for the 256 x 128 GEMM, where it takes the shape; the image on m.weight's index is the Toeplitz weight's
  p->pk_of_param.assign(p->n_params, 0);
  plan_add_pack(p, &off, SRF_PO_L1, B, N);
  for (int i = 0; i < U; ++i) {
    plan_add_pack(p, &off, orig_p_proj(p, i), C, B);
    plan_add_pack(p, &off, orig_p_exp(p, i), B, C);
  }
  if (B != N) plan_add_pack(p, &off, orig_p_reshape(p), N, B);
  plan_add_pack(p, &off, orig_p_mask(p), S * N, N);
  p->total_bytes = off;
  // (the pyramid: three launches fused, D + 1 level by level -- as the default kernel mode and debug flags run it)
  p->n_launches = 1 /*zero*/ + 2 /*mask weight, decoder weight*/ + (p->pk_param.empty() ? 0 : 1) /*pack*/ + 2 +
                  U * ((p->fused_pyramid ? 3 : D + 1) + 6) + (B != N ? 1 : 0) + 2 /*mask GEMM, softmax*/ + 4 /*decoder*/ + 1 /*bias*/;
  *out = p;
  return SRF_OK;
}

// ---------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------
// ---- the two weights this model needs in another form: the mask layer as a [S N, N] GEMM weight, the grouped decoder's as a
// block-diagonal one
int srf_original_weight_forms(const srf_plan* p, const float* const* P, float* tz, float* wdec, void* stream) {
  const int N = p->cfg.enc_num_basis, S = p->cfg.num_sources;
  const SrfOrigTail t = orig_tail(p, P);
  const int rc = srf_mask_weight_fill(t.m_w, t.m_b, tz, tz + orig_tz_bias_at(S, N), N, S, stream);
  if (rc) return rc;
  return srf_decoder_weight_expand(t.dec_w, wdec, N, S, p->cfg.enc_kernel_size, stream);
}

// the inference forward (rg: a ragged batch): one set of tensors in the plan's workspace, the plan's packed images
int srf_original_forward(const srf_plan* p, const float* const* P, const float* wav, float* out, void* workspace,
                         const float* wav_stats, int mixture_consistency, void* stream, const Ragged* rg) {
  char* ws = (char*)workspace;
  auto fptr = [&](size_t o) { return (float*)(ws + o); };
  SrfOrigAddrs a{};
  a.stats = (double*)(ws + p->off_stats);
  a.enc = fptr(p->off_enc);
  a.x = ws + p->off_xa, a.blk = ws;      // (strides 0)
  a.o_y1 = a.o_m = p->off_y1, a.o_g = p->off_orig_g, a.o_gx = p->off_orig_gx;
  for (int k = 0; k < p->cfg.upsampling_depth; ++k) a.o_lv[k] = p->off_lv[k];
  a.act = fptr(p->off_orig_act), a.xr = fptr(p->off_orig_xr), a.z = fptr(p->off_orig_z), a.masked = fptr(p->off_masked);
  a.dec = fptr(p->off_dec), a.tz = fptr(p->off_orig_tz), a.wdec = fptr(p->off_orig_wdec);
  a.pyr = ws + p->off_pyr;
  // (a ragged batch runs what srf_original_ragged_supported has made sure of: packed weights, the register-resident fused pyramid)
  const bool use_pack = rg || plan_use_pack(p);
  const int i_m = orig_p_mask(p);
  auto pack = [&](const float* tz) -> int {
    return use_pack ? plan_pack_weights(p, [&](int param) -> const float* { return param == i_m ? tz : P[param]; }, ws, stream) : SRF_OK;
  };
  auto conv = [&](const float* x, const float* w, int param, const float* bias, float* y, int Cin, int Cout, const srf_norm* in_norm,
                  double* out_sums) {
    return orig_conv(rg, x, w, plan_packed(p, ws, use_pack, param), bias, y, p->Bt, Cin, Cout, p->L, in_norm, out_sums, stream);
  };
  return orig_walk(p, P, wav, out, a, pack, conv, rg || plan_fused_pyramid_now(p), rg, wav_stats, mixture_consistency, stream);
}

// ---------------------------------------------------------------------------------------------
// ragged forward (opt-in: srf_plan_ragged_supported / srf_forward_ragged / srf_separate_ragged keep refusing an original plan)
// ---------------------------------------------------------------------------------------------
// the gate: whether the walk above, with a frames table, has a ragged kernel for every step of this plan -- now, under the current
// kernel mode and debug flags
static bool orig_ragged_now(const srf_plan* p, const char** why) {
  auto no = [&](const char* w) {
    if (why) *why = w;
    return false;
  };
  if (p->cfg.variant != SRF_VARIANT_ORIGINAL) return no("not a plan of srf_original_plan_create");
  const srf_config& c = p->cfg;
  const int D = c.upsampling_depth, N = c.enc_num_basis, S = c.num_sources, B = p->nB, C = p->nC, L = p->L, Bt = p->Bt;
  if (c.enc_kernel_size != 21) return no("the ragged encoder is the K = 21 kernel");
  if (Bt > SRF_RAGGED_MAX_BATCH) return no("the batch exceeds SRF_RAGGED_MAX_BATCH");
  if (S > 16) return no("more than 16 sources");
  if (srf_kernel_mode() != 0 || !plan_use_pack(p)) return no("the forward does not run the packed 256 x 128 GEMMs (kernel mode / debug flags / shapes)");
  if (srf_dbg(SRF_DBG_NO_GEMM_256)) return no("the 256 x 128 GEMM is switched off (debug flags)");
  // every conv of the walk on the 256 x 128 kernel: shape, 32-bit reach of its input, at least 8 tiles
  auto takes = [&](int Cin, int Cout) {
    return srf_x3w_shape_supported(Cin, Cout, L) && (long)Bt * Cin * L * 4 < (1L << 31) &&
           (long)Bt * ((Cout + 255) / 256) * ((L + 127) / 128) >= 8;
  };
  if (!takes(N, B)) return no("l1's shape is outside the 256 x 128 GEMM (or too few tiles)");
  if (!takes(B, C)) return no("proj_1x1's shape is outside the 256 x 128 GEMM (or too few tiles)");
  if (!takes(C, B)) return no("conv_1x1_exp's shape is outside the 256 x 128 GEMM (needs at least 192 output channels; or too few tiles)");
  if (orig_has_reshape(p) && !takes(B, N)) return no("reshape_before_masks' shape is outside the 256 x 128 GEMM (or too few tiles)");
  if (!takes(N, S * N)) return no("the mask GEMM's shape is outside the 256 x 128 GEMM (or too few tiles)");
  if (!plan_fused_pyramid_now(p) || srf_dbg(SRF_DBG_PYR_NO_REG) || !srf_pyramid_reg_supported(L, D))
    return no("the forward does not run the register-resident fused pyramid at this length");
  return true;
}
extern "C" int srf_original_ragged_supported(const srf_plan* p) { return p && orig_ragged_now(p, nullptr) ? 1 : 0; }
extern "C" size_t srf_original_ragged_workspace_bytes(const srf_plan* p) { return p && orig_ragged_now(p, nullptr) ? p->total_bytes : 0; }

// What the two entry points (`who`) share: the gate, the argument checks and every example's own padded length, as its batch-1
// plan would have it -- all refusals BEFORE the first launch
static int orig_ragged_prepare(const char* who, const srf_plan* p, const float* const* P, int num_params, const int* lengths,
                               const void* workspace, size_t workspace_bytes, Ragged* rg) {
  const char* why = "";
  SRF_CHECK_ARG(orig_ragged_now(p, &why), "%s: plan not supported by the original model's ragged forward: %s", who, why);
  // (the entry checks' messages carry the suffix; the gate's above and the tables' below do not.  `who` is one of the two entry
  // points' names below, 28 characters at the most: nothing is cut)
  char who_original[64];
  snprintf(who_original, sizeof(who_original), "%s (original)", who);
  int rc = forward_check_args(who_original, true /* checked by the caller */, p, P, num_params, workspace, workspace_bytes);
  if (rc) return rc;
  const int D = p->cfg.upsampling_depth, h = p->cfg.enc_kernel_size / 2;
  rg->lengths = lengths;
  for (int b = 0; b < p->Bt; ++b) {
    SRF_CHECK_ARG(lengths[b] >= 1 && lengths[b] <= p->T, "%s (original): example %d has length %d (allowed: 1..%d)", who, b, lengths[b],
                  p->T);
    // the example alone, padded by the model's own rule
    rg->frames[b] = (int)(orig_padded_length(lengths[b], h, D) / h);
    SRF_CHECK_ARG(srf_pyramid_ragged_frames_ok(rg->frames[b], p->L, D),
                  "%s (original): example %d (length %d = %d frames) is too short for the fused pyramid or off its chunk grid", who, b,
                  lengths[b], rg->frames[b]);
  }
  rc = srf_frames_table(who, lengths, p->Bt, p->T, &rg->lens_t);
  if (rc) return rc;
  return srf_frames_table(who, rg->frames, p->Bt, p->L, &rg->frames_t);
}

extern "C" int srf_original_forward_ragged(const srf_plan* p, const float* const* P, int num_params, const float* wav, const int* lengths,
                                           float* out, void* workspace, size_t workspace_bytes, void* stream) {
  SRF_CHECK_ARG(p && P && wav && lengths && out && workspace, "srf_original_forward_ragged: null pointer");
  Ragged rg;
  const int rc = orig_ragged_prepare("srf_original_forward_ragged", p, P, num_params, lengths, workspace, workspace_bytes, &rg);
  if (rc) return rc;
  if (srf_profiling()) srf_prof_mark("(gap)", (hipStream_t)stream);
  return srf_original_forward(p, P, wav, out, workspace, nullptr, 0, stream, &rg);
}

// srf_separate over a ragged batch: the ragged forward with a statistics launch over every row's own samples in front, the
// normalisation in the ragged encoder's load and the rescale (+ mixture consistency) in the ragged srf_bias_rescale.  wav: the RAW
// padded mixture; nothing at or past lengths[b] is read by any of the three.
extern "C" int srf_original_separate_ragged(const srf_plan* p, const float* const* P, int num_params, const float* wav,
                                            const int* lengths, float* out, float* stats, int mixture_consistency, void* workspace,
                                            size_t workspace_bytes, void* stream) {
  SRF_CHECK_ARG(p && P && wav && lengths && out && stats && workspace, "srf_original_separate_ragged: null pointer");
  Ragged rg;
  int rc = orig_ragged_prepare("srf_original_separate_ragged", p, P, num_params, lengths, workspace, workspace_bytes, &rg);
  if (rc) return rc;
  if (srf_profiling()) srf_prof_mark("(gap)", (hipStream_t)stream);
  rc = srf_wav_stats_ragged_launch(wav, rg.lens_t, stats, p->Bt, p->T, (hipStream_t)stream);
  if (rc) return rc;
  return srf_original_forward(p, P, wav, out, workspace, stats, mixture_consistency, stream, &rg);
}

