// K3 -- depthwise k=5 Conv1d (stride 1|2, padding 2, groups=C) with the PREVIOUS GlobLN (+PReLU)
//       applied on load and the {sum,sumsq} of the output produced for the NEXT GlobLN
//       (reference: DilatedConvNorm improved_sudormrf.py:138-159 as used in UConvBlock :178-189,
//        :206-211; the conv zero-pads the *normalised* tensor, so out-of-range taps contribute 0).
// K4 -- bottom-up nearest-x2 upsample + add over the D normalised levels (:190-194, :214-216), each
//       level's GlobLN applied on load, {sum,sumsq} of the merged tensor produced for final_norm.
//
// Both are pure HBM streaming kernels (<= 5 MAC per 4-byte element).  Fast paths: one wavefront per
// (batch,channel) row, 16-B loads/stores along time, halo exchange between neighbouring lanes with
// wavefront shuffles (no LDS round trip), next chunk prefetched while the current one is computed,
// per-channel scale/shift/taps wave-uniform.  Generic paths: one thread per output element.
#include "srf_plan.h"

__device__ __forceinline__ void srf_wave_stats_atomic(double s, double q, double* dst) {
  s = srf_wave_sum(s);
  q = srf_wave_sum(q);
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(dst, s);
    atomicAdd(dst + 1, q);
  }
}

struct RowCoef {
  float sc, sh, slope;
  bool act;
};

__device__ __forceinline__ RowCoef srf_row_coef(const SrfNormDev& nrm, long g, int c, double inv_count) {
  RowCoef rc{1.f, 0.f, 1.f, false};
  if (nrm.sums) {
    float mean, rstd;
    srf_finalize_stats(nrm.sums, g, inv_count, mean, rstd);
    rc.sc = nrm.gamma[c] * rstd;
    rc.sh = nrm.beta[c] - mean * rc.sc;
  }
  if (nrm.prelu) {
    rc.act = true;
    rc.slope = nrm.prelu[0];
  }
  return rc;
}

__device__ __forceinline__ float srf_tf(float v, const RowCoef& rc) {
  v = fmaf(v, rc.sc, rc.sh);
  if (rc.act) v = srf_prelu(v, rc.slope);
  return v;
}

__device__ __forceinline__ float4 srf_tf4(float4 v, const RowCoef& rc) {
  v.x = srf_tf(v.x, rc);
  v.y = srf_tf(v.y, rc);
  v.z = srf_tf(v.z, rc);
  v.w = srf_tf(v.w, rc);
  return v;
}

__device__ __forceinline__ float srf_tap5(float bs, float w0, float w1, float w2, float w3, float w4,
                                          float x0, float x1, float x2, float x3, float x4) {
  return fmaf(w4, x4, fmaf(w3, x3, fmaf(w2, x2, fmaf(w1, x1, fmaf(w0, x0, bs)))));
}

// ---------------------------------------------------------------------------------------------
// depthwise conv, generic: block = (row, chunk of 256 outputs), thread = one output
// RAGGED (srf_dwconv5_ragged; FR = SrfFrames): Lin and Lout stay the row strides, example b is in_frames[b] columns long.  x is
// not read at columns >= in_frames[b] (the taps meet literal zeros there), the on-load norm counts C * in_frames[b], y is exact
// 0 from its own output length on and out_sums run over its own outputs.
// ---------------------------------------------------------------------------------------------
template <typename... FR>
__global__ __launch_bounds__(256) void srf_dwconv5_generic_kernel(
    const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
    float* __restrict__ y, SrfNormDev nrm, double inv_count, double* __restrict__ out_sums, int C,
    int Lin, int Lout, int stride, int chunks, FR... fr) {
  constexpr bool RAGGED = sizeof...(FR) != 0;
  __shared__ double red[8];
  const long row = blockIdx.x / chunks;
  const int chunk = blockIdx.x - row * chunks;
  const int c = (int)(row % C);
  const long b = row / C;
  int own_in = Lin, own_out = Lout;      // (RAGGED) the example's own input and output columns
  if constexpr (RAGGED) {
    own_in = srf_frames_of((int)b, fr...);
    own_out = (own_in - 1) / stride + 1;
    inv_count = 1.0 / ((double)C * (double)own_in);
  }
  const RowCoef rc = srf_row_coef(nrm, b, c, inv_count);
  const int j = chunk * 256 + threadIdx.x;
  double ds = 0.0, dq = 0.0;
  if (j < own_out) {
    const float* xr = x + (size_t)row * Lin;
    float acc = bias[c];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const int i = stride * j + k - 2;
      const float v = (i >= 0 && i < own_in) ? srf_tf(xr[i], rc) : 0.f;
      acc = fmaf(w[c * 5 + k], v, acc);
    }
    y[(size_t)row * Lout + j] = acc;
    ds = (double)acc;
    dq = (double)acc * (double)acc;
  } else if constexpr (RAGGED) {
    if (j < Lout) y[(size_t)row * Lout + j] = 0.f;
  }
  if (out_sums) srf_block_stats_atomic<4>(ds, dq, srf_stat_slot(out_sums, b, blockIdx.x), red);
}

// ---------------------------------------------------------------------------------------------
// depthwise conv, fast: one wavefront per row; requires Lin % (4*STRIDE) == 0, 16-B aligned bases
// RAGGED (FR = SrfFrames; every in_frames[b] % (4*STRIDE) == 0 too): the row's own float4 groups take the place of the row's,
// and the output groups between the example's own end and the row stride are stored as zeros.
// ---------------------------------------------------------------------------------------------
template <int STRIDE, typename... FR>
__global__ __launch_bounds__(256) void srf_dwconv5_fast_kernel(
    const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
    float* __restrict__ y, SrfNormDev nrm, double inv_count, double* __restrict__ out_sums, int C,
    int Lin, int Lout, long rows, FR... fr) {
  constexpr bool RAGGED = sizeof...(FR) != 0;
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (row >= rows) return;  // wave-uniform; no block-level barrier below
  const int c = (int)(row % C);
  const long b = row / C;
  int own_in = Lin;      // (RAGGED) the example's own input columns
  if constexpr (RAGGED) {
    own_in = srf_frames_of((int)b, fr...);
    inv_count = 1.0 / ((double)C * (double)own_in);
  }
  const RowCoef rc = srf_row_coef(nrm, b, c, inv_count);
  const float w0 = w[c * 5 + 0], w1 = w[c * 5 + 1], w2 = w[c * 5 + 2], w3 = w[c * 5 + 3],
              w4 = w[c * 5 + 4];
  const float bs = bias[c];
  const float4* xr = reinterpret_cast<const float4*>(x + (size_t)row * Lin);
  float4* yr = reinterpret_cast<float4*>(y + (size_t)row * Lout);
  const int nin4 = own_in >> 2, nout4 = RAGGED ? (own_in / STRIDE) >> 2 : Lout >> 2;
  const int nchunks = ((Lout >> 2) + 63) >> 6;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  double ds = 0.0, dq = 0.0;
  float cz = 0.f, cw = 0.f;  // last two (transformed) inputs of the previous chunk = left halo of lane 0

  if (STRIDE == 1) {
    // prefetches are unconditional loads from a clamped index, zeroed afterwards by a select (a
    // "cond ? load : 0" makes hipcc branch around the load and drain vmcnt(0): no prefetch at all)
    float4 nxt = srf_tf4(xr[min(lane, nin4 - 1)], rc);
    if (lane >= nin4) nxt = zero4;
    for (int it = 0; it < nchunks; ++it) {
      const float4 cur = nxt;
      const int g = it * 64 + lane;
      nxt = srf_tf4(xr[min(g + 64, nin4 - 1)], rc);
      if (g + 64 >= nin4) nxt = zero4;
      float lz = __shfl_up(cur.z, 1, 64), lw = __shfl_up(cur.w, 1, 64);
      float rx = __shfl_down(cur.x, 1, 64), ry = __shfl_down(cur.y, 1, 64);
      const float nx0 = __shfl(nxt.x, 0, 64), ny0 = __shfl(nxt.y, 0, 64);
      if (lane == 0) {
        lz = cz;
        lw = cw;
      }
      if (lane == 63) {
        rx = nx0;
        ry = ny0;
      }
      cz = __shfl(cur.z, 63, 64);
      cw = __shfl(cur.w, 63, 64);
      if (g < nout4) {
        float4 o;
        o.x = srf_tap5(bs, w0, w1, w2, w3, w4, lz, lw, cur.x, cur.y, cur.z);
        o.y = srf_tap5(bs, w0, w1, w2, w3, w4, lw, cur.x, cur.y, cur.z, cur.w);
        o.z = srf_tap5(bs, w0, w1, w2, w3, w4, cur.x, cur.y, cur.z, cur.w, rx);
        o.w = srf_tap5(bs, w0, w1, w2, w3, w4, cur.y, cur.z, cur.w, rx, ry);
        yr[g] = o;
        const float s = (o.x + o.y) + (o.z + o.w);
        const float q = fmaf(o.x, o.x, fmaf(o.y, o.y, fmaf(o.z, o.z, o.w * o.w)));
        ds += (double)s;
        dq += (double)q;
      } else if constexpr (RAGGED) {
        if (g < (Lout >> 2)) yr[g] = zero4;
      }
    }
  } else {
    // output group g (4 outputs j0..j0+3, j0 = 4g) needs inputs 2*j0-2 .. 2*j0+8:
    // float4 A = in[2g], B = in[2g+1], left halo = left neighbour's (B.z,B.w), right = right's A.x
    float4 nA = srf_tf4(xr[min(2 * lane, nin4 - 1)], rc);
    float4 nB = srf_tf4(xr[min(2 * lane + 1, nin4 - 1)], rc);
    if (2 * lane >= nin4) nA = zero4;
    if (2 * lane + 1 >= nin4) nB = zero4;
    for (int it = 0; it < nchunks; ++it) {
      const float4 cA = nA, cB = nB;
      const int g = it * 64 + lane;
      const int gn = g + 64;
      nA = srf_tf4(xr[min(2 * gn, nin4 - 1)], rc);
      nB = srf_tf4(xr[min(2 * gn + 1, nin4 - 1)], rc);
      if (2 * gn >= nin4) nA = zero4;
      if (2 * gn + 1 >= nin4) nB = zero4;
      float lz = __shfl_up(cB.z, 1, 64), lw = __shfl_up(cB.w, 1, 64);
      float rx = __shfl_down(cA.x, 1, 64);
      const float nx0 = __shfl(nA.x, 0, 64);
      if (lane == 0) {
        lz = cz;
        lw = cw;
      }
      if (lane == 63) rx = nx0;
      cz = __shfl(cB.z, 63, 64);
      cw = __shfl(cB.w, 63, 64);
      if (g < nout4) {
        float4 o;
        o.x = srf_tap5(bs, w0, w1, w2, w3, w4, lz, lw, cA.x, cA.y, cA.z);
        o.y = srf_tap5(bs, w0, w1, w2, w3, w4, cA.x, cA.y, cA.z, cA.w, cB.x);
        o.z = srf_tap5(bs, w0, w1, w2, w3, w4, cA.z, cA.w, cB.x, cB.y, cB.z);
        o.w = srf_tap5(bs, w0, w1, w2, w3, w4, cB.x, cB.y, cB.z, cB.w, rx);
        yr[g] = o;
        const float s = (o.x + o.y) + (o.z + o.w);
        const float q = fmaf(o.x, o.x, fmaf(o.y, o.y, fmaf(o.z, o.z, o.w * o.w)));
        ds += (double)s;
        dq += (double)q;
      } else if constexpr (RAGGED) {
        if (g < (Lout >> 2)) yr[g] = zero4;
      }
    }
  }
  if (out_sums) srf_wave_stats_atomic(ds, dq, srf_stat_slot(out_sums, b, row));
}

extern "C" int srf_dwconv5(const float* x, const float* w, const float* bias, float* y, int Bt, int C,
                           int Lin, int stride, const srf_norm* in_norm, double* out_sums,
                           void* stream) {
  SRF_CHECK_ARG(x && w && bias && y, "srf_dwconv5: null pointer");
  SRF_CHECK_ARG(Bt > 0 && C > 0 && Lin > 0, "srf_dwconv5: bad sizes");
  SRF_CHECK_ALIGNED16("srf_dwconv5", {"in_norm.sums", in_norm ? in_norm->sums : nullptr});     // (read as pairs of doubles)
  SRF_CHECK_ARG(stride == 1 || stride == 2, "srf_dwconv5: stride must be 1 or 2 (got %d)", stride);
  const int Lout = (Lin - 1) / stride + 1;
  const long rows = (long)Bt * C;
  const double inv_count = 1.0 / ((double)C * (double)Lin);
  SrfNormDev nd = srf_norm_dev(in_norm);
  hipStream_t st = (hipStream_t)stream;
  const bool fast = srf_kernel_mode() != 1 && (Lin % (4 * stride) == 0) && srf_aligned16(x) &&
                    srf_aligned16(y) && rows < (1L << 32);
  if (fast) {
    const unsigned blocks = (unsigned)((rows + 3) / 4);
    if (stride == 1)
      hipLaunchKernelGGL(srf_dwconv5_fast_kernel<1>, dim3(blocks), dim3(256), 0, st, x, w, bias, y, nd,
                         inv_count, out_sums, C, Lin, Lout, rows);
    else
      hipLaunchKernelGGL(srf_dwconv5_fast_kernel<2>, dim3(blocks), dim3(256), 0, st, x, w, bias, y, nd,
                         inv_count, out_sums, C, Lin, Lout, rows);
  } else {
    const int chunks = (Lout + 255) / 256;
    const long blocks = rows * chunks;
    SRF_CHECK_ARG(blocks < (1L << 31), "srf_dwconv5: tensor too large");
    hipLaunchKernelGGL(srf_dwconv5_generic_kernel<>, dim3((unsigned)blocks), dim3(256), 0, st, x, w, bias,
                       y, nd, inv_count, out_sums, C, Lin, Lout, stride, chunks);
  }
  SRF_CHECK_LAUNCH(fast ? (stride == 1 ? "dwconv5_s1_fast" : "dwconv5_s2_fast") : "dwconv5_generic", st);
  return SRF_OK;
}

// The ragged form: srf_dwconv5's kernels with the table of input lengths behind their arguments.  The fast kernels serve a batch
// whose every in_frames[b] lies on their grid of 4 * stride columns, the generic kernel any other.
extern "C" int srf_dwconv5_ragged(const float* x, const float* w, const float* bias, float* y, int Bt, int C, int Lin, int stride,
                                  const srf_norm* in_norm, double* out_sums, const int* in_frames, void* stream) {
  SRF_CHECK_ARG(x && w && bias && y, "srf_dwconv5_ragged: null pointer");
  SRF_CHECK_ARG(Bt > 0 && C > 0 && Lin > 0, "srf_dwconv5_ragged: bad sizes");
  SRF_CHECK_ALIGNED16("srf_dwconv5_ragged", {"in_norm.sums", in_norm ? in_norm->sums : nullptr});
  SRF_CHECK_ARG(stride == 1 || stride == 2, "srf_dwconv5_ragged: stride must be 1 or 2 (got %d)", stride);
  SRF_CHECK_ARG(stride == 1 || Lin % 2 == 0, "srf_dwconv5_ragged: stride 2 needs an even row stride (Lin = %d)", Lin);
  SrfFrames fr;
  const int rc = srf_frames_table("srf_dwconv5_ragged", in_frames, Bt, Lin, &fr);
  if (rc) return rc;
  bool grid = true;      // every example on the fast kernels' grid
  for (int b = 0; b < Bt; ++b) {
    SRF_CHECK_ARG(stride == 1 || in_frames[b] % 2 == 0, "srf_dwconv5_ragged: example %d has %d input frames: stride 2 needs an even count",
                  b, in_frames[b]);
    grid = grid && in_frames[b] % (4 * stride) == 0;
  }
  const int Lout = (Lin - 1) / stride + 1;
  const long rows = (long)Bt * C;
  const double inv_count = 1.0 / ((double)C * (double)Lin);      // (the kernels count the example's own columns)
  SrfNormDev nd = srf_norm_dev(in_norm);
  hipStream_t st = (hipStream_t)stream;
  const bool fast = srf_kernel_mode() != 1 && (Lin % (4 * stride) == 0) && grid && srf_aligned16(x) && srf_aligned16(y);
  if (fast) {
    const unsigned blocks = (unsigned)((rows + 3) / 4);
    if (stride == 1)
      hipLaunchKernelGGL((srf_dwconv5_fast_kernel<1, SrfFrames>), dim3(blocks), dim3(256), 0, st, x, w, bias, y, nd, inv_count, out_sums,
                         C, Lin, Lout, rows, fr);
    else
      hipLaunchKernelGGL((srf_dwconv5_fast_kernel<2, SrfFrames>), dim3(blocks), dim3(256), 0, st, x, w, bias, y, nd, inv_count, out_sums,
                         C, Lin, Lout, rows, fr);
  } else {
    const int chunks = (Lout + 255) / 256;
    const long blocks = rows * chunks;
    SRF_CHECK_ARG(blocks < (1L << 31), "srf_dwconv5_ragged: tensor too large");
    hipLaunchKernelGGL(srf_dwconv5_generic_kernel<SrfFrames>, dim3((unsigned)blocks), dim3(256), 0, st, x, w, bias, y, nd, inv_count,
                       out_sums, C, Lin, Lout, stride, chunks, fr);
  }
  SRF_CHECK_LAUNCH(fast ? (stride == 1 ? "dwconv5_s1_fast_ragged" : "dwconv5_s2_fast_ragged") : "dwconv5_generic_ragged", st);
  return SRF_OK;
}

// ---------------------------------------------------------------------------------------------
// merge (upsample-add over D levels)
// ---------------------------------------------------------------------------------------------
struct MergeArgs {
  const float* lv[SRF_MAX_DEPTH];
  SrfNormDev nrm[SRF_MAX_DEPTH];
  double inv_count[SRF_MAX_DEPTH];
  int D;
};

// RAGGED (srf_merge_ragged; FR = SrfFrames): L stays the level-0 row stride, example b is frames[b] columns long on level 0 (a
// multiple of 2^(D-1)) and frames[b] >> k on level k, whose norm counts C * (frames[b] >> k); no level is read past its own end,
// y is exact 0 on [frames[b], L) and out_sums run over the example's own columns.
template <typename... FR>
__global__ __launch_bounds__(256) void srf_merge_generic_kernel(MergeArgs a, float* __restrict__ y,
                                                                double* __restrict__ out_sums, int C,
                                                                int L, int chunks, FR... fr) {
  constexpr bool RAGGED = sizeof...(FR) != 0;
  __shared__ double red[8];
  const long row = blockIdx.x / chunks;
  const int chunk = blockIdx.x - row * chunks;
  const int c = (int)(row % C);
  const long b = row / C;
  const int j = chunk * 256 + threadIdx.x;
  int own = L;      // (RAGGED) the example's own level-0 columns
  if constexpr (RAGGED) own = srf_frames_of((int)b, fr...);
  double ds = 0.0, dq = 0.0;
  RowCoef rcs[SRF_MAX_DEPTH];  // statistics are finalised by the whole (converged) wavefront
#pragma unroll
  for (int k = 0; k < SRF_MAX_DEPTH; ++k) {
    SrfNormDev nk = a.nrm[k];
    nk.prelu = nullptr;
    if (k >= a.D) nk.sums = nullptr;
    rcs[k] = srf_row_coef(nk, b, c, RAGGED ? 1.0 / ((double)C * (double)max(own >> k, 1)) : a.inv_count[k]);
  }
  if (RAGGED && j >= own) {
    if (j < L) y[(size_t)row * L + j] = 0.f;
  } else if (j < L) {
    float t = 0.f;
#pragma unroll
    for (int k = SRF_MAX_DEPTH - 1; k >= 0; --k) {
      if (k < a.D) {
        const int Lk = L >> k;
        const float v = srf_tf(a.lv[k][(size_t)row * Lk + (j >> k)], rcs[k]);
        t = (k == a.D - 1) ? v : v + t;
      }
    }
    y[(size_t)row * L + j] = t;
    ds = (double)t;
    dq = (double)t * (double)t;
  }
  if (out_sums) srf_block_stats_atomic<4>(ds, dq, srf_stat_slot(out_sums, b, blockIdx.x), red);
}

// fast: one wavefront per row, lane = one float4 of level-0 output; level 1 as float2, deeper levels
// as (lane-shared) dwords.  Requires L % 4 == 0 and L % 2^(D-1) == 0, aligned bases.
// RAGGED (every frames[b] % 4 == 0 too): the example's own float4 groups, then zeros up to the row stride.
template <typename... FR>
__global__ __launch_bounds__(256) void srf_merge_fast_kernel(MergeArgs a, float* __restrict__ y,
                                                             double* __restrict__ out_sums, int C, int L,
                                                             long rows, FR... fr) {
  constexpr bool RAGGED = sizeof...(FR) != 0;
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (row >= rows) return;
  const int c = (int)(row % C);
  const long b = row / C;
  const int D = a.D;
  int own = L;      // (RAGGED) the example's own level-0 columns
  if constexpr (RAGGED) own = srf_frames_of((int)b, fr...);
  float sc[SRF_MAX_DEPTH], sh[SRF_MAX_DEPTH];
#pragma unroll
  for (int k = 0; k < SRF_MAX_DEPTH; ++k) {
    sc[k] = 1.f;
    sh[k] = 0.f;
    if (k < D) {
      SrfNormDev nk = a.nrm[k];
      nk.prelu = nullptr;
      const RowCoef rc = srf_row_coef(nk, b, c, RAGGED ? 1.0 / ((double)C * (double)max(own >> k, 1)) : a.inv_count[k]);
      sc[k] = rc.sc;
      sh[k] = rc.sh;
    }
  }
  const float4* l0 = reinterpret_cast<const float4*>(a.lv[0] + (size_t)row * L);
  const float2* l1 = (D > 1) ? reinterpret_cast<const float2*>(a.lv[1] + (size_t)row * (L >> 1)) : nullptr;
  float4* yr = reinterpret_cast<float4*>(y + (size_t)row * L);
  const int n4 = own >> 2;
  double ds = 0.0, dq = 0.0;
  if constexpr (RAGGED)
    for (int g = n4 + lane; g < (L >> 2); g += 64) yr[g] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int g = lane; g < n4; g += 64) {
    const float4 d0 = l0[g];
    // levels >= 2 are constant over this lane's 4 outputs: bottom-up chain n_k + (n_{k+1} + ...)
    float t = 0.f;
    bool have = false;
#pragma unroll
    for (int k = SRF_MAX_DEPTH - 1; k >= 2; --k) {
      if (k < D) {
        const float v = a.lv[k][(size_t)row * (L >> k) + (g >> (k - 2))];
        const float nk = fmaf(v, sc[k], sh[k]);
        t = have ? nk + t : nk;
        have = true;
      }
    }
    float ta = t, tb = t;
    if (D > 1) {
      const float2 e = l1[g];
      const float na = fmaf(e.x, sc[1], sh[1]), nb = fmaf(e.y, sc[1], sh[1]);
      ta = have ? na + t : na;
      tb = have ? nb + t : nb;
    }
    float4 o;
    o.x = fmaf(d0.x, sc[0], sh[0]);
    o.y = fmaf(d0.y, sc[0], sh[0]);
    o.z = fmaf(d0.z, sc[0], sh[0]);
    o.w = fmaf(d0.w, sc[0], sh[0]);
    if (D > 1) {
      o.x += ta;
      o.y += ta;
      o.z += tb;
      o.w += tb;
    }
    yr[g] = o;
    const float s = (o.x + o.y) + (o.z + o.w);
    const float q = fmaf(o.x, o.x, fmaf(o.y, o.y, fmaf(o.z, o.z, o.w * o.w)));
    ds += (double)s;
    dq += (double)q;
  }
  if (out_sums) srf_wave_stats_atomic(ds, dq, srf_stat_slot(out_sums, b, row));
}

// who: the entry point's name in its refusals; frames: NULL = the uniform call, else one entry per example (srf_merge_ragged)
static int merge_impl(const char* who, const float* const* levels, const srf_norm* norms, int D, float* y, int Bt, int C, int L,
                      double* out_sums, const int* frames, void* stream) {
  SRF_CHECK_ARG(levels && norms && y, "%s: null pointer", who);
  SRF_CHECK_ARG(D >= 1 && D <= SRF_MAX_DEPTH, "%s: depth %d unsupported (1..%d)", who, D, SRF_MAX_DEPTH);
  SRF_CHECK_ARG(Bt > 0 && C > 0 && L > 0, "%s: bad sizes", who);
  SRF_CHECK_ARG(L % (1 << (D - 1)) == 0, "%s: L=%d not divisible by 2^(D-1)", who, L);
  SrfFrames fr;
  bool grid = true;      // (ragged) every example on the fast kernel's grid of 4 columns
  if (frames) {
    const int rc = srf_frames_table(who, frames, Bt, L, &fr);
    if (rc) return rc;
    for (int b = 0; b < Bt; ++b) {
      SRF_CHECK_ARG(frames[b] % (1 << (D - 1)) == 0, "%s: example %d has %d frames: not a multiple of 2^(D-1) = %d", who, b, frames[b],
                    1 << (D - 1));
      grid = grid && frames[b] % 4 == 0;
    }
  }
  MergeArgs a;
  bool aligned = srf_aligned16(y);
  for (int k = 0; k < SRF_MAX_DEPTH; ++k) {
    a.lv[k] = nullptr;
    a.nrm[k] = SrfNormDev{nullptr, nullptr, nullptr, nullptr};
    a.inv_count[k] = 1.0;
    if (k < D) {
      SRF_CHECK_ARG(levels[k] != nullptr, "%s: null level %d", who, k);
      SRF_CHECK_ALIGNED16(who, {"norms.sums", norms[k].sums});
      a.lv[k] = levels[k];
      a.nrm[k] = srf_norm_dev(&norms[k]);
      a.inv_count[k] = 1.0 / ((double)C * (double)(L >> k));
      aligned = aligned && srf_aligned16(levels[k]);
    }
  }
  a.D = D;
  const long rows = (long)Bt * C;
  hipStream_t st = (hipStream_t)stream;
  const bool fast = srf_kernel_mode() != 1 && (L % 4 == 0) && grid && aligned && rows < (1L << 32);
  const int chunks = (L + 255) / 256;
  const long blocks = rows * chunks;
  SRF_CHECK_ARG(fast || blocks < (1L << 31), "%s: tensor too large", who);
  if (frames) {
    if (fast)
      hipLaunchKernelGGL(srf_merge_fast_kernel<SrfFrames>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, a, y, out_sums, C, L,
                         rows, fr);
    else
      hipLaunchKernelGGL(srf_merge_generic_kernel<SrfFrames>, dim3((unsigned)blocks), dim3(256), 0, st, a, y, out_sums, C, L, chunks,
                         fr);
    SRF_CHECK_LAUNCH(fast ? "merge_fast_ragged" : "merge_generic_ragged", st);
    return SRF_OK;
  }
  if (fast) {
    hipLaunchKernelGGL(srf_merge_fast_kernel<>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, a, y,
                       out_sums, C, L, rows);
  } else {
    hipLaunchKernelGGL(srf_merge_generic_kernel<>, dim3((unsigned)blocks), dim3(256), 0, st, a, y, out_sums,
                       C, L, chunks);
  }
  SRF_CHECK_LAUNCH(fast ? "merge_fast" : "merge_generic", st);
  return SRF_OK;
}

extern "C" int srf_merge(const float* const* levels, const srf_norm* norms, int D, float* y, int Bt,
                         int C, int L, double* out_sums, void* stream) {
  return merge_impl("srf_merge", levels, norms, D, y, Bt, C, L, out_sums, nullptr, stream);
}

extern "C" int srf_merge_ragged(const float* const* levels, const srf_norm* norms, int D, float* y, int Bt, int C, int L,
                                double* out_sums, const int* frames, void* stream) {
  SRF_CHECK_ARG(frames != nullptr, "srf_merge_ragged: null frames table");
  return merge_impl("srf_merge_ragged", levels, norms, D, y, Bt, C, L, out_sums, frames, stream);
}

// A block's pyramid as D depthwise launches + the merge: what the forwards run where the fused kernels (srf_pyramid.hip) do
// not.  lv[k]: level k's output [Bg, nC, L >> k]; level 0 reads x through in_norm (the Improved model: proj_1x1's norm + PReLU;
// NULL, the original model: x as it is), level k > 0 reads level k - 1 through that level's norm with stride 2; merged may alias
// x (dead once every level has been produced).
int srf_pyramid_per_level(const float* x, const srf_norm* in_norm, float* const* lv, float* merged, const float* const* w,
                          const float* const* bias, const float* const* gamma, const float* const* beta, double* const* lv_sums,
                          double* merged_sums, int Bg, int nC, int L, int D, void* stream) {
  const float* levels[SRF_MAX_DEPTH];
  srf_norm norms[SRF_MAX_DEPTH];
  for (int k = 0; k < D; ++k) {
    const int rc = srf_dwconv5(k == 0 ? x : lv[k - 1], w[k], bias[k], lv[k], Bg, nC, k == 0 ? L : L >> (k - 1), k == 0 ? 1 : 2,
                               k == 0 ? in_norm : &norms[k - 1], lv_sums[k], stream);
    if (rc) return rc;
    levels[k] = lv[k];
    norms[k] = srf_norm{lv_sums[k], gamma[k], beta[k], nullptr};
  }
  return srf_merge(levels, norms, D, merged, Bg, nC, L, merged_sums, stream);   // upsample + add   improved_sudormrf.py:214-216
}


// =============================================================================================
// General Conv1d (round 6): any kernel size / stride / dilation / zero padding / groups, fp32 FMA, one thread per output.
// NOT on the model's path -- UConvBlock only ever builds kSize = 1 (srf_pw_conv) and depthwise k = 5 (srf_dwconv5) -- but the
// reference's building blocks ConvNormAct / DilatedConvNorm (improved_sudormrf.py:50-73,:138-159) are ordinary nn.Conv1d
// wrappers that accept any of these, and a user who instantiates one stand-alone gets the same result here.
//   y[b, co, l] = bias[co] + sum_{ci < Cin/groups, k < K} w[co, ci, k] x[b, g Cin/groups + ci, l stride - pad + k dil],  g = co / (Cout/groups)
// out_sums (nullable): [Bt][SRF_STAT_BUCKETS][2] += {sum, sumsq} of y (the GlobLN that follows).
// =============================================================================================
struct Conv1dArgs {
  const float* x;
  const float* w;
  const float* bias;
  float* y;
  double* out_sums;
  int Cin, Cout, Lin, Lout, K, stride, pad, dil, groups;
};

__global__ __launch_bounds__(256) void srf_conv1d_kernel(Conv1dArgs a) {
  __shared__ double red[8];
  const long b = blockIdx.z;
  const int co = blockIdx.y;
  const int l = blockIdx.x * 256 + threadIdx.x;
  const int cpg = a.Cin / a.groups, g = co / (a.Cout / a.groups);
  float acc = a.bias ? a.bias[co] : 0.f;
  const bool ok = l < a.Lout;
  if (ok) {
    const float* xb = a.x + (b * a.Cin + (long)g * cpg) * a.Lin;
    const float* wr = a.w + (long)co * cpg * a.K;
    const int i0 = l * a.stride - a.pad;
    for (int ci = 0; ci < cpg; ++ci) {
      const float* xr = xb + (long)ci * a.Lin;
      for (int k = 0; k < a.K; ++k) {
        const int i = i0 + k * a.dil;
        if (i >= 0 && i < a.Lin) acc = fmaf(wr[ci * a.K + k], xr[i], acc);
      }
    }
    a.y[(b * a.Cout + co) * (long)a.Lout + l] = acc;
  }
  if (a.out_sums) {
    const double v = ok ? (double)acc : 0.0;
    srf_block_stats_atomic<4>(v, v * v, srf_stat_slot(a.out_sums, b, (long)co * gridDim.x + blockIdx.x), red);
  }
}

extern "C" int srf_conv1d(const float* x, const float* w, const float* bias, float* y, int Bt, int Cin, int Cout, int Lin,
                          int K, int stride, int padding, int dilation, int groups, double* out_sums, void* stream) {
  SRF_CHECK_ARG(x && w && y, "srf_conv1d: null pointer");
  SRF_CHECK_ARG(Bt > 0 && Cin > 0 && Cout > 0 && Lin > 0 && K > 0 && stride > 0 && padding >= 0 && dilation > 0 && groups > 0,
                "srf_conv1d: bad sizes");
  SRF_CHECK_ARG(Cin % groups == 0 && Cout % groups == 0, "srf_conv1d: channels (%d, %d) must be divisible by groups (%d)", Cin,
                Cout, groups);
  const long span = (long)dilation * (K - 1) + 1;
  SRF_CHECK_ARG((long)Lin + 2L * padding >= span, "srf_conv1d: kernel span %ld exceeds the padded input (%d + 2 x %d)", span, Lin,
                padding);
  Conv1dArgs a;
  a.x = x;
  a.w = w;
  a.bias = bias;
  a.y = y;
  a.out_sums = out_sums;
  a.Cin = Cin;
  a.Cout = Cout;
  a.Lin = Lin;
  a.Lout = (int)(((long)Lin + 2L * padding - span) / stride + 1);
  a.K = K;
  a.stride = stride;
  a.pad = padding;
  a.dil = dilation;
  a.groups = groups;
  SRF_CHECK_ARG(Cout <= 65535 && Bt <= 65535, "srf_conv1d: too many channels / examples");
  dim3 grid((unsigned)((a.Lout + 255) / 256), (unsigned)Cout, (unsigned)Bt);
  hipLaunchKernelGGL(srf_conv1d_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  SRF_CHECK_LAUNCH("conv1d", stream);
  return SRF_OK;
}
