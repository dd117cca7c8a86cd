// The FUSS recipe's loss, metric and augmentation (experiments/run_fuss_separation.py), on the device:
//     PermInvariantSNRwithZeroRefs          losses/snr.py:13-142    training loss, forward and backward
//     StabilizedPermInvSISDRMetric          losses/sisdr.py:460-576 validation metric, fewer targets than estimates
//     online_augment + mixture normalisation run_fuss_separation.py:195-215, :237-243
// Organisation shared by all three: ONE streaming pass over the waveforms that accumulates a handful of fp64 sums per
// example, and one small finalize launch that does everything else.  Unlike srf_pit_stats_kernel (srf_loss.hip), which
// adds its block sums with an fp64 atomicAdd in arrival order, the blocks here WRITE their partial sums and the finalize
// kernel adds them in block order: the same inputs give the same bits on every run, and the exact ties the zero-reference
// loss produces (permutations that differ only on inactive targets) cannot be broken by summation order.
//
// Zero-reference SNR, per example (S sources, eps = 1e-9, thresh = 0.001, theta = inactivity threshold in dB):
//     M = |sum_j t_j|^2, P_j = |t_j|^2, active_j = [10 log10(P_j / (M + eps)) >= theta], n_act = sum_j active_j
//     stab_j = thresh (active_j ? P_j : M)
//     term(i, j) = 10 active_j log10((P_j + eps) / (|e_i - t_j|^2 + stab_j + eps) + eps)
//     value = max_perm n_act sum_j term(perm(j), j)          (itertools order, first maximum)
// |e_i - t_j|^2 is accumulated from the differences themselves (S^2 sums), not expanded into |e|^2 - 2<e,t> + |t|^2,
// so it keeps its digits when the error is 80 dB below the signals.  With zero_mean the centred quantities follow from
// the raw ones and the row sums: |(e - me) - (t - mt)|^2 = |e - t|^2 - T (me - mt)^2.
//     d value / d e_i = c_i ((e_i - me_i) - (t_j - mt_j))   for the ACTIVE target j matched with estimate i,  0 otherwise
//     c_i = -n_act (20 / ln 10) r / ((r + eps) den),  r = (P_j + eps) / den,  den = |e_i - t_j|^2 + stab_j + eps
#include "srf_common.h"

#define SRF_FUSS_MAX_SRC 4        // FUSS's maximum; everything below keeps its sums in registers for 1..4 sources
#define SRF_FUSS_PER_BLOCK 4096   // samples of one example per block of the streaming passes (a multiple of 4)

static inline int fuss_blocks(int T) { return (T + SRF_FUSS_PER_BLOCK - 1) / SRF_FUSS_PER_BLOCK; }

// Block-wide sums of NSTAT per-thread fp64 accumulators, written (not added) to dst[0..NSTAT): wavefront sums on the
// VALU (DPP, total in lane 63), the four wavefronts added in a fixed order.  Must be reached by the whole block.
template <int NSTAT>
__device__ __forceinline__ void fuss_block_store(const double (&acc)[NSTAT], double* __restrict__ dst,
                                                 double (*red)[NSTAT]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NSTAT; ++k) {
    const double v = srf_dpp_wave_sum(acc[k]);
    if (lane == 63) red[wave][k] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < NSTAT) {
    const int k = threadIdx.x;
    dst[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
  }
}

// Totals of every (example, statistic) pair: partial sums added in BLOCK ORDER.  One block; ends with a barrier.
__device__ __forceinline__ void fuss_totals(const double* __restrict__ part, double* __restrict__ tot, int Bt, int nblk,
                                            int nstat) {
  for (long it = threadIdx.x; it < (long)Bt * nstat; it += blockDim.x) {
    const long b = it / nstat;
    const int k = (int)(it - b * nstat);
    const double* p = part + b * nblk * (long)nstat + k;
    double s = 0.0;
    int blk = 0;
    for (; blk + 8 <= nblk; blk += 8) {      // eight independent loads in flight, added in block order
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = p[(long)(blk + u) * nstat];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; blk < nblk; ++blk) s += p[(long)blk * nstat];
    tot[it] = s;
  }
  __threadfence_block();
  __syncthreads();
}

// =============================================================================================
// 1. zero-reference PIT-SNR
// =============================================================================================
// statistics of one example: D[i][j] = sum (e_i - t_j)^2 | P[j] = sum t_j^2 | M = sum (sum_j t_j)^2 | sum e_i | sum t_j
template <int S>
struct ZrLayout {
  static constexpr int D = 0, P = S * S, M = S * S + S, SE = S * S + S + 1, ST = S * S + 2 * S + 1, N = S * S + 3 * S + 1;
};
__host__ __device__ static inline int zr_nstat(int S) { return S * S + 3 * S + 1; }

template <int S>
__device__ __forceinline__ void zr_accum(double (&acc)[ZrLayout<S>::N], const float (&e)[S], const float (&g)[S]) {
  typedef ZrLayout<S> L;
  double mix = 0.0;
#pragma unroll
  for (int j = 0; j < S; ++j) {
    const double t = (double)g[j];
    mix += t;
    acc[L::P + j] += t * t;
    acc[L::ST + j] += t;
  }
  acc[L::M] += mix * mix;
#pragma unroll
  for (int i = 0; i < S; ++i) {
    acc[L::SE + i] += (double)e[i];
#pragma unroll
    for (int j = 0; j < S; ++j) {
      const double d = (double)e[i] - (double)g[j];   // exact: the difference of two floats fits a double
      acc[L::D + i * S + j] += d * d;
    }
  }
}

// grid (blocks of T, Bt).  VEC: every row is 16-byte aligned (T % 4 == 0, aligned bases) -> 16-byte loads.
template <int S, bool VEC>
__global__ __launch_bounds__(256) void srf_zeroref_stats_kernel(const float* __restrict__ est, const float* __restrict__ tgt,
                                                                double* __restrict__ part, int T) {
  typedef ZrLayout<S> L;
  __shared__ double red[4][L::N];
  const long b = blockIdx.y;
  const int beg = blockIdx.x * SRF_FUSS_PER_BLOCK, end = min(beg + SRF_FUSS_PER_BLOCK, T);
  double acc[L::N];
#pragma unroll
  for (int k = 0; k < L::N; ++k) acc[k] = 0.0;
  const float* eb = est + b * (long)S * T;
  const float* tb = tgt + b * (long)S * T;
  if constexpr (VEC) {
    for (int t = beg + 4 * (int)threadIdx.x; t < end; t += 1024) {
      float4 e4[S], g4[S];
#pragma unroll
      for (int i = 0; i < S; ++i) {
        e4[i] = *reinterpret_cast<const float4*>(eb + (long)i * T + t);
        g4[i] = *reinterpret_cast<const float4*>(tb + (long)i * T + t);
      }
      float e[S], g[S];
#pragma unroll
      for (int i = 0; i < S; ++i) { e[i] = e4[i].x; g[i] = g4[i].x; }
      zr_accum<S>(acc, e, g);
#pragma unroll
      for (int i = 0; i < S; ++i) { e[i] = e4[i].y; g[i] = g4[i].y; }
      zr_accum<S>(acc, e, g);
#pragma unroll
      for (int i = 0; i < S; ++i) { e[i] = e4[i].z; g[i] = g4[i].z; }
      zr_accum<S>(acc, e, g);
#pragma unroll
      for (int i = 0; i < S; ++i) { e[i] = e4[i].w; g[i] = g4[i].w; }
      zr_accum<S>(acc, e, g);
    }
  } else {
    for (int t = beg + (int)threadIdx.x; t < end; t += 256) {
      float e[S], g[S];
#pragma unroll
      for (int i = 0; i < S; ++i) {
        e[i] = eb[(long)i * T + t];
        g[i] = tb[(long)i * T + t];
      }
      zr_accum<S>(acc, e, g);
    }
  }
  fuss_block_store<L::N>(acc, part + (b * gridDim.x + blockIdx.x) * (long)L::N, red);
}

struct ZrFin {
  const double* part;   // [Bt][nblk][nstat]
  double* tot;          // [Bt][nstat]
  float* coef;          // [Bt][S][2]: per estimate i {c_i, me_i - mt_j}
  int* tmatch;          // [Bt][S]: the active target matched with estimate i, or -1 (no gradient)
  float* values;        // [Bt]
  int* best_perm;       // [Bt]: index into itertools.permutations(range(S))
  float* loss;          // [1]: -mean(values)
  int Bt, S, T, nblk, zero_mean;
  double theta, thresh, eps;
};

// One block, S a template parameter: the totals of a thread's example are loaded into registers at once (independent loads,
// one latency) and every loop over sources is unrolled, so the S^2 logarithms overlap.  The S x S term table lives in LDS
// (column = thread) because the permutation walk indexes it dynamically: nothing is indexed dynamically in registers, no
// scratch.  Permutations are walked as the S-digit numbers base 4 (two bits per digit: no integer division) in ascending
// order (= lexicographic = itertools order), skipping those with a digit >= S or a repeated one; digit j, most significant
// first, = the estimate for target j.
template <int S>
__global__ __launch_bounds__(256) void srf_zeroref_finalize_kernel(ZrFin a) {
  typedef ZrLayout<S> L;
  __shared__ double term[S * S][256];
  __shared__ double red[4];
  fuss_totals(a.part, a.tot, a.Bt, a.nblk, L::N);
  const int tid = threadIdx.x;
  const double dT = (double)a.T, zm = a.zero_mean ? 1.0 / dT : 0.0, k20 = 20.0 / log(10.0);
  constexpr int ncode = 1 << (2 * S);
  double mysum = 0.0;
  for (int b = tid; b < a.Bt; b += 256) {
    double w[L::N];
#pragma unroll
    for (int k = 0; k < L::N; ++k) w[k] = a.tot[(long)b * L::N + k];
    double mt[S], P[S], stab[S], smt = 0.0;
    bool active[S];
#pragma unroll
    for (int j = 0; j < S; ++j) {
      mt[j] = zm * w[L::ST + j];
      smt += mt[j];
    }
    const double M = w[L::M] - dT * smt * smt;
    int n_act = 0;
#pragma unroll
    for (int j = 0; j < S; ++j) {
      P[j] = w[L::P + j] - dT * mt[j] * mt[j];
      active[j] = 10.0 * log10(P[j] / (M + a.eps)) >= a.theta;     // P = 0: -inf, inactive
      n_act += active[j] ? 1 : 0;
      stab[j] = a.thresh * (active[j] ? P[j] : M);
    }
    // per (estimate, target): the term, and the gradient coefficient it would have if matched (0 for an inactive target)
    float cf[S * S], dmf[S * S];
#pragma unroll
    for (int i = 0; i < S; ++i) {
#pragma unroll
      for (int j = 0; j < S; ++j) {
        const double dm = zm * w[L::SE + i] - mt[j];
        const double den = w[L::D + i * S + j] - dT * dm * dm + stab[j] + a.eps;
        const double r = (P[j] + a.eps) / den;
        term[i * S + j][tid] = active[j] ? 10.0 * log10(r + a.eps) : 0.0;
        cf[i * S + j] = active[j] ? (float)(-(double)n_act * k20 * r / ((r + a.eps) * den)) : 0.f;
        dmf[i * S + j] = (float)dm;
      }
    }
    double best = 0.0;
    int best_code = 0, best_idx = 0, idx = 0;
    for (int code = 0; code < ncode; ++code) {
      int used = 0;
      bool ok = true;
#pragma unroll
      for (int j = 0; j < S; ++j) {      // registers only: most codes are not permutations and never touch the table
        const int i = (code >> (2 * j)) & 3;
        ok = ok && i < S && !(used & (1 << i));
        used |= 1 << i;
      }
      if (!ok) continue;
      double v = 0.0;
#pragma unroll
      for (int j = 0; j < S; ++j)        // the sum runs over j in ascending order
        v += term[((code >> (2 * (S - 1 - j))) & 3) * S + j][tid];
      v *= (double)n_act;
      if (idx == 0 || v > best) {        // strict: the first maximum wins, like torch.max
        best = v;
        best_code = code;
        best_idx = idx;
      }
      ++idx;
    }
    a.values[b] = (float)best;
    a.best_perm[b] = best_idx;
    mysum += best;
#pragma unroll
    for (int i = 0; i < S; ++i) {        // estimate i: its target is the digit position that holds i
      int tj = -1;
      float c = 0.f, dm = 0.f;
#pragma unroll
      for (int j = 0; j < S; ++j) {
        if (((best_code >> (2 * (S - 1 - j))) & 3) == i && active[j]) {
          tj = j;
          c = cf[i * S + j];
          dm = dmf[i * S + j];
        }
      }
      a.coef[((long)b * S + i) * 2] = c;
      a.coef[((long)b * S + i) * 2 + 1] = dm;
      a.tmatch[(long)b * S + i] = tj;
    }
  }
  mysum = srf_wave_sum(mysum);
  if ((tid & 63) == 0) red[tid >> 6] = mysum;
  __syncthreads();
  if (tid == 0) a.loss[0] = (float)(-((red[0] + red[1]) + (red[2] + red[3])) / (double)a.Bt);
}

// grid (T / 1024, S, Bt): row i of example b.  per_example: grad = upstream[b] d values[b] / d est, else
// grad = upstream[0] d loss / d est with loss = -mean(values); upstream NULL = 1.  Rows without a gradient get zeros.
template <bool VEC>
__global__ __launch_bounds__(256) void srf_zeroref_grad_kernel(const float* __restrict__ est, const float* __restrict__ tgt,
                                                               const float* __restrict__ coef, const int* __restrict__ tmatch,
                                                               const float* __restrict__ upstream, int per_example,
                                                               float* __restrict__ grad, int Bt, int S, int T) {
  const long b = blockIdx.z;
  const int i = blockIdx.y;
  const int j = tmatch[b * S + i];
  float* g = grad + (b * S + i) * (long)T;
  const float up = upstream ? upstream[per_example ? b : 0] : 1.f;
  const float c = j >= 0 ? coef[(b * S + i) * 2] * (per_example ? up : -up / (float)Bt) : 0.f;
  const float dm = j >= 0 ? coef[(b * S + i) * 2 + 1] : 0.f;
  const float* e = est + (b * S + i) * (long)T;
  const float* t = tgt + (b * S + (j >= 0 ? j : 0)) * (long)T;
  if constexpr (VEC) {
    const int x = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (x >= T) return;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j >= 0) {
      const float4 ev = *reinterpret_cast<const float4*>(e + x), tv = *reinterpret_cast<const float4*>(t + x);
      o = make_float4(c * (ev.x - tv.x - dm), c * (ev.y - tv.y - dm), c * (ev.z - tv.z - dm), c * (ev.w - tv.w - dm));
    }
    *reinterpret_cast<float4*>(g + x) = o;
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int x = blockIdx.x * 1024 + u * 256 + threadIdx.x;
      if (x < T) g[x] = j >= 0 ? c * (e[x] - t[x] - dm) : 0.f;
    }
  }
}

struct ZrWork {
  double *part, *tot;
  float* coef;
  int* tmatch;
};
static ZrWork zr_carve(void* work, int Bt, int S, int T) {
  ZrWork w;
  const size_t nstat = (size_t)zr_nstat(S);
  w.part = reinterpret_cast<double*>(work);
  w.tot = w.part + (size_t)Bt * fuss_blocks(T) * nstat;
  w.coef = reinterpret_cast<float*>(w.tot + (size_t)Bt * nstat);
  w.tmatch = reinterpret_cast<int*>(w.coef + (size_t)Bt * S * 2);
  return w;
}

extern "C" size_t srf_zeroref_snr_work_bytes(int Bt, int S, int T) {
  if (Bt <= 0 || S <= 0 || S > SRF_FUSS_MAX_SRC || T <= 0) return 0;
  return (size_t)Bt * ((size_t)(fuss_blocks(T) + 1) * zr_nstat(S) * sizeof(double) + S * 2 * sizeof(float) + S * sizeof(int));
}

#define ZR_CHECK_SIZES(fn)                                                                                              \
  SRF_CHECK_ARG(S >= 1, fn ": %d sources", S);                                                                          \
  SRF_CHECK_ARG(S <= SRF_FUSS_MAX_SRC, fn ": %d sources unsupported: the limit is %d (FUSS's maximum)", S,              \
                SRF_FUSS_MAX_SRC);                                                                                      \
  SRF_CHECK_ARG(Bt > 0 && Bt <= 65535 && T > 0, fn ": bad sizes (Bt = %d in 1..65535, T = %d >= 1)", Bt, T)

extern "C" int srf_zeroref_snr_forward(const float* est, const float* tgt, int Bt, int S, int T, int zero_mean,
                                       float threshold_db, float thresh, float eps, void* work, float* values,
                                       int* best_perm, float* loss, void* stream) {
  ZR_CHECK_SIZES("srf_zeroref_snr_forward");
  SRF_CHECK_ARG(est && tgt && work && values && best_perm && loss, "srf_zeroref_snr_forward: null pointer");
  SRF_CHECK_ARG((((size_t)work) & 7) == 0, "srf_zeroref_snr_forward: work %p is not 8-byte aligned", work);
  hipStream_t st = (hipStream_t)stream;
  const ZrWork w = zr_carve(work, Bt, S, T);
  const bool vec = (T % 4 == 0) && srf_aligned16(est) && srf_aligned16(tgt);
  const dim3 grid((unsigned)fuss_blocks(T), (unsigned)Bt);
#define ZR_LAUNCH(SS)                                                                                                   \
  case SS:                                                                                                              \
    if (vec) hipLaunchKernelGGL((srf_zeroref_stats_kernel<SS, true>), grid, dim3(256), 0, st, est, tgt, w.part, T);     \
    else hipLaunchKernelGGL((srf_zeroref_stats_kernel<SS, false>), grid, dim3(256), 0, st, est, tgt, w.part, T);        \
    break;
  switch (S) {
    ZR_LAUNCH(1)
    ZR_LAUNCH(2)
    ZR_LAUNCH(3)
    ZR_LAUNCH(4)
  }
#undef ZR_LAUNCH
  SRF_CHECK_LAUNCH("zeroref_snr_stats", st);
  ZrFin a;
  a.part = w.part;
  a.tot = w.tot;
  a.coef = w.coef;
  a.tmatch = w.tmatch;
  a.values = values;
  a.best_perm = best_perm;
  a.loss = loss;
  a.Bt = Bt;
  a.S = S;
  a.T = T;
  a.nblk = fuss_blocks(T);
  a.zero_mean = zero_mean ? 1 : 0;
  a.theta = (double)threshold_db;
  a.thresh = (double)thresh;
  a.eps = (double)eps;
  switch (S) {
    case 1: hipLaunchKernelGGL(srf_zeroref_finalize_kernel<1>, dim3(1), dim3(256), 0, st, a); break;
    case 2: hipLaunchKernelGGL(srf_zeroref_finalize_kernel<2>, dim3(1), dim3(256), 0, st, a); break;
    case 3: hipLaunchKernelGGL(srf_zeroref_finalize_kernel<3>, dim3(1), dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL(srf_zeroref_finalize_kernel<4>, dim3(1), dim3(256), 0, st, a); break;
  }
  SRF_CHECK_LAUNCH("zeroref_snr_finalize", st);
  return SRF_OK;
}

extern "C" int srf_zeroref_snr_backward(const float* est, const float* tgt, int Bt, int S, int T, const void* work,
                                        const float* upstream, int upstream_per_example, float* grad_est, void* stream) {
  ZR_CHECK_SIZES("srf_zeroref_snr_backward");
  SRF_CHECK_ARG(est && tgt && work && grad_est, "srf_zeroref_snr_backward: null pointer");
  SRF_CHECK_ARG((((size_t)work) & 7) == 0, "srf_zeroref_snr_backward: work %p is not 8-byte aligned", work);
  const ZrWork w = zr_carve(const_cast<void*>(work), Bt, S, T);
  const bool vec = (T % 4 == 0) && srf_aligned16(est) && srf_aligned16(tgt) && srf_aligned16(grad_est);
  const dim3 grid((unsigned)((T + 1023) / 1024), (unsigned)S, (unsigned)Bt);
  if (vec)
    hipLaunchKernelGGL(srf_zeroref_grad_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, est, tgt, w.coef, w.tmatch,
                       upstream, upstream_per_example ? 1 : 0, grad_est, Bt, S, T);
  else
    hipLaunchKernelGGL(srf_zeroref_grad_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, est, tgt, w.coef, w.tmatch,
                       upstream, upstream_per_example ? 1 : 0, grad_est, Bt, S, T);
  SRF_CHECK_LAUNCH("zeroref_snr_grad", stream);
  return SRF_OK;
}

// =============================================================================================
// 2. stabilized SI-SDR metric, n_act <= n_est
//     rho^2(i, j) = <p_i, t_j>^2 / (|p_i|^2 |t_j|^2 + eps);  value(i, j) = 10 log10((rho^2 + eps) / (1 - rho^2 + eps))
//     best = max over the partial permutations (itertools.permutations(range(n_est), r = n_act) order, first maximum) of
//     the mean over the n_act targets; improvement: minus the batch-and-source mean of the same value for the
//     (zero-meaned) sum of the targets against every target.
// =============================================================================================
// statistics of one example (fixed layout for up to 4 x 4): sum p_i | sum p_i^2 | sum t_j | sum t_j^2 | sum p_i t_j |
// sum m^2 | sum m t_j   with m = sum_j t_j
#define SM_P 0
#define SM_PP 4
#define SM_T 8
#define SM_TT 12
#define SM_PT 16
#define SM_MM 32
#define SM_MT 33
#define SM_N 37

__device__ __forceinline__ void sm_accum(double (&acc)[SM_N], const float (&p)[4], const float (&g)[4], int NE, int NA) {
  double mix = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < NA) mix += (double)g[j];
  acc[SM_MM] += mix * mix;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (j < NA) {
      const double t = (double)g[j];
      acc[SM_T + j] += t;
      acc[SM_TT + j] += t * t;
      acc[SM_MT + j] += mix * t;
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i < NE) {
      const double e = (double)p[i];
      acc[SM_P + i] += e;
      acc[SM_PP + i] += e * e;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < NA) acc[SM_PT + i * 4 + j] += e * (double)g[j];
    }
  }
}

// pr: [Bt, rows, T]; NE estimates = the rows themselves, or (sum_rows) ONE estimate = their sum (single_source).
template <bool VEC>
__global__ __launch_bounds__(256) void srf_stab_sisdr_stats_kernel(const float* __restrict__ pr, const float* __restrict__ tgt,
                                                                   double* __restrict__ part, int rows, int sum_rows,
                                                                   int NA, int T) {
  __shared__ double red[4][SM_N];
  const long b = blockIdx.y;
  const int NE = sum_rows ? 1 : rows;
  const int beg = blockIdx.x * SRF_FUSS_PER_BLOCK, end = min(beg + SRF_FUSS_PER_BLOCK, T);
  double acc[SM_N];
#pragma unroll
  for (int k = 0; k < SM_N; ++k) acc[k] = 0.0;
  const float* pb = pr + b * (long)rows * T;
  const float* tb = tgt + b * (long)NA * T;
  auto one = [&](float p0, float p1, float p2, float p3, float g0, float g1, float g2, float g3) {
    if (sum_rows) p0 = ((p0 + p1) + p2) + p3;      // torch.sum over the source axis, in fp32 like the class
    const float pe[4] = {p0, p1, p2, p3}, ge[4] = {g0, g1, g2, g3};
    sm_accum(acc, pe, ge, NE, NA);
  };
  if constexpr (VEC) {
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t = beg + 4 * (int)threadIdx.x; t < end; t += 1024) {
      const float4 p0 = *reinterpret_cast<const float4*>(pb + t);
      const float4 p1 = 1 < rows ? *reinterpret_cast<const float4*>(pb + 1L * T + t) : z;
      const float4 p2 = 2 < rows ? *reinterpret_cast<const float4*>(pb + 2L * T + t) : z;
      const float4 p3 = 3 < rows ? *reinterpret_cast<const float4*>(pb + 3L * T + t) : z;
      const float4 g0 = *reinterpret_cast<const float4*>(tb + t);
      const float4 g1 = 1 < NA ? *reinterpret_cast<const float4*>(tb + 1L * T + t) : z;
      const float4 g2 = 2 < NA ? *reinterpret_cast<const float4*>(tb + 2L * T + t) : z;
      const float4 g3 = 3 < NA ? *reinterpret_cast<const float4*>(tb + 3L * T + t) : z;
      one(p0.x, p1.x, p2.x, p3.x, g0.x, g1.x, g2.x, g3.x);
      one(p0.y, p1.y, p2.y, p3.y, g0.y, g1.y, g2.y, g3.y);
      one(p0.z, p1.z, p2.z, p3.z, g0.z, g1.z, g2.z, g3.z);
      one(p0.w, p1.w, p2.w, p3.w, g0.w, g1.w, g2.w, g3.w);
    }
  } else {
    for (int t = beg + (int)threadIdx.x; t < end; t += 256) {
      one(pb[t], 1 < rows ? pb[1L * T + t] : 0.f, 2 < rows ? pb[2L * T + t] : 0.f, 3 < rows ? pb[3L * T + t] : 0.f,
          tb[t], 1 < NA ? tb[1L * T + t] : 0.f, 2 < NA ? tb[2L * T + t] : 0.f, 3 < NA ? tb[3L * T + t] : 0.f);
    }
  }
  fuss_block_store<SM_N>(acc, part + (b * gridDim.x + blockIdx.x) * (long)SM_N, red);
}

struct SmFin {
  const double* part;
  double* tot;
  float* values;      // [Bt]
  int* best_perm;     // [Bt]: index into itertools.permutations(range(NE), r = NA)
  int Bt, NE, NA, T, nblk, zero_mean, improvement;
  double eps;
};

__device__ __forceinline__ double sm_value(double pp, double tt, double pt, double eps) {
  const double rho = pt * pt / (pp * tt + eps);
  return 10.0 * log10((rho + eps) / (1.0 - rho + eps));
}

__global__ __launch_bounds__(256) void srf_stab_sisdr_finalize_kernel(SmFin a) {
  __shared__ double val[16][256];
  __shared__ double red[4];
  fuss_totals(a.part, a.tot, a.Bt, a.nblk, SM_N);
  const int tid = threadIdx.x, NE = a.NE, NA = a.NA;
  const double dT = (double)a.T, zm = a.zero_mean ? 1.0 : 0.0;
  const int ncode = 1 << (2 * NA);      // NA digits base 4, as in srf_zeroref_finalize_kernel
  double base_sum = 0.0;
  const int rounds = (a.Bt + 255) / 256;
  for (int r = 0; r < rounds; ++r) {
    const int b = r * 256 + tid;
    if (b < a.Bt) {
      const double* w = a.tot + (long)b * SM_N;
      double smt = 0.0;
      for (int j = 0; j < NA; ++j) smt += zm * w[SM_T + j] / dT;
      const double mm = w[SM_MM] - dT * smt * smt;
      for (int j = 0; j < NA; ++j) {
        const double mt = zm * w[SM_T + j] / dT;
        const double tt = w[SM_TT + j] - dT * mt * mt;
        for (int i = 0; i < NE; ++i) {
          const double me = zm * w[SM_P + i] / dT;
          val[i * 4 + j][tid] = sm_value(w[SM_PP + i] - dT * me * me, tt, w[SM_PT + i * 4 + j] - dT * me * mt, a.eps);
        }
        base_sum += sm_value(mm, tt, w[SM_MT + j] - dT * smt * mt, a.eps);
      }
      double best = 0.0;
      int best_idx = 0, idx = 0;
      for (int code = 0; code < ncode; ++code) {
        int used = 0;
        bool ok = true;
        for (int j = 0; j < NA; ++j) {
          const int i = (code >> (2 * j)) & 3;
          ok = ok && i < NE && !(used & (1 << i));
          used |= 1 << i;
        }
        if (!ok) continue;
        double v = 0.0;
        for (int j = 0; j < NA; ++j) v += val[((code >> (2 * (NA - 1 - j))) & 3) * 4 + j][tid];
        v /= (double)NA;
        if (idx == 0 || v > best) {
          best = v;
          best_idx = idx;
        }
        ++idx;
      }
      a.best_perm[b] = best_idx;
      a.values[b] = (float)best;
      a.tot[(long)b * SM_N] = best;      // (this thread's own slot: kept in fp64 until the baseline is known)
    }
  }
  if (!a.improvement) return;
  base_sum = srf_wave_sum(base_sum);
  if ((tid & 63) == 0) red[tid >> 6] = base_sum;
  __syncthreads();
  const double base = ((red[0] + red[1]) + (red[2] + red[3])) / ((double)a.Bt * (double)NA);
  for (int b = tid; b < a.Bt; b += 256) a.values[b] = (float)(a.tot[(long)b * SM_N] - base);
}

extern "C" size_t srf_stab_sisdr_work_bytes(int Bt, int T) {
  if (Bt <= 0 || T <= 0) return 0;
  return (size_t)Bt * (size_t)(fuss_blocks(T) + 1) * SM_N * sizeof(double);
}

extern "C" int srf_stab_sisdr(const float* pr, const float* tgt, int Bt, int pr_rows, int n_est, int n_act, int T,
                              int zero_mean, int improvement, double eps, void* work, float* values, int* best_perm,
                              void* stream) {
  SRF_CHECK_ARG(n_est >= 1 && n_est <= SRF_FUSS_MAX_SRC, "srf_stab_sisdr: %d estimated sources unsupported: the limit is %d",
                n_est, SRF_FUSS_MAX_SRC);
  SRF_CHECK_ARG(n_act >= 1 && n_act <= n_est, "srf_stab_sisdr: %d actual sources with %d estimated ones (1 <= n_act <= n_est)",
                n_act, n_est);
  SRF_CHECK_ARG(pr_rows == n_est || (n_est == 1 && pr_rows >= 1 && pr_rows <= SRF_FUSS_MAX_SRC),
                "srf_stab_sisdr: %d estimate rows for %d estimated sources (equal, or 1..%d rows summed into one)", pr_rows,
                n_est, SRF_FUSS_MAX_SRC);
  SRF_CHECK_ARG(Bt > 0 && Bt <= 65535 && T > 0, "srf_stab_sisdr: bad sizes (Bt = %d in 1..65535, T = %d >= 1)", Bt, T);
  SRF_CHECK_ARG(pr && tgt && work && values && best_perm, "srf_stab_sisdr: null pointer");
  SRF_CHECK_ARG((((size_t)work) & 7) == 0, "srf_stab_sisdr: work %p is not 8-byte aligned", work);
  hipStream_t st = (hipStream_t)stream;
  double* part = reinterpret_cast<double*>(work);
  const int nblk = fuss_blocks(T);
  const int sum_rows = pr_rows != n_est ? 1 : 0;
  const bool vec = (T % 4 == 0) && srf_aligned16(pr) && srf_aligned16(tgt);
  const dim3 grid((unsigned)nblk, (unsigned)Bt);
  if (vec) hipLaunchKernelGGL(srf_stab_sisdr_stats_kernel<true>, grid, dim3(256), 0, st, pr, tgt, part, pr_rows, sum_rows, n_act, T);
  else hipLaunchKernelGGL(srf_stab_sisdr_stats_kernel<false>, grid, dim3(256), 0, st, pr, tgt, part, pr_rows, sum_rows, n_act, T);
  SRF_CHECK_LAUNCH("stab_sisdr_stats", st);
  SmFin a;
  a.part = part;
  a.tot = part + (size_t)Bt * nblk * SM_N;
  a.values = values;
  a.best_perm = best_perm;
  a.Bt = Bt;
  a.NE = n_est;
  a.NA = n_act;
  a.T = T;
  a.nblk = nblk;
  a.zero_mean = zero_mean ? 1 : 0;
  a.improvement = improvement ? 1 : 0;
  a.eps = eps;
  hipLaunchKernelGGL(srf_stab_sisdr_finalize_kernel, dim3(1), dim3(256), 0, st, a);
  SRF_CHECK_LAUNCH("stab_sisdr_finalize", st);
  return SRF_OK;
}

// =============================================================================================
// 3. FUSS online augmentation (run_fuss_separation.py:195-215) + the loop's mixture normalisation (:237-243)
//     out[b, k] = clean[src_b[src_s[k]][b], src_s[k]] * gain[b, k];  mix = sum_k out[b, k];
//     mix = (mix - mean) / (std + eps), std unbiased
// Pass 1 gathers, scales, sums and writes the sources and the raw mixture, and stores every block's fp64 {sum, sum of
// squares} of the mixture; pass 2 adds those in block order and normalises the mixture in place.
// =============================================================================================
struct FussAug {
  const float* clean;   // [B,S,T]
  const int* src_b;     // [S][B]
  const int* src_s;     // [S]
  const float* gain;    // [B][S]
  float* out;           // [B,S,T]
  float* mix;           // [B,T]
  double* part;         // [B][nblk][2]
  float* stats;         // [B][2] {mean, std}
  int B, S, T;
  float eps;
};

template <bool VEC>
__global__ __launch_bounds__(256) void srf_fuss_gather_kernel(FussAug a) {
  __shared__ double red[4][2];
  const int b = blockIdx.y;
  const int beg = blockIdx.x * SRF_FUSS_PER_BLOCK, end = min(beg + SRF_FUSS_PER_BLOCK, a.T);
  const float* row[SRF_FUSS_MAX_SRC];
  float gain[SRF_FUSS_MAX_SRC];
#pragma unroll
  for (int k = 0; k < SRF_FUSS_MAX_SRC; ++k) {
    if (k < a.S) {
      const int s = a.src_s[k];
      row[k] = a.clean + ((long)a.src_b[s * a.B + b] * a.S + s) * (long)a.T;
      gain[k] = a.gain[b * a.S + k];
    } else {
      row[k] = a.clean;
      gain[k] = 0.f;
    }
  }
  double acc[2] = {0.0, 0.0};
  constexpr int W = VEC ? 4 : 1;
  for (int t = beg + W * (int)threadIdx.x; t < end; t += W * 256) {
    float m[W];
#pragma unroll
    for (int u = 0; u < W; ++u) m[u] = 0.f;
#pragma unroll
    for (int k = 0; k < SRF_FUSS_MAX_SRC; ++k) {
      if (k < a.S) {
        float* o = a.out + ((long)b * a.S + k) * (long)a.T + t;
        if constexpr (VEC) {
          float4 v = *reinterpret_cast<const float4*>(row[k] + t);
          v = make_float4(v.x * gain[k], v.y * gain[k], v.z * gain[k], v.w * gain[k]);
          *reinterpret_cast<float4*>(o) = v;
          m[0] += v.x; m[1] += v.y; m[2] += v.z; m[3] += v.w;
        } else {
          const float v = row[k][t] * gain[k];
          *o = v;
          m[0] += v;
        }
      }
    }
    if constexpr (VEC) *reinterpret_cast<float4*>(a.mix + (long)b * a.T + t) = make_float4(m[0], m[1], m[2], m[3]);
    else a.mix[(long)b * a.T + t] = m[0];
#pragma unroll
    for (int u = 0; u < W; ++u) {
      acc[0] += (double)m[u];
      acc[1] += (double)m[u] * (double)m[u];
    }
  }
  fuss_block_store<2>(acc, a.part + ((long)b * gridDim.x + blockIdx.x) * 2, red);
}

template <bool VEC>
__global__ __launch_bounds__(256) void srf_fuss_normalize_kernel(FussAug a) {
  const int b = blockIdx.y;
  const double* p = a.part + (long)b * gridDim.x * 2;
  double s = 0.0, q = 0.0;
  for (unsigned blk = 0; blk < gridDim.x; ++blk) {   // every thread adds the same numbers in the same (block) order
    s += p[2 * blk];
    q += p[2 * blk + 1];
  }
  const double dT = (double)a.T, mu = s / dT;
  double var = (q - dT * mu * mu) / (dT - 1.0);      // unbiased like torch.std (T = 1: NaN there as here)
  var = var < 0.0 ? 0.0 : var;
  const float mean = (float)mu, sd = (float)sqrt(var);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.stats[2 * b] = mean;
    a.stats[2 * b + 1] = sd;
  }
  const float den = sd + a.eps;
  const int beg = blockIdx.x * SRF_FUSS_PER_BLOCK, end = min(beg + SRF_FUSS_PER_BLOCK, a.T);
  float* m = a.mix + (long)b * a.T;
  constexpr int W = VEC ? 4 : 1;
  for (int t = beg + W * (int)threadIdx.x; t < end; t += W * 256) {
    if constexpr (VEC) {
      float4 v = *reinterpret_cast<float4*>(m + t);
      v = make_float4((v.x - mean) / den, (v.y - mean) / den, (v.z - mean) / den, (v.w - mean) / den);
      *reinterpret_cast<float4*>(m + t) = v;
    } else {
      m[t] = (m[t] - mean) / den;
    }
  }
}

extern "C" size_t srf_fuss_augment_scratch_bytes(int B, int T) {
  return B > 0 && T > 0 ? sizeof(double) * 2 * (size_t)B * fuss_blocks(T) : 0;
}

// clean, out: [B,S,T] (out must not alias clean); src_b: [S][B], src_s: [S] int32 and gain: [B][S] float32 on the device;
// mix: [B,T]; stats: [B][2] {mean, std} of the un-normalised mixture.
extern "C" int srf_fuss_augment(const float* clean, const int* src_b, const int* src_s, const float* gain, int B, int S,
                                int T, float eps, float* out, float* mix, float* stats, void* scratch, void* stream) {
  SRF_CHECK_ARG(S >= 1 && S <= SRF_FUSS_MAX_SRC, "srf_fuss_augment: %d sources unsupported: the limit is %d", S,
                SRF_FUSS_MAX_SRC);
  SRF_CHECK_ARG(B > 0 && B <= 65535 && T > 0, "srf_fuss_augment: bad sizes (B = %d in 1..65535, T = %d >= 1)", B, T);
  SRF_CHECK_ARG(clean && src_b && src_s && gain && out && mix && stats && scratch, "srf_fuss_augment: null pointer");
  SRF_CHECK_ARG(out != clean, "srf_fuss_augment: out must not alias clean (rows are gathered across the batch)");
  SRF_CHECK_ARG((((size_t)scratch) & 7) == 0, "srf_fuss_augment: scratch %p is not 8-byte aligned", scratch);
  hipStream_t st = (hipStream_t)stream;
  FussAug a;
  a.clean = clean;
  a.src_b = src_b;
  a.src_s = src_s;
  a.gain = gain;
  a.out = out;
  a.mix = mix;
  a.part = reinterpret_cast<double*>(scratch);
  a.stats = stats;
  a.B = B;
  a.S = S;
  a.T = T;
  a.eps = eps;
  const bool vec = (T % 4 == 0) && srf_aligned16(clean) && srf_aligned16(out) && srf_aligned16(mix);
  const dim3 grid((unsigned)fuss_blocks(T), (unsigned)B);
  if (vec) hipLaunchKernelGGL(srf_fuss_gather_kernel<true>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(srf_fuss_gather_kernel<false>, grid, dim3(256), 0, st, a);
  SRF_CHECK_LAUNCH("fuss_augment_gather", st);
  if (vec) hipLaunchKernelGGL(srf_fuss_normalize_kernel<true>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(srf_fuss_normalize_kernel<false>, grid, dim3(256), 0, st, a);
  SRF_CHECK_LAUNCH("fuss_augment_normalize", st);
  return SRF_OK;
}
