// Causal SuDoRM-RF (v3), backward kernels of one UConvBlock's k = 21 depthwise pyramid and the small
// kernels the training step needs around it.  Notation: u = proj_1x1's pre-activation, a_p = PReLU_p(u), d_k = level k's
// pre-activation, a_k = PReLU_k(d_k), live taps t = 0..10, conv input index s j - 10 + t (s = 1 at level 0, else 2).
//   srf_causal_dwconv_bwd   <- ONE level: G = pool_2^shift(g_merged) + conv-transpose of the next level's gd; gd = G PReLU'(d);
//                              weight / bias / slope gradients of this level.  The path of record (kernel mode 1).
//   srf_causal_pyramid_bwd  <- every level of one block and proj_1x1's PReLU in ONE launch, all levels of a tile in LDS.
//   srf_causal_merge_act    <- the training forward's merge: sum_k PReLU_k(d_k[j >> k]) from the saved pre-activations
//   srf_causal_prelu_bwd    <- a stand-alone PReLU's backward with its slope gradient summed in a fixed order
//   srf_causal_gain_fold    <- dW_r, db_r and d skipinit_gain from the gradient of the folded res_conv
//   srf_causal_enc_scatter  <- the encoder weight gradient into the stored [N, A, 2K-1] layout (masked taps written as 0)
// Both forms of the pyramid backward share cb_taps1 / cb_taps2 / cb_dprelu and the pairwise pooling order, so their data gradients are
// bit-identical.  Parameter gradients: every block writes its partial sums (one record per row and chunk / tile), a finalize
// launch adds them in a fixed order -- no floating-point atomics, the same inputs give the same bits.
#include "srf_internal.h"

#define SRF_CBWD_TILE 1024   // level-0 frames per block of the fused kernel (a multiple of 2^(SRF_MAX_DEPTH-1))
#define SRF_CBWD_REC 13      // one partial record: 11 tap sums | bias sum | slope sum

// d PReLU_a(d) / d d with torch's convention at the kink: an exact 0 takes the slope branch
__device__ __forceinline__ float cb_dprelu(float d, float a) { return d > 0.f ? 1.f : a; }

// sum of 2^K consecutive values as a balanced tree, left + right: P_k[i] = P_{k-1}[2 i] + P_{k-1}[2 i + 1]
template <int K>
__device__ __forceinline__ float cb_pool(const float* g) {
  if constexpr (K == 0) {
    return g[0];
  } else {
    return cb_pool<K - 1>(g) + cb_pool<K - 1>(g + (1 << (K - 1)));
  }
}

// G + sum over the live taps t, ascending, of w[t] gd_next[n]: the conv that consumed position i of this tensor (n >= 0 always).
//   cb_taps1 (the consumer has stride 1): n = i + 10 - t, n < Ln.
//   cb_taps2 (stride 2): only the taps of i's parity reach i: t = 2 q + (i & 1), n = (i >> 1) + 5 - q, n < Ln.  ws holds those
//   taps (cb_load_taps2: picked when they are LOADED, so that every register array is indexed by constants only).
template <class Load>
__device__ __forceinline__ float cb_taps1(float G, const float (&w)[SRF_CAUSAL_TAPS], Load ld, int i, int Ln) {
#pragma unroll
  for (int t = 0; t < SRF_CAUSAL_TAPS; ++t) {
    const int n = i + (SRF_CAUSAL_TAPS - 1) - t;
    if (n < Ln) G = fmaf(w[t], ld(n), G);
  }
  return G;
}
__device__ __forceinline__ void cb_load_taps2(const float* wc, int odd, float (&ws)[6]) {
#pragma unroll
  for (int q = 0; q < 5; ++q) ws[q] = wc[2 * q + odd];
  ws[5] = odd ? 0.f : wc[10];
}
template <class Load>
__device__ __forceinline__ float cb_taps2(float G, const float (&ws)[6], Load ld, int i, int Ln) {
  const bool odd = i & 1;
  const int base = (i >> 1) + 5;
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    const int n = base - q;
    if ((q < 5 || !odd) && n < Ln) G = fmaf(ws[q], ld(n), G);
  }
  return G;
}

// Block sum of SRF_CBWD_REC values per thread (256 threads), fixed order: DPP wavefront sums, then the four wavefronts in
// order.  red: 4 * SRF_CBWD_REC floats of LDS.  Every thread of the block must call it; `out` gets the record.
__device__ __forceinline__ void cb_block_reduce(float (&v)[SRF_CBWD_REC], float* red, float* out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < SRF_CBWD_REC; ++q) {
    const float s = srf_dpp_wave_sum(v[q]);
    if (lane == 63) red[wave * SRF_CBWD_REC + q] = s;
  }
  __syncthreads();
  if (threadIdx.x < SRF_CBWD_REC) {
    const int q = threadIdx.x;
    out[q] = ((red[q] + red[SRF_CBWD_REC + q]) + red[2 * SRF_CBWD_REC + q]) + red[3 * SRF_CBWD_REC + q];
  }
  __syncthreads();
}

// ---------------------------------------------------------------------------------------------
// one level
// ---------------------------------------------------------------------------------------------
struct CausalDwBwdArgs {
  const float* g_pool;    // [rows, Lout << shift] or NULL
  const float* g_next;    // [rows, Lnext] or NULL
  const float* w_next;    // [C, 21]
  const float* d;         // [rows, Lout]
  const float* slope;     // [1]
  const float* xin;       // [rows, Lout * stride] or NULL (no weight / bias gradient)
  const float* in_slope;  // [1]
  float* gd;              // [rows, Lout]
  float* part;            // [rows][nchunks][SRF_CBWD_REC]
  int next_stride, stride, C, Lout, nchunks;
  long rows;
};

template <int SHIFT>
__global__ __launch_bounds__(256) void srf_causal_dw_bwd_kernel(CausalDwBwdArgs a) {
  __shared__ float red[4 * SRF_CBWD_REC];
  const int chunk = blockIdx.x;
  const int i = chunk * 256 + threadIdx.x;
  const int Lout = a.Lout;
  const float ak = a.slope[0];
  const float ain = a.xin ? a.in_slope[0] : 1.f;
  for (long r = blockIdx.y; r < a.rows; r += gridDim.y) {
    const int c = (int)(r % a.C);
    float acc[SRF_CBWD_REC];
#pragma unroll
    for (int q = 0; q < SRF_CBWD_REC; ++q) acc[q] = 0.f;
    if (i < Lout) {
      float G = 0.f;
      if (a.g_pool) G = cb_pool<SHIFT>(a.g_pool + ((size_t)r * Lout + i) * ((size_t)1 << SHIFT));
      if (a.g_next) {
        const float* wc = a.w_next + (size_t)c * SRF_CAUSAL_KW;
        const int Ln = a.next_stride == 1 ? Lout : (Lout >> 1);
        const float* gn = a.g_next + (size_t)r * Ln;
        auto ld = [&](int n) { return gn[n]; };
        if (a.next_stride == 1) {
          float w[SRF_CAUSAL_TAPS];
#pragma unroll
          for (int t = 0; t < SRF_CAUSAL_TAPS; ++t) w[t] = wc[t];
          G = cb_taps1(G, w, ld, i, Ln);
        } else {
          float ws[6];
          cb_load_taps2(wc, i & 1, ws);
          G = cb_taps2(G, ws, ld, i, Ln);
        }
      }
      const float dv = a.d[(size_t)r * Lout + i];
      const float gdv = G * cb_dprelu(dv, ak);
      a.gd[(size_t)r * Lout + i] = gdv;
      acc[12] = G * fminf(dv, 0.f);
      if (a.xin) {
        const float* xr = a.xin + (size_t)r * Lout * a.stride;
        acc[11] = gdv;
#pragma unroll
        for (int t = 0; t < SRF_CAUSAL_TAPS; ++t) {
          const int idx = a.stride * i - (SRF_CAUSAL_TAPS - 1) + t;
          acc[t] = gdv * (idx >= 0 ? srf_prelu(xr[idx], ain) : 0.f);
        }
      }
    }
    cb_block_reduce(acc, red, a.part + ((size_t)r * a.nchunks + chunk) * SRF_CBWD_REC);
  }
}

// ---------------------------------------------------------------------------------------------
// finalize: part [nlev][rows][nrec][SRF_CBWD_REC] -> dw [C, 21] (taps 11..20 = 0), dbias [C], per-channel slope sums;
// then the slope sums of a level over its channels.  Sums run over (example, record) in index order.
// ---------------------------------------------------------------------------------------------
struct CausalBwdFinArgs {
  const float* part;
  float* slope_c;                       // [nlev][C]
  float* dw[SRF_MAX_DEPTH + 1];         // NULL = this level has no weight / bias gradient
  float* db[SRF_MAX_DEPTH + 1];
  float* dslope[SRF_MAX_DEPTH + 1];
  int C, Bt, nrec;
};

__global__ __launch_bounds__(64) void srf_causal_bwd_finalize_kernel(CausalBwdFinArgs a) {
  const int c = blockIdx.x, lev = blockIdx.y, q = threadIdx.x;
  const size_t rows = (size_t)a.Bt * a.C;
  if (q < SRF_CBWD_REC) {
    float s = 0.f;
    for (int b = 0; b < a.Bt; ++b) {
      const float* p = a.part + ((lev * rows + (size_t)b * a.C + c) * a.nrec) * SRF_CBWD_REC + q;
      for (int t = 0; t < a.nrec; ++t) s += p[(size_t)t * SRF_CBWD_REC];
    }
    if (q < SRF_CAUSAL_TAPS) {
      if (a.dw[lev]) a.dw[lev][(size_t)c * SRF_CAUSAL_KW + q] = s;
    } else if (q == 11) {
      if (a.db[lev]) a.db[lev][c] = s;
    } else {
      a.slope_c[(size_t)lev * a.C + c] = s;
    }
  } else if (q < SRF_CBWD_REC + SRF_CAUSAL_KW - SRF_CAUSAL_TAPS) {
    if (a.dw[lev]) a.dw[lev][(size_t)c * SRF_CAUSAL_KW + q - 2] = 0.f;     // the masked taps 11..20
  }
}

__global__ __launch_bounds__(64) void srf_causal_bwd_slope_kernel(CausalBwdFinArgs a) {
  const int lev = blockIdx.x;
  float s = 0.f;
  for (int c = threadIdx.x; c < a.C; c += 64) s += a.slope_c[(size_t)lev * a.C + c];
  s = srf_dpp_wave_sum(s);
  if (threadIdx.x == 63 && a.dslope[lev]) a.dslope[lev][0] = s;
}

static int cb_finalize(CausalBwdFinArgs& f, int nlev, hipStream_t st) {
  hipLaunchKernelGGL(srf_causal_bwd_finalize_kernel, dim3(f.C, nlev), dim3(64), 0, st, f);
  SRF_CHECK_LAUNCH("causal_bwd_finalize", st);
  hipLaunchKernelGGL(srf_causal_bwd_slope_kernel, dim3(nlev), dim3(64), 0, st, f);
  SRF_CHECK_LAUNCH("causal_bwd_slope", st);
  return SRF_OK;
}

static size_t cb_part_floats(long rows, int nrec, int nlev, int C) {
  return (size_t)nlev * rows * nrec * SRF_CBWD_REC + (size_t)nlev * C;
}

extern "C" size_t srf_causal_dwconv_bwd_scratch_bytes(int Bt, int C, int Lout) {
  if (Bt <= 0 || C <= 0 || Lout <= 0) return 0;
  return sizeof(float) * cb_part_floats((long)Bt * C, (Lout + 255) / 256, 1, C);
}

extern "C" int srf_causal_dwconv_bwd(const float* g_pool, int shift, const float* g_next, const float* w_next, int next_stride,
                                     const float* d, const float* slope, const float* xin, const float* in_slope, int stride,
                                     float* gd, float* dw, float* dbias, float* dslope, int Bt, int C, int Lout, void* scratch,
                                     void* stream) {
  SRF_CHECK_ARG(d && slope && gd && dslope && scratch, "srf_causal_dwconv_bwd: null pointer");
  SRF_CHECK_ARG(g_pool || g_next, "srf_causal_dwconv_bwd: neither g_pool nor g_next given");
  SRF_CHECK_ARG(Bt > 0 && C > 0 && Lout > 0, "srf_causal_dwconv_bwd: bad sizes");
  SRF_CHECK_ARG(shift >= 0 && shift < SRF_MAX_DEPTH && (g_pool || shift == 0), "srf_causal_dwconv_bwd: shift %d unsupported (0..%d)",
                shift, SRF_MAX_DEPTH - 1);
  SRF_CHECK_ARG((long)Lout << shift < (1L << 31), "srf_causal_dwconv_bwd: pooled row too long");
  if (g_next) {
    SRF_CHECK_ARG(w_next, "srf_causal_dwconv_bwd: g_next without w_next");
    SRF_CHECK_ARG(next_stride == 1 || (next_stride == 2 && Lout % 2 == 0),
                  "srf_causal_dwconv_bwd: next_stride must be 1, or 2 with an even Lout (got %d, Lout %d)", next_stride, Lout);
  }
  if (xin) {
    SRF_CHECK_ARG(in_slope && dw && dbias, "srf_causal_dwconv_bwd: xin without in_slope / dw / dbias");
    SRF_CHECK_ARG(stride == 1 || stride == 2, "srf_causal_dwconv_bwd: stride must be 1 or 2 (got %d)", stride);
    SRF_CHECK_ARG((long)Lout * stride < (1L << 31), "srf_causal_dwconv_bwd: input row too long");
  } else {
    SRF_CHECK_ARG(!dw && !dbias, "srf_causal_dwconv_bwd: dw / dbias without xin");
  }
  SRF_CHECK_ARG(gd != g_pool && gd != g_next && gd != d && gd != xin, "srf_causal_dwconv_bwd: gd must not alias an input");
  CausalDwBwdArgs a;
  a.g_pool = g_pool;
  a.g_next = g_next;
  a.w_next = w_next;
  a.d = d;
  a.slope = slope;
  a.xin = xin;
  a.in_slope = in_slope;
  a.gd = gd;
  a.part = (float*)scratch;
  a.next_stride = next_stride;
  a.stride = xin ? stride : 1;
  a.C = C;
  a.Lout = Lout;
  a.nchunks = (Lout + 255) / 256;
  a.rows = (long)Bt * C;
  hipStream_t st = (hipStream_t)stream;
  dim3 grid(a.nchunks, (unsigned)(a.rows < 65535 ? a.rows : 65535));
  switch (shift) {
    case 0: hipLaunchKernelGGL(srf_causal_dw_bwd_kernel<0>, grid, dim3(256), 0, st, a); break;
    case 1: hipLaunchKernelGGL(srf_causal_dw_bwd_kernel<1>, grid, dim3(256), 0, st, a); break;
    case 2: hipLaunchKernelGGL(srf_causal_dw_bwd_kernel<2>, grid, dim3(256), 0, st, a); break;
    case 3: hipLaunchKernelGGL(srf_causal_dw_bwd_kernel<3>, grid, dim3(256), 0, st, a); break;
    case 4: hipLaunchKernelGGL(srf_causal_dw_bwd_kernel<4>, grid, dim3(256), 0, st, a); break;
    case 5: hipLaunchKernelGGL(srf_causal_dw_bwd_kernel<5>, grid, dim3(256), 0, st, a); break;
    case 6: hipLaunchKernelGGL(srf_causal_dw_bwd_kernel<6>, grid, dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL(srf_causal_dw_bwd_kernel<7>, grid, dim3(256), 0, st, a); break;
  }
  SRF_CHECK_LAUNCH("causal_dw_bwd", st);
  CausalBwdFinArgs f{};
  f.part = a.part;
  f.slope_c = a.part + (size_t)a.rows * a.nchunks * SRF_CBWD_REC;
  f.dw[0] = dw;
  f.db[0] = dbias;
  f.dslope[0] = dslope;
  f.C = C;
  f.Bt = Bt;
  f.nrec = a.nchunks;
  return cb_finalize(f, 1, st);
}

// ---------------------------------------------------------------------------------------------
// fused pyramid backward.  One block = one row (b, c) x one tile [j0, je) of level-0 frames.  The dependency cone opens to
// the RIGHT: gd_k is produced on [j0 >> k, (je >> k) + 10) (10 frames of right halo at every level, clipped at L >> k), so
// g_merged is read 10 * 2^(D-1) frames past the tile; its 2:1 pair sums P_k live on [j0 >> k, (je >> k) + 10 * 2^(D-1-k)) and
// are overwritten in place by G_k, then gd_k.  d_k is held on [(j0 >> k) - 10, (je >> k) + 10): the LEFT halo of 10 feeds the
// weight gradient of level k + 1 (u: [j0 - 10, je)).  Parameter partial sums count OWNED positions [j0 >> k, je >> k) only.
// ---------------------------------------------------------------------------------------------
struct CausalPyrBwdArgs {
  const float* gm;
  const float* u;
  const float* d[SRF_MAX_DEPTH];
  const float* in_prelu;
  const float* w[SRF_MAX_DEPTH];
  const float* a[SRF_MAX_DEPTH];
  float* gu;
  float* part;     // [D + 1][rows][ntiles][SRF_CBWD_REC]; record D = proj_1x1's PReLU (slope sum only)
  int C, L, ntiles;
  long rows;
};

template <int D>
struct CausalPyrBwdGeom {
  static constexpr int plen(int k) { return (SRF_CBWD_TILE >> k) + (10 << (D - 1 - k)); }
  static constexpr int poff(int k) { return k == 0 ? 0 : poff(k - 1) + plen(k - 1); }
  static constexpr int dlen(int k) { return (SRF_CBWD_TILE >> k) + 20; }
  static constexpr int doff(int k) { return k == 0 ? poff(D - 1) + plen(D - 1) : doff(k - 1) + dlen(k - 1); }
  static constexpr int uoff() { return doff(D - 1) + dlen(D - 1); }
  static constexpr int floats() { return uoff() + SRF_CBWD_TILE + 10; }
};

template <int D, int K>
__device__ __forceinline__ void cb_pyr_level(const CausalPyrBwdArgs& a, float* sm, float* red, long r, int c, int tile, int j0, int je) {
  using G = CausalPyrBwdGeom<D>;
  const int Lk = a.L >> K;
  const int s = j0 >> K;
  const int own = (je >> K) - s;
  const int n = min((je >> K) + 10, Lk) - s;
  float ws[6];      // (s and the thread stride are even: a thread's positions all have the parity of its index)
  if constexpr (K < D - 1) cb_load_taps2(a.w[K + 1] + (size_t)c * SRF_CAUSAL_KW, threadIdx.x & 1, ws);
  const float ak = a.a[K][0];
  const float ain = K == 0 ? a.in_prelu[0] : a.a[K > 0 ? K - 1 : 0][0];
  float* pk = sm + G::poff(K);
  const float* dk = sm + G::doff(K) + 10;
  const float* in = K == 0 ? sm + G::uoff() : sm + G::doff(K > 0 ? K - 1 : 0);
  constexpr int stride = K == 0 ? 1 : 2;
  float acc[SRF_CBWD_REC];
#pragma unroll
  for (int q = 0; q < SRF_CBWD_REC; ++q) acc[q] = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    float Gv = pk[i];
    if constexpr (K < D - 1) {
      const float* nx = sm + G::poff(K + 1);
      const int s1 = j0 >> (K + 1);
      Gv = cb_taps2(Gv, ws, [&](int m) { return nx[m - s1]; }, s + i, a.L >> (K + 1));
    }
    const float dv = dk[i];
    const float gdv = Gv * cb_dprelu(dv, ak);
    pk[i] = gdv;
    if (i < own) {
      acc[12] += Gv * fminf(dv, 0.f);
      acc[11] += gdv;
#pragma unroll
      for (int t = 0; t < SRF_CAUSAL_TAPS; ++t) acc[t] = fmaf(gdv, srf_prelu(in[stride * i + t], ain), acc[t]);
    }
  }
  cb_block_reduce(acc, red, a.part + (((size_t)K * a.rows + r) * a.ntiles + tile) * SRF_CBWD_REC);
  if constexpr (K > 0) cb_pyr_level<D, K - 1>(a, sm, red, r, c, tile, j0, je);
}

template <int D>
__global__ __launch_bounds__(256) void srf_causal_pyramid_bwd_kernel(CausalPyrBwdArgs a) {
  using G = CausalPyrBwdGeom<D>;
  __shared__ float sm[G::floats()];
  __shared__ float red[4 * SRF_CBWD_REC];
  const long blk = blockIdx.x;
  const long r = blk / a.ntiles;
  const int tile = (int)(blk - r * a.ntiles);
  const int c = (int)(r % a.C);
  const int L = a.L;
  const int j0 = tile * SRF_CBWD_TILE;
  const int je = min(j0 + SRF_CBWD_TILE, L);
  // g_merged on [j0, je + 10 * 2^(D-1)), u on [j0 - 10, je), d_k on [(j0 >> k) - 10, (je >> k) + 10); 0 outside the row
  {
    const float* gr = a.gm + (size_t)r * L;
    const int n = (je - j0) + (10 << (D - 1));
    for (int i = threadIdx.x; i < G::plen(0); i += 256) sm[i] = (i < n && j0 + i < L) ? gr[j0 + i] : 0.f;
    const float* ur = a.u + (size_t)r * L;
    for (int i = threadIdx.x; i < je - j0 + 10; i += 256) {
      const int j = j0 - 10 + i;
      sm[G::uoff() + i] = j >= 0 ? ur[j] : 0.f;
    }
  }
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const int Lk = L >> k;
    const float* dr = a.d[k] + (size_t)r * Lk;
    const int s = (j0 >> k) - 10, e = min((je >> k) + 10, Lk);
    float* dst = sm + G::doff(k);
    for (int i = threadIdx.x; i < G::dlen(k); i += 256) {
      const int j = s + i;
      dst[i] = (j >= 0 && j < e) ? dr[j] : 0.f;
    }
  }
  __syncthreads();
  // pair sums of g_merged, level by level
#pragma unroll
  for (int k = 1; k < D; ++k) {
    const float* src = sm + G::poff(k - 1);
    float* dst = sm + G::poff(k);
    for (int i = threadIdx.x; i < G::plen(k); i += 256) dst[i] = src[2 * i] + src[2 * i + 1];
    __syncthreads();
  }
  // levels D-1 .. 0 (each ends with the block reduction of its partial sums, which is also the barrier between levels)
  cb_pyr_level<D, D - 1>(a, sm, red, r, c, tile, j0, je);
  // proj_1x1's PReLU: ga_p = conv-transpose of gd_0, gu = ga_p PReLU_p'(u)
  {
    float w[SRF_CAUSAL_TAPS];
#pragma unroll
    for (int t = 0; t < SRF_CAUSAL_TAPS; ++t) w[t] = a.w[0][(size_t)c * SRF_CAUSAL_KW + t];
    const float ap = a.in_prelu[0];
    float* gur = a.gu + (size_t)r * L;
    float acc[SRF_CBWD_REC];
#pragma unroll
    for (int q = 0; q < SRF_CBWD_REC; ++q) acc[q] = 0.f;
    for (int i = threadIdx.x; i < je - j0; i += 256) {
      const float ga = cb_taps1(0.f, w, [&](int m) { return sm[m - j0]; }, j0 + i, L);
      const float uu = sm[G::uoff() + 10 + i];
      gur[j0 + i] = ga * cb_dprelu(uu, ap);
      acc[12] += ga * fminf(uu, 0.f);
    }
    cb_block_reduce(acc, red, a.part + (((size_t)D * a.rows + r) * a.ntiles + tile) * SRF_CBWD_REC);
  }
}

extern "C" int srf_causal_pyramid_bwd_tile(void) { return SRF_CBWD_TILE; }

extern "C" int srf_causal_pyramid_bwd_supported(int C, int L, int D) {
  return C > 0 && L > 0 && D >= 1 && D <= SRF_MAX_DEPTH && L % (1 << (D - 1)) == 0 ? 1 : 0;
}

extern "C" size_t srf_causal_pyramid_bwd_scratch_bytes(int Bt, int C, int L, int D) {
  if (Bt <= 0 || !srf_causal_pyramid_bwd_supported(C, L, D)) return 0;
  return sizeof(float) * cb_part_floats((long)Bt * C, (L + SRF_CBWD_TILE - 1) / SRF_CBWD_TILE, D + 1, C);
}

extern "C" int srf_causal_pyramid_bwd(const float* g_merged, const float* u, const float* const* d, const float* in_prelu,
                                      const float* const* w, const float* const* prelu, float* gu, float* const* dw,
                                      float* const* dbias, float* const* dslope, float* dslope_in, int Bt, int C, int L, int D,
                                      void* scratch, void* stream) {
  SRF_CHECK_ARG(g_merged && u && d && in_prelu && w && prelu && gu && dw && dbias && dslope && dslope_in && scratch,
                "srf_causal_pyramid_bwd: null pointer");
  SRF_CHECK_ARG(Bt > 0, "srf_causal_pyramid_bwd: bad batch %d", Bt);
  SRF_CHECK_ARG(srf_causal_pyramid_bwd_supported(C, L, D), "srf_causal_pyramid_bwd: shape C=%d L=%d D=%d not supported", C, L, D);
  SRF_CHECK_ARG(gu != g_merged && gu != u, "srf_causal_pyramid_bwd: gu must not alias g_merged or u (tiles re-read both as halos)");
  CausalPyrBwdArgs a;
  CausalBwdFinArgs f{};
  for (int k = 0; k < D; ++k) {
    SRF_CHECK_ARG(d[k] && w[k] && prelu[k] && dw[k] && dbias[k] && dslope[k], "srf_causal_pyramid_bwd: level %d has a null pointer", k);
    SRF_CHECK_ARG(gu != d[k], "srf_causal_pyramid_bwd: gu must not alias d[%d]", k);
    a.d[k] = d[k];
    a.w[k] = w[k];
    a.a[k] = prelu[k];
    f.dw[k] = dw[k];
    f.db[k] = dbias[k];
    f.dslope[k] = dslope[k];
  }
  f.dslope[D] = dslope_in;
  a.gm = g_merged;
  a.u = u;
  a.in_prelu = in_prelu;
  a.gu = gu;
  a.part = (float*)scratch;
  a.C = C;
  a.L = L;
  a.ntiles = (L + SRF_CBWD_TILE - 1) / SRF_CBWD_TILE;
  a.rows = (long)Bt * C;
  const long blocks = a.rows * a.ntiles;
  SRF_CHECK_ARG(blocks < (1L << 31), "srf_causal_pyramid_bwd: too many blocks");
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)blocks), block(256);
  switch (D) {
    case 1: hipLaunchKernelGGL(srf_causal_pyramid_bwd_kernel<1>, grid, block, 0, st, a); break;
    case 2: hipLaunchKernelGGL(srf_causal_pyramid_bwd_kernel<2>, grid, block, 0, st, a); break;
    case 3: hipLaunchKernelGGL(srf_causal_pyramid_bwd_kernel<3>, grid, block, 0, st, a); break;
    case 4: hipLaunchKernelGGL(srf_causal_pyramid_bwd_kernel<4>, grid, block, 0, st, a); break;
    case 5: hipLaunchKernelGGL(srf_causal_pyramid_bwd_kernel<5>, grid, block, 0, st, a); break;
    case 6: hipLaunchKernelGGL(srf_causal_pyramid_bwd_kernel<6>, grid, block, 0, st, a); break;
    case 7: hipLaunchKernelGGL(srf_causal_pyramid_bwd_kernel<7>, grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL(srf_causal_pyramid_bwd_kernel<8>, grid, block, 0, st, a); break;
  }
  SRF_CHECK_LAUNCH("causal_pyramid_bwd", st);
  f.part = a.part;
  f.slope_c = a.part + (size_t)(D + 1) * a.rows * a.ntiles * SRF_CBWD_REC;
  f.C = C;
  f.Bt = Bt;
  f.nrec = a.ntiles;
  return cb_finalize(f, D + 1, st);
}

// ---------------------------------------------------------------------------------------------
// training forward's merge: y[r,j] = a_0[j] + (a_1[j>>1] + (... + a_{D-1}[j>>(D-1)])), a_k = PReLU_k(d_k) applied on load --
// the values and the sum order of srf_causal_merge on the activated levels
// ---------------------------------------------------------------------------------------------
struct CausalMergeActArgs {
  const float* d[SRF_MAX_DEPTH];
  const float* a[SRF_MAX_DEPTH];
};

__global__ __launch_bounds__(256) void srf_causal_merge_act_kernel(CausalMergeActArgs lv, float* __restrict__ y, int D, int L, long rows) {
  const long n = rows * L;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long r = i / L;
    const int j = (int)(i - r * L);
    float acc = srf_prelu(lv.d[D - 1][r * (L >> (D - 1)) + (j >> (D - 1))], lv.a[D - 1][0]);
    for (int k = D - 2; k >= 0; --k) acc = srf_prelu(lv.d[k][r * (L >> k) + (j >> k)], lv.a[k][0]) + acc;
    y[i] = acc;
  }
}

int srf_causal_merge_act(const float* const* d, const float* const* prelu, int D, float* y, int Bt, int C, int L, hipStream_t st) {
  SRF_CHECK_ARG(d && prelu && y && D >= 1 && D <= SRF_MAX_DEPTH && Bt > 0 && C > 0 && L > 0 && L % (1 << (D - 1)) == 0,
                "srf_causal_merge_act: bad arguments");
  CausalMergeActArgs lv;
  for (int k = 0; k < D; ++k) {
    SRF_CHECK_ARG(d[k] && prelu[k] && d[k] != y, "srf_causal_merge_act: level %d is null or aliases y", k);
    lv.d[k] = d[k];
    lv.a[k] = prelu[k];
  }
  const long rows = (long)Bt * C, blocks = (rows * L + 255) / 256;
  hipLaunchKernelGGL(srf_causal_merge_act_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, st, lv, y, D, L, rows);
  SRF_CHECK_LAUNCH("causal_merge_act", st);
  return SRF_OK;
}

// ---------------------------------------------------------------------------------------------
// res_conv ran as W_f = g alpha W_r, b_f = g alpha b_r (g = skipinit_gain, a device scalar).  From dW_f / db_f (held in the
// gradient tensors of W_r / b_r): d g = alpha (<dW_f, W_r> + <db_f, b_r>), then dW_r = g alpha dW_f, db_r = g alpha db_f in
// place.  One block per model block, fixed summation order.
// ---------------------------------------------------------------------------------------------
#define SRF_GAIN_MAX 32
struct CausalGainEntry {
  float* dw;
  float* db;
  const float* w;
  const float* b;
  const float* gain;
  float* dgain;
  float alpha;
  int nw, nb;
};
struct CausalGainArgs {
  CausalGainEntry e[SRF_GAIN_MAX];
};

__global__ __launch_bounds__(256) void srf_causal_gain_kernel(CausalGainArgs a) {
  __shared__ float red[4];
  const CausalGainEntry& e = a.e[blockIdx.x];
  const float s = e.gain[0] * e.alpha;
  float acc = 0.f;
  for (int i = threadIdx.x; i < e.nw; i += 256) {
    const float f = e.dw[i];
    acc = fmaf(f, e.w[i], acc);
    e.dw[i] = s * f;
  }
  for (int i = threadIdx.x; i < e.nb; i += 256) {
    const float f = e.db[i];
    acc = fmaf(f, e.b[i], acc);
    e.db[i] = s * f;
  }
  acc = srf_dpp_wave_sum(acc);
  if ((threadIdx.x & 63) == 63) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) e.dgain[0] = e.alpha * (((red[0] + red[1]) + red[2]) + red[3]);
}

int srf_causal_gain_fold(float* const* dw, float* const* db, const float* const* w, const float* const* b,
                         const float* const* gain, float* const* dgain, const float* alpha, int nw, int nb, int count,
                         hipStream_t st) {
  for (int i0 = 0; i0 < count; i0 += SRF_GAIN_MAX) {
    const int m = count - i0 < SRF_GAIN_MAX ? count - i0 : SRF_GAIN_MAX;
    CausalGainArgs a;
    for (int i = 0; i < m; ++i) {
      const int j = i0 + i;
      SRF_CHECK_ARG(dw[j] && db[j] && w[j] && b[j] && gain[j] && dgain[j], "srf_causal_gain_fold: entry %d has a null pointer", j);
      a.e[i] = CausalGainEntry{dw[j], db[j], w[j], b[j], gain[j], dgain[j], alpha[j], nw, nb};
    }
    hipLaunchKernelGGL(srf_causal_gain_kernel, dim3(m), dim3(256), 0, st, a);
    SRF_CHECK_LAUNCH("causal_gain_fold", st);
  }
  return SRF_OK;
}

// ---------------------------------------------------------------------------------------------
// encoder weight gradient [N][A K] (live taps, from the weight-gradient GEMM over gathered frames) -> the stored layout
// [N][A][2K-1]; taps K..2K-2 are written as 0 (the reference multiplies by causal_mask)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void srf_causal_enc_scatter_kernel(const float* __restrict__ src, float* __restrict__ dst, int A,
                                                                     int K, long n) {
  const int KW = 2 * K - 1;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long na = i / KW;
    const int k = (int)(i - na * KW);
    dst[i] = k < K ? src[na * K + k] : 0.f;
  }
}

int srf_causal_enc_scatter(const float* src, float* dst, int N, int A, int K, hipStream_t st) {
  SRF_CHECK_ARG(src && dst && N > 0 && A > 0 && K > 0, "srf_causal_enc_scatter: bad arguments");
  const long n = (long)N * A * (2 * K - 1), blocks = (n + 255) / 256;
  hipLaunchKernelGGL(srf_causal_enc_scatter_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, st, src, dst, A, K, n);
  SRF_CHECK_LAUNCH("causal_enc_scatter", st);
  return SRF_OK;
}

// ---------------------------------------------------------------------------------------------
// stand-alone PReLU backward (mask_net.0, mask_nl_class): srf_prelu_bwd's arithmetic, but the slope gradient is WRITTEN and
// summed without atomics -- every block leaves its partial sum in scratch, one wavefront adds them in block order -- and an
// exact 0 takes the slope branch, as torch does
// ---------------------------------------------------------------------------------------------
#define SRF_CPRELU_BLOCKS 1024

__global__ __launch_bounds__(256) void srf_causal_prelu_bwd_kernel(const float* gout, const float* __restrict__ x,
                                                                   const float* __restrict__ slope, float* gx, float* part, long n) {
  __shared__ float red[4];
  const float a = slope[0];
  float acc = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float g = gout[i], xv = x[i];
    gx[i] = g * cb_dprelu(xv, a);
    acc = fmaf(g, fminf(xv, 0.f), acc);
  }
  acc = srf_dpp_wave_sum(acc);
  if ((threadIdx.x & 63) == 63) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(64) void srf_causal_prelu_fold_kernel(const float* __restrict__ part, int nparts, float* dslope) {
  float s = 0.f;
  for (int i = threadIdx.x; i < nparts; i += 64) s += part[i];
  s = srf_dpp_wave_sum(s);
  if (threadIdx.x == 63) dslope[0] = s;
}

size_t srf_causal_prelu_bwd_scratch_floats() { return SRF_CPRELU_BLOCKS; }

int srf_causal_prelu_bwd(const float* gout, const float* x, const float* slope, float* gx, float* dslope, long n, float* scratch,
                         hipStream_t st) {
  SRF_CHECK_ARG(gout && x && slope && gx && dslope && scratch && n > 0, "srf_causal_prelu_bwd: bad arguments");
  const long blocks = (n + 255) / 256;
  const int nb = (int)(blocks < SRF_CPRELU_BLOCKS ? blocks : SRF_CPRELU_BLOCKS);
  hipLaunchKernelGGL(srf_causal_prelu_bwd_kernel, dim3(nb), dim3(256), 0, st, gout, x, slope, gx, scratch, n);
  SRF_CHECK_LAUNCH("causal_prelu_bwd", st);
  hipLaunchKernelGGL(srf_causal_prelu_fold_kernel, dim3(1), dim3(64), 0, st, scratch, nb, dslope);
  SRF_CHECK_LAUNCH("causal_prelu_fold", st);
  return SRF_OK;
}
