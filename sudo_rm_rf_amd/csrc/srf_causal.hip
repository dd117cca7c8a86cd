// Causal SuDoRM-RF (v3) kernels: CausalSuDORMRF (causal_improved_sudormrf_v3.py).  Its blocks have no GlobLN, so nothing
// here needs a statistic of a whole example and every output depends on past inputs only.
//   srf_causal_encoder        <- encoder: ScaledWSConv1d(A, N, 2K-1, stride h, padding K-1), live taps 0..K-1
//   srf_causal_dwconv         <- one spp_dw level: ConvAct(C, C, 21, stride 1|2, groups C), live taps 0..10, + PReLU
//   srf_causal_merge          <- the bottom-up nearest-x2 upsample-and-add of UConvBlock.forward
//   srf_causal_pyramid        <- all of the above for one block's pyramid in ONE launch (y1 read once, merged written once)
//   srf_causal_scale          <- skipinit_gain * alpha folded into res_conv, 1 / beta into proj_1x1 (device scalars)
//   srf_prelu_apply           <- a stand-alone nn.PReLU (ConvAct with a 1x1 conv)
// The masked taps of the stored weights (the reference multiplies them by causal_mask at every forward) are never read.
#include "srf_internal.h"

#define SRF_CAUSAL_TILE 1024 // level-0 frames per block of the fused pyramid

// ---------------------------------------------------------------------------------------------
// encoder: out[b,n,l] = sum_{a, k<K} w[n,a,k] x[b,a, h l + k - 2h]   (weight row stride 2K-1; samples outside [0,T) are 0)
// 64 frames per block, the input window staged in LDS, one basis function per wavefront and step (taps are scalar operands).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void srf_causal_encoder_kernel(const float* __restrict__ wav, const float* __restrict__ w,
                                                                 float* __restrict__ out, int A, int T, int N, int K, int L) {
  extern __shared__ float win[];   // [A][WIN]
  const int H = K / 2, KW = 2 * K - 1;
  const int WIN = 63 * H + K;
  const int b = blockIdx.y;
  const int l0 = blockIdx.x * 64;
  for (int i = threadIdx.x; i < A * WIN; i += 256) {
    const int a = i / WIN, j = i - a * WIN;
    const long t = (long)H * l0 - 2 * H + j;
    win[i] = (t >= 0 && t < T) ? wav[((size_t)b * A + a) * T + t] : 0.f;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l = l0 + lane;
  const int per = ((N + (int)gridDim.z - 1) / (int)gridDim.z + 3) & ~3;
  const int n_lo = blockIdx.z * per, n_hi = min(N, n_lo + per);
  for (int n = n_lo + wave; n < n_hi; n += 4) {
    float acc = 0.f;
    for (int a = 0; a < A; ++a) {
      const float* wn = w + ((size_t)n * A + a) * KW;
      const float* xw = win + a * WIN + H * lane;
      for (int k = 0; k < K; ++k) acc = fmaf(wn[k], xw[k], acc);
    }
    if (l < L) out[((size_t)b * N + n) * L + l] = acc;
  }
}

extern "C" int srf_causal_encoder(const float* wav, const float* w, float* out, int Bt, int A, int T, int N, int K, int L,
                                  void* stream) {
  SRF_CHECK_ARG(wav && w && out, "srf_causal_encoder: null pointer");
  SRF_CHECK_ARG(Bt > 0 && A > 0 && T > 0 && N > 0 && L > 0, "srf_causal_encoder: bad sizes");
  SRF_CHECK_ARG(K >= 3 && (K & 1), "srf_causal_encoder: enc_kernel_size must be odd (got %d)", K);
  SRF_CHECK_ARG(Bt <= 65535, "srf_causal_encoder: batch %d too large for one launch", Bt);
  const size_t lds = sizeof(float) * (size_t)A * (63 * (K / 2) + K);
  SRF_CHECK_ARG(lds <= 64 * 1024, "srf_causal_encoder: window does not fit LDS (A=%d K=%d)", A, K);
  hipStream_t st = (hipStream_t)stream;
  // basis slices per (time tile, example) so that a batch-1 forward still fills the GPU (at least 16 functions per slice)
  const long bxy = (long)((L + 63) / 64) * Bt, want = 16L * srf_device_cus();
  int nz = bxy >= want ? 1 : (int)((want + bxy - 1) / bxy);
  const int nz_max = N / 16 > 0 ? N / 16 : 1;
  nz = nz > nz_max ? nz_max : nz;
  hipLaunchKernelGGL(srf_causal_encoder_kernel, dim3((L + 63) / 64, Bt, nz), dim3(256), lds, st, wav, w, out, A, T, N, K, L);
  SRF_CHECK_LAUNCH("causal_encoder", st);
  return SRF_OK;
}

// ---------------------------------------------------------------------------------------------
// one pyramid level: y[r,j] = PReLU_out(bias[c] + sum_{k<11} w[c,k] f(x[r, s j - 10 + k])), r = (b,c), f = PReLU_in or
// identity, zero outside [0, Lin) after f.  The conv is causal, so s j - 10 + k <= s j <= Lin - 1: only the left edge pads.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void srf_causal_dw_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ bias, const float* __restrict__ in_prelu,
                                                            const float* __restrict__ out_prelu, float* __restrict__ y, long rows,
                                                            int C, int Lin, int Lout, int stride) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  const float ai = in_prelu ? in_prelu[0] : 1.f;
  for (long r = blockIdx.y; r < rows; r += gridDim.y) {
    if (j >= Lout) continue;
    const int c = (int)(r % C);
    const float* xr = x + (size_t)r * Lin;
    const float* wc = w + (size_t)c * SRF_CAUSAL_KW;
    float acc = bias[c];
#pragma unroll
    for (int k = 0; k < SRF_CAUSAL_TAPS; ++k) {
      const int t = stride * j - (SRF_CAUSAL_TAPS - 1) + k;
      float v = t >= 0 ? xr[t] : 0.f;
      if (in_prelu) v = srf_prelu(v, ai);
      acc = fmaf(wc[k], v, acc);
    }
    y[(size_t)r * Lout + j] = out_prelu ? srf_prelu(acc, out_prelu[0]) : acc;
  }
}

extern "C" int srf_causal_dwconv(const float* x, const float* w, const float* bias, const float* in_prelu,
                                 const float* out_prelu, float* y, int Bt, int C, int Lin, int stride, void* stream) {
  SRF_CHECK_ARG(x && w && bias && y, "srf_causal_dwconv: null pointer");
  SRF_CHECK_ARG(Bt > 0 && C > 0 && Lin > 0, "srf_causal_dwconv: bad sizes");
  SRF_CHECK_ARG(stride == 1 || stride == 2, "srf_causal_dwconv: stride must be 1 or 2 (got %d)", stride);
  SRF_CHECK_ARG(x != y, "srf_causal_dwconv: y must not alias x");
  const int Lout = (Lin - 1) / stride + 1;
  const long rows = (long)Bt * C;
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((Lout + 255) / 256, (unsigned)(rows < 65535 ? rows : 65535));
  hipLaunchKernelGGL(srf_causal_dw_kernel, grid, dim3(256), 0, st, x, w, bias, in_prelu, out_prelu, y, rows, C, Lin, Lout,
                     stride);
  SRF_CHECK_LAUNCH("causal_dwconv", st);
  return SRF_OK;
}

// ---------------------------------------------------------------------------------------------
// merge: y[r,j] = l_0[j] + (l_1[j>>1] + (... + l_{D-1}[j>>(D-1)])) -- the reference's bottom-up order
// ---------------------------------------------------------------------------------------------
struct CausalLevels {
  const float* p[SRF_MAX_DEPTH];
};

__global__ __launch_bounds__(256) void srf_causal_merge_kernel(CausalLevels lv, float* __restrict__ y, int D, int L, long rows) {
  const long n = rows * L;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long r = i / L;
    const int j = (int)(i - r * L);
    float acc = lv.p[D - 1][r * (L >> (D - 1)) + (j >> (D - 1))];
    for (int k = D - 2; k >= 0; --k) acc = lv.p[k][r * (L >> k) + (j >> k)] + acc;
    y[i] = acc;
  }
}

extern "C" int srf_causal_merge(const float* const* levels, int D, float* y, int Bt, int C, int L, void* stream) {
  SRF_CHECK_ARG(levels && y, "srf_causal_merge: null pointer");
  SRF_CHECK_ARG(D >= 1 && D <= SRF_MAX_DEPTH, "srf_causal_merge: depth %d unsupported (1..%d)", D, SRF_MAX_DEPTH);
  SRF_CHECK_ARG(Bt > 0 && C > 0 && L > 0 && L % (1 << (D - 1)) == 0, "srf_causal_merge: L=%d must be a positive multiple of 2^(D-1)", L);
  CausalLevels lv;
  for (int k = 0; k < D; ++k) {
    SRF_CHECK_ARG(levels[k] && levels[k] != y, "srf_causal_merge: level %d is null or aliases y", k);
    lv.p[k] = levels[k];
  }
  const long rows = (long)Bt * C, n = rows * L;
  const long blocks = (n + 255) / 256;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(srf_causal_merge_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, st, lv, y, D, L, rows);
  SRF_CHECK_LAUNCH("causal_merge", st);
  return SRF_OK;
}

// ---------------------------------------------------------------------------------------------
// fused pyramid.  One block = one row (b, c) x one tile of TILE level-0 frames [j0, je).  Every level of the tile lives in
// LDS; the one-sided dependency cone is recomputed per tile as a LEFT halo: level k is produced on [s_k, je >> k) with
//   s_{D-1} = j0 >> (D-1),   s_k = 2 s_{k+1} - 10      (H_k = (j0 >> k) - s_k = 10 (2^(D-1-k) - 1) extra frames)
// and PReLU_p(y1) is loaded on [s_0 - 10, je), i.e. 10 * 2^(D-1) frames left of the tile.  Frames at negative indices are
// the zero padding of the next level's conv.  Same FMA order per output as srf_causal_dw_kernel and same sum order as
// srf_causal_merge_kernel: the fused and per-level paths are bit-identical.
// ---------------------------------------------------------------------------------------------
struct CausalPyrArgs {
  const float* y1;
  float* merged;
  const float* in_prelu;
  const float* w[SRF_MAX_DEPTH];
  const float* b[SRF_MAX_DEPTH];
  const float* a[SRF_MAX_DEPTH];
  int C, L, ntiles;
  int vec;   // y1 rows 16-byte aligned (L % 4 == 0, aligned base): quad loads
  long rows;
};

template <int D>
struct CausalPyrGeom {
  static constexpr int HY = 10 << (D - 1);                       // y1 frames loaded left of the tile
  static constexpr int halo(int k) { return 10 * ((1 << (D - 1 - k)) - 1); }
  static constexpr int len(int k) { return (SRF_CAUSAL_TILE >> k) + halo(k); }
  static constexpr int off(int k) { return k == 0 ? SRF_CAUSAL_TILE + HY : off(k - 1) + len(k - 1); }
  static constexpr int floats() { return off(D); }
};

template <int D>
__global__ __launch_bounds__(256) void srf_causal_pyramid_kernel(CausalPyrArgs a) {
  using G = CausalPyrGeom<D>;
  __shared__ float sm[G::floats()];
  const long blk = blockIdx.x;
  const long r = blk / a.ntiles;
  const int tile = (int)(blk - r * a.ntiles);
  const int c = (int)(r % a.C);
  const int L = a.L;
  const int j0 = tile * SRF_CAUSAL_TILE;
  const int je = min(j0 + SRF_CAUSAL_TILE, L);
  const float* yr = a.y1 + (size_t)r * L;
  // PReLU_p(y1) on [j0 - HY, je)
  {
    const float ap = a.in_prelu[0];
    const int n = je - j0 + G::HY;
    const int t0 = j0 - G::HY;
    if (a.vec && (G::HY & 3) == 0) {
      for (int i = 4 * threadIdx.x; i < n; i += 4 * 256) {
        const int t = t0 + i;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t >= 0) v = srf_ld4<false>(yr + t);   // (t and the tile bounds are multiples of 4: a quad is all in or all out)
        sm[i] = srf_prelu(v.x, ap);
        sm[i + 1] = srf_prelu(v.y, ap);
        sm[i + 2] = srf_prelu(v.z, ap);
        sm[i + 3] = srf_prelu(v.w, ap);
      }
    } else {
      for (int i = threadIdx.x; i < n; i += 256) {
        const int t = t0 + i;
        sm[i] = t >= 0 ? srf_prelu(yr[t], ap) : 0.f;
      }
    }
  }
  __syncthreads();
  // levels: buffer k holds level k on [s_k, e_k)
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const float* in = k == 0 ? sm : sm + G::off(k - 1);
    float* outk = sm + G::off(k);
    const int stride = k == 0 ? 1 : 2;
    const int s = (j0 >> k) - G::halo(k);
    const int n = (je >> k) - s;
    const float* wc = a.w[k] + (size_t)c * SRF_CAUSAL_KW;
    float wk[SRF_CAUSAL_TAPS];
#pragma unroll
    for (int q = 0; q < SRF_CAUSAL_TAPS; ++q) wk[q] = wc[q];
    const float bk = a.b[k][c], ak = a.a[k][0];
    for (int i = threadIdx.x; i < n; i += 256) {
      float v = 0.f;
      if (s + i >= 0) {
        float acc = bk;
#pragma unroll
        for (int q = 0; q < SRF_CAUSAL_TAPS; ++q) acc = fmaf(wk[q], in[stride * i + q], acc);
        v = srf_prelu(acc, ak);
      }
      outk[i] = v;
    }
    __syncthreads();
  }
  // merge, bottom-up
  float* mr = a.merged + (size_t)r * L;
  for (int j = j0 + threadIdx.x; j < je; j += 256) {
    float acc = sm[G::off(D - 1) + (j >> (D - 1)) - (j0 >> (D - 1))];
#pragma unroll
    for (int k = D - 2; k >= 0; --k) acc = sm[G::off(k) + (j >> k) - ((j0 >> k) - G::halo(k))] + acc;
    mr[j] = acc;
  }
}

extern "C" int srf_causal_pyramid_supported(int C, int L, int D) {
  return C > 0 && L > 0 && D >= 1 && D <= SRF_MAX_DEPTH && L % (1 << (D - 1)) == 0 ? 1 : 0;
}

extern "C" int srf_causal_pyramid(const float* y1, float* merged, const float* in_prelu, const float* const* w,
                                  const float* const* bias, const float* const* prelu, int Bt, int C, int L, int D,
                                  void* stream) {
  SRF_CHECK_ARG(y1 && merged && in_prelu && w && bias && prelu, "srf_causal_pyramid: null pointer");
  SRF_CHECK_ARG(Bt > 0, "srf_causal_pyramid: bad batch %d", Bt);
  SRF_CHECK_ARG(srf_causal_pyramid_supported(C, L, D), "srf_causal_pyramid: shape C=%d L=%d D=%d not supported", C, L, D);
  SRF_CHECK_ARG(y1 != merged, "srf_causal_pyramid: merged must not alias y1 (neighbouring tiles re-read y1 as their halo)");
  CausalPyrArgs a;
  a.y1 = y1;
  a.merged = merged;
  a.in_prelu = in_prelu;
  for (int k = 0; k < D; ++k) {
    SRF_CHECK_ARG(w[k] && bias[k] && prelu[k], "srf_causal_pyramid: level %d parameter is null", k);
    a.w[k] = w[k];
    a.b[k] = bias[k];
    a.a[k] = prelu[k];
  }
  a.C = C;
  a.L = L;
  a.ntiles = (L + SRF_CAUSAL_TILE - 1) / SRF_CAUSAL_TILE;
  a.rows = (long)Bt * C;
  a.vec = (L % 4 == 0) && srf_aligned16(y1);
  const long blocks = a.rows * a.ntiles;
  SRF_CHECK_ARG(blocks < (1L << 31), "srf_causal_pyramid: too many blocks");
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)blocks), block(256);
  switch (D) {
    case 1: hipLaunchKernelGGL(srf_causal_pyramid_kernel<1>, grid, block, 0, st, a); break;
    case 2: hipLaunchKernelGGL(srf_causal_pyramid_kernel<2>, grid, block, 0, st, a); break;
    case 3: hipLaunchKernelGGL(srf_causal_pyramid_kernel<3>, grid, block, 0, st, a); break;
    case 4: hipLaunchKernelGGL(srf_causal_pyramid_kernel<4>, grid, block, 0, st, a); break;
    case 5: hipLaunchKernelGGL(srf_causal_pyramid_kernel<5>, grid, block, 0, st, a); break;
    case 6: hipLaunchKernelGGL(srf_causal_pyramid_kernel<6>, grid, block, 0, st, a); break;
    case 7: hipLaunchKernelGGL(srf_causal_pyramid_kernel<7>, grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL(srf_causal_pyramid_kernel<8>, grid, block, 0, st, a); break;
  }
  SRF_CHECK_LAUNCH("causal_pyramid", st);
  return SRF_OK;
}

// ---------------------------------------------------------------------------------------------
// scaled copies: dst_i = src_i * (dscale_i ? dscale_i[0] : 1) * hscale_i, several tensors per launch.  dscale is a DEVICE
// scalar (skipinit_gain): the fold never synchronises with the host.
// ---------------------------------------------------------------------------------------------
#define SRF_SCALE_MAX 48
struct CausalScaleEntry {
  const float* src;
  float* dst;
  const float* dscale;
  float hscale;
  long n;
};
struct CausalScaleArgs {
  CausalScaleEntry e[SRF_SCALE_MAX];
};

__global__ __launch_bounds__(256) void srf_causal_scale_kernel(CausalScaleArgs a) {
  const CausalScaleEntry& e = a.e[blockIdx.y];
  const float s = (e.dscale ? e.dscale[0] : 1.f) * e.hscale;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < e.n; i += (long)gridDim.x * 256) e.dst[i] = e.src[i] * s;
}

// (library-internal: srf_forward folds every block's scales with as few launches as possible)
int srf_causal_scale_many(const float* const* src, float* const* dst, const long* n, const float* const* dscale,
                          const float* hscale, int count, hipStream_t st) {
  for (int i0 = 0; i0 < count; i0 += SRF_SCALE_MAX) {
    const int m = count - i0 < SRF_SCALE_MAX ? count - i0 : SRF_SCALE_MAX;
    CausalScaleArgs a;
    long longest = 1;
    for (int i = 0; i < m; ++i) {
      SRF_CHECK_ARG(src[i0 + i] && dst[i0 + i] && n[i0 + i] > 0, "srf_causal_scale: bad entry %d", i0 + i);
      a.e[i] = CausalScaleEntry{src[i0 + i], dst[i0 + i], dscale[i0 + i], hscale[i0 + i], n[i0 + i]};
      longest = n[i0 + i] > longest ? n[i0 + i] : longest;
    }
    const long bx = (longest + 255) / 256;
    hipLaunchKernelGGL(srf_causal_scale_kernel, dim3((unsigned)(bx < 256 ? bx : 256), m), dim3(256), 0, st, a);
    SRF_CHECK_LAUNCH("causal_scale", st);
  }
  return SRF_OK;
}

extern "C" int srf_causal_scale(const float* src, float* dst, long n, const float* dscale, float hscale, void* stream) {
  SRF_CHECK_ARG(src && dst && n > 0, "srf_causal_scale: bad arguments");
  return srf_causal_scale_many(&src, &dst, &n, &dscale, &hscale, 1, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// y = PReLU_a(x) elementwise (a stand-alone nn.PReLU with one shared slope)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void srf_prelu_apply_kernel(const float* __restrict__ x, const float* __restrict__ slope,
                                                              float* __restrict__ y, long n) {
  const float a = slope[0];
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) y[i] = srf_prelu(x[i], a);
}

extern "C" int srf_prelu_apply(const float* x, const float* slope, float* y, long n, void* stream) {
  SRF_CHECK_ARG(x && slope && y && n > 0, "srf_prelu_apply: bad arguments");
  const long blocks = (n + 255) / 256;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(srf_prelu_apply_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, st, x, slope, y, n);
  SRF_CHECK_LAUNCH("prelu_apply", st);
  return SRF_OK;
}
