// Original SuDoRM-RF (sudormrf.py) training step, device side: srf_original_forward_train keeps what the
// backward needs, srf_original_backward turns d loss / d output into every parameter gradient -- torch autograd over the
// reference's SuDORMRF.forward, as a walk over this library's backward kernels plus the six this model has that no other has
// (below).  Opt-in: the general training entry points (srf_train.hip) keep refusing original plans.
//   saved   : GroupNorm statistics | encoder output s | block stream x_0 .. x_U | per block: y1, the D raw levels d_k, m, g,
//             g + x | reshape_before_masks' output (B != N) | the logits z.  The activations a = PReLU_c(proj_1x1.norm(y1)) and
//             e = PReLU_c(final_norm(m)) are re-computed in the backward, one srf_gln_apply_c launch each.
//   grads   : ACCUMULATED into, same order and shapes as the parameters; ln_mask_in.* (the last two) are never touched.
// Every reduction of the new kernels writes block partials and adds them in a fixed order: no floating-point atomics.
#include <vector>
#include "srf_original_walk.h"

namespace {

// Block-wide sum in a fixed order: the lanes of a wavefront by xor-shuffles, then the four wavefronts left to right.  Every
// thread of the 256-thread block must reach it; every thread gets the total.  sh: 4 entries of LDS.
template <typename T>
__device__ __forceinline__ T ot_block_sum(T v, T* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) sh[w] = v;
  __syncthreads();
  const T r = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  __syncthreads();
  return r;
}

// dwords from p up to the 16-byte grid (0 .. 3), at most n
__device__ __forceinline__ int ot_head(const void* p, long n) {
  const long h = (long)(((16 - ((size_t)p & 15)) & 15) >> 2);
  return (int)(h < n ? h : n);
}

// ---------------------------------------------------------------------------------------------
// srf_gln_c_bwd: backward of y = [PReLU_c](GroupNorm(1, C)(x)) [+ add].  One block per (row = (g, c), chunk of GCB_CHUNK
// positions) in both launches, as srf_gln_apply_c.  VEC: gout, gout2, x and gx share their phase on the 16-byte grid -- a scalar
// head up to the grid, 16-byte loads / stores, a scalar tail; else dwords.
//   reduce : part[block] = {sum g', sum g' xh, sum gout v [v < 0], 0}
//   apply  : the example's S1 = sum_c gamma_c part[.][0], S2 = sum_c gamma_c part[.][1] (fp64, fixed order), then
//            gx = rstd (gamma_c g' - S1 / n - xh S2 / n); the block of (g = 0, chunk 0) of every channel adds the channel's
//            partials over the batch, in block order, onto dgamma / dbeta / dslope.
// ---------------------------------------------------------------------------------------------
constexpr int GCB_CHUNK = 2048;

struct GlnCBwdArgs {
  const float *gout, *gout2, *x;
  SrfNormDev nrm;
  const float* slopes;
  float* gx;
  float *dgamma, *dbeta, *dslope;
  float* part;      // [groups * C * chunks][4]
  double inv_count;
  int groups, C, L, chunks, accumulate;
};

struct GlnCBwdRow {
  float mean, rstd, gam, bet, slope;
  bool act;
};
// g' and xh of one element; sneg += gout v where v <= 0 (torch's convention, as in srf_gln_bwd: the slope at 0 and -0.0)
__device__ __forceinline__ void gln_c_bwd_elem(float gv, float x, const GlnCBwdRow& r, float& xh, float& gp, float& sneg) {
  xh = (x - r.mean) * r.rstd;
  const float v = fmaf(r.gam, xh, r.bet);
  const bool neg = r.act && v <= 0.f;
  sneg = fmaf(neg ? gv : 0.f, v, sneg);
  gp = neg ? gv * r.slope : gv;
}

__device__ __forceinline__ GlnCBwdRow gln_c_bwd_row(const GlnCBwdArgs& a, long g, int c) {
  GlnCBwdRow r;
  srf_finalize_stats(a.nrm.sums, g, a.inv_count, r.mean, r.rstd);
  r.gam = a.nrm.gamma[c];
  r.bet = a.nrm.beta[c];
  r.act = a.slopes != nullptr;
  r.slope = r.act ? a.slopes[c] : 1.f;
  return r;
}

template <bool VEC>
__global__ __launch_bounds__(256) void srf_gln_c_bwd_reduce_kernel(GlnCBwdArgs a) {
  __shared__ float sh[4];
  const long row = blockIdx.x / a.chunks;
  const int chunk = (int)(blockIdx.x - row * a.chunks);
  const int c = (int)(row % a.C);
  const long g = row / a.C;
  const GlnCBwdRow r = gln_c_bwd_row(a, g, c);
  const size_t base = (size_t)row * a.L + (size_t)chunk * GCB_CHUNK;
  const int cnt = min(GCB_CHUNK, a.L - chunk * GCB_CHUNK);
  const float* go = a.gout + base;
  const float* go2 = a.gout2 ? a.gout2 + base : nullptr;
  const float* xp = a.x + base;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  auto one = [&](float gv, float xv) {
    float xh, gp;
    gln_c_bwd_elem(gv, xv, r, xh, gp, s2);
    s0 += gp;
    s1 = fmaf(gp, xh, s1);
  };
  auto scalar = [&](int i) { one(go2 ? go[i] + go2[i] : go[i], xp[i]); };
  if constexpr (VEC) {
    const int head = ot_head(xp, cnt);
    const int nv = (cnt - head) >> 2;
    const int tail0 = head + 4 * nv;
    if ((int)threadIdx.x < head) scalar(threadIdx.x);
    for (int i = threadIdx.x; i < nv; i += 256) {
      float4 gv = *reinterpret_cast<const float4*>(go + head + 4 * i);
      const float4 xv = *reinterpret_cast<const float4*>(xp + head + 4 * i);
      if (go2) {
        const float4 t = *reinterpret_cast<const float4*>(go2 + head + 4 * i);
        gv.x += t.x, gv.y += t.y, gv.z += t.z, gv.w += t.w;
      }
      one(gv.x, xv.x), one(gv.y, xv.y), one(gv.z, xv.z), one(gv.w, xv.w);
    }
    if ((int)threadIdx.x < cnt - tail0) scalar(tail0 + threadIdx.x);
  } else {
    for (int i = threadIdx.x; i < cnt; i += 256) scalar(i);
  }
  s0 = ot_block_sum(s0, sh);
  s1 = ot_block_sum(s1, sh);
  s2 = ot_block_sum(s2, sh);
  if (threadIdx.x == 0) *reinterpret_cast<float4*>(a.part + (size_t)blockIdx.x * 4) = make_float4(s0, s1, s2, 0.f);
}

template <bool VEC>
__global__ __launch_bounds__(256) void srf_gln_c_bwd_apply_kernel(GlnCBwdArgs a) {
  __shared__ double shd[4];
  const long row = blockIdx.x / a.chunks;
  const int chunk = (int)(blockIdx.x - row * a.chunks);
  const int c = (int)(row % a.C);
  const long g = row / a.C;
  const GlnCBwdRow r = gln_c_bwd_row(a, g, c);
  // the example's two sums, from every (channel, chunk) partial of the example: the same order in every block
  const int per = a.C * a.chunks;
  const float4* pe = reinterpret_cast<const float4*>(a.part) + (size_t)g * per;
  double d1 = 0.0, d2 = 0.0;
  for (int i = threadIdx.x; i < per; i += 256) {
    const float4 t = pe[i];
    const double gm = (double)a.nrm.gamma[i / a.chunks];
    d1 += gm * (double)t.x;
    d2 += gm * (double)t.y;
  }
  const float m1 = (float)(ot_block_sum(d1, shd) * a.inv_count), m2 = (float)(ot_block_sum(d2, shd) * a.inv_count);
  const size_t base = (size_t)row * a.L + (size_t)chunk * GCB_CHUNK;
  const int cnt = min(GCB_CHUNK, a.L - chunk * GCB_CHUNK);
  const float* go = a.gout + base;
  const float* go2 = a.gout2 ? a.gout2 + base : nullptr;
  const float* xp = a.x + base;
  float* gxp = a.gx + base;
  auto one = [&](float gv, float xv) {
    float xh, gp, unused = 0.f;
    gln_c_bwd_elem(gv, xv, r, xh, gp, unused);
    return r.rstd * (r.gam * gp - m1 - xh * m2);
  };
  auto scalar = [&](int i) {
    float o = one(go2 ? go[i] + go2[i] : go[i], xp[i]);
    if (a.accumulate) o += gxp[i];
    gxp[i] = o;
  };
  if constexpr (VEC) {
    const int head = ot_head(xp, cnt);
    const int nv = (cnt - head) >> 2;
    const int tail0 = head + 4 * nv;
    if ((int)threadIdx.x < head) scalar(threadIdx.x);
    for (int i = threadIdx.x; i < nv; i += 256) {
      float4 gv = *reinterpret_cast<const float4*>(go + head + 4 * i);
      const float4 xv = *reinterpret_cast<const float4*>(xp + head + 4 * i);
      if (go2) {
        const float4 t = *reinterpret_cast<const float4*>(go2 + head + 4 * i);
        gv.x += t.x, gv.y += t.y, gv.z += t.z, gv.w += t.w;
      }
      float4 o = make_float4(one(gv.x, xv.x), one(gv.y, xv.y), one(gv.z, xv.z), one(gv.w, xv.w));
      if (a.accumulate) {
        const float4 t = *reinterpret_cast<const float4*>(gxp + head + 4 * i);
        o.x += t.x, o.y += t.y, o.z += t.z, o.w += t.w;
      }
      *reinterpret_cast<float4*>(gxp + head + 4 * i) = o;
    }
    if ((int)threadIdx.x < cnt - tail0) scalar(tail0 + threadIdx.x);
  } else {
    for (int i = threadIdx.x; i < cnt; i += 256) scalar(i);
  }
  // the channel's parameter sums over the batch: one block per channel, partials added in block order
  if (g == 0 && chunk == 0 && (a.dgamma || a.dbeta || a.dslope)) {      // (block-uniform)
    const int n = a.groups * a.chunks;
    const float4* pa = reinterpret_cast<const float4*>(a.part);
    double t0 = 0.0, t1 = 0.0, t2 = 0.0;
    for (int j = threadIdx.x; j < n; j += 256) {
      const int gi = j / a.chunks, k = j - gi * a.chunks;
      const float4 t = pa[((size_t)gi * a.C + c) * a.chunks + k];
      t0 += (double)t.x, t1 += (double)t.y, t2 += (double)t.z;
    }
    t0 = ot_block_sum(t0, shd);
    t1 = ot_block_sum(t1, shd);
    t2 = ot_block_sum(t2, shd);
    if (threadIdx.x == 0) {
      if (a.dbeta) a.dbeta[c] += (float)t0;
      if (a.dgamma) a.dgamma[c] += (float)t1;
      if (a.dslope) a.dslope[c] += (float)t2;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// srf_softmax_mask_bwd: one thread per (b, i, l) as srf_softmax_mask -- the S logits and the S incoming gradients of the thread
// in registers (SMAX = 4 serves S <= 4, SMAX = 16 the rest), the source planes walked with one per-lane pointer.  With
// dot = sum_r p_r gv_r:  gz_s = p_s enc (gv_s - dot),  genc = dot.  gz may be gv: a thread reads all of its gv before it writes.
// ---------------------------------------------------------------------------------------------
template <int SMAX>
__global__ __launch_bounds__(256) void srf_softmax_mask_bwd_kernel(const float* __restrict__ z, const float* __restrict__ enc,
                                                                   const float* gv, float* gz, float* __restrict__ genc, int acc,
                                                                   int S, int N, int L, size_t per_example, size_t total) {
  const size_t plane = (size_t)N * L;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const size_t b = idx / per_example, r = idx - b * per_example;
    const size_t at = b * S * plane + r;
    const float e = enc[idx];
    float zv[SMAX], gg[SMAX];
    float mx = -__builtin_inff();
    const float* zp = z + at;
    const float* gp = gv + at;
#pragma unroll
    for (int s = 0; s < SMAX; ++s) {
      zv[s] = -__builtin_inff();
      gg[s] = 0.f;
      if (s < S) {
        zv[s] = *zp;
        gg[s] = *gp;
        zp += plane;
        gp += plane;
      }
      mx = fmaxf(mx, zv[s]);
    }
    float ge;
    if (S == 1) {
      // p as the forward has it; 1 - p without cancellation: q p on the side where q = expf(-z) is small, else 1 / (1 + expf(z))
      const float q = expf(-zv[0]);
      const float p = 1.f / (1.f + q);
      const float omp = zv[0] >= 0.f ? q * p : 1.f / (1.f + expf(zv[0]));
      ge = gg[0] * p;
      gz[at] = (gg[0] * e) * (p * omp);
    } else {
      float sum = 0.f;
#pragma unroll
      for (int s = 0; s < SMAX; ++s) {
        zv[s] = expf(zv[s] - mx);      // (a source past S: expf(-inf) = 0)
        sum += zv[s];
      }
      const float inv = 1.f / sum;
      float dot = 0.f;
#pragma unroll
      for (int s = 0; s < SMAX; ++s) {
        zv[s] *= inv;
        dot = fmaf(zv[s], gg[s], dot);
      }
      ge = dot;
      float* op = gz + at;
#pragma unroll
      for (int s = 0; s < SMAX; ++s)
        if (s < S) {
          *op = (zv[s] * e) * (gg[s] - dot);
          op += plane;
        }
    }
    genc[idx] = acc ? genc[idx] + ge : ge;
  }
}

// ---------------------------------------------------------------------------------------------
// srf_mask_weight_fold: one block per (s, tap j): the diagonal n - i + pad = j of source s's [N, N] block of dtz; the blocks of
// tap 0 also add the source's N bias rows.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void srf_mask_weight_fold_kernel(const float* __restrict__ dtz, const float* __restrict__ drow,
                                                                   float* __restrict__ dmw, float* __restrict__ dmb, int N) {
  __shared__ double shd[4];
  const int s = blockIdx.x / (N + 1), j = blockIdx.x - s * (N + 1);
  const int pad = N - N / 2;
  double acc = 0.0;
  for (int i = threadIdx.x; i < N; i += 256) {
    const int n = j + i - pad;
    if (n >= 0 && n < N) acc += (double)dtz[((size_t)s * N + i) * N + n];
  }
  acc = ot_block_sum(acc, shd);
  if (threadIdx.x == 0) dmw[(size_t)s * (N + 1) + j] += (float)acc;
  if (j == 0) {      // (block-uniform)
    double b = 0.0;
    for (int i = threadIdx.x; i < N; i += 256) b += (double)drow[(size_t)s * N + i];
    b = ot_block_sum(b, shd);
    if (threadIdx.x == 0) dmb[s] += (float)b;
  }
}

// dw[c, k] += dwexp[c, c / N, k]
__global__ __launch_bounds__(256) void srf_decoder_weight_contract_kernel(const float* __restrict__ dwexp, float* __restrict__ dw, int N,
                                                                          int S, int K) {
  const size_t total = (size_t)S * N * K;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int k = (int)(idx % K);
    const size_t c = idx / K;
    dw[idx] += dwexp[(c * S + c / N) * K + k];
  }
}

// ---------------------------------------------------------------------------------------------
// srf_decoder_bias_grad: DBG_PARTS blocks per source write their sums of grad_out[:, s, :] (a grid stride over (b, t)), then one
// wavefront per source adds them in block order.
// ---------------------------------------------------------------------------------------------
constexpr int DBG_PARTS = 128;
__global__ __launch_bounds__(256) void srf_decoder_bias_part_kernel(const float* __restrict__ go, float* __restrict__ part, int S, int T,
                                                                    size_t per_source) {
  __shared__ double shd[4];
  const int s = blockIdx.y;
  double acc = 0.0;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < per_source; idx += (size_t)DBG_PARTS * 256) {
    const size_t b = idx / T, t = idx - b * T;
    acc += (double)go[(b * S + s) * T + t];
  }
  acc = ot_block_sum(acc, shd);
  if (threadIdx.x == 0) part[(size_t)s * DBG_PARTS + blockIdx.x] = (float)acc;
}
__global__ __launch_bounds__(64) void srf_decoder_bias_fold_kernel(const float* __restrict__ part, float* __restrict__ dbias) {
  const int s = blockIdx.x;
  double acc = 0.0;
  for (int i = threadIdx.x; i < DBG_PARTS; i += 64) acc += (double)part[(size_t)s * DBG_PARTS + i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (threadIdx.x == 0) dbias[s] += (float)acc;
}

// g *= [s > 0]; VEC: g and s share their phase on the 16-byte grid
template <bool VEC>
__global__ __launch_bounds__(256) void srf_relu_gate_kernel(float* __restrict__ g, const float* __restrict__ s, long n) {
  const long tid = (long)blockIdx.x * 256 + threadIdx.x, step = (long)gridDim.x * 256;
  auto one = [&](long i) { g[i] = s[i] > 0.f ? g[i] : 0.f; };
  if constexpr (VEC) {
    const int head = ot_head(g, n);
    const long nv = (n - head) >> 2, tail0 = head + 4 * nv;
    if (tid < head) one(tid);
    for (long i = tid; i < nv; i += step) {
      float4 a = *reinterpret_cast<const float4*>(g + head + 4 * i);
      const float4 b = *reinterpret_cast<const float4*>(s + head + 4 * i);
      a.x = b.x > 0.f ? a.x : 0.f, a.y = b.y > 0.f ? a.y : 0.f, a.z = b.z > 0.f ? a.z : 0.f, a.w = b.w > 0.f ? a.w : 0.f;
      *reinterpret_cast<float4*>(g + head + 4 * i) = a;
    }
    if (tid < n - tail0) one(tail0 + tid);
  } else {
    for (long i = tid; i < n; i += step) one(i);
  }
}

inline bool ot_float_aligned(std::initializer_list<const void*> ps) {
  size_t v = 0;
  for (const void* p : ps) v |= (size_t)p;
  return (v & 3) == 0;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// kernel entry points
// ---------------------------------------------------------------------------------------------
extern "C" size_t srf_gln_c_bwd_scratch_bytes(int groups, int channels, int length) {
  if (groups <= 0 || channels <= 0 || length <= 0) return 0;
  return sizeof(float) * 4 * (size_t)groups * channels * ((length + GCB_CHUNK - 1) / GCB_CHUNK);
}

extern "C" int srf_gln_c_bwd(const float* gout, const float* gout2, const float* x, const srf_norm* norm, const float* slopes,
                             int groups, int channels, int length, float* gx, int accumulate_gx, float* dgamma, float* dbeta,
                             float* dslope, void* scratch, void* stream) {
  SRF_CHECK_ARG(gout && x && gx && norm && scratch, "srf_gln_c_bwd: null pointer (gout, x, gx, norm and scratch are required)");
  SRF_CHECK_ARG(groups > 0 && channels > 0 && length > 0, "srf_gln_c_bwd: bad sizes");
  SRF_CHECK_ARG(norm->sums && norm->gamma && norm->beta, "srf_gln_c_bwd: the norm needs statistics, gamma and beta");
  SRF_CHECK_ALIGNED16("srf_gln_c_bwd", {"norm.sums", norm->sums}, {"scratch", scratch});
  SRF_CHECK_ARG(ot_float_aligned({gout, gout2, x, gx, slopes, dgamma, dbeta, dslope, norm->gamma, norm->beta}),
                "srf_gln_c_bwd: gout, gout2, x, gx, slopes and the parameter gradients must be float-aligned");
  const int chunks = (length + GCB_CHUNK - 1) / GCB_CHUNK;
  const long blocks = (long)groups * channels * chunks;
  SRF_CHECK_ARG(blocks < (1L << 31), "srf_gln_c_bwd: tensor too large");
  GlnCBwdArgs a;
  a.gout = gout, a.gout2 = gout2, a.x = x;
  a.nrm = SrfNormDev{norm->sums, norm->gamma, norm->beta, nullptr};
  a.slopes = slopes;
  a.gx = gx;
  a.dgamma = dgamma, a.dbeta = dbeta, a.dslope = slopes ? dslope : nullptr;
  a.part = (float*)scratch;
  a.inv_count = 1.0 / ((double)channels * (double)length);
  a.groups = groups, a.C = channels, a.L = length, a.chunks = chunks, a.accumulate = accumulate_gx;
  const bool vec = srf_kernel_mode() != 1 && ((((size_t)x ^ (size_t)gout) | ((size_t)x ^ (size_t)gx)) & 15) == 0 &&
                   (!gout2 || (((size_t)x ^ (size_t)gout2) & 15) == 0);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks), blk(256);
  if (vec)
    hipLaunchKernelGGL(srf_gln_c_bwd_reduce_kernel<true>, grid, blk, 0, st, a);
  else
    hipLaunchKernelGGL(srf_gln_c_bwd_reduce_kernel<false>, grid, blk, 0, st, a);
  SRF_CHECK_LAUNCH(vec ? "gln_c_bwd_reduce" : "gln_c_bwd_reduce_scalar", st);
  if (vec)
    hipLaunchKernelGGL(srf_gln_c_bwd_apply_kernel<true>, grid, blk, 0, st, a);
  else
    hipLaunchKernelGGL(srf_gln_c_bwd_apply_kernel<false>, grid, blk, 0, st, a);
  SRF_CHECK_LAUNCH(vec ? "gln_c_bwd_apply" : "gln_c_bwd_apply_scalar", st);
  return SRF_OK;
}

extern "C" int srf_softmax_mask_bwd(const float* z, const float* enc, const float* gv, float* gz, float* genc, int accumulate_genc,
                                    int Bt, int S, int N, int L, void* stream) {
  SRF_CHECK_ARG(z && enc && gv && gz && genc, "srf_softmax_mask_bwd: null pointer");
  SRF_CHECK_ARG(Bt > 0 && N > 0 && L > 0, "srf_softmax_mask_bwd: bad sizes");
  SRF_CHECK_ARG(S >= 1 && S <= SRF_SOFTMAX_MASK_MAX_SOURCES, "srf_softmax_mask_bwd: num_sources = %d unsupported (1..%d)", S,
                SRF_SOFTMAX_MASK_MAX_SOURCES);
  SRF_CHECK_ARG(ot_float_aligned({z, enc, gv, gz, genc}), "srf_softmax_mask_bwd: z, enc, gv, gz and genc must be float-aligned");
  SRF_CHECK_ARG((const void*)gz != (const void*)z && (const void*)genc != (const void*)enc && (const void*)genc != (const void*)gz &&
                    (const void*)genc != (const void*)gv,
                "srf_softmax_mask_bwd: gz must not be z; genc must be none of enc, gv, gz");
  const size_t per = (size_t)N * L, total = per * Bt, blocks = (total + 255) / 256;
  const dim3 grid((unsigned)(blocks < (1u << 20) ? blocks : (1u << 20)));
  if (S <= 4)
    hipLaunchKernelGGL(srf_softmax_mask_bwd_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, z, enc, gv, gz, genc, accumulate_genc, S,
                       N, L, per, total);
  else
    hipLaunchKernelGGL((srf_softmax_mask_bwd_kernel<SRF_SOFTMAX_MASK_MAX_SOURCES>), grid, dim3(256), 0, (hipStream_t)stream, z, enc, gv,
                       gz, genc, accumulate_genc, S, N, L, per, total);
  SRF_CHECK_LAUNCH("softmax_mask_bwd", stream);
  return SRF_OK;
}

extern "C" int srf_mask_weight_fold(const float* dtz, const float* drow, float* dmw, float* dmb, int N, int S, void* stream) {
  SRF_CHECK_ARG(dtz && drow && dmw && dmb, "srf_mask_weight_fold: null pointer");
  SRF_CHECK_ARG(N >= 2 && N % 2 == 0, "srf_mask_weight_fold: enc_num_basis = %d must be even and positive", N);
  SRF_CHECK_ARG(S >= 1 && (long)S * N < (1L << 24), "srf_mask_weight_fold: num_sources = %d out of range", S);
  SRF_CHECK_ARG(ot_float_aligned({dtz, drow, dmw, dmb}), "srf_mask_weight_fold: dtz, drow, dmw and dmb must be float-aligned");
  hipLaunchKernelGGL(srf_mask_weight_fold_kernel, dim3((unsigned)(S * (N + 1))), dim3(256), 0, (hipStream_t)stream, dtz, drow, dmw, dmb, N);
  SRF_CHECK_LAUNCH("mask_weight_fold", stream);
  return SRF_OK;
}

extern "C" int srf_decoder_weight_contract(const float* dwexp, float* dw, int N, int S, int K, void* stream) {
  SRF_CHECK_ARG(dwexp && dw, "srf_decoder_weight_contract: null pointer");
  SRF_CHECK_ARG(N > 0 && S > 0 && K > 0 && (long)S * N < (1L << 24) && (long)S * K < (1L << 16), "srf_decoder_weight_contract: bad sizes");
  SRF_CHECK_ARG(ot_float_aligned({dwexp, dw}), "srf_decoder_weight_contract: dwexp and dw must be float-aligned");
  const size_t total = (size_t)S * N * K, blocks = (total + 255) / 256;
  hipLaunchKernelGGL(srf_decoder_weight_contract_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0,
                     (hipStream_t)stream, dwexp, dw, N, S, K);
  SRF_CHECK_LAUNCH("decoder_weight_contract", stream);
  return SRF_OK;
}

extern "C" size_t srf_decoder_bias_grad_scratch_floats(int S) { return S > 0 ? (size_t)S * DBG_PARTS : 0; }

extern "C" int srf_decoder_bias_grad(const float* grad_out, float* dbias, int Bt, int S, int T, float* scratch, void* stream) {
  SRF_CHECK_ARG(grad_out && dbias && scratch, "srf_decoder_bias_grad: null pointer");
  SRF_CHECK_ARG(Bt > 0 && T > 0 && S > 0 && S <= 65535, "srf_decoder_bias_grad: bad sizes");
  SRF_CHECK_ARG(ot_float_aligned({grad_out, dbias, scratch}), "srf_decoder_bias_grad: grad_out, dbias and scratch must be float-aligned");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(srf_decoder_bias_part_kernel, dim3(DBG_PARTS, S), dim3(256), 0, st, grad_out, scratch, S, T, (size_t)Bt * T);
  SRF_CHECK_LAUNCH("decoder_bias_part", st);
  hipLaunchKernelGGL(srf_decoder_bias_fold_kernel, dim3(S), dim3(64), 0, st, scratch, dbias);
  SRF_CHECK_LAUNCH("decoder_bias_fold", st);
  return SRF_OK;
}

extern "C" int srf_relu_gate(float* g, const float* s, long n, void* stream) {
  SRF_CHECK_ARG(g && s, "srf_relu_gate: null pointer");
  SRF_CHECK_ARG(n > 0, "srf_relu_gate: bad size");
  SRF_CHECK_ARG(ot_float_aligned({g, s}), "srf_relu_gate: g and s must be float-aligned");
  SRF_CHECK_ARG((const void*)g != (const void*)s, "srf_relu_gate: g must not be s");
  const bool vec = srf_kernel_mode() != 1 && (((size_t)g ^ (size_t)s) & 15) == 0;
  const long per = vec ? 1024 : 256, blocks = (n + per - 1) / per;
  const dim3 grid((unsigned)(blocks < (1L << 20) ? blocks : (1L << 20)));
  if (vec)
    hipLaunchKernelGGL(srf_relu_gate_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, g, s, n);
  else
    hipLaunchKernelGGL(srf_relu_gate_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, g, s, n);
  SRF_CHECK_LAUNCH("relu_gate", stream);
  return SRF_OK;
}

// ---------------------------------------------------------------------------------------------
// the training walk
// ---------------------------------------------------------------------------------------------
namespace {

struct OTrainLayout {
  size_t stats, enc, x0, x_stride, blk0, blk_stride, y1, lv[SRF_MAX_DEPTH], m, g, gx, xr, z, total;
};

OTrainLayout otrain_layout(const srf_plan* p) {
  OTrainLayout t{};
  const srf_config& c = p->cfg;
  const size_t F = sizeof(float), L = p->L, Bt = p->Bt;
  const int D = c.upsampling_depth, U = c.num_blocks, N = c.enc_num_basis, B = p->nB, C = p->nC, S = c.num_sources;
  SrfCarve all, blk;      // (blk: one block's slices, offsets relative to the block's start)
  t.stats = all.take(p->stats_bytes);
  t.enc = all.take(F * Bt * N * L);
  t.x_stride = srf_align_up(F * Bt * B * L, 256);
  t.x0 = all.take(t.x_stride * (U + 1));
  t.y1 = blk.take(F * Bt * C * L);
  for (int k = 0; k < D; ++k) t.lv[k] = blk.take(F * Bt * C * (L >> k));
  t.m = blk.take(F * Bt * C * L);
  t.g = blk.take(F * Bt * B * L);
  t.gx = blk.take(F * Bt * B * L);
  t.blk_stride = blk.off;
  t.blk0 = all.take(blk.off * U);
  t.xr = orig_has_reshape(p) ? all.take(F * Bt * N * L) : 0;
  t.z = all.take(F * Bt * S * N * L);
  t.total = all.off;
  return t;
}

struct OScratchLayout {
  size_t dec, vbuf, gv, genc, gxm, gb[4], act, gc1, gc2, gd, gu[SRF_MAX_DEPTH], gn[SRF_MAX_DEPTH], frames, wt, zeros, tz, wdec, wdpad, dtz,
      dwexp, wg, gln, glnc, dwb, bias, padg, padx, pk3, pkT, total;
  size_t zero_floats;
  int dec_rows, L4;
};

OScratchLayout oscratch_layout(const srf_plan* p) {
  OScratchLayout s{};
  const srf_config& c = p->cfg;
  const size_t F = sizeof(float), L = p->L, Bt = p->Bt;
  const int D = c.upsampling_depth, U = c.num_blocks, K = c.enc_kernel_size, N = c.enc_num_basis, B = p->nB, C = p->nC,
            S = c.num_sources, SN = S * N;
  SrfCarve all{0, /*min_one=*/true};
  s.dec_rows = (S * K + 63) / 64 * 64;
  s.L4 = (p->L + 3) / 4 * 4;      // the weight-gradient GEMM takes L % 4 == 0 only: else its operands are copied to this pitch
  s.dec = all.take(F * srf_decoder_scratch_floats(p->Bt, SN, S, K, p->L));
  s.vbuf = all.take(F * Bt * SN * L);
  s.gv = all.take(F * Bt * SN * L);
  s.genc = all.take(F * Bt * N * L);
  s.gxm = all.take(F * Bt * N * L);
  for (int i = 0; i < 4; ++i) s.gb[i] = all.take(F * Bt * B * L);
  s.act = all.take(F * Bt * C * L);
  s.gc1 = all.take(F * Bt * C * L);
  s.gc2 = all.take(F * Bt * C * L);
  s.gd = all.take(F * Bt * C * L);
  for (int k = 0; k + 1 < D; ++k) s.gu[k] = all.take(F * Bt * C * (L >> k));
  for (int k = 1; k < D; ++k) s.gn[k] = all.take(F * Bt * C * (L >> k));
  s.frames = all.take(F * Bt * L * std::max((size_t)s.dec_rows, (size_t)K));
  s.wt = all.take(F * std::max({(size_t)B * N, (size_t)B * C, (size_t)SN * N}));
  s.zero_floats = std::max({C, SN, N, B});
  s.zeros = all.take(F * s.zero_floats);
  s.tz = all.take(F * orig_tz_floats(S, N));
  s.wdec = all.take(F * (size_t)SN * S * K);
  s.wdpad = all.take(F * (size_t)SN * s.dec_rows);
  s.dtz = all.take(F * orig_tz_floats(S, N));
  s.dwexp = all.take(F * (size_t)SN * S * K);
  size_t wg = 0;
  auto wgmax = [&](int cout, int cin) { wg = std::max(wg, srf_pw_wgrad_scratch_bytes(p->Bt, cout, cin, s.L4)); };
  wgmax(SN, s.dec_rows);
  wgmax(SN, N);
  wgmax(N, B);
  wgmax(B, C);
  wgmax(C, B);
  wgmax(B, N);
  wgmax(N, K);
  s.wg = all.take(wg);
  s.gln = all.take(srf_gln_bwd_scratch_bytes(p->Bt, C > N ? C : N));
  s.glnc = all.take(srf_gln_c_bwd_scratch_bytes(p->Bt, C > B ? C : B, p->L));
  s.dwb = all.take(srf_dwconv5_bwd_scratch_bytes(p->Bt, C));
  s.bias = all.take(F * srf_decoder_bias_grad_scratch_floats(S));
  if (s.L4 != p->L) {
    const size_t rows = std::max({C, SN, N, B, s.dec_rows, K});
    s.padg = all.take(F * Bt * rows * s.L4);
    s.padx = all.take(F * Bt * rows * s.L4);
  }
  // the images of every 1x1 weight [cout, cin]: l1, the Toeplitz weight, reshape_before_masks, U x (proj_1x1, conv_1x1_exp) -- the
  // forward's exact-class images, and the backward's images of the transposes
  auto images = [&](size_t (*bytes)(int, int), bool transposed) {
    auto one = [&](int cout, int cin) { return srf_align_up(transposed ? bytes(cin, cout) : bytes(cout, cin), 256); };
    return one(B, N) + one(SN, N) + one(N, B) + (size_t)U * (one(C, B) + one(B, C));
  };
  s.pk3 = all.take(images(srf_packed3_pw_weight_bytes, false));
  s.pkT = all.take(images(srf_packed_pw_weight_bytes, true));
  s.total = all.off;
  return s;
}

bool original_plan(const srf_plan* p, const char* who) {
  if (p && p->cfg.variant == SRF_VARIANT_ORIGINAL) return true;
  srf_set_error("%s: %s", who, p ? "original plans only (srf_original_plan_create; the other models train through srf_forward_train / "
                                   "srf_backward or srf_causal_forward_train / srf_causal_backward)"
                                 : "null plan");
  return false;
}

// where the training forward keeps the walk's tensors: what the backward reads in `saved`, every block's own slices and one
// block-stream buffer per block boundary; the rest (a / e, the masked tensor, the decoder's scratch, the two weight forms) in `scratch`
SrfOrigAddrs otrain_addrs(const srf_plan* p, const OTrainLayout& t, const OScratchLayout& s, char* sv, char* sc) {
  auto fp = [&](size_t o) { return (float*)(sc + o); };
  SrfOrigAddrs a{};
  a.stats = (double*)(sv + t.stats);
  a.enc = (float*)(sv + t.enc);
  a.x = sv + t.x0, a.x_stride = t.x_stride;
  a.blk = sv + t.blk0, a.blk_stride = t.blk_stride;
  a.o_y1 = t.y1, a.o_m = t.m, a.o_g = t.g, a.o_gx = t.gx;
  for (int k = 0; k < p->cfg.upsampling_depth; ++k) a.o_lv[k] = t.lv[k];
  a.act = fp(s.act), a.xr = (float*)(sv + t.xr), a.z = (float*)(sv + t.z), a.masked = fp(s.vbuf);
  a.dec = fp(s.dec), a.tz = fp(s.tz), a.wdec = fp(s.wdec);
  return a;
}

}  // namespace

extern "C" size_t srf_original_train_saved_bytes(const srf_plan* p) {
  return original_plan(p, "srf_original_train_saved_bytes") ? otrain_layout(p).total : 0;
}
extern "C" size_t srf_original_train_scratch_bytes(const srf_plan* p) {
  return original_plan(p, "srf_original_train_scratch_bytes") ? oscratch_layout(p).total : 0;
}

extern "C" int srf_original_forward_train(const srf_plan* p, const float* const* P, int num_params, const float* wav, float* out,
                                          void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes, void* stream) {
  if (!original_plan(p, "srf_original_forward_train")) return SRF_EINVAL;
  int rc = srf_train_entry_check("srf_original_forward_train", p, P, nullptr, num_params, 0, {wav, out},
                                 {saved, saved_bytes, otrain_layout(p).total, scratch, scratch_bytes, oscratch_layout(p).total});
  if (rc) return rc;
  // the exact-fp32 class for the 1x1 convolutions where srf_train_fwd_exact() says so -- and of
  // its two forms the THREE-bf16-part one (24 mantissa bits), not the two-fp16-part default (22): this model puts three per-channel
  // PReLUs behind GroupNorms into every block, and every pre-activation that the forward's rounding moves across 0 flips a slope in
  // the backward.  Measured at the recipe's channel counts (256 / 512 / N 512, U 2, D 3, 512 frames, 64 examples) against fp64
  // autograd: two parts leave l1.weight 5.8e-3 of its largest entry off (torch's own fp32 autograd: 4.5e-4) and five tensors over
  // the 2e-3 bar; three parts 3.0e-4 and none.
  const SrfKernelModeScope exact_class(srf_train_fwd_exact(), 2);
  const SrfThreePartsScope three_parts;
  if (srf_profiling()) srf_prof_mark("(gap)", (hipStream_t)stream);
  // (the decoder's frame GEMM stays in the exact class too, unlike srf_forward_train's: its rounding is the output's, and the
  // runner's loss and its gradient go with 1 / <estimate, target>)
  // the walk of the inference forward with every block's tensors kept, the pyramid level by level (the backward reads every raw
  // level) and the exact-class images of the 1x1 weights the 256 x 128 GEMM takes, as srf_forward_train packs them
  const OScratchLayout s = oscratch_layout(p);
  const int U = p->cfg.num_blocks, N = p->cfg.enc_num_basis, SN = p->cfg.num_sources * N, B = p->nB, C = p->nC;
  std::vector<const void*> image(p->n_params, nullptr);      // parameter index -> its packed image (NULL: none)
  auto pack = [&](const float* tz) {
    SrfPackQueue pk{(char*)scratch + s.pk3};
    auto add = [&](int param, const float* w, int cout, int cin) {
      image[param] = pk.add3(w, cout, cin);
    };
    add(SRF_PO_L1, P[SRF_PO_L1], B, N);
    add(orig_p_mask(p), tz, SN, N);
    if (orig_has_reshape(p)) add(orig_p_reshape(p), P[orig_p_reshape(p)], N, B);
    for (int i = 0; i < U; ++i) {
      add(orig_p_proj(p, i), P[orig_p_proj(p, i)], C, B);
      add(orig_p_exp(p, i), P[orig_p_exp(p, i)], B, C);
    }
    return pk.pack3(stream);
  };
  auto conv = [&](const float* x, const float* w, int param, const float* bias, float* y, int Cin, int Cout, const srf_norm* in_norm,
                  double* out_sums) {
    return srf_pw_conv_packed3(x, w, image[param], bias, y, p->Bt, Cin, Cout, p->L, in_norm, nullptr, out_sums, stream);
  };
  return orig_walk(p, P, wav, out, otrain_addrs(p, otrain_layout(p), s, (char*)saved, (char*)scratch), pack, conv, /*fused=*/false,
                   nullptr, nullptr, 0, stream);
}

extern "C" int srf_original_backward(const srf_plan* p, const float* const* P, float* const* G, int num_params, const float* wav,
                                     const float* grad_out, const void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes,
                                     void* stream) {
  if (!original_plan(p, "srf_original_backward")) return SRF_EINVAL;
  const OTrainLayout t = otrain_layout(p);
  const OScratchLayout s = oscratch_layout(p);
  // (ln_mask_in.{weight, bias}, the last two, receive no gradient: their entries may be NULL)
  int rc = srf_train_entry_check("srf_original_backward", p, P, G, num_params, 2, {G, wav, grad_out},
                                 {saved, saved_bytes, t.total, scratch, scratch_bytes, s.total});
  if (rc) return rc;
  const srf_config& c = p->cfg;
  const int D = c.upsampling_depth, U = c.num_blocks, N = c.enc_num_basis, K = c.enc_kernel_size, h = K / 2, S = c.num_sources,
            SN = S * N;
  const int Bt = p->Bt, L = p->L, B = p->nB, C = p->nC, L4 = s.L4;
  const char* sv = (const char*)saved;
  char* sc = (char*)scratch;
  hipStream_t st = (hipStream_t)stream;
  auto xbuf = [&](int i) { return (const float*)(sv + t.x0 + t.x_stride * i); };
  auto fp = [&](size_t o) { return (float*)(sc + o); };
  double* stats = (double*)const_cast<char*>(sv + t.stats);      // (read only: srf_norm carries a plain pointer)
  const float* enc = (const float*)(sv + t.enc);
  const float* z = (const float*)(sv + t.z);
  float* zeros = fp(s.zeros);
  float* wt = fp(s.wt);
  void* wg = sc + s.wg;
  const SrfOrigFront f = orig_front(P);
  const SrfOrigFrontT<float> gf = orig_front(G);
  const SrfOrigTail tl = orig_tail(p, P);
  const SrfOrigTailT<float> gtl = orig_tail(p, G);
  if (srf_profiling()) srf_prof_mark("(gap)", st);
  SRF_CHECK_HIP(hipMemsetAsync(zeros, 0, sizeof(float) * s.zero_floats, st));
  // the weight-gradient GEMMs of this call fold their partial sums in a fixed order
  const SrfWgradOrderedScope ordered_for_this_call;
  // ---- the two weights in their GEMM forms, again (scratch is not kept between the calls)
  float* tz = fp(s.tz);
  float* wdec = fp(s.wdec);
  rc = srf_original_weight_forms(p, P, tz, wdec, stream);
  if (rc) return rc;
  // transposed weights of the data-gradient GEMMs, pre-split for the 256 x 128 kernel where it takes the shape
  SrfPackQueue pk{sc + s.pkT};
  auto packT = [&](const float* wf, int cout_d, int cin_d) {   // wf: forward weight [cin_d][cout_d]
    return pk.add(wf, srf_kernel_mode() == 0 ? srf_packed_pw_weight_bytes(cout_d, cin_d) : 0, cout_d, cin_d);
  };
  const void* pkT_mask = packT(tz, N, SN);
  const void* pkT_rs = orig_has_reshape(p) ? packT(tl.rs_w, B, N) : nullptr;
  const void* pkT_l1 = packT(f.l1_w, N, B);
  std::vector<const void*> pkT_proj(U, nullptr), pkT_exp(U, nullptr);
  for (int i = 0; i < U; ++i) {
    const SrfOrigBlock b = orig_block(p, P, i);
    pkT_proj[i] = packT(b.proj_w, B, C);
    pkT_exp[i] = packT(b.exp_w, C, B);
  }
  rc = pk.packT(st);
  if (rc) return rc;
  // g_x = W^T g (+ skip): cin_d -> cout_d, w the forward weight [cin_d][cout_d]
  // Where no packed image serves the launch the GEMM would fall to the kernels that split fp32 into two bf16 parts on the fly (16
  // mantissa bits per operand); those launches run in the exact-fp32 class instead (kernel mode 2 for this thread, as the
  // training forward does).  Measured on the trajectory fixture: with the on-the-fly split a gradient entry of 9.7e-7 (2.8e-6 of
  // its tensor's largest) came out as 1.74e-6, in the exact class as 1.04e-6 -- after the clip that entry sits inside Adam's eps,
  // where the step follows the gradient's size, and the first moved one tensor's update by 4.3e-3 of its norm, the second by 6e-4.
  auto data_grad = [&](const float* g, const float* w, const void* pkT, float* y, int cin_d, int cout_d, const float* skip) -> int {
    const SrfKernelModeScope exact(!srf_pw_packed_only(pkT, g, Bt, cin_d, cout_d, L) && srf_kernel_mode() == 0, 2);
    return srf_pw_data_grad(g, w, pkT, wt, zeros, y, Bt, cin_d, cout_d, L, skip, st);
  };
  // dW (+ db) of y = W x + b.  The GEMM takes L % 4 == 0; any other L (D = 1 models only) goes through copies at a pitch of L4
  // floats with zeros behind every row.
  auto wgrad = [&](const float* g, const float* x, const srf_norm* in_norm, int Cin, int Cout, float* dw, int dw_cols, float* dbias,
                   int accumulate) -> int {
    if (L4 == L) return srf_pw_wgrad_cols(g, x, in_norm, Bt, Cin, Cout, L, dw, dw_cols, dbias, accumulate, wg, stream);
    if (in_norm) {
      srf_set_error("srf_original_backward: internal: a prologue on the padded weight-gradient path");
      return SRF_EINVAL;
    }
    float *pg = fp(s.padg), *px = fp(s.padx);
    const size_t F = sizeof(float);
    SRF_CHECK_HIP(hipMemsetAsync(pg, 0, F * Bt * Cout * L4, st));
    SRF_CHECK_HIP(hipMemsetAsync(px, 0, F * Bt * Cin * L4, st));
    SRF_CHECK_HIP(hipMemcpy2DAsync(pg, F * L4, g, F * L, F * L, (size_t)Bt * Cout, hipMemcpyDeviceToDevice, st));
    SRF_CHECK_HIP(hipMemcpy2DAsync(px, F * L4, x, F * L, F * L, (size_t)Bt * Cin, hipMemcpyDeviceToDevice, st));
    return srf_pw_wgrad_cols(pg, px, nullptr, Bt, Cin, Cout, L4, dw, dw_cols, dbias, accumulate, wg, stream);
  };
  auto gln_c_bwd = [&](const float* gout, const float* x, double* sums, const float* gamma, const float* beta, const float* slopes,
                       int Cn, float* gx, float* dgamma, float* dbeta, float* dslope) -> int {
    const srf_norm n{sums, gamma, beta, nullptr};
    return srf_gln_c_bwd(gout, nullptr, x, &n, slopes, Bt, Cn, L, gx, 0, dgamma, dbeta, dslope, sc + s.glnc, stream);
  };

  // ---- 1. decoder: out = overlap_add(Wexp^T v) + bias, v = softmax(z) * s
  rc = srf_decoder_bias_grad(grad_out, gtl.dec_b, Bt, S, p->T, fp(s.bias), stream);
  if (rc) return rc;
  float* frames = fp(s.frames);
  rc = srf_frames_gather(grad_out, frames, Bt, S, p->T, K, h, h, L, s.dec_rows, stream);
  if (rc) return rc;
  float* wdpad = fp(s.wdpad);
  SRF_CHECK_HIP(hipMemsetAsync(wdpad, 0, sizeof(float) * (size_t)SN * s.dec_rows, st));
  SRF_CHECK_HIP(hipMemcpy2DAsync(wdpad, sizeof(float) * s.dec_rows, wdec, sizeof(float) * S * K, sizeof(float) * S * K, SN,
                                 hipMemcpyDeviceToDevice, st));
  float* gv = fp(s.gv);
  {
    // (the backward's FIRST linear map: its rounding reaches every gradient)
    const SrfKernelModeScope exact(srf_kernel_mode() == 0, 2);
    rc = srf_pw_conv(frames, wdpad, zeros, gv, Bt, s.dec_rows, SN, L, nullptr, nullptr, nullptr, 0, nullptr, 0, stream);
  }
  if (rc) return rc;
  float* v = fp(s.vbuf);
  rc = srf_softmax_mask(z, enc, v, Bt, S, N, L, stream);      // v, re-computed
  if (rc) return rc;
  float* dwexp = fp(s.dwexp);
  rc = wgrad(v, frames, nullptr, s.dec_rows, SN, dwexp, S * K, nullptr, 0);
  if (rc) return rc;
  rc = srf_decoder_weight_contract(dwexp, gtl.dec_w, N, S, K, stream);
  if (rc) return rc;
  // ---- 2. softmax over the sources times s: gv becomes g_z, genc the mask path's share of g_s
  float* genc = fp(s.genc);
  rc = srf_softmax_mask_bwd(z, enc, gv, gv, genc, 0, Bt, S, N, L, stream);
  if (rc) return rc;
  // ---- 3. mask GEMM z = Tz xm + bias rows
  const float* xm = orig_has_reshape(p) ? (const float*)(sv + t.xr) : xbuf(U);
  float* dtz = fp(s.dtz);
  float* drow = dtz + orig_tz_bias_at(S, N);
  rc = wgrad(gv, xm, nullptr, N, SN, dtz, N, drow, 0);
  if (rc) return rc;
  rc = srf_mask_weight_fold(dtz, drow, gtl.m_w, gtl.m_b, N, S, stream);
  if (rc) return rc;
  float *gx = fp(s.gb[0]), *gx_other = fp(s.gb[3]);
  float *g_gx = fp(s.gb[1]), *g_g = fp(s.gb[2]);
  // ---- 4. reshape_before_masks
  if (orig_has_reshape(p)) {
    float* gxm = fp(s.gxm);
    rc = data_grad(gv, tz, pkT_mask, gxm, SN, N, nullptr);
    if (rc) return rc;
    rc = wgrad(gxm, xbuf(U), nullptr, B, N, gtl.rs_w, B, gtl.rs_b, 1);
    if (rc) return rc;
    rc = data_grad(gxm, tl.rs_w, pkT_rs, gx, N, B, nullptr);
    if (rc) return rc;
  } else {
    rc = data_grad(gv, tz, pkT_mask, gx, SN, N, nullptr);
    if (rc) return rc;
  }
  // ---- 5. blocks, last to first: gx = g_x(i + 1) -> g_x(i)
  float *act = fp(s.act), *gc1 = fp(s.gc1), *gc2 = fp(s.gc2), *gd = fp(s.gd);
  for (int i = U - 1; i >= 0; --i) {
    const SrfOrigBlock b = orig_block(p, P, i);
    const SrfOrigBlockT<float> g = orig_block(p, G, i);
    const SrfOrigSlots sl = orig_slots(p, stats, i);
    const char* blk = sv + t.blk0 + t.blk_stride * i;
    const float *y1 = (const float*)(blk + t.y1), *m = (const float*)(blk + t.m), *gs = (const float*)(blk + t.g),
                *gxs = (const float*)(blk + t.gx);
    // module_act on g + x: g_gx is the skip into the block input's gradient and conv_1x1_exp.norm's incoming gradient
    rc = gln_c_bwd(gx, gxs, sl.act, b.act_g, b.act_be, b.act_slope, B, g_gx, g.act_g, g.act_be, g.act_slope);
    if (rc) return rc;
    rc = gln_c_bwd(g_gx, gs, sl.exp, b.exp_g, b.exp_be, nullptr, B, g_g, g.exp_g, g.exp_be, nullptr);
    if (rc) return rc;
    // conv_1x1_exp over e = PReLU_c(final_norm(m)), re-computed
    const srf_norm fn{sl.merged, b.fin_g, b.fin_be, nullptr};
    rc = srf_gln_apply_c(m, &fn, b.fin_slope, nullptr, act, nullptr, Bt, C, L, stream);
    if (rc) return rc;
    rc = wgrad(g_g, act, nullptr, C, B, g.exp_w, C, g.exp_b, 1);
    if (rc) return rc;
    rc = data_grad(g_g, b.exp_w, pkT_exp[i], gc1, B, C, nullptr);      // gc1 = g_e
    if (rc) return rc;
    rc = gln_c_bwd(gc1, m, sl.merged, b.fin_g, b.fin_be, b.fin_slope, C, gc2, g.fin_g, g.fin_be, g.fin_slope);      // gc2 = g_m
    if (rc) return rc;
    // the pyramid: g_m is the gradient w.r.t. the normalised level 0, its pair sums that of the levels below
    float* gn[SRF_MAX_DEPTH] = {};
    gn[0] = gc2;
    for (int k = 1; k < D; ++k) gn[k] = fp(s.gn[k]);
    rc = srf_merge_bwd(gn[0], gn, D, (long)Bt * C, L, stream);
    if (rc) return rc;
    // a = PReLU_c(proj_1x1.norm(y1)), re-computed (e is dead)
    const srf_norm pn{sl.proj, b.proj_g, b.proj_be, nullptr};
    rc = srf_gln_apply_c(y1, &pn, b.proj_slope, nullptr, act, nullptr, Bt, C, L, stream);
    if (rc) return rc;
    for (int k = D - 1; k >= 0; --k) {
      const float* dk = (const float*)(blk + t.lv[k]);
      const srf_norm nk{sl.level[k], b.lv_g[k], b.lv_be[k], nullptr};
      // gradient w.r.t. the normalised level k: the merge's share + what level k + 1's conv sent down
      rc = srf_gln_bwd(gn[k], k < D - 1 ? fp(s.gu[k]) : nullptr, dk, &nk, Bt, C, L >> k, gd, 0, g.lv_g[k], g.lv_be[k], nullptr, sc + s.gln,
                       stream);
      if (rc) return rc;
      const srf_norm in{k ? sl.level[k - 1] : nullptr, k ? b.lv_g[k - 1] : nullptr, k ? b.lv_be[k - 1] : nullptr, nullptr};
      rc = srf_dwconv5_bwd(gd, k ? (const float*)(blk + t.lv[k - 1]) : act, k ? &in : nullptr, b.lv_w[k], Bt, C, k ? L >> (k - 1) : L,
                           k ? 2 : 1, k ? fp(s.gu[k - 1]) : gc1, g.lv_w[k], g.lv_b[k], sc + s.dwb, stream);      // level 0: gc1 = g_a
      if (rc) return rc;
    }
    rc = gln_c_bwd(gc1, y1, sl.proj, b.proj_g, b.proj_be, b.proj_slope, C, gc2, g.proj_g, g.proj_be, g.proj_slope);      // gc2 = g_y1
    if (rc) return rc;
    rc = wgrad(gc2, xbuf(i), nullptr, B, C, g.proj_w, B, g.proj_b, 1);
    if (rc) return rc;
    rc = data_grad(gc2, b.proj_w, pkT_proj[i], gx_other, C, B, g_gx);      // + the skip
    if (rc) return rc;
    float* tmp = gx;
    gx = gx_other;
    gx_other = tmp;
  }
  // ---- 6. front: x_0 = l1(ln(s)), s = relu(encoder(wav))
  const srf_norm ln{stats, f.ln_g, f.ln_b, nullptr};
  float* gln = fp(s.vbuf);      // (v is dead)
  if (L4 == L) {
    rc = wgrad(gx, enc, &ln, N, B, gf.l1_w, N, gf.l1_b, 1);
  } else {      // the padded path has no prologue: ln(s) materialised first
    rc = srf_gln_apply_c(enc, &ln, nullptr, nullptr, gln, nullptr, Bt, N, L, stream);
    if (rc) return rc;
    rc = wgrad(gx, gln, nullptr, N, B, gf.l1_w, N, gf.l1_b, 1);
  }
  if (rc) return rc;
  rc = data_grad(gx, f.l1_w, pkT_l1, gln, B, N, nullptr);
  if (rc) return rc;
  rc = srf_gln_bwd(gln, nullptr, enc, &ln, Bt, N, L, genc, 1, gf.ln_g, gf.ln_b, nullptr, sc + s.gln, stream);
  if (rc) return rc;
  rc = srf_relu_gate(genc, enc, (long)Bt * N * L, stream);
  if (rc) return rc;
  rc = srf_frames_gather(wav, frames, Bt, 1, p->T, K, h, h, L, K, stream);
  if (rc) return rc;
  return wgrad(genc, frames, nullptr, K, N, gf.enc_w, K, gf.enc_b, 1);
}
