// Softmax attention and the small glue kernels of the attentive models' transformer layers
// (attentive_sudormrf_v2.py: MHAttentionLayer.forward, TransformerLayer.forward; attentive_sudormrf_v3.py:
// ConditionalTransformerLayer.forward, AttentiveUConvBlock.forward).
//
//   srf_mha_attention   o[b, h d + j, lq] = sum_lk softmax_lk(scale * sum_j q[b, h d + j, lq] k[b, h d + j, lk]) v[b, h d + j, lk]
//   srf_mha_attention_lse   the same, + lse[b, h, lq] = log sum_lk exp(score): what srf_mha_attention_bwd recomputes P from
//   srf_posenc_apply    x[b, c, l] = GlobLN(a)[b, c, l] + pe[l, c]                      (PositionalEncoding on the transposed tensor)
//   srf_posenc_apply_dropout / srf_posenc_dropout_bwd / srf_dropout_mask   the same under a Philox keep mask, and its gradient
//   srf_gln_apply2_add  z = norm_f(f) + norm_y(y), {sum, sumsq} of z accumulated       (out_norm's input: ffn(y) + y)
//   srf_gln_apply_stats y = norm(x), {sum, sumsq} of y accumulated                     (v3: O_proj's residual; final_norm's input)
//
// Every tensor is [batch, channel, time] like the rest of the library: q, k, v are the outputs of 1x1 convolutions, channel
// h d + j belongs to head h, and nothing is transposed in memory.
//
// The MFMA form (d % 16 == 0, 16 <= d <= 256): one wavefront per (example, head, 32 queries), key tiles of 32, online softmax.
// Both contractions run on v_mfma_f32_32x32x2_f32 (exact fp32) with the QUERY as the N index of both products:
//     S^T[key, query] = sum_j K[j, key] Q[j, query]        A = K (lane: key = l & 31, j = 2 s + (l >> 5)), B = Q, d / 2 steps
//     O^T[j, query]  += sum_key V[j, key] P^T[key, query]   A = V, B = P^T, 16 steps per 32 output channels
// so that a lane owns ONE query (column l & 31) in S^T, P^T and O^T alike: the running maximum, the running denominator and the
// rescale of the accumulators are per-lane scalars, and the probabilities go from the first product's accumulator registers
// straight into the second product's B operand -- register r of S^T holds key (r & 3) + 8 (r >> 2) + 4 (l >> 5), and step r of
// the second product simply contracts over THAT pair of keys (the order of a contraction is free as long as A agrees: V is
// read from LDS at the same key).  The score matrix never leaves the registers.
//   Q (pre-scaled, as the reference scales it before the product) is staged once in LDS, [d][32 queries]; O^T takes 16
//   accumulator registers per 32 channels;
//   K is read from global memory as the A operand (a half-wavefront reads 32 consecutive keys of one channel);
//   V goes through LDS 32 channels at a time (32 keys x 32 channels, XOR-swizzled rows: the A operand of the second product
//   walks channels across lanes), so that a block holds 32 d + 1024 floats of LDS -- 36 KB at d = 256, four blocks per CU.
// Edges.  Every global load is predicated (keys >= Lk, queries >= Lq, channels >= d read nothing and count as 0) and a dword
// wide: rows are L floats long with L generally odd, so no wider load is aligned.  Keys >= Lk get the score -inf, i.e. the
// weight exp(-inf) = 0 exactly; a key tile always holds at least one real key (kt < Lk), so the new running maximum is finite and
// "m_old - m_new" is never inf - inf (m_old = -inf gives the rescale factor exp(-inf) = 0).  Queries >= Lq compute on zeros and
// store nothing.
//
// The generic form (any other d <= 1024): one wavefront per query, a lane per key for the scores and a lane per output channel
// for the weighted sum (the probabilities travel by v_readlane), plain fp32 FMA.
//
// Host path: the four public entries (plain, lse, and the ragged form of each) check their sizes, set the contiguous strides
// and call srf_mha_forward, which the attentive walks call with strides of their own: checks, tables, one dispatch.
#include "srf_mha.h"

#define SRF_MHA_NEG_INF (-__builtin_inff())

// The forms that also write the per-query log-sum-exp (srf_mha_attention_lse: what the backward recomputes P from) take the
// [Bt, H, Lq] table as a trailing parameter PACK, the idiom of the ragged forms (srf_internal.h): empty in the plain
// instantiations, whose arguments and code stay what they were.
// The ragged forms (srf_mha_attention*_ragged) append two SrfFrames to that pack: example b owns q_len[b] <= Lq queries and
// k_len[b] <= Lk keys.  Lq and Lk stay the ROW STRIDES of every address; every predicate and loop bound uses the example's own
// count (qn, kn below -- the strides themselves in the uniform instantiations).  Nothing at or past a count is read; o and lse
// are written as exact 0.f from qn up to the stride; a block whose whole tile lies at or past qn stores those zeros and returns
// before any load, LDS write or MFMA.  Inside the counts the arithmetic and its order are the uniform kernel's on example b
// alone with Lq = qn, Lk = kn: the tiles start at position 0 of the example either way.  (The pack's readers: srf_mha.h.)
template <int NCH, typename... X>   // 32-channel chunks of the head dimension (d <= 32 NCH): 16 accumulator registers each
__global__ __launch_bounds__(64) void srf_mha_mfma_kernel(MhaArgs a, X... x) {
  constexpr bool LSE = sizeof...(X) & 1, RAGGED = sizeof...(X) >= 2;
  __shared__ float Qs[NCH * 32 * 32];   // [channel][query], pre-scaled
  __shared__ float Vs[32 * 32];         // one 32-channel chunk of the key tile: [channel][key ^ channel]
  const int lane = threadIdx.x, col = lane & 31, half = lane >> 5;
  const int h = blockIdx.y, b = blockIdx.z, d = a.d, Lq = a.Lq, Lk = a.Lk;
  const int qn = srf_mha_qlen(b, Lq, x...), kn = srf_mha_klen(b, Lk, x...);   // the example's own counts (block-uniform)
  const float* qh = a.q + (size_t)b * a.qs + (size_t)h * d * Lq;
  const float* kh = a.k + (size_t)b * a.ks + (size_t)h * d * Lk;
  const float* vh = a.v + (size_t)b * a.vs + (size_t)h * d * Lk;
  float* oh = a.o + (size_t)b * a.os + (size_t)h * d * Lq;
  const int ql = blockIdx.x * 32 + col;
  const bool qok = ql < qn;
  const bool wok = RAGGED ? ql < Lq : qok;   // ragged: the queries from qn up to the stride are written, as zeros
  if constexpr (RAGGED) {
    if ((int)blockIdx.x * 32 >= qn) {   // the whole tile lies past the example's end
      if (wok) {
        for (int j = half; j < d; j += 2) oh[(size_t)j * Lq + ql] = 0.f;
        if (LSE && half == 0) srf_mha_store_lse(((size_t)b * a.H + h) * Lq + ql, 0.f, x...);
      }
      return;
    }
  }

  // (a uniform row pointer + one per-lane offset per operand: 32-bit offsets, checked by the launcher)
  for (int j0 = 0; j0 < NCH * 32; j0 += 2) {
    const int j = j0 + half;
    Qs[j * 32 + col] = (qok && j0 < d) ? qh[(size_t)j * Lq + ql] * a.scale : 0.f;
  }
  srf_f32x16 acc[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
  float m = SRF_MHA_NEG_INF, den = 0.f;
  __syncthreads();

  for (int kt = 0; kt < kn; kt += 32) {
    const int key = kt + col;
    const bool kok = key < kn;
    const float* kp = kh + (size_t)half * Lk + key;   // (dereferenced under kok only)
    const float* vp = vh + (size_t)half * Lk + key;
    // ---- S^T = K^T Q, 16 contraction steps (32 channels) at a time
    srf_f32x16 st;
#pragma unroll
    for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      if (c * 32 < d) {
        float t[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) t[r] = (kok && c * 32 + 2 * r < d) ? kp[(size_t)(c * 32 + 2 * r) * Lk] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r)
          st = __builtin_amdgcn_mfma_f32_32x32x2f32(t[r], Qs[(c * 32 + 2 * r + half) * 32 + col], st, 0, 0, 0);
      }
    }
    // ---- online softmax over this lane's 16 keys and the other half-wavefront's 16
    float tmax = SRF_MHA_NEG_INF;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ki = kt + (r & 3) + 8 * (r >> 2) + 4 * half;
      st[r] = ki < kn ? st[r] : SRF_MHA_NEG_INF;
      tmax = fmaxf(tmax, st[r]);
    }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const float mn = fmaxf(m, tmax);       // finite: key kt itself is inside
    const float alpha = expf(m - mn);      // m = -inf (first tile): 0
    float psum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      st[r] = expf(st[r] - mn);            // masked keys: exp(-inf) = 0
      psum += st[r];
    }
    psum += __shfl_xor(psum, 32, 64);
    den = den * alpha + psum;
    m = mn;
    // ---- O^T = alpha O^T + V P^T per 32-channel chunk, contracting over the key pair that register s of S^T holds
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      if (c * 32 < d) {
        float t[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) t[r] = (kok && c * 32 + 2 * r < d) ? vp[(size_t)(c * 32 + 2 * r) * Lk] : 0.f;
        __syncthreads();   // (the previous chunk's reads of Vs are done)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int j = 2 * r + half;
          Vs[j * 32 + (col ^ j)] = t[r];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[c][r] *= alpha;
        __syncthreads();   // (Vs is written)
#pragma unroll
        for (int s = 0; s < 16; ++s) {
          const int kk = (s & 3) + 8 * (s >> 2) + 4 * half;
          acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[col * 32 + (kk ^ col)], st[s], acc[c], 0, 0, 0);
        }
      }
    }
  }
  const float inv = 1.f / den;
  if constexpr (LSE)
    if (wok && half == 0) srf_mha_store_lse(((size_t)b * a.H + h) * Lq + ql, (RAGGED && !qok) ? 0.f : m + logf(den), x...);
  if (wok) {
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int j = c * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (j < d) oh[(size_t)j * Lq + ql] = (RAGGED && !qok) ? 0.f : acc[c][r] * inv;
      }
  }
}

// ---- generic form: one wavefront per query (SRF_MHA_GEN_T output channels per lane)
__device__ __forceinline__ float srf_mha_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float srf_mha_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
template <typename... X>   // (the pack and the ragged contract: srf_mha_mfma_kernel above)
__global__ __launch_bounds__(256) void srf_mha_generic_kernel(MhaArgs a, X... x) {
  constexpr bool LSE = sizeof...(X) & 1, RAGGED = sizeof...(X) >= 2;
  const int lane = threadIdx.x & 63;
  const int ql = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int h = blockIdx.y, b = blockIdx.z, d = a.d, Lq = a.Lq, Lk = a.Lk;
  if (ql >= Lq) return;   // (wavefront-uniform; the kernel has no block-wide barrier)
  const int qn = srf_mha_qlen(b, Lq, x...), kn = srf_mha_klen(b, Lk, x...);   // the example's own counts
  const float* qh = a.q + (size_t)b * a.qs + (size_t)h * d * Lq + ql;
  const float* kh = a.k + (size_t)b * a.ks + (size_t)h * d * Lk;
  const float* vh = a.v + (size_t)b * a.vs + (size_t)h * d * Lk;
  float* oh = a.o + (size_t)b * a.os + (size_t)h * d * Lq + ql;
  if constexpr (RAGGED) {
    if (ql >= qn) {   // a query past the example's end: zeros, nothing read
      for (int j = lane; j < d; j += 64) oh[(size_t)j * Lq] = 0.f;
      if (LSE && lane == 0) srf_mha_store_lse(((size_t)b * a.H + h) * Lq + ql, 0.f, x...);
      return;
    }
  }
  float acc[SRF_MHA_GEN_T];
#pragma unroll
  for (int t = 0; t < SRF_MHA_GEN_T; ++t) acc[t] = 0.f;
  float m = SRF_MHA_NEG_INF, den = 0.f;
  for (int kt = 0; kt < kn; kt += 64) {
    const int key = kt + lane;
    const bool kok = key < kn;
    float s = 0.f;
    if (kok)
      for (int j = 0; j < d; ++j) s = fmaf(qh[(size_t)j * Lq] * a.scale, kh[(size_t)j * Lk + key], s);
    s = kok ? s : SRF_MHA_NEG_INF;
    const float mn = fmaxf(m, srf_mha_wave_max(s));   // finite: key kt itself is inside
    const float alpha = expf(m - mn);
    const float p = expf(s - mn);                     // masked keys: 0
    den = den * alpha + srf_mha_wave_sum(p);
    m = mn;
#pragma unroll
    for (int t = 0; t < SRF_MHA_GEN_T; ++t) acc[t] *= alpha;
    const int nk = kn - kt < 64 ? kn - kt : 64;
    for (int kk = 0; kk < nk; ++kk) {
      const float pk = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p), kk));
#pragma unroll
      for (int t = 0; t < SRF_MHA_GEN_T; ++t) {
        const int j = lane + 64 * t;
        if (j < d) acc[t] = fmaf(pk, vh[(size_t)j * Lk + kt + kk], acc[t]);
      }
    }
  }
  const float inv = 1.f / den;
  if constexpr (LSE)
    if (lane == 0) srf_mha_store_lse(((size_t)b * a.H + h) * Lq + ql, m + logf(den), x...);
#pragma unroll
  for (int t = 0; t < SRF_MHA_GEN_T; ++t) {
    const int j = lane + 64 * t;
    if (j < d) oh[(size_t)j * Lq] = acc[t] * inv;
  }
}

// the dispatch test: 1 = the MFMA form serves head dimension d under the current kernel mode (mode 1: generic kernels only)
extern "C" int srf_mha_attention_mfma_supported(int d) {
  return srf_kernel_mode() != 1 && d % 16 == 0 && d >= 16 && d <= 256;
}

// one dispatch for the plain, the lse and the ragged forms: x = the kernels' pack ([float* lse] [SrfFrames, SrfFrames])
template <typename... X>
static int srf_mha_launch(const MhaArgs& a, int Bt, hipStream_t st, const char* mfma_name, const char* generic_name, X... x) {
  const int H = a.H, d = a.d, Lq = a.Lq;
  if (srf_mha_attention_mfma_supported(d)) {
    const dim3 grid((Lq + 31) / 32, H, Bt), block(64);
    if (d <= 32) hipLaunchKernelGGL((srf_mha_mfma_kernel<1, X...>), grid, block, 0, st, a, x...);
    else if (d <= 64) hipLaunchKernelGGL((srf_mha_mfma_kernel<2, X...>), grid, block, 0, st, a, x...);
    else if (d <= 128) hipLaunchKernelGGL((srf_mha_mfma_kernel<4, X...>), grid, block, 0, st, a, x...);
    else hipLaunchKernelGGL((srf_mha_mfma_kernel<8, X...>), grid, block, 0, st, a, x...);
    SRF_CHECK_LAUNCH(mfma_name, st);
    return SRF_OK;
  }
  SRF_CHECK_ARG(d <= 64 * SRF_MHA_GEN_T, "srf_mha_attention: head dimension d = %d exceeds the generic kernel's %d", d,
                64 * SRF_MHA_GEN_T);
  hipLaunchKernelGGL((srf_mha_generic_kernel<X...>), dim3((Lq + 3) / 4, H, Bt), dim3(256), 0, st, a, x...);
  SRF_CHECK_LAUNCH(generic_name, st);
  return SRF_OK;
}

static int srf_mha_check(const float* q, const float* k, const float* v, float* o, int Bt, int H, int d, int Lq, int Lk) {
  SRF_CHECK_ARG(q && k && v && o, "srf_mha_attention: null pointer");
  SRF_CHECK_ARG(Bt > 0 && H > 0 && d > 0 && Lq > 0 && Lk > 0, "srf_mha_attention: bad sizes (Bt %d, H %d, d %d, Lq %d, Lk %d)", Bt,
                H, d, Lq, Lk);
  SRF_CHECK_ARG(Bt <= 65535 && H <= 65535, "srf_mha_attention: batch / heads too large (max 65535 each)");
  SRF_CHECK_ARG((long)H * d * (Lq > Lk ? Lq : Lk) < (1L << 31), "srf_mha_attention: one example exceeds 2^31 elements");
  return SRF_OK;
}

// ---- the two tables of a ragged call (NULL = every example full on that side)
int srf_mha_ragged_tables(const char* fn, int Bt, int Lq, int Lk, const int* q_lengths, const int* k_lengths, SrfFrames* qf,
                          SrfFrames* kf) {
  SRF_CHECK_ARG(Bt >= 1 && Bt <= SRF_RAGGED_MAX_BATCH, "%s: a ragged batch holds 1..%d examples (got Bt = %d)", fn,
                SRF_RAGGED_MAX_BATCH, Bt);
  const int* given[2] = {q_lengths, k_lengths};
  const int stride[2] = {Lq, Lk};
  SrfFrames* out[2] = {qf, kf};
  for (int s = 0; s < 2; ++s) {
    for (int b = 0; b < SRF_RAGGED_MAX_BATCH; ++b) out[s]->n[b] = 0;
    for (int b = 0; b < Bt; ++b) {
      const int n = given[s] ? given[s][b] : stride[s];
      SRF_CHECK_ARG(n >= 1 && n <= stride[s], "%s: example %d has %s = %d (allowed: 1..%s = %d)", fn, b,
                    s ? "k_lengths[b]" : "q_lengths[b]", n, s ? "Lk" : "Lq", stride[s]);
      out[s]->n[b] = n;
    }
  }
  return SRF_OK;
}

// ---- the host path of all four forms: the uniform checks, lse, the two tables, then the one dispatch on the form's pack.
// Row `form` of each table: the public entry (the error strings) and the profiler names, string literals that outlive the call.
int srf_mha_forward(int form, const MhaArgs& a, int Bt, float* lse, const int* q_lengths, const int* k_lengths, hipStream_t st) {
  static const char* const entry[4] = {"srf_mha_attention", "srf_mha_attention_lse", "srf_mha_attention_ragged",
                                       "srf_mha_attention_lse_ragged"};
  static const char* const name[4][2] = {{"mha_attention_mfma", "mha_attention_generic"},
                                         {"mha_attention_lse_mfma", "mha_attention_lse_generic"},
                                         {"mha_attention_mfma_ragged", "mha_attention_generic_ragged"},
                                         {"mha_attention_lse_mfma_ragged", "mha_attention_lse_generic_ragged"}};
  int rc = srf_mha_check(a.q, a.k, a.v, a.o, Bt, a.H, a.d, a.Lq, a.Lk);
  if (rc != SRF_OK) return rc;
  if (form & SRF_MHA_LSE) SRF_CHECK_ARG(lse, "%s: lse is null", entry[form]);
  const char *mfma = name[form][0], *generic = name[form][1];
  if (form == 0) return srf_mha_launch(a, Bt, st, mfma, generic);
  if (form == SRF_MHA_LSE) return srf_mha_launch(a, Bt, st, mfma, generic, lse);
  SrfFrames qf, kf;
  rc = srf_mha_ragged_tables(entry[form], Bt, a.Lq, a.Lk, q_lengths, k_lengths, &qf, &kf);
  if (rc != SRF_OK) return rc;
  if (form == SRF_MHA_RAGGED) return srf_mha_launch(a, Bt, st, mfma, generic, qf, kf);
  return srf_mha_launch(a, Bt, st, mfma, generic, lse, qf, kf);
}

// the contiguous tensors of the public entries: q, o [Bt, H d, Lq], k, v [Bt, H d, Lk]
static MhaArgs srf_mha_contiguous(const float* q, const float* k, const float* v, float* o, int H, int d, int Lq, int Lk,
                                  float scale) {
  const long sq = (long)H * d * Lq, sk = (long)H * d * Lk;
  return MhaArgs{q, k, v, o, sq, sk, sk, sq, H, d, Lq, Lk, scale};
}

extern "C" int srf_mha_attention(const float* q, const float* k, const float* v, float* o, int Bt, int H, int d, int Lq, int Lk,
                                 float scale, void* stream) {
  SRF_CHECK_ARG(H > 0 && d > 0 && Lq > 0 && Lk > 0, "srf_mha_attention: bad sizes (H %d, d %d, Lq %d, Lk %d)", H, d, Lq, Lk);
  return srf_mha_forward(0, srf_mha_contiguous(q, k, v, o, H, d, Lq, Lk, scale), Bt, nullptr, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int srf_mha_attention_lse(const float* q, const float* k, const float* v, float* o, float* lse, int Bt, int H, int d,
                                     int Lq, int Lk, float scale, void* stream) {
  SRF_CHECK_ARG(H > 0 && d > 0 && Lq > 0 && Lk > 0, "srf_mha_attention_lse: bad sizes (H %d, d %d, Lq %d, Lk %d)", H, d, Lq, Lk);
  return srf_mha_forward(SRF_MHA_LSE, srf_mha_contiguous(q, k, v, o, H, d, Lq, Lk, scale), Bt, lse, nullptr, nullptr,
                         (hipStream_t)stream);
}

extern "C" int srf_mha_attention_ragged(const float* q, const float* k, const float* v, float* o, int Bt, int H, int d, int Lq,
                                        int Lk, const int* q_lengths, const int* k_lengths, float scale, void* stream) {
  SRF_CHECK_ARG(H > 0 && d > 0 && Lq > 0 && Lk > 0, "srf_mha_attention_ragged: bad sizes (H %d, d %d, Lq %d, Lk %d)", H, d, Lq, Lk);
  return srf_mha_forward(SRF_MHA_RAGGED, srf_mha_contiguous(q, k, v, o, H, d, Lq, Lk, scale), Bt, nullptr, q_lengths, k_lengths,
                         (hipStream_t)stream);
}

extern "C" int srf_mha_attention_lse_ragged(const float* q, const float* k, const float* v, float* o, float* lse, int Bt, int H,
                                            int d, int Lq, int Lk, const int* q_lengths, const int* k_lengths, float scale,
                                            void* stream) {
  SRF_CHECK_ARG(H > 0 && d > 0 && Lq > 0 && Lk > 0, "srf_mha_attention_lse_ragged: bad sizes (H %d, d %d, Lq %d, Lk %d)", H, d, Lq,
                Lk);
  return srf_mha_forward(SRF_MHA_LSE | SRF_MHA_RAGGED, srf_mha_contiguous(q, k, v, o, H, d, Lq, Lk, scale), Bt, lse, q_lengths,
                         k_lengths, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// x[b, c, l] = GlobLN(a)[b, c, l] + pe[l, c]: the level's lazy norm applied on load, the position table read through a
// 32 x 32 LDS tile (pe is [max_len, C]: consecutive lanes read consecutive channels, then write consecutive positions)
//
// Dropout (srf_posenc_apply_dropout, the PositionalEncoding's nn.Dropout in train() mode).  The keep bit of element
// i = (b C + c) L + l is a pure function of (seed, offset, i): word i & 3 of Philox4x32-10 with the key {lo(seed), hi(seed)} on the
// counter {lo(i >> 2), hi(i >> 2), lo(offset), hi(offset)}, kept where word >= floor(p 2^32) (the threshold is a 64-bit number:
// p = 1 gives 2^32, which no word reaches).  Nothing of the launch enters it, so the backward and a numpy restatement
// (tests/attentive_train_ref.py) recompute the same bit and the mask is never stored.  A dropped element is SELECTED 0.f, never
// multiplied: inv_keep = 1.f / (1.f - p) comes from the host and is inf at p = 1.
// The dropout form takes its state as a trailing parameter PACK (the idiom of the lse forms above): the plain instantiation's
// arguments and code stay what they were.
// ---------------------------------------------------------------------------------------------
struct SrfDropoutDev {
  unsigned key0, key1, off0, off1;
  unsigned long long threshold;   // floor(p * 2^32), in [0, 2^32]
  float inv_keep;                 // 1.f / (1.f - p)
};

__device__ __forceinline__ bool srf_dropout_keep(const SrfDropoutDev& d, unsigned long long i) {
  const unsigned long long blk = i >> 2;
  unsigned c0 = (unsigned)blk, c1 = (unsigned)(blk >> 32), c2 = d.off0, c3 = d.off1;
  unsigned k0 = d.key0, k1 = d.key1;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const unsigned h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  const unsigned w = (unsigned)i & 3u;
  const unsigned word = w == 0 ? c0 : (w == 1 ? c1 : (w == 2 ? c2 : c3));
  return (unsigned long long)word >= d.threshold;
}

__device__ __forceinline__ float srf_posenc_drop(size_t, float v) { return v; }   // (plain)
__device__ __forceinline__ float srf_posenc_drop(size_t at, float v, SrfDropoutDev d) {
  return srf_dropout_keep(d, at) ? v * d.inv_keep : 0.f;
}
__device__ __forceinline__ float srf_posenc_drop(size_t, float v, const SrfFrames&) { return v; }   // (ragged: inference only)
template <typename... X>
struct SrfPosencRagged { static constexpr bool value = false; };
template <>
struct SrfPosencRagged<SrfFrames> { static constexpr bool value = true; };

// RAGGED (srf_posenc_apply_ragged; the pack is one SrfFrames): L stays the row stride, example g is frames[g] positions long;
// the norm counts C * frames[g], neither a nor pe is read at positions >= frames[g], and x is exact 0 there.
template <typename... Drop>
__global__ __launch_bounds__(256) void srf_posenc_apply_kernel(const float* __restrict__ a, SrfNormDev nrm, const float* __restrict__ pe,
                                                               float* __restrict__ x, double inv_count, int C, int L, Drop... drop) {
  constexpr bool RAGGED = SrfPosencRagged<Drop...>::value;
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int l0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const long g = blockIdx.z;
  int own = L;      // (RAGGED) the example's own positions
  if constexpr (RAGGED) {
    own = srf_frames_of((int)g, drop...);
    inv_count = 1.0 / ((double)C * (double)own);
  }
  float mean = 0.f, rstd = 1.f;
  if (nrm.sums) srf_finalize_stats(nrm.sums, g, inv_count, mean, rstd);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int l = l0 + ty + 8 * i, c = c0 + tx;
    tile[ty + 8 * i][tx] = (l < own && c < C) ? pe[(size_t)l * C + c] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = c0 + ty + 8 * i, l = l0 + tx;
    if (c < C && l < own) {
      float sc = 1.f, sh = 0.f;
      if (nrm.sums) {
        sc = nrm.gamma[c] * rstd;
        sh = nrm.beta[c] - mean * sc;
      }
      const size_t at = ((size_t)g * C + c) * L + l;
      x[at] = srf_posenc_drop(at, fmaf(a[at], sc, sh) + tile[tx][ty + 8 * i], drop...);
    } else if constexpr (RAGGED) {
      if (c < C && l < L) x[((size_t)g * C + c) * L + l] = 0.f;
    }
  }
}

// the grid and the launch of both entries (drop: nothing, or the dropout state); the arguments are the entry's to check
template <typename... Drop>
static void srf_posenc_launch(const float* a, const SrfNormDev& nd, const float* pe, float* x, int Bt, int C, int L, void* stream,
                              Drop... drop) {
  hipLaunchKernelGGL(srf_posenc_apply_kernel<Drop...>, dim3((L + 31) / 32, (C + 31) / 32, Bt), dim3(256), 0, (hipStream_t)stream, a, nd,
                     pe, x, 1.0 / ((double)C * (double)L), C, L, drop...);
}

extern "C" int srf_posenc_apply(const float* a, const srf_norm* norm, const float* pe, float* x, int Bt, int C, int L,
                                int max_len, void* stream) {
  SRF_CHECK_ARG(a && pe && x && Bt > 0 && C > 0 && L > 0, "srf_posenc_apply: bad arguments");
  SRF_CHECK_ARG(L <= max_len, "srf_posenc_apply: L = %d positions exceed the table's max_len = %d", L, max_len);
  SRF_CHECK_ARG(Bt <= 65535 && (C + 31) / 32 <= 65535, "srf_posenc_apply: batch / channels too large");
  const SrfNormDev nd = srf_norm_dev(norm);
  if (nd.sums) SRF_CHECK_ARG(nd.gamma && nd.beta, "srf_posenc_apply: norm without gamma/beta");
  SRF_CHECK_ALIGNED16("srf_posenc_apply", {"norm.sums", nd.sums});
  srf_posenc_launch(a, nd, pe, x, Bt, C, L, stream);
  SRF_CHECK_LAUNCH("posenc_apply", stream);
  return SRF_OK;
}

extern "C" int srf_posenc_apply_ragged(const float* a, const srf_norm* norm, const float* pe, float* x, int Bt, int C, int L,
                                       int max_len, const int* frames, void* stream) {
  SRF_CHECK_ARG(a && pe && x && Bt > 0 && C > 0 && L > 0, "srf_posenc_apply_ragged: bad arguments");
  SRF_CHECK_ARG(L <= max_len, "srf_posenc_apply_ragged: L = %d positions exceed the table's max_len = %d", L, max_len);
  SRF_CHECK_ARG((C + 31) / 32 <= 65535, "srf_posenc_apply_ragged: channels too large");
  const SrfNormDev nd = srf_norm_dev(norm);
  if (nd.sums) SRF_CHECK_ARG(nd.gamma && nd.beta, "srf_posenc_apply_ragged: norm without gamma/beta");
  SRF_CHECK_ALIGNED16("srf_posenc_apply_ragged", {"norm.sums", nd.sums});
  SrfFrames fr;
  const int rc = srf_frames_table("srf_posenc_apply_ragged", frames, Bt, L, &fr);
  if (rc) return rc;
  srf_posenc_launch(a, nd, pe, x, Bt, C, L, stream, fr);
  SRF_CHECK_LAUNCH("posenc_apply_ragged", stream);
  return SRF_OK;
}

// p in [0, 1] (NaN fails both comparisons) -> the by-value state of the dropout kernels
static int srf_dropout_state(const char* fn, float p, unsigned long long seed, unsigned long long offset, SrfDropoutDev* out) {
  SRF_CHECK_ARG(p >= 0.f && p <= 1.f, "%s: p = %g is outside [0, 1]", fn, (double)p);
  out->key0 = (unsigned)seed;
  out->key1 = (unsigned)(seed >> 32);
  out->off0 = (unsigned)offset;
  out->off1 = (unsigned)(offset >> 32);
  out->threshold = (unsigned long long)((double)p * 4294967296.0);   // floor: the product is exact in double and >= 0
  out->inv_keep = 1.f / (1.f - p);
  return SRF_OK;
}

extern "C" int srf_posenc_apply_dropout(const float* a, const srf_norm* norm, const float* pe, float* x, int Bt, int C, int L,
                                        int max_len, float p, unsigned long long seed, unsigned long long offset, void* stream) {
  SrfDropoutDev dd;
  const int rc = srf_dropout_state("srf_posenc_apply_dropout", p, seed, offset, &dd);
  if (rc != SRF_OK) return rc;
  if (p == 0.f) return srf_posenc_apply(a, norm, pe, x, Bt, C, L, max_len, stream);   // the plain kernel: today's bits
  SRF_CHECK_ARG(a, "srf_posenc_apply_dropout: a is null");
  SRF_CHECK_ARG(pe, "srf_posenc_apply_dropout: pe is null");
  SRF_CHECK_ARG(x, "srf_posenc_apply_dropout: x is null");
  SRF_CHECK_ARG(Bt > 0 && C > 0 && L > 0, "srf_posenc_apply_dropout: bad sizes (Bt %d, C %d, L %d)", Bt, C, L);
  SRF_CHECK_ARG(L <= max_len, "srf_posenc_apply_dropout: L = %d positions exceed the table's max_len = %d", L, max_len);
  SRF_CHECK_ARG(Bt <= 65535 && (C + 31) / 32 <= 65535, "srf_posenc_apply_dropout: batch / channels too large");
  const SrfNormDev nd = srf_norm_dev(norm);
  if (nd.sums) SRF_CHECK_ARG(nd.gamma && nd.beta, "srf_posenc_apply_dropout: norm without gamma/beta");
  SRF_CHECK_ALIGNED16("srf_posenc_apply_dropout", {"norm.sums", nd.sums});
  srf_posenc_launch(a, nd, pe, x, Bt, C, L, stream, dd);
  SRF_CHECK_LAUNCH("posenc_apply_dropout", stream);
  return SRF_OK;
}

// gn[i] = keep(i) ? gx[i] * inv_keep : 0 (in place when gn == gx: every element is read and written by one thread), and the
// mask itself as bytes.  Grid-stride over a 64-bit index; every access is under i < n.
__global__ __launch_bounds__(256) void srf_posenc_dropout_bwd_kernel(const float* gx, float* gn, long n, SrfDropoutDev dd) {
  const long step = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += step)
    gn[i] = srf_dropout_keep(dd, (unsigned long long)i) ? gx[i] * dd.inv_keep : 0.f;
}

__global__ __launch_bounds__(256) void srf_dropout_mask_kernel(unsigned char* __restrict__ keep, long n, SrfDropoutDev dd) {
  const long step = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += step)
    keep[i] = srf_dropout_keep(dd, (unsigned long long)i) ? 1 : 0;
}

static unsigned srf_dropout_blocks(long n) { return (unsigned)std::min<long>((n + 255) / 256, 1L << 20); }

extern "C" int srf_posenc_dropout_bwd(const float* gx, float* gn, int Bt, int C, int L, float p, unsigned long long seed,
                                      unsigned long long offset, void* stream) {
  SrfDropoutDev dd;
  const int rc = srf_dropout_state("srf_posenc_dropout_bwd", p, seed, offset, &dd);
  if (rc != SRF_OK) return rc;
  SRF_CHECK_ARG(gx, "srf_posenc_dropout_bwd: gx is null");
  SRF_CHECK_ARG(gn, "srf_posenc_dropout_bwd: gn is null");
  SRF_CHECK_ARG(Bt > 0 && C > 0 && L > 0, "srf_posenc_dropout_bwd: bad sizes (Bt %d, C %d, L %d)", Bt, C, L);
  const long n = (long)Bt * C * L;
  if (p == 0.f && gn == gx) return SRF_OK;   // the identity in place
  hipLaunchKernelGGL(srf_posenc_dropout_bwd_kernel, dim3(srf_dropout_blocks(n)), dim3(256), 0, (hipStream_t)stream, gx, gn, n, dd);
  SRF_CHECK_LAUNCH("posenc_dropout_bwd", stream);
  return SRF_OK;
}

extern "C" int srf_dropout_mask(unsigned char* keep, long n, float p, unsigned long long seed, unsigned long long offset,
                                void* stream) {
  SrfDropoutDev dd;
  const int rc = srf_dropout_state("srf_dropout_mask", p, seed, offset, &dd);
  if (rc != SRF_OK) return rc;
  SRF_CHECK_ARG(keep, "srf_dropout_mask: keep is null");
  SRF_CHECK_ARG(n > 0, "srf_dropout_mask: n = %ld", n);
  hipLaunchKernelGGL(srf_dropout_mask_kernel, dim3(srf_dropout_blocks(n)), dim3(256), 0, (hipStream_t)stream, keep, n, dd);
  SRF_CHECK_LAUNCH("dropout_mask", stream);
  return SRF_OK;
}

// ---------------------------------------------------------------------------------------------
// z = norm_f(f) + norm_y(y) (each a GlobLN with optional PReLU, statistics from its own slot), out_sums += {sum, sumsq} of z.
// The transformer layer's closing step: ffn's GlobLN + PReLU and out_mha_norm applied on load, the sum's statistics for out_norm.
// One block per (row = (g, c), chunk of 1024 positions), as srf_gln_apply.
// ---------------------------------------------------------------------------------------------
// RAGGED (srf_gln_apply2_add_ragged; FR = SrfFrames): `length` stays the row stride, group g is frames[g] columns long (any count
// >= 1: every access is a dword); both norms count channels * frames[g], f and y are not read at columns >= frames[g], z is
// exact 0 there and out_sums run over the group's own columns.
template <typename... FR>
__global__ __launch_bounds__(256) void srf_gln_apply2_add_kernel(const float* __restrict__ f, SrfNormDev nf, const float* __restrict__ y,
                                                                 SrfNormDev ny, float* __restrict__ z, double* __restrict__ out_sums,
                                                                 double inv_count, int channels, int length, int chunks, FR... fr) {
  constexpr bool RAGGED = sizeof...(FR) != 0;
  __shared__ double red[8];
  const long row = blockIdx.x / chunks;
  const int chunk = blockIdx.x - row * chunks;
  const int c = (int)(row % channels);
  const long g = row / channels;
  int own = length;      // (RAGGED) the group's own columns
  if constexpr (RAGGED) {
    own = srf_frames_of((int)g, fr...);
    inv_count = 1.0 / ((double)channels * (double)own);
  }
  float mf, rf, my, ry;
  srf_finalize_stats(nf.sums, g, inv_count, mf, rf);
  srf_finalize_stats(ny.sums, g, inv_count, my, ry);
  const float scf = nf.gamma[c] * rf, shf = nf.beta[c] - mf * scf;
  const float scy = ny.gamma[c] * ry, shy = ny.beta[c] - my * scy;
  const bool actf = nf.prelu != nullptr, acty = ny.prelu != nullptr;
  const float slf = actf ? nf.prelu[0] : 1.f, sly = acty ? ny.prelu[0] : 1.f;
  const size_t base = (size_t)row * length;
  double ds = 0.0, dq = 0.0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int l = chunk * 1024 + u * 256 + threadIdx.x;
    if (l < own) {
      float vf = fmaf(f[base + l], scf, shf);
      if (actf) vf = srf_prelu(vf, slf);
      float vy = fmaf(y[base + l], scy, shy);
      if (acty) vy = srf_prelu(vy, sly);
      const float v = vf + vy;
      z[base + l] = v;
      ds += (double)v;
      dq += (double)v * (double)v;
    } else if constexpr (RAGGED) {
      if (l < length) z[base + l] = 0.f;
    }
  }
  if (out_sums) srf_block_stats_atomic<4>(ds, dq, srf_stat_slot(out_sums, g, blockIdx.x), red);
}

// who: the entry point's name in its refusals; frames: NULL = the uniform call, else one entry per group (srf_gln_apply2_add_ragged)
static int gln_apply2_add_impl(const char* who, const float* f, const srf_norm* fnorm, const float* y, const srf_norm* ynorm, float* z,
                               double* out_sums, int groups, int channels, int length, const int* frames, void* stream) {
  SRF_CHECK_ARG(f && y && z && fnorm && ynorm && groups > 0 && channels > 0 && length > 0, "%s: bad arguments", who);
  SRF_CHECK_ARG(fnorm->sums && fnorm->gamma && fnorm->beta && ynorm->sums && ynorm->gamma && ynorm->beta,
                "%s: both norms need statistics, gamma and beta", who);
  SRF_CHECK_ALIGNED16(who, {"fnorm.sums", fnorm->sums}, {"ynorm.sums", ynorm->sums});
  const int chunks = (length + 1023) / 1024;
  const long blocks = (long)groups * channels * chunks;
  SRF_CHECK_ARG(blocks < (1L << 31), "%s: tensor too large", who);
  if (frames) {
    SrfFrames fr;
    const int rc = srf_frames_table(who, frames, groups, length, &fr);
    if (rc) return rc;
    hipLaunchKernelGGL(srf_gln_apply2_add_kernel<SrfFrames>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, f,
                       srf_norm_dev(fnorm), y, srf_norm_dev(ynorm), z, out_sums, 1.0 / ((double)channels * (double)length), channels,
                       length, chunks, fr);
    SRF_CHECK_LAUNCH("gln_apply2_add_ragged", stream);
    return SRF_OK;
  }
  hipLaunchKernelGGL(srf_gln_apply2_add_kernel<>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, f, srf_norm_dev(fnorm), y,
                     srf_norm_dev(ynorm), z, out_sums, 1.0 / ((double)channels * (double)length), channels, length, chunks);
  SRF_CHECK_LAUNCH("gln_apply2_add", stream);
  return SRF_OK;
}

extern "C" int srf_gln_apply2_add(const float* f, const srf_norm* fnorm, const float* y, const srf_norm* ynorm, float* z,
                                  double* out_sums, int groups, int channels, int length, void* stream) {
  return gln_apply2_add_impl("srf_gln_apply2_add", f, fnorm, y, ynorm, z, out_sums, groups, channels, length, nullptr, stream);
}

extern "C" int srf_gln_apply2_add_ragged(const float* f, const srf_norm* fnorm, const float* y, const srf_norm* ynorm, float* z,
                                         double* out_sums, int groups, int channels, int length, const int* frames, void* stream) {
  SRF_CHECK_ARG(frames != nullptr, "srf_gln_apply2_add_ragged: null frames table");
  return gln_apply2_add_impl("srf_gln_apply2_add_ragged", f, fnorm, y, ynorm, z, out_sums, groups, channels, length, frames, stream);
}

// ---------------------------------------------------------------------------------------------
// y = norm(x) (a GlobLN with optional PReLU, statistics from its slot), out_sums += {sum, sumsq} of the stored y.
// Attentive v3 needs a normalised tensor in memory twice per block: the asking level is the residual of O_proj (the GEMM's
// residual is a raw pointer), and final_norm sits on top of the last resampler's out_norm -- a GlobLN over an already-normalised
// tensor, whose moments (gamma and beta are per channel) do not follow from the global sums of its input.
// One block per (row = (g, c), chunk of 1024 positions), as srf_gln_apply2_add; dword accesses: any address, any length.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void srf_gln_apply_stats_kernel(const float* __restrict__ x, SrfNormDev n, float* __restrict__ y,
                                                                  double* __restrict__ out_sums, double inv_count, int channels,
                                                                  int length, int chunks) {
  __shared__ double red[8];
  const long row = blockIdx.x / chunks;
  const int chunk = blockIdx.x - row * chunks;
  const int c = (int)(row % channels);
  const long g = row / channels;
  float mean, rstd;
  srf_finalize_stats(n.sums, g, inv_count, mean, rstd);
  const float sc = n.gamma[c] * rstd, sh = n.beta[c] - mean * sc;
  const bool act = n.prelu != nullptr;
  const float slope = act ? n.prelu[0] : 1.f;
  const size_t base = (size_t)row * length;
  double ds = 0.0, dq = 0.0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int l = chunk * 1024 + u * 256 + threadIdx.x;
    if (l < length) {
      float v = fmaf(x[base + l], sc, sh);
      if (act) v = srf_prelu(v, slope);
      y[base + l] = v;
      ds += (double)v;
      dq += (double)v * (double)v;
    }
  }
  if (out_sums) srf_block_stats_atomic<4>(ds, dq, srf_stat_slot(out_sums, g, blockIdx.x), red);
}

extern "C" int srf_gln_apply_stats(const float* x, const srf_norm* norm, float* y, double* out_sums, int groups, int channels,
                                   int length, void* stream) {
  SRF_CHECK_ARG(x && y && norm && groups > 0 && channels > 0 && length > 0, "srf_gln_apply_stats: bad arguments");
  SRF_CHECK_ARG(norm->sums && norm->gamma && norm->beta, "srf_gln_apply_stats: the norm needs statistics, gamma and beta");
  SRF_CHECK_ARG((const void*)norm->sums != (const void*)out_sums, "srf_gln_apply_stats: out_sums must not be norm.sums");
  SRF_CHECK_ALIGNED16("srf_gln_apply_stats", {"norm.sums", norm->sums});
  const int chunks = (length + 1023) / 1024;
  const long blocks = (long)groups * channels * chunks;
  SRF_CHECK_ARG(blocks < (1L << 31), "srf_gln_apply_stats: tensor too large");
  hipLaunchKernelGGL(srf_gln_apply_stats_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, srf_norm_dev(norm), y,
                     out_sums, 1.0 / ((double)channels * (double)length), channels, length, chunks);
  SRF_CHECK_LAUNCH("gln_apply_stats", stream);
  return SRF_OK;
}
