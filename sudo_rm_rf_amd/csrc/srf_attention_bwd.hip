// Backward of softmax attention (srf_mha_attention_bwd; forward: srf_attention.hip, whose header comment this one continues).
//
// Per (example, head), with S = (scale q)^T k, P = softmax_keys(S) = exp(S - lse), O = P V and the incoming gO:
//     delta[lq] = sum_j gO[j, lq] O[j, lq]
//     gV[j, lk] = sum_lq P[lq, lk] gO[j, lq]
//     dP[lq, lk] = sum_j gO[j, lq] V[j, lk]            dS = P o (dP - delta)
//     gQ[j, lq] = scale sum_lk dS[lq, lk] K[j, lk]      gK[j, lk] = scale sum_lq dS[lq, lk] Q[j, lq]
// P is recomputed from the forward's per-query log-sum-exp; neither S, P, dP nor dS ever reaches memory.  No float atomics
// and no reduction across blocks: every output element is accumulated by ONE wavefront in a fixed order, so equal inputs
// give equal bits.
//
// Launches: delta (one thread per query, into the caller's workspace [Bt, H, Lq]), then
//   the MFMA form (d % 16 == 0, 16 <= d <= 256, kernel modes 0 and 2), ONE kernel template in four roles.  A wavefront OWNS a
//   tile of 32 positions of one side and loops over tiles of 32 of the other side:
//     role Q   owns 32 queries, loops over key tiles,   accumulates gQ            (mha_attention_bwd_dq_mfma)
//     role KV  owns 32 keys,    loops over query tiles, accumulates gK and gV     (mha_attention_bwd_dkv_mfma, d <= 128)
//     role V / role K: the same with one accumulator each -- at d = 256 the two together would be 2 x 128 accumulator
//              registers per wavefront, so the key side runs as two passes    (mha_attention_bwd_dv_mfma, .._dk_mfma)
//   As in the forward the OWNED position is the N index of every product (lane l owns column l & 31), on exact-fp32
//   v_mfma_f32_32x32x2_f32:
//     T[other, own]  = sum_j Y1[j, other] X1[j, own]      A = Y1 read from global, B = X1 staged once in LDS ([d][32])
//     dT[other, own] = sum_j Y2[j, other] X2[j, own]      A = Y2 read from global, B = X2 read from global (dword, predicated)
//     G^T[j, own]   += sum_other Y[j, other] W[other, own]  A = a 32-channel chunk of Y through LDS (XOR-swizzled rows),
//                                                          B = W = dS or P, straight from the accumulator registers
//   with (X1, X2, Y1, Y2) = (scale q, gO, k, v) for role Q, where T = S^T, and (k, v, scale q, gO) for the key side, where
//   T = S.  Register r of T holds the other-side position (r & 3) + 8 (r >> 2) + 4 (l >> 5), and step r of the third product
//   contracts over exactly that pair, so P and dS go from one product's accumulator into the next product's B operand
//   without leaving the registers (the forward's trick, used for P -> gV and dS -> gQ / gK alike).  lse and delta belong to
//   the QUERY: per-lane scalars in role Q, per-register values (read once per query tile) on the key side.
//   LDS: 32 d + 1024 floats per block as in the forward (36 KB at d = 256, four blocks per CU); X2 is re-read from global per
//   tile (32 d floats, cache-resident) rather than staged, which would double that.
//   the generic form (every other d <= 1024, every d in kernel mode 1): a wavefront per query for gQ and a wavefront per key
//   for gK / gV, a lane per other-side position for the scores and a lane per channel for the sums (v_readlane), plain FMA.
// Edges, as in the forward: every global access is one dword wide and predicated; keys >= Lk, queries >= Lq and channels >= d
// read nothing, count as 0 and store nothing; a masked position has P = 0 EXACTLY (selected, never exp of a stale register).
//
// Ragged forms (srf_mha_attention_bwd_ragged): every kernel takes a trailing parameter pack, empty in the uniform instantiations
// (arguments and code unchanged) and (SrfFrames q_len, SrfFrames k_len) -- delta: q_len alone -- in the ragged ones.  Lq and Lk
// stay the row strides of every address; every predicate and loop bound uses example b's own counts.  Nothing at or past a count
// is read (q, go, o, lse, delta on the query side; k, v on the key side); gq, gk and gv are written as exact 0.f from the count
// up to the stride, delta is left alone there; a block whose whole owned tile lies past the count stores its zeros and returns
// before any load, LDS write or MFMA, and the loop over the other side runs to that side's own count.  Inside the counts the
// arithmetic and its order are those of the uniform kernel on example b alone.
//
// Host path: both public entries check their sizes, set the contiguous strides and call srf_mha_backward: checks, (ragged)
// tables, then srf_mha_bwd_run, the one launch sequence, instantiated without and with the tables.
#include "srf_mha.h"

// ---- delta[b, h, lq] = sum_j gO[j, lq] O[j, lq]: one thread per query, channels in order
template <typename... R>
__global__ __launch_bounds__(256) void srf_mha_bwd_delta_kernel(const float* __restrict__ o, const float* __restrict__ go,
                                                                float* __restrict__ delta, long os, long gos, int H, int d, int Lq,
                                                                R... qlen) {
  const int lq = blockIdx.x * 256 + threadIdx.x;
  const int h = blockIdx.y, b = blockIdx.z;
  if (lq >= Lq) return;
  if constexpr (sizeof...(R) > 0)
    if (lq >= srf_frames_of(b, qlen...)) return;   // (past the example's end: nothing read, delta left as it is)
  const float* oh = o + (size_t)b * os + (size_t)h * d * Lq + lq;
  const float* gh = go + (size_t)b * gos + (size_t)h * d * Lq + lq;
  float s = 0.f;
  for (int j = 0; j < d; ++j) s = fmaf(gh[(size_t)j * Lq], oh[(size_t)j * Lq], s);
  delta[((size_t)b * H + h) * Lq + lq] = s;
}

// ---- MFMA form
enum { SRF_MHA_BWD_Q = 0, SRF_MHA_BWD_KV = 1, SRF_MHA_BWD_V = 2, SRF_MHA_BWD_K = 3 };

// t[r] = p[(c0 + 2 r) L] for the channels below d, else 0 -- nothing is read where !ok.  c0 < d and d % 16 == 0: the chunk is full
// or holds its first 16 channels, so two predicates serve the 16 loads (one branch each instead of one per load)
__device__ __forceinline__ void srf_mha_bwd_load16(float (&t)[16], const float* p, bool ok, int c0, int d, int L) {
#pragma unroll
  for (int r = 0; r < 16; ++r) t[r] = 0.f;
  if (ok) {
#pragma unroll
    for (int r = 0; r < 8; ++r) t[r] = p[(size_t)(c0 + 2 * r) * L];
    if (c0 + 16 < d) {
#pragma unroll
      for (int r = 8; r < 16; ++r) t[r] = p[(size_t)(c0 + 2 * r) * L];
    }
  }
}

// G^T[j, own] += sum_other Y[j, other] W[other, own] for one 32-channel chunk: Y's tile (this lane: position `tok ? yp : none`,
// channels c0 + 2 r + half) goes through the swizzled LDS tile, W comes from the registers
__device__ __forceinline__ void srf_mha_bwd_accumulate(srf_f32x16& acc, const srf_f32x16& w, const float* yp, bool tok, int c0, int d,
                                                       int Lt, float* Ys, int col, int half) {
  float t[16];
  srf_mha_bwd_load16(t, yp, tok, c0, d, Lt);
  __syncthreads();   // (the previous chunk's reads of Ys are done)
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int j = 2 * r + half;
    Ys[j * 32 + (col ^ j)] = t[r];
  }
  __syncthreads();   // (Ys is written)
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    const int kk = (s & 3) + 8 * (s >> 2) + 4 * half;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Ys[col * 32 + (kk ^ col)], w[s], acc, 0, 0, 0);
  }
}

template <int NCH, int ROLE, typename... R>   // 32-channel chunks of the head dimension (d <= 32 NCH): 16 accumulator registers each per output
__global__ __launch_bounds__(64) void srf_mha_bwd_mfma_kernel(MhaBwdArgs a, R... r2) {
  constexpr bool RAGGED = sizeof...(R) > 0;
  constexpr bool OQ = ROLE == SRF_MHA_BWD_Q;                                // the owned side is the query
  constexpr bool WANT_DS = ROLE != SRF_MHA_BWD_V;                            // gQ / gK: needs dP and dS
  constexpr bool WANT_P = ROLE == SRF_MHA_BWD_KV || ROLE == SRF_MHA_BWD_V;   // gV
  __shared__ float Xs[NCH * 32 * 32];   // [channel][owned position]: scale q (role Q) or k
  __shared__ float Ys[32 * 32];         // one 32-channel chunk of the other side's tile: [channel][position ^ channel]
  const int lane = threadIdx.x, col = lane & 31, half = lane >> 5;
  const int h = blockIdx.y, b = blockIdx.z, d = a.d;
  const int Lo = OQ ? a.Lq : a.Lk, Lt = OQ ? a.Lk : a.Lq;   // owned / other row stride
  // owned / other count: the example's own (block-uniform), the strides themselves in the uniform instantiation
  const int no = OQ ? srf_mha_qlen(b, a.Lq, r2...) : srf_mha_klen(b, a.Lk, r2...);
  const int nt = OQ ? srf_mha_klen(b, a.Lk, r2...) : srf_mha_qlen(b, a.Lq, r2...);
  const float* qh = a.q + (size_t)b * a.qs + (size_t)h * d * a.Lq;
  const float* kh = a.k + (size_t)b * a.ks + (size_t)h * d * a.Lk;
  const float* vh = a.v + (size_t)b * a.vs + (size_t)h * d * a.Lk;
  const float* gh = a.go + (size_t)b * a.gos + (size_t)h * d * a.Lq;
  const float* lse = a.lse + ((size_t)b * a.H + h) * a.Lq;
  const float* delta = a.delta + ((size_t)b * a.H + h) * a.Lq;
  const float *x1 = OQ ? qh : kh, *x2 = OQ ? gh : vh, *y1 = OQ ? kh : qh, *y2 = OQ ? vh : gh;
  const float sx = OQ ? a.scale : 1.f, sy = OQ ? 1.f : a.scale;   // q is scaled before the product, as in the forward
  const int oi = blockIdx.x * 32 + col;
  const bool ook = oi < no;
  const bool wok = RAGGED ? oi < Lo : ook;   // ragged: the owned positions from the count up to the stride are written, as zeros
  if constexpr (RAGGED) {
    if ((int)blockIdx.x * 32 >= no) {   // the whole owned tile lies past the example's end
      if (wok) {
        float* gd = (OQ ? a.gq + (size_t)b * a.gqs : a.gk + (size_t)b * a.gks) + (size_t)h * d * Lo + oi;
        float* gp = a.gv + (size_t)b * a.gvs + (size_t)h * d * Lo + oi;
        for (int j = half; j < d; j += 2) {
          if constexpr (WANT_DS) gd[(size_t)j * Lo] = 0.f;
          if constexpr (WANT_P) gp[(size_t)j * Lo] = 0.f;
        }
      }
      return;
    }
  }
  const int nch = (d + 31) / 32;   // chunks in use (<= NCH)

  // (a uniform row pointer + one per-lane offset per operand: 32-bit offsets, checked by the launcher)
  for (int j0 = 0; j0 < NCH * 32; j0 += 2) {
    const int j = j0 + half;
    Xs[j * 32 + col] = (ook && j0 < d) ? x1[(size_t)j * Lo + oi] * sx : 0.f;
  }
  srf_f32x16 accd[WANT_DS ? NCH : 1], accp[WANT_P ? NCH : 1];
#pragma unroll
  for (int c = 0; c < (WANT_DS ? NCH : 1); ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) accd[c][r] = 0.f;
#pragma unroll
  for (int c = 0; c < (WANT_P ? NCH : 1); ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) accp[c][r] = 0.f;
  float lse_l = 0.f, delta_l = 0.f;   // role Q: this lane's query
  if (OQ && ook) {
    lse_l = lse[oi];
    delta_l = delta[oi];
  }
  __syncthreads();

  for (int t0 = 0; t0 < nt; t0 += 32) {
    const int ti = t0 + col;
    const bool tok = ti < nt;
    const float* y1p = y1 + (size_t)half * Lt + ti;   // (dereferenced under tok only)
    const float* y2p = y2 + (size_t)half * Lt + ti;
    // ---- T = Y1^T X1 (S^T in role Q, S on the key side), 16 contraction steps (32 channels) at a time
    srf_f32x16 st, ds;
#pragma unroll
    for (int r = 0; r < 16; ++r) st[r] = ds[r] = 0.f;
    // (the chunk loops of the first two products stay rolled: unrolled, the scheduler hoists every chunk's loads above the
    // first MFMA and the <8> instantiations spill)
#pragma unroll 1
    for (int c = 0; c < nch; ++c) {
      float t[16];
      srf_mha_bwd_load16(t, y1p, tok, c * 32, d, Lt);
#pragma unroll
      for (int r = 0; r < 16; ++r)
        st = __builtin_amdgcn_mfma_f32_32x32x2f32(t[r] * sy, Xs[(c * 32 + 2 * r + half) * 32 + col], st, 0, 0, 0);
    }
    // ---- dT = Y2^T X2 (dP^T / dP): both operands from global memory
    if constexpr (WANT_DS) {
      const float* x2p = x2 + (size_t)half * Lo + oi;   // (dereferenced under ook only)
#pragma unroll 1
      for (int c = 0; c < nch; ++c) {
        float t[16], u[16];
        srf_mha_bwd_load16(t, y2p, tok, c * 32, d, Lt);
        srf_mha_bwd_load16(u, x2p, ook, c * 32, d, Lo);
#pragma unroll
        for (int r = 0; r < 16; ++r) ds = __builtin_amdgcn_mfma_f32_32x32x2f32(t[r], u[r], ds, 0, 0, 0);
      }
    }
    // ---- P = exp(T - lse), dS = P (dT - delta); a position outside its tensor: P = dS = 0 exactly
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ri = t0 + (r & 3) + 8 * (r >> 2) + 4 * half;   // the other-side position register r holds
      const bool rok = ri < nt;
      float l = lse_l, dl = delta_l;
      if (!OQ) {
        l = rok ? lse[ri] : 0.f;
        if (WANT_DS) dl = rok ? delta[ri] : 0.f;
      }
      const float p = (rok && ook) ? expf(st[r] - l) : 0.f;
      st[r] = p;
      if (WANT_DS) ds[r] = p * (ds[r] - dl);
    }
    // ---- G^T += Y W per 32-channel chunk, contracting over the pair of positions that register s of T holds
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      if (c * 32 < d) {
        if constexpr (WANT_P) srf_mha_bwd_accumulate(accp[c], st, y2p, tok, c * 32, d, Lt, Ys, col, half);
        if constexpr (WANT_DS) srf_mha_bwd_accumulate(accd[c], ds, y1p, tok, c * 32, d, Lt, Ys, col, half);
      }
    }
  }
  if (wok) {
    float* gd = (OQ ? a.gq + (size_t)b * a.gqs : a.gk + (size_t)b * a.gks) + (size_t)h * d * Lo + oi;
    float* gp = a.gv + (size_t)b * a.gvs + (size_t)h * d * Lo + oi;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int j = c * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (j < d) {
          if constexpr (WANT_DS) gd[(size_t)j * Lo] = (RAGGED && !ook) ? 0.f : accd[c][r] * a.scale;
          if constexpr (WANT_P) gp[(size_t)j * Lo] = (RAGGED && !ook) ? 0.f : accp[c][r];
        }
      }
  }
}

// ---- generic form (SRF_MHA_GEN_T channels per lane)
// gQ: one wavefront per query, a lane per key for dS, a lane per channel for the sum over keys
template <typename... R>
__global__ __launch_bounds__(256) void srf_mha_bwd_dq_generic_kernel(MhaBwdArgs a, R... r2) {
  const int lane = threadIdx.x & 63;
  const int ql = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int h = blockIdx.y, b = blockIdx.z, d = a.d, Lq = a.Lq, Lk = a.Lk;
  if (ql >= Lq) return;   // (wavefront-uniform; the kernel has no block-wide barrier)
  const int kn = srf_mha_klen(b, Lk, r2...);   // the example's own key count
  if constexpr (sizeof...(R) > 0) {
    if (ql >= srf_mha_qlen(b, Lq, r2...)) {   // a query past the example's end: zeros, nothing read
      float* gz = a.gq + (size_t)b * a.gqs + (size_t)h * d * Lq + ql;
      for (int j = lane; j < d; j += 64) gz[(size_t)j * Lq] = 0.f;
      return;
    }
  }
  const float* qh = a.q + (size_t)b * a.qs + (size_t)h * d * Lq + ql;
  const float* gh = a.go + (size_t)b * a.gos + (size_t)h * d * Lq + ql;
  const float* kh = a.k + (size_t)b * a.ks + (size_t)h * d * Lk;
  const float* vh = a.v + (size_t)b * a.vs + (size_t)h * d * Lk;
  const float lse = a.lse[((size_t)b * a.H + h) * Lq + ql], delta = a.delta[((size_t)b * a.H + h) * Lq + ql];
  float acc[SRF_MHA_GEN_T];
#pragma unroll
  for (int t = 0; t < SRF_MHA_GEN_T; ++t) acc[t] = 0.f;
  for (int kt = 0; kt < kn; kt += 64) {
    const int key = kt + lane;
    float ds = 0.f;   // masked keys: 0
    if (key < kn) {
      float s = 0.f, dp = 0.f;
      for (int j = 0; j < d; ++j) {
        s = fmaf(qh[(size_t)j * Lq] * a.scale, kh[(size_t)j * Lk + key], s);
        dp = fmaf(gh[(size_t)j * Lq], vh[(size_t)j * Lk + key], dp);
      }
      ds = expf(s - lse) * (dp - delta);
    }
    const int nk = kn - kt < 64 ? kn - kt : 64;
    for (int kk = 0; kk < nk; ++kk) {
      const float dk = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ds), kk));
#pragma unroll
      for (int t = 0; t < SRF_MHA_GEN_T; ++t) {
        const int j = lane + 64 * t;
        if (j < d) acc[t] = fmaf(dk, kh[(size_t)j * Lk + kt + kk], acc[t]);
      }
    }
  }
  float* gq = a.gq + (size_t)b * a.gqs + (size_t)h * d * Lq + ql;
#pragma unroll
  for (int t = 0; t < SRF_MHA_GEN_T; ++t) {
    const int j = lane + 64 * t;
    if (j < d) gq[(size_t)j * Lq] = acc[t] * a.scale;
  }
}

// gK, gV: one wavefront per key, a lane per query for P and dS, a lane per channel for the sums over queries
template <typename... R>
__global__ __launch_bounds__(256) void srf_mha_bwd_dkv_generic_kernel(MhaBwdArgs a, R... r2) {
  const int lane = threadIdx.x & 63;
  const int kl = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int h = blockIdx.y, b = blockIdx.z, d = a.d, Lq = a.Lq, Lk = a.Lk;
  if (kl >= Lk) return;   // (wavefront-uniform; the kernel has no block-wide barrier)
  const int qn = srf_mha_qlen(b, Lq, r2...);   // the example's own query count
  if constexpr (sizeof...(R) > 0) {
    if (kl >= srf_mha_klen(b, Lk, r2...)) {   // a key past the example's end: zeros, nothing read
      float* gzk = a.gk + (size_t)b * a.gks + (size_t)h * d * Lk + kl;
      float* gzv = a.gv + (size_t)b * a.gvs + (size_t)h * d * Lk + kl;
      for (int j = lane; j < d; j += 64) gzk[(size_t)j * Lk] = gzv[(size_t)j * Lk] = 0.f;
      return;
    }
  }
  const float* qh = a.q + (size_t)b * a.qs + (size_t)h * d * Lq;
  const float* gh = a.go + (size_t)b * a.gos + (size_t)h * d * Lq;
  const float* kh = a.k + (size_t)b * a.ks + (size_t)h * d * Lk + kl;
  const float* vh = a.v + (size_t)b * a.vs + (size_t)h * d * Lk + kl;
  const float* lse = a.lse + ((size_t)b * a.H + h) * Lq;
  const float* delta = a.delta + ((size_t)b * a.H + h) * Lq;
  float acck[SRF_MHA_GEN_T], accv[SRF_MHA_GEN_T];
#pragma unroll
  for (int t = 0; t < SRF_MHA_GEN_T; ++t) acck[t] = accv[t] = 0.f;
  for (int qt = 0; qt < qn; qt += 64) {
    const int ql = qt + lane;
    float p = 0.f, ds = 0.f;   // queries >= Lq: 0
    if (ql < qn) {
      float s = 0.f, dp = 0.f;
      for (int j = 0; j < d; ++j) {
        s = fmaf(qh[(size_t)j * Lq + ql] * a.scale, kh[(size_t)j * Lk], s);
        dp = fmaf(gh[(size_t)j * Lq + ql], vh[(size_t)j * Lk], dp);
      }
      p = expf(s - lse[ql]);
      ds = p * (dp - delta[ql]);
    }
    const int nq = qn - qt < 64 ? qn - qt : 64;
    for (int qq = 0; qq < nq; ++qq) {
      const float pq = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p), qq));
      const float dq = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ds), qq));
#pragma unroll
      for (int t = 0; t < SRF_MHA_GEN_T; ++t) {
        const int j = lane + 64 * t;
        if (j < d) {
          accv[t] = fmaf(pq, gh[(size_t)j * Lq + qt + qq], accv[t]);
          acck[t] = fmaf(dq, qh[(size_t)j * Lq + qt + qq], acck[t]);
        }
      }
    }
  }
  float* gk = a.gk + (size_t)b * a.gks + (size_t)h * d * Lk + kl;
  float* gv = a.gv + (size_t)b * a.gvs + (size_t)h * d * Lk + kl;
#pragma unroll
  for (int t = 0; t < SRF_MHA_GEN_T; ++t) {
    const int j = lane + 64 * t;
    if (j < d) {
      gk[(size_t)j * Lk] = acck[t] * a.scale;
      gv[(size_t)j * Lk] = accv[t];
    }
  }
}

// the dispatch test: the forward's (the two directions of one op always run the same family)
extern "C" int srf_mha_attention_bwd_mfma_supported(int d) { return srf_mha_attention_mfma_supported(d); }

// workspace: delta, [Bt, H, Lq] floats
extern "C" size_t srf_mha_attention_bwd_workspace_bytes(int Bt, int H, int d, int Lq, int Lk) {
  (void)d;
  (void)Lk;
  if (Bt <= 0 || H <= 0 || Lq <= 0) return 0;
  return (size_t)Bt * H * Lq * sizeof(float);
}

// (role KV has no <8> instantiation: the caller sends d > 128 to roles V and K)
template <int ROLE, typename... R>
static void srf_mha_bwd_mfma_launch(const MhaBwdArgs& a, int Bt, hipStream_t st, const R&... r2) {
  const int L = ROLE == SRF_MHA_BWD_Q ? a.Lq : a.Lk;
  const dim3 grid((L + 31) / 32, a.H, Bt), block(64);
  if (a.d <= 32) hipLaunchKernelGGL((srf_mha_bwd_mfma_kernel<1, ROLE, R...>), grid, block, 0, st, a, r2...);
  else if (a.d <= 64) hipLaunchKernelGGL((srf_mha_bwd_mfma_kernel<2, ROLE, R...>), grid, block, 0, st, a, r2...);
  else if (a.d <= 128) hipLaunchKernelGGL((srf_mha_bwd_mfma_kernel<4, ROLE, R...>), grid, block, 0, st, a, r2...);
  else if constexpr (ROLE != SRF_MHA_BWD_KV) hipLaunchKernelGGL((srf_mha_bwd_mfma_kernel<8, ROLE, R...>), grid, block, 0, st, a, r2...);
}

static int srf_mha_bwd_check(const MhaBwdArgs& a, const float* o, int Bt) {
  const int H = a.H, d = a.d, Lq = a.Lq, Lk = a.Lk;
  SRF_CHECK_ARG(a.q && a.k && a.v && o && a.lse && a.go, "srf_mha_attention_bwd: null input (q, k, v, o, lse or go)");
  SRF_CHECK_ARG(a.gq && a.gk && a.gv, "srf_mha_attention_bwd: null output (gq, gk or gv)");
  SRF_CHECK_ARG(a.delta, "srf_mha_attention_bwd: workspace is null (srf_mha_attention_bwd_workspace_bytes)");
  SRF_CHECK_ARG(Bt > 0 && H > 0 && d > 0 && Lq > 0 && Lk > 0, "srf_mha_attention_bwd: bad sizes (Bt %d, H %d, d %d, Lq %d, Lk %d)",
                Bt, H, d, Lq, Lk);
  SRF_CHECK_ARG(Bt <= 65535 && H <= 65535, "srf_mha_attention_bwd: batch / heads too large (max 65535 each)");
  SRF_CHECK_ARG((long)H * d * (Lq > Lk ? Lq : Lk) < (1L << 31), "srf_mha_attention_bwd: one example exceeds 2^31 elements");
  const bool mfma = srf_mha_attention_bwd_mfma_supported(d);
  SRF_CHECK_ARG(mfma || d <= 64 * SRF_MHA_GEN_T, "srf_mha_attention_bwd: head dimension d = %d exceeds the generic kernel's %d", d,
                64 * SRF_MHA_GEN_T);
  return SRF_OK;
}

// The launch sequence, once: tables = nothing (the uniform instantiations) or (q_len, k_len), of which delta takes the first.
// A profiler name is a string literal either way (the profiler keeps the pointer): the uniform name, + "_ragged" with tables.
#define SRF_MHA_BWD_NAME(base) (sizeof...(R) ? base "_ragged" : base)
static const SrfFrames& srf_mha_bwd_first(const SrfFrames& qf, const SrfFrames&) { return qf; }
template <typename... Q>
static void srf_mha_bwd_delta_launch(const MhaBwdArgs& a, const float* o, long os, int Bt, hipStream_t st, const Q&... qf) {
  hipLaunchKernelGGL(srf_mha_bwd_delta_kernel<Q...>, dim3((a.Lq + 255) / 256, a.H, Bt), dim3(256), 0, st, o, a.go,
                     const_cast<float*>(a.delta), os, a.gos, a.H, a.d, a.Lq, qf...);   // (delta: the caller's workspace)
}

template <typename... R>
static int srf_mha_bwd_run(const MhaBwdArgs& a, const float* o, long os, int Bt, hipStream_t st, R... tables) {
  const dim3 block(256);
  if constexpr (sizeof...(R) == 0) srf_mha_bwd_delta_launch(a, o, os, Bt, st);
  else srf_mha_bwd_delta_launch(a, o, os, Bt, st, srf_mha_bwd_first(tables...));
  SRF_CHECK_LAUNCH(SRF_MHA_BWD_NAME("mha_attention_bwd_delta"), st);
  if (srf_mha_attention_bwd_mfma_supported(a.d)) {
    srf_mha_bwd_mfma_launch<SRF_MHA_BWD_Q>(a, Bt, st, tables...);
    SRF_CHECK_LAUNCH(SRF_MHA_BWD_NAME("mha_attention_bwd_dq_mfma"), st);
    if (a.d <= 128) {
      srf_mha_bwd_mfma_launch<SRF_MHA_BWD_KV>(a, Bt, st, tables...);
      SRF_CHECK_LAUNCH(SRF_MHA_BWD_NAME("mha_attention_bwd_dkv_mfma"), st);
    } else {   // 2 x 128 accumulator registers would not fit beside the operands: one pass per output
      srf_mha_bwd_mfma_launch<SRF_MHA_BWD_V>(a, Bt, st, tables...);
      SRF_CHECK_LAUNCH(SRF_MHA_BWD_NAME("mha_attention_bwd_dv_mfma"), st);
      srf_mha_bwd_mfma_launch<SRF_MHA_BWD_K>(a, Bt, st, tables...);
      SRF_CHECK_LAUNCH(SRF_MHA_BWD_NAME("mha_attention_bwd_dk_mfma"), st);
    }
    return SRF_OK;
  }
  hipLaunchKernelGGL((srf_mha_bwd_dq_generic_kernel<R...>), dim3((a.Lq + 3) / 4, a.H, Bt), block, 0, st, a, tables...);
  SRF_CHECK_LAUNCH(SRF_MHA_BWD_NAME("mha_attention_bwd_dq_generic"), st);
  hipLaunchKernelGGL((srf_mha_bwd_dkv_generic_kernel<R...>), dim3((a.Lk + 3) / 4, a.H, Bt), block, 0, st, a, tables...);
  SRF_CHECK_LAUNCH(SRF_MHA_BWD_NAME("mha_attention_bwd_dkv_generic"), st);
  return SRF_OK;
}

// The host path of both entries: the uniform checks, (ragged) the two tables, the launches.  o with its own example stride like
// the operands in `a`; lse and the workspace (a.delta) contiguous.  ragged with both tables NULL still runs the ragged kernels.
static int srf_mha_backward(const MhaBwdArgs& a, const float* o, long os, int Bt, bool ragged, const int* q_lengths,
                            const int* k_lengths, hipStream_t st) {
  int rc = srf_mha_bwd_check(a, o, Bt);
  if (rc != SRF_OK) return rc;
  if (!ragged) return srf_mha_bwd_run(a, o, os, Bt, st);
  SrfFrames qf, kf;
  rc = srf_mha_ragged_tables("srf_mha_attention_bwd_ragged", Bt, a.Lq, a.Lk, q_lengths, k_lengths, &qf, &kf);
  if (rc != SRF_OK) return rc;
  return srf_mha_bwd_run(a, o, os, Bt, st, qf, kf);
}

// the contiguous tensors of the public entries: q, o, go, gq [Bt, H d, Lq], k, v, gk, gv [Bt, H d, Lk]
static MhaBwdArgs srf_mha_bwd_contiguous(const float* q, const float* k, const float* v, const float* lse, const float* go, float* gq,
                                         float* gk, float* gv, void* workspace, int H, int d, int Lq, int Lk, float scale) {
  const long sq = (long)H * d * Lq, sk = (long)H * d * Lk;
  return MhaBwdArgs{q, k, v, go, lse, (const float*)workspace, gq, gk, gv, sq, sk, sk, sq, sq, sk, sk, H, d, Lq, Lk, scale};
}

extern "C" int srf_mha_attention_bwd_ragged(const float* q, const float* k, const float* v, const float* o, const float* lse,
                                            const float* go, float* gq, float* gk, float* gv, void* workspace, int Bt, int H, int d,
                                            int Lq, int Lk, const int* q_lengths, const int* k_lengths, float scale, void* stream) {
  SRF_CHECK_ARG(H > 0 && d > 0 && Lq > 0 && Lk > 0, "srf_mha_attention_bwd_ragged: bad sizes (H %d, d %d, Lq %d, Lk %d)", H, d, Lq, Lk);
  const MhaBwdArgs a = srf_mha_bwd_contiguous(q, k, v, lse, go, gq, gk, gv, workspace, H, d, Lq, Lk, scale);
  return srf_mha_backward(a, o, a.qs, Bt, true, q_lengths, k_lengths, (hipStream_t)stream);
}

extern "C" int srf_mha_attention_bwd(const float* q, const float* k, const float* v, const float* o, const float* lse,
                                     const float* go, float* gq, float* gk, float* gv, void* workspace, int Bt, int H, int d, int Lq,
                                     int Lk, float scale, void* stream) {
  SRF_CHECK_ARG(H > 0 && d > 0 && Lq > 0 && Lk > 0, "srf_mha_attention_bwd: bad sizes (H %d, d %d, Lq %d, Lk %d)", H, d, Lq, Lk);
  const MhaBwdArgs a = srf_mha_bwd_contiguous(q, k, v, lse, go, gq, gk, gv, workspace, H, d, Lq, Lk, scale);
  return srf_mha_backward(a, o, a.qs, Bt, false, nullptr, nullptr, (hipStream_t)stream);
}
