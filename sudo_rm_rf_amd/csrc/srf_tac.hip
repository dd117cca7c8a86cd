// K6 -- transform-average-concatenate group communication (TAC.forward up to TAC_norm,
// reference: groupcomm_sudormrf_v2.py:356-377).  Rows of the reference's Linear layers are
// (batch, time, group); here one lane owns one (batch, time) column and walks the G groups, so
// every activation load/store is coalesced along time and every weight is a wave-uniform scalar.
//   z_g  = PReLU(Wi x_g + bi)                      Linear(n -> H) + PReLU          :365-366
//   zbar = mean_g z_g                                                               :369
//   q    = PReLU(Wm zbar + bm)                     Linear(H -> H) + PReLU          :372-373
//   o_g  = PReLU(Wo [z_g ; q] + bo)                Linear(2H -> n) + PReLU         :375-377
// The group mean needs all z_g before any o_g: z_g is recomputed in a second sweep instead of being
// spilled (n*H MACs are cheaper than 4*H bytes of traffic per group and column).  The q-half of Wo
// is group-independent and folded into a per-column vector r once.
// The output is the PRE-norm tensor; {sum,sumsq} per (batch, group) feed TAC_norm (GlobLN).
#include "srf_internal.h"

struct TacArgs {
  const float* x;
  float* q;
  const float *wi, *bi, *ai, *wm, *bm, *am, *wo, *bo, *ao;
  double* out_sums;
  int G, L;
};

template <int NN>
__global__ __launch_bounds__(128) void srf_tac_kernel(TacArgs a) {
  constexpr int HH = 3 * NN;
  const int l = blockIdx.x * 128 + threadIdx.x;
  const long b = blockIdx.y;
  const bool valid = l < a.L;
  const int G = a.G, L = a.L;
  const float ai = a.ai[0], am = a.am[0], ao = a.ao[0];
  const float* xb = a.x + (size_t)b * G * NN * L;
  float* qb = a.q + (size_t)b * G * NN * L;

  float zbar[HH];
#pragma unroll
  for (int j = 0; j < HH; ++j) zbar[j] = 0.f;
  for (int g = 0; g < G; ++g) {
    float xg[NN];
#pragma unroll
    for (int i = 0; i < NN; ++i) xg[i] = valid ? xb[((size_t)g * NN + i) * L + l] : 0.f;
#pragma unroll
    for (int j = 0; j < HH; ++j) {
      float z = 0.f;
#pragma unroll
      for (int i = 0; i < NN; ++i) z = fmaf(a.wi[j * NN + i], xg[i], z);
      z = srf_prelu(z + a.bi[j], ai);
      zbar[j] += z;
    }
  }
  const float fG = (float)G;
#pragma unroll
  for (int j = 0; j < HH; ++j) zbar[j] = zbar[j] / fG;

  // r = bo + Wo[:, H:2H] * PReLU(Wm zbar + bm)
  float r[NN];
#pragma unroll
  for (int i = 0; i < NN; ++i) r[i] = 0.f;
  for (int j = 0; j < HH; ++j) {
    float qj = 0.f;
#pragma unroll
    for (int i = 0; i < HH; ++i) qj = fmaf(a.wm[j * HH + i], zbar[i], qj);
    qj = srf_prelu(qj + a.bm[j], am);
#pragma unroll
    for (int i = 0; i < NN; ++i) r[i] = fmaf(a.wo[i * 2 * HH + HH + j], qj, r[i]);
  }

  for (int g = 0; g < G; ++g) {
    float xg[NN];
#pragma unroll
    for (int i = 0; i < NN; ++i) xg[i] = valid ? xb[((size_t)g * NN + i) * L + l] : 0.f;
    float o[NN];
#pragma unroll
    for (int i = 0; i < NN; ++i) o[i] = 0.f;
    for (int j = 0; j < HH; ++j) {
      float z = 0.f;
#pragma unroll
      for (int i = 0; i < NN; ++i) z = fmaf(a.wi[j * NN + i], xg[i], z);
      z = srf_prelu(z + a.bi[j], ai);
#pragma unroll
      for (int i = 0; i < NN; ++i) o[i] = fmaf(a.wo[i * 2 * HH + j], z, o[i]);
    }
    float s = 0.f, qq = 0.f;
#pragma unroll
    for (int i = 0; i < NN; ++i) {
      const float v = srf_prelu((o[i] + r[i]) + a.bo[i], ao);
      if (valid) {
        qb[((size_t)g * NN + i) * L + l] = v;
        s += v;
        qq = fmaf(v, v, qq);
      }
    }
    if (a.out_sums) {
      const double ds = srf_wave_sum((double)s), dq = srf_wave_sum((double)qq);
      if ((threadIdx.x & 63) == 0) {
        double* dst = srf_stat_slot(a.out_sums, b * G + g, blockIdx.x * 2 + (threadIdx.x >> 6));
        atomicAdd(dst, ds);
        atomicAdd(dst + 1, dq);
      }
    }
  }
}


// ---------------------------------------------------------------------------------------------
// Group-per-lane kernel (G in {2,4,8,16}, n <= 16).  lane = c*G + g: a wavefront holds 64/G time steps
// x all G groups, so the mean over groups is a butterfly of DPP row operations (VALU only, no LDS, no
// barrier), z_g stays in registers between the two sweeps (no recompute), the H x H "mean" layer is
// SPLIT over the G lanes of a column (lane g owns ceil(H/G) hidden units; its slice of Wm / Wo[:, H:]
// comes from an LDS copy staged once per block) and the per-column vector r is all-reduced the same way.
// Per (column, group): n*H + H*n MACs with wave-uniform scalar weights + ~H^2/G with per-lane weights,
// against 3*n*H + (H^2 + H*n)/G... for the column-per-lane kernel above, which also ran at 1.6
// wavefronts per SIMD on the headline shape (B*L = 102400 columns).
// Global accesses are (64/G)*4-byte segments per group row; neighbouring wavefronts of the block use the
// rest of each cache line.
// ---------------------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ float srf_dpp_mov(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, true));
}

// sum over the aligned group of G lanes, result in every lane (bitwise identical across the group)
template <int G>
__device__ __forceinline__ float srf_group_allsum(float v) {
  if (G >= 2) v += srf_dpp_mov<0xB1>(v);    // quad_perm [1,0,3,2]
  if (G >= 4) v += srf_dpp_mov<0x4E>(v);    // quad_perm [2,3,0,1]
  if (G >= 8) v += srf_dpp_mov<0x141>(v);   // row_half_mirror
  if (G >= 16) v += srf_dpp_mov<0x140>(v);  // row_mirror
  return v;
}

// TW time steps per lane (1 | 2): with TW = 2 every matrix-vector FMA is a v_pk_fma_f32 (two fp32 FMAs per lane and
// issue slot, the weight a broadcast SGPR) and the loads / stores are 8-byte; the kernel is VALU-bound (n = 16, G = 16:
// ~2300 VALU instructions per wavefront and time-step group, 150 us per launch at TW = 1), the group all-sums stay per
// component.  TW = 2 needs an even L.
template <int TW>
struct SrfTacVec {
  typedef float type __attribute__((ext_vector_type(TW)));
};
template <int TW, int G>
__device__ __forceinline__ typename SrfTacVec<TW>::type srf_group_allsum_v(typename SrfTacVec<TW>::type v) {
#pragma unroll
  for (int u = 0; u < TW; ++u) v[u] = srf_group_allsum<G>(v[u]);
  return v;
}
// v + s on every component, s wave-uniform (SGPR) resp. per-lane (VGPR).
// NOT written as `v + (vT)(s)`: for TW = 2 hipcc then picks v_pk_add_f32 with op_sel:[0,1] on src1 whenever s sits in the
// high half of a loaded pair, and on gfx950 a packed-fp32 instruction whose SRC1 carries op_sel = 1 returns a wrong LOW
// result in lanes 48..63 while another wavefront's bf16 MFMA executes on the same SIMD (tools/probes/pk_opsel_probe.hip
// reproduces it in isolation; DESIGN.md "Two wrong-result bugs, one cause").  That was the GroupComm two-stream corruption:
// this kernel next to the other stream's split-bf16 GEMM.  Here the scalar is placed in the LOW half of a 64-bit operand
// and broadcast with op_sel_hi (a form the probe shows to be safe); sudo_rm_rf_amd/build.py refuses any object that still
// contains the hazardous form.
template <int TW>
__device__ __forceinline__ typename SrfTacVec<TW>::type srf_add_uniform(typename SrfTacVec<TW>::type v, float s) {
  if constexpr (TW == 2) {
    typename SrfTacVec<TW>::type r;
    const unsigned long long pair = (unsigned long long)__float_as_uint(s);
    asm("v_pk_add_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(r) : "v"(v), "s"(pair));
    return r;
  } else {
    v[0] += s;
    return v;
  }
}
template <int TW>
__device__ __forceinline__ typename SrfTacVec<TW>::type srf_add_lane(typename SrfTacVec<TW>::type v, float s) {
  if constexpr (TW == 2) {
    typename SrfTacVec<TW>::type r;
    const unsigned long long pair = (unsigned long long)__float_as_uint(s);
    asm("v_pk_add_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(r) : "v"(v), "v"(pair));
    return r;
  } else {
    v[0] += s;
    return v;
  }
}
template <int TW>
__device__ __forceinline__ typename SrfTacVec<TW>::type srf_prelu_v(typename SrfTacVec<TW>::type v, float a) {
#pragma unroll
  for (int u = 0; u < TW; ++u) v[u] = srf_prelu(v[u], a);
  return v;
}

template <int NN, int G, int TW>
__global__ __launch_bounds__(256) void srf_tac_lanes_kernel(
    TacArgs a, int tiles_per_block,
    // the weights again as noalias kernel arguments: only then does the compiler know the stores to q
    // cannot clobber them and fetch them with scalar loads (s_load -> SGPR operands) instead of per-lane
    // VMEM loads (measured in the ISA: 431 global_load + 654 v_mov per tile without this)
    const float* __restrict__ wi, const float* __restrict__ bi, const float* __restrict__ wo,
    const float* __restrict__ bo) {
  typedef typename SrfTacVec<TW>::type vT;
  constexpr int HH = 3 * NN, CW = 64 / G, JPL = (HH + G - 1) / G;
  constexpr int PM = HH + 4, PO = NN + 4;   // LDS row pitches (floats), 16-B aligned rows
  __shared__ __attribute__((aligned(16))) float s_wm[HH * PM];   // Wm[j][i]
  __shared__ __attribute__((aligned(16))) float s_wq[HH * PO];   // Wo[i][H + j] stored as [j][i]
  __shared__ __attribute__((aligned(16))) float s_wd[HH * PO];   // Wo[i][j]     stored as [j][i]
  __shared__ float s_bm[HH];
  __shared__ float s_red[4][G][2];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane & (G - 1), c = lane / G;
  const long b = blockIdx.y;
  const int L = a.L;
  for (int e = tid; e < HH * HH; e += 256) s_wm[(e / HH) * PM + (e % HH)] = a.wm[e];
  for (int e = tid; e < HH * NN; e += 256) {
    const int j = e / NN, i = e % NN;
    s_wq[j * PO + i] = a.wo[i * 2 * HH + HH + j];
    s_wd[j * PO + i] = a.wo[i * 2 * HH + j];
  }
  for (int e = tid; e < HH; e += 256) s_bm[e] = a.bm[e];
  __syncthreads();

  const float ai = a.ai[0], am = a.am[0], ao = a.ao[0];
  const float* xb = a.x + ((size_t)b * G + g) * NN * L;
  float* qb = a.q + ((size_t)b * G + g) * NN * L;
  float ss = 0.f, sq = 0.f;

  for (int it = 0; it < tiles_per_block; ++it) {
    const int l0 = ((blockIdx.x * tiles_per_block + it) * 4 + wave) * (CW * TW);   // wave-uniform
    if (l0 >= L) break;
    const int l = l0 + c * TW;
    const bool valid = l < L;              // TW = 2: L is even, both time steps are in range together
    const int lc = valid ? l : L - TW;

    vT x[NN];
#pragma unroll
    for (int i = 0; i < NN; ++i) x[i] = *reinterpret_cast<const vT*>(xb + (size_t)i * L + lc);

    // z_g = PReLU(Wi x_g + bi); zbar = mean_g z_g is consumed on the fly by this lane's JPL rows of Wm
    // (rolled: the fully unrolled form kept z[H] and all H*n output weights alive -- 107 VGPRs + spilled SGPRs at
    // n = 16; the output layer's direct part Wo[:, :H] z accumulates on the fly from the transposed LDS copy)
    vT o[NN], qacc[JPL];
#pragma unroll
    for (int i = 0; i < NN; ++i) o[i] = (vT)(0.f);
#pragma unroll
    for (int t = 0; t < JPL; ++t) qacc[t] = (vT)(0.f);
    const int jrow = g * JPL;
#pragma unroll 2
    for (int j = 0; j < HH; ++j) {
      vT t = (vT)(0.f);
#pragma unroll
      for (int i = 0; i < NN; ++i) t = __builtin_elementwise_fma((vT)(wi[j * NN + i]), x[i], t);
      const vT zj = srf_prelu_v<TW>(srf_add_uniform<TW>(t, bi[j]), ai);
      const vT zb = srf_group_allsum_v<TW, G>(zj) * (vT)(1.f / (float)G);
#pragma unroll
      for (int t2 = 0; t2 < JPL; ++t2) {
        const int jr = jrow + t2 < HH ? jrow + t2 : HH - 1;
        qacc[t2] = __builtin_elementwise_fma((vT)(s_wm[jr * PM + j]), zb, qacc[t2]);
      }
      const float* wd = s_wd + j * PO;
#pragma unroll
      for (int i = 0; i < NN; ++i) o[i] = __builtin_elementwise_fma((vT)(wd[i]), zj, o[i]);
    }

    // this lane's slice of q = PReLU(Wm zbar + bm) and of r = Wo[:, H:2H] q
    vT r[NN];
#pragma unroll
    for (int i = 0; i < NN; ++i) r[i] = (vT)(0.f);
#pragma unroll
    for (int t = 0; t < JPL; ++t) {
      const bool jm = jrow + t < HH;
      const int jc = jm ? jrow + t : HH - 1;
      vT qv = srf_prelu_v<TW>(srf_add_lane<TW>(qacc[t], s_bm[jc]), am);
      qv = jm ? qv : (vT)(0.f);
      const float* wq = s_wq + jc * PO;
#pragma unroll
      for (int i = 0; i < NN; ++i) r[i] = __builtin_elementwise_fma((vT)(wq[i]), qv, r[i]);
    }
#pragma unroll
    for (int i = 0; i < NN; ++i) r[i] = srf_group_allsum_v<TW, G>(r[i]);

    // o_g = PReLU(Wo[:, :H] z_g + r + bo)
#pragma unroll
    for (int i = 0; i < NN; ++i) {
      const vT v = srf_prelu_v<TW>(srf_add_uniform<TW>(o[i] + r[i], bo[i]), ao);
      if (valid) {
        *reinterpret_cast<vT*>(qb + (size_t)i * L + l) = v;
#pragma unroll
        for (int u = 0; u < TW; ++u) {
          ss += v[u];
          sq = fmaf(v[u], v[u], sq);
        }
      }
    }
  }

  if (a.out_sums) {
    // lanes that share g: c = 0..CW-1 -> xor over the lane bits above log2(G)
#pragma unroll
    for (int o = G; o < 64; o <<= 1) {
      ss += __shfl_xor(ss, o, 64);
      sq += __shfl_xor(sq, o, 64);
    }
    if (lane < G) {
      s_red[wave][lane][0] = ss;
      s_red[wave][lane][1] = sq;
    }
    __syncthreads();
    if (tid < G) {
      double ds = 0.0, dq = 0.0;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        ds += (double)s_red[w][tid][0];
        dq += (double)s_red[w][tid][1];
      }
      double* dst = srf_stat_slot(a.out_sums, b * G + tid, blockIdx.x);
      atomicAdd(dst, ds);
      atomicAdd(dst + 1, dq);
    }
  }
}

template <int NN, int G>
static void srf_tac_lanes_go(const TacArgs& a, int Bt, hipStream_t st) {
  constexpr int CW = 64 / G;
  const int TW = (a.L % 2 == 0 && !srf_dbg(SRF_DBG_TAC_ONE_STEP_PER_LANE)) ? 2 : 1;   // debug flag 1024: one time step per lane
  const int tiles = (a.L + 4 * CW * TW - 1) / (4 * CW * TW);   // block-tiles (4 wavefronts x CW*TW columns) per row
  // enough blocks to keep >= ~8 per CU in flight, otherwise fold tiles into one block (fewer atomics,
  // weight staging amortised)
  int tpb = 1;
  while (tpb < 8 && (long)Bt * (tiles / (tpb * 2)) >= 8 * 256) tpb *= 2;
  if (srf_dbg(SRF_DBG_TAC_LANES_4TILES)) tpb = 4;      // (tests: the several-tiles-per-block path at small sizes)
  dim3 grid((tiles + tpb - 1) / tpb, Bt), block(256);
  if (TW == 2)
    hipLaunchKernelGGL((srf_tac_lanes_kernel<NN, G, 2>), grid, block, 0, st, a, tpb, a.wi, a.bi, a.wo, a.bo);
  else
    hipLaunchKernelGGL((srf_tac_lanes_kernel<NN, G, 1>), grid, block, 0, st, a, tpb, a.wi, a.bi, a.wo, a.bo);
}

template <int NN>
static bool srf_tac_lanes_g(const TacArgs& a, int Bt, hipStream_t st) {
  switch (a.G) {
    case 2: srf_tac_lanes_go<NN, 2>(a, Bt, st); return true;
    case 4: srf_tac_lanes_go<NN, 4>(a, Bt, st); return true;
    case 8: srf_tac_lanes_go<NN, 8>(a, Bt, st); return true;
    case 16: srf_tac_lanes_go<NN, 16>(a, Bt, st); return true;
    default: return false;
  }
}

static bool srf_tac_lanes_launch(const TacArgs& a, int n, int Bt, hipStream_t st) {
  switch (n) {
    case 2: return srf_tac_lanes_g<2>(a, Bt, st);
    case 4: return srf_tac_lanes_g<4>(a, Bt, st);
    case 8: return srf_tac_lanes_g<8>(a, Bt, st);
    case 16: return srf_tac_lanes_g<16>(a, Bt, st);
    default: return false;
  }
}

// =============================================================================================================================
// MFMA form (round 4) for n = 16, H = 48, G = 16 -- the shape of BASELINE's GroupComm configuration (cfg 3).
// The lane-per-(time step, group) kernel above is VALU-bound (134 us per launch at cfg 3: ~2 300 VALU instructions per wavefront
// and 8 columns).  Here the three Linear layers are small GEMMs on the matrix pipe: a wavefront owns 32 time steps of one example
// and walks the 16 groups,
//   z_g  [48 x 32] = Wi [48 x 16] x_g [16 x 32]                     2 M-blocks x 1 k-step
//   q    [48 x 32] = Wm [48 x 48] zbar [48 x 32],  r = Wo[:, H:] q    (2 + 1) M-blocks x 3 k-steps, once per tile
//   o_g  [16 x 32] = Wo[:, :H] [16 x 48] z_g [48 x 32] + r            1 M-block x 3 k-steps       (second sweep: z_g recomputed)
// with fp32 operands split into TWO FP16 PARTS (hi = fp16(v), lo = fp16(v - hi): 22 mantissa bits, the training forward's scheme,
// srf_pwconv_x3w.hip NP = 4) and three v_mfma_f32_32x32x16_f16 per product block, fp32 accumulate -- the fp32 VALU kernel's
// accuracy class (test_tac's bar is unchanged).  Weights are stored times 2^4 so that their lo parts stay normal in fp16; the
// biases ride in as the MFMAs' C operand at the matching scale and PReLU commutes with the positive scale, so every rescale is
// one exact multiply at the end of a chain.  What the MFMA hands back (C layout: lane = column, registers = rows (r & 3) +
// 8 (r >> 2) + 4 (lane >> 5)) becomes the next GEMM's B operand (lane = column, 8 consecutive k) with four
// v_permlane32_swap_b32 per 8 rows -- no LDS round trip.  The A fragments of Wm / Wo live in LDS (24 KB, built once per block),
// Wi's in registers.  One 32-column tile per wavefront, four per block: the hardware balances 3 200 tiles.
// RAGGED (srf_tac_ragged; FR = one SrfFrames): L stays the row stride, example b is frames[b] columns long.  TAC is pointwise in
// time -- the group mean is per time step and the MFMAs' B columns are independent -- so nothing is masked on load (x past the
// end may hold anything, NaN included); q carries GlobLN statistics, so columns >= frames[b] are selected to exact 0 before
// the store and the sums, per column (a tile may straddle the end).  A tile wholly past the end stores its zeros without a
// load of x or an MFMA -- after the block's barrier.
typedef _Float16 tac_f16x8 __attribute__((ext_vector_type(8)));
typedef float tac_f32x16 __attribute__((ext_vector_type(16)));
constexpr float TAC_WS = 16.f;

__device__ __forceinline__ void tac_split8(const float (&v)[8], tac_f16x8& hi, tac_f16x8& lo) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const _Float16 h = (_Float16)v[j];
    hi[j] = h;
    lo[j] = (_Float16)(v[j] - (float)h);
  }
}
// c + A B with A = ah + al, B = bh + bl (lo * lo dropped), smallest terms first
__device__ __forceinline__ tac_f32x16 tac_mma3(const tac_f16x8& ah, const tac_f16x8& al, const tac_f16x8& bh, const tac_f16x8& bl,
                                               tac_f32x16 c) {
  c = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, c, 0, 0, 0);
  return c;
}
// 8 C-layout registers c[0..7] of one 16-row group (c[0..3]: rows e | 4 + e of the lower 8, c[4..7]: of the upper 8, by lane
// half) -> this lane's B-operand values: 8 consecutive rows 8 (lane >> 5) + 0..7 of its column
__device__ __forceinline__ void tac_c_to_b(const float (&c)[8], float (&v)[8]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(c[e]), __float_as_uint(c[4 + e]), false, false);
    v[e] = __uint_as_float(r[0]);
    v[4 + e] = __uint_as_float(r[1]);
  }
}

template <typename... FR>
__global__ __launch_bounds__(256) void srf_tac_mfma_kernel(TacArgs a, int tiles_per_row, int total_tiles, FR... fr) {
  constexpr int NN = 16, HH = 48, G = 16;
  constexpr bool RAGGED = sizeof...(FR) != 0;
  __shared__ tac_f16x8 s_frag[24][64];     // A fragments {hi, lo}: Wm (2 M-blocks x 3 k-steps), Wo[:, H:] (3), Wo[:, :H] (3)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (uniform for the compiler: buffer descriptors in SGPRs)
  const int t = lane & 31, h = lane >> 5;
  const int L = a.L;
  // ---- A fragments: element (lane, e) = W[row = 32 blk + (lane & 31)][k = 16 s + 8 (lane >> 5) + e] x 2^4, zero beyond the
  // matrix.  8 consecutive k = two float4 loads (rows are 192 / 384 bytes long: 16-byte aligned when the tensor is)
  __shared__ float s_bias[HH + HH + NN];   // bi | bm | bo
  for (int e = tid; e < HH + HH + NN; e += 256) s_bias[e] = e < HH ? a.bi[e] : (e < 2 * HH ? a.bm[e - HH] : a.bo[e - 2 * HH]);
  auto row8 = [&](const float* p, bool ok, float (&v)[8]) __attribute__((always_inline)) {
    float4 lo4 = make_float4(0.f, 0.f, 0.f, 0.f), hi4 = lo4;
    if (ok) {
      if ((((size_t)p) & 15) == 0) {
        lo4 = reinterpret_cast<const float4*>(p)[0];
        hi4 = reinterpret_cast<const float4*>(p)[1];
      } else {
        lo4 = make_float4(p[0], p[1], p[2], p[3]);
        hi4 = make_float4(p[4], p[5], p[6], p[7]);
      }
    }
    v[0] = lo4.x * TAC_WS; v[1] = lo4.y * TAC_WS; v[2] = lo4.z * TAC_WS; v[3] = lo4.w * TAC_WS;
    v[4] = hi4.x * TAC_WS; v[5] = hi4.y * TAC_WS; v[6] = hi4.z * TAC_WS; v[7] = hi4.w * TAC_WS;
  };
  for (int id = tid; id < 12 * 64; id += 256) {
    const int f = id >> 6, ln = id & 63, row32 = ln & 31, kh = ln >> 5;
    float v[8];
    if (f < 6) {                         // Wm [48][48]: f = blk * 3 + s
      const int blk = f / 3, sidx = f - blk * 3, j = blk * 32 + row32;
      row8(a.wm + (j < HH ? j : 0) * HH + 16 * sidx + 8 * kh, j < HH, v);
    } else {                             // Wo [16][96]: f - 6 = half * 3 + s, half 0 = the q columns (H ..), 1 = the z columns
      const int half = (f - 6) / 3, sidx = (f - 6) - half * 3;
      row8(a.wo + (row32 < NN ? row32 : 0) * 2 * HH + (half == 0 ? HH : 0) + 16 * sidx + 8 * kh, row32 < NN, v);
    }
    tac_f16x8 hi, lo;
    tac_split8(v, hi, lo);
    s_frag[2 * f][ln] = hi;
    s_frag[2 * f + 1][ln] = lo;
  }
  tac_f16x8 wi_h[2], wi_l[2];            // Wi [48][16]: 2 M-blocks, one k-step
#pragma unroll
  for (int blk = 0; blk < 2; ++blk) {
    float v[8];
    const int j = blk * 32 + t;
    row8(a.wi + (j < HH ? j : 0) * NN + 8 * h, j < HH, v);
    tac_split8(v, wi_h[blk], wi_l[blk]);
  }
  __syncthreads();
  tac_f32x16 bi16[2];                    // 2^4 bi in the C layout (the first MFMA's C operand)
#pragma unroll
  for (int blk = 0; blk < 2; ++blk)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = blk * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      bi16[blk][r] = row < HH ? s_bias[row] * TAC_WS : 0.f;
    }
  const float ai = a.ai[0], am = a.am[0], ao = a.ao[0];
  // ONE tile per wavefront (a loop over tiles keeps ~80 more registers alive across iterations: 296 instead of 216, one
  // wavefront per SIMD instead of two, 134 instead of 105 us)
  const int tile = blockIdx.x * 4 + wave;
  if (tile >= total_tiles) return;       // (after the barrier; wave-uniform)
  const int b = tile / tiles_per_row, l0 = (tile - b * tiles_per_row) * 32;
  const int col = l0 + t;
  const bool valid = col < L;
  __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x) + (size_t)b * G * NN * L, 0, G * NN * L * 4, 0x00020000);
  __amdgpu_buffer_rsrc_t qrs = __builtin_amdgcn_make_buffer_rsrc(a.q + (size_t)b * G * NN * L, 0, G * NN * L * 4, 0x00020000);
  const int x_vo = valid ? (8 * h * L + col) * 4 : 0x7ffffff0;     // (out of range: the load returns 0, the store is dropped)
  const int q_vo = valid ? (4 * h * L + col) * 4 : 0x7ffffff0;
  int Lb = L;                      // (RAGGED: the example's own length; a column at or past it is stored as 0)
  if constexpr (RAGGED) {
    Lb = srf_frames_of(b, fr...);
    if (l0 >= Lb) {                // wave-uniform: the whole tile lies past the example's end
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int r = 0; r < 8; ++r)
          __builtin_amdgcn_raw_buffer_store_b32(0u, qrs, q_vo, (g * NN + (r & 3) + 8 * (r >> 2)) * L * 4, 0);
      return;
    }
  }

  // x_g's B fragment: 8 dword loads (rows 8 h + e of group g at this lane's column), requested one group ahead
  struct XRaw {
    float v[8];
  };
  auto issue_x = [&](int g, XRaw& r) __attribute__((always_inline)) {
#pragma unroll
    for (int e = 0; e < 8; ++e) r.v[e] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(xrs, x_vo, (g * NN + e) * L * 4, 0));
  };
  // (no fp16 range guard -- round 5, ADVICE r4: beyond fp16's range the parts become inf / NaN and poison the output, as a
  // NaN input does; rounds 3-4 clamped to +-6e4, which turned NaN into -6e4 and overflow into a plausible wrong number.  The
  // residual stream of every model we have stays below 1e3; debug flag 1 << 22 selects the fp32 VALU kernels, which have fp32's range)
  auto clamp8 = [&](float (&v)[8]) __attribute__((always_inline)) { (void)v; };
  // 2^4 PReLU(Wi x + bi) of group g in the C layout: zA rows 0..31, zB rows 32..47 (registers 0..7)
  auto z_of = [&](const tac_f16x8& xh, const tac_f16x8& xl, tac_f32x16& zA, tac_f32x16& zB) __attribute__((always_inline)) {
    zA = tac_mma3(wi_h[0], wi_l[0], xh, xl, bi16[0]);
    zB = tac_mma3(wi_h[1], wi_l[1], xh, xl, bi16[1]);
#pragma unroll
    for (int r = 0; r < 16; ++r) zA[r] = srf_prelu(zA[r], ai);
#pragma unroll
    for (int r = 0; r < 8; ++r) zB[r] = srf_prelu(zB[r], ai);
  };
  // the three k-steps' B fragments of a [48 x 32] C-layout pair (A: rows 0..31, B: rows 32..47), values times `scale`
  auto frags_of = [&](const tac_f32x16& cA, const tac_f32x16& cB, float scale, tac_f16x8 (&fh)[3], tac_f16x8 (&fl)[3])
      __attribute__((always_inline)) {
#pragma unroll
    for (int sidx = 0; sidx < 3; ++sidx) {
      float c8[8], v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) c8[e] = (sidx < 2 ? cA[8 * sidx + e] : cB[e]) * scale;
      tac_c_to_b(c8, v);
      tac_split8(v, fh[sidx], fl[sidx]);
    }
  };

  // ---- sweep 1: zsum = sum_g 2^4 z_g
  tac_f32x16 zsA, zsB;
#pragma unroll
  for (int r = 0; r < 16; ++r) zsA[r] = zsB[r] = 0.f;
  XRaw xa, xb;
  issue_x(0, xa);
  auto sweep1 = [&](XRaw& cur, XRaw& nxt, int g) __attribute__((always_inline)) {
    issue_x(g + 1 < G ? g + 1 : 0, nxt);             // (the last one requests group 0 again: sweep 2 starts with it)
    tac_f16x8 xh, xl;
    clamp8(cur.v);
    tac_split8(cur.v, xh, xl);
    tac_f32x16 zA, zB;
    z_of(xh, xl, zA, zB);
#pragma unroll
    for (int r = 0; r < 16; ++r) zsA[r] += zA[r];
#pragma unroll
    for (int r = 0; r < 8; ++r) zsB[r] += zB[r];
  };
  for (int g = 0; g < G; g += 2) {
    sweep1(xa, xb, g);
    sweep1(xb, xa, g + 1);
  }
  // ---- q = PReLU(Wm zbar + bm), r = Wo[:, H:] q + bo.  B fragments of 2^4 zbar = zsum / G; Wm is stored times 2^4: the
  // accumulators hold 2^8 (Wm zbar + bm)
  tac_f32x16 r256;
  {
    tac_f16x8 fh[3], fl[3];
    frags_of(zsA, zsB, 1.f / (float)G, fh, fl);
    tac_f32x16 qA, qB;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
      qA[r] = s_bias[HH + row] * (TAC_WS * TAC_WS);
      qB[r] = row < HH - 32 ? s_bias[HH + 32 + row] * (TAC_WS * TAC_WS) : 0.f;
    }
#pragma unroll
    for (int sidx = 0; sidx < 3; ++sidx) {
      qA = tac_mma3(s_frag[2 * sidx][lane], s_frag[2 * sidx + 1][lane], fh[sidx], fl[sidx], qA);
      qB = tac_mma3(s_frag[2 * (3 + sidx)][lane], s_frag[2 * (3 + sidx) + 1][lane], fh[sidx], fl[sidx], qB);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      qA[r] = srf_prelu(qA[r], am);
      qB[r] = srf_prelu(qB[r], am);
    }
    frags_of(qA, qB, 1.f / TAC_WS, fh, fl);          // 2^4 q
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
      r256[r] = row < NN ? s_bias[2 * HH + row] * (TAC_WS * TAC_WS) : 0.f;
    }
#pragma unroll
    for (int sidx = 0; sidx < 3; ++sidx)
      r256 = tac_mma3(s_frag[2 * (6 + sidx)][lane], s_frag[2 * (6 + sidx) + 1][lane], fh[sidx], fl[sidx], r256);
  }
  // ---- sweep 2: o_g = PReLU(Wo[:, :H] z_g + r + bo)
  auto sweep2 = [&](XRaw& cur, XRaw& nxt, int g) __attribute__((always_inline)) {
    if (g + 1 < G) issue_x(g + 1, nxt);
    tac_f16x8 xh, xl;
    clamp8(cur.v);
    tac_split8(cur.v, xh, xl);
    tac_f32x16 zA, zB;
    z_of(xh, xl, zA, zB);
    tac_f16x8 fh[3], fl[3];
    frags_of(zA, zB, 1.f, fh, fl);                   // 2^4 z_g
    tac_f32x16 o = r256;
#pragma unroll
    for (int sidx = 0; sidx < 3; ++sidx)
      o = tac_mma3(s_frag[2 * (9 + sidx)][lane], s_frag[2 * (9 + sidx) + 1][lane], fh[sidx], fl[sidx], o);
    float ss = 0.f, sq = 0.f;
#pragma unroll
    for (int r = 0; r < 8; ++r) {                    // rows (r & 3) + 8 (r >> 2) + 4 h = 0 .. 15
      const float v = srf_prelu(o[r] * (1.f / (TAC_WS * TAC_WS)), ao);
      if constexpr (!RAGGED) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), qrs, q_vo, (g * NN + (r & 3) + 8 * (r >> 2)) * L * 4, 0);
      const float vz = (RAGGED ? col < Lb : valid) ? v : 0.f;
      if constexpr (RAGGED) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(vz), qrs, q_vo, (g * NN + (r & 3) + 8 * (r >> 2)) * L * 4, 0);
      ss += vz;
      sq = fmaf(vz, vz, sq);
    }
    if (a.out_sums) {      // (64 fp32 partials of 8 values each, summed in fp32 like the VALU kernel's lane sums, then fp64 buckets)
      const float fs = srf_dpp_wave_sum(ss), fq = srf_dpp_wave_sum(sq);
      if (lane == 63) {
        double* dst = srf_stat_slot(a.out_sums, (long)b * G + g, tile);
        atomicAdd(dst, (double)fs);
        atomicAdd(dst + 1, (double)fq);
      }
    }
  };
  for (int g = 0; g < G; g += 2) {
    sweep2(xa, xb, g);
    sweep2(xb, xa, g + 1);
  }
}

extern "C" int srf_tac(const float* x, float* q, const float* const* params, int Bt, int G, int n, int H,
                       int L, double* out_sums, void* stream) {
  SRF_CHECK_ARG(x && q && params, "srf_tac: null pointer");
  SRF_CHECK_ARG(Bt > 0 && G > 0 && n > 0 && L > 0 && Bt <= 65535, "srf_tac: bad sizes");
  SRF_CHECK_ARG(H == 3 * n, "srf_tac: hidden size must be 3*n (got n=%d H=%d)", n, H);
  for (int i = 0; i < 9; ++i) SRF_CHECK_ARG(params[i] != nullptr, "srf_tac: null parameter %d", i);
  TacArgs a;
  a.x = x;
  a.q = q;
  a.wi = params[0];
  a.bi = params[1];
  a.ai = params[2];
  a.wm = params[3];
  a.bm = params[4];
  a.am = params[5];
  a.wo = params[6];
  a.bo = params[7];
  a.ao = params[8];
  a.out_sums = out_sums;
  a.G = G;
  a.L = L;
  dim3 grid((L + 127) / 128, Bt), block(128);
  hipStream_t st = (hipStream_t)stream;
  // debug flags 1 << 22 / 24 / 25 / 26, 1024: the VALU kernels (the MFMA form serves n = 16, G = 16; 1 << 22 = just not the MFMA form)
  // (the MFMA form moves x and q with 16-byte buffer accesses: float-aligned bases take the VALU kernels)
  if (srf_kernel_mode() != 1 && n == 16 && G == 16 && !srf_dbg(SRF_DBG_TAC_ONE_STEP_PER_LANE | SRF_DBG_TAC_VALU | SRF_DBG_TAC_GENERIC | SRF_DBG_TAC_LANES_4TILES) &&
      (long)G * n * L * 4 < (1L << 31) && srf_aligned16(x) && srf_aligned16(q)) {
    const int tiles_per_row = (L + 31) / 32;
    const long total = (long)Bt * tiles_per_row;
    if (total < (1L << 30)) {
      const long blocks = (total + 3) / 4;
      hipLaunchKernelGGL(srf_tac_mfma_kernel<>, dim3((unsigned)blocks), dim3(256), 0, st, a, tiles_per_row, (int)total);
      SRF_CHECK_LAUNCH("tac_mfma", st);
      return SRF_OK;
    }
  }
  if (srf_kernel_mode() != 1 && !srf_dbg(SRF_DBG_TAC_GENERIC) && srf_tac_lanes_launch(a, n, Bt, st)) {
    SRF_CHECK_LAUNCH("tac", st);
    return SRF_OK;
  }
  switch (n) {
    case 2: hipLaunchKernelGGL(srf_tac_kernel<2>, grid, block, 0, st, a); break;
    case 4: hipLaunchKernelGGL(srf_tac_kernel<4>, grid, block, 0, st, a); break;
    case 8: hipLaunchKernelGGL(srf_tac_kernel<8>, grid, block, 0, st, a); break;
    case 16: hipLaunchKernelGGL(srf_tac_kernel<16>, grid, block, 0, st, a); break;
    case 32: hipLaunchKernelGGL(srf_tac_kernel<32>, grid, block, 0, st, a); break;
    default:
      srf_set_error("srf_tac: channels per group n=%d unsupported (2,4,8,16,32)", n);
      return SRF_EINVAL;
  }
  SRF_CHECK_LAUNCH("tac", st);
  return SRF_OK;
}

// The ragged form: the MFMA kernel only (n = 16, G = 16), everything else is refused before any launch.
extern "C" int srf_tac_ragged(const float* x, float* q, const float* const* params, int Bt, int G, int n, int H, int L,
                              double* out_sums, const int* frames, void* stream) {
  SrfFrames fr;
  int rc = srf_frames_table("srf_tac_ragged", frames, Bt, L, &fr);
  if (rc) return rc;
  SRF_CHECK_ARG(x && q && params, "srf_tac_ragged: null pointer");
  SRF_CHECK_ARG(G > 0 && n > 0 && L > 0, "srf_tac_ragged: bad sizes");
  SRF_CHECK_ARG(n == 16 && G == 16 && H == 48,
                "srf_tac_ragged: only the MFMA kernel has a ragged form (n = 16, H = 48, G = 16; got n=%d H=%d G=%d)", n, H, G);
  for (int i = 0; i < 9; ++i) SRF_CHECK_ARG(params[i] != nullptr, "srf_tac_ragged: null parameter %d", i);
  SRF_CHECK_ARG(srf_kernel_mode() != 1 && !srf_dbg(SRF_DBG_TAC_ONE_STEP_PER_LANE | SRF_DBG_TAC_VALU | SRF_DBG_TAC_GENERIC | SRF_DBG_TAC_LANES_4TILES),
                "srf_tac_ragged: the MFMA kernel is switched off (kernel mode %d / debug flags)", srf_kernel_mode());
  SRF_CHECK_ARG((long)G * n * L * 4 < (1L << 31), "srf_tac_ragged: L=%d beyond the reach of the kernel's 32-bit offsets", L);
  SRF_CHECK_ALIGNED16("srf_tac_ragged", {"x", x}, {"q", q});
  TacArgs a;
  a.x = x;
  a.q = q;
  a.wi = params[0];
  a.bi = params[1];
  a.ai = params[2];
  a.wm = params[3];
  a.bm = params[4];
  a.am = params[5];
  a.wo = params[6];
  a.bo = params[7];
  a.ao = params[8];
  a.out_sums = out_sums;
  a.G = G;
  a.L = L;
  const int tiles_per_row = (L + 31) / 32;
  const long total = (long)Bt * tiles_per_row;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL((srf_tac_mfma_kernel<SrfFrames>), dim3((unsigned)((total + 3) / 4)), dim3(256), 0, st, a, tiles_per_row,
                     (int)total, fr);
  SRF_CHECK_LAUNCH("tac_mfma_ragged", st);
  return SRF_OK;
}

__global__ void srf_tac_slope_add_kernel(const float* __restrict__ d, float* gi, float* gm, float* go) {
  if (threadIdx.x == 0) {
    gi[0] += d[0];
    gm[0] += d[1];
    go[0] += d[2];
  }
}

// =============================================================================================
// TAC backward (training step; reference autograd over groupcomm_sudormrf_v2.py:356-377).
// Same lane = (time step, group) mapping as the forward: the whole MLP is recomputed per lane, the three
// group reductions of the backward (sum_g g_po for the q path, the hidden-unit split of Wm^T g_pq, and its
// all-reduce) are DPP butterflies again.  The kernel writes the input gradient of the MLP path and the operand
// tensors of the four weight-gradient GEMMs (srf_pw_wgrad: dWi = g_pz x^T, dWo[:, :H] = g_po z^T,
// dWo[:, H:] = (sum_g g_po) q^T, dWm = g_pq zbar^T; their bias sums come with them), and accumulates the three
// PReLU slope gradients.
// =============================================================================================
struct TacBwdArgs {
  const float* x;     // [Bt,G,n,L]
  const float* go;    // [Bt,G,n,L] gradient w.r.t. the MLP output (pre TAC_norm)
  const float *wm, *bm, *ai, *am, *ao;
  float* gx;          // [Bt,G,n,L]
  float *Z, *GPZ;     // [Bt*G,H,L]
  float* GPO;         // [Bt*G,n,L]
  float* GS;          // [Bt,n,L]
  float *Q, *GPQ, *ZB;   // [Bt,H,L]
  float* dslope;      // 3 accumulators {ai, am, ao} (device, atomically added)
  int G, L;
};

// Register budget: the first version kept pz[H], gz[H] and every weight of the fully unrolled loops alive (256 VGPRs,
// 630 spilled SGPRs, ONE wavefront per SIMD at n = 16: 1.47 ms per launch on cfg 3).  Now two rolled loops over the
// hidden units with O(n) live values each: loop A computes pz_j -> z_j, zbar_j and accumulates the output layer and
// this lane's slice of the q path on the fly; loop B RECOMPUTES pz_j from x (n FMAs -- cheaper than keeping or
// re-reading it) and folds g_z_j straight into g_pz_j and g_x.  Wo is staged in LDS transposed ([j][i], both halves) so
// a hidden unit's n weights are one broadcast 16-byte-vector read; Wi rows are scalar loads.
template <int NN, int G>
__global__ __launch_bounds__(256) void srf_tac_bwd_lanes_kernel(TacBwdArgs a, const float* __restrict__ wi,
                                                                const float* __restrict__ bi,
                                                                const float* __restrict__ wo,
                                                                const float* __restrict__ bo,
                                                                const float* __restrict__ wi2,
                                                                const float* __restrict__ bi2) {
  constexpr int HH = 3 * NN, CW = 64 / G, JPL = (HH + G - 1) / G;
  constexpr int PM = HH + 4, PO = NN + 4;
  __shared__ __attribute__((aligned(16))) float s_wm[HH * PM];   // Wm[j][i]
  __shared__ __attribute__((aligned(16))) float s_wq[HH * PO];   // Wo[i][H + j] stored as [j][i]
  __shared__ __attribute__((aligned(16))) float s_wd[HH * PO];   // Wo[i][j]     stored as [j][i]
  __shared__ float s_bm[HH];
  __shared__ float s_red[4][3];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane & (G - 1), c = lane / G;
  const long b = blockIdx.y;
  const int L = a.L;
  for (int e = tid; e < HH * HH; e += 256) s_wm[(e / HH) * PM + (e % HH)] = a.wm[e];
  for (int e = tid; e < HH * NN; e += 256) {
    const int j = e / NN, i = e % NN;
    s_wq[j * PO + i] = wo[i * 2 * HH + HH + j];
    s_wd[j * PO + i] = wo[i * 2 * HH + j];
  }
  for (int e = tid; e < HH; e += 256) s_bm[e] = a.bm[e];
  __syncthreads();
  const float ai = a.ai[0], am = a.am[0], ao = a.ao[0];
  const size_t rowg = (size_t)b * G + g;   // folded (batch, group) row
  float d_ai = 0.f, d_am = 0.f, d_ao = 0.f;

  const int l0 = (blockIdx.x * 4 + wave) * CW;   // wave-uniform
  if (l0 < L) {
    const int l = l0 + c;
    const bool valid = l < L;
    const int lc = valid ? l : L - 1;
    const int jrow = g * JPL;

    float x[NN];
#pragma unroll
    for (int i = 0; i < NN; ++i) x[i] = a.x[(rowg * NN + i) * L + lc];

    // ---- loop A: pz_j, z_j, zbar_j; output-layer pre-activation and this lane's slice of pq accumulate on the fly
    float po[NN], qacc[JPL];
#pragma unroll
    for (int i = 0; i < NN; ++i) po[i] = 0.f;
#pragma unroll
    for (int t = 0; t < JPL; ++t) qacc[t] = 0.f;
#pragma unroll 2
    for (int j = 0; j < HH; ++j) {
      float t = 0.f;
#pragma unroll
      for (int i = 0; i < NN; ++i) t = fmaf(wi[j * NN + i], x[i], t);
      const float zj = srf_prelu(t + bi[j], ai);
      const float zb = srf_group_allsum<G>(zj) * (1.f / (float)G);
      if (valid) {
        a.Z[(rowg * HH + j) * L + l] = zj;
        if (j / JPL == g) a.ZB[((size_t)b * HH + j) * L + l] = zb;
      }
#pragma unroll
      for (int t2 = 0; t2 < JPL; ++t2) {
        const int jr = jrow + t2 < HH ? jrow + t2 : HH - 1;
        qacc[t2] = fmaf(s_wm[jr * PM + j], zb, qacc[t2]);
      }
      const float* wd = s_wd + j * PO;
#pragma unroll
      for (int i = 0; i < NN; ++i) po[i] = fmaf(wd[i], zj, po[i]);
    }
    float pq[JPL], r[NN];
#pragma unroll
    for (int i = 0; i < NN; ++i) r[i] = 0.f;
#pragma unroll
    for (int t = 0; t < JPL; ++t) {
      const bool jm = jrow + t < HH;
      const int jc = jm ? jrow + t : HH - 1;
      pq[t] = qacc[t] + s_bm[jc];
      float qv = srf_prelu(pq[t], am);
      qv = jm ? qv : 0.f;
      if (valid && jm) a.Q[((size_t)b * HH + jc) * L + l] = qv;
      const float* wq = s_wq + jc * PO;
#pragma unroll
      for (int i = 0; i < NN; ++i) r[i] = fmaf(wq[i], qv, r[i]);
    }

    // ---- output layer backward
    float gpo[NN], gs[NN];
#pragma unroll
    for (int i = 0; i < NN; ++i) {
      const float pv = (po[i] + srf_group_allsum<G>(r[i])) + bo[i];
      const float gv = valid ? a.go[(rowg * NN + i) * L + lc] : 0.f;
      gpo[i] = pv > 0.f ? gv : gv * ao;
      if (pv < 0.f) d_ao = fmaf(gv, pv, d_ao);
      if (valid) a.GPO[(rowg * NN + i) * L + l] = gpo[i];
      gs[i] = srf_group_allsum<G>(gpo[i]);
      if (valid && g == 0) a.GS[((size_t)b * NN + i) * L + l] = gs[i];
    }
    // this lane's slice of g_pq = PReLU'(pq) * (Wo[:, H:]^T sum_g g_po)
    float gpq[JPL];
#pragma unroll
    for (int t = 0; t < JPL; ++t) {
      const bool jm = jrow + t < HH;
      const int jc = jm ? jrow + t : HH - 1;
      const float* wq = s_wq + jc * PO;
      float gq = 0.f;
#pragma unroll
      for (int i = 0; i < NN; ++i) gq = fmaf(wq[i], gs[i], gq);
      gq = jm ? gq : 0.f;
      gpq[t] = pq[t] > 0.f ? gq : gq * am;
      if (valid && jm) {
        if (pq[t] < 0.f) d_am = fmaf(gq, pq[t], d_am);
        a.GPQ[((size_t)b * HH + jc) * L + l] = gpq[t];
      }
    }
    // ---- loop B: g_z_j = Wo[:, j]^T g_po + (Wm[:, j]^T g_pq summed over the group) / G -> g_pz_j -> g_x
    float gx[NN];
#pragma unroll
    for (int i = 0; i < NN; ++i) gx[i] = 0.f;
#pragma unroll 2
    for (int j = 0; j < HH; ++j) {
      float pz = 0.f;
#pragma unroll
      for (int i = 0; i < NN; ++i) pz = fmaf(wi2[j * NN + i], x[i], pz);
      pz += bi2[j];
      const float* wd = s_wd + j * PO;
      float gz = 0.f;
#pragma unroll
      for (int i = 0; i < NN; ++i) gz = fmaf(wd[i], gpo[i], gz);
      float t = 0.f;
#pragma unroll
      for (int t2 = 0; t2 < JPL; ++t2) {
        const int jr = jrow + t2 < HH ? jrow + t2 : HH - 1;
        t = fmaf(s_wm[jr * PM + j], gpq[t2], t);
      }
      gz = fmaf(srf_group_allsum<G>(t), 1.f / (float)G, gz);
      const float gp = pz > 0.f ? gz : gz * ai;
      if (valid) {
        if (pz < 0.f) d_ai = fmaf(gz, pz, d_ai);
        a.GPZ[(rowg * HH + j) * L + l] = gp;
      }
#pragma unroll
      for (int i = 0; i < NN; ++i) gx[i] = fmaf(wi2[j * NN + i], gp, gx[i]);
    }
    if (valid) {
#pragma unroll
      for (int i = 0; i < NN; ++i) a.gx[(rowg * NN + i) * L + l] = gx[i];
    } else {
      d_ao = 0.f;
    }
  }
  // ---- slope gradients: block reduction, one atomic per block and slope
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    d_ai += __shfl_xor(d_ai, o, 64);
    d_am += __shfl_xor(d_am, o, 64);
    d_ao += __shfl_xor(d_ao, o, 64);
  }
  if (lane == 0) {
    s_red[wave][0] = d_ai;
    s_red[wave][1] = d_am;
    s_red[wave][2] = d_ao;
  }
  __syncthreads();
  if (tid < 3) {
    const float t = (s_red[0][tid] + s_red[1][tid]) + (s_red[2][tid] + s_red[3][tid]);
    if (t != 0.f) atomicAdd(a.dslope + tid, t);
  }
}

// =============================================================================================================================
// MFMA form of the backward (round 4) for n = 16, H = 48, G = 16: same tile ownership and layout tricks as srf_tac_mfma_kernel.
// Per 32-column tile and wavefront:
//   sweep 1 (groups): z_g (fp16 parts, as the forward) -> Z, zsum            | once: zbar -> ZB, pq, q -> Q, r
//   sweep 2 (groups): z_g again, po_g = Wo[:, :H] z_g + r -> g_po -> GPO, gs | once: GS, g_pq = PReLU'(pq) Wo[:, H:]^T gs -> GPQ,
//                                                                            |       g_zbar = Wm^T g_pq / G
//   sweep 3 (groups): pz_g again, g_z = Wo[:, :H]^T g_po + g_zbar, g_pz = PReLU'(pz) g_z -> GPZ, g_x = Wi^T g_pz -> gx
// The forward recomputation uses the forward kernel's fp16 hi + lo parts (identical z); every GRADIENT operand (g_po, gs, g_pq,
// g_pz and the transposed weights) is split into two BF16 parts (16 mantissa bits, fp32's exponent range -- gradients can be far
// below fp16's 6e-5) like the rest of the backward's GEMMs.  g_po is re-read in sweep 3 straight in the B layout from GPO, which
// this wavefront wrote in sweep 2 (device-scope loads behind a vmcnt(0): other lanes' stores).
typedef __bf16 tac_bf16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ void tac_split8_bf(const float (&v)[8], tac_bf16x8& hi, tac_bf16x8& lo) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const __bf16 h = (__bf16)v[j];
    hi[j] = h;
    lo[j] = (__bf16)(v[j] - (float)h);
  }
}
__device__ __forceinline__ tac_f32x16 tac_mma3_bf(const tac_bf16x8& ah, const tac_bf16x8& al, const tac_bf16x8& bh,
                                                  const tac_bf16x8& bl, tac_f32x16 c) {
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, c, 0, 0, 0);
  return c;
}

__global__ __launch_bounds__(256, 2) void srf_tac_bwd_mfma_kernel(TacBwdArgs a, const float* __restrict__ wi,
                                                               const float* __restrict__ bi, const float* __restrict__ wo,
                                                               const float* __restrict__ bo, int tiles_per_row, int total_tiles) {
  constexpr int NN = 16, HH = 48, G = 16;
  // A fragments {hi, lo}, 1 KB each.  fp16 (x 2^4): 0..5 Wm (blk * 3 + s), 6..8 Wo[:, H:] (s), 9..11 Wo[:, :H] (s).
  // bf16: 12..13 Wo[:, H:]^T (blk), 14..19 Wm^T (blk * 3 + s), 20..21 Wo[:, :H]^T (blk), 22..24 Wi^T (s).
  __shared__ tac_f16x8 s_frag[50][64];
  __shared__ float s_bias[HH + HH + NN];   // bi | bm | bo
  __shared__ float s_red[4][3];
  // wave-private [48 rows][32 columns] strips (pitch 36): the big operand tensors (Z, GPZ: 24 registers per lane and group) leave
  // as float4 row stores -- 6 vector-memory instructions instead of 24 dword ones (the paired-block GEMM's epilogue lesson)
  __shared__ __attribute__((aligned(16))) float s_strip[4][HH * 36];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int t = lane & 31, h = lane >> 5;
  const int L = a.L;
  for (int e = tid; e < HH + HH + NN; e += 256) s_bias[e] = e < HH ? bi[e] : (e < 2 * HH ? a.bm[e - HH] : bo[e - 2 * HH]);
  for (int id = tid; id < 25 * 64; id += 256) {
    const int f = id >> 6, ln = id & 63, row32 = ln & 31, kh = ln >> 5;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float w = 0.f;
      if (f < 6) {
        const int blk = f / 3, sidx = f - blk * 3, j = blk * 32 + row32, k = 16 * sidx + 8 * kh + e;
        if (j < HH) w = a.wm[j * HH + k];
      } else if (f < 12) {
        const int half = (f - 6) / 3, sidx = (f - 6) - half * 3, k = 16 * sidx + 8 * kh + e;
        if (row32 < NN) w = wo[row32 * 2 * HH + (half == 0 ? HH : 0) + k];
      } else if (f < 14) {               // Wo[:, H:]^T [48][16]
        const int j = (f - 12) * 32 + row32, k = 8 * kh + e;
        if (j < HH) w = wo[k * 2 * HH + HH + j];
      } else if (f < 20) {               // Wm^T [48][48]
        const int blk = (f - 14) / 3, sidx = (f - 14) - blk * 3, j = blk * 32 + row32, k = 16 * sidx + 8 * kh + e;
        if (j < HH) w = a.wm[k * HH + j];
      } else if (f < 22) {               // Wo[:, :H]^T [48][16]
        const int j = (f - 20) * 32 + row32, k = 8 * kh + e;
        if (j < HH) w = wo[k * 2 * HH + j];
      } else {                           // Wi^T [16][48]
        const int sidx = f - 22, k = 16 * sidx + 8 * kh + e;
        if (row32 < NN) w = wi[k * NN + row32];
      }
      v[e] = f < 12 ? w * TAC_WS : w;
    }
    if (f < 12) {
      tac_f16x8 hi, lo;
      tac_split8(v, hi, lo);
      s_frag[2 * f][ln] = hi;
      s_frag[2 * f + 1][ln] = lo;
    } else {
      tac_bf16x8 hi, lo;
      tac_split8_bf(v, hi, lo);
      s_frag[2 * f][ln] = __builtin_bit_cast(tac_f16x8, hi);
      s_frag[2 * f + 1][ln] = __builtin_bit_cast(tac_f16x8, lo);
    }
  }
  tac_f16x8 wi_h[2], wi_l[2];
#pragma unroll
  for (int blk = 0; blk < 2; ++blk) {
    float v[8];
    const int j = blk * 32 + t;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = j < HH ? wi[j * NN + 8 * h + e] * TAC_WS : 0.f;
    tac_split8(v, wi_h[blk], wi_l[blk]);
  }
  __syncthreads();
  tac_f32x16 bi16[2];
#pragma unroll
  for (int blk = 0; blk < 2; ++blk)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = blk * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      bi16[blk][r] = row < HH ? s_bias[row] * TAC_WS : 0.f;
    }
  const float ai = a.ai[0], am = a.am[0], ao = a.ao[0];
  float d_ai = 0.f, d_am = 0.f, d_ao = 0.f;
  const int tile = blockIdx.x * 4 + wave;
  if (tile < total_tiles) {              // (wave-uniform; the block reduction below needs every wavefront)
    const int b = tile / tiles_per_row, l0 = (tile - b * tiles_per_row) * 32;
    const int col = l0 + t;
    const bool valid = col < L;
    const float vmask = valid ? 1.f : 0.f;
    auto rsrc = [&](const float* base, size_t per_example_rows) __attribute__((always_inline)) {
      return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base) + (size_t)b * per_example_rows * L, 0,
                                               (int)(per_example_rows * L * 4), 0x00020000);
    };
    __amdgpu_buffer_rsrc_t xrs = rsrc(a.x, G * NN), gors = rsrc(a.go, G * NN), gxrs = rsrc(a.gx, G * NN);
    __amdgpu_buffer_rsrc_t zrs = rsrc(a.Z, G * HH), gpzrs = rsrc(a.GPZ, G * HH), gpors = rsrc(a.GPO, G * NN);
    __amdgpu_buffer_rsrc_t gsrs = rsrc(a.GS, NN), qrs = rsrc(a.Q, HH), gpqrs = rsrc(a.GPQ, HH), zbrs = rsrc(a.ZB, HH);
    const int b_vo = valid ? (8 * h * L + col) * 4 : 0x7ffffff0;     // B layout: rows 8 h + e
    const int c_vo = valid ? (4 * h * L + col) * 4 : 0x7ffffff0;     // C layout: rows (r & 3) + 8 (r >> 2) + 4 h

    struct Raw8 {
      float v[8];
    };
    // 8 rows (row0 + 8 h + e) of this lane's column: a B fragment's values
    auto load_b8 = [&](__amdgpu_buffer_rsrc_t rs, int row0, Raw8& r, int aux) __attribute__((always_inline)) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (aux) r.v[e] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, b_vo, (row0 + e) * L * 4, 17));
        else r.v[e] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, b_vo, (row0 + e) * L * 4, 0));
      }
    };
    // C-layout registers c[0 .. n) (16-row groups) <-> rows row0 + (r & 3) + 8 (r >> 2) + 4 h
    auto store_c = [&](__amdgpu_buffer_rsrc_t rs, int row0, const float* c, int n) __attribute__((always_inline)) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (r < n) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(c[r]), rs, c_vo, (row0 + (r & 3) + 8 * (r >> 2)) * L * 4, 0);
    };
    auto clamp8 = [&](float (&v)[8]) __attribute__((always_inline)) { (void)v; };      // (no range guard: see the forward kernel)
    // 48 rows (C layout: c[0..15] rows 0..31, c[16..23] rows 32..47) of this tile -> rows row0 .. row0 + 47 of `rs`, through the strip
    float* strip = s_strip[wave];
    auto store_rows48 = [&](__amdgpu_buffer_rsrc_t rs, int row0, const float* c) __attribute__((always_inline)) {
      typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
#pragma unroll
      for (int r = 0; r < 24; ++r)
        strip[((r < 16 ? 0 : 32) + (r & 3) + 8 * ((r & 15) >> 2) + 4 * h) * 36 + t] = c[r];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (int it = 0; it < 6; ++it) {
        const int idx = it * 64 + lane, row = idx >> 3, c4 = (idx & 7) * 4;
        const float4 v = *reinterpret_cast<const float4*>(strip + row * 36 + c4);
        const u32x4 ov = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
        const int off = l0 + c4 < L ? ((row0 + row) * L + l0 + c4) * 4 : 0x7ffffff0;     // (L % 4 == 0: whole float4s)
        __builtin_amdgcn_raw_buffer_store_b128(ov, rs, off, 0, 0);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    // 2^4 (Wi x + bi) of a group in the C layout (pre-activation): zA rows 0..31, zB rows 32..47 (registers 0..7)
    auto pz_of = [&](Raw8& xr, tac_f32x16& zA, tac_f32x16& zB) __attribute__((always_inline)) {
      tac_f16x8 xh, xl;
      clamp8(xr.v);
      tac_split8(xr.v, xh, xl);
      zA = tac_mma3(wi_h[0], wi_l[0], xh, xl, bi16[0]);
      zB = tac_mma3(wi_h[1], wi_l[1], xh, xl, bi16[1]);
    };
    auto frags16 = [&](const tac_f32x16& cA, const tac_f32x16& cB, float scale, tac_f16x8 (&fh)[3], tac_f16x8 (&fl)[3])
        __attribute__((always_inline)) {
#pragma unroll
      for (int sidx = 0; sidx < 3; ++sidx) {
        float c8[8], v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) c8[e] = (sidx < 2 ? cA[8 * sidx + e] : cB[e]) * scale;
        tac_c_to_b(c8, v);
        tac_split8(v, fh[sidx], fl[sidx]);
      }
    };
    auto frags_bf = [&](const tac_f32x16& cA, const tac_f32x16& cB, tac_bf16x8 (&fh)[3], tac_bf16x8 (&fl)[3])
        __attribute__((always_inline)) {
#pragma unroll
      for (int sidx = 0; sidx < 3; ++sidx) {
        float c8[8], v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) c8[e] = sidx < 2 ? cA[8 * sidx + e] : cB[e];
        tac_c_to_b(c8, v);
        tac_split8_bf(v, fh[sidx], fl[sidx]);
      }
    };
    auto fragA16 = [&](int f, tac_f16x8& hi, tac_f16x8& lo) __attribute__((always_inline)) {
      hi = s_frag[2 * f][lane];
      lo = s_frag[2 * f + 1][lane];
    };
    auto fragAbf = [&](int f, tac_bf16x8& hi, tac_bf16x8& lo) __attribute__((always_inline)) {
      hi = __builtin_bit_cast(tac_bf16x8, s_frag[2 * f][lane]);
      lo = __builtin_bit_cast(tac_bf16x8, s_frag[2 * f + 1][lane]);
    };

    // ================= sweep 1: z_g -> Z, zsum
    tac_f32x16 zsA, zsB;
#pragma unroll
    for (int r = 0; r < 16; ++r) zsA[r] = zsB[r] = 0.f;
    Raw8 xa, xb;
    load_b8(xrs, 0, xa, 0);
    auto sweep1 = [&](Raw8& cur, Raw8& nxt, int g) __attribute__((always_inline)) {
      load_b8(xrs, (g + 1 < G ? g + 1 : 0) * NN, nxt, 0);
      tac_f32x16 zA, zB;
      pz_of(cur, zA, zB);
      float zs[24];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        zA[r] = srf_prelu(zA[r], ai);
        zsA[r] += zA[r];
        zs[r] = zA[r] * (1.f / TAC_WS);
      }
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        zB[r] = srf_prelu(zB[r], ai);
        zsB[r] += zB[r];
        zs[16 + r] = zB[r] * (1.f / TAC_WS);
      }
      store_rows48(zrs, g * HH, zs);
    };
    for (int g = 0; g < G; g += 2) {
      sweep1(xa, xb, g);
      sweep1(xb, xa, g + 1);
    }
    // ================= zbar -> ZB; pq, q -> Q; r = Wo[:, H:] q + bo
    tac_f32x16 r256;
    {
      tac_f32x16 pqA, pqB;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        zsA[r] *= 1.f / (float)G;          // 2^4 zbar
        zsB[r] *= 1.f / (float)G;
      }
      float zb[24];
#pragma unroll
      for (int r = 0; r < 16; ++r) zb[r] = zsA[r] * (1.f / TAC_WS);
#pragma unroll
      for (int r = 0; r < 8; ++r) zb[16 + r] = zsB[r] * (1.f / TAC_WS);
      store_c(zbrs, 0, zb, 16);
      store_c(zbrs, 32, zb + 16, 8);
      tac_f16x8 fh[3], fl[3];
      frags16(zsA, zsB, 1.f, fh, fl);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
        pqA[r] = s_bias[HH + row] * (TAC_WS * TAC_WS);
        pqB[r] = row < HH - 32 ? s_bias[HH + 32 + row] * (TAC_WS * TAC_WS) : 0.f;
      }
#pragma unroll
      for (int sidx = 0; sidx < 3; ++sidx) {
        tac_f16x8 ah, al;
        fragA16(sidx, ah, al);
        pqA = tac_mma3(ah, al, fh[sidx], fl[sidx], pqA);
        fragA16(3 + sidx, ah, al);
        pqB = tac_mma3(ah, al, fh[sidx], fl[sidx], pqB);
      }
      tac_f32x16 qA, qB;
      float qs[24], pqs[24];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        pqA[r] *= 1.f / (TAC_WS * TAC_WS);
        pqB[r] *= 1.f / (TAC_WS * TAC_WS);
        qA[r] = srf_prelu(pqA[r], am);
        qB[r] = srf_prelu(pqB[r], am);
        qs[r] = qA[r];
        pqs[r] = pqA[r];
      }
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        qs[16 + r] = qB[r];
        pqs[16 + r] = pqB[r];
      }
      store_c(qrs, 0, qs, 16);
      store_c(qrs, 32, qs + 16, 8);
      // pq is needed again behind sweep 2 (PReLU'): parked in GPQ's own slots -- each lane re-reads exactly what it wrote, and
      // overwrites it with g_pq afterwards -- instead of 24 registers across the sweep
      store_c(gpqrs, 0, pqs, 16);
      store_c(gpqrs, 32, pqs + 16, 8);
      frags16(qA, qB, TAC_WS, fh, fl);           // 2^4 q
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
        r256[r] = row < NN ? s_bias[2 * HH + row] * (TAC_WS * TAC_WS) : 0.f;
      }
#pragma unroll
      for (int sidx = 0; sidx < 3; ++sidx) {
        tac_f16x8 ah, al;
        fragA16(6 + sidx, ah, al);
        r256 = tac_mma3(ah, al, fh[sidx], fl[sidx], r256);
      }
    }
    // ================= sweep 2: po_g -> g_po -> GPO, gs
    float gs[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) gs[r] = 0.f;
    auto sweep2 = [&](Raw8& cur, Raw8& nxt, int g) __attribute__((always_inline)) {
      load_b8(xrs, (g + 1 < G ? g + 1 : 0) * NN, nxt, 0);
      float gov[8];
#pragma unroll
      for (int r = 0; r < 8; ++r)
        gov[r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(gors, c_vo, (g * NN + (r & 3) + 8 * (r >> 2)) * L * 4, 0));
      tac_f32x16 zA, zB;
      pz_of(cur, zA, zB);
#pragma unroll
      for (int r = 0; r < 16; ++r) zA[r] = srf_prelu(zA[r], ai);
#pragma unroll
      for (int r = 0; r < 8; ++r) zB[r] = srf_prelu(zB[r], ai);
      tac_f16x8 fh[3], fl[3];
      frags16(zA, zB, 1.f, fh, fl);
      tac_f32x16 o = r256;
#pragma unroll
      for (int sidx = 0; sidx < 3; ++sidx) {
        tac_f16x8 ah, al;
        fragA16(9 + sidx, ah, al);
        o = tac_mma3(ah, al, fh[sidx], fl[sidx], o);
      }
      float gpo[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const float pv = o[r] * (1.f / (TAC_WS * TAC_WS));
        const float gv = gov[r];                 // (out-of-range columns loaded 0)
        gpo[r] = pv > 0.f ? gv : gv * ao;
        d_ao = pv < 0.f ? fmaf(gv, pv, d_ao) : d_ao;
        gs[r] += gpo[r];
      }
      store_c(gpors, g * NN, gpo, 8);
    };
    for (int g = 0; g < G; g += 2) {
      sweep2(xa, xb, g);
      sweep2(xb, xa, g + 1);
    }
    // ================= GS; g_pq = PReLU'(pq) (Wo[:, H:]^T gs) -> GPQ; g_zbar / G = Wm^T g_pq / G
    tac_f32x16 gzbA, gzbB;
    {
      store_c(gsrs, 0, gs, 8);
      tac_bf16x8 gh, gl;
      {
        float v[8];
        tac_c_to_b(gs, v);
        tac_split8_bf(v, gh, gl);
      }
      tac_f32x16 gqA, gqB;
#pragma unroll
      for (int r = 0; r < 16; ++r) gqA[r] = gqB[r] = 0.f;
      tac_bf16x8 ah, al;
      fragAbf(12, ah, al);
      gqA = tac_mma3_bf(ah, al, gh, gl, gqA);
      fragAbf(13, ah, al);
      gqB = tac_mma3_bf(ah, al, gh, gl, gqB);
      float gpq[24], pqv[24];
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
      for (int r = 0; r < 24; ++r)
        pqv[r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
            gpqrs, c_vo, ((r < 16 ? 0 : 32) + (r & 3) + 8 * ((r & 15) >> 2)) * L * 4, 17));
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float gq = gqA[r], pv = pqv[r];
        gqA[r] = pv > 0.f ? gq : gq * am;
        d_am = pv < 0.f ? fmaf(gq * vmask, pv, d_am) : d_am;
        gpq[r] = gqA[r];
      }
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const float gq = gqB[r], pv = pqv[16 + r];
        gqB[r] = pv > 0.f ? gq : gq * am;
        d_am = pv < 0.f ? fmaf(gq * vmask, pv, d_am) : d_am;
        gpq[16 + r] = gqB[r];
      }
      store_c(gpqrs, 0, gpq, 16);
      store_c(gpqrs, 32, gpq + 16, 8);
      tac_bf16x8 fh[3], fl[3];
      frags_bf(gqA, gqB, fh, fl);
#pragma unroll
      for (int r = 0; r < 16; ++r) gzbA[r] = gzbB[r] = 0.f;
#pragma unroll
      for (int sidx = 0; sidx < 3; ++sidx) {
        fragAbf(14 + sidx, ah, al);
        gzbA = tac_mma3_bf(ah, al, fh[sidx], fl[sidx], gzbA);
        fragAbf(17 + sidx, ah, al);
        gzbB = tac_mma3_bf(ah, al, fh[sidx], fl[sidx], gzbB);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        gzbA[r] *= 1.f / (float)G;
        gzbB[r] *= 1.f / (float)G;
      }
    }
    // ================= sweep 3: g_z = Wo[:, :H]^T g_po + g_zbar / G, g_pz -> GPZ, g_x = Wi^T g_pz
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wavefront's GPO stores have left before other lanes read them
    auto sweep3 = [&](Raw8& cur, Raw8& nxt, int g) __attribute__((always_inline)) {
      if (g + 1 < G) load_b8(xrs, (g + 1) * NN, nxt, 0);
      Raw8 gp;
      load_b8(gpors, g * NN, gp, 1);                    // g_po of the group in the B layout (device-scope loads)
      tac_f32x16 pzA, pzB;
      pz_of(cur, pzA, pzB);                             // 2^4 pz
      tac_bf16x8 gh, gl;
      tac_split8_bf(gp.v, gh, gl);
      tac_f32x16 gzA = gzbA, gzB = gzbB;
      tac_bf16x8 ah, al;
      fragAbf(20, ah, al);
      gzA = tac_mma3_bf(ah, al, gh, gl, gzA);
      fragAbf(21, ah, al);
      gzB = tac_mma3_bf(ah, al, gh, gl, gzB);
      float gpz[24];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float pv = pzA[r] * (1.f / TAC_WS), gz = gzA[r];
        gzA[r] = pv > 0.f ? gz : gz * ai;
        d_ai = pv < 0.f ? fmaf(gz * vmask, pv, d_ai) : d_ai;
        gpz[r] = gzA[r];
      }
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const float pv = pzB[r] * (1.f / TAC_WS), gz = gzB[r];
        gzB[r] = pv > 0.f ? gz : gz * ai;
        d_ai = pv < 0.f ? fmaf(gz * vmask, pv, d_ai) : d_ai;
        gpz[16 + r] = gzB[r];
      }
      store_rows48(gpzrs, g * HH, gpz);
      tac_bf16x8 fh[3], fl[3];
      frags_bf(gzA, gzB, fh, fl);
      tac_f32x16 gx;
#pragma unroll
      for (int r = 0; r < 16; ++r) gx[r] = 0.f;
#pragma unroll
      for (int sidx = 0; sidx < 3; ++sidx) {
        fragAbf(22 + sidx, ah, al);
        gx = tac_mma3_bf(ah, al, fh[sidx], fl[sidx], gx);
      }
      float gxv[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) gxv[r] = gx[r];
      store_c(gxrs, g * NN, gxv, 8);
    };
    load_b8(xrs, 0, xa, 0);
    for (int g = 0; g < G; g += 2) {
      sweep3(xa, xb, g);
      sweep3(xb, xa, g + 1);
    }
  }
  // ---- slope gradients: wavefront sums, block sum, one atomic per block and slope
  d_ai = srf_dpp_wave_sum(d_ai);
  d_am = srf_dpp_wave_sum(d_am);
  d_ao = srf_dpp_wave_sum(d_ao);
  if (lane == 63) {
    s_red[wave][0] = d_ai;
    s_red[wave][1] = d_am;
    s_red[wave][2] = d_ao;
  }
  __syncthreads();
  if (tid < 3) {
    const float tsum = (s_red[0][tid] + s_red[1][tid]) + (s_red[2][tid] + s_red[3][tid]);
    if (tsum != 0.f) atomicAdd(a.dslope + tid, tsum);
  }
}

template <int NN>
static bool srf_tac_bwd_g(const TacBwdArgs& a, const float* const* P, int Bt, hipStream_t st) {
#define SRF_TAC_BWD_GO(GG)                                                                                  \
  {                                                                                                          \
    constexpr int CW = 64 / GG;                                                                              \
    dim3 grid((a.L + 4 * CW - 1) / (4 * CW), Bt);                                                            \
    hipLaunchKernelGGL((srf_tac_bwd_lanes_kernel<NN, GG>), grid, dim3(256), 0, st, a, P[0], P[1], P[6], P[7], P[0], P[1]); \
    return true;                                                                                             \
  }
  switch (a.G) {
    case 2: SRF_TAC_BWD_GO(2)
    case 4: SRF_TAC_BWD_GO(4)
    case 8: SRF_TAC_BWD_GO(8)
    case 16: SRF_TAC_BWD_GO(16)
    default: return false;
  }
#undef SRF_TAC_BWD_GO
}

static size_t tac_al(size_t v) { return (v + 63) / 64 * 64; }

extern "C" size_t srf_tac_bwd_scratch_bytes(int Bt, int G, int n, int L) {
  if (Bt <= 0 || G <= 0 || n <= 0 || L <= 0) return 0;
  const size_t H = 3 * (size_t)n, BG = (size_t)Bt * G;
  const size_t fl = 2 * tac_al(BG * H * L) + tac_al(BG * n * L) + tac_al((size_t)Bt * n * L) + 3 * tac_al((size_t)Bt * H * L) + 64;
  size_t wg = srf_pw_wgrad_scratch_bytes((int)BG, (int)H, n, L);
  const size_t w2 = srf_pw_wgrad_scratch_bytes((int)BG, n, (int)H, L), w3 = srf_pw_wgrad_scratch_bytes(Bt, (int)H, (int)H, L);
  if (w2 > wg) wg = w2;
  if (w3 > wg) wg = w3;
  return sizeof(float) * fl + wg + 256;
}

// x, go, gx: [Bt,G,n,L]; params: the 9 TAC tensors as in srf_tac; grads: 9 device pointers of the same shapes,
// ACCUMULATED into.  gx receives the MLP-path gradient only (the residual / TAC_norm paths are the caller's).
extern "C" int srf_tac_bwd(const float* x, const float* go, const float* const* params, float* const* grads, int Bt,
                           int G, int n, int H, int L, float* gx, void* scratch, void* stream) {
  SRF_CHECK_ARG(x && go && params && grads && gx && scratch, "srf_tac_bwd: null pointer");
  SRF_CHECK_ARG(Bt > 0 && G > 0 && n > 0 && L > 0 && Bt <= 65535 && (L % 4) == 0, "srf_tac_bwd: bad sizes (L %% 4 == 0)");
  SRF_CHECK_ARG(H == 3 * n, "srf_tac_bwd: hidden size must be 3*n");
  for (int i = 0; i < 9; ++i) SRF_CHECK_ARG(params[i] && grads[i], "srf_tac_bwd: null parameter / gradient %d", i);
  // x and the scratch slices feed srf_pw_wgrad (which has no unaligned form) after the first launch; go / gx move as 16-byte
  // rows in the MFMA kernel: refuse here, before anything runs
  SRF_CHECK_ALIGNED16("srf_tac_bwd", {"x", x}, {"go", go}, {"gx", gx}, {"scratch", scratch});
  hipStream_t st = (hipStream_t)stream;
  const size_t BG = (size_t)Bt * G;
  float* f = reinterpret_cast<float*>(scratch);
  TacBwdArgs a;
  a.x = x;
  a.go = go;
  a.wm = params[3];
  a.bm = params[4];
  a.ai = params[2];
  a.am = params[5];
  a.ao = params[8];
  a.gx = gx;
  a.Z = f;
  f += tac_al(BG * H * L);
  a.GPZ = f;
  f += tac_al(BG * H * L);
  a.GPO = f;
  f += tac_al(BG * n * L);
  a.GS = f;
  f += tac_al((size_t)Bt * n * L);
  a.Q = f;
  f += tac_al((size_t)Bt * H * L);
  a.GPQ = f;
  f += tac_al((size_t)Bt * H * L);
  a.ZB = f;
  f += tac_al((size_t)Bt * H * L);
  a.dslope = f;
  f += 64;
  void* wg = f;
  a.G = G;
  a.L = L;
  SRF_CHECK_HIP(hipMemsetAsync(a.dslope, 0, 3 * sizeof(float), st));
  bool ok = false, mfma = false;
  // debug flag 1 << 22: the VALU kernel (the MFMA form serves n = 16, G = 16)
  if (srf_kernel_mode() != 1 && n == 16 && G == 16 && !srf_dbg(SRF_DBG_TAC_VALU) && (long)G * H * L * 4 < (1L << 31) &&
      (long)Bt * ((L + 31) / 32) < (1L << 30)) {
    const int tiles_per_row = (L + 31) / 32;
    const long total = (long)Bt * tiles_per_row;
    hipLaunchKernelGGL(srf_tac_bwd_mfma_kernel, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, st, a, params[0], params[1],
                       params[6], params[7], tiles_per_row, (int)total);
    ok = mfma = true;
  } else
  switch (n) {
    case 2: ok = srf_tac_bwd_g<2>(a, params, Bt, st); break;
    case 4: ok = srf_tac_bwd_g<4>(a, params, Bt, st); break;
    case 8: ok = srf_tac_bwd_g<8>(a, params, Bt, st); break;
    case 16: ok = srf_tac_bwd_g<16>(a, params, Bt, st); break;
    default: break;
  }
  if (!ok) {
    srf_set_error("srf_tac_bwd: n=%d, G=%d unsupported (n in 2,4,8,16; G in 2,4,8,16)", n, G);
    return SRF_EINVAL;
  }
  if (mfma) {
    SRF_CHECK_LAUNCH("tac_bwd_mfma", st);
  } else {
    SRF_CHECK_LAUNCH("tac_bwd", st);
  }
  int rc;
  // weight / bias gradients: four reductions over (batch, group, time) as weight-gradient GEMMs
  rc = srf_pw_wgrad(a.GPZ, x, nullptr, (int)BG, n, H, L, grads[0], grads[1], 1, wg, stream);              // dWi, dbi
  if (rc) return rc;
  rc = srf_pw_wgrad_ld(a.GPO, a.Z, nullptr, (int)BG, H, n, L, grads[6], H, 2 * H, grads[7], 1, wg, stream);   // dWo[:, :H], dbo
  if (rc) return rc;
  rc = srf_pw_wgrad_ld(a.GS, a.Q, nullptr, Bt, H, n, L, grads[6] + H, H, 2 * H, nullptr, 1, wg, stream);      // dWo[:, H:]
  if (rc) return rc;
  rc = srf_pw_wgrad(a.GPQ, a.ZB, nullptr, Bt, H, H, L, grads[3], grads[4], 1, wg, stream);                 // dWm, dbm
  if (rc) return rc;
  // the three slope gradients: grads[2,5,8] += dslope[0,1,2]
  hipLaunchKernelGGL(srf_tac_slope_add_kernel, dim3(1), dim3(64), 0, st, a.dslope, grads[2], grads[5], grads[8]);
  SRF_CHECK_LAUNCH("tac_bwd_slopes", st);
  return SRF_OK;
}
