// Stateful streaming inference for the causal SuDoRM-RF (v3): a session (srf_stream) takes the next n samples of every
// stream and returns n separated samples delayed by h = K/2, carrying on the device what the next push needs:
//   encoder history   [Bt, A, 2h]          the last 2h input samples (zeros = the conv's left padding)
//   depthwise state   [U][D][Bt, C, 10]    the last 10 INPUTS of every pyramid level (level 0: PReLU_p(y1), i.e. after
//                                          proj_1x1.act; level k: level k-1's output after its PReLU)
//   decoder tail      [Bt, S*A, h+1]       the pending overlap-add sums of the samples that later frames still touch
// Activations of a push are [channels][Bt * Lc] (column = b * Lc + l, Lc = n / h frames), so a 1x1 conv is one plain GEMM and a
// pyramid row (b, c) is contiguous.  Every output element is accumulated in an order that does not depend on n: the same
// samples under any chunk schedule give the same bits.
//   srf_stream_enc_kernel      causal encoder over [history | chunk]
//   srf_stream_pw_kernel       skinny exact-fp32 1x1 GEMM, any number of columns >= 1 (bias, PReLU on load, residual)
//   srf_stream_pyramid_kernel  all D levels + merge of one block for a chunk, reads and rolls the depthwise state
//   srf_stream_ola_kernel      overlap-add of the decoder frames with the stored tail; also rolls the encoder history
// Plain launches only; a push allocates nothing, copies nothing and never synchronises.
// Only the encoder, the pyramid and the overlap-add (and the flush) turn a column into a stream.  Each is ONE device body
// templated on a row mapper: StreamRowsUniform is the lock-step push (row b of the launch = state slot b, Lc frames each),
// StreamRowsTable the row-table push of srf_stream_push_rows (row j = {state slot, first column, frames}, passed by value as
// a kernel argument).  FMA order, LDS layout and merge order are therefore shared by construction.
#include <new>
#include <vector>

#include "srf_plan.h"

#define SRF_STREAM_HIST (SRF_CAUSAL_TAPS - 1)
#define SRF_STREAM_TN 8      // columns per GEMM tile
#define SRF_STREAM_RPW 4     // pyramid rows per wavefront (16 lanes each)
#define SRF_STREAM_LDS_MAX (64 * 1024)

// ---------------------------------------------------------------------------------------------
// row mappers.  Row j of a launch owns columns [col0(j), col0(j) + frames(j)) of the [channels][ncol] activations, the
// contiguous [A, h frames] block at float offset A h col0(j) of wav, the [S*A, h frames] block at S*A h col0(j) of out, and
// the state of slot(j).  For the uniform mapper these are the [Bt, A, n] / [Bt, S*A, n] tensors of srf_stream_push.
// ---------------------------------------------------------------------------------------------
struct StreamRowsUniform {
  int Bt, Lc;
  int chan_major;   // pyramid only: rows of y1 / merged ordered (c, b) (the push's layout) instead of (b, c)
  __device__ __forceinline__ int slot(int j) const { return j; }
  __device__ __forceinline__ int col0(int j) const { return j * Lc; }
  __device__ __forceinline__ int frames(int) const { return Lc; }
  __device__ __forceinline__ int max_frames() const { return Lc; }
  __device__ __forceinline__ size_t ncol() const { return (size_t)Bt * Lc; }
  // pyramid row r of `rows` -> channel, state slot, offset of its y1 / merged row, frames
  __device__ __forceinline__ void pyr_row(long r, int C, int& c, int& sl, size_t& off, int& frames_) const {
    c = chan_major ? (int)(r / Bt) : (int)(r % C);
    sl = chan_major ? (int)(r % Bt) : (int)(r / C);
    off = (size_t)r * Lc;
    frames_ = Lc;
  }
};

// The host validates every entry before a launch (slots in range and distinct, frames a positive multiple of 2^(D-1) and at
// most max_lc, col0 the prefix sum): no kernel indexes memory through a value the host has not checked.
struct StreamRowsTable {
  int slot_[SRF_STREAM_ROWS_PER_LAUNCH], col0_[SRF_STREAM_ROWS_PER_LAUNCH], frames_[SRF_STREAM_ROWS_PER_LAUNCH];
  int rows, max_frames_, ncol_;   // rows of this group, its largest frames, columns of the whole push
  __device__ __forceinline__ int slot(int j) const { return slot_[j]; }
  __device__ __forceinline__ int col0(int j) const { return col0_[j]; }
  __device__ __forceinline__ int frames(int j) const { return frames_[j]; }
  __device__ __forceinline__ int max_frames() const { return max_frames_; }
  __device__ __forceinline__ size_t ncol() const { return (size_t)ncol_; }
  __device__ __forceinline__ void pyr_row(long r, int, int& c, int& sl, size_t& off, int& frames_o) const {
    c = (int)(r / rows);
    const int j = (int)(r % rows);
    sl = slot_[j];
    off = (size_t)c * ncol_ + col0_[j];
    frames_o = frames_[j];
  }
};
static_assert(sizeof(StreamRowsTable) <= 2048, "the row table travels as a kernel argument");

// ---------------------------------------------------------------------------------------------
// encoder: out[nb][col0 + l] = sum_{a, k<K} w[nb,a,k] win[a, h l + k],  win = [hist of the slot (2h) | the row's chunk].
// A block = 32 basis functions x 8 frames of one row; grid z = the rows of the launch, grid y covers the longest row and a
// block past its own row's frames exits before touching memory.  Same FMA order per output as srf_causal_encoder_kernel.
// The history is NOT written here (every basis tile of the stream reads it): srf_stream_ola_kernel rolls it.
// ---------------------------------------------------------------------------------------------
template <class M>
__global__ __launch_bounds__(256) void srf_stream_enc_kernel(const float* __restrict__ wav, const float* __restrict__ hist,
                                                             const float* __restrict__ w, float* __restrict__ out, int A,
                                                             int N, int K, M m) {
  extern __shared__ float win[];   // [A][WIN]
  const int H = K / 2, KW = 2 * K - 1;
  const int WIN = 7 * H + K;
  const int j = blockIdx.z;
  const int l0 = blockIdx.y * 8;
  const int Lc = m.frames(j);
  if (l0 >= Lc) return;            // the whole block: a shorter row of a row-table launch
  const int n = H * Lc, sl = m.slot(j), c0 = m.col0(j);
  const float* wr = wav + (size_t)A * H * c0;   // this row's [A, n] block
  for (int i = threadIdx.x; i < A * WIN; i += 256) {
    const int a = i / WIN, q = i - a * WIN;
    const int s = H * l0 + q;                  // index into [hist | chunk]
    float v = 0.f;
    if (s < 2 * H) v = hist[((size_t)sl * A + a) * 2 * H + s];
    else if (s - 2 * H < n) v = wr[(size_t)a * n + s - 2 * H];
    win[i] = v;
  }
  __syncthreads();
  const int lf = threadIdx.x & 7;
  const int nb = blockIdx.x * 32 + (threadIdx.x >> 3);
  const int l = l0 + lf;
  if (nb >= N || l >= Lc) return;
  float acc = 0.f;
  for (int a = 0; a < A; ++a) {
    const float* wn = w + ((size_t)nb * A + a) * KW;
    const float* xw = win + a * WIN + H * lf;
    for (int k = 0; k < K; ++k) acc = fmaf(wn[k], xw[k], acc);
  }
  out[(size_t)nb * m.ncol() + c0 + l] = acc;
}

// ---------------------------------------------------------------------------------------------
// skinny 1x1 GEMM: y[co][j] = bias[co] + sum_k w[co][k] f(x[k][j]) (+ res[co][j]), f = PReLU (slope in_prelu[0]) or identity.
// A block = 4 output channels (one per wavefront) x a tile of TN columns; the activation tile [Cin][TN] is staged in LDS.
// Lane i of a wavefront sums k = i, i + 64, ... in that order, the 64 partial sums are added by a fixed DPP tree: the
// accumulation order of an output depends on Cin only, never on the number of columns.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void srf_stream_pw_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ bias, const float* __restrict__ in_prelu,
                                                            const float* __restrict__ res, float* __restrict__ y, int Cin,
                                                            int Cout, long Ncol) {
  extern __shared__ float xs[];   // [Cin][TN]
  const long j0 = (long)blockIdx.y * SRF_STREAM_TN;
  const float ai = in_prelu ? in_prelu[0] : 1.f;
  for (int i = threadIdx.x; i < Cin * SRF_STREAM_TN; i += 256) {
    const int k = i / SRF_STREAM_TN, c = i - k * SRF_STREAM_TN;
    float v = j0 + c < Ncol ? x[(size_t)k * Ncol + j0 + c] : 0.f;
    if (in_prelu) v = srf_prelu(v, ai);
    xs[i] = v;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int co = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (co >= Cout) return;
  float acc[SRF_STREAM_TN];
#pragma unroll
  for (int c = 0; c < SRF_STREAM_TN; ++c) acc[c] = 0.f;
  const float* wr = w + (size_t)co * Cin;
  for (int k = lane; k < Cin; k += 64) {
    const float wk = wr[k];
    const float4 p = *reinterpret_cast<const float4*>(xs + k * SRF_STREAM_TN);
    const float4 q = *reinterpret_cast<const float4*>(xs + k * SRF_STREAM_TN + 4);
    acc[0] = fmaf(wk, p.x, acc[0]);
    acc[1] = fmaf(wk, p.y, acc[1]);
    acc[2] = fmaf(wk, p.z, acc[2]);
    acc[3] = fmaf(wk, p.w, acc[3]);
    acc[4] = fmaf(wk, q.x, acc[4]);
    acc[5] = fmaf(wk, q.y, acc[5]);
    acc[6] = fmaf(wk, q.z, acc[6]);
    acc[7] = fmaf(wk, q.w, acc[7]);
  }
  float mine = 0.f;
#pragma unroll
  for (int c = 0; c < SRF_STREAM_TN; ++c) {
    const float t = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(srf_dpp_wave_sum(acc[c])), 63));
    if (lane == c) mine = t;
  }
  if (lane < SRF_STREAM_TN && j0 + lane < Ncol) {
    const size_t o = (size_t)co * Ncol + j0 + lane;
    float v = mine + (bias ? bias[co] : 0.f);
    if (res) v += res[o];
    y[o] = v;
  }
}

static int stream_pw(const float* x, const float* w, const float* bias, const float* in_prelu, const float* res, float* y,
                     int Cin, int Cout, long Ncol, hipStream_t st) {
  const size_t lds = sizeof(float) * (size_t)Cin * SRF_STREAM_TN;
  const long ty = (Ncol + SRF_STREAM_TN - 1) / SRF_STREAM_TN;
  SRF_CHECK_ARG(lds <= SRF_STREAM_LDS_MAX && ty <= 65535, "stream_pw: Cin=%d / %ld columns out of range", Cin, Ncol);
  hipLaunchKernelGGL(srf_stream_pw_kernel, dim3((Cout + 3) / 4, (unsigned)ty), dim3(256), lds, st, x, w, bias, in_prelu, res, y,
                     Cin, Cout, Ncol);
  SRF_CHECK_LAUNCH("stream_pw", st);
  return SRF_OK;
}

// ---------------------------------------------------------------------------------------------
// streaming pyramid.  A wavefront owns SRF_STREAM_RPW rows (stream, c), 16 lanes each, and nobody else touches their state.  Per row,
// in LDS:  in_k = [state_k (10) | chunk input of level k]  for every level, where the chunk input of level 0 is PReLU_p(y1) and
// that of level k >= 1 is level k-1's output.  The state is copied into LDS before any of it is overwritten; the new state
// is the last 10 entries of in_k (old entries shifted where the chunk is shorter than 10 frames).  Output j of level k reads
// in_k[s j .. s j + 10] (s = 1 for level 0, 2 below): the same operands, FMA order and merge order as srf_causal_dw_kernel /
// srf_causal_merge_kernel on the whole sequence, because chunk boundaries fall on even positions of every strided level.
// The LDS stride of a row comes from the launch's largest frames; every row lays out its levels (stream_pyr_off) and bounds
// its loops by its OWN frames, so the four rows of a wavefront may belong to streams with different chunk lengths.  The
// barriers are unconditional.
// ---------------------------------------------------------------------------------------------
struct StreamPyrArgs {
  const float* y1;
  float* merged;
  float* state[SRF_MAX_DEPTH];   // level k: [Bt, C, 10]
  const float* in_prelu;
  const float* w[SRF_MAX_DEPTH];
  const float* b[SRF_MAX_DEPTH];
  const float* a[SRF_MAX_DEPTH];
  int C;
  long rows;
};

template <int D>
__host__ __device__ constexpr int stream_pyr_off(int k, int Lc) {   // offset of in_k (k = D: the last level's output)
  int o = 0;
  for (int i = 0; i < k; ++i) o += SRF_STREAM_HIST + (i == 0 ? Lc : (Lc >> (i - 1)));
  return o;
}

template <int D, class M>
__global__ __launch_bounds__(64) void srf_stream_pyramid_kernel(StreamPyrArgs a, M m) {
  extern __shared__ float sm[];
  const int Lm = m.max_frames();
  const int per_row = stream_pyr_off<D>(D, Lm) + (Lm >> (D - 1));
  const int sub = threadIdx.x & 15;
  const long r = (long)blockIdx.x * SRF_STREAM_RPW + (threadIdx.x >> 4);
  const bool live = r < a.rows;
  int c = 0, sl = 0, Lc = 0;
  size_t yoff = 0;
  if (live) m.pyr_row(r, a.C, c, sl, yoff, Lc);
  const size_t srow = ((size_t)sl * a.C + c) * SRF_STREAM_HIST;
  float* row = sm + (size_t)(threadIdx.x >> 4) * per_row;
  if (live) {
    if (sub < SRF_STREAM_HIST) {
#pragma unroll
      for (int k = 0; k < D; ++k) row[stream_pyr_off<D>(k, Lc) + sub] = a.state[k][srow + sub];
    }
    const float ap = a.in_prelu[0];
    const float* yr = a.y1 + yoff;
    for (int i = sub; i < Lc; i += 16) row[SRF_STREAM_HIST + i] = srf_prelu(yr[i], ap);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const float* in = row + stream_pyr_off<D>(k, Lc);
    float* outk = row + stream_pyr_off<D>(k + 1, Lc) + (k + 1 < D ? SRF_STREAM_HIST : 0);
    const int stride = k == 0 ? 1 : 2;
    const int nin = k == 0 ? Lc : (Lc >> (k - 1));
    const int nout = Lc >> k;
    if (live) {
      const float* wc = a.w[k] + (size_t)c * SRF_CAUSAL_KW;
      float wk[SRF_CAUSAL_TAPS];
#pragma unroll
      for (int q = 0; q < SRF_CAUSAL_TAPS; ++q) wk[q] = wc[q];
      const float bk = a.b[k][c], ak = a.a[k][0];
      for (int i = sub; i < nout; i += 16) {
        float acc = bk;
#pragma unroll
        for (int q = 0; q < SRF_CAUSAL_TAPS; ++q) acc = fmaf(wk[q], in[stride * i + q], acc);
        outk[i] = srf_prelu(acc, ak);
      }
      if (sub < SRF_STREAM_HIST) a.state[k][srow + sub] = in[nin + sub];   // the last 10 of [state | chunk]
    }
    __syncthreads();
  }
  if (live) {
    float* mr = a.merged + yoff;
    for (int j = sub; j < Lc; j += 16) {
      float acc = row[stream_pyr_off<D>(D, Lc) + (j >> (D - 1))];
#pragma unroll
      for (int k = D - 2; k >= 0; --k) acc = row[stream_pyr_off<D>(k + 1, Lc) + SRF_STREAM_HIST + (j >> k)] + acc;
      mr[j] = acc;
    }
  }
}

static size_t stream_pyr_lds(int D, int Lc) {
  size_t per_row = 0;
  for (int i = 0; i < D; ++i) per_row += SRF_STREAM_HIST + (i == 0 ? Lc : (Lc >> (i - 1)));
  per_row += Lc >> (D - 1);
  return sizeof(float) * per_row * SRF_STREAM_RPW;
}

// max_frames: the largest frames of the launch's rows (what m.max_frames() returns on the device)
template <class M>
static int stream_pyramid_launch(const StreamPyrArgs& a, const M& m, int max_frames, int D, hipStream_t st) {
  const size_t lds = stream_pyr_lds(D, max_frames);
  const long blocks = (a.rows + SRF_STREAM_RPW - 1) / SRF_STREAM_RPW;
  SRF_CHECK_ARG(lds <= SRF_STREAM_LDS_MAX, "srf_causal_stream_pyramid: a chunk of %d frames does not fit LDS at depth %d", max_frames, D);
  SRF_CHECK_ARG(blocks < (1L << 31), "srf_causal_stream_pyramid: too many rows");
  dim3 grid((unsigned)blocks), block(64);
  switch (D) {
    case 1: hipLaunchKernelGGL((srf_stream_pyramid_kernel<1, M>), grid, block, lds, st, a, m); break;
    case 2: hipLaunchKernelGGL((srf_stream_pyramid_kernel<2, M>), grid, block, lds, st, a, m); break;
    case 3: hipLaunchKernelGGL((srf_stream_pyramid_kernel<3, M>), grid, block, lds, st, a, m); break;
    case 4: hipLaunchKernelGGL((srf_stream_pyramid_kernel<4, M>), grid, block, lds, st, a, m); break;
    case 5: hipLaunchKernelGGL((srf_stream_pyramid_kernel<5, M>), grid, block, lds, st, a, m); break;
    case 6: hipLaunchKernelGGL((srf_stream_pyramid_kernel<6, M>), grid, block, lds, st, a, m); break;
    case 7: hipLaunchKernelGGL((srf_stream_pyramid_kernel<7, M>), grid, block, lds, st, a, m); break;
    default: hipLaunchKernelGGL((srf_stream_pyramid_kernel<8, M>), grid, block, lds, st, a, m); break;
  }
  SRF_CHECK_LAUNCH("stream_pyramid", st);
  return SRF_OK;
}

// y1 / merged: [Bt, C, Lc]; state: D pointers to [Bt, C, 10] (read, then overwritten with the last 10 inputs of each level).
extern "C" int srf_causal_stream_pyramid(const float* y1, float* merged, float* const* state, const float* in_prelu,
                                         const float* const* w, const float* const* bias, const float* const* prelu, int Bt,
                                         int C, int Lc, int D, void* stream) {
  SRF_CHECK_ARG(y1 && merged && state && in_prelu && w && bias && prelu, "srf_causal_stream_pyramid: null pointer");
  SRF_CHECK_ARG(Bt > 0 && C > 0, "srf_causal_stream_pyramid: bad sizes Bt=%d C=%d", Bt, C);
  SRF_CHECK_ARG(D >= 1 && D <= SRF_MAX_DEPTH, "srf_causal_stream_pyramid: depth %d unsupported (1..%d)", D, SRF_MAX_DEPTH);
  SRF_CHECK_ARG(Lc > 0 && Lc % (1 << (D - 1)) == 0, "srf_causal_stream_pyramid: chunk of %d frames is not a positive multiple of 2^(D-1) = %d",
                Lc, 1 << (D - 1));
  StreamPyrArgs a;
  a.y1 = y1;
  a.merged = merged;
  a.in_prelu = in_prelu;
  for (int k = 0; k < D; ++k) {
    SRF_CHECK_ARG(state[k] && w[k] && bias[k] && prelu[k], "srf_causal_stream_pyramid: level %d pointer is null", k);
    a.state[k] = state[k];
    a.w[k] = w[k];
    a.b[k] = bias[k];
    a.a[k] = prelu[k];
  }
  a.C = C;
  a.rows = (long)Bt * C;
  const StreamRowsUniform m{Bt, Lc, 0};
  return stream_pyramid_launch(a, m, Lc, D, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// decoder overlap-add.  z[(co K + k)][col0 + l] are the frame values of a row (stream_pw over the transposed decoder weight,
// with mask_nl_class's PReLU applied on load).  Position i of the row's push = sample pos - h + i; frame l covers
// i = h l .. h l + 2h; n = h frames of THIS row.
//   i < n:       out[co,i]  = tail[i] (i <= h) + the frames covering i, ascending l
//   n <= i <= n+h: new tail[i - n] = tail[i] (only where i <= h) + the frames covering i
// Starting from the stored partial sum and adding frames in ascending order gives the same bits wherever the chunk was cut.
// The block (0, 0, row) also rolls the encoder history of the row's slot: no encoder block of this push is still running.
// ---------------------------------------------------------------------------------------------
// sum of position i: the stored partial sum (i <= h) plus the frames covering i, ascending
__device__ __forceinline__ float srf_stream_ola_at(const float* __restrict__ z, const float* tl, int i, int co, int c0, int H, int K,
                                                   int Lc, size_t ld) {
  float acc = i <= H ? tl[i] : 0.f;
  const int l_lo = i < 2 * H ? 0 : (i - H - 1) / H;   // ceil((i - 2h) / h)
  const int l_hi = min(Lc - 1, i / H);
  for (int l = l_lo; l <= l_hi; ++l) acc += z[(size_t)(co * K + i - H * l) * ld + (size_t)c0 + l];
  return acc;
}

// grid (ceil(longest n / 256), S*A, rows).  Block x = 0 is the only reader and writer of its (slot, co) tail (h + 1 <= 256
// entries): it reads all of it before a barrier and writes the new one after it.  Threads with i >= the row's n write nothing.
template <class M>
__global__ __launch_bounds__(256) void srf_stream_ola_kernel(const float* __restrict__ z, float* __restrict__ tail,
                                                             float* __restrict__ out, const float* __restrict__ wav,
                                                             float* __restrict__ hist, int A, int SA, int K, M m) {
  const int H = K / 2;
  const int j = blockIdx.z, co = blockIdx.y;
  const int tid = threadIdx.x;
  const int i = blockIdx.x * 256 + tid;
  const int Lc = m.frames(j), n = H * Lc, sl = m.slot(j), c0 = m.col0(j);
  const size_t ld = m.ncol();
  float* tl = tail + ((size_t)sl * SA + co) * (H + 1);
  if (i < n) out[(size_t)SA * H * c0 + (size_t)co * n + i] = srf_stream_ola_at(z, tl, i, co, c0, H, K, Lc, ld);
  if (blockIdx.x != 0) return;
  const float pend = tid <= H ? srf_stream_ola_at(z, tl, n + tid, co, c0, H, K, Lc, ld) : 0.f;
  __syncthreads();
  if (tid <= H) tl[tid] = pend;
  if (co != 0) return;
  const float* wr = wav + (size_t)A * H * c0;   // this row's [A, n] block
  for (int a = 0; a < A; ++a) {
    float* hr = hist + ((size_t)sl * A + a) * 2 * H;
    const int s = n + tid;   // index into [hist | chunk]
    float v = 0.f;
    if (tid < 2 * H) v = s < 2 * H ? hr[s] : wr[(size_t)a * n + s - 2 * H];
    __syncthreads();
    if (tid < 2 * H) hr[tid] = v;
  }
}

// out[j,co,t] = tail[slot(j),co,t], t < h, for the `rows` rows of the launch: the pending samples as they are (the stream's
// last h samples once zeros were fed)
template <class M>
__global__ __launch_bounds__(256) void srf_stream_flush_kernel(const float* __restrict__ tail, float* __restrict__ out, long rows,
                                                               int SA, int H, M m) {
  const long n = rows * SA * H;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long r = i / H;            // (j, co)
    const int j = (int)(r / SA), co = (int)(r - (long)j * SA);
    out[i] = tail[((size_t)m.slot(j) * SA + co) * (H + 1) + (i - r * H)];
  }
}

// zero `count` floats at p + row * stride for every row in [row_lo, row_hi) of each of `reps` repetitions `rep_stride` apart
__global__ __launch_bounds__(256) void srf_stream_zero_kernel(float* __restrict__ p, long rep_stride, int reps, long row_stride,
                                                              int row_lo, int nrows, long count) {
  const long per_rep = (long)nrows * count, n = per_rep * reps;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long rep = i / per_rep, j = i - rep * per_rep;
    p[rep * rep_stride + (long)row_lo * row_stride + j] = 0.f;   // rows [row_lo, row_lo + nrows) are contiguous
  }
}

// ---------------------------------------------------------------------------------------------
// session
// ---------------------------------------------------------------------------------------------
struct srf_stream {
  srf_config cfg;
  int Bt, max_n, max_lc;
  int A, B, C, U, D, K, N, S, SA, M, h, g;
  SrfCausalLayout lay;         // the parameter order (srf_plan.h)
  std::vector<float> alpha, beta;
  std::vector<size_t> w_off;   // [n_params] float offsets into the prepared weight buffer
  std::vector<long> w_n;       // [n_params] element counts
  size_t weights_floats;
  size_t st_hist, st_dw, st_tail, state_floats;   // float offsets of the three state sections
  size_t ws_enc, ws_xa, ws_xb, ws_y1, ws_merged, ws_masks, ws_z, ws_floats;
};

extern "C" int srf_stream_create(const srf_config* c, int batch, int max_chunk_samples, srf_stream** out) {
  SRF_CHECK_ARG(c && out, "srf_stream_create: null pointer");
  SRF_CHECK_ARG(c->variant == SRF_VARIANT_CAUSAL, "srf_stream_create: only the causal variant streams (variant %d has whole-signal statistics)",
                c->variant);
  SRF_CHECK_ARG(c->in_audio_channels > 0 && c->out_channels > 0 && c->in_channels > 0 && c->num_blocks > 0 &&
                    c->enc_num_basis > 0 && c->num_sources > 0,
                "srf_stream_create: non-positive model dimension");
  SRF_CHECK_ARG(c->group_size == 1, "srf_stream_create: the causal variant has no groups (group_size must be 1, got %d)", c->group_size);
  SRF_CHECK_ARG(c->upsampling_depth >= 1 && c->upsampling_depth <= SRF_MAX_DEPTH, "srf_stream_create: upsampling_depth %d unsupported (1..%d)",
                c->upsampling_depth, SRF_MAX_DEPTH);
  SRF_CHECK_ARG(c->enc_kernel_size >= 3 && (c->enc_kernel_size & 1) && c->enc_kernel_size <= 257,
                "srf_stream_create: enc_kernel_size must be odd and in 3..257 (got %d)", c->enc_kernel_size);
  SRF_CHECK_ARG(batch > 0 && batch <= 65535, "srf_stream_create: batch %d out of range (1..65535)", batch);
  const int D = c->upsampling_depth, U = c->num_blocks, K = c->enc_kernel_size, N = c->enc_num_basis;
  const int h = K / 2, g = h << (D - 1);
  SRF_CHECK_ARG(max_chunk_samples > 0 && max_chunk_samples % g == 0,
                "srf_stream_create: max_chunk_samples %d is not a positive multiple of the granule %d", max_chunk_samples, g);
  const int max_lc = max_chunk_samples / h;
  const int SA = c->num_sources * c->in_audio_channels, SAN = SA * N;
  int cin_max = SAN > c->in_channels ? SAN : c->in_channels;   // widest input of any 1x1 conv (SAN >= N)
  cin_max = cin_max > c->out_channels ? cin_max : c->out_channels;
  SRF_CHECK_ARG(sizeof(float) * (size_t)cin_max * SRF_STREAM_TN <= SRF_STREAM_LDS_MAX,
                "srf_stream_create: %d input channels of a 1x1 conv do not fit the GEMM's LDS tile", cin_max);
  SRF_CHECK_ARG(stream_pyr_lds(D, max_lc) <= SRF_STREAM_LDS_MAX,
                "srf_stream_create: max_chunk_samples %d (%d frames) does not fit the pyramid's LDS; split the push", max_chunk_samples, max_lc);
  SRF_CHECK_ARG(sizeof(float) * (size_t)c->in_audio_channels * (7 * h + K) <= SRF_STREAM_LDS_MAX, "srf_stream_create: encoder window does not fit LDS (A=%d K=%d)",
                c->in_audio_channels, K);
  SRF_CHECK_ARG(((long)batch * max_lc + SRF_STREAM_TN - 1) / SRF_STREAM_TN <= 65535,
                "srf_stream_create: batch %d x max_chunk_samples %d is too many columns for one launch", batch, max_chunk_samples);
  srf_stream* s = new (std::nothrow) srf_stream();
  SRF_CHECK_ARG(s != nullptr, "srf_stream_create: out of host memory");
  s->cfg = *c;
  s->Bt = batch; s->max_n = max_chunk_samples; s->max_lc = max_lc;
  s->A = c->in_audio_channels; s->B = c->out_channels; s->C = c->in_channels; s->U = U; s->D = D; s->K = K; s->N = N;
  s->S = c->num_sources; s->SA = SA; s->M = SA * K; s->h = h; s->g = g;
  s->lay = causal_layout(U, D);
  const int n_params = s->lay.n_params;
  s->alpha.assign(U, 1.f);
  s->beta.assign(U, 1.f);
  // prepared weights: one slot per parameter in state_dict order (64-float aligned); decoder.weight's slot holds its transpose
  s->w_n.assign(n_params, 0);
  std::vector<long*> wn(n_params);
  for (int p = 0; p < n_params; ++p) wn[p] = &s->w_n[p];
  const SrfCausalFront<long> nf = causal_front<long>(wn);
  *nf.enc_w = (long)N * s->A * (2 * K - 1), *nf.bott_w = (long)s->B * N, *nf.bott_b = s->B;
  for (int i = 0; i < U; ++i) {
    const SrfCausalBlock<long> nb = causal_block<long>(s->lay, wn, i);
    *nb.gain = 1, *nb.proj_w = (long)s->C * s->B, *nb.proj_b = s->C, *nb.proj_prelu = 1;
    for (int k = 0; k < D; ++k) *nb.lv_w[k] = (long)s->C * SRF_CAUSAL_KW, *nb.lv_b[k] = s->C, *nb.lv_prelu[k] = 1;
    *nb.res_w = (long)s->B * s->C, *nb.res_b = s->B;
  }
  const SrfCausalTail<long> nt = causal_tail<long>(s->lay, wn);
  *nt.mask_prelu = 1, *nt.mask_w = (long)SAN * s->B, *nt.mask_b = SAN, *nt.dec_w = (long)SAN * s->M, *nt.out_prelu = 1;
  s->w_off.assign(n_params, 0);
  size_t off = 0;
  for (int p = 0; p < n_params; ++p) {
    s->w_off[p] = off;
    off += srf_align_up((size_t)s->w_n[p], 64);
  }
  s->weights_floats = off;
  // state: three sections, each 64-float aligned
  s->st_hist = 0;
  s->st_dw = srf_align_up((size_t)batch * s->A * 2 * h, 64);
  s->st_tail = s->st_dw + srf_align_up((size_t)U * D * batch * s->C * SRF_STREAM_HIST, 64);
  s->state_floats = s->st_tail + srf_align_up((size_t)batch * SA * (h + 1), 64);
  // workspace
  const size_t ncol = (size_t)batch * max_lc;
  off = 0;
  auto take = [&](size_t f) { const size_t o = off; off += srf_align_up(f, 64); return o; };
  s->ws_enc = take((size_t)N * ncol);
  s->ws_xa = take((size_t)s->B * ncol);
  s->ws_xb = take((size_t)s->B * ncol);
  s->ws_y1 = take((size_t)s->C * ncol);
  s->ws_merged = take((size_t)s->C * ncol);
  s->ws_masks = take((size_t)SAN * ncol);
  s->ws_z = take((size_t)s->M * ncol);
  s->ws_floats = off;
  *out = s;
  return SRF_OK;
}

extern "C" void srf_stream_destroy(srf_stream* s) { delete s; }
extern "C" int srf_stream_granule(const srf_stream* s) { return s ? s->g : 0; }
extern "C" int srf_stream_delay(const srf_stream* s) { return s ? s->h : 0; }
extern "C" size_t srf_stream_state_bytes(const srf_stream* s) { return s ? sizeof(float) * s->state_floats : 0; }
extern "C" size_t srf_stream_weights_bytes(const srf_stream* s) { return s ? sizeof(float) * s->weights_floats : 0; }
extern "C" size_t srf_stream_workspace_bytes(const srf_stream* s) { return s ? sizeof(float) * s->ws_floats : 0; }
extern "C" int srf_stream_num_launches(const srf_stream* s) { return s ? 3 * s->U + 5 : 0; }

extern "C" int srf_stream_set_block_scales(srf_stream* s, const float* alpha, const float* beta, int n) {
  SRF_CHECK_ARG(s && alpha && beta, "srf_stream_set_block_scales: null pointer");
  SRF_CHECK_ARG(n == s->U, "srf_stream_set_block_scales: expected %d blocks, got %d", s->U, n);
  for (int i = 0; i < n; ++i) SRF_CHECK_ARG(beta[i] != 0.f, "srf_stream_set_block_scales: beta[%d] is zero", i);
  s->alpha.assign(alpha, alpha + n);
  s->beta.assign(beta, beta + n);
  return SRF_OK;
}

// Snapshot of the weights as a push uses them: every parameter copied, skipinit_gain * alpha (the gain read on the DEVICE)
// folded into res_conv's weight and bias, 1 / beta into proj_1x1's weight, the decoder weight transposed to [Co K][Ci].
extern "C" int srf_stream_prepare(const srf_stream* s, const float* const* P, int num_params, void* weights_buf, void* stream) {
  SRF_CHECK_ARG(s && P && weights_buf, "srf_stream_prepare: null pointer");
  SRF_CHECK_ARG(num_params == s->lay.n_params, "srf_stream_prepare: expected %d parameters, got %d", s->lay.n_params, num_params);
  SRF_CHECK_ARG(((size_t)weights_buf & 255) == 0, "srf_stream_prepare: weights_buf %p is not 256-byte aligned", weights_buf);
  for (int p = 0; p < num_params; ++p) SRF_CHECK_ARG(P[p] != nullptr, "srf_stream_prepare: parameter %d is null", p);
  float* wb = (float*)weights_buf;
  hipStream_t st = (hipStream_t)stream;
  // per parameter: the device scalar and the host factor it is copied with (skipinit_gain * alpha, 1 / beta; else 1)
  std::vector<const float*> gain_of(num_params, nullptr);
  std::vector<float> factor_of(num_params, 1.f);
  for (int i = 0; i < s->U; ++i) {
    const SrfCausalBlock<const float> b = causal_block<const float>(s->lay, P, i);
    factor_of[b.i_proj] = 1.f / s->beta[i];
    gain_of[b.i_res] = gain_of[b.i_res + 1] = b.gain;      // res_conv weight and bias
    factor_of[b.i_res] = factor_of[b.i_res + 1] = s->alpha[i];
  }
  std::vector<const float*> src, dsc;
  std::vector<float*> dst;
  std::vector<long> cnt;
  std::vector<float> hs;
  const int dec = causal_p_dec(s->lay);      // transposed below
  for (int p = 0; p < num_params; ++p) {
    if (p == dec) continue;
    src.push_back(P[p]); dst.push_back(wb + s->w_off[p]); cnt.push_back(s->w_n[p]); dsc.push_back(gain_of[p]); hs.push_back(factor_of[p]);
  }
  int rc = srf_causal_scale_many(src.data(), dst.data(), cnt.data(), dsc.data(), hs.data(), (int)src.size(), st);
  if (rc) return rc;
  return srf_transpose_launch(P[dec], wb + s->w_off[dec], s->SA * s->N, s->M, st);
}

extern "C" int srf_stream_reset(const srf_stream* s, void* state, int row, void* stream) {
  SRF_CHECK_ARG(s && state, "srf_stream_reset: null pointer");
  SRF_CHECK_ARG(((size_t)state & 255) == 0, "srf_stream_reset: state %p is not 256-byte aligned", state);
  SRF_CHECK_ARG(row >= -1 && row < s->Bt, "srf_stream_reset: row %d out of range (-1 = all, 0..%d)", row, s->Bt - 1);
  float* sp = (float*)state;
  hipStream_t st = (hipStream_t)stream;
  const int lo = row < 0 ? 0 : row, nr = row < 0 ? s->Bt : 1;
  struct Sec { float* p; long rep_stride; int reps; long row_stride; };
  const Sec secs[3] = {{sp + s->st_hist, 0, 1, (long)s->A * 2 * s->h},
                       {sp + s->st_dw, (long)s->Bt * s->C * SRF_STREAM_HIST, s->U * s->D, (long)s->C * SRF_STREAM_HIST},
                       {sp + s->st_tail, 0, 1, (long)s->SA * (s->h + 1)}};
  for (const Sec& e : secs) {
    const long n = (long)nr * e.row_stride * e.reps, blocks = (n + 255) / 256;
    hipLaunchKernelGGL(srf_stream_zero_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, st, e.p, e.rep_stride,
                       e.reps, e.row_stride, lo, nr, e.row_stride);
    SRF_CHECK_LAUNCH("stream_reset", st);
  }
  return SRF_OK;
}

// The launches of one push.  ncol columns in all; the encoder, the pyramids and the overlap-add go out once per group of rows
// (mapper grp[i], its largest frames maxf[i], its rows nrows[i]), the 1x1 GEMMs once over all columns.
template <class M>
static int stream_forward(const srf_stream* s, const float* wb, float* sp, const float* wav, float* out, float* ws, long ncol,
                          const M* grp, const int* maxf, const int* nrows, int ngrp, hipStream_t st) {
  const int D = s->D;
  const SrfOffsetTable<const float> W{wb, s->w_off.data()};
  const SrfCausalFront<const float> f = causal_front<const float>(W);
  const SrfCausalTail<const float> t = causal_tail<const float>(s->lay, W);
  float* enc = ws + s->ws_enc;
  float* cur = ws + s->ws_xa;
  float* nxt = ws + s->ws_xb;
  float* y1 = ws + s->ws_y1;
  float* merged = ws + s->ws_merged;
  float* masks = ws + s->ws_masks;
  float* z = ws + s->ws_z;
  float* hist = sp + s->st_hist;
  for (int gi = 0; gi < ngrp; ++gi) {
    const size_t lds = sizeof(float) * (size_t)s->A * (7 * s->h + s->K);
    hipLaunchKernelGGL(srf_stream_enc_kernel<M>, dim3((s->N + 31) / 32, (maxf[gi] + 7) / 8, nrows[gi]), dim3(256), lds, st, wav,
                       hist, f.enc_w, enc, s->A, s->N, s->K, grp[gi]);
    SRF_CHECK_LAUNCH("stream_encoder", st);
  }
  int rc = stream_pw(enc, f.bott_w, f.bott_b, nullptr, nullptr, cur, s->N, s->B, ncol, st);
  if (rc) return rc;
  for (int i = 0; i < s->U; ++i) {
    const SrfCausalBlock<const float> b = causal_block<const float>(s->lay, W, i);
    rc = stream_pw(cur, b.proj_w, b.proj_b, nullptr, nullptr, y1, s->B, s->C, ncol, st);
    if (rc) return rc;
    StreamPyrArgs a;
    a.y1 = y1;
    a.merged = merged;
    a.in_prelu = b.proj_prelu;
    for (int k = 0; k < D; ++k) {
      a.state[k] = sp + s->st_dw + ((size_t)i * D + k) * s->Bt * s->C * SRF_STREAM_HIST;
      a.w[k] = b.lv_w[k], a.b[k] = b.lv_b[k], a.a[k] = b.lv_prelu[k];
    }
    a.C = s->C;
    for (int gi = 0; gi < ngrp; ++gi) {
      a.rows = (long)nrows[gi] * s->C;
      rc = stream_pyramid_launch(a, grp[gi], maxf[gi], D, st);
      if (rc) return rc;
    }
    rc = stream_pw(merged, b.res_w, b.res_b, nullptr, cur, nxt, s->C, s->B, ncol, st);
    if (rc) return rc;
    float* tmp = cur;
    cur = nxt;
    nxt = tmp;
  }
  rc = stream_pw(cur, t.mask_w, t.mask_b, t.mask_prelu, nullptr, masks, s->B, s->SA * s->N, ncol, st);
  if (rc) return rc;
  rc = stream_pw(masks, t.dec_w, nullptr, t.out_prelu, nullptr, z, s->SA * s->N, s->M, ncol, st);
  if (rc) return rc;
  for (int gi = 0; gi < ngrp; ++gi) {
    hipLaunchKernelGGL(srf_stream_ola_kernel<M>, dim3((s->h * maxf[gi] + 255) / 256, s->SA, nrows[gi]), dim3(256), 0, st, z,
                       sp + s->st_tail, out, wav, hist, s->A, s->SA, s->K, grp[gi]);
    SRF_CHECK_LAUNCH("stream_ola", st);
  }
  return SRF_OK;
}

extern "C" int srf_stream_push(const srf_stream* s, const void* weights_buf, void* state, const float* wav, int n, float* out,
                               void* workspace, size_t workspace_bytes, void* stream) {
  SRF_CHECK_ARG(s && weights_buf && state && wav && out && workspace, "srf_stream_push: null pointer");
  SRF_CHECK_ARG(n > 0, "srf_stream_push: n = %d samples (must be positive)", n);
  SRF_CHECK_ARG(n % s->g == 0, "srf_stream_push: n = %d is not a multiple of the granule %d", n, s->g);
  SRF_CHECK_ARG(n <= s->max_n, "srf_stream_push: n = %d exceeds the session's max_chunk_samples %d", n, s->max_n);
  SRF_CHECK_ARG(workspace_bytes >= sizeof(float) * s->ws_floats, "srf_stream_push: workspace of %zu bytes is too small (need %zu)",
                workspace_bytes, sizeof(float) * s->ws_floats);
  SRF_CHECK_ARG((((size_t)weights_buf | (size_t)state | (size_t)workspace) & 255) == 0,
                "srf_stream_push: weights_buf %p, state %p and workspace %p must be 256-byte aligned", weights_buf, state, workspace);
  const int Lc = n / s->h;
  const StreamRowsUniform m{s->Bt, Lc, 1};
  return stream_forward(s, (const float*)weights_buf, (float*)state, wav, out, (float*)workspace, (long)s->Bt * Lc, &m, &Lc,
                        &s->Bt, 1, (hipStream_t)stream);
}

extern "C" int srf_stream_push_rows_num_launches(const srf_stream* s, int m) {
  if (!s || m < 1) return 0;
  const int groups = (m + SRF_STREAM_ROWS_PER_LAUNCH - 1) / SRF_STREAM_ROWS_PER_LAUNCH;
  return 2 * s->U + 3 + groups * (s->U + 2);
}

// One push for any subset of the session's streams, each with its own number of granules.  rows is a HOST array; everything a
// kernel will index with is checked here, and the row tables travel as kernel arguments (no device-side table, no copy).
extern "C" int srf_stream_push_rows(const srf_stream* s, const void* weights_buf, void* state, const srf_stream_row* rows, int m,
                                    const float* wav, float* out, void* workspace, size_t workspace_bytes, void* stream) {
  SRF_CHECK_ARG(s && weights_buf && state && rows && wav && out && workspace, "srf_stream_push_rows: null pointer");
  SRF_CHECK_ARG(m >= 1 && m <= s->Bt, "srf_stream_push_rows: m = %d rows out of range (1..%d, the session's batch)", m, s->Bt);
  SRF_CHECK_ARG(workspace_bytes >= sizeof(float) * s->ws_floats, "srf_stream_push_rows: workspace of %zu bytes is too small (need %zu)",
                workspace_bytes, sizeof(float) * s->ws_floats);
  SRF_CHECK_ARG((((size_t)weights_buf | (size_t)state | (size_t)workspace) & 255) == 0,
                "srf_stream_push_rows: weights_buf %p, state %p and workspace %p must be 256-byte aligned", weights_buf, state, workspace);
  const int ngrp = (m + SRF_STREAM_ROWS_PER_LAUNCH - 1) / SRF_STREAM_ROWS_PER_LAUNCH;
  std::vector<unsigned char> seen((size_t)s->Bt, 0);
  std::vector<StreamRowsTable> grp((size_t)ngrp);
  std::vector<int> maxf((size_t)ngrp, 0), nrows((size_t)ngrp, 0);
  long ncol = 0;
  for (int j = 0; j < m; ++j) {
    const int slot = rows[j].slot, n = rows[j].n;
    SRF_CHECK_ARG(slot >= 0 && slot < s->Bt, "srf_stream_push_rows: row %d: slot %d out of range (0..%d)", j, slot, s->Bt - 1);
    SRF_CHECK_ARG(!seen[slot], "srf_stream_push_rows: row %d: slot %d is listed twice (two rows would race on one state)", j, slot);
    SRF_CHECK_ARG(n > 0, "srf_stream_push_rows: row %d: n = %d samples (must be positive)", j, n);
    SRF_CHECK_ARG(n % s->g == 0, "srf_stream_push_rows: row %d: n = %d is not a multiple of the granule %d", j, n, s->g);
    SRF_CHECK_ARG(n <= s->max_n, "srf_stream_push_rows: row %d: n = %d exceeds the session's max_chunk_samples %d", j, n, s->max_n);
    seen[slot] = 1;
    const int gi = j / SRF_STREAM_ROWS_PER_LAUNCH, q = j % SRF_STREAM_ROWS_PER_LAUNCH, frames = n / s->h;
    StreamRowsTable& t = grp[gi];
    t.slot_[q] = slot;
    t.col0_[q] = (int)ncol;        // m <= batch rows of at most max_lc frames: ncol <= batch * max_lc, which create bounds
    t.frames_[q] = frames;
    ncol += frames;
    nrows[gi] = q + 1;
    if (frames > maxf[gi]) maxf[gi] = frames;
  }
  for (int gi = 0; gi < ngrp; ++gi) {
    StreamRowsTable& t = grp[gi];
    for (int q = nrows[gi]; q < SRF_STREAM_ROWS_PER_LAUNCH; ++q) t.slot_[q] = t.col0_[q] = t.frames_[q] = 0;   // never indexed
    t.rows = nrows[gi];
    t.max_frames_ = maxf[gi];
    t.ncol_ = (int)ncol;
  }
  return stream_forward(s, (const float*)weights_buf, (float*)state, wav, out, (float*)workspace, ncol, grp.data(), maxf.data(),
                        nrows.data(), ngrp, (hipStream_t)stream);
}

extern "C" int srf_stream_flush(const srf_stream* s, const void* state, float* out_tail, void* stream) {
  SRF_CHECK_ARG(s && state && out_tail, "srf_stream_flush: null pointer");
  SRF_CHECK_ARG(((size_t)state & 255) == 0, "srf_stream_flush: state %p is not 256-byte aligned", state);
  const long n = (long)s->Bt * s->SA * s->h, blocks = (n + 255) / 256;
  hipStream_t st = (hipStream_t)stream;
  const StreamRowsUniform m{s->Bt, 0, 0};
  hipLaunchKernelGGL(srf_stream_flush_kernel<StreamRowsUniform>, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, st,
                     (const float*)state + s->st_tail, out_tail, (long)s->Bt, s->SA, s->h, m);
  SRF_CHECK_LAUNCH("stream_flush", st);
  return SRF_OK;
}

// out_tail[j] = the pending h samples of slots[j] (a HOST array), j < m; the state is left unchanged
extern "C" int srf_stream_flush_rows(const srf_stream* s, const void* state, const int* slots, int m, float* out_tail, void* stream) {
  SRF_CHECK_ARG(s && state && slots && out_tail, "srf_stream_flush_rows: null pointer");
  SRF_CHECK_ARG(((size_t)state & 255) == 0, "srf_stream_flush_rows: state %p is not 256-byte aligned", state);
  SRF_CHECK_ARG(m >= 1 && m <= s->Bt, "srf_stream_flush_rows: m = %d rows out of range (1..%d, the session's batch)", m, s->Bt);
  for (int j = 0; j < m; ++j)
    SRF_CHECK_ARG(slots[j] >= 0 && slots[j] < s->Bt, "srf_stream_flush_rows: row %d: slot %d out of range (0..%d)", j, slots[j], s->Bt - 1);
  hipStream_t st = (hipStream_t)stream;
  for (int j0 = 0; j0 < m; j0 += SRF_STREAM_ROWS_PER_LAUNCH) {
    StreamRowsTable t = {};
    t.rows = m - j0 < SRF_STREAM_ROWS_PER_LAUNCH ? m - j0 : SRF_STREAM_ROWS_PER_LAUNCH;
    for (int q = 0; q < t.rows; ++q) t.slot_[q] = slots[j0 + q];
    const long n = (long)t.rows * s->SA * s->h, blocks = (n + 255) / 256;
    hipLaunchKernelGGL(srf_stream_flush_kernel<StreamRowsTable>, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, st,
                       (const float*)state + s->st_tail, out_tail + (size_t)j0 * s->SA * s->h, (long)t.rows, s->SA, s->h, t);
    SRF_CHECK_LAUNCH("stream_flush", st);
  }
  return SRF_OK;
}
