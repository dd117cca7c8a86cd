// Causal SuDoRM-RF (v3) training step, device side: srf_causal_forward_train keeps what the backward
// needs, srf_causal_backward turns d loss / d output into every parameter gradient -- torch autograd over the reference's
// CausalSuDORMRF.forward (causal_improved_sudormrf_v3.py), as sequences of this library's per-kernel entry points.  Opt-in: the
// general training entry points (srf_train.hip) keep refusing causal plans.
//   saved   : encoder output | residual stream x_0 .. x_U | per block: proj_1x1's pre-activation u, the D pre-activations d_k of
//             the pyramid, merged | mask_net's output m (pre mask_nl_class).  Pre-activations, because a PReLU slope may be zero
//             or negative and the sign of the activated value then no longer tells the branch.
//   grads   : WRITTEN (not accumulated into), same order and shapes as the parameters.
#include "srf_plan.h"

namespace {

struct CTrainLayout {
  size_t enc, x0, x_stride, blk0, blk_stride, u, lv[SRF_MAX_DEPTH], merged, m, total;
};

CTrainLayout ctrain_layout(const srf_plan* p) {
  CTrainLayout t{};
  const srf_config& c = p->cfg;
  const size_t F = sizeof(float), L = p->L, Bt = p->Bt;
  const int D = c.upsampling_depth, U = c.num_blocks;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t o = off;
    off = srf_align_up(off + bytes, 256);
    return o;
  };
  t.enc = take(F * Bt * c.enc_num_basis * L);
  t.x_stride = srf_align_up(F * Bt * c.out_channels * L, 256);
  t.x0 = take(t.x_stride * (U + 1));
  size_t rel = 0;
  auto rtake = [&](size_t bytes) {
    const size_t o = rel;
    rel = srf_align_up(rel + bytes, 256);
    return o;
  };
  t.u = rtake(F * Bt * c.in_channels * L);
  for (int k = 0; k < D; ++k) t.lv[k] = rtake(F * Bt * c.in_channels * (L >> k));
  t.merged = rtake(F * Bt * c.in_channels * L);
  t.blk_stride = rel;
  t.blk0 = take(rel * U);
  t.m = take(F * Bt * p->SA * c.enc_num_basis * L);
  t.total = off;
  return t;
}

struct CScratchLayout {
  size_t dec, gv, genc, gxa, gxb, gm, gu, gd[SRF_MAX_DEPTH], frames, wt, zeros, wdpad, wg, pyr, fold_res, fold_proj, encw, pk3,
      pkT, total;
  size_t res_floats, zero_floats;
  int dec_rows;
};

size_t cmax(size_t a, size_t b) { return a > b ? a : b; }

CScratchLayout cscratch_layout(const srf_plan* p) {
  CScratchLayout s{};
  const srf_config& c = p->cfg;
  const size_t F = sizeof(float), L = p->L, Bt = p->Bt;
  const int D = c.upsampling_depth, U = c.num_blocks, K = c.enc_kernel_size, N = c.enc_num_basis, B = c.out_channels,
            C = c.in_channels;
  const int SAN = p->SA * N;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t o = off;
    off = srf_align_up(off + (bytes ? bytes : 1), 256);
    return o;
  };
  s.dec = take(F * srf_decoder_scratch_floats(p->Bt, SAN, p->SA, K, p->L));
  s.gv = take(F * Bt * SAN * L);
  s.genc = take(F * Bt * N * L);
  s.gxa = take(F * Bt * B * L);
  s.gxb = take(F * Bt * B * L);
  s.gm = take(F * Bt * C * L);
  s.gu = take(F * Bt * C * L);
  for (int k = 0; k < D; ++k) s.gd[k] = take(F * Bt * C * (L >> k));
  s.dec_rows = (p->SA * K + 63) / 64 * 64;
  const size_t enc_rows = (size_t)p->A * K;
  s.frames = take(F * Bt * L * cmax((size_t)s.dec_rows, enc_rows));
  s.wt = take(F * cmax(cmax((size_t)B * N, (size_t)B * C), (size_t)B * SAN));
  s.zero_floats = cmax(cmax(C, SAN), cmax(N, B));
  s.zeros = take(F * s.zero_floats);
  s.wdpad = take(F * (size_t)SAN * s.dec_rows);
  size_t wg = 0;
  auto wgmax = [&](int cout, int cin) { wg = cmax(wg, srf_pw_wgrad_scratch_bytes(p->Bt, cout, cin, p->L)); };
  wgmax(B, N);
  wgmax(SAN, B);
  wgmax(SAN, s.dec_rows);
  wgmax(N, (int)enc_rows);
  wgmax(C, B);
  wgmax(B, C);
  s.wg = take(wg);
  s.pyr = take(cmax(cmax(srf_causal_pyramid_bwd_scratch_bytes(p->Bt, C, p->L, D), srf_causal_dwconv_bwd_scratch_bytes(p->Bt, C, p->L)),
                    F * srf_causal_prelu_bwd_scratch_floats()));
  s.res_floats = srf_align_up((size_t)B * C, 64) + srf_align_up((size_t)B, 64);
  s.fold_res = take(F * s.res_floats * U);
  s.fold_proj = take(F * (size_t)C * B * U);
  s.encw = take(F * (size_t)N * enc_rows);
  {
    size_t pk = srf_align_up(srf_packed3_pw_weight_bytes(B, N), 256) + srf_align_up(srf_packed3_pw_weight_bytes(SAN, B), 256);
    pk += (size_t)U * srf_align_up(srf_packed3_pw_weight_bytes(C, B), 256);
    s.pk3 = take(pk);
  }
  {
    size_t pk = srf_align_up(srf_packed_pw_weight_bytes(B, SAN), 256) + srf_align_up(srf_packed_pw_weight_bytes(N, B), 256);
    pk += (size_t)U * (srf_align_up(srf_packed_pw_weight_bytes(C, B), 256) + srf_align_up(srf_packed_pw_weight_bytes(B, C), 256));
    s.pkT = take(pk);
  }
  s.total = off;
  return s;
}

bool causal_plan(const srf_plan* p, const char* who) {
  if (p && p->cfg.variant == SRF_VARIANT_CAUSAL) return true;
  srf_set_error("%s: %s", who, p ? "causal plans only (the other models train through srf_forward_train / srf_backward)" : "null plan");
  return false;
}

int ctrain_check(const srf_plan* p, const char* who) {
  if (p->L % 4 != 0) {      // (the weight-gradient GEMM's limit; only D = 1 models can miss it)
    srf_set_error("%s: L=%d must be a multiple of 4", who, p->L);
    return SRF_EINVAL;
  }
  return SRF_OK;
}

// res_conv weight / bias * (skipinit_gain * alpha) for every block, proj_1x1 weight / beta where beta != 1 (as srf_forward)
int ctrain_fold(const srf_plan* p, const float* const* P, const CScratchLayout& s, char* sc, std::vector<const float*>& wproj,
                std::vector<const float*>& wres, std::vector<const float*>& bres, hipStream_t st) {
  const int D = p->cfg.upsampling_depth, U = p->cfg.num_blocks, B = p->nB, Cc = p->nC;
  std::vector<const float*> fsrc, fscale;
  std::vector<float*> fdst;
  std::vector<long> fn;
  std::vector<float> fh;
  wproj.assign(U, nullptr);
  wres.assign(U, nullptr);
  bres.assign(U, nullptr);
  for (int i = 0; i < U; ++i) {
    const float* const* Pb = P + p->p_block0 + (size_t)i * p->p_block_stride;
    float* rw = (float*)(sc + s.fold_res) + (size_t)i * s.res_floats;
    float* rb = rw + srf_align_up((size_t)B * Cc, 64);
    fsrc.push_back(Pb[4 + 3 * D]); fdst.push_back(rw); fn.push_back((long)B * Cc); fscale.push_back(Pb[0]); fh.push_back(p->alpha[i]);
    fsrc.push_back(Pb[5 + 3 * D]); fdst.push_back(rb); fn.push_back((long)B); fscale.push_back(Pb[0]); fh.push_back(p->alpha[i]);
    wres[i] = rw;
    bres[i] = rb;
    wproj[i] = Pb[1];
    if (p->beta[i] != 1.f) {
      float* pw = (float*)(sc + s.fold_proj) + (size_t)i * Cc * B;
      fsrc.push_back(Pb[1]); fdst.push_back(pw); fn.push_back((long)Cc * B); fscale.push_back(nullptr); fh.push_back(1.f / p->beta[i]);
      wproj[i] = pw;
    }
  }
  return srf_causal_scale_many(fsrc.data(), fdst.data(), fn.data(), fscale.data(), fh.data(), (int)fsrc.size(), st);
}

int cforward_train_impl(const srf_plan* p, const float* const* P, const float* wav, float* out, void* saved, void* scratch,
                        bool split_tail, void* stream) {
  const CTrainLayout t = ctrain_layout(p);
  const CScratchLayout s = cscratch_layout(p);
  const srf_config& c = p->cfg;
  const int D = c.upsampling_depth, U = c.num_blocks, N = c.enc_num_basis, K = c.enc_kernel_size;
  const int Bt = p->Bt, L = p->L, B = p->nB, Cc = p->nC, SAN = p->SA * N;
  char* sv = (char*)saved;
  char* sc = (char*)scratch;
  hipStream_t st = (hipStream_t)stream;
  auto xbuf = [&](int i) { return (float*)(sv + t.x0 + t.x_stride * i); };
  std::vector<const float*> wproj, wres, bres;
  int rc = ctrain_fold(p, P, s, sc, wproj, wres, bres, st);
  if (rc) return rc;
  // three-part (or two-fp16-part) images of the 1x1 weights the 256 x 128 GEMM takes, as forward_train_impl packs them
  const bool three = srf_kernel_mode() == 2 && !srf_dbg(SRF_DBG_TRAIN_FWD_EXACT_MFMA);
  std::vector<const float*> pk_w;
  std::vector<void*> pk_d;
  std::vector<int> pk_co, pk_ci;
  size_t pk_off = s.pk3;
  auto pack3 = [&](const float* w, int cout, int cin) -> const void* {
    const size_t bytes = srf_packed3_pw_weight_bytes(cout, cin);
    if (!three || !bytes) return nullptr;
    void* d = sc + pk_off;
    pk_off += srf_align_up(bytes, 256);
    pk_w.push_back(w);
    pk_d.push_back(d);
    pk_co.push_back(cout);
    pk_ci.push_back(cin);
    return d;
  };
  const float* const* Pt = P + p->p_tail;
  const void* pk_bott = pack3(P[1], B, N);
  const void* pk_mask = pack3(Pt[1], SAN, B);
  std::vector<const void*> pk_proj(U, nullptr);
  for (int i = 0; i < U; ++i) pk_proj[i] = pack3(wproj[i], Cc, B);
  if (!pk_w.empty()) {
    rc = srf_pack3_pw_weights(pk_w.data(), pk_d.data(), pk_co.data(), pk_ci.data(), (int)pk_w.size(), stream);
    if (rc) return rc;
  }
  float* enc = (float*)(sv + t.enc);
  rc = srf_causal_encoder(wav, P[0], enc, Bt, p->A, p->T, N, K, L, stream);
  if (rc) return rc;
  rc = srf_pw_conv_packed3(enc, P[1], pk_bott, P[2], xbuf(0), Bt, N, B, L, nullptr, nullptr, nullptr, stream);
  if (rc) return rc;
  for (int i = 0; i < U; ++i) {
    const float* const* Pb = P + p->p_block0 + (size_t)i * p->p_block_stride;
    char* blk = sv + t.blk0 + t.blk_stride * i;
    float* u = (float*)(blk + t.u);
    float* merged = (float*)(blk + t.merged);
    rc = srf_pw_conv_packed3(xbuf(i), wproj[i], pk_proj[i], Pb[2], u, Bt, B, Cc, L, nullptr, nullptr, nullptr, stream);
    if (rc) return rc;
    // the per-level kernels with the activation moved to the consumer's load: d_k is stored BEFORE its PReLU
    const float *dv[SRF_MAX_DEPTH], *av[SRF_MAX_DEPTH];
    for (int k = 0; k < D; ++k) {
      float* dk = (float*)(blk + t.lv[k]);
      rc = srf_causal_dwconv(k == 0 ? u : dv[k - 1], Pb[4 + 3 * k], Pb[5 + 3 * k], k == 0 ? Pb[3] : Pb[6 + 3 * (k - 1)], nullptr, dk,
                             Bt, Cc, k == 0 ? L : (L >> (k - 1)), k == 0 ? 1 : 2, stream);
      if (rc) return rc;
      dv[k] = dk;
      av[k] = Pb[6 + 3 * k];
    }
    rc = srf_causal_merge_act(dv, av, D, merged, Bt, Cc, L, st);
    if (rc) return rc;
    rc = srf_pw_conv_packed3(merged, wres[i], nullptr, bres[i], xbuf(i + 1), Bt, Cc, B, L, nullptr, xbuf(i), nullptr, stream);
    if (rc) return rc;
  }
  float* m = (float*)(sv + t.m);
  {
    srf_norm pre{nullptr, nullptr, nullptr, Pt[0]};
    rc = srf_pw_conv_packed3(xbuf(U), Pt[1], pk_mask, Pt[2], m, Bt, B, SAN, L, &pre, nullptr, nullptr, stream);
    if (rc) return rc;
  }
  float* v = (float*)(sc + s.gv);
  rc = srf_prelu_apply(m, Pt[4], v, (long)Bt * SAN * L, stream);
  if (rc) return rc;
  // the decoder's frame GEMM is the last linear map: on the split kernel when the exact class was this call's own choice
  const int tail_prev = split_tail ? srf_kernel_mode_override(0) : -1;
  rc = srf_decoder(v, Pt[3], out, Bt, SAN, p->SA, K, L, p->T, (float*)(sc + s.dec), stream);
  if (split_tail) srf_kernel_mode_override(tail_prev);
  return rc;
}

}  // namespace

extern "C" size_t srf_causal_train_saved_bytes(const srf_plan* p) {
  return causal_plan(p, "srf_causal_train_saved_bytes") ? ctrain_layout(p).total : 0;
}
extern "C" size_t srf_causal_train_scratch_bytes(const srf_plan* p) {
  return causal_plan(p, "srf_causal_train_scratch_bytes") ? cscratch_layout(p).total : 0;
}

extern "C" int srf_causal_forward_train(const srf_plan* p, const float* const* P, int num_params, const float* wav, float* out,
                                        void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes, void* stream) {
  if (!causal_plan(p, "srf_causal_forward_train")) return SRF_EINVAL;
  SRF_CHECK_ARG(P && wav && out && saved && scratch, "srf_causal_forward_train: null pointer");
  SRF_CHECK_ARG(num_params == p->n_params, "srf_causal_forward_train: expected %d parameter tensors, got %d", p->n_params, num_params);
  int rc = ctrain_check(p, "srf_causal_forward_train");
  if (rc) return rc;
  for (int i = 0; i < num_params; ++i) SRF_CHECK_ARG(P[i] != nullptr, "srf_causal_forward_train: parameter %d is null", i);
  SRF_CHECK_ARG(saved_bytes >= ctrain_layout(p).total && scratch_bytes >= cscratch_layout(p).total,
                "srf_causal_forward_train: saved / scratch buffer too small");
  SRF_CHECK_ARG(((((size_t)saved) | ((size_t)scratch)) & 255) == 0, "srf_causal_forward_train: buffers must be 256-byte aligned");
  // the exact-fp32 class for the 1x1 convolutions, under the flags of srf_forward_train (srf_train.hip has the reasons)
  const bool exact = srf_kernel_mode() == 0 && !srf_dbg(SRF_DBG_TRAIN_FWD_SPLIT_BF16);
  const int prev = exact ? srf_kernel_mode_override(2) : -1;
  if (srf_profiling()) srf_prof_mark("(gap)", (hipStream_t)stream);
  rc = cforward_train_impl(p, P, wav, out, saved, scratch, exact, stream);
  if (exact) srf_kernel_mode_override(prev);
  return rc;
}

extern "C" int srf_causal_backward(const srf_plan* p, const float* const* P, float* const* G, int num_params, const float* wav,
                                   const float* grad_out, const void* saved, size_t saved_bytes, void* scratch,
                                   size_t scratch_bytes, void* stream) {
  if (!causal_plan(p, "srf_causal_backward")) return SRF_EINVAL;
  SRF_CHECK_ARG(P && G && wav && grad_out && saved && scratch, "srf_causal_backward: null pointer");
  SRF_CHECK_ARG(num_params == p->n_params, "srf_causal_backward: expected %d parameter tensors, got %d", p->n_params, num_params);
  int rc = ctrain_check(p, "srf_causal_backward");
  if (rc) return rc;
  for (int i = 0; i < num_params; ++i) SRF_CHECK_ARG(P[i] && G[i], "srf_causal_backward: parameter / gradient %d is null", i);
  const CTrainLayout t = ctrain_layout(p);
  const CScratchLayout s = cscratch_layout(p);
  SRF_CHECK_ARG(saved_bytes >= t.total && scratch_bytes >= s.total, "srf_causal_backward: saved / scratch buffer too small");
  SRF_CHECK_ARG(((((size_t)saved) | ((size_t)scratch)) & 255) == 0, "srf_causal_backward: buffers must be 256-byte aligned");
  const srf_config& c = p->cfg;
  const int D = c.upsampling_depth, U = c.num_blocks, N = c.enc_num_basis, K = c.enc_kernel_size, h = K / 2;
  const int Bt = p->Bt, L = p->L, B = p->nB, C = p->nC, SA = p->SA, SAN = p->SA * N;
  const char* sv = (const char*)saved;
  char* sc = (char*)scratch;
  hipStream_t st = (hipStream_t)stream;
  auto xbuf = [&](int i) { return (const float*)(sv + t.x0 + t.x_stride * i); };
  auto fp = [&](size_t o) { return (float*)(sc + o); };
  const float* enc = (const float*)(sv + t.enc);
  const float* m = (const float*)(sv + t.m);
  float* zeros = fp(s.zeros);
  float* wt = fp(s.wt);
  void* wg = sc + s.wg;
  const int pt = p->p_tail;
  if (srf_profiling()) srf_prof_mark("(gap)", st);
  SRF_CHECK_HIP(hipMemsetAsync(zeros, 0, sizeof(float) * s.zero_floats, st));
  // the weight-gradient GEMMs of this call fold their partial sums in a fixed order: two backwards of one step give equal bits
  struct Ordered {
    Ordered() { srf_pw_wgrad_ordered(true); }
    ~Ordered() { srf_pw_wgrad_ordered(false); }
  } ordered_for_this_call;
  std::vector<const float*> wproj, wres, bres;
  rc = ctrain_fold(p, P, s, sc, wproj, wres, bres, st);
  if (rc) return rc;
  // transposed weights of the data-gradient GEMMs, pre-split for the 256 x 128 kernel where it takes the shape
  std::vector<const float*> pk_w;
  std::vector<void*> pk_d;
  std::vector<int> pk_co, pk_ci;
  size_t pk_off = s.pkT;
  auto packT = [&](const float* w, int cout_d, int cin_d) -> const void* {   // w: forward weight [cin_d][cout_d]
    const size_t bytes = srf_packed_pw_weight_bytes(cout_d, cin_d);
    if (!bytes || srf_kernel_mode() != 0) return nullptr;
    void* d = sc + pk_off;
    pk_off += srf_align_up(bytes, 256);
    pk_w.push_back(w);
    pk_d.push_back(d);
    pk_co.push_back(cout_d);
    pk_ci.push_back(cin_d);
    return d;
  };
  const void* pkT_mask = packT(P[pt + 1], B, SAN);
  const void* pkT_bott = packT(P[1], N, B);
  std::vector<const void*> pkT_res(U, nullptr), pkT_proj(U, nullptr);
  for (int i = 0; i < U; ++i) {
    pkT_res[i] = packT(wres[i], C, B);
    pkT_proj[i] = packT(wproj[i], B, C);
  }
  if (!pk_w.empty()) {
    rc = srf_pack_pw_weights_transposed(pk_w.data(), pk_d.data(), pk_co.data(), pk_ci.data(), (int)pk_w.size(), st);
    if (rc) return rc;
  }
  // g_x = W^T g (+ residual): cin_d -> cout_d, w the forward weight [cin_d][cout_d]
  auto data_grad = [&](const float* g, const float* w, const void* pk, float* y, int cin_d, int cout_d, const float* residual) -> int {
    return srf_pw_data_grad(g, w, pk, wt, zeros, y, Bt, cin_d, cout_d, L, residual, st);
  };
  // ---- decoder: out = overlap_add(W_d^T PReLU_c(m))
  float* frames = fp(s.frames);
  float* gv = fp(s.gv);
  rc = srf_frames_gather(grad_out, frames, Bt, SA, p->T, K, h, h, L, s.dec_rows, stream);
  if (rc) return rc;
  rc = srf_prelu_apply(m, P[pt + 4], gv, (long)Bt * SAN * L, stream);     // v, re-computed
  if (rc) return rc;
  rc = srf_pw_wgrad_cols(gv, frames, nullptr, Bt, s.dec_rows, SAN, L, G[pt + 3], SA * K, nullptr, 0, wg, stream);
  if (rc) return rc;
  float* wdpad = fp(s.wdpad);
  SRF_CHECK_HIP(hipMemsetAsync(wdpad, 0, sizeof(float) * (size_t)SAN * s.dec_rows, st));
  SRF_CHECK_HIP(hipMemcpy2DAsync(wdpad, sizeof(float) * s.dec_rows, P[pt + 3], sizeof(float) * SA * K, sizeof(float) * SA * K, SAN,
                                 hipMemcpyDeviceToDevice, st));
  rc = srf_pw_conv(frames, wdpad, zeros, gv, Bt, s.dec_rows, SAN, L, nullptr, nullptr, nullptr, 0, nullptr, 0, stream);
  if (rc) return rc;
  // ---- mask_nl_class, mask_net
  rc = srf_causal_prelu_bwd(gv, m, P[pt + 4], gv, G[pt + 4], (long)Bt * SAN * L, fp(s.pyr), st);      // gv = g_m
  if (rc) return rc;
  float* gx = fp(s.gxa);
  float* gx_other = fp(s.gxb);
  {
    srf_norm pre{nullptr, nullptr, nullptr, P[pt]};
    rc = srf_pw_wgrad(gv, xbuf(U), &pre, Bt, B, SAN, L, G[pt + 1], G[pt + 2], 0, wg, stream);
    if (rc) return rc;
    rc = data_grad(gv, P[pt + 1], pkT_mask, gx, SAN, B, nullptr);
    if (rc) return rc;
    rc = srf_causal_prelu_bwd(gx, xbuf(U), P[pt], gx, G[pt], (long)Bt * B * L, fp(s.pyr), st);
    if (rc) return rc;
  }
  // ---- blocks in reverse
  const bool fused = srf_kernel_mode() != 1 && !srf_dbg(SRF_DBG_PYR_PER_LEVEL) && srf_causal_pyramid_bwd_supported(C, L, D);
  float* gm = fp(s.gm);
  float* gu = fp(s.gu);
  std::vector<float*> g_dw(U), g_db(U), g_gain(U);
  std::vector<const float*> p_w(U), p_b(U), p_gain(U);
  std::vector<const float*> bsrc, bscale;
  std::vector<float*> bdst;
  std::vector<long> bn;
  std::vector<float> bh;
  for (int i = U - 1; i >= 0; --i) {
    const int pb = p->p_block0 + i * p->p_block_stride;
    const float* const* Pb = P + pb;
    float* const* Gb = G + pb;
    const char* blk = sv + t.blk0 + t.blk_stride * i;
    const float* u = (const float*)(blk + t.u);
    const float* merged = (const float*)(blk + t.merged);
    // res_conv in its folded form: dW_f, db_f now (scaled to dW_r, db_r and reduced to d gain after the loop), g_M = W_f^T g_x'
    rc = srf_pw_wgrad(gx, merged, nullptr, Bt, C, B, L, Gb[4 + 3 * D], Gb[5 + 3 * D], 0, wg, stream);
    if (rc) return rc;
    g_dw[i] = Gb[4 + 3 * D]; g_db[i] = Gb[5 + 3 * D]; g_gain[i] = Gb[0];
    p_w[i] = Pb[4 + 3 * D]; p_b[i] = Pb[5 + 3 * D]; p_gain[i] = Pb[0];
    rc = data_grad(gx, wres[i], pkT_res[i], gm, B, C, nullptr);
    if (rc) return rc;
    const float *dv[SRF_MAX_DEPTH], *wv[SRF_MAX_DEPTH], *av[SRF_MAX_DEPTH];
    float *dwv[SRF_MAX_DEPTH], *dbv[SRF_MAX_DEPTH], *dsv[SRF_MAX_DEPTH];
    for (int k = 0; k < D; ++k) {
      dv[k] = (const float*)(blk + t.lv[k]);
      wv[k] = Pb[4 + 3 * k];
      av[k] = Pb[6 + 3 * k];
      dwv[k] = Gb[4 + 3 * k];
      dbv[k] = Gb[5 + 3 * k];
      dsv[k] = Gb[6 + 3 * k];
    }
    if (fused) {
      rc = srf_causal_pyramid_bwd(gm, u, dv, Pb[3], wv, av, gu, dwv, dbv, dsv, Gb[3], Bt, C, L, D, sc + s.pyr, stream);
      if (rc) return rc;
    } else {
      for (int k = D - 1; k >= 0; --k) {
        rc = srf_causal_dwconv_bwd(gm, k, k < D - 1 ? fp(s.gd[k + 1]) : nullptr, k < D - 1 ? wv[k + 1] : nullptr, 2, dv[k], av[k],
                                   k == 0 ? u : dv[k - 1], k == 0 ? Pb[3] : av[k - 1], k == 0 ? 1 : 2, fp(s.gd[k]), dwv[k], dbv[k],
                                   dsv[k], Bt, C, L >> k, sc + s.pyr, stream);
        if (rc) return rc;
      }
      rc = srf_causal_dwconv_bwd(nullptr, 0, fp(s.gd[0]), wv[0], 1, u, Pb[3], nullptr, nullptr, 1, gu, nullptr, nullptr, Gb[3], Bt,
                                 C, L, sc + s.pyr, stream);
      if (rc) return rc;
    }
    // proj_1x1 (its weight ran as W_p / beta): dW_p = gu x^T / beta, db_p, g_x = g_x' + W_p^T gu / beta
    rc = srf_pw_wgrad(gu, xbuf(i), nullptr, Bt, B, C, L, Gb[1], Gb[2], 0, wg, stream);
    if (rc) return rc;
    if (p->beta[i] != 1.f) {
      bsrc.push_back(Gb[1]); bdst.push_back(Gb[1]); bn.push_back((long)C * B); bscale.push_back(nullptr); bh.push_back(1.f / p->beta[i]);
    }
    rc = data_grad(gu, wproj[i], pkT_proj[i], gx_other, C, B, gx);
    if (rc) return rc;
    float* tmp = gx;
    gx = gx_other;
    gx_other = tmp;
  }
  // ---- bottleneck, encoder
  float* genc = fp(s.genc);
  rc = srf_pw_wgrad(gx, enc, nullptr, Bt, N, B, L, G[1], G[2], 0, wg, stream);
  if (rc) return rc;
  rc = data_grad(gx, P[1], pkT_bott, genc, B, N, nullptr);
  if (rc) return rc;
  rc = srf_frames_gather(wav, frames, Bt, p->A, p->T, K, h, 2 * h, L, p->A * K, stream);
  if (rc) return rc;
  rc = srf_pw_wgrad(genc, frames, nullptr, Bt, p->A * K, N, L, fp(s.encw), nullptr, 0, wg, stream);
  if (rc) return rc;
  rc = srf_causal_enc_scatter(fp(s.encw), G[0], N, p->A, K, st);
  if (rc) return rc;
  // ---- every block's skipinit_gain / res_conv gradients and the 1 / beta of the proj_1x1 weight gradients
  std::vector<float> alpha(p->alpha.begin(), p->alpha.end());
  rc = srf_causal_gain_fold(g_dw.data(), g_db.data(), p_w.data(), p_b.data(), p_gain.data(), g_gain.data(), alpha.data(), B * C, B, U, st);
  if (rc) return rc;
  if (!bsrc.empty()) rc = srf_causal_scale_many(bsrc.data(), bdst.data(), bn.data(), bscale.data(), bh.data(), (int)bsrc.size(), st);
  return rc;
}
