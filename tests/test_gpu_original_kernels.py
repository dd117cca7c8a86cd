"""The original SuDoRM-RF's own kernels (csrc/srf_original.hip) against fp64 on the host, at the smallest shapes at which they
can go wrong: odd sizes, more than one block, lengths that leave a scalar head and tail around the 16-byte body, bases 4 and 12
bytes off the 16-byte grid inside the guard-banded arena of tests/placement.py.

The bar of every float result is the rule of tests/test_gpu_attention.py: torch's own fp32 evaluation of the same formula on the
CPU deviates from the fp64 one by some max-abs amount; the kernel may deviate by 8 times that.  Copies (the Toeplitz mask weight,
the expanded decoder weight) are compared bit for bit.  Statistics: the kernels add fp32 values in fp64, so {sum, sumsq} of the
STORED output are reproduced to n * 2^-53 of sum |y| resp. sum y^2 -- the bar is 1e-9 of exactly those two scales.
Measured on an MI355X, worst over the cases (kernel error; as a multiple of torch's own fp32 deviation): srf_gln_apply_c 5.9e-7
(1.3 x), srf_encoder_bias_relu 6.0e-7 (1.4 x), srf_softmax_mask 1.7e-7 (1.2 x), srf_bias_rescale 7.4e-7 (1.0 x); statistics
<= 2.4e-16 relative; the fused pyramid without an input norm <= 1.6e-6 at max |ref| 12."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import original_fixtures as of
from tests import original_ref as orf
from tests import placement as pl

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    from sudo_rm_rf_amd import _lib, ops
    _lib.load()
    ops.set_kernel_mode(0)
    ops.set_debug_flags(0)
    yield
    ops.set_kernel_mode(0)


@functools.lru_cache(maxsize=None)
def arena():
    return pl.Arena(DEV, 8 << 20)


def bar_check(what, got, ref64, ref32):
    """got (device, fp32) against ref64; the bar: 8 x the deviation of torch's fp32 evaluation ref32 from ref64"""
    dev32 = (ref32.double() - ref64).abs().max().item()
    err = (got.double().cpu() - ref64).abs().max().item()
    print("%s: kernel err %.3e, torch fp32 dev %.3e, bar %.3e" % (what, err, dev32, 8 * dev32))
    assert got.shape == ref64.shape and torch.isfinite(got).all()
    assert err <= 8 * dev32
    return err


def bucket_sums(x64):
    """fp64 {sum, sumsq} per group of x [groups, C, L] in the library's bucket layout, spread over two buckets"""
    s = torch.zeros(x64.shape[0], 64, 2, dtype=torch.float64)
    half = x64.shape[2] // 2
    for bucket, part in ((5, x64[:, :, :half]), (63, x64[:, :, half:])):
        s[:, bucket, 0] = part.sum((1, 2))
        s[:, bucket, 1] = (part * part).sum((1, 2))
    return s


def stats_check(what, sums_dev, y_dev):
    y = y_dev.double().cpu()
    got = sums_dev.cpu().sum(1)
    want_s, want_q = y.sum((1, 2)), (y * y).sum((1, 2))
    rel_s = ((got[:, 0] - want_s).abs() / y.abs().sum((1, 2))).max().item()
    rel_q = ((got[:, 1] - want_q).abs() / want_q).max().item()
    print("%s: statistics rel err sum %.2e sumsq %.2e" % (what, rel_s, rel_q))
    assert rel_s <= 1e-9 and rel_q <= 1e-9


# ---- srf_gln_apply_c ----------------------------------------------------------------------------------------------------------------
GLN_SHAPES = [(3, 5, 7), (2, 64, 130), (1, 512, 201), (1, 3, 4500)]      # (the last: three chunks of one row, a body of 16-byte loads)
# the four sites of a block: (slopes, addend, statistics of the stored result)
GLN_USES = {"a": (True, False, False), "e": (True, False, False), "g_plus_x": (False, True, True), "block_out": (True, False, False)}


@functools.lru_cache(maxsize=None)
def gln_case(shape, use):
    groups, Cc, L = shape
    slopes, add, _ = GLN_USES[use]
    g = torch.Generator().manual_seed(1000 * Cc + L + 17 * sorted(GLN_USES).index(use))
    x = (torch.randn(shape, generator=g, dtype=torch.float64) * 1.7 + 0.4).float()
    gamma = (torch.rand(Cc, generator=g, dtype=torch.float64) + 0.5).float()
    beta = (torch.rand(Cc, generator=g, dtype=torch.float64) * 0.6 - 0.3).float()
    sl = (torch.rand(Cc, generator=g, dtype=torch.float64) * 0.4 + 0.05).float() if slopes else None
    ad = torch.randn(shape, generator=g, dtype=torch.float64).float() if add else None

    def run(dt):
        y = orf.gn(x.to(dt), gamma.to(dt), beta.to(dt))
        if sl is not None:
            y = orf.prelu_c(y, sl.to(dt))
        return y + ad.to(dt) if ad is not None else y
    return x, gamma, beta, sl, ad, bucket_sums(x.double()), run(torch.float64), run(torch.float32)


@pytest.mark.parametrize("shifts", [(1, 1, 1), (3, 3, 3), (0, 0, 0), (1, 3, 1)], ids=lambda s: "x%d_y%d_add%d" % s)
@pytest.mark.parametrize("use", sorted(GLN_USES))
@pytest.mark.parametrize("shape", GLN_SHAPES, ids=lambda s: "g%d_C%d_L%d" % s)
def test_gln_apply_c(shape, use, shifts):
    from sudo_rm_rf_amd import ops, original
    x, gamma, beta, sl, ad, sums, ref64, ref32 = gln_case(shape, use)
    a = arena()
    a.reset()
    xs, ys, adds = shifts
    xd = a.put(x, shift_floats=xs, name="x")
    gd, bd = a.put(gamma, shift_floats=1, name="gamma"), a.put(beta, shift_floats=3, name="beta")
    sd = a.put(sl, shift_floats=1, name="slopes") if sl is not None else None
    add_d = a.put(ad, shift_floats=adds, name="add") if ad is not None else None
    sums_d = a.put(sums, dtype=torch.float64, name="sums")
    out_sums = a.place((shape[0], 64, 2), torch.float64, name="out_sums", zero=True) if GLN_USES[use][2] else None
    yd = a.place(shape, shift_floats=ys, name="y")
    with ops.kernel_trace(DEV) as tr:
        original.gln_apply_c(xd, sums_d, gd, bd, slopes=sd, add=add_d, out_sums=out_sums, out=yd)
    torch.cuda.synchronize()
    same_phase = xs == ys and (ad is None or adds == xs)
    assert [n for n, _ in tr.launches] == ["gln_apply_c" if same_phase else "gln_apply_c_scalar"]
    a.check()
    a.assert_written(yd)
    a.assert_clean(yd)
    bar_check("gln_apply_c %s %s %s" % (shape, use, shifts), yd, ref64, ref32)
    if out_sums is not None:
        stats_check("gln_apply_c %s %s" % (shape, use), out_sums, yd)


def test_gln_apply_c_scalar_kernel_in_kernel_mode_1():
    from sudo_rm_rf_amd import ops, original
    x, gamma, beta, sl, ad, sums, ref64, ref32 = gln_case((2, 64, 130), "g_plus_x")
    ops.set_kernel_mode(1)
    try:
        s_out = ops.new_sums(2, DEV)
        with ops.kernel_trace(DEV) as tr:
            y = original.gln_apply_c(x.to(DEV), sums.to(DEV), gamma.to(DEV), beta.to(DEV), add=ad.to(DEV), out_sums=s_out)
        torch.cuda.synchronize()
    finally:
        ops.set_kernel_mode(0)
    assert tr.names == {"gln_apply_c_scalar"}
    bar_check("gln_apply_c scalar", y, ref64, ref32)
    stats_check("gln_apply_c scalar", s_out, y)


# ---- the fused pyramid on an input that has NO lazy norm (what the original model's walk hands it) --------------------------------
# (Bt, C, L, D, debug flags): the register-resident kernels | two LDS tiles per row | the block-per-row LDS kernels | depth 1
PYR_CASES = [(2, 6, 64, 3, 0), (1, 5, 1280, 3, 64), (2, 6, 64, 3, 64 | 32), (2, 3, 64, 1, 0), (1, 4, 3200, 5, 0)]


@pytest.mark.parametrize("case", PYR_CASES, ids=lambda c: "B%d_C%d_L%d_D%d_flags%d" % c)
def test_fused_pyramid_without_an_input_norm(case):
    """srf_pyramid with in_norm = NULL against the chain conv -> GlobLN per level + upsample-and-add in fp64.  An existing kernel
    on a path no other walk takes: the bar is that kernel's own (tests/test_gpu_ops.py test_fused_pyramid: 5e-5 max-abs, its
    statistics go through the linearity of conv o GlobLN), and the per-level kernels must agree with it."""
    from sudo_rm_rf_amd import _lib, ops
    Bt, Cc, L, D, flags = case
    g = torch.Generator().manual_seed(L + D)
    rnd = lambda *s, scale=1.0, shift=0.0: (torch.randn(*s, generator=g, dtype=torch.float64) * scale + shift).float()
    a = torch.where(rnd(Bt, Cc, L, scale=1.4, shift=0.2) >= 0, rnd(Bt, Cc, L), rnd(Bt, Cc, L) * 0.2)      # an activation's shape
    W, Bi = [rnd(Cc, 1, 5, scale=0.5) for _ in range(D)], [rnd(Cc, scale=0.2) for _ in range(D)]
    Ga, Be = [rnd(Cc, scale=0.3, shift=1.0) for _ in range(D)], [rnd(Cc, scale=0.3) for _ in range(D)]
    cur, outs = a.double(), []
    for k in range(D):
        cur = orf.gn(F.conv1d(cur, W[k].double(), Bi[k].double(), stride=1 if k == 0 else 2, padding=2, groups=Cc), Ga[k].double(),
                     Be[k].double())
        outs.append(cur)
    want = outs[-1]
    for k in range(D - 2, -1, -1):
        want = outs[k] + want.repeat_interleave(2, dim=-1)
    dev = lambda ts: [t.to(DEV) for t in ts]
    osums = ops.new_sums(Bt, DEV)
    with ops.debug_flags(flags):
        assert _lib.load().srf_pyramid_supported(Cc, L, D)
        with ops.kernel_trace(DEV) as tr:
            got = ops.pyramid(a.to(DEV), None, None, None, None, dev(W), dev(Bi), dev(Ga), dev(Be), out_sums=osums)
    torch.cuda.synchronize()
    assert [n for n, _ in tr.launches][-3:] == ["pyramid_moments", "pyramid_finalize", "pyramid_merge"]
    err = (got.double().cpu() - want).abs().max().item()
    # level by level: srf_dwconv5 with no norm on level 0, then srf_merge
    src, levels, sums, norm = a.to(DEV), [], [], {}
    for k in range(D):
        s_k = ops.new_sums(Bt, DEV)
        src = ops.dwconv5(src, W[k].to(DEV), Bi[k].to(DEV), 1 if k == 0 else 2, out_sums=s_k, **norm)
        levels.append(src)
        sums.append(s_k)
        norm = dict(in_sums=s_k, in_gamma=Ga[k].to(DEV), in_beta=Be[k].to(DEV))
    per_level = ops.merge(levels, sums, dev(Ga), dev(Be))
    err2 = (per_level.double().cpu() - want).abs().max().item()
    print("pyramid without input norm %s: fused err %.3e, per-level err %.3e (max|ref| %.2f)" % (case, err, err2, want.abs().max()))
    assert torch.isfinite(got).all() and err <= 5e-5 and err2 <= 5e-5
    y = want.reshape(Bt, -1)
    s = osums.cpu().sum(1)
    assert ((s[:, 0] - y.sum(1)).abs() <= 4e-6 * y.abs().sum(1) + 1e-9).all()
    assert ((s[:, 1] - (y * y).sum(1)).abs() <= 4e-6 * (y * y).sum(1) + 1e-9).all()


# ---- the encoder with bias and ReLU ---------------------------------------------------------------------------------------------------
# (Bt, T, N, K, L): K = 21 with a partial last block | K = 9, odd basis count | ONE frame | two time tiles
ENC_SHAPES = [(2, 1001, 6, 21, 104), (2, 100, 5, 9, 26), (1, 10, 4, 21, 1), (1, 1300, 20, 21, 130)]


@functools.lru_cache(maxsize=None)
def enc_case(shape, normalise):
    Bt, T, N, K, L = shape
    g = torch.Generator().manual_seed(31 * T + K)
    wav = (torch.randn(Bt, 1, T, generator=g, dtype=torch.float64) * (2.5 if normalise else 1.0) + (0.7 if normalise else 0.0)).float()
    w = (torch.randn(N, 1, K, generator=g, dtype=torch.float64) / K ** 0.5).float()
    b = (torch.rand(N, generator=g, dtype=torch.float64) * 0.2 - 0.1).float()
    stats = torch.stack([wav[:, 0].double().mean(-1), wav[:, 0].double().std(-1)], 1).float() if normalise else None

    def run(dt):
        x = wav.to(dt)
        if normalise:
            x = (x - stats[:, 0].to(dt)[:, None, None]) / (stats[:, 1].to(dt)[:, None, None] + 1e-9)
        h = K // 2
        x = F.pad(x, (0, max(0, h * L - T)))
        return torch.relu(F.conv1d(x, w.to(dt), b.to(dt), stride=h, padding=h))[..., :L]
    return wav, w, b, stats, run(torch.float64), run(torch.float32)


@pytest.mark.parametrize("normalise", [False, True], ids=["raw", "in_stats"])
@pytest.mark.parametrize("shape", ENC_SHAPES, ids=lambda s: "B%d_T%d_N%d_K%d_L%d" % s)
def test_encoder_bias_relu(shape, normalise):
    from sudo_rm_rf_amd import ops, original
    wav, w, b, stats, ref64, ref32 = enc_case(shape, normalise)
    assert ref64.shape[-1] == shape[4] and (ref64 == 0).any() and (ref64 > 0).any()       # the ReLU cuts some, not all
    a = arena()
    a.reset()
    wd, ww, bb = a.put(wav, shift_floats=1, name="wav"), a.put(w, shift_floats=3, name="w"), a.put(b, shift_floats=1, name="bias")
    st = a.put(stats, shift_floats=1, name="in_stats") if normalise else None
    sums = a.place((shape[0], 64, 2), torch.float64, name="sums", zero=True)
    with a.allocating(original, names=("out",), shifts={"out": 3}) as made:
        with ops.kernel_trace(DEV) as tr:
            out = original.encoder_bias_relu(wd, ww, bb, shape[4], sums=sums, in_stats=st)
    torch.cuda.synchronize()
    assert tr.names == {"encoder_bias_relu"} and a.owns(out) and made[0][0] == "out"
    a.check()
    a.assert_written(out)
    a.assert_clean(out)
    bar_check("encoder_bias_relu %s" % (shape,), out, ref64, ref32)
    stats_check("encoder_bias_relu %s" % (shape,), sums, out)


# ---- the mask layer as a GEMM weight: a copy, bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [4, 6, 64, 512])
@pytest.mark.parametrize("S", [1, 2, 3])
def test_mask_weight_fill_is_the_numpy_helper_bit_for_bit(N, S):
    from sudo_rm_rf_amd import original
    rng = np.random.default_rng(7 * N + S)
    w = rng.standard_normal((S, 1, N + 1, 1)).astype(np.float32)
    b = rng.standard_normal((S,)).astype(np.float32)
    want_tz, want_rows = of.toeplitz(w, b)
    a = arena()
    a.reset()
    wd, bd = a.put(torch.from_numpy(w), shift_floats=1, name="m.weight"), a.put(torch.from_numpy(b), shift_floats=3, name="m.bias")
    with a.allocating(original, names=("tz", "rows"), shifts={"tz": 1, "rows": 3}):
        tz, rows = original.mask_weight_fill(wd, bd)
    torch.cuda.synchronize()
    a.check()
    a.assert_written(rows)
    assert a.owns(tz) and not torch.isnan(tz).any()           # (zeros are written: nothing of the poison is left)
    assert np.array_equal(tz.cpu().numpy().view(np.int32), want_tz.view(np.int32))
    assert np.array_equal(rows.cpu().numpy().view(np.int32), want_rows.view(np.int32))


# ---- srf_softmax_mask ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def softmax_case(S, N, L, gain):
    g = torch.Generator().manual_seed(100 * S + N + L)
    z = (torch.randn(2, S, N, L, generator=g, dtype=torch.float64) * gain).float()
    if gain > 1:                                             # logits of exactly +-80 next to each other
        z[0, 0, 0, 0], z[1, S - 1, N - 1, L - 1] = 80.0, -80.0
        if S > 1:
            z[0, 1, 0, 0], z[1, 0, N - 1, L - 1] = -80.0, 80.0
    enc = torch.rand(2, N, L, generator=g, dtype=torch.float64).float()

    def run(dt):
        p = torch.sigmoid(z.to(dt)) if S == 1 else torch.softmax(z.to(dt), 1)
        return (p * enc.to(dt).unsqueeze(1)).reshape(2, S * N, L)
    return z.reshape(2, S * N, L).contiguous(), enc, run(torch.float64), run(torch.float32)


@pytest.mark.parametrize("NL", [(6, 5), (64, 130)], ids=lambda s: "N%d_L%d" % s)
@pytest.mark.parametrize("S", [1, 2, 3, 9])
def test_softmax_mask(S, NL):
    from sudo_rm_rf_amd import ops, original
    z, enc, ref64, ref32 = softmax_case(S, NL[0], NL[1], 1.0)
    a = arena()
    a.reset()
    zd, ed = a.put(z, shift_floats=1, name="z"), a.put(enc, shift_floats=3, name="enc")
    vd = a.place(z.shape, shift_floats=1, name="v")
    with ops.kernel_trace(DEV) as tr:
        original.softmax_mask(zd, ed, S, out=vd)
    torch.cuda.synchronize()
    assert tr.names == {"softmax_mask"}
    a.check()
    a.assert_written(vd)
    a.assert_clean(vd)
    bar_check("softmax_mask S %d %s" % (S, NL), vd, ref64, ref32)


@pytest.mark.parametrize("S", [1, 2, 3, 9])
def test_softmax_mask_large_logits_stay_finite_and_sum_to_one(S):
    from sudo_rm_rf_amd import original
    N, L = 64, 130
    z, enc, ref64, ref32 = softmax_case(S, N, L, 30.0)
    assert z.abs().max().item() >= 80.0
    v = original.softmax_mask(z.to(DEV), enc.to(DEV), S)
    bar_check("softmax_mask large logits S %d" % S, v, ref64, ref32)
    masks = original.softmax_mask(z.to(DEV), torch.ones_like(enc).to(DEV), S)
    torch.cuda.synchronize()
    assert torch.isfinite(masks).all() and (masks >= 0).all() and (masks <= 1).all()
    if S > 1:
        assert (masks.double().reshape(2, S, N, L).sum(1) - 1).abs().max().item() <= 1e-6
    # in place over z: a thread reads its S logits before it writes any
    zz = z.to(DEV).clone()
    assert torch.equal(original.softmax_mask(zz, enc.to(DEV), S, out=zz), v)


# ---- the grouped decoder's weight, expanded: exact ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("SNK", [(1, 4, 21), (2, 6, 9), (3, 64, 21), (2, 512, 21)], ids=lambda s: "S%d_N%d_K%d" % s)
def test_decoder_weight_expand_is_exact(SNK):
    from sudo_rm_rf_amd import original
    S, N, K = SNK
    w = np.random.default_rng(S + N).standard_normal((S * N, 1, K)).astype(np.float32)
    a = arena()
    a.reset()
    wd = a.put(torch.from_numpy(w), shift_floats=1, name="decoder.weight")
    with a.allocating(original, names=("wexp",), shifts={"wexp": 3}):
        got = original.decoder_weight_expand(wd, S)
    torch.cuda.synchronize()
    a.check()
    assert not torch.isnan(got).any()
    assert np.array_equal(got.cpu().numpy().view(np.int32), of.expand_decoder(w, S).view(np.int32))


# ---- decoder.bias before the rescale (and mixture consistency) -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bias_only", "rescale", "rescale_mc"])
@pytest.mark.parametrize("shape", [(2, 3, 7), (2, 2, 1001), (3, 1, 300)], ids=lambda s: "B%d_S%d_T%d" % s)
def test_bias_goes_in_before_the_rescale(shape, mode):
    from sudo_rm_rf_amd import original
    Bt, S, T = shape
    g = torch.Generator().manual_seed(T + S)
    est = torch.randn(shape, generator=g, dtype=torch.float64).float()
    bias = (torch.rand(S, generator=g, dtype=torch.float64) - 0.5).float()
    wav = (torch.randn(Bt, 1, T, generator=g, dtype=torch.float64) * 3.0 + 0.8).float()
    stats = torch.stack([wav[:, 0].double().mean(-1), wav[:, 0].double().std(-1)], 1).float()

    def run(dt):
        y = est.to(dt) + bias.to(dt)[None, :, None]
        if mode == "bias_only":
            return y
        m, sd = stats[:, 0].to(dt)[:, None, None], stats[:, 1].to(dt)[:, None, None]
        y = y * sd + m
        if mode == "rescale_mc":
            y = y + ((wav.to(dt) - m) / (sd + 1e-9) - y.sum(1, keepdim=True)) / S
        return y
    a = arena()
    a.reset()
    ed, bd = a.put(est, shift_floats=1, name="est"), a.put(bias, shift_floats=3, name="bias")
    wd, sd_ = a.put(wav, shift_floats=3, name="wav"), a.put(stats, shift_floats=1, name="stats")
    if mode == "bias_only":
        original.bias_rescale(ed, bd)
    else:
        original.bias_rescale(ed, bd, stats=sd_, wav=wd, mixture_consistency=mode == "rescale_mc")
    torch.cuda.synchronize()
    a.check()
    a.assert_clean(ed)
    bar_check("bias_rescale %s %s" % (shape, mode), ed, run(torch.float64), run(torch.float32))


def test_refusals_leave_the_output_untouched():
    from sudo_rm_rf_amd import _lib, original
    a = arena()
    a.reset()
    z = a.place((1, 17 * 4, 3), name="z", zero=True)
    enc = a.place((1, 4, 3), name="enc", zero=True)
    v = a.place((1, 17 * 4, 3), name="v")
    with pytest.raises(_lib.SrfError, match="num_sources = 17"):
        original.softmax_mask(z, enc, 17, out=v)
    w = a.place((2, 1, 6, 1), name="m.weight", zero=True)          # N = 5: odd
    with a.allocating(original, names=("tz", "rows")) as made:
        with pytest.raises(_lib.SrfError, match="even"):
            original.mask_weight_fill(w, a.place((2,), name="m.bias", zero=True))
    torch.cuda.synchronize()
    a.check()
    a.assert_untouched(v)
    for _, t in made:
        a.assert_untouched(t)
