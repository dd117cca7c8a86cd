"""The ragged forms of the original SuDoRM-RF's own kernels (csrc/srf_original.hip) and the fused ragged pyramid without an input
norm, each example against fp64 on the host over ITS OWN columns.

The bar is the rule of tests/test_gpu_original_kernels.py: 8 x the deviation of torch's fp32 CPU evaluation from fp64 on the same
inputs.  Bases sit 0, 4 and 12 bytes off the 16-byte grid inside the guard-banded arena of tests/placement.py, whose payloads
start out as 0xFF bytes (NaN as floats): every output must be written everywhere, exact zeros past every example's end.  The
inputs hold NaN at and past every end: a read there would surface as a NaN in the result or in the statistics (a read-mask check;
nothing is provoked -- NaN is data).  Statistics: within 1e-9 relative of fp64 over the example's own columns.
Measured on an MI355X, worst over the cases (kernel error; as a multiple of torch's own fp32 deviation): srf_gln_apply_c_ragged
5.5e-7 (1.1 x), srf_encoder_bias_relu_ragged 7.6e-7 (1.0 x), srf_softmax_mask_ragged 4.1e-7 (1.0 x), srf_bias_rescale_ragged 7.5e-7
(1.0 x); statistics <= 1.6e-16 relative; the fused ragged pyramid without an input norm 2.8e-6 (D = 3) / 3.6e-6 (D = 5) at max
|ref| 21."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import original_ref as orf
from tests.test_gpu_original_kernels import arena, bar_check, stats_check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
SHIFTS = [0, 1, 3]          # floats off the 16-byte grid: bases 0, 4 and 12 bytes off


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


def poison_past(x, ends):
    """x [groups, ., n] with NaN at and past ends[g] of every group"""
    x = x.clone()
    for g, e in enumerate(ends):
        x[g, ..., e:] = NAN
    return x


def zeros_past(what, got, ends):
    for g, e in enumerate(ends):
        tail = got[g, ..., e:]
        assert tail.numel() == 0 or bool((tail == 0).all()), "%s: example %d is not exact zero from %d on" % (what, g, e)


def own_sums(x64, ends):
    """fp64 {sum, sumsq} per group over its own columns, in the library's bucket layout (two buckets)"""
    s = torch.zeros(x64.shape[0], 64, 2, dtype=torch.float64)
    for g, e in enumerate(ends):
        half = e // 2
        for bucket, part in ((5, x64[g, :, :half]), (63, x64[g, :, half:e])):
            s[g, bucket, 0] = part.sum()
            s[g, bucket, 1] = (part * part).sum()
    return s


# ---- srf_gln_apply_c_ragged ---------------------------------------------------------------------------------------------------------
# (3, 5, 4500) with frames [4500, 2048, 100]: rows of three 2048-chunks -- group 1 ends exactly on a chunk boundary (its chunks 1
# and 2 lie wholly past the end), group 2 ends inside chunk 0.  (2, 64, 132) with frames [132, 4]: one chunk, the shortest length.
GLN_CASES = [((3, 5, 4500), (4500, 2048, 100)), ((2, 64, 132), (132, 4))]
# the four sites of a block: (slopes, addend, statistics of the stored result)
GLN_USES = {"a": (True, False, False), "e": (True, False, False), "g_plus_x": (False, True, True), "block_out": (True, False, False)}


@functools.lru_cache(maxsize=None)
def gln_case(shape, frames, use):
    groups, Cc, L = shape
    slopes, add, _ = GLN_USES[use]
    g = torch.Generator().manual_seed(1000 * Cc + L + 17 * sorted(GLN_USES).index(use) + 5)
    x = (torch.randn(shape, generator=g, dtype=torch.float64) * 1.7 + 0.4).float()
    gamma = (torch.rand(Cc, generator=g, dtype=torch.float64) + 0.5).float()
    beta = (torch.rand(Cc, generator=g, dtype=torch.float64) * 0.6 - 0.3).float()
    sl = (torch.rand(Cc, generator=g, dtype=torch.float64) * 0.4 + 0.05).float() if slopes else None
    ad = torch.randn(shape, generator=g, dtype=torch.float64).float() if add else None

    def run(dt):
        out = torch.zeros(shape, dtype=dt)
        for b, n in enumerate(frames):          # every group alone, over its own columns
            y = orf.gn(x[b:b + 1, :, :n].to(dt), gamma.to(dt), beta.to(dt))
            if sl is not None:
                y = orf.prelu_c(y, sl.to(dt))
            out[b, :, :n] = (y + ad[b:b + 1, :, :n].to(dt) if ad is not None else y)[0]
        return out
    return x, gamma, beta, sl, ad, own_sums(x.double(), frames), run(torch.float64), run(torch.float32)


@pytest.mark.parametrize("shifts", [(0, 0, 0), (1, 1, 1), (3, 3, 3), (1, 3, 1)], ids=lambda s: "x%d_y%d_add%d" % s)
@pytest.mark.parametrize("use", sorted(GLN_USES))
@pytest.mark.parametrize("case", GLN_CASES, ids=lambda c: "g%d_C%d_L%d" % c[0])
def test_gln_apply_c_ragged(case, use, shifts):
    from sudo_rm_rf_amd import ops, original
    shape, frames = case
    x, gamma, beta, sl, ad, sums, ref64, ref32 = gln_case(shape, frames, use)
    a = arena()
    a.reset()
    xs, ys, adds = shifts
    xd = a.put(poison_past(x, frames), shift_floats=xs, name="x")
    gd, bd = a.put(gamma, shift_floats=1, name="gamma"), a.put(beta, shift_floats=3, name="beta")
    sd = a.put(sl, shift_floats=1, name="slopes") if sl is not None else None
    add_d = a.put(poison_past(ad, frames), shift_floats=adds, name="add") if ad is not None else None
    sums_d = a.put(sums, dtype=torch.float64, name="sums")
    out_sums = a.place((shape[0], 64, 2), torch.float64, name="out_sums", zero=True) if GLN_USES[use][2] else None
    yd = a.place(shape, shift_floats=ys, name="y")
    with ops.kernel_trace(DEV) as tr:
        original.gln_apply_c_ragged(xd, sums_d, gd, bd, list(frames), slopes=sd, add=add_d, out_sums=out_sums, out=yd)
    torch.cuda.synchronize()
    same_phase = xs == ys and (ad is None or adds == xs)
    assert [n for n, _ in tr.launches] == ["gln_apply_c_ragged" if same_phase else "gln_apply_c_scalar_ragged"]
    a.check()
    a.assert_written(yd)
    a.assert_clean(yd)
    zeros_past("gln_apply_c_ragged", yd, frames)
    bar_check("gln_apply_c_ragged %s %s %s" % (shape, use, shifts), yd, ref64, ref32)
    if out_sums is not None:
        assert torch.isfinite(out_sums).all()
        stats_check("gln_apply_c_ragged %s %s" % (shape, use), out_sums, yd)


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("use", ["a", "g_plus_x"])
@pytest.mark.parametrize("shape", [(3, 5, 4500), (2, 64, 132)], ids=lambda s: "g%d_C%d_L%d" % s)
def test_gln_apply_c_ragged_at_full_length_is_the_uniform_kernel_bit_for_bit(shape, use, shift):
    from sudo_rm_rf_amd import original
    full = (shape[2],) * shape[0]
    x, gamma, beta, sl, ad, sums, _, _ = gln_case(shape, full, use)
    a = arena()
    a.reset()
    xd = a.put(x, shift_floats=shift, name="x")
    add_d = a.put(ad, shift_floats=shift, name="add") if ad is not None else None
    sums_d = a.put(sums, dtype=torch.float64, name="sums")
    dev = lambda t: None if t is None else t.to(DEV)
    y_u, y_r = a.place(shape, shift_floats=shift, name="y_uniform"), a.place(shape, shift_floats=shift, name="y_ragged")
    s_u, s_r = (a.place((shape[0], 64, 2), torch.float64, name=n, zero=True) for n in ("sums_u", "sums_r"))
    original.gln_apply_c(xd, sums_d, dev(gamma), dev(beta), slopes=dev(sl), add=add_d, out_sums=s_u, out=y_u)
    original.gln_apply_c_ragged(xd, sums_d, dev(gamma), dev(beta), list(full), slopes=dev(sl), add=add_d, out_sums=s_r, out=y_r)
    torch.cuda.synchronize()
    a.check()
    assert torch.equal(y_u, y_r) and torch.isfinite(y_r).all()
    assert torch.allclose(s_u.sum(1), s_r.sum(1), rtol=1e-12, atol=0)


# ---- srf_encoder_bias_relu_ragged -----------------------------------------------------------------------------------------------------
ENC_N, ENC_L, ENC_T, ENC_K = 64, 200, 2000, 21
ENC_LENGTHS = (2000, 1991, 650, 10)          # 200 frames twice (one row 9 samples short of them), 65 frames, ONE frame
ENC_FRAMES = (200, 200, 65, 1)


@functools.lru_cache(maxsize=None)
def enc_case(normalise):
    g = torch.Generator().manual_seed(4242)
    Bt, h = len(ENC_LENGTHS), ENC_K // 2
    wav = (torch.randn(Bt, 1, ENC_T, generator=g, dtype=torch.float64) * (2.5 if normalise else 1.0) + (0.7 if normalise else 0.0)).float()
    w = (torch.randn(ENC_N, 1, ENC_K, generator=g, dtype=torch.float64) / ENC_K ** 0.5).float()
    b = (torch.rand(ENC_N, generator=g, dtype=torch.float64) * 0.2 - 0.1).float()
    stats = None
    if normalise:          # every row's own samples
        stats = torch.stack([torch.stack([wav[r, 0, :n].double().mean(), wav[r, 0, :n].double().std() if n > 1 else torch.tensor(1.0, dtype=torch.float64)])
                             for r, n in enumerate(ENC_LENGTHS)]).float()

    def run(dt):
        out = torch.zeros(Bt, ENC_N, ENC_L, dtype=dt)
        for r, (n, fr) in enumerate(zip(ENC_LENGTHS, ENC_FRAMES)):          # the row alone, zero-padded to its own frames
            x = wav[r:r + 1, :, :n].to(dt)
            if normalise:
                x = (x - stats[r, 0].to(dt)) / (stats[r, 1].to(dt) + 1e-9)
            x = F.pad(x, (0, h * fr - n))
            out[r, :, :fr] = torch.relu(F.conv1d(x, w.to(dt), b.to(dt), stride=h, padding=h))[0, :, :fr]
        return out
    return wav, w, b, stats, run(torch.float64), run(torch.float32)


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("normalise", [False, True], ids=["raw", "in_stats"])
def test_encoder_bias_relu_ragged(normalise, shift):
    from sudo_rm_rf_amd import ops, original
    wav, w, b, stats, ref64, ref32 = enc_case(normalise)
    assert (b > 0).any()          # relu(bias) is not zero: a frame past the end that merely saw zero samples would show
    a = arena()
    a.reset()
    wd = a.put(poison_past(wav, ENC_LENGTHS), shift_floats=shift, name="wav")
    ww, bb = a.put(w, shift_floats=3, name="w"), a.put(b, shift_floats=1, name="bias")
    st = a.put(stats, shift_floats=1, name="in_stats") if normalise else None
    sums = a.place((len(ENC_LENGTHS), 64, 2), torch.float64, name="sums", zero=True)
    with a.allocating(original, names=("out",), shifts={"out": shift}) as made:
        with ops.kernel_trace(DEV) as tr:
            out = original.encoder_bias_relu_ragged(wd, ww, bb, ENC_L, list(ENC_LENGTHS), list(ENC_FRAMES), sums=sums, in_stats=st)
    torch.cuda.synchronize()
    assert [n for n, _ in tr.launches] == ["encoder_bias_relu_ragged"] and [n for n, _ in made] == ["out"]
    a.check()
    a.assert_written(out)
    a.assert_clean(out)
    # zeros from L_b on -- frame L_b included, which would otherwise see the row's last h samples
    zeros_past("encoder_bias_relu_ragged", out, ENC_FRAMES)
    assert bool((ref64[2, :, 64] > 0).any()) and bool((out[2, :, 65] == 0).all())
    bar_check("encoder_bias_relu_ragged normalise=%s shift=%d" % (normalise, shift), out, ref64, ref32)
    assert torch.isfinite(sums).all()
    stats_check("encoder_bias_relu_ragged", sums, out)


# ---- srf_softmax_mask_ragged ----------------------------------------------------------------------------------------------------------
SM_N, SM_L, SM_FRAMES = 8, 200, (200, 64, 4)


@functools.lru_cache(maxsize=None)
def softmax_case(S):
    g = torch.Generator().manual_seed(77 + S)
    Bt = len(SM_FRAMES)
    z = (torch.randn(Bt, S * SM_N, SM_L, generator=g, dtype=torch.float64) * 3.0).float()
    enc = torch.relu(torch.randn(Bt, SM_N, SM_L, generator=g, dtype=torch.float64)).float()

    def run(dt):
        zz = z.to(dt).view(Bt, S, SM_N, SM_L)
        p = torch.sigmoid(zz) if S == 1 else torch.softmax(zz, dim=1)
        out = (p * enc.to(dt).unsqueeze(1)).reshape(Bt, S * SM_N, SM_L)
        for b, n in enumerate(SM_FRAMES):
            out[b, :, n:] = 0
        return out
    return z, enc, run(torch.float64), run(torch.float32)


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("S", [1, 2, 3, 9])
def test_softmax_mask_ragged(S, shift):
    from sudo_rm_rf_amd import ops, original
    z, enc, ref64, ref32 = softmax_case(S)
    a = arena()
    a.reset()
    zd = a.put(poison_past(z, SM_FRAMES), shift_floats=shift, name="z")
    ed = a.put(poison_past(enc, SM_FRAMES), shift_floats=(shift + 1) % 4 if shift else 0, name="enc")
    vd = a.place(tuple(z.shape), shift_floats=shift, name="v")
    with ops.kernel_trace(DEV) as tr:
        original.softmax_mask_ragged(zd, ed, S, list(SM_FRAMES), out=vd)
    torch.cuda.synchronize()
    assert [n for n, _ in tr.launches] == ["softmax_mask_ragged"]
    a.check()
    a.assert_written(vd)
    a.assert_clean(vd)
    zeros_past("softmax_mask_ragged", vd, SM_FRAMES)
    bar_check("softmax_mask_ragged S=%d shift=%d" % (S, shift), vd, ref64, ref32)
    # in place (v = z): the same bits as out of place
    original.softmax_mask_ragged(zd, ed, S, list(SM_FRAMES), out=zd)
    torch.cuda.synchronize()
    a.check()
    assert torch.equal(zd, vd)


# ---- srf_bias_rescale_ragged ----------------------------------------------------------------------------------------------------------
BR_T, BR_S, BR_LENGTHS = 1000, 3, (1000, 999, 1)


@functools.lru_cache(maxsize=None)
def bias_case(form):
    g = torch.Generator().manual_seed(991)
    Bt = len(BR_LENGTHS)
    est = torch.randn(Bt, BR_S, BR_T, generator=g, dtype=torch.float64).float()
    bias = (torch.randn(BR_S, generator=g, dtype=torch.float64) * 0.3).float()
    wav = (torch.randn(Bt, 1, BR_T, generator=g, dtype=torch.float64) * 2.0 + 0.5).float()
    stats = torch.tensor([[0.5, 2.0], [-0.25, 0.6], [0.125, 1.5]], dtype=torch.float32) if form != "plain" else None

    def run(dt):
        out = est.to(dt) + bias.to(dt)[None, :, None]
        if stats is not None:
            mean, sd = stats[:, 0].to(dt)[:, None, None], stats[:, 1].to(dt)[:, None, None]
            out = out * sd + mean
            if form == "stats_mc":
                out = out + ((wav.to(dt) - mean) / (sd + 1e-9) - out.sum(1, keepdim=True)) / BR_S
        for b, n in enumerate(BR_LENGTHS):
            out[b, :, n:] = 0
        return out
    return est, bias, wav, stats, run(torch.float64), run(torch.float32)


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("form", ["plain", "stats", "stats_mc"])
def test_bias_rescale_ragged(form, shift):
    from sudo_rm_rf_amd import ops, original
    est, bias, wav, stats, ref64, ref32 = bias_case(form)
    a = arena()
    a.reset()
    od = a.put(poison_past(est, BR_LENGTHS), shift_floats=shift, name="out")          # (in place: past the end it is only written)
    bd = a.put(bias, shift_floats=1, name="bias")
    wd = a.put(poison_past(wav, BR_LENGTHS), shift_floats=3 - shift, name="wav") if stats is not None else None
    sd = a.put(stats, shift_floats=1, name="stats") if stats is not None else None
    with ops.kernel_trace(DEV) as tr:
        original.bias_rescale_ragged(od, bd, list(BR_LENGTHS), stats=sd, wav=wd, mixture_consistency=form == "stats_mc")
    torch.cuda.synchronize()
    assert [n for n, _ in tr.launches] == ["bias_rescale_ragged"]
    a.check()
    a.assert_clean(od)
    zeros_past("bias_rescale_ragged", od, BR_LENGTHS)
    bar_check("bias_rescale_ragged %s shift=%d" % (form, shift), od, ref64, ref32)


# ---- the fused ragged pyramid on an input that has NO lazy norm (what the original model's ragged walk hands it) -------------------
@pytest.mark.parametrize("D", [3, 5])
def test_fused_ragged_pyramid_without_an_input_norm(D):
    """srf_pyramid_ragged with in_norm = NULL, every example against the chain conv -> GlobLN per level + upsample-and-add in fp64
    over its own columns.  An existing kernel on a path no other walk takes: the bar is that kernel's own 5e-5 max-abs."""
    from sudo_rm_rf_amd import ops, ragged
    Bt, Cc, L, frames = 2, 64, 256, (256, 128)
    g = torch.Generator().manual_seed(L + D + 3)
    rnd = lambda *s, scale=1.0, shift=0.0: (torch.randn(*s, generator=g, dtype=torch.float64) * scale + shift).float()
    act = torch.where(rnd(Bt, Cc, L, scale=1.4, shift=0.2) >= 0, rnd(Bt, Cc, L), rnd(Bt, Cc, L) * 0.2)      # an activation's shape
    W, Bi = [rnd(Cc, 1, 5, scale=0.5) for _ in range(D)], [rnd(Cc, scale=0.2) for _ in range(D)]
    Ga, Be = [rnd(Cc, scale=0.3, shift=1.0) for _ in range(D)], [rnd(Cc, scale=0.3) for _ in range(D)]
    want = torch.zeros(Bt, Cc, L, dtype=torch.float64)
    for b, n in enumerate(frames):
        cur, outs = act[b:b + 1, :, :n].double(), []
        for k in range(D):
            cur = orf.gn(F.conv1d(cur, W[k].double(), Bi[k].double(), stride=1 if k == 0 else 2, padding=2, groups=Cc), Ga[k].double(),
                         Be[k].double())
            outs.append(cur)
        m = outs[-1]
        for k in range(D - 2, -1, -1):
            m = outs[k] + m.repeat_interleave(2, dim=-1)
        want[b, :, :n] = m[0]
    dev = lambda ts: [t.to(DEV) for t in ts]
    osums = ops.new_sums(Bt, DEV)
    with ops.kernel_trace(DEV) as tr:
        got = ragged.pyramid(poison_past(act, frames).to(DEV), None, None, None, None, dev(W), dev(Bi), dev(Ga), dev(Be), list(frames),
                             out_sums=osums)
    torch.cuda.synchronize()
    assert all(n.endswith("_ragged") for n, _ in tr.launches if n.startswith("pyramid")), tr.launches
    err = (got.double().cpu() - want).abs().max().item()
    print("ragged pyramid without input norm D=%d: err %.3e (max|ref| %.2f)" % (D, err, want.abs().max()))
    assert torch.isfinite(got).all() and err <= 5e-5
    zeros_past("pyramid_ragged", got, frames)
    y = want.reshape(Bt, -1)
    s = osums.cpu().sum(1)
    assert ((s[:, 0] - y.sum(1)).abs() <= 4e-6 * y.abs().sum(1) + 1e-9).all()
    assert ((s[:, 1] - (y * y).sum(1)).abs() <= 4e-6 * (y * y).sum(1) + 1e-9).all()
