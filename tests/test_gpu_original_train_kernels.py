"""The kernels the original SuDoRM-RF's training step has that no other model has (csrc/srf_original_train.hip) against fp64
autograd on the host, at the smallest shapes at which they can go wrong: odd sizes, more than one block, a row longer than one
2048-position chunk, lengths that leave a scalar head and tail around the 16-byte body, bases 4 and 12 bytes off the 16-byte grid
inside the guard-banded arena of tests/placement.py.

The bar of every float result is the rule of tests/test_gpu_original_kernels.py: torch's own fp32 CPU autograd on the same inputs
deviates from the fp64 one by some max-abs amount; the kernel may deviate by 8 times that.  Copies and gates (srf_relu_gate, the
contract) are compared bit for bit.  Every reduction of these kernels has a fixed order: a second call gives the same bits.
PReLU inputs come from fixed seeds for which NO pre-activation lies within 1e-5 of the kink in fp64 (asserted, nothing masked);
test_gln_c_bwd_zero_channels_take_the_slope alone puts whole channels exactly ON it, to pin torch's convention there."""
import functools

import numpy as np
import pytest
import torch

from tests import original_fixtures as of
from tests import original_ref as orf
from tests import original_train_ref as otr
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
    return pl.Arena(DEV, 16 << 20)


def bar_check(what, got, ref64, ref32):
    """got (device, fp32) against ref64; the bar: 8 x the deviation of torch's fp32 evaluation ref32 from ref64"""
    dev32 = (ref32.double() - ref64).abs().max().item()
    err = (got.double().cpu() - ref64).abs().max().item()
    print("%s: kernel err %.3e, torch fp32 dev %.3e, bar %.3e (max|ref| %.3g)" % (what, err, dev32, 8 * dev32, ref64.abs().max()))
    assert got.shape == ref64.shape and torch.isfinite(got).all()
    assert err <= 8 * dev32, (what, err, 8 * dev32)
    return err


def bucket_sums(x64):
    """fp64 {sum, sumsq} per group of x [groups, C, L] in the library's bucket layout, spread over two buckets"""
    s = torch.zeros(x64.shape[0], 64, 2, dtype=torch.float64)
    half = x64.shape[2] // 2
    for bucket, part in ((5, x64[:, :, :half]), (63, x64[:, :, half:])):
        s[:, bucket, 0] = part.sum((1, 2))
        s[:, bucket, 1] = (part * part).sum((1, 2))
    return s


# ---- srf_gln_c_bwd ---------------------------------------------------------------------------------------------------------------------
GLN_SHAPES = [(3, 5, 7), (2, 64, 130), (1, 512, 201), (1, 3, 4500)]      # (the last: three chunks per row)
KINK = 1e-5


@functools.lru_cache(maxsize=None)
def gln_case(shape):
    """Inputs of one shape, from the first seed of a fixed sequence at which no pre-activation is within KINK of 0 in fp64 (the
    choice looks at the inputs alone), and the fp64 / fp32 autograd of sum(y * (gout + gout2)) with and without slopes / gout2."""
    groups, Cc, L = shape
    for seed in range(7000 + Cc + L, 7000 + Cc + L + 64):
        g = torch.Generator().manual_seed(seed)
        x = (torch.randn(shape, generator=g, dtype=torch.float64) * 1.7 + 0.4).float()
        gamma = (torch.rand(Cc, generator=g, dtype=torch.float64) + 0.5).float()
        beta = (torch.rand(Cc, generator=g, dtype=torch.float64) * 0.6 - 0.3).float()
        v = orf.gn(x.double(), gamma.double(), beta.double())
        if float(v.abs().min()) > KINK:
            break
    else:
        raise AssertionError("no seed keeps every pre-activation %g away from the kink" % KINK)
    assert float(v.abs().min()) > KINK          # in fp64, on exactly the inputs the kernel gets; nothing is masked out
    sl = (torch.rand(Cc, generator=g, dtype=torch.float64) * 0.4 + 0.05).float()
    gout = torch.randn(shape, generator=g, dtype=torch.float64).float()
    gout2 = torch.randn(shape, generator=g, dtype=torch.float64).float()
    gx0 = torch.randn(shape, generator=g, dtype=torch.float64).float()          # what an accumulating call adds to
    p0 = [torch.randn(Cc, generator=g, dtype=torch.float64).float() for _ in range(3)]

    def run(dt, slopes, two):
        xs, ga, be, s_ = (t.to(dt).clone().requires_grad_() for t in (x, gamma, beta, sl))
        y = orf.gn(xs, ga, be)
        if slopes:
            y = orf.prelu_c(y, s_)
        go = gout.to(dt) + gout2.to(dt) if two else gout.to(dt)
        (y * go).sum().backward()
        return xs.grad, ga.grad, be.grad, (s_.grad if slopes else None)
    refs = {(slopes, two): (run(torch.float64, slopes, two), run(torch.float32, slopes, two))
            for slopes in (False, True) for two in (False, True)}
    return x, gamma, beta, sl, gout, gout2, gx0, p0, bucket_sums(x.double()), refs


@pytest.mark.parametrize("shifts", [(1, 1, 1, 1), (3, 3, 3, 3), (1, 3, 1, 1), (1, 1, 1, 3)], ids=lambda s: "x%d_gout%d_gout2_%d_gx%d" % s)
@pytest.mark.parametrize("slopes", [False, True], ids=["no_slopes", "slopes"])
@pytest.mark.parametrize("shape", GLN_SHAPES, ids=lambda s: "g%d_C%d_L%d" % s)
def test_gln_c_bwd(shape, slopes, shifts):
    """With and without gout2, overwriting and accumulating gx, on equal phases (16-byte kernels) and different ones (dword
    kernels); the parameter gradients are added to what their buffers hold; a second call gives the same bits."""
    from sudo_rm_rf_amd import ops, original
    x, gamma, beta, sl, gout, gout2, gx0, p0, sums, refs = gln_case(shape)
    xs, gs, g2s, gxs = shifts
    for two in (False, True):
        for acc in (False, True):
            (r64, r32) = refs[(slopes, two)]
            a = arena()
            a.reset()
            xd = a.put(x, shift_floats=xs, name="x")
            god = a.put(gout, shift_floats=gs, name="gout")
            go2d = a.put(gout2, shift_floats=g2s, name="gout2") if two else None
            gd, bd = a.put(gamma, shift_floats=1, name="gamma"), a.put(beta, shift_floats=3, name="beta")
            sld = a.put(sl, shift_floats=1, name="slopes") if slopes else None
            sums_d = a.put(sums, dtype=torch.float64, name="sums")
            runs = []
            for rep in range(2):
                gxd = a.put(gx0, shift_floats=gxs, name="gx%d" % rep) if acc else a.place(shape, shift_floats=gxs, name="gx%d" % rep)
                dg, db = a.put(p0[0], shift_floats=3, name="dgamma%d" % rep), a.put(p0[1], shift_floats=1, name="dbeta%d" % rep)
                ds = a.put(p0[2], shift_floats=3, name="dslope%d" % rep) if slopes else None
                with ops.kernel_trace(DEV) as tr:
                    original.gln_c_bwd(god, xd, sums_d, gd, bd, slopes=sld, gout2=go2d, gx=gxd, accumulate=acc, dgamma=dg, dbeta=db,
                                       dslope=ds)
                torch.cuda.synchronize()
                same = xs == gs == gxs and (not two or g2s == xs)
                suffix = "" if same else "_scalar"
                assert [n for n, _ in tr.launches] == ["gln_c_bwd_reduce" + suffix, "gln_c_bwd_apply" + suffix]
                runs.append((gxd, dg, db, ds))
            a.check()
            for t in runs[0][:3]:
                a.assert_written(t)
                a.assert_clean(t)
            assert all(torch.equal(p, q) for p, q in zip(runs[0], runs[1]) if p is not None), "second call differs"
            gxd, dg, db, ds = runs[0]
            tag = "gln_c_bwd %s slopes=%s gout2=%s acc=%s %s" % (shape, slopes, two, acc, shifts)
            add = (lambda t, dt: t.to(dt)) if acc else (lambda t, dt: 0)
            bar_check(tag + " gx", gxd, r64[0] + add(gx0, torch.float64), r32[0] + add(gx0, torch.float32))
            bar_check(tag + " dgamma", dg, r64[1] + p0[0].double(), r32[1] + p0[0])
            bar_check(tag + " dbeta", db, r64[2] + p0[1].double(), r32[2] + p0[1])
            if slopes:
                bar_check(tag + " dslope", ds, r64[3] + p0[2].double(), r32[3] + p0[2])


@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 64, 130)], ids=lambda s: "g%d_C%d_L%d" % s)
def test_gln_c_bwd_every_nullable_output_null(shape):
    """dgamma, dbeta, dslope and gout2 each left out: what remains has the bits of the full call; dslope without slopes is
    ignored (never written)."""
    from sudo_rm_rf_amd import original
    x, gamma, beta, sl, gout, gout2, gx0, p0, sums, refs = gln_case(shape)
    d = lambda t: t.to(DEV)
    args = (d(gout), d(x), d(sums), d(gamma), d(beta))
    full = [d(p0[0]), d(p0[1]), d(p0[2])]
    gx_full = original.gln_c_bwd(*args, slopes=d(sl), dgamma=full[0], dbeta=full[1], dslope=full[2])
    for hole in range(3):
        outs = [d(p0[0]), d(p0[1]), d(p0[2])]
        kw = {k: (None if i == hole else outs[i]) for i, k in enumerate(("dgamma", "dbeta", "dslope"))}
        gx = original.gln_c_bwd(*args, slopes=d(sl), **kw)
        assert torch.equal(gx, gx_full)
        assert all(torch.equal(outs[i], full[i]) for i in range(3) if i != hole) and torch.equal(outs[hole], d(p0[hole]))
    gx_none = original.gln_c_bwd(*args, slopes=d(sl))
    assert torch.equal(gx_none, gx_full)
    untouched = torch.full((shape[1],), 7.0, device=DEV)
    original.gln_c_bwd(*args, dslope=untouched)                     # no slopes: dslope is never written
    torch.cuda.synchronize()
    assert torch.equal(untouched, torch.full((shape[1],), 7.0, device=DEV))


def test_gln_c_bwd_dword_kernels_in_kernel_mode_1():
    from sudo_rm_rf_amd import ops, original
    shape = (2, 64, 130)
    x, gamma, beta, sl, gout, gout2, gx0, p0, sums, refs = gln_case(shape)
    d = lambda t: t.to(DEV)
    ops.set_kernel_mode(1)
    try:
        dg, db, ds = torch.zeros(64, device=DEV), torch.zeros(64, device=DEV), torch.zeros(64, device=DEV)
        with ops.kernel_trace(DEV) as tr:
            gx = original.gln_c_bwd(d(gout), d(x), d(sums), d(gamma), d(beta), slopes=d(sl), gout2=d(gout2), dgamma=dg, dbeta=db, dslope=ds)
        torch.cuda.synchronize()
    finally:
        ops.set_kernel_mode(0)
    assert tr.names == {"gln_c_bwd_reduce_scalar", "gln_c_bwd_apply_scalar"}
    r64, r32 = refs[(True, True)]
    for name, got, i in (("gx", gx, 0), ("dgamma", dg, 1), ("dbeta", db, 2), ("dslope", ds, 3)):
        bar_check("gln_c_bwd mode 1 " + name, got, r64[i], r32[i])


@pytest.mark.parametrize("mode", [0, 1], ids=["float4", "dword"])
@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 64, 130)], ids=lambda s: "g%d_C%d_L%d" % s)
def test_gln_c_bwd_zero_channels_take_the_slope(shape, mode):
    """The kink itself, which every case above stays away from: channels whose weight and bias are 0 have the pre-activation
    exactly 0 at every position.  torch's autograd gives PReLU's slope there (F.prelu: slope where x <= 0, -0.0 included), so
    their dgamma / dbeta are the slope times what the other side of the kink gives (gx is the same either way: gamma is 0).  Reference:
    fp64 autograd of F.prelu with per-channel slopes; bar: this file's rule."""
    import torch.nn.functional as F
    from sudo_rm_rf_amd import ops, original
    x, gamma, beta, sl, gout, gout2, gx0, p0, sums, refs = gln_case(shape)
    Cc = shape[1]
    dead = [0, Cc // 2, Cc - 1]
    gamma, beta = gamma.clone(), beta.clone()
    gamma[dead], beta[dead] = 0.0, 0.0

    def run(dt):
        xs, ga, be, s_ = (t.to(dt).clone().requires_grad_() for t in (x, gamma, beta, sl))
        (F.prelu(orf.gn(xs, ga, be), s_) * (gout.to(dt) + gout2.to(dt))).sum().backward()
        return xs.grad, ga.grad, be.grad, s_.grad
    r64, r32 = run(torch.float64), run(torch.float32)
    for i in (1, 2):                      # the dead channels are visible at the tensor's scale
        assert float(r64[i][dead].abs().max()) >= 1e-2 * float(r64[i].abs().max())
    d = lambda t: t.to(DEV)
    dg, db, ds = (torch.zeros(Cc, device=DEV) for _ in range(3))
    ops.set_kernel_mode(mode)
    try:
        with ops.kernel_trace(DEV) as tr:
            gx = original.gln_c_bwd(d(gout), d(x), d(sums), d(gamma), d(beta), slopes=d(sl), gout2=d(gout2), dgamma=dg, dbeta=db, dslope=ds)
        torch.cuda.synchronize()
    finally:
        ops.set_kernel_mode(0)
    suffix = "_scalar" if mode else ""
    assert tr.names == {"gln_c_bwd_reduce" + suffix, "gln_c_bwd_apply" + suffix}
    for name, got, i in (("gx", gx, 0), ("dgamma", dg, 1), ("dbeta", db, 2), ("dslope", ds, 3)):
        bar_check("gln_c_bwd kink %s mode %d %s" % (shape, mode, name), got, r64[i], r32[i])


# ---- srf_softmax_mask_bwd ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def softmax_case(S, N, L):
    Bt = 2
    g = torch.Generator().manual_seed(100 * S + N + L)
    z = (torch.randn(Bt, S * N, L, generator=g, dtype=torch.float64) * 2.0).float()
    enc = torch.relu(torch.randn(Bt, N, L, generator=g, dtype=torch.float64)).float()
    gv = torch.randn(Bt, S * N, L, generator=g, dtype=torch.float64).float()
    genc0 = torch.randn(Bt, N, L, generator=g, dtype=torch.float64).float()

    def run(dt):
        zz, ee = z.to(dt).clone().requires_grad_(), enc.to(dt).clone().requires_grad_()
        z4 = zz.view(Bt, S, N, L)
        p = torch.sigmoid(z4) if S == 1 else torch.softmax(z4, dim=1)
        ((p * ee.unsqueeze(1)).reshape(Bt, S * N, L) * gv.to(dt)).sum().backward()
        return zz.grad, ee.grad
    return z, enc, gv, genc0, run(torch.float64), run(torch.float32)


@pytest.mark.parametrize("shift", [1, 3], ids=["off4", "off12"])
@pytest.mark.parametrize("NL", [(6, 37), (64, 130)], ids=lambda s: "N%d_L%d" % s)
@pytest.mark.parametrize("S", [1, 2, 3, 9])
def test_softmax_mask_bwd(S, NL, shift):
    from sudo_rm_rf_amd import ops, original
    N, L = NL
    z, enc, gv, genc0, r64, r32 = softmax_case(S, N, L)
    a = arena()
    a.reset()
    zd, ed = a.put(z, shift_floats=shift, name="z"), a.put(enc, shift_floats=shift, name="enc")
    gvd = a.put(gv, shift_floats=shift, name="gv")
    gz = a.place(z.shape, shift_floats=shift, name="gz")
    genc = a.place(enc.shape, shift_floats=shift, name="genc")
    with ops.kernel_trace(DEV) as tr:
        original.softmax_mask_bwd(zd, ed, gvd, S, gz=gz, genc=genc)
    assert [n for n, _ in tr.launches] == ["softmax_mask_bwd"]
    # accumulating genc, and gz written over gv: the same bits
    genc_acc = a.put(genc0, shift_floats=shift, name="genc_acc")
    gv_alias = a.put(gv, shift_floats=shift, name="gv_alias")
    original.softmax_mask_bwd(zd, ed, gv_alias, S, gz=gv_alias, genc=genc_acc, accumulate_genc=True)
    torch.cuda.synchronize()
    a.check()
    for t in (gz, genc):
        a.assert_written(t)
        a.assert_clean(t)
    tag = "softmax_mask_bwd S=%d N=%d L=%d shift %d" % (S, N, L, shift)
    bar_check(tag + " gz", gz, r64[0], r32[0])
    bar_check(tag + " genc", genc, r64[1], r32[1])
    assert torch.equal(gv_alias, gz), "aliased gz differs"
    bar_check(tag + " genc accumulated", genc_acc, r64[1] + genc0.double(), r32[1] + genc0)


@pytest.mark.parametrize("S", [1, 2, 3, 9])
def test_softmax_mask_bwd_extreme_logits_stay_finite(S):
    """Logits of +-80 (and a whole column of each) give finite gradients, and rows that are saturated give the limits: p (1 - p)
    = 0 for the sigmoid, a one-hot softmax passes nothing to its logits."""
    from sudo_rm_rf_amd import original
    N, L = 6, 37
    z, enc, gv, _, _, _ = softmax_case(S, N, L)
    z = z.clone().view(2, S, N, L)
    z[0, :, 0, :] = 80.0
    z[0, :, 1, :] = -80.0
    z[1, 0, 2, :] = 80.0
    z[1, S - 1, 3, :] = -80.0
    z = z.view(2, S * N, L)
    gz, genc = original.softmax_mask_bwd(z.to(DEV), enc.to(DEV), gv.to(DEV), S)
    torch.cuda.synchronize()
    assert torch.isfinite(gz).all() and torch.isfinite(genc).all()
    z4 = z.double().view(2, S, N, L).clone().requires_grad_()
    p = torch.sigmoid(z4) if S == 1 else torch.softmax(z4, dim=1)
    ((p * enc.double().unsqueeze(1)).reshape(2, S * N, L) * gv.double()).sum().backward()
    assert float((gz.double().cpu() - z4.grad.view(2, S * N, L)).abs().max()) <= 1e-5


# ---- the fold, the contract, the bias gradient, the gate ---------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("N", [6, 64, 512])
def test_mask_weight_fold(N, S):
    """Against the fp64 sum over original_fixtures.toeplitz's index map; accumulated onto what dm.weight / dm.bias hold."""
    from sudo_rm_rf_amd import ops, original
    g = torch.Generator().manual_seed(N + S)
    dtz = torch.randn(S * N, N, generator=g, dtype=torch.float64).float()
    drow = torch.randn(S * N, generator=g, dtype=torch.float64).float()
    w0 = torch.randn(S, 1, N + 1, 1, generator=g, dtype=torch.float64).float()
    b0 = torch.randn(S, generator=g, dtype=torch.float64).float()
    idx = torch.from_numpy(otr.toeplitz_index(S, N)).reshape(-1)

    def ref(dt):
        acc = torch.zeros(S * (N + 1) + 1, dtype=dt).index_add_(0, idx, dtz.to(dt).reshape(-1))
        return w0.to(dt) + acc[1:].view(S, 1, N + 1, 1), b0.to(dt) + drow.to(dt).view(S, N).sum(1)
    a = arena()
    a.reset()
    dtz_d, drow_d = a.put(dtz, shift_floats=1, name="dtz"), a.put(drow, shift_floats=3, name="drow")
    outs = []
    for rep in range(2):
        dw, db = a.put(w0, shift_floats=3, name="dmw%d" % rep), a.put(b0, shift_floats=1, name="dmb%d" % rep)
        with ops.kernel_trace(DEV) as tr:
            original.mask_weight_fold(dtz_d, drow_d, dw, db)
        outs.append((dw, db))
    torch.cuda.synchronize()
    assert [n for n, _ in tr.launches] == ["mask_weight_fold"]
    a.check()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    (w64, b64), (w32, b32) = ref(torch.float64), ref(torch.float32)
    bar_check("mask_weight_fold N=%d S=%d weight" % (N, S), outs[0][0], w64, w32)
    bar_check("mask_weight_fold N=%d S=%d bias" % (N, S), outs[0][1], b64, b32)


@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("NK", [(6, 9), (64, 21), (512, 21)], ids=lambda s: "N%d_K%d" % s)
def test_decoder_weight_contract_is_bit_exact(NK, S):
    from sudo_rm_rf_amd import original
    N, K = NK
    g = torch.Generator().manual_seed(N + K + S)
    dwexp = torch.randn(S * N, S, K, generator=g, dtype=torch.float64).float()
    w0 = torch.randn(S * N, 1, K, generator=g, dtype=torch.float64).float()
    diag = torch.stack([dwexp[c, c // N] for c in range(S * N)]).view(S * N, 1, K)
    a = arena()
    a.reset()
    src = a.put(dwexp, shift_floats=1, name="dwexp")
    onto_zero = a.put(torch.zeros_like(w0), shift_floats=3, name="dw_zero")
    onto_w0 = a.put(w0, shift_floats=1, name="dw")
    original.decoder_weight_contract(src, onto_zero)
    original.decoder_weight_contract(src, onto_w0)
    torch.cuda.synchronize()
    a.check()
    assert torch.equal(onto_zero.cpu(), diag) and torch.equal(onto_w0.cpu(), w0 + diag)
    # the transpose of the forward's copy: expanding what was contracted puts the diagonal blocks back
    assert torch.equal(original.decoder_weight_expand(onto_zero.contiguous(), S).cpu(), torch.from_numpy(of.expand_decoder(diag.numpy(), S)))


@pytest.mark.parametrize("shape", [(2, 2, 1001), (3, 3, 20000), (1, 1, 5)], ids=lambda s: "B%d_S%d_T%d" % s)
def test_decoder_bias_grad(shape):
    from sudo_rm_rf_amd import ops, original
    g = torch.Generator().manual_seed(sum(shape))
    go = (torch.randn(shape, generator=g, dtype=torch.float64) + 0.1).float()
    b0 = torch.randn(shape[1], generator=g, dtype=torch.float64).float()
    a = arena()
    a.reset()
    god = a.put(go, shift_floats=1, name="grad_out")
    outs = []
    for rep in range(2):
        db = a.put(b0, shift_floats=3, name="dbias%d" % rep)
        with ops.kernel_trace(DEV) as tr:
            original.decoder_bias_grad(god, db)
        outs.append(db)
    torch.cuda.synchronize()
    assert [n for n, _ in tr.launches] == ["decoder_bias_part", "decoder_bias_fold"]
    a.check()
    assert torch.equal(outs[0], outs[1])
    bar_check("decoder_bias_grad %s" % (shape,), outs[0], b0.double() + go.double().sum((0, 2)), b0 + go.sum((0, 2)))


@pytest.mark.parametrize("shifts", [(1, 1), (3, 3), (0, 0), (1, 3)], ids=lambda s: "g%d_s%d" % s)
@pytest.mark.parametrize("n", [1, 7, 1000, 5003])
def test_relu_gate_is_bit_exact(n, shifts):
    from sudo_rm_rf_amd import ops, original
    gen = torch.Generator().manual_seed(n)
    g = torch.randn(n, generator=gen, dtype=torch.float64).float()
    s = torch.relu(torch.randn(n, generator=gen, dtype=torch.float64)).float()       # about half exact zeros
    a = arena()
    a.reset()
    gd, sd = a.put(g, shift_floats=shifts[0], name="g"), a.put(s, shift_floats=shifts[1], name="s")
    with ops.kernel_trace(DEV) as tr:
        original.relu_gate(gd, sd)
    torch.cuda.synchronize()
    assert [n_ for n_, _ in tr.launches] == ["relu_gate"]
    a.check()
    assert torch.equal(gd.cpu(), torch.where(s > 0, g, torch.zeros_like(g)))
    assert torch.equal(sd.cpu(), s)


# ---- PermInvariantSISDR as run_sudormrf.py's training loss (srf_perm_inv_sisdr_backward) -----------------------------------------------
# (batch, sources, T, zero_mean, improvement, individual results): the runner's configuration | three sources, no centring | one
# source | five sources (the generic statistics kernel) with per-example results and their own upstream weights
PERM_INV_CASES = [(3, 2, 1001, True, True, False), (2, 3, 4500, False, False, False), (2, 1, 37, True, True, False),
                  (2, 5, 333, True, False, True)]


@pytest.mark.parametrize("case", PERM_INV_CASES, ids=lambda c: "B%d_S%d_T%d_zm%d_imp%d_ind%d" % c)
def test_perm_invariant_sisdr_backward(case):
    """The gradient w.r.t. the estimates against fp64 autograd over the class's formula (tests/original_train_ref
    .perm_inv_sisdr_loss, the torch form of oracle.loss_oracle.perm_invariant_sisdr); bar: 8 x torch's own fp32 autograd.  The
    value is the evaluation path's, bit for bit; a second backward gives the same bits; the metric form keeps refusing."""
    import sudo_rm_rf.dnn.losses.sisdr as sisdr_lib
    from oracle.loss_oracle import make_loss_case
    Bt, S, T, zm, imp, ind = case
    est, tgt = make_loss_case(Bt, S, T, 77 + S, 5.0, "noisy")
    est, tgt = torch.from_numpy(est), torch.from_numpy(tgt)
    mix = tgt.sum(1, keepdim=True)
    wts = torch.randn(Bt, generator=torch.Generator().manual_seed(T), dtype=torch.float64).float()

    def ref(dt):
        e = est.to(dt).clone().requires_grad_()
        v = otr.perm_inv_sisdr_loss(e, tgt.to(dt), mix.to(dt) if imp else None, zm, imp, True, ind)
        (v * wts.to(dt)).sum().backward() if ind else v.backward()
        return v.detach(), e.grad
    (v64, g64), (_, g32) = ref(torch.float64), ref(torch.float32)
    fn = sisdr_lib.PermInvariantSISDR(batch_size=Bt, n_sources=S, zero_mean=zm, backward_loss=True, improvement=imp,
                                      return_individual_results=ind)
    kw = dict(initial_mixtures=mix.to(DEV)) if imp else {}
    grads = []
    for _ in range(2):
        e = est.to(DEV).requires_grad_()
        v = fn(e, tgt.to(DEV), **kw)
        ((v * wts.to(DEV)).sum() if ind else v).backward()
        grads.append(e.grad)
    torch.cuda.synchronize()
    with torch.no_grad():
        assert torch.equal(fn(est.to(DEV), tgt.to(DEV), **kw), v.detach())
    assert float((v.detach().cpu().double() - v64).abs().max()) <= 1e-4
    assert torch.equal(grads[0], grads[1])
    bar_check("perm_inv_sisdr_backward %s" % (case,), grads[0], g64, g32)
    metric = sisdr_lib.PermInvariantSISDR(batch_size=Bt, n_sources=S, zero_mean=zm, backward_loss=False, improvement=imp)
    with pytest.raises(NotImplementedError):
        metric(est.to(DEV).requires_grad_(), tgt.to(DEV), **kw)
    with pytest.raises(NotImplementedError):
        fn(est.to(DEV), tgt.to(DEV).requires_grad_(), **kw)
