"""srf_mha_attention_lse / srf_mha_attention_bwd, the autograd op behind attention.mha_attention and
MHAttentionLayer.enable_hip_training() against fp64 autograd on the CPU (tests.attentive_ref.attention).

The bar of the raw kernels is the forward test's (tests/test_gpu_attention.py): the SAME autograd call in fp32 on the CPU
deviates from the fp64 one by some max-abs amount per tensor; the kernel may deviate by 8 times that.  Where the yardstick is
exactly zero -- gq and gk with a single key: P = 1, dP = delta in exact arithmetic, the reference gradients are exact zeros --
the kernel, which forms dP and delta as two fp32 dot products over the same d terms in different orders, gets a floor instead:
8 * 2^-24 * sqrt(d) * max|go| * max|v| * scale * max|k| for gq (max|q| for gk), a rounding estimate with the forward's margin
of 8, not a measurement.  Inputs are drawn as the forward test draws them, plus a seeded normal go.  The layer is held to
2e-4 of each tensor's largest reference entry, the bar of tests/test_gpu_causal_train.py for tiny gradient cases on the
split-bf16 GEMMs -- with one tensor the bar as worded cannot apply to: K_proj.bias.  Its exact gradient is ZERO (the bias
shifts every key's score of a query by the same amount, which the softmax ignores: sum_lk dS[lq, lk] = 0), the fp64
reference holds 1e-16 of its own rounding there, and 2e-4 of that would refuse the exact answer 0.0 as well.  Following what
the raw kernels do where their yardstick is exactly zero, that one tensor is measured against the size of what cancels
instead: 2e-4 of max_c sum_{b, lk} |gk_ref[b, c, lk]|, the terms of its sum taken from the fp64 reference, never from the
kernel (measured: errors of 1.0e-7 and 5.5e-7 beside cancelling terms of order 1).  Dispatch is asserted by profiler name;
placement runs off the 16-byte grid in tests/placement.py's arena."""
import ctypes as C
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from tests import attentive_ref as ar
from tests import placement as pl

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# the forward test's SHAPES
FWD_SHAPES = [(2, 3, 16, 26, 26), (3, 1, 64, 2, 2), (1, 4, 256, 1, 1), (2, 4, 256, 130, 130), (1, 3, 256, 202, 202),
              (1, 3, 256, 201, 201), (1, 2, 32, 321, 321), (2, 3, 24, 25, 25), (2, 1, 64, 70, 45),
              (1, 2, 48, 33, 33), (1, 1, 80, 5, 37), (1, 1, 144, 40, 70)]
# (Bt, H, d, Lq, Lk): one key, one query, fewer keys than a tile, tile edges at 31 / 32 / 33 / 65, Lq != Lk both ways, head
# dimensions that leave a 32-channel chunk half full (16, 48, 80, 144) or skipped (80, 144), the two-pass form (256), generic (24)
BWD_SHAPES = [(2, 3, 16, 26, 26), (3, 1, 64, 2, 2), (1, 4, 256, 1, 1), (1, 1, 16, 40, 1), (1, 1, 16, 1, 40),
              (2, 4, 256, 130, 130), (2, 1, 64, 70, 45), (2, 1, 64, 45, 70), (1, 2, 32, 31, 65), (1, 2, 48, 33, 33),
              (1, 1, 80, 5, 37), (1, 1, 144, 40, 70), (2, 3, 24, 25, 25)]
LARGE = (2, 4, 256, 130, 130)          # run once more with logits of +-80
NAMES = ("gq", "gk", "gv")


def _id(s):
    return "B%d_H%d_d%d_Lq%d_Lk%d" % s


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


def draw(shape, q_gain=1.0):
    """q, k, v as tests/test_gpu_attention.py draws them, then go from the same generator"""
    Bt, H, d, Lq, Lk = shape
    g = torch.Generator().manual_seed(1000 * d + Lq + 7 * Lk)
    q = (torch.randn(Bt, H * d, Lq, generator=g, dtype=torch.float64) * q_gain).float()
    k = torch.randn(Bt, H * d, Lk, generator=g, dtype=torch.float64).float()
    v = torch.randn(Bt, H * d, Lk, generator=g, dtype=torch.float64).float()
    go = torch.randn(Bt, H * d, Lq, generator=g, dtype=torch.float64).float()
    return q, k, v, go


def cpu_grads(q, k, v, go, H, dtype):
    q, k, v = (t.detach().to(dtype, copy=True).requires_grad_() for t in (q, k, v))      # (never the caller's own tensors)
    return torch.autograd.grad(ar.attention(q, k, v, H), (q, k, v), go.to(dtype))


def yardstick(q, k, v, go, H):
    """(fp64 reference gradients, max-abs deviation of the same call in fp32 on the CPU), per tensor"""
    ref = cpu_grads(q, k, v, go, H, torch.float64)
    f32 = cpu_grads(q, k, v, go, H, torch.float32)
    return ref, [(a.double() - b).abs().max().item() for a, b in zip(f32, ref)]


@functools.lru_cache(maxsize=None)
def case(shape, q_gain=1.0):
    """(q, k, v, go in fp32, fp64 reference gradients, fp32 deviations): once per shape, shared, never written to"""
    q, k, v, go = draw(shape, q_gain)
    ref, dev32 = yardstick(q, k, v, go, shape[1])
    return q, k, v, go, ref, dev32


def floors(q, k, v, go, shape):
    """the single-key floor of gq and gk (module docstring); gv has none"""
    d = shape[2]
    f = 8 * 2.0 ** -24 * math.sqrt(d) * go.abs().max().item() * v.abs().max().item() / math.sqrt(d)
    return [f * k.abs().max().item(), f * q.abs().max().item(), 0.0]


def check(got, shape, inputs, ref, dev32, what=""):
    q, k, v, go = inputs
    fl = floors(q, k, v, go, shape) if shape[4] == 1 else [0.0, 0.0, 0.0]
    bad = []
    for name, g, r, dv, f in zip(NAMES, got, ref, dev32, fl):
        assert g.shape == r.shape
        assert torch.isfinite(g).all(), name
        err = (g.double().cpu() - r).abs().max().item()
        bar = max(8 * dv, f)
        print("%s %s %s: kernel err %.3e, torch fp32 dev %.3e, floor %.3e, bar %.3e, max|ref| %.3e"
              % (_id(shape), what, name, err, dv, f, bar, r.abs().max().item()))
        if not err <= bar:
            bad.append((name, err, bar))
    assert not bad, bad


def dev(*ts):
    return [t.to(DEV) for t in ts]


def run(shape, q_gain=1.0):
    """forward with lse + backward on the device; the trace covers the backward only"""
    from sudo_rm_rf_amd import attention, ops
    q, k, v, go = dev(*case(shape, q_gain)[:4])
    o, lse = attention.mha_attention_lse(q, k, v, shape[1])
    with ops.kernel_trace(DEV) as tr:
        got = attention.mha_attention_bwd(q, k, v, o, lse, go, shape[1])
    torch.cuda.synchronize()
    return got, tr


def expected_kernels(d):
    from sudo_rm_rf_amd import attention
    if not attention.mha_attention_bwd_mfma_supported(d):
        return ["mha_attention_bwd_delta", "mha_attention_bwd_dq_generic", "mha_attention_bwd_dkv_generic"]
    if d <= 128:
        return ["mha_attention_bwd_delta", "mha_attention_bwd_dq_mfma", "mha_attention_bwd_dkv_mfma"]
    return ["mha_attention_bwd_delta", "mha_attention_bwd_dq_mfma", "mha_attention_bwd_dv_mfma", "mha_attention_bwd_dk_mfma"]


# ---- 1. the forward with lse ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", FWD_SHAPES, ids=_id)
def test_forward_with_lse_keeps_the_output_bits_and_the_plain_kernel_its_name(shape):
    from sudo_rm_rf_amd import attention, ops
    Bt, H, d, Lq, Lk = shape
    q, k, v, _ = draw(shape)
    dq, dk, dv = dev(q, k, v)
    with ops.kernel_trace(DEV) as tr_plain:
        plain = attention.mha_attention(dq, dk, dv, H)
    with ops.kernel_trace(DEV) as tr_lse:
        o, lse = attention.mha_attention_lse(dq, dk, dv, H)
    torch.cuda.synchronize()
    mfma = attention.mha_attention_mfma_supported(d)
    assert mfma == (d % 16 == 0 and 16 <= d <= 256)
    assert [n for n, _ in tr_plain.launches] == ["mha_attention_mfma" if mfma else "mha_attention_generic"]
    assert [n for n, _ in tr_lse.launches] == ["mha_attention_lse_mfma" if mfma else "mha_attention_lse_generic"]
    assert torch.equal(o, plain)

    def lse_of(dtype):
        s = torch.einsum("bhdl,bhds->bhls", (q.to(dtype) * (1.0 / math.sqrt(d))).reshape(Bt, H, d, Lq), k.to(dtype).reshape(Bt, H, d, Lk))
        return torch.logsumexp(s, dim=-1)
    ref = lse_of(torch.float64)
    dev32 = (lse_of(torch.float32).double() - ref).abs().max().item()
    assert lse.shape == ref.shape and torch.isfinite(lse).all()
    err = (lse.double().cpu() - ref).abs().max().item()
    print("%s lse: kernel err %.3e, torch fp32 dev %.3e, bar %.3e" % (_id(shape), err, dev32, 8 * dev32))
    assert err <= 8 * dev32


# ---- 2. the backward against fp64 autograd ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", BWD_SHAPES, ids=_id)
def test_backward_matches_fp64_autograd_and_dispatch(shape):
    got, tr = run(shape)
    names = [n for n, _ in tr.launches]
    assert all(n.startswith("mha_attention_bwd") for n in names)
    assert names == expected_kernels(shape[2])
    q, k, v, go, ref, dev32 = case(shape)
    check(got, shape, (q, k, v, go), ref, dev32)


# ---- 3. large logits --------------------------------------------------------------------------------------------------
def test_backward_large_logits_stay_finite_and_correct():
    q, k, v, go, ref, dev32 = case(LARGE, 20.0)
    logits = torch.einsum("bhdl,bhds->bhls", q.double().reshape(2, 4, 256, -1), k.double().reshape(2, 4, 256, -1)) / 16.0
    assert logits.abs().max().item() >= 80.0
    got, tr = run(LARGE, 20.0)
    assert [n for n, _ in tr.launches] == expected_kernels(256)
    check(got, LARGE, (q, k, v, go), ref, dev32, "gain 20")


# ---- 4. kernel mode 1 -------------------------------------------------------------------------------------------------
def test_generic_backward_serves_mfma_shapes_in_kernel_mode_1():
    from sudo_rm_rf_amd import attention, ops
    shape = (2, 3, 16, 26, 26)
    ops.set_kernel_mode(1)
    try:
        assert not attention.mha_attention_bwd_mfma_supported(16)
        got, tr = run(shape)
    finally:
        ops.set_kernel_mode(0)
    assert [n for n, _ in tr.launches] == ["mha_attention_bwd_delta", "mha_attention_bwd_dq_generic", "mha_attention_bwd_dkv_generic"]
    q, k, v, go, ref, dev32 = case(shape)
    check(got, shape, (q, k, v, go), ref, dev32, "mode 1")


# ---- 5. determinism ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 4, 256, 130, 130), (2, 1, 64, 70, 45)], ids=_id)
def test_backward_is_deterministic(shape):
    a, _ = run(shape)
    b, _ = run(shape)
    for name, x, y in zip(NAMES, a, b):
        assert torch.equal(x, y), name


# ---- 6. placement -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def arena():
    return pl.Arena(DEV, 64 << 20)


@functools.lru_cache(maxsize=None)
def forward_on_host(shape):
    from sudo_rm_rf_amd import attention
    q, k, v = dev(*case(shape)[:3])
    o, lse = attention.mha_attention_lse(q, k, v, shape[1])
    return o.cpu(), lse.cpu()


@pytest.mark.parametrize("shape", [(2, 3, 16, 26, 26), (2, 4, 256, 130, 130), (2, 3, 24, 25, 25), (2, 1, 64, 70, 45)], ids=_id)
@pytest.mark.parametrize("shifts", [(0,) * 10, (1, 2, 3, 1, 2, 3, 1, 2, 3, 1), (3, 1, 2, 3, 1, 2, 3, 3, 2, 1)],
                         ids=lambda s: "shift" + "".join(map(str, s)))
def test_backward_off_the_16_byte_grid_with_guard_bands(arena, shape, shifts):
    from sudo_rm_rf_amd import attention
    Bt, H, d, Lq, Lk = shape
    q, k, v, go, ref, dev32 = case(shape)
    o, lse = forward_on_host(shape)
    arena.reset()
    host = (q, k, v, o, lse, go)
    ins = [arena.put(t, shift_floats=s, name=n) for t, s, n in zip(host, shifts, ("q", "k", "v", "o", "lse", "go"))]
    outs = [arena.place(t.shape, shift_floats=s, name=n) for t, s, n in zip((q, k, v), shifts[6:9], NAMES)]
    ws = arena.place((attention.mha_attention_bwd_workspace_bytes(Bt, H, d, Lq, Lk) // 4,), shift_floats=shifts[9], name="workspace")
    for t in outs:
        t.fill_(float("nan"))
    attention.mha_attention_bwd(*ins, H, gq=outs[0], gk=outs[1], gv=outs[2], workspace=ws)
    torch.cuda.synchronize()
    arena.check()
    for t in outs:
        arena.assert_clean(t)
    for t, h in zip(ins, host):
        assert torch.equal(t.cpu(), h)
    check(outs, shape, (q, k, v, go), ref, dev32, "shifts %s" % (shifts,))


# ---- 7. degenerate signals --------------------------------------------------------------------------------------------
def _bwd(q, k, v, go, H):
    from sudo_rm_rf_amd import attention
    q, k, v, go = dev(q, k, v, go)
    o, lse = attention.mha_attention_lse(q, k, v, H)
    got = attention.mha_attention_bwd(q, k, v, o, lse, go, H)
    torch.cuda.synchronize()
    for name, g in zip(NAMES, got):
        assert torch.isfinite(g).all(), name
    return got


@pytest.mark.parametrize("shape", [(2, 3, 16, 26, 26), (2, 1, 64, 70, 45), (2, 3, 24, 25, 25)], ids=_id)
def test_backward_degenerate_signals(shape):
    Bt, H, d, Lq, Lk = shape
    q, k, v, go = draw(shape)
    z = torch.zeros_like
    # go = 0: every gradient is exactly 0
    for name, g in zip(NAMES, _bwd(q, k, v, z(go), H)):
        assert torch.equal(g.cpu(), torch.zeros_like(g.cpu())), name
    # q = k = 0: P is uniform, gv[j, lk] = sum_lq go[j, lq] / Lk, gq = 0 (k = 0) -- within the bar of these inputs
    ref, dev32 = yardstick(z(q), z(k), v, go, H)
    got = _bwd(z(q), z(k), v, go, H)
    uniform = go.double().sum(-1, keepdim=True).expand(-1, -1, Lk) / Lk
    assert (ref[2] - uniform).abs().max().item() <= 1e-12
    assert ref[0].abs().max().item() == 0.0
    check(got, shape, (z(q), z(k), v, go), ref, dev32, "q = k = 0")
    # v = 0: o = 0, delta = dP = 0, so gq = gk = 0 within the floor -- which max|v| = 0 makes 0
    ref, dev32 = yardstick(q, k, z(v), go, H)
    assert ref[0].abs().max().item() == 0.0 and ref[1].abs().max().item() == 0.0
    got = _bwd(q, k, z(v), go, H)
    fl = floors(q, k, z(v), go, shape)
    assert got[0].abs().max().item() <= fl[0] and got[1].abs().max().item() <= fl[1]
    check(got, shape, (q, k, z(v), go), ref, dev32, "v = 0")


# ---- 8. refusals ------------------------------------------------------------------------------------------------------
def test_backward_refuses_bad_arguments_before_launching():
    from sudo_rm_rf_amd import _lib, attention, ops
    from sudo_rm_rf_amd._lib import SrfError
    q = torch.zeros(1, 2 * 1040, 3, device=DEV)
    lse = torch.zeros(1, 2, 3, device=DEV)
    with ops.kernel_trace(DEV) as tr:
        with pytest.raises(SrfError, match="d = 1040"):
            attention.mha_attention_bwd(q, q, q, q, lse, q, 2)
        with pytest.raises(SrfError, match="heads"):
            attention.mha_attention_bwd(q, q, q, q, lse, q, 7)
        q = torch.zeros(1, 2 * 16, 5, device=DEV)
        lse = torch.zeros(1, 2, 5, device=DEV)
        need = attention.mha_attention_bwd_workspace_bytes(1, 2, 16, 5, 5)
        assert need == 2 * 5 * 4
        with pytest.raises(SrfError, match="workspace"):          # a null workspace: only the C entry point can be handed one
            p, st = _lib.ptr(q), _lib.current_stream(torch.device(DEV))
            g = [_lib.ptr(torch.empty_like(q)) for _ in range(3)]
            rc = _lib.load().srf_mha_attention_bwd(p, p, p, p, _lib.ptr(lse), p, g[0], g[1], g[2], None, 1, 2, 16, 5, 5,
                                                   C.c_float(0.25), st)
            _lib.check(rc, "srf_mha_attention_bwd")
        with pytest.raises(SrfError, match="workspace"):
            attention.mha_attention_bwd(q, q, q, q, lse, q, 2, workspace=torch.empty(need - 4, dtype=torch.uint8, device=DEV))
        with pytest.raises(SrfError, match="lse"):
            attention.mha_attention_bwd(q, q, q, q, torch.zeros(1, 2, 4, device=DEV), q, 2)
        with pytest.raises(SrfError, match="lse"):
            attention.mha_attention_lse(q, q, q, 2, lse=torch.zeros(1, 2, 6, device=DEV))
    assert tr.launches == []


# ---- 9. the autograd op -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 16, 26, 26), (2, 1, 64, 70, 45), (2, 3, 24, 25, 25)], ids=_id)
def test_autograd_through_mha_attention_is_the_raw_backward(shape):
    from sudo_rm_rf_amd import attention, ops
    H = shape[1]
    q, k, v, go = dev(*case(shape)[:4])
    o_raw, lse = attention.mha_attention_lse(q, k, v, H)
    raw = attention.mha_attention_bwd(q, k, v, o_raw, lse, go, H)
    qg, kg, vg = (t.clone().requires_grad_() for t in (q, k, v))
    o = attention.mha_attention(qg, kg, vg, H)
    assert o.grad_fn is not None and torch.equal(o.detach(), attention.mha_attention(q, k, v, H))
    for name, a, b in zip(NAMES, torch.autograd.grad(o, (qg, kg, vg), go), raw):
        assert torch.equal(a, b), name
    # only v requires grad: gv alone comes back, and it is the same gv
    vg = v.clone().requires_grad_()
    o = attention.mha_attention(q, k, vg, H)
    assert o.grad_fn is not None
    o.backward(go)
    assert torch.equal(vg.grad, raw[2]) and q.grad is None and k.grad is None
    _, _, _, _, ref, dev32 = case(shape)
    err = (vg.grad.double().cpu() - ref[2]).abs().max().item()
    assert err <= 8 * dev32[2]
    # no_grad, or nothing requiring grad: the plain forward kernel only
    plain = "mha_attention_mfma" if attention.mha_attention_mfma_supported(shape[2]) else "mha_attention_generic"
    with ops.kernel_trace(DEV) as tr:
        with torch.no_grad():
            attention.mha_attention(qg, kg, vg, H)
        out = attention.mha_attention(q, k, v, H)
    assert [n for n, _ in tr.launches] == [plain, plain] and out.grad_fn is None


# ---- 10. MHAttentionLayer ---------------------------------------------------------------------------------------------
SMALL_TOL = 2e-4          # tests/test_gpu_causal_train.py


def layer_ref(Q, K, V, par, H):
    """the layer restated in fp64: four nn.Linear around ar.attention (which scales by 1 / sqrt(d_model)); -> (output, k)"""
    wq, bq, wk, bk, wv, bv, wo, bo = par
    lin = lambda x, w, b: F.linear(x, w, b).transpose(1, 2)
    k = lin(K, wk, bk)
    o = ar.attention(lin(Q, wq, bq), k, lin(V, wv, bv), H)
    return F.linear(o.transpose(1, 2), wo, bo), k


@pytest.mark.parametrize("emb,d_model,H,B,Lq,Lk", [(24, 16, 3, 2, 26, 26), (128, 64, 1, 2, 70, 45)], ids=["self", "cross"])
def test_mha_layer_trains_on_hip_after_the_opt_in(emb, d_model, H, B, Lq, Lk):
    from sudo_rm_rf_amd.dnn.models.attentive_sudormrf_v2 import MHAttentionLayer
    from sudo_rm_rf_amd.dnn.models import attentive_sudormrf_v3 as v3
    assert v3.MHAttentionLayer is MHAttentionLayer          # one class, one method
    torch.manual_seed(emb + Lq)
    layer = MHAttentionLayer(emb, d_model, H).to(DEV).eval()
    g = torch.Generator().manual_seed(7 * emb + Lk)
    xq = torch.randn(B, Lq, emb, generator=g, dtype=torch.float64).float()
    xkv = xq if Lq == Lk else torch.randn(B, Lk, emb, generator=g, dtype=torch.float64).float()
    gy = torch.randn(B, Lq, emb, generator=g, dtype=torch.float64).float()
    dq = xq.to(DEV).requires_grad_()
    dkv = dq if Lq == Lk else xkv.to(DEV).requires_grad_()
    # without the opt-in: the inference forward, no grad_fn
    y0 = layer(dq, dkv, dkv)
    assert y0.grad_fn is None and not y0.requires_grad
    assert layer.enable_hip_training() is layer
    y = layer(dq, dkv, dkv)
    assert y.grad_fn is not None and torch.equal(y.detach(), y0)
    with torch.no_grad():
        assert layer(dq, dkv, dkv).grad_fn is None
    par = [p for m in (layer.Q_proj, layer.K_proj, layer.V_proj, layer.O_proj) for p in (m.weight, m.bias)]
    ins = [dq] if dkv is dq else [dq, dkv]
    got = torch.autograd.grad(y, ins + par, gy.to(DEV))
    torch.cuda.synchronize()
    # fp64 restatement on the same values
    rq = xq.double().requires_grad_()
    rkv = rq if Lq == Lk else xkv.double().requires_grad_()
    rpar = [p.detach().double().cpu().requires_grad_() for p in par]
    yr, rk = layer_ref(rq, rkv, rkv, rpar, H)
    assert (y.detach().double().cpu() - yr.detach()).abs().max().item() <= SMALL_TOL * yr.abs().max().item()
    want = torch.autograd.grad(yr, ([rq] if rkv is rq else [rq, rkv]) + rpar + [rk], gy.double())
    want, gk_ref = want[:-1], want[-1]
    names = (["x"] if dkv is dq else ["Q", "KV"]) + ["%s_proj.%s" % (m, w) for m in "QKVO" for w in ("weight", "bias")]
    bad = []
    for name, a, b in zip(names, got, want):
        assert a.shape == b.shape and torch.isfinite(a).all(), name
        err, top = (a.double().cpu() - b).abs().max().item(), b.abs().max().item()
        if name == "K_proj.bias":          # exactly zero by the softmax's shift invariance: the size of what cancels (docstring)
            assert top <= 1e-12
            top = gk_ref.abs().sum(dim=(0, 2)).max().item()
        print("%s: err %.3e, max|ref| %.3e, relative %.3e" % (name, err, top, err / top))
        if not err <= SMALL_TOL * top:
            bad.append((name, err / top))
    assert not bad, bad
    layer.enable_hip_training(False)
    assert layer(dq, dkv, dkv).grad_fn is None


def test_mha_layer_with_random_dropout_still_refuses_train_mode():
    from sudo_rm_rf_amd.dnn.models.attentive_sudormrf_v2 import MHAttentionLayer
    layer = MHAttentionLayer(24, 16, 3, dropout=0.1).to(DEV).enable_hip_training().train()
    x = torch.zeros(2, 26, 24, device=DEV, requires_grad=True)
    with pytest.raises(RuntimeError, match="dropout"):
        layer(x, x, x)
