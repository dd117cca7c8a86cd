"""The ragged attention forms (srf_mha_attention_ragged, _lse_ragged, _bwd_ragged), the lengths keywords of
attention.mha_attention / mha_attention_lse / mha_attention_bwd, and MHAttentionLayer.forward(Q, K, V, q_lengths, k_lengths).

The requirement is BIT IDENTITY per example: inside its lengths example b of a ragged call holds the bits of the existing uniform
functions called on that example's contiguous slices at its own lengths (torch.equal), and exact zeros past them.  That carries
the accuracy established for the uniform kernels (tests/test_gpu_attention.py, tests/test_gpu_attention_bwd.py) over; the rule
itself -- attention on the slices IS masked attention -- is checked in fp64 on the CPU (tests/test_attention_ragged_host.py) and
once more directly here, against tests.attentive_ref.attention in fp64 on the slices, with the uniform tests' bar: 8 times the
deviation of the same call in fp32 on the CPU, per tensor, and tests/test_gpu_attention_bwd.py's single-key floor for gq / gk
where k_len = 1.  The layer is held to that file's layer bar: 2e-4 of each tensor's largest reference entry, K_proj.bias (exact
gradient zero) to 2e-4 of the size of what cancels."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from tests import attentive_ref as ar
from tests import placement as pl

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("o", "lse", "gq", "gk", "gv")

# ((Bt, H, d, Lq, Lk), q_lengths, k_lengths); None = NULL on that side
CASES = [
    ((4, 3, 16, 40, 40), [40, 33, 32, 1], [40, 33, 32, 1]),     # full row, tile edges at 32 / 33, a single query and key
    ((3, 1, 64, 70, 45), [70, 31, 1], [45, 1, 33]),             # independent sides, a single key beside many queries
    ((3, 4, 256, 130, 130), [130, 65, 97], [130, 65, 97]),      # the <8> forms and the two-pass key side
    ((2, 1, 80, 37, 70), [5, 37], [70, 31]),                    # a half-filled and a skipped chunk
    ((2, 3, 24, 25, 25), [25, 7], [25, 7]),                     # generic forms
    ((2, 1, 64, 70, 45), None, [45, 20]),                       # one side only
    ((2, 1, 64, 70, 45), [70, 9], None),                        # the converse
    ((128, 1, 16, 8, 8), [1 + b % 8 for b in range(128)], [1 + b % 8 for b in range(128)]),   # the batch cap
]
D256, GENERIC, MFMA64 = 2, 4, 1


def _id(i):
    (Bt, H, d, Lq, Lk), ql, kl = CASES[i]
    return "B%d_H%d_d%d_Lq%d_Lk%d_%s%s" % (Bt, H, d, Lq, Lk, "q" if ql else "-", "k" if kl else "-")


ALL = pytest.mark.parametrize("ci", range(len(CASES)), ids=_id)


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


def full(ci):
    """the two length lists with None spelled out"""
    (Bt, H, d, Lq, Lk), ql, kl = CASES[ci]
    return (ql or [Lq] * Bt), (kl or [Lk] * Bt)


@functools.lru_cache(maxsize=None)
def draw(ci, seed=0):
    """q, k, v, go in fp32 on the host (finite everywhere): once per case, shared, never written to"""
    (Bt, H, d, Lq, Lk), _, _ = CASES[ci]
    g = torch.Generator().manual_seed(1000 * d + Lq + 7 * Lk + 100003 * seed)
    r = lambda L: torch.randn(Bt, H * d, L, generator=g, dtype=torch.float64).float()
    return r(Lq), r(Lk), r(Lk), r(Lq)


def dev(*ts):
    return [t.to(DEV) for t in ts]


def ragged_call(ci, q, k, v, go, poison=False, **outs):
    """plain forward, forward with lse and backward of case ci on device tensors -> (o, lse, gq, gk, gv); poison: o and lse
    are NaN past the query lengths before the backward reads them, outputs and the workspace start as 0xFF"""
    from sudo_rm_rf_amd import attention
    (Bt, H, d, Lq, Lk), ql, kl = CASES[ci]
    kw = dict(q_lengths=ql, k_lengths=kl)
    ff = lambda shape: torch.full(shape, float("nan"), device=DEV).view(torch.int32).fill_(-1).view(torch.float32)
    if poison:
        o_plain = attention.mha_attention(q, k, v, H, out=ff(q.shape), **kw)
        o, lse = attention.mha_attention_lse(q, k, v, H, out=ff(q.shape), lse=ff((Bt, H, Lq)), **kw)
    else:
        o_plain = attention.mha_attention(q, k, v, H, **kw)
        o, lse = attention.mha_attention_lse(q, k, v, H, **kw)
    assert torch.equal(o_plain.view(torch.int32), o.view(torch.int32))
    o_in, lse_in = o, lse
    if poison:
        o_in, lse_in = o.clone(), lse.clone()
        for b, n in enumerate(full(ci)[0]):
            o_in[b, :, n:] = float("nan")
            lse_in[b, :, n:] = float("nan")
        need = attention.mha_attention_bwd_workspace_bytes(Bt, H, d, Lq, Lk)
        outs = dict(gq=ff(q.shape), gk=ff(k.shape), gv=ff(v.shape), workspace=torch.full((need,), 255, dtype=torch.uint8, device=DEV))
    g = attention.mha_attention_bwd(q, k, v, o_in, lse_in, go, H, **outs, **kw)
    torch.cuda.synchronize()
    return (o, lse) + tuple(g)


@functools.lru_cache(maxsize=None)
def ragged_run(ci):
    return tuple(t.cpu() for t in ragged_call(ci, *dev(*draw(ci))))


@functools.lru_cache(maxsize=None)
def per_example(ci):
    """the existing UNIFORM functions on each example's contiguous slices at its own lengths -> [(o, lse, gq, gk, gv)] on the host"""
    from sudo_rm_rf_amd import attention
    H = CASES[ci][0][1]
    q, k, v, go = draw(ci)
    out = []
    for b, (nq, nk) in enumerate(zip(*full(ci))):
        qb, kb, vb, gb = dev(q[b:b + 1, :, :nq].contiguous(), k[b:b + 1, :, :nk].contiguous(), v[b:b + 1, :, :nk].contiguous(),
                             go[b:b + 1, :, :nq].contiguous())
        o, lse = attention.mha_attention_lse(qb, kb, vb, H)
        assert torch.equal(o, attention.mha_attention(qb, kb, vb, H))
        out.append(tuple(t.cpu() for t in (o, lse) + tuple(attention.mha_attention_bwd(qb, kb, vb, o, lse, gb, H))))
    return out


def bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def assert_is_per_example(ci, got, what=""):
    """inside the lengths: the per-example call's bits; past them: exact zeros"""
    ql, kl = full(ci)
    for b, (nq, nk, want) in enumerate(zip(ql, kl, per_example(ci))):
        for name, g, w in zip(NAMES, got, want):
            n = nk if name in ("gk", "gv") else nq
            assert bits(g[b:b + 1, :, :n].cpu(), w), "%s example %d %s" % (what, b, name)
            tail = g[b, :, n:].cpu()
            assert torch.equal(tail, torch.zeros_like(tail)), "%s example %d %s past its length" % (what, b, name)


# ---- 1. bit identity per example --------------------------------------------------------------------------------------
@ALL
def test_every_example_has_the_bits_of_its_own_uniform_call(ci):
    assert_is_per_example(ci, ragged_run(ci))


# ---- 2. never read, always written ------------------------------------------------------------------------------------
@ALL
def test_padding_is_never_read_and_outputs_are_always_written(ci):
    ql, kl = full(ci)
    q, k, v, go = (t.clone() for t in draw(ci))
    for b, (nq, nk) in enumerate(zip(ql, kl)):
        q[b, :, nq:] = float("nan")
        go[b, :, nq:] = float("nan")
        k[b, :, nk:] = float("nan")
        v[b, :, nk:] = float("nan")
    got = ragged_call(ci, *dev(q, k, v, go), poison=True)
    for name, g, w in zip(NAMES, got, ragged_run(ci)):
        assert bits(g.cpu(), w), name
    assert_is_per_example(ci, got, "NaN padding")


@ALL
def test_an_example_does_not_depend_on_the_others(ci):
    Bt = CASES[ci][0][0]
    ql, kl = full(ci)
    base, other = draw(ci), draw(ci, seed=1)
    for keep in sorted({0, Bt // 2, Bt - 1}):
        mixed = [o.clone() for o in other]
        for m, t in zip(mixed, base):
            m[keep] = t[keep]
        got = ragged_call(ci, *dev(*mixed))
        for name, g, w in zip(NAMES, got, ragged_run(ci)):
            assert bits(g[keep].cpu(), w[keep]), "example %d %s" % (keep, name)


# ---- 3. full lengths --------------------------------------------------------------------------------------------------
@ALL
def test_full_lengths_give_the_uniform_call_on_the_whole_batch(ci):
    from sudo_rm_rf_amd import attention
    (Bt, H, d, Lq, Lk), _, _ = CASES[ci]
    q, k, v, go = dev(*draw(ci))
    o, lse = attention.mha_attention_lse(q, k, v, H)
    want = (o, lse) + tuple(attention.mha_attention_bwd(q, k, v, o, lse, go, H))
    for kw in (dict(q_lengths=[Lq] * Bt, k_lengths=[Lk] * Bt), dict(q_lengths=torch.tensor([Lq] * Bt)), dict(k_lengths=[Lk] * Bt)):
        o2, lse2 = attention.mha_attention_lse(q, k, v, H, **kw)
        got = (o2, lse2) + tuple(attention.mha_attention_bwd(q, k, v, o2, lse2, go, H, **kw))
        assert bits(attention.mha_attention(q, k, v, H, **kw), o)
        for name, g, w in zip(NAMES, got, want):
            assert bits(g, w), (name, sorted(kw))


# ---- 4. fp64, directly ------------------------------------------------------------------------------------------------
def _ref(q, k, v, go, H, dtype):
    q, k, v = (t.detach().to(dtype, copy=True).requires_grad_() for t in (q, k, v))
    o = ar.attention(q, k, v, H)
    return (o.detach(),) + torch.autograd.grad(o, (q, k, v), go.to(dtype))


@pytest.mark.parametrize("ci", [D256, GENERIC], ids=_id)
def test_each_example_matches_fp64_attention_on_its_slices(ci):
    (Bt, H, d, Lq, Lk), _, _ = CASES[ci]
    q, k, v, go = draw(ci)
    o, _, gq, gk, gv = ragged_run(ci)
    bad = []
    for b, (nq, nk) in enumerate(zip(*full(ci))):
        sl = (q[b:b + 1, :, :nq], k[b:b + 1, :, :nk], v[b:b + 1, :, :nk], go[b:b + 1, :, :nq])
        ref, f32 = _ref(*sl, H, torch.float64), _ref(*sl, H, torch.float32)
        floor = 8 * 2.0 ** -24 * math.sqrt(d) * sl[3].abs().max().item() * sl[2].abs().max().item() / math.sqrt(d)
        floors = {"gq": floor * sl[1].abs().max().item(), "gk": floor * sl[0].abs().max().item()} if nk == 1 else {}
        got = (o[b:b + 1, :, :nq], gq[b:b + 1, :, :nq], gk[b:b + 1, :, :nk], gv[b:b + 1, :, :nk])
        for name, g, r, f in zip(("o", "gq", "gk", "gv"), got, ref, f32):
            err = (g.double() - r).abs().max().item()
            bar = max(8 * (f.double() - r).abs().max().item(), floors.get(name, 0.0))
            print("%s example %d %s: kernel err %.3e, bar %.3e, max|ref| %.3e" % (_id(ci), b, name, err, bar, r.abs().max().item()))
            if not err <= bar:
                bad.append((b, name, err, bar))
    assert not bad, bad


# ---- 5. dispatch ------------------------------------------------------------------------------------------------------
def _names(d, mfma, suffix):
    fwd = ["mha_attention_mfma" if mfma else "mha_attention_generic", "mha_attention_lse_mfma" if mfma else "mha_attention_lse_generic"]
    if not mfma:
        bwd = ["mha_attention_bwd_delta", "mha_attention_bwd_dq_generic", "mha_attention_bwd_dkv_generic"]
    elif d <= 128:
        bwd = ["mha_attention_bwd_delta", "mha_attention_bwd_dq_mfma", "mha_attention_bwd_dkv_mfma"]
    else:
        bwd = ["mha_attention_bwd_delta", "mha_attention_bwd_dq_mfma", "mha_attention_bwd_dv_mfma", "mha_attention_bwd_dk_mfma"]
    return [n + suffix for n in fwd + bwd]


def _traced(ci, ragged):
    from sudo_rm_rf_amd import attention, ops
    (Bt, H, d, Lq, Lk), ql, kl = CASES[ci]
    kw = dict(q_lengths=ql, k_lengths=kl) if ragged else {}
    q, k, v, go = dev(*draw(ci))
    with ops.kernel_trace(DEV) as tr:
        attention.mha_attention(q, k, v, H, **kw)
        o, lse = attention.mha_attention_lse(q, k, v, H, **kw)
        g = attention.mha_attention_bwd(q, k, v, o, lse, go, H, **kw)
    torch.cuda.synchronize()
    return [n for n, _ in tr.launches], (o, lse) + tuple(g)


@ALL
def test_dispatch_by_profiler_name(ci):
    from sudo_rm_rf_amd import attention
    d = CASES[ci][0][2]
    mfma = attention.mha_attention_mfma_supported(d)
    assert mfma == (d % 16 == 0 and 16 <= d <= 256)
    assert _traced(ci, True)[0] == _names(d, mfma, "_ragged")
    assert _traced(ci, False)[0] == _names(d, mfma, "")


def test_kernel_mode_1_sends_mfma_shapes_through_the_generic_ragged_forms():
    from sudo_rm_rf_amd import ops
    ops.set_kernel_mode(1)
    per_example.cache_clear()          # (the per-example calls of THIS mode: the generic kernels' bits, not the cached MFMA ones)
    try:
        names, got = _traced(0, True)
        assert names == _names(16, False, "_ragged")
        assert_is_per_example(0, got, "mode 1")
    finally:
        per_example.cache_clear()
        ops.set_kernel_mode(0)


# ---- 6. determinism ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", [D256, MFMA64, GENERIC], ids=_id)
def test_two_runs_give_equal_bits(ci):
    a = ragged_call(ci, *dev(*draw(ci)))
    b = ragged_call(ci, *dev(*draw(ci)))
    for name, x, y in zip(NAMES, a, b):
        assert bits(x, y), name


# ---- 7. placement -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def arena():
    return pl.Arena(DEV, 16 << 20)


@pytest.mark.parametrize("ci", [MFMA64, GENERIC], ids=_id)
@pytest.mark.parametrize("shifts", [(1, 2, 3, 1, 2, 3, 1, 2, 3, 1), (3, 1, 2, 3, 1, 2, 3, 3, 2, 1)], ids=lambda s: "shift" + "".join(map(str, s)))
def test_off_the_16_byte_grid_with_guard_bands(arena, ci, shifts):
    from sudo_rm_rf_amd import attention
    (Bt, H, d, Lq, Lk), ql, kl = CASES[ci]
    kw = dict(q_lengths=ql, k_lengths=kl)
    q, k, v, go = draw(ci)
    want = ragged_run(ci)
    arena.reset()
    dq, dk, dv, dgo = (arena.put(t, shift_floats=s, name=n) for t, s, n in zip((q, k, v, go), shifts, ("q", "k", "v", "go")))
    o_plain = arena.place(q.shape, shift_floats=shifts[4], name="o_plain")
    o = arena.place(q.shape, shift_floats=shifts[4], name="o")
    lse = arena.place((Bt, H, Lq), shift_floats=shifts[5], name="lse")
    outs = [arena.place(t.shape, shift_floats=s, name=n) for t, s, n in zip((q, k, v), shifts[6:9], NAMES[2:])]
    ws = arena.place((attention.mha_attention_bwd_workspace_bytes(Bt, H, d, Lq, Lk) // 4,), shift_floats=shifts[9], name="workspace")
    attention.mha_attention(dq, dk, dv, H, out=o_plain, **kw)
    attention.mha_attention_lse(dq, dk, dv, H, out=o, lse=lse, **kw)
    attention.mha_attention_bwd(dq, dk, dv, o, lse, dgo, H, gq=outs[0], gk=outs[1], gv=outs[2], workspace=ws, **kw)
    torch.cuda.synchronize()
    arena.check()
    for t, h in zip((dq, dk, dv, dgo), (q, k, v, go)):
        assert torch.equal(t.cpu(), h)
    assert bits(o_plain.cpu(), want[0])
    for name, g, w in zip(NAMES, [o, lse] + outs, want):
        arena.assert_written(g)
        arena.assert_clean(g)
        assert bits(g.cpu(), w), name


# ---- 8. refusals ------------------------------------------------------------------------------------------------------
def test_bad_lengths_are_refused_before_any_launch():
    from sudo_rm_rf_amd import attention, ops
    from sudo_rm_rf_amd._lib import SrfError
    Bt, H, d, L = 3, 2, 16, 9

    def attempt(match, Bt=Bt, **kw):
        q = torch.zeros(Bt, H * d, L, device=DEV)
        lse_in = torch.zeros(Bt, H, L, device=DEV)
        pat = lambda shape: torch.full(shape, 1234.5, device=DEV)
        o, lse, gq, gk, gv = pat(q.shape), pat((Bt, H, L)), pat(q.shape), pat(q.shape), pat(q.shape)
        ws = torch.full((attention.mha_attention_bwd_workspace_bytes(Bt, H, d, L, L),), 77, dtype=torch.uint8, device=DEV)
        with ops.kernel_trace(DEV) as tr:
            with pytest.raises(SrfError, match=match):
                attention.mha_attention(q, q, q, H, out=o, **kw)
            with pytest.raises(SrfError, match=match):
                attention.mha_attention_lse(q, q, q, H, out=o, lse=lse, **kw)
            with pytest.raises(SrfError, match=match):
                attention.mha_attention_bwd(q, q, q, q, lse_in, q, H, gq=gq, gk=gk, gv=gv, workspace=ws, **kw)
            qg = q.clone().requires_grad_()
            with pytest.raises(SrfError, match=match):
                attention.mha_attention(qg, q, q, H, **kw)
        torch.cuda.synchronize()
        assert tr.launches == []
        for t in (o, lse, gq, gk, gv):
            assert (t == 1234.5).all()
        assert (ws == 77).all()

    attempt(r"example 1 has q_lengths\[b\] = 0", q_lengths=[9, 0, 3])
    attempt(r"example 2 has k_lengths\[b\] = 0", k_lengths=[9, 1, 0])
    attempt(r"example 0 has q_lengths\[b\] = 10 \(allowed: 1\.\.Lq = 9\)", q_lengths=[10, 1, 3], k_lengths=[1, 1, 1])
    attempt(r"example 1 has k_lengths\[b\] = 10", q_lengths=[9, 1, 3], k_lengths=[1, 10, 1])
    attempt(r"2 q_lengths for a batch of 3", q_lengths=[9, 1])
    attempt(r"4 k_lengths for a batch of 3", k_lengths=[9, 1, 1, 1])
    attempt(r"k_lengths must be a list or a CPU tensor", k_lengths=torch.tensor([9, 1, 1], device=DEV))
    attempt(r"q_lengths must be a list or a CPU tensor", q_lengths=torch.tensor([9, 1, 1], device=DEV))
    attempt(r"1\.\.128 examples \(got Bt = 129\)", Bt=129, q_lengths=[1] * 129)


# ---- 9. autograd ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", [0, MFMA64, GENERIC, 5], ids=_id)
def test_autograd_through_mha_attention_is_the_raw_ragged_backward(ci):
    from sudo_rm_rf_amd import attention, ops
    (Bt, H, d, Lq, Lk), ql, kl = CASES[ci]
    q, k, v, go = dev(*draw(ci))
    want = ragged_run(ci)
    qg, kg, vg = (t.clone().requires_grad_() for t in (q, k, v))
    with ops.kernel_trace(DEV) as tr:
        o = attention.mha_attention(qg, kg, vg, H, q_lengths=ql, k_lengths=None if kl is None else torch.tensor(kl))
        got = torch.autograd.grad(o, (qg, kg, vg), go)
    torch.cuda.synchronize()
    mfma = attention.mha_attention_mfma_supported(d)
    assert [n for n, _ in tr.launches] == _names(d, mfma, "_ragged")[1:]
    assert o.grad_fn is not None and bits(o.detach().cpu(), want[0])
    for name, g, w in zip(NAMES[2:], got, want[2:]):
        assert bits(g.cpu(), w), name


# ---- 10. MHAttentionLayer ---------------------------------------------------------------------------------------------
SMALL_TOL = 2e-4          # tests/test_gpu_attention_bwd.py: test_mha_layer_trains_on_hip_after_the_opt_in


def layer_ref(Q, K, V, par, H):
    """the layer restated in fp64: four nn.Linear around ar.attention; -> (output, k)"""
    wq, bq, wk, bk, wv, bv, wo, bo = par
    lin = lambda x, w, b: F.linear(x, w, b).transpose(1, 2)
    k = lin(K, wk, bk)
    o = ar.attention(lin(Q, wq, bq), k, lin(V, wv, bv), H)
    return F.linear(o.transpose(1, 2), wo, bo), k


@pytest.mark.parametrize("emb,d_model,H,B,Lq,Lk,ql,kl", [(24, 16, 3, 3, 26, 26, [26, 9, 17], [26, 9, 17]),
                                                        (128, 64, 1, 2, 70, 45, [70, 30], [45, 11])], ids=["self", "cross"])
def test_mha_layer_takes_a_ragged_batch_in_inference_and_training(emb, d_model, H, B, Lq, Lk, ql, kl):
    from sudo_rm_rf_amd.dnn.models.attentive_sudormrf_v2 import MHAttentionLayer
    from sudo_rm_rf_amd.dnn.models import attentive_sudormrf_v3 as v3
    assert v3.MHAttentionLayer is MHAttentionLayer
    self_att = Lq == Lk
    torch.manual_seed(emb + Lq)
    layer = MHAttentionLayer(emb, d_model, H).to(DEV).eval()
    par = [p for m in (layer.Q_proj, layer.K_proj, layer.V_proj, layer.O_proj) for p in (m.weight, m.bias)]
    g = torch.Generator().manual_seed(7 * emb + Lk)
    xq = torch.randn(B, Lq, emb, generator=g, dtype=torch.float64).float()          # (finite random values in the padding too)
    xkv = xq if self_att else torch.randn(B, Lk, emb, generator=g, dtype=torch.float64).float()
    gy = torch.randn(B, Lq, emb, generator=g, dtype=torch.float64).float()

    # the fp64 restatement, example by example on slices; parameter gradients summed over the examples
    rpar = [p.detach().double().cpu().requires_grad_() for p in par]
    want_y = torch.zeros(B, Lq, emb, dtype=torch.float64)
    want_x = [torch.zeros(B, Lq, emb, dtype=torch.float64), torch.zeros(B, Lk, emb, dtype=torch.float64)]
    want_p = [torch.zeros_like(p) for p in rpar]
    cancel = torch.zeros(H * d_model, dtype=torch.float64)
    for b in range(B):
        rq = xq[b:b + 1, :ql[b]].double().requires_grad_()
        rkv = rq if self_att else xkv[b:b + 1, :kl[b]].double().requires_grad_()
        yr, rk = layer_ref(rq, rkv, rkv, rpar, H)
        gr = torch.autograd.grad(yr, ([rq] if self_att else [rq, rkv]) + rpar + [rk], gy[b:b + 1, :ql[b]].double())
        want_y[b, :ql[b]] = yr.detach()[0]
        want_x[0][b, :ql[b]] = gr[0][0]
        if not self_att:
            want_x[1][b, :kl[b]] = gr[1][0]
        for acc, t in zip(want_p, gr[(1 if self_att else 2):-1]):
            acc += t
        cancel += gr[-1].abs().sum(dim=(0, 2))
    want = ([want_x[0]] if self_att else want_x) + want_p
    names = (["x"] if self_att else ["Q", "KV"]) + ["%s_proj.%s" % (m, w) for m in "QKVO" for w in ("weight", "bias")]
    ybar = SMALL_TOL * want_y.abs().max().item()

    def run(xq, xkv):
        dq = xq.to(DEV).requires_grad_()
        dkv = dq if self_att else xkv.to(DEV).requires_grad_()
        layer.enable_hip_training(False)
        y0 = layer(dq, dkv, dkv, q_lengths=ql, k_lengths=kl)
        assert y0.grad_fn is None
        layer.enable_hip_training()
        y = layer(dq, dkv, dkv, q_lengths=torch.tensor(ql), k_lengths=kl)
        assert y.grad_fn is not None and torch.equal(y.detach(), y0)
        got = torch.autograd.grad(y, ([dq] if self_att else [dq, dkv]) + par, gy.to(DEV))
        torch.cuda.synchronize()
        layer.enable_hip_training(False)
        return y0.cpu(), [t.cpu() for t in got]

    def check(y, got, what):
        bad = []
        err = (y.double() - want_y).abs().max().item()
        print("%s y: err %.3e, bar %.3e" % (what, err, ybar))
        if not err <= ybar:
            bad.append(("y", err, ybar))
        for b in range(B):
            assert torch.equal(y[b, ql[b]:], torch.zeros_like(y[b, ql[b]:])), "output rows past q_lengths[%d]" % b
            assert torch.equal(got[0][b, ql[b]:], torch.zeros_like(got[0][b, ql[b]:])), "input gradient past q_lengths[%d]" % b
            if not self_att:
                assert torch.equal(got[1][b, kl[b]:], torch.zeros_like(got[1][b, kl[b]:])), "input gradient past k_lengths[%d]" % b
        for name, a, r in zip(names, got, want):
            assert a.shape == r.shape and torch.isfinite(a).all(), name
            e, top = (a.double() - r).abs().max().item(), r.abs().max().item()
            if name == "K_proj.bias":          # exactly zero by the softmax's shift invariance: the size of what cancels
                assert top <= 1e-12
                top = cancel.max().item()
            print("%s %s: err %.3e, max|ref| %.3e, relative %.3e" % (what, name, e, top, e / top))
            if not e <= SMALL_TOL * top:
                bad.append((name, e / top))
        assert not bad, bad

    y1, got1 = run(xq, xkv)
    check(y1, got1, "padding A")
    # other finite values in the padding: the same reference, the same bar; and the two runs agree within it
    xq2, xkv2 = xq.clone(), xkv.clone()
    for b in range(B):
        xq2[b, ql[b]:] = 3.0 * torch.randn(Lq - ql[b], emb, generator=g)
        if not self_att:
            xkv2[b, kl[b]:] = 3.0 * torch.randn(Lk - kl[b], emb, generator=g)
    if self_att:
        xkv2 = xq2
    y2, got2 = run(xq2, xkv2)
    check(y2, got2, "padding B")
    assert (y1 - y2).abs().max().item() <= ybar
    for name, a, b_, r in zip(names, got1, got2, want):
        top = cancel.max().item() if name == "K_proj.bias" else r.abs().max().item()
        assert (a - b_).abs().max().item() <= SMALL_TOL * top, name
    # without lengths nothing changes
    dq = xq.to(DEV)
    dkv = dq if self_att else xkv.to(DEV)
    assert torch.equal(layer(dq, dkv, dkv), layer(dq, dkv, dkv, None, None))
