"""Dropout in srf_posenc_apply and the opt-in HIP training of TransformerLayer / AttentiveUConvBlock.

Kernels: srf_dropout_mask against the numpy Philox restatement (tests/attentive_train_ref.py) EXACTLY; srf_posenc_apply_dropout
and srf_posenc_dropout_bwd: dropped elements exactly 0.0, kept elements bit-equal to plain * inv_keep with
inv_keep = np.float32(1) / (np.float32(1) - np.float32(p)) -- the fp32 scale the library forms on the host and MULTIPLIES by --
and `plain` the existing kernel's output; p = 0 bit-equal to plain.
Modules: every reference-generated fixture (tests/golden/attn_train_*.npz, tools/make_golden_attentive_train.py: the
reference's own TransformerLayer / AttentiveUConvBlock in fp64 under the same mask).  The output within 1e-4 (the project's
forward bar); each gradient tensor's max-abs error at most 2e-4 of that tensor's largest reference entry (the bar of
tests/test_gpu_attention_bwd.py's layer test and of the tiny training fixtures), K_proj.bias -- an exact zero -- against the
sum of the reference terms that cancel there, as that test measures it (the fixture stores it: k_bias_cancel).  The fixture's
(seed, offset) pair reaches the module through attention.draw_dropout_state, the one place the modules draw from.
"""
import functools

import numpy as np
import pytest
import torch

from tests import attentive_train_ref as tr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD_TOL = 1e-4
GRAD_TOL = 2e-4
BIG = (1 << 32) + 0x9E3779B9          # offsets above 2^32: both counter words in use


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


# ---- 1. the kernels ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1249, 70001])
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5, 1.0])
def test_dropout_mask_is_the_numpy_restatement(n, p):
    from sudo_rm_rf_amd import attention
    for seed, offset in ((0x0123_4567_89AB_CDEF, BIG), (2 ** 64 - 1, (3 << 40) + 1)):
        got = attention.dropout_mask(n, p, seed, offset, DEV).cpu().numpy()
        want = tr.dropout_mask(n, p, seed, offset)
        assert got.dtype == np.uint8 and set(np.unique(got)) <= {0, 1}
        assert np.array_equal(got.astype(bool), want), (n, p, int((got.astype(bool) != want).sum()))


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


@functools.lru_cache(maxsize=None)
def _posenc_case(Bt, C, L, lazy):
    """(a, pe, norm or (), plain): drawn once, shared, never written to"""
    from sudo_rm_rf_amd import attention, ops
    g = torch.Generator().manual_seed(100 * C + L + lazy)
    a = (torch.randn(Bt, C, L, generator=g) * 1.5 + 0.3).to(DEV)
    pe = torch.randn(1, L + 3, C, generator=g).to(DEV)
    norm = ()
    if lazy:
        norm = (ops.gln_stats(a, Bt), (torch.randn(C, generator=g) * 0.2 + 1).to(DEV), (torch.randn(C, generator=g) * 0.2).to(DEV))
    return a, pe, norm, attention.posenc_apply(a, pe, *norm)


@pytest.mark.parametrize("lazy", [False, True], ids=["plain", "lazy_norm"])
@pytest.mark.parametrize("Bt,C,L", [(2, 24, 26), (1, 33, 65), (3, 64, 1)])
def test_posenc_apply_dropout(Bt, C, L, lazy):
    from sudo_rm_rf_amd import attention, ops
    a, pe, norm, plain = _posenc_case(Bt, C, L, lazy)
    with ops.kernel_trace(DEV) as t0:
        x0 = attention.posenc_apply(a, pe, *norm, p=0.0, seed=5, offset=BIG)
    assert [n for n, _ in t0.launches] == ["posenc_apply"] and np.array_equal(_bits(x0), _bits(plain))
    for p in (0.1, 0.5, 1.0):
        seed = 1000 + int(10 * p)
        with ops.kernel_trace(DEV) as t1:
            x = attention.posenc_apply(a, pe, *norm, p=p, seed=seed, offset=BIG)
        assert [n for n, _ in t1.launches] == ["posenc_apply_dropout"]
        keep = tr.dropout_mask(Bt * C * L, p, seed, BIG).reshape(Bt, C, L)
        got, base = x.cpu().numpy(), plain.cpu().numpy()
        assert np.array_equal(got[~keep].view(np.uint32), np.zeros(int((~keep).sum()), np.uint32))      # +0.0 exactly
        inv = tr.inv_keep(p)                                  # np.float32(1) / (np.float32(1) - np.float32(p))
        if keep.any():
            want = base[keep] * inv
            assert want.dtype == np.float32 and np.array_equal(got[keep].view(np.uint32), want.view(np.uint32)), (p, Bt, C, L)
        assert np.isfinite(got).all()
    assert np.array_equal(_bits(attention.posenc_apply(a, pe, *norm)), _bits(plain))                    # inputs untouched


@pytest.mark.parametrize("alias", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("Bt,C,L", [(2, 24, 26), (1, 33, 65), (3, 64, 1)])
def test_posenc_dropout_bwd(Bt, C, L, alias):
    from sudo_rm_rf_amd import attention
    g = torch.Generator().manual_seed(C + L)
    gx0 = torch.randn(Bt, C, L, generator=g)
    for p in (0.0, 0.1, 0.5, 1.0):
        seed = 77 + int(10 * p)
        gx = gx0.to(DEV)
        gn = attention.posenc_dropout_bwd(gx, p, seed, BIG, out=gx if alias else None)
        assert (gn.data_ptr() == gx.data_ptr()) == alias
        if not alias:
            assert np.array_equal(_bits(gx), gx0.numpy().view(np.uint32))
        keep = tr.dropout_mask(Bt * C * L, p, seed, BIG).reshape(Bt, C, L)
        got = gn.cpu().numpy()
        assert np.array_equal(got[~keep].view(np.uint32), np.zeros(int((~keep).sum()), np.uint32))
        inv = tr.inv_keep(p)                                  # np.float32(1) / (np.float32(1) - np.float32(p))
        if keep.any():
            assert np.array_equal(got[keep].view(np.uint32), (gx0.numpy()[keep] * inv).view(np.uint32)), p


def test_library_refuses_bad_p_and_null_pointers_before_launching():
    from sudo_rm_rf_amd import _lib, attention, ops
    a, pe, _, _ = _posenc_case(2, 24, 26, False)
    with ops.kernel_trace(DEV) as t:
        for p in (1.5, -0.1, float("nan")):
            for call in (lambda: attention.posenc_apply(a, pe, p=p, seed=1, offset=2),
                         lambda: attention.posenc_dropout_bwd(a.clone(), p, 1, 2),
                         lambda: attention.dropout_mask(16, p, 1, 2, DEV)):
                with pytest.raises(_lib.SrfError, match=r"\bp = "):
                    call()
        lib, st = _lib.load(), _lib.current_stream(torch.device(DEV))
        u = lambda v: __import__("ctypes").c_ulonglong(v)
        f = __import__("ctypes").c_float(0.5)
        assert lib.srf_posenc_apply_dropout(None, None, _lib.ptr(pe), _lib.ptr(a), 2, 24, 26, 29, f, u(1), u(2), st) != 0
        assert b"a is null" in lib.srf_last_error()
        assert lib.srf_posenc_apply_dropout(_lib.ptr(a), None, None, _lib.ptr(a), 2, 24, 26, 29, f, u(1), u(2), st) != 0
        assert b"pe is null" in lib.srf_last_error()
        assert lib.srf_posenc_apply_dropout(_lib.ptr(a), None, _lib.ptr(pe), None, 2, 24, 26, 29, f, u(1), u(2), st) != 0
        assert b"x is null" in lib.srf_last_error()
        assert lib.srf_posenc_apply_dropout(_lib.ptr(a), None, _lib.ptr(pe), _lib.ptr(a), 2, 24, 26, 25, f, u(1), u(2), st) != 0
        assert b"max_len" in lib.srf_last_error()
        assert lib.srf_posenc_dropout_bwd(None, _lib.ptr(a), 2, 24, 26, f, u(1), u(2), st) != 0
        assert b"gx is null" in lib.srf_last_error()
        assert lib.srf_dropout_mask(None, 16, f, u(1), u(2), st) != 0 and b"keep is null" in lib.srf_last_error()
    assert t.launches == []


# ---- 2. the fixtures -----------------------------------------------------------------------------------------------------
MAX_LEN = 5000


def _build(name):
    """(module on the device in train() mode, opted in; fixture arrays; parameter names in fixture keys)"""
    from sudo_rm_rf_amd.dnn.models import attentive_sudormrf_v2 as v2
    c, A = tr.CASES[name], tr.load_case(name)
    P = tr.case_params(A, torch.float32, MAX_LEN)
    if c["module"] == "layer":
        m = v2.TransformerLayer(c["emb"], c["d_model"], c["heads"], dropout=c["p"], max_len=MAX_LEN)
    else:
        m = v2.AttentiveUConvBlock(c["out"], c["emb"], c["depth"], c["heads"], c["d_model"], att_dropout=c["p"])
    sd = {k: v for k, v in P.items() if not k.startswith("in_norm.")}
    assert sorted(sd) == sorted(m.state_dict()) and m.state_dict()[[k for k in sd if k.endswith("pe")][0]].shape[1] == MAX_LEN
    m.load_state_dict(sd)                                  # pe: the stored rows, NaN behind them -- a read past Ld shows
    return m.to(DEV).train(), c, A, P


def _run_fixture(name, monkeypatch):
    from sudo_rm_rf_amd import attention, ops
    m, c, A, P = _build(name)
    assert m.enable_hip_training() is m
    monkeypatch.setattr(attention, "draw_dropout_state", lambda: (int(A["seed"]), int(A["offset"])))
    x = torch.from_numpy(A["x"]).to(DEV).requires_grad_()
    gout = torch.from_numpy(A["gout"]).to(DEV)
    names, wrt, extra = ["x"], [x], ()
    if c.get("lazy"):
        in_g, in_b = (P["in_norm." + k].to(DEV).requires_grad_() for k in ("gamma", "beta"))
        extra = (ops.gln_stats(x.detach(), c["Bt"]), in_g, in_b)
        names, wrt = names + ["in_norm.gamma", "in_norm.beta"], wrt + [in_g, in_b]
    for k, prm in m.named_parameters():
        names.append(k)
        wrt.append(prm)
    with ops.kernel_trace(DEV) as trace:
        out = m(x, *extra)
        got = torch.autograd.grad(out, wrt, gout)
    torch.cuda.synchronize()
    return c, A, out, dict(zip(names, got)), trace


@pytest.mark.parametrize("name", list(tr.CASES))
def test_fixture_output_and_every_gradient(name, monkeypatch):
    c, A, out, G, trace = _run_fixture(name, monkeypatch)
    err = float(np.abs(out.detach().cpu().numpy().astype(np.float64) - A["out"]).max())
    print("%s: output max|hip - reference| = %.3e (bar %.0e, max|ref| %.3f)" % (name, err, FWD_TOL, np.abs(A["out"]).max()))
    assert out.grad_fn is not None and err <= FWD_TOL
    grads = [k[len("grad."):] for k in A if k.startswith("grad.")]
    assert sorted(grads) == sorted(G)
    worst, bad = ("", 0.0), []
    for n in grads:
        want, got = A["grad." + n].astype(np.float64), G[n].cpu().numpy().astype(np.float64)
        assert got.shape == want.shape and np.isfinite(got).all(), n
        e, top = float(np.abs(got - want).max()), float(np.abs(want).max())
        if n.endswith("mha.K_proj.bias"):                  # exactly zero: the size of what cancels (module docstring)
            assert top <= 1e-12
            top = float(A["k_bias_cancel"])
        print("  %-34s err %.3e  max|ref| %.3e  ratio %.3e" % (n, e, top, e / top))
        worst = max(worst, (n, e / top), key=lambda t: t[1])
        if not e <= GRAD_TOL * top:
            bad.append((n, e / top))
    print("%s: worst gradient ratio %.3e (%s), bar %.0e" % (name, worst[1], worst[0], GRAD_TOL))
    assert not bad, bad
    names = [n for n, _ in trace.launches]
    assert ("posenc_apply_dropout" in names) == (c["p"] > 0) and ("posenc_dropout_bwd" in names) == (c["p"] > 0)
    if name == "tl_generic":
        assert "mha_attention_lse_generic" in names and "mha_attention_bwd_dkv_generic" in names
    if name == "tl_mfma":                                  # the kernels of the bench shape, read from the trace
        gemms = sorted({n for n in names if n.startswith("pw_")})
        print("  tl_mfma kernels:", sorted(set(names)))
        assert "mha_attention_lse_mfma" in names and "mha_attention_bwd_dq_mfma" in names and "mha_attention_bwd_dkv_mfma" in names
        assert "pw_conv_generic" not in names and any(n.startswith("pw_conv_bf16x3") for n in names), gemms
        assert any(n.startswith("pw_wgrad") for n in names), gemms
    if c["module"] == "block":
        assert any(n.startswith("merge_") and n != "merge_bwd" for n in names) and "merge_bwd" in names, sorted(set(names))
        assert names.count("dwconv5_bwd") == c["depth"] and "gln_apply" not in names, sorted(set(names))


# ---- 3. bits, seeds, refusals ----------------------------------------------------------------------------------------------
def _fresh(kind, p):
    from sudo_rm_rf_amd.dnn.models import attentive_sudormrf_v2 as v2
    torch.manual_seed(3)
    if kind == "layer":
        m, x = v2.TransformerLayer(24, 16, 3, dropout=p), torch.randn(2, 24, 26)
    else:
        m, x = v2.AttentiveUConvBlock(16, 32, 3, 2, 16, att_dropout=p), torch.randn(2, 16, 52)
    with torch.no_grad():
        for k, prm in m.named_parameters():
            if k.endswith("gamma") or k.endswith("beta"):
                prm.add_(torch.randn_like(prm) * 0.2)
    return m.to(DEV), x.to(DEV)


@pytest.mark.parametrize("kind", ["layer", "block"])
def test_opt_in_keeps_the_inference_bits(kind):
    m, x = _fresh(kind, 0.1)
    m.eval()
    with torch.no_grad():
        base = m(x)
    assert m.enable_hip_training() is m and "_srf_hip_training" not in m.state_dict()
    sub = m.attention if kind == "block" else m
    assert all(s.__dict__.get("_srf_hip_training") for s in (sub, sub.pos_enc, sub.mha))
    with torch.no_grad():
        assert torch.equal(m(x), base)
    xg = x.clone().requires_grad_()
    y = m(xg)                                              # eval(): autograd, no dropout -- the plain kernels
    assert y.grad_fn is not None
    if kind == "layer":
        assert torch.equal(y.detach(), base)
    else:
        # the block merges through srf_merge under autograd (out_norm as level D - 1's lazy norm), the stand-alone inference
        # forward through gln_apply + repeat_interleave + add: the same sum in another association.  Outputs here are below 8,
        # an fp32 ulp there is 4.8e-7; three added levels through a unit-gain norm and a 32-term res_conv sum stay within 20 ulp
        assert (y.detach() - base).abs().max().item() <= 1e-5
    import pickle
    assert "_srf_hip_training" not in pickle.loads(pickle.dumps(m)).__dict__
    m.enable_hip_training(False)
    assert m(xg).grad_fn is None and not sub.pos_enc.__dict__.get("_srf_hip_training")


def test_train_mode_p0_under_autograd_has_the_inference_bits():
    m, x = _fresh("layer", 0.0)
    with torch.no_grad():
        base = m.eval()(x)
    y = m.enable_hip_training().train()(x.clone().requires_grad_())
    assert y.grad_fn is not None and torch.equal(y.detach(), base)


@pytest.mark.parametrize("kind", ["layer", "block", "posenc"])
def test_manual_seed_fixes_the_mask(kind):
    if kind == "posenc":
        from sudo_rm_rf_amd.dnn.models import attentive_sudormrf_v2 as v2
        m, x = v2.PositionalEncoding(24, dropout=0.5, max_len=64).to(DEV), torch.randn(2, 26, 24, device=DEV)
    else:
        m, x = _fresh(kind, 0.5)
    m.enable_hip_training().train()
    x = x.requires_grad_(kind != "posenc")
    torch.manual_seed(7)
    y1 = m(x).detach()
    torch.manual_seed(7)
    y2 = m(x).detach()
    torch.manual_seed(8)
    y3 = m(x).detach()
    assert torch.equal(y1, y2) and not torch.equal(y1, y3)
    if kind == "posenc":
        torch.manual_seed(7)
        from sudo_rm_rf_amd import attention
        seed, offset = attention.draw_dropout_state()
        keep = tr.dropout_mask(2 * 24 * 26, 0.5, seed, offset).reshape(2, 24, 26)
        assert np.array_equal(y1.transpose(1, 2).cpu().numpy() != 0, keep)


def test_refusals_stay():
    from sudo_rm_rf_amd.dnn.models import attentive_sudormrf_v2 as v2, attentive_sudormrf_v3 as v3
    for kind in ("layer", "block"):
        m, x = _fresh(kind, 0.1)
        with pytest.raises(RuntimeError, match=r"inference path: in train\(\) mode the reference's dropout \(p = 0.1\) is random"):
            m.train()(x.clone().requires_grad_())
        m.enable_hip_training()
        with pytest.raises(RuntimeError, match="float32 tensors on an MI355X only"):
            m(x.cpu().requires_grad_())
        with pytest.raises(RuntimeError, match="float32 tensors on an MI355X only"):
            m(x.double().requires_grad_())
    pe = v2.PositionalEncoding(24, dropout=0.1, max_len=64).to(DEV).train()
    with pytest.raises(RuntimeError, match="is random"):
        pe(torch.zeros(2, 26, 24, device=DEV))
    for mod in (v2, v3):
        model = mod.SuDORMRF(out_channels=16, in_channels=32, num_blocks=1, upsampling_depth=2, enc_kernel_size=21,
                             enc_num_basis=32, num_sources=2).to(DEV).eval()
        with pytest.raises(RuntimeError, match="inference forward only"):
            model(torch.zeros(1, 1, 800, device=DEV))
