"""What srf_mha_attention_bwd implements, pinned on the CPU: the six closed-form gradient formulas of softmax attention
(the header comment of csrc/srf_attention_bwd.hip) against fp64 autograd through
tests.attentive_ref.attention, and the new symbols' declarations against their ctypes bindings."""
import math
import os
import re

import pytest
import torch

from tests import attentive_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("srf_mha_attention_lse", "srf_mha_attention_bwd", "srf_mha_attention_bwd_workspace_bytes",
               "srf_mha_attention_bwd_mfma_supported")


def closed_form(q, k, v, go, H, scale):
    """(gq, gk, gv, lse) from the formulas the kernels implement, per (example, head); q is scaled before the product"""
    B, HD, Lq = q.shape
    d = HD // H
    qh, gh = q.reshape(B, H, d, Lq), go.reshape(B, H, d, Lq)
    kh, vh = k.reshape(B, H, d, -1), v.reshape(B, H, d, -1)
    S = torch.einsum("bhjl,bhjs->bhls", qh * scale, kh)
    lse = torch.logsumexp(S, dim=-1)
    P = torch.exp(S - lse[..., None])
    O = torch.einsum("bhls,bhjs->bhjl", P, vh)
    delta = (gh * O).sum(2)                                   # [B, H, Lq]
    gv = torch.einsum("bhls,bhjl->bhjs", P, gh)
    dP = torch.einsum("bhjl,bhjs->bhls", gh, vh)
    dS = P * (dP - delta[..., None])
    gq = scale * torch.einsum("bhls,bhjs->bhjl", dS, kh)
    gk = scale * torch.einsum("bhls,bhjl->bhjs", dS, qh)
    return gq.reshape(q.shape), gk.reshape(k.shape), gv.reshape(v.shape), lse


@pytest.mark.parametrize("shape", [(2, 3, 16, 26, 26), (2, 1, 64, 70, 45)])
def test_closed_form_gradients_agree_with_fp64_autograd(shape):
    Bt, H, d, Lq, Lk = shape
    g = torch.Generator().manual_seed(1000 * d + Lq + 7 * Lk)
    q = torch.randn(Bt, H * d, Lq, generator=g, dtype=torch.float64).requires_grad_()
    k = torch.randn(Bt, H * d, Lk, generator=g, dtype=torch.float64).requires_grad_()
    v = torch.randn(Bt, H * d, Lk, generator=g, dtype=torch.float64).requires_grad_()
    go = torch.randn(Bt, H * d, Lq, generator=g, dtype=torch.float64)
    want = torch.autograd.grad(ar.attention(q, k, v, H), (q, k, v), go)
    got = closed_form(q.detach(), k.detach(), v.detach(), go, H, 1.0 / math.sqrt(d))
    for name, a, b in zip(("gq", "gk", "gv"), got, want):
        err = (a - b).abs().max().item()
        print("%s %s: closed form vs fp64 autograd %.3e" % (shape, name, err))
        assert err <= 1e-12


def _header_arity(name):
    text = open(os.path.join(ROOT, "include", "sudormrf_hip.h")).read()
    m = re.search(r"^(?:int|size_t)\s+%s\(([^;]*)\);" % name, text, re.M | re.S)
    assert m, "%s is not declared in include/sudormrf_hip.h" % name
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_header_declares_and_lib_binds_the_new_symbols(name):
    from sudo_rm_rf_amd import _lib
    lib = _lib.load()
    assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    fn = getattr(lib, name)
    assert len(fn.argtypes) == _header_arity(name)
    assert lib.srf_abi_version() == 19 == _lib.ABI_VERSION


def test_workspace_size_and_dispatch_predicate():
    from sudo_rm_rf_amd import _lib, attention
    lib = _lib.load()
    assert attention.mha_attention_bwd_workspace_bytes(2, 3, 16, 26, 31) == 2 * 3 * 26 * 4      # delta: [Bt, H, Lq] floats
    assert [d for d in range(1, 300) if lib.srf_mha_attention_bwd_mfma_supported(d)] == list(range(16, 257, 16))
    for name in ("mha_attention_lse", "mha_attention_bwd"):
        assert callable(getattr(attention, name))
