"""The ragged attention forms without a GPU: the three new symbols' declarations against their ctypes bindings, the refusals
that come before any launch, and -- in fp64 torch -- the definition the GPU tests' per-example comparison relies on: attention
with the keys masked at k_len and the queries cut at q_len IS tests.attentive_ref.attention on the example's slices."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from tests import attentive_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("srf_mha_attention_ragged", "srf_mha_attention_lse_ragged", "srf_mha_attention_bwd_ragged")


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
    assert len(getattr(lib, name).argtypes) == _header_arity(name)
    uniform = name[:-len("_ragged")]
    assert _header_arity(name) == _header_arity(uniform) + 2          # + q_lengths, k_lengths
    assert lib.srf_abi_version() == 19 == _lib.ABI_VERSION
    assert _lib.RAGGED_MAX_BATCH == 128


def test_python_ops_take_the_lengths_keywords():
    import inspect
    from sudo_rm_rf_amd import attention
    from sudo_rm_rf_amd.dnn.models.attentive_sudormrf_v2 import MHAttentionLayer
    for fn in (attention.mha_attention, attention.mha_attention_lse, attention.mha_attention_bwd, attention.mha_layer_train,
               MHAttentionLayer.forward):
        par = inspect.signature(fn).parameters
        assert par["q_lengths"].default is None and par["k_lengths"].default is None, fn


def test_bad_lengths_are_refused_by_the_c_entry_points_before_any_launch():
    """(never-dereferenced dummy pointers: every call below returns SRF_EINVAL from its argument checks)"""
    from sudo_rm_rf_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(0x1000)
    Bt, H, d, Lq, Lk = 3, 2, 16, 9, 7
    tab = lambda *v: (C.c_int * len(v))(*v)
    sc = C.c_float(0.25)

    def calls(ql, kl, Bt=Bt):
        yield "srf_mha_attention_ragged", lib.srf_mha_attention_ragged(p, p, p, p, Bt, H, d, Lq, Lk, ql, kl, sc, None)
        yield "srf_mha_attention_lse_ragged", lib.srf_mha_attention_lse_ragged(p, p, p, p, p, Bt, H, d, Lq, Lk, ql, kl, sc, None)
        yield "srf_mha_attention_bwd_ragged", lib.srf_mha_attention_bwd_ragged(p, p, p, p, p, p, p, p, p, p, Bt, H, d, Lq, Lk, ql, kl,
                                                                               sc, None)

    def refused(ql, kl, pattern, Bt=Bt):
        gen = calls(ql, kl, Bt)
        for name, rc in gen:
            msg = lib.srf_last_error().decode()
            assert rc == -1, (name, rc)          # SRF_EINVAL
            assert msg.startswith(name + ":") and re.search(pattern, msg), msg

    refused(tab(9, 0, 3), None, r"example 1 has q_lengths\[b\] = 0 \(allowed: 1\.\.Lq = 9\)")
    refused(tab(9, 10, 3), tab(1, 1, 1), r"example 1 has q_lengths\[b\] = 10")
    refused(None, tab(7, 7, 8), r"example 2 has k_lengths\[b\] = 8 \(allowed: 1\.\.Lk = 7\)")
    refused(tab(1, 1, 1), tab(1, -4, 1), r"example 1 has k_lengths\[b\] = -4")
    refused(tab(*([1] * 129)), None, r"1\.\.128 examples \(got Bt = 129\)", Bt=129)


def masked_attention(q, k, v, heads, q_lengths, k_lengths):
    """attention over a padded batch: keys >= k_len get the score -inf, queries >= q_len the output 0"""
    B, HD, Lq = q.shape
    Lk, d = k.shape[-1], HD // heads
    qh = (q / math.sqrt(d)).reshape(B, heads, d, Lq)
    kh, vh = k.reshape(B, heads, d, Lk), v.reshape(B, heads, d, Lk)
    s = torch.einsum("bhdl,bhds->bhls", qh, kh)
    kmask = torch.arange(Lk)[None, :] >= torch.tensor(k_lengths)[:, None]          # [B, Lk]
    s = s.masked_fill(kmask[:, None, None, :], float("-inf"))
    o = torch.einsum("bhls,bhds->bhdl", torch.softmax(s, dim=-1), vh).reshape(B, HD, Lq)
    qmask = torch.arange(Lq)[None, :] >= torch.tensor(q_lengths)[:, None]
    return o.masked_fill(qmask[:, None, :], 0.0)


@pytest.mark.parametrize("shape,ql,kl", [((4, 3, 16, 40, 40), [40, 33, 32, 1], [40, 33, 32, 1]),
                                         ((3, 1, 64, 70, 45), [70, 31, 1], [45, 1, 33]),
                                         ((2, 3, 24, 25, 25), [25, 7], [25, 7])])
def test_masked_attention_is_attention_on_the_slices(shape, ql, kl):
    Bt, H, d, Lq, Lk = shape
    g = torch.Generator().manual_seed(1000 * d + Lq + 7 * Lk)
    q = torch.randn(Bt, H * d, Lq, generator=g, dtype=torch.float64).requires_grad_()
    k = torch.randn(Bt, H * d, Lk, generator=g, dtype=torch.float64).requires_grad_()
    v = torch.randn(Bt, H * d, Lk, generator=g, dtype=torch.float64).requires_grad_()
    go = torch.randn(Bt, H * d, Lq, generator=g, dtype=torch.float64)
    o = masked_attention(q, k, v, H, ql, kl)
    grads = torch.autograd.grad(o, (q, k, v), go)
    for b in range(Bt):
        qs, ks, vs = (t[b:b + 1, :, :n].detach().clone().requires_grad_() for t, n in ((q, ql[b]), (k, kl[b]), (v, kl[b])))
        want = ar.attention(qs, ks, vs, H)
        wg = torch.autograd.grad(want, (qs, ks, vs), go[b:b + 1, :, :ql[b]])
        assert (o[b:b + 1, :, :ql[b]] - want).abs().max().item() <= 1e-12
        assert o[b, :, ql[b]:].abs().sum().item() == 0.0
        for name, a, w, n in zip(("gq", "gk", "gv"), grads, wg, (ql[b], kl[b], kl[b])):
            err = (a[b:b + 1, :, :n] - w).abs().max().item()
            assert err <= 1e-12, (b, name, err)
            assert a[b, :, n:].abs().sum().item() == 0.0, (b, name)          # and nothing flows into the padding
