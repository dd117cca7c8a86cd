"""Thin ctypes wrappers of the attention kernels (csrc/srf_attention.hip; include/sudormrf_hip.h, "Attentive SuDoRM-RF v2" / "v3").

Same conventions as ``ops``: CUDA float32 tensors in, new tensors out, torch's current stream.  Kept out of ``ops`` on
purpose: these serve the attentive models' sub-module forwards and the kernel tests only."""
import ctypes as C
import math

import torch

from . import _lib, ops
from .ops import _chk, _norm


def mha_attention_mfma_supported(d):
    """Whether the exact-fp32 MFMA kernel serves head dimension d under the current kernel mode (else: the VALU kernel)."""
    return bool(_lib.load().srf_mha_attention_mfma_supported(int(d)))


def mha_attention_bwd_mfma_supported(d):
    """Whether the exact-fp32 MFMA backward serves head dimension d under the current kernel mode (else: the VALU kernels)."""
    return bool(_lib.load().srf_mha_attention_bwd_mfma_supported(int(d)))


def _mha_shapes(what, q, k, v, heads):
    Bt, HD, Lq = q.shape
    Lk = k.shape[-1]
    if k.shape != (Bt, HD, Lk) or v.shape != (Bt, HD, Lk) or HD % heads:
        raise _lib.SrfError("%s: q %s, k %s, v %s do not fit %d heads" % (what, tuple(q.shape), tuple(k.shape), tuple(v.shape),
                                                                          heads))
    return Bt, HD, HD // heads, Lq, Lk


def _mha_scale(scale, d):
    return C.c_float(1.0 / math.sqrt(d) if scale is None else scale)


def mha_attention(q, k, v, heads, scale=None, out=None):
    """q [Bt, H d, Lq], k / v [Bt, H d, Lk] -> [Bt, H d, Lq]: softmax(scale q^T k) v per (example, head); channel h d + j
    belongs to head h.  scale defaults to 1 / sqrt(d).
    Differentiable: with autograd on and q, k or v requiring grad the result carries a grad_fn whose backward is
    mha_attention_bwd (the forward then is mha_attention_lse, same output bits); otherwise the plain launch, as ever."""
    if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
        if out is not None:
            raise _lib.SrfError("mha_attention: out= cannot be combined with autograd")
        return _MHAttention.apply(q, k, v, heads, scale)
    dev = _chk(q, k, v, out)
    Bt, HD, d, Lq, Lk = _mha_shapes("mha_attention", q, k, v, heads)
    if out is None:
        out = torch.empty((Bt, HD, Lq), dtype=torch.float32, device=dev)
    rc = _lib.load().srf_mha_attention(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(out), Bt, heads, d, Lq, Lk,
                                       _mha_scale(scale, d), _lib.current_stream(dev))
    _lib.check(rc, "srf_mha_attention")
    return out


def mha_attention_lse(q, k, v, heads, scale=None, out=None, lse=None):
    """mha_attention that also returns lse [Bt, H, Lq], the per-query log-sum-exp of the scaled scores: -> (out, lse).  out has
    mha_attention's bits."""
    dev = _chk(q, k, v, out, lse)
    Bt, HD, d, Lq, Lk = _mha_shapes("mha_attention_lse", q, k, v, heads)
    if out is None:
        out = torch.empty((Bt, HD, Lq), dtype=torch.float32, device=dev)
    if lse is None:
        lse = torch.empty((Bt, heads, Lq), dtype=torch.float32, device=dev)
    elif lse.numel() != Bt * heads * Lq:
        raise _lib.SrfError("mha_attention_lse: lse has %d elements, [Bt, H, Lq] = %d" % (lse.numel(), Bt * heads * Lq))
    rc = _lib.load().srf_mha_attention_lse(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(out), _lib.ptr(lse), Bt, heads, d, Lq, Lk,
                                           _mha_scale(scale, d), _lib.current_stream(dev))
    _lib.check(rc, "srf_mha_attention_lse")
    return out, lse


def mha_attention_bwd_workspace_bytes(Bt, heads, d, Lq, Lk):
    return int(_lib.load().srf_mha_attention_bwd_workspace_bytes(Bt, heads, d, Lq, Lk))


def mha_attention_bwd(q, k, v, o, lse, go, heads, scale=None, gq=None, gk=None, gv=None, workspace=None):
    """The gradient of mha_attention: o, lse as mha_attention_lse returned them for (q, k, v, scale), go the gradient of o
    -> (gq, gk, gv), written in full.  workspace: a tensor of at least mha_attention_bwd_workspace_bytes() (default: a new one)."""
    dev = _chk(q, k, v, o, lse, go, gq, gk, gv, workspace)
    Bt, HD, d, Lq, Lk = _mha_shapes("mha_attention_bwd", q, k, v, heads)
    if o.shape != q.shape or go.shape != q.shape:
        raise _lib.SrfError("mha_attention_bwd: o %s / go %s differ from q %s" % (tuple(o.shape), tuple(go.shape), tuple(q.shape)))
    if lse.numel() != Bt * heads * Lq:
        raise _lib.SrfError("mha_attention_bwd: lse has %d elements, [Bt, H, Lq] = %d" % (lse.numel(), Bt * heads * Lq))
    need = mha_attention_bwd_workspace_bytes(Bt, heads, d, Lq, Lk)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    elif workspace.numel() * workspace.element_size() < need:
        raise _lib.SrfError("mha_attention_bwd: workspace of %d bytes, %d needed" % (workspace.numel() * workspace.element_size(),
                                                                                     need))
    gq = torch.empty_like(q) if gq is None else gq
    gk = torch.empty_like(k) if gk is None else gk
    gv = torch.empty_like(v) if gv is None else gv
    if gq.shape != q.shape or gk.shape != k.shape or gv.shape != v.shape:
        raise _lib.SrfError("mha_attention_bwd: gq / gk / gv do not have the shapes of q / k / v")
    rc = _lib.load().srf_mha_attention_bwd(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(o), _lib.ptr(lse), _lib.ptr(go),
                                           _lib.ptr(gq), _lib.ptr(gk), _lib.ptr(gv), _lib.ptr(workspace), Bt, heads, d, Lq, Lk,
                                           _mha_scale(scale, d), _lib.current_stream(dev))
    _lib.check(rc, "srf_mha_attention_bwd")
    return gq, gk, gv


class _MHAttention(torch.autograd.Function):
    """mha_attention under autograd: the forward with lse, the HIP backward.  Saves q, k, v, o, lse -- nothing of size Lq x Lk."""

    @staticmethod
    def forward(ctx, q, k, v, heads, scale):
        q, k, v = q.detach(), k.detach(), v.detach()
        o, lse = mha_attention_lse(q, k, v, heads, scale)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.heads, ctx.scale = heads, scale
        return o

    @staticmethod
    def backward(ctx, go):
        q, k, v, o, lse = ctx.saved_tensors
        g = mha_attention_bwd(q, k, v, o, lse, go.contiguous(), ctx.heads, ctx.scale)
        return tuple(t if need else None for t, need in zip(g, ctx.needs_input_grad[:3])) + (None, None)


class _MHALayer(torch.autograd.Function):
    """MHAttentionLayer.forward under autograd (enable_hip_training): the layer's own kernel sequence with the lse forward, and a
    backward of mha_attention_bwd, ops.pw_conv on the transposed weights (data gradients) and ops.pw_wgrad (weight and bias
    gradients).  Saves the transposed inputs and q, k, v, o, lse -- nothing of size Lq x Lk."""

    @staticmethod
    def forward(ctx, heads, scale, Q, K, V, wq, bq, wk, bk, wv, bv, wo, bo):
        t = lambda x: x.detach().transpose(1, 2).contiguous()
        xq = t(Q)
        xk = xq if K is Q else t(K)
        xv = xk if V is K else (xq if V is Q else t(V))
        q, k, v = ops.pw_conv(xq, wq, bq), ops.pw_conv(xk, wk, bk), ops.pw_conv(xv, wv, bv)
        o, lse = mha_attention_lse(q, k, v, heads, scale)
        ctx.save_for_backward(xq, xk, xv, q, k, v, o, lse, wq, wk, wv, wo)
        ctx.heads, ctx.scale = heads, scale
        return ops.pw_conv(o, wo, bo).transpose(1, 2).contiguous()

    @staticmethod
    def backward(ctx, gy):
        xq, xk, xv, q, k, v, o, lse, wq, wk, wv, wo = ctx.saved_tensors
        need = ctx.needs_input_grad
        g = gy.transpose(1, 2).contiguous()

        def data(gout, w):       # the data gradient of y = W x + b: W^T gout
            wt = w.t().contiguous()
            return ops.pw_conv(gout, wt, torch.zeros(wt.shape[0], dtype=torch.float32, device=gout.device))

        def wgrad(gout, x):      # srf_pw_wgrad reads rows as float4 (L % 4 == 0): zero columns add nothing to either sum
            pad = -gout.shape[-1] % 4
            if pad:
                gout, x = torch.nn.functional.pad(gout, (0, pad)), torch.nn.functional.pad(x, (0, pad))
            return ops.pw_wgrad(gout, x)

        dwo, dbo = wgrad(g, o)
        gq, gk, gv = mha_attention_bwd(q, k, v, o, lse, data(g, wo), ctx.heads, ctx.scale)
        grads = [None, None]
        for i, (gp, w) in enumerate(((gq, wq), (gk, wk), (gv, wv))):
            grads.append(data(gp, w).transpose(1, 2).contiguous() if need[2 + i] else None)
        for gp, x in ((gq, xq), (gk, xk), (gv, xv)):
            grads.extend(wgrad(gp, x))
        return tuple(grads) + (dwo, dbo)


def mha_layer_train(layer, Q, K, V):
    """MHAttentionLayer.forward of an opted-in layer under autograd (the attentive models v2 and v3 share the class):
    Q [batch, Lq, emb_dim], K / V [batch, Lk, emb_dim] -> [batch, Lq, emb_dim], differentiable in the eight projection parameters
    and in Q, K, V."""
    par = [p for m in (layer.Q_proj, layer.K_proj, layer.V_proj, layer.O_proj) for p in (m.weight, m.bias)]
    _chk(*par)
    return _MHALayer.apply(layer.n_heads, layer.q_normalizer, Q, K, V, *par)


def posenc_apply(a, pe, sums=None, gamma=None, beta=None, out=None):
    """x[b, c, l] = GlobLN(a)[b, c, l] + pe[l, c] (no norm when sums is None).  a [Bt, C, L]; pe [max_len, C] or [1, max_len, C]."""
    dev = _chk(a, pe, sums, gamma, beta, out)
    Bt, Cc, L = a.shape
    if pe.shape[-1] != Cc:
        raise _lib.SrfError("posenc_apply: the table has %d channels, the input %d" % (pe.shape[-1], Cc))
    if out is None:
        out = torch.empty_like(a)
    rc = _lib.load().srf_posenc_apply(_lib.ptr(a), _norm(sums, gamma, beta, None), _lib.ptr(pe), _lib.ptr(out), Bt, Cc, L,
                                      pe.shape[-2], _lib.current_stream(dev))
    _lib.check(rc, "srf_posenc_apply")
    return out


def gln_apply2_add(f, f_sums, f_gamma, f_beta, f_prelu, y, y_sums, y_gamma, y_beta, y_prelu=None, out_sums=None, out=None):
    """z = norm_f(f) + norm_y(y), each GlobLN (+ PReLU where a slope is given); out_sums += {sum, sumsq} of z."""
    dev = _chk(f, f_sums, f_gamma, f_beta, f_prelu, y, y_sums, y_gamma, y_beta, y_prelu, out_sums, out)
    groups, channels, length = f.shape
    if out is None:
        out = torch.empty_like(f)
    rc = _lib.load().srf_gln_apply2_add(_lib.ptr(f), _norm(f_sums, f_gamma, f_beta, f_prelu), _lib.ptr(y),
                                        _norm(y_sums, y_gamma, y_beta, y_prelu), _lib.ptr(out), _lib.ptr(out_sums), groups,
                                        channels, length, _lib.current_stream(dev))
    _lib.check(rc, "srf_gln_apply2_add")
    return out


def gln_apply_stats(x, sums, gamma, beta, prelu=None, out_sums=None, out=None):
    """y = GlobLN(x) from `sums` (+ PReLU where a slope is given); out_sums += {sum, sumsq} of the stored y."""
    dev = _chk(x, sums, gamma, beta, prelu, out_sums, out)
    groups, channels, length = x.shape
    if out is None:
        out = torch.empty_like(x)
    rc = _lib.load().srf_gln_apply_stats(_lib.ptr(x), _norm(sums, gamma, beta, prelu), _lib.ptr(out), _lib.ptr(out_sums), groups,
                                         channels, length, _lib.current_stream(dev))
    _lib.check(rc, "srf_gln_apply_stats")
    return out
