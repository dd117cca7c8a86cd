"""Thin ctypes wrappers of the attention kernels (csrc/srf_attention.hip; include/sudormrf_hip.h, "Attentive SuDoRM-RF v2" / "v3").

Same conventions as ``ops``: CUDA float32 tensors in, new tensors out, torch's current stream.  Kept out of ``ops`` on
purpose: these serve the attentive models' sub-module forwards and the kernel tests only."""
import ctypes as C
import math

import torch

from . import _lib, ops, ragged
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


def _mha_entry(name, Bt, q_lengths, k_lengths):
    """The C entry of one of the three ops and what its call inserts between the sizes and the scale: -> (function, its name,
    tables).  Neither list given: (srf_<name>, (): today's entry and profiler names).  Else srf_<name>_ragged and the two host
    tables (q table or None, k table or None); None = every example is full on that side (NULL in C).  The range of every
    entry and the batch cap are checked in C, before the first launch."""
    tabs, entry = [], "srf_" + name
    if q_lengths is not None or k_lengths is not None:
        entry += "_ragged"
        for what, values in (("q_lengths", q_lengths), ("k_lengths", k_lengths)):
            if values is None:
                tabs.append(None)
                continue
            tab, n = ragged._table(values, what)
            if n != Bt:
                raise _lib.SrfError("%s: %d %s for a batch of %d" % (name, n, what, Bt))
            tabs.append(tab)
    return getattr(_lib.load(), entry), entry, tabs


def _host_lengths(values, what):
    """lengths as a list of ints (None stays None); a device tensor is refused as ragged._table refuses it"""
    return None if values is None else list(ragged._table(values, what)[0])


def mha_attention(q, k, v, heads, scale=None, out=None, q_lengths=None, k_lengths=None):
    """q [Bt, H d, Lq], k / v [Bt, H d, Lk] -> [Bt, H d, Lq]: softmax(scale q^T k) v per (example, head); channel h d + j
    belongs to head h.  scale defaults to 1 / sqrt(d).
    Differentiable: with autograd on and q, k or v requiring grad the result carries a grad_fn whose backward is
    mha_attention_bwd (the forward then is mha_attention_lse, same output bits); otherwise the plain launch, as ever.
    q_lengths / k_lengths (each a list or a CPU tensor of Bt entries, or None = full): the ragged form -- example b attends
    from its first q_lengths[b] queries to its first k_lengths[b] keys; nothing past them is read, the output is exact 0 at
    queries past q_lengths[b], and inside the lengths the bits are those of the call on the example's own slices.  Both None:
    today's code path and bits."""
    if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
        if out is not None:
            raise _lib.SrfError("mha_attention: out= cannot be combined with autograd")
        return _MHAttention.apply(q, k, v, heads, scale, _host_lengths(q_lengths, "q_lengths"),
                                  _host_lengths(k_lengths, "k_lengths"))
    dev = _chk(q, k, v, out)
    Bt, HD, d, Lq, Lk = _mha_shapes("mha_attention", q, k, v, heads)
    fn, entry, tables = _mha_entry("mha_attention", Bt, q_lengths, k_lengths)
    if out is None:
        out = torch.empty((Bt, HD, Lq), dtype=torch.float32, device=dev)
    _lib.check(fn(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(out), Bt, heads, d, Lq, Lk, *tables, _mha_scale(scale, d),
                  _lib.current_stream(dev)), entry)
    return out


def mha_attention_lse(q, k, v, heads, scale=None, out=None, lse=None, q_lengths=None, k_lengths=None):
    """mha_attention that also returns lse [Bt, H, Lq], the per-query log-sum-exp of the scaled scores: -> (out, lse).  out has
    mha_attention's bits.  q_lengths / k_lengths: the ragged form (mha_attention); lse is exact 0 past q_lengths[b] too."""
    dev = _chk(q, k, v, out, lse)
    Bt, HD, d, Lq, Lk = _mha_shapes("mha_attention_lse", q, k, v, heads)
    fn, entry, tables = _mha_entry("mha_attention_lse", Bt, q_lengths, k_lengths)
    if out is None:
        out = torch.empty((Bt, HD, Lq), dtype=torch.float32, device=dev)
    if lse is None:
        lse = torch.empty((Bt, heads, Lq), dtype=torch.float32, device=dev)
    elif lse.numel() != Bt * heads * Lq:
        raise _lib.SrfError("mha_attention_lse: lse has %d elements, [Bt, H, Lq] = %d" % (lse.numel(), Bt * heads * Lq))
    _lib.check(fn(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(out), _lib.ptr(lse), Bt, heads, d, Lq, Lk, *tables,
                  _mha_scale(scale, d), _lib.current_stream(dev)), entry)
    return out, lse


def mha_attention_bwd_workspace_bytes(Bt, heads, d, Lq, Lk):
    return int(_lib.load().srf_mha_attention_bwd_workspace_bytes(Bt, heads, d, Lq, Lk))


def mha_attention_bwd(q, k, v, o, lse, go, heads, scale=None, gq=None, gk=None, gv=None, workspace=None, q_lengths=None,
                      k_lengths=None):
    """The gradient of mha_attention: o, lse as mha_attention_lse returned them for (q, k, v, scale), go the gradient of o
    -> (gq, gk, gv), written in full.  workspace: a tensor of at least mha_attention_bwd_workspace_bytes() (default: a new one).
    q_lengths / k_lengths: the ragged form, for o and lse of the ragged forward with the same lengths -- go, o and lse are not
    read past q_lengths[b]; gq is exact 0 past q_lengths[b], gk and gv past k_lengths[b]."""
    dev = _chk(q, k, v, o, lse, go, gq, gk, gv, workspace)
    Bt, HD, d, Lq, Lk = _mha_shapes("mha_attention_bwd", q, k, v, heads)
    fn, entry, tables = _mha_entry("mha_attention_bwd", Bt, q_lengths, k_lengths)
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
    _lib.check(fn(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(o), _lib.ptr(lse), _lib.ptr(go), _lib.ptr(gq), _lib.ptr(gk),
                  _lib.ptr(gv), _lib.ptr(workspace), Bt, heads, d, Lq, Lk, *tables, _mha_scale(scale, d), _lib.current_stream(dev)),
               entry)
    return gq, gk, gv


class _MHAttention(torch.autograd.Function):
    """mha_attention under autograd: the forward with lse, the HIP backward.  Saves q, k, v, o, lse -- nothing of size Lq x Lk."""

    @staticmethod
    def forward(ctx, q, k, v, heads, scale, q_lengths=None, k_lengths=None):
        q, k, v = q.detach(), k.detach(), v.detach()
        o, lse = mha_attention_lse(q, k, v, heads, scale, q_lengths=q_lengths, k_lengths=k_lengths)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.heads, ctx.scale, ctx.lengths = heads, scale, (q_lengths, k_lengths)
        return o

    @staticmethod
    def backward(ctx, go):
        q, k, v, o, lse = ctx.saved_tensors
        g = mha_attention_bwd(q, k, v, o, lse, go.contiguous(), ctx.heads, ctx.scale, q_lengths=ctx.lengths[0],
                              k_lengths=ctx.lengths[1])
        return tuple(t if need else None for t, need in zip(g, ctx.needs_input_grad[:3])) + (None, None, None, None)


def zero_past(x, lengths):
    """x [Bt, C, L], in place: exact 0.f at positions >= lengths[b] of example b (None: nothing to do) -> x.  One strided fill per
    shortened example on the current stream: nothing is uploaded, nothing synchronises."""
    if lengths is not None:
        for b, n in enumerate(lengths):
            if n < x.shape[-1]:
                x[b, :, n:].zero_()
    return x


def _data(gout, w):
    """the data gradient of y = W x + b: W^T gout, on the GEMM kernels"""
    wt = w.reshape(w.shape[0], -1).t().contiguous()
    return ops.pw_conv(gout, wt, torch.zeros(wt.shape[0], dtype=torch.float32, device=gout.device))


def _wgrad(gout, x, sums=None, gamma=None, beta=None, prelu=None):
    """ops.pw_wgrad for any length.  srf_pw_wgrad reads rows as float4 (L % 4 == 0): other lengths are zero-padded -- zero
    columns of gout add nothing to either sum, whatever the norm on load makes of x's padding.
    The kernel derives mean and variance from `sums` and the length it is GIVEN, so the padded call gets the sums scaled by
    padded / real length: the same mean and variance."""
    L = gout.shape[-1]
    pad = -L % 4
    if pad:
        gout, x = torch.nn.functional.pad(gout, (0, pad)), torch.nn.functional.pad(x, (0, pad))
        if sums is not None:
            sums = sums * ((L + pad) / L)
    return ops.pw_wgrad(gout, x, sums, gamma, beta, prelu)


class _MHALayer(torch.autograd.Function):
    """MHAttentionLayer.forward under autograd (enable_hip_training): the layer's own kernel sequence with the lse forward, and a
    backward of mha_attention_bwd, ops.pw_conv on the transposed weights (data gradients) and ops.pw_wgrad (weight and bias
    gradients).  Saves the transposed inputs and q, k, v, o, lse -- nothing of size Lq x Lk.
    With lengths (the ragged layer): the projections stay uniform -- a column of a 1x1 convolution depends on that column alone
    -- and the ragged attention sits between them.  The output is zeroed past q_lengths (it would hold O_proj.bias), and the
    backward zeroes its copy of the incoming gradient there, so o, go, gq, gk and gv are all exact zeros past the lengths:
    every weight-gradient GEMM multiplies the (finite) padding of its other operand by 0, every bias sum adds 0, and the data
    gradients past the lengths are W^T 0 = 0."""

    @staticmethod
    def forward(ctx, heads, scale, q_lengths, k_lengths, Q, K, V, wq, bq, wk, bk, wv, bv, wo, bo):
        t = lambda x: x.detach().transpose(1, 2).contiguous()
        xq = t(Q)
        xk = xq if K is Q else t(K)
        xv = xk if V is K else (xq if V is Q else t(V))
        q, k, v = ops.pw_conv(xq, wq, bq), ops.pw_conv(xk, wk, bk), ops.pw_conv(xv, wv, bv)
        o, lse = mha_attention_lse(q, k, v, heads, scale, q_lengths=q_lengths, k_lengths=k_lengths)
        ctx.save_for_backward(xq, xk, xv, q, k, v, o, lse, wq, wk, wv, wo)
        ctx.heads, ctx.scale, ctx.lengths = heads, scale, (q_lengths, k_lengths)
        return zero_past(ops.pw_conv(o, wo, bo), q_lengths).transpose(1, 2).contiguous()

    @staticmethod
    def backward(ctx, gy):
        xq, xk, xv, q, k, v, o, lse, wq, wk, wv, wo = ctx.saved_tensors
        need = ctx.needs_input_grad[2:]
        q_lengths, k_lengths = ctx.lengths
        g = gy.transpose(1, 2).contiguous()
        if q_lengths is not None:      # the gradient arriving at rows past q_lengths is ignored: zeroed in a copy of our own
            g = zero_past(g.clone() if g.data_ptr() == gy.data_ptr() else g, q_lengths)
        dwo, dbo = _wgrad(g, o)
        gq, gk, gv = mha_attention_bwd(q, k, v, o, lse, _data(g, wo), ctx.heads, ctx.scale, q_lengths=q_lengths, k_lengths=k_lengths)
        grads = [None, None, None, None]
        for i, (gp, w) in enumerate(((gq, wq), (gk, wk), (gv, wv))):
            grads.append(_data(gp, w).transpose(1, 2).contiguous() if need[2 + i] else None)
        for gp, x in ((gq, xq), (gk, xk), (gv, xv)):
            grads.extend(_wgrad(gp, x))
        return tuple(grads) + (dwo, dbo)


def mha_layer_train(layer, Q, K, V, q_lengths=None, k_lengths=None):
    """MHAttentionLayer.forward of an opted-in layer under autograd (the attentive models v2 and v3 share the class):
    Q [batch, Lq, emb_dim], K / V [batch, Lk, emb_dim] -> [batch, Lq, emb_dim], differentiable in the eight projection parameters
    and in Q, K, V.  q_lengths / k_lengths: the ragged layer (MHAttentionLayer.forward)."""
    par = [p for m in (layer.Q_proj, layer.K_proj, layer.V_proj, layer.O_proj) for p in (m.weight, m.bias)]
    _chk(*par)
    return _MHALayer.apply(layer.n_heads, layer.q_normalizer, _host_lengths(q_lengths, "q_lengths"),
                           _host_lengths(k_lengths, "k_lengths"), Q, K, V, *par)


def _u64(v):
    return C.c_ulonglong(int(v) & 0xFFFFFFFFFFFFFFFF)


def posenc_apply(a, pe, sums=None, gamma=None, beta=None, out=None, p=0.0, seed=0, offset=0, lengths=None):
    """x[b, c, l] = GlobLN(a)[b, c, l] + pe[l, c] (no norm when sums is None).  a [Bt, C, L]; pe [max_len, C] or [1, max_len, C].
    p > 0: under dropout (srf_posenc_apply_dropout): an element is kept and scaled by the fp32 1 / (1 - p), or exactly 0, by
    the Philox bit of (seed, offset, its flat index); p == 0 is the plain kernel.
    lengths (a list or a CPU tensor of Bt entries; None: nothing changes): the ragged form (srf_posenc_apply_ragged, inference
    only) -- example b is lengths[b] positions long, `sums` are its own-column sums and the norm counts C * lengths[b]; a and pe
    are not read at or past lengths[b] and x is exact 0 there."""
    dev = _chk(a, pe, sums, gamma, beta, out)
    Bt, Cc, L = a.shape
    if pe.shape[-1] != Cc:
        raise _lib.SrfError("posenc_apply: the table has %d channels, the input %d" % (pe.shape[-1], Cc))
    if out is None:
        out = torch.empty_like(a)
    if lengths is not None:
        if p != 0.0:
            raise _lib.SrfError("posenc_apply: the ragged form has no dropout (p = %g)" % p)
        frs = ragged._frames_for("srf_posenc_apply_ragged", lengths, Bt, "lengths")
        rc = _lib.load().srf_posenc_apply_ragged(_lib.ptr(a), _norm(sums, gamma, beta, None), _lib.ptr(pe), _lib.ptr(out), Bt, Cc, L,
                                                 pe.shape[-2], frs, _lib.current_stream(dev))
        _lib.check(rc, "srf_posenc_apply_ragged")
        return out
    if p == 0.0 and seed == 0 and offset == 0:
        rc = _lib.load().srf_posenc_apply(_lib.ptr(a), _norm(sums, gamma, beta, None), _lib.ptr(pe), _lib.ptr(out), Bt, Cc, L,
                                          pe.shape[-2], _lib.current_stream(dev))
        _lib.check(rc, "srf_posenc_apply")
        return out
    rc = _lib.load().srf_posenc_apply_dropout(_lib.ptr(a), _norm(sums, gamma, beta, None), _lib.ptr(pe), _lib.ptr(out), Bt, Cc, L,
                                              pe.shape[-2], C.c_float(p), _u64(seed), _u64(offset), _lib.current_stream(dev))
    _lib.check(rc, "srf_posenc_apply_dropout")
    return out


def posenc_dropout_bwd(gx, p, seed, offset, out=None):
    """gn = keep ? gx / (1 - p) : 0 with the mask of posenc_apply(..., p, seed, offset) recomputed; out may be gx itself."""
    dev = _chk(gx, out)
    Bt, Cc, L = gx.shape
    if out is None:
        out = torch.empty_like(gx)
    elif out.shape != gx.shape:
        raise _lib.SrfError("posenc_dropout_bwd: out %s differs from gx %s" % (tuple(out.shape), tuple(gx.shape)))
    rc = _lib.load().srf_posenc_dropout_bwd(_lib.ptr(gx), _lib.ptr(out), Bt, Cc, L, C.c_float(p), _u64(seed), _u64(offset),
                                            _lib.current_stream(dev))
    _lib.check(rc, "srf_posenc_dropout_bwd")
    return out


def dropout_mask(n, p, seed, offset, device="cuda"):
    """keep [n] uint8 in {0, 1}: the mask srf_posenc_apply_dropout applies to elements 0 .. n - 1."""
    keep = torch.empty(int(n), dtype=torch.uint8, device=device)
    _chk(keep)
    rc = _lib.load().srf_dropout_mask(_lib.ptr(keep), int(n), C.c_float(p), _u64(seed), _u64(offset),
                                      _lib.current_stream(keep.device))
    _lib.check(rc, "srf_dropout_mask")
    return keep


def draw_dropout_state():
    """One (seed, offset) pair from torch's CPU default generator: one randint of two int64 values, no device
    synchronisation.  torch.manual_seed(s) in front of two runs gives the same pairs, hence the same masks."""
    s = torch.randint(0, 2 ** 63 - 1, (2,), dtype=torch.int64)
    return int(s[0]), int(s[1])


def _drop_state(training, layer):
    """(p, seed, offset) of one call of a transformer layer's position-table dropout: in train() mode with p > 0 one pair from
    draw_dropout_state, else (0.0, 0, 0) = the plain kernels"""
    p = float(layer.pos_enc.dropout.p) if training else 0.0
    return (p,) + draw_dropout_state() if p > 0 else (0.0, 0, 0)


# ---- TransformerLayer / AttentiveUConvBlock under autograd -----------------------------------
_TL_PARAMS = 17   # mha.{Q,K,V,O}_proj.{weight, bias}, out_norm, out_mha_norm, ffn.conv, ffn.norm, ffn.act: state_dict() order
_TL_OUT_NORM = slice(8, 10)        # out_norm.{gamma, beta} in that list
_TL_Z, _TL_S_OUT = 9, 12           # z and out_norm's statistics slot in _tl_forward's saved tuple


def _tl_params(layer):
    m = layer.mha
    return [p for lin in (m.Q_proj, m.K_proj, m.V_proj, m.O_proj) for p in (lin.weight, lin.bias)] + [
        layer.out_norm.gamma, layer.out_norm.beta, layer.out_mha_norm.gamma, layer.out_mha_norm.beta, layer.ffn.conv.weight,
        layer.ffn.conv.bias, layer.ffn.norm.gamma, layer.ffn.norm.beta, layer.ffn.act.weight]


def _tl_forward(a, in_norm, pe, par, heads, scale, drop, apply_out_norm=True):
    """The layer's kernel sequence with the lse attention and (drop = (p, seed, offset), p > 0) the dropout posenc.
    -> (output, the tensors the backward reads); apply_out_norm=False leaves out_norm to the caller (the block merges z with
    out_norm as a lazy norm) and returns None for the output"""
    wq, bq, wk, bk, wv, bv, wo, bo, g_out, b_out, g_mha, b_mha, w_ffn, b_ffn, g_ffn, be_ffn, slope = par
    Bt, dev = a.shape[0], a.device
    xp = posenc_apply(a, pe, *(in_norm or (None, None, None)), p=drop[0], seed=drop[1], offset=drop[2])
    wqkv, bqkv = torch.cat([wq, wk, wv], 0).contiguous(), torch.cat([bq, bk, bv], 0).contiguous()
    qkv = ops.pw_conv(xp, wqkv, bqkv)
    hd = wq.shape[0]
    q, k, v = (qkv[:, i * hd:(i + 1) * hd].contiguous() for i in range(3))
    o, lse = mha_attention_lse(q, k, v, heads, scale)
    s_mha, s_ffn, s_out = (ops.new_sums(Bt, dev) for _ in range(3))
    y = ops.pw_conv(o, wo, bo, residual=xp, out_sums=s_mha)
    f = ops.pw_conv(y, w_ffn, b_ffn, in_sums=s_mha, in_gamma=g_mha, in_beta=b_mha, out_sums=s_ffn)
    z = gln_apply2_add(f, s_ffn, g_ffn, be_ffn, slope, y, s_mha, g_mha, b_mha, out_sums=s_out)
    out = ops.gln_apply(z, s_out, g_out, b_out) if apply_out_norm else None
    return out, (a, xp, q, k, v, o, lse, y, f, z, s_mha, s_ffn, s_out, wqkv)


def _tl_backward(g, saved, in_norm, par, heads, scale, drop):
    """-> (the 17 parameter gradients in _tl_params order, gx, (dgamma, dbeta) of in_norm or None): DESIGN.md 16.2's order"""
    a, xp, q, k, v, o, lse, y, f, z, s_mha, s_ffn, s_out, wqkv = saved
    wq, bq, wk, bk, wv, bv, wo, bo, g_out, b_out, g_mha, b_mha, w_ffn, b_ffn, g_ffn, be_ffn, slope = par
    gz, dg_out, db_out, _ = ops.gln_bwd(g, z, s_out, g_out, b_out)
    gf, dg_ffn, dbe_ffn, dslope = ops.gln_bwd(gz, f, s_ffn, g_ffn, be_ffn, slope)
    dw_ffn, db_ffn = _wgrad(gf, y, s_mha, g_mha, b_mha)
    g_yn = _data(gf, w_ffn)
    gy, dg_mha, db_mha, _ = ops.gln_bwd(gz, y, s_mha, g_mha, b_mha, gout2=g_yn)      # norm(y) has two consumers: one call
    dwo, dbo = _wgrad(gy, o)
    gq, gk, gv = mha_attention_bwd(q, k, v, o, lse, _data(gy, wo), heads, scale)
    gqkv = torch.cat([gq, gk, gv], 1)
    dwqkv, dbqkv = _wgrad(gqkv, xp)
    gxp = _data(gqkv, wqkv).add_(gy)                                                 # + the residual
    gn = posenc_dropout_bwd(gxp, drop[0], drop[1], drop[2], out=gxp) if drop[0] > 0 else gxp
    hd = wq.shape[0]
    dw = [dwqkv[i * hd:(i + 1) * hd].contiguous() for i in range(3)]
    db = [dbqkv[i * hd:(i + 1) * hd].contiguous() for i in range(3)]
    grads = [dw[0], db[0], dw[1], db[1], dw[2], db[2], dwo, dbo, dg_out, db_out, dg_mha, db_mha, dw_ffn.reshape(w_ffn.shape),
             db_ffn, dg_ffn, dbe_ffn, dslope]
    if in_norm is None:
        return grads, gn, None
    gx, dg_in, db_in, _ = ops.gln_bwd(gn, a, *in_norm)
    return grads, gx, (dg_in, db_in)


class _TransformerLayerTrain(torch.autograd.Function):
    """TransformerLayer.forward under autograd (enable_hip_training): one node around the whole layer.  Saves a, xp, q, k, v, o,
    lse, y, f, z, the statistics slots and (p, seed, offset) -- nothing of size Ld x Ld, and not the mask."""

    @staticmethod
    def forward(ctx, heads, scale, drop, pe, x, in_sums, in_gamma, in_beta, *par):
        par = [t.detach() for t in par]
        in_norm = None if in_sums is None else (in_sums, in_gamma.detach(), in_beta.detach())
        out, saved = _tl_forward(x.detach(), in_norm, pe, par, heads, scale, drop)
        ctx.save_for_backward(*saved, *par, *(in_norm or ()))
        ctx.n_saved, ctx.cfg = len(saved), (heads, scale, drop)
        return out

    @staticmethod
    def backward(ctx, g):
        t = ctx.saved_tensors
        saved, par, in_norm = t[:ctx.n_saved], t[ctx.n_saved:ctx.n_saved + _TL_PARAMS], t[ctx.n_saved + _TL_PARAMS:] or None
        grads, gx, din = _tl_backward(g.contiguous(), saved, in_norm, par, *ctx.cfg)
        dg_in, db_in = din or (None, None)
        return (None, None, None, None, gx, None, dg_in, db_in) + tuple(grads)


def transformer_layer_train(layer, x, in_sums=None, in_gamma=None, in_beta=None):
    """TransformerLayer.forward of an opted-in layer under autograd: x [Bt, emb_dim, Ld] (with in_sums / in_gamma / in_beta: the
    level's lazy GlobLN applied on load) -> the layer's output, differentiable in the layer's 17 parameters, in x and in
    in_gamma / in_beta.  In train() mode with pos_enc.dropout.p > 0 one (seed, offset) pair is drawn from torch's CPU
    generator per call; eval() or p == 0 runs the plain kernels (the inference forward's bits)."""
    par = _tl_params(layer)
    _chk(*par)
    return _TransformerLayerTrain.apply(layer.mha.n_heads, layer.mha.q_normalizer, _drop_state(layer.training, layer),
                                        layer.pos_enc.pe.detach(), x, in_sums, in_gamma, in_beta, *par)


def _ub_params(block):
    D = block.depth
    par = [block.proj_1x1.conv.weight, block.proj_1x1.conv.bias, block.proj_1x1.norm.gamma, block.proj_1x1.norm.beta,
           block.proj_1x1.act.weight]
    for k in range(D):
        m = block.spp_dw[k]
        par += [m.conv.weight, m.conv.bias, m.norm.gamma, m.norm.beta]
    return par + [block.final_norm.norm.gamma, block.final_norm.norm.beta, block.final_norm.act.weight, block.res_conv.weight,
                  block.res_conv.bias] + _tl_params(block.attention)


def _ub_split(par, D):
    """_ub_params' list by module: -> (proj_1x1's five, [the four of each level], final_norm's three + res_conv's two, the layer's)"""
    return par[:5], [par[5 + 4 * k:9 + 4 * k] for k in range(D)], par[5 + 4 * D:10 + 4 * D], par[10 + 4 * D:]


class _AttentiveUConvBlockTrain(torch.autograd.Function):
    """AttentiveUConvBlock.forward under autograd (enable_hip_training): one node around the block -- proj_1x1, the D dwconv5
    levels, the transformer layer on level D - 1 with that level's lazy norm, srf_merge, res_conv with final_norm on load plus
    the residual -- and the backward of DESIGN.md section 16.2."""

    @staticmethod
    def forward(ctx, D, heads, scale, drop, pe, x, *par):
        x, par = x.detach(), [t.detach() for t in par]
        (w_in, b_in, g_in, be_in, a_in), lv, (g_fin, b_fin, a_fin, w_res, b_res), tl = _ub_split(par, D)
        Bt, dev = x.shape[0], x.device
        s_in = ops.new_sums(Bt, dev)
        y1 = ops.pw_conv(x, w_in, b_in, out_sums=s_in)
        levels, sums, src, norm = [], [], y1, (s_in, g_in, be_in, a_in)
        for k in range(D):
            s_k = ops.new_sums(Bt, dev)
            src = ops.dwconv5(src, lv[k][0], lv[k][1], 1 if k == 0 else 2, *norm, out_sums=s_k)
            levels.append(src)
            sums.append(s_k)
            norm = (s_k, lv[k][2], lv[k][3], None)
        _, saved = _tl_forward(levels[-1], norm[:3], pe, tl, heads, scale, drop, apply_out_norm=False)
        z, s_out = saved[_TL_Z], saved[_TL_S_OUT]
        g_out, b_out = tl[_TL_OUT_NORM]
        # out_norm is merged as level D - 1's lazy norm (the whole-model walk does the same): no normalised z is stored
        s_m = ops.new_sums(Bt, dev)
        merged = ops.merge(levels[:-1] + [z], sums[:-1] + [s_out], [l[2] for l in lv[:-1]] + [g_out],
                           [l[3] for l in lv[:-1]] + [b_out], out_sums=s_m)
        out = ops.pw_conv(merged, w_res, b_res, in_sums=s_m, in_gamma=g_fin, in_beta=b_fin, in_prelu=a_fin, residual=x)
        ctx.save_for_backward(x, y1, s_in, merged, s_m, *levels[:-1], *sums, *saved, *par)
        ctx.cfg = (D, heads, scale, drop, len(saved))
        return out

    @staticmethod
    def backward(ctx, g):
        D, heads, scale, drop, n_saved = ctx.cfg
        t = list(ctx.saved_tensors)
        x, y1, s_in, merged, s_m = t[:5]
        levels, sums = t[5:4 + D], t[4 + D:4 + 2 * D]
        saved, par = t[4 + 2 * D:4 + 2 * D + n_saved], t[4 + 2 * D + n_saved:]
        (w_in, b_in, g_in, be_in, a_in), lv, (g_fin, b_fin, a_fin, w_res, b_res), tl = _ub_split(par, D)
        g = g.contiguous()
        dw_res, db_res = _wgrad(g, merged, s_m, g_fin, b_fin, a_fin)
        gm, dg_fin, db_fin, da_fin = ops.gln_bwd(_data(g, w_res), merged, s_m, g_fin, b_fin, a_fin)
        parts = ops.merge_bwd(gm, D)
        # level D - 1: its merge part is the gradient of the layer's OUTPUT; the layer returns the gradient of the level's
        # pre-norm tensor and of the level's norm
        tl_grads, gd, (dg_k, db_k) = _tl_backward(parts[D - 1], saved, (sums[D - 1], lv[D - 1][2], lv[D - 1][3]), tl, heads, scale,
                                                  drop)
        lgrads = [None] * D
        for k in range(D - 1, -1, -1):
            if k < D - 1:
                gd, dg_k, db_k, _ = ops.gln_bwd(parts[k], levels[k], sums[k], lv[k][2], lv[k][3], gout2=gin)
            xin, norm = (levels[k - 1], (sums[k - 1], lv[k - 1][2], lv[k - 1][3], None)) if k else (y1, (s_in, g_in, be_in, a_in))
            gin, dw_k, dbias_k = ops.dwconv5_bwd(gd, xin, lv[k][0], 1 if k == 0 else 2, *norm)
            lgrads[k] = [dw_k, dbias_k, dg_k, db_k]
        gy1, dg_in, dbe_in, da_in = ops.gln_bwd(gin, y1, s_in, g_in, be_in, a_in)
        dw_in, db_in = _wgrad(gy1, x)
        gx = _data(gy1, w_in).add_(g)                                               # + the skip
        grads = [dw_in.reshape(w_in.shape), db_in, dg_in, dbe_in, da_in] + [t_ for l in lgrads for t_ in l] + [
            dg_fin, db_fin, da_fin, dw_res.reshape(w_res.shape), db_res] + tl_grads
        return (None, None, None, None, None, gx) + tuple(grads)


def uconv_block_train(block, x):
    """AttentiveUConvBlock.forward of an opted-in block under autograd: x [Bt, out_channels, L] -> the same shape,
    differentiable in every parameter of the block and in x (pos_enc.pe is a buffer and gets none)."""
    par = _ub_params(block)
    _chk(*par)
    layer = block.attention
    return _AttentiveUConvBlockTrain.apply(block.depth, layer.mha.n_heads, layer.mha.q_normalizer, _drop_state(block.training, layer),
                                           layer.pos_enc.pe.detach(), x, *par)


def gln_apply2_add(f, f_sums, f_gamma, f_beta, f_prelu, y, y_sums, y_gamma, y_beta, y_prelu=None, out_sums=None, out=None,
                   lengths=None):
    """z = norm_f(f) + norm_y(y), each GlobLN (+ PReLU where a slope is given); out_sums += {sum, sumsq} of z.
    lengths (a list or a CPU tensor of `groups` entries; None: nothing changes): the ragged form (srf_gln_apply2_add_ragged) --
    group g is lengths[g] columns long (any count >= 1), both sums are own-column sums and both norms count C * lengths[g];
    z is exact 0 at or past lengths[g] and out_sums run over the group's own columns."""
    dev = _chk(f, f_sums, f_gamma, f_beta, f_prelu, y, y_sums, y_gamma, y_beta, y_prelu, out_sums, out)
    groups, channels, length = f.shape
    if out is None:
        out = torch.empty_like(f)
    if lengths is not None:
        frs = ragged._frames_for("srf_gln_apply2_add_ragged", lengths, groups, "lengths")
        rc = _lib.load().srf_gln_apply2_add_ragged(_lib.ptr(f), _norm(f_sums, f_gamma, f_beta, f_prelu), _lib.ptr(y),
                                                   _norm(y_sums, y_gamma, y_beta, y_prelu), _lib.ptr(out), _lib.ptr(out_sums),
                                                   groups, channels, length, frs, _lib.current_stream(dev))
        _lib.check(rc, "srf_gln_apply2_add_ragged")
        return out
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
