"""Thin ctypes wrappers of the attention kernels (csrc/srf_attention.hip; include/sudormrf_hip.h, "Attentive SuDoRM-RF v2" / "v3").

Same conventions as ``ops``: CUDA float32 tensors in, new tensors out, torch's current stream.  Kept out of ``ops`` on
purpose: these serve the attentive models' sub-module forwards and the kernel tests only."""
import ctypes as C
import math

import torch

from . import _lib
from .ops import _chk, _norm


def mha_attention_mfma_supported(d):
    """Whether the exact-fp32 MFMA kernel serves head dimension d under the current kernel mode (else: the VALU kernel)."""
    return bool(_lib.load().srf_mha_attention_mfma_supported(int(d)))


def mha_attention(q, k, v, heads, scale=None, out=None):
    """q [Bt, H d, Lq], k / v [Bt, H d, Lk] -> [Bt, H d, Lq]: softmax(scale q^T k) v per (example, head); channel h d + j
    belongs to head h.  scale defaults to 1 / sqrt(d)."""
    dev = _chk(q, k, v, out)
    Bt, HD, Lq = q.shape
    Lk = k.shape[-1]
    if k.shape != (Bt, HD, Lk) or v.shape != (Bt, HD, Lk) or HD % heads:
        raise _lib.SrfError("mha_attention: q %s, k %s, v %s do not fit %d heads" % (tuple(q.shape), tuple(k.shape),
                                                                                     tuple(v.shape), heads))
    d = HD // heads
    if out is None:
        out = torch.empty((Bt, HD, Lq), dtype=torch.float32, device=dev)
    rc = _lib.load().srf_mha_attention(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(out), Bt, heads, d, Lq, Lk,
                                       C.c_float(1.0 / math.sqrt(d) if scale is None else scale), _lib.current_stream(dev))
    _lib.check(rc, "srf_mha_attention")
    return out


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
