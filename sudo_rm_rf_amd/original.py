"""Thin ctypes wrappers of the original SuDoRM-RF's own kernels (csrc/srf_original.hip; include/sudormrf_hip.h, "Original SuDoRM-RF").

Same conventions as ``ops``: CUDA float32 tensors in, new tensors out (or ``out=``), torch's current stream.  Kept out of ``ops``
on purpose: these serve the original model's sub-module forwards and the kernel tests only."""
import torch

from . import _lib
from .ops import _chk, _norm

MAX_SOURCES = _lib.SOFTMAX_MASK_MAX_SOURCES


def gln_apply_c(x, sums, gamma, beta, slopes=None, add=None, out_sums=None, out=None):
    """y = GlobLN(x) from `sums`, PReLU with one slope per channel where `slopes` [C] is given, + `add` where given; out_sums +=
    {sum, sumsq} of the stored y.  x [groups, C, L]."""
    dev = _chk(x, sums, gamma, beta, slopes, add, out_sums, out)
    groups, channels, length = x.shape
    if out is None:
        out = torch.empty_like(x)
    rc = _lib.load().srf_gln_apply_c(_lib.ptr(x), _norm(sums, gamma, beta, None), _lib.ptr(slopes), _lib.ptr(add), _lib.ptr(out),
                                     _lib.ptr(out_sums), groups, channels, length, _lib.current_stream(dev))
    _lib.check(rc, "srf_gln_apply_c")
    return out


def encoder_bias_relu(wav, weight, bias, L, sums=None, in_stats=None):
    """wav [Bt, 1, T], weight [N, 1, K], bias [N] -> relu(conv + bias) [Bt, N, L]; sums += statistics of the result; in_stats
    [Bt, 2] {mean, std}: the rows are normalised on load."""
    dev = _chk(wav, weight, bias, sums, in_stats)
    Bt, A, T = wav.shape
    N, A2, K = weight.shape
    if A != 1 or A2 != 1:
        raise _lib.SrfError("encoder_bias_relu: one audio channel only")
    out = torch.empty((Bt, N, L), dtype=torch.float32, device=dev)
    rc = _lib.load().srf_encoder_bias_relu(_lib.ptr(wav), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(out), _lib.ptr(sums), Bt, T, N, K,
                                           L, _lib.ptr(in_stats), _lib.current_stream(dev))
    _lib.check(rc, "srf_encoder_bias_relu")
    return out


def mask_weight_fill(m_weight, m_bias):
    """m.weight [S, 1, N + 1, 1], m.bias [S] -> (Tz [S N, N], row bias [S N]): the mask layer as a 1x1 convolution's weight."""
    dev = _chk(m_weight, m_bias)
    S, N = m_weight.shape[0], m_weight.shape[2] - 1
    tz = torch.empty((S * N, N), dtype=torch.float32, device=dev)
    rows = torch.empty((S * N,), dtype=torch.float32, device=dev)
    rc = _lib.load().srf_mask_weight_fill(_lib.ptr(m_weight), _lib.ptr(m_bias), _lib.ptr(tz), _lib.ptr(rows), N, S,
                                          _lib.current_stream(dev))
    _lib.check(rc, "srf_mask_weight_fill")
    return tz, rows


def softmax_mask(z, enc, sources, out=None):
    """z [Bt, S N, L], enc [Bt, N, L] -> softmax over the S sources (S = 1: sigmoid) times enc, [Bt, S N, L]."""
    dev = _chk(z, enc, out)
    Bt, SN, L = z.shape
    N = enc.shape[1]
    if SN != sources * N or enc.shape != (Bt, N, L):
        raise _lib.SrfError("softmax_mask: z %s and enc %s do not fit %d sources" % (tuple(z.shape), tuple(enc.shape), sources))
    if out is None:
        out = torch.empty_like(z)
    rc = _lib.load().srf_softmax_mask(_lib.ptr(z), _lib.ptr(enc), _lib.ptr(out), Bt, sources, N, L, _lib.current_stream(dev))
    _lib.check(rc, "srf_softmax_mask")
    return out


def decoder_weight_expand(weight, sources):
    """The grouped ConvTranspose1d weight [S N, 1, K] -> the block-diagonal [S N, S, K] of an ungrouped one."""
    dev = _chk(weight)
    SN, one, K = weight.shape
    if one != 1 or SN % sources:
        raise _lib.SrfError("decoder_weight_expand: weight %s does not fit %d groups" % (tuple(weight.shape), sources))
    out = torch.empty((SN, sources, K), dtype=torch.float32, device=dev)
    rc = _lib.load().srf_decoder_weight_expand(_lib.ptr(weight), _lib.ptr(out), SN // sources, sources, K, _lib.current_stream(dev))
    _lib.check(rc, "srf_decoder_weight_expand")
    return out


def bias_rescale(est, bias, stats=None, wav=None, mixture_consistency=False):
    """IN PLACE over est [Bt, S, T]: + bias[s]; with stats [Bt, 2] {mean, std} of the raw mixture wav [Bt, 1, T]: (est + bias) * std
    + mean and, on request, mixture consistency against the mixture normalised on the fly.  Returns est."""
    dev = _chk(est, bias, stats, wav)
    Bt, S, T = est.shape
    rc = _lib.load().srf_bias_rescale(_lib.ptr(est), _lib.ptr(bias), _lib.ptr(stats), _lib.ptr(wav), int(bool(mixture_consistency)),
                                      Bt, S, T, _lib.current_stream(dev))
    _lib.check(rc, "srf_bias_rescale")
    return est
