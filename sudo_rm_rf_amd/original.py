"""Thin ctypes wrappers of the original SuDoRM-RF's own kernels (csrc/srf_original.hip, csrc/srf_original_train.hip;
include/sudormrf_hip.h, "Original SuDoRM-RF").

Same conventions as ``ops``: CUDA float32 tensors in, new tensors out (or ``out=``), torch's current stream.  Kept out of ``ops``
on purpose: these serve the original model's sub-module forwards and the kernel tests only."""
import math

import torch

from . import _lib
from .ops import _chk, _norm
from .ragged import _table as _host_table

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


# ---- the ragged forms (include/sudormrf_hip.h, "Ragged forms"): `frames` / `lengths` are host lists, one entry per example
def _table(values, what, n):
    arr, got = _host_table(values, what)
    if got != n:
        raise _lib.SrfError("%s: %d entries for a batch of %d" % (what, got, n))
    return arr


def padded_frames(length, kernel_size, depth):
    """Frames of one example of `length` samples as its own batch-1 forward has them: the length padded up to a multiple of
    lcm(K // 2, 2^depth), only when it is not one already (sudormrf.py, pad_to_appropriate_length), in hops."""
    h = kernel_size // 2
    lcm = h * 2 ** depth // math.gcd(h, 2 ** depth)
    return -(-int(length) // lcm) * lcm // h


def gln_apply_c_ragged(x, sums, gamma, beta, frames, slopes=None, add=None, out_sums=None, out=None):
    """gln_apply_c over groups of unequal length: group g is frames[g] columns long (a multiple of 4); x and add are not read past
    it, y is exact 0 there, the GlobLN count is C * frames[g] and out_sums run over the group's own columns."""
    dev = _chk(x, sums, gamma, beta, slopes, add, out_sums, out)
    groups, channels, length = x.shape
    if out is None:
        out = torch.empty_like(x)
    rc = _lib.load().srf_gln_apply_c_ragged(_lib.ptr(x), _norm(sums, gamma, beta, None), _lib.ptr(slopes), _lib.ptr(add), _lib.ptr(out),
                                            _lib.ptr(out_sums), groups, channels, length, _table(frames, "frames", groups),
                                            _lib.current_stream(dev))
    _lib.check(rc, "srf_gln_apply_c_ragged")
    return out


def encoder_bias_relu_ragged(wav, weight, bias, L, lengths, frames, sums=None, in_stats=None):
    """encoder_bias_relu over rows of unequal length (K = 21): row b is lengths[b] samples = frames[b] frames long; nothing at or
    past lengths[b] is read, frames at or past frames[b] are exact 0, the sums run over the row's own frames."""
    dev = _chk(wav, weight, bias, sums, in_stats)
    Bt, A, T = wav.shape
    N, A2, K = weight.shape
    if A != 1 or A2 != 1:
        raise _lib.SrfError("encoder_bias_relu_ragged: one audio channel only")
    out = torch.empty((Bt, N, L), dtype=torch.float32, device=dev)
    rc = _lib.load().srf_encoder_bias_relu_ragged(_lib.ptr(wav), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(out), _lib.ptr(sums), Bt, T,
                                                  N, K, L, _table(lengths, "lengths", Bt), _table(frames, "frames", Bt),
                                                  _lib.ptr(in_stats), _lib.current_stream(dev))
    _lib.check(rc, "srf_encoder_bias_relu_ragged")
    return out


def softmax_mask_ragged(z, enc, sources, frames, out=None):
    """softmax_mask over examples of unequal length: z and enc are not read at columns >= frames[b], the result is exact 0 there."""
    dev = _chk(z, enc, out)
    Bt, SN, L = z.shape
    N = enc.shape[1]
    if SN != sources * N or enc.shape != (Bt, N, L):
        raise _lib.SrfError("softmax_mask_ragged: z %s and enc %s do not fit %d sources" % (tuple(z.shape), tuple(enc.shape), sources))
    if out is None:
        out = torch.empty_like(z)
    rc = _lib.load().srf_softmax_mask_ragged(_lib.ptr(z), _lib.ptr(enc), _lib.ptr(out), Bt, sources, N, L, _table(frames, "frames", Bt),
                                             _lib.current_stream(dev))
    _lib.check(rc, "srf_softmax_mask_ragged")
    return out


def bias_rescale_ragged(est, bias, lengths, stats=None, wav=None, mixture_consistency=False):
    """bias_rescale IN PLACE over rows of unequal length: t < lengths[b] as bias_rescale, t >= lengths[b] exactly 0; wav is never
    read at or past lengths[b].  Returns est."""
    dev = _chk(est, bias, stats, wav)
    Bt, S, T = est.shape
    rc = _lib.load().srf_bias_rescale_ragged(_lib.ptr(est), _lib.ptr(bias), _lib.ptr(stats), _lib.ptr(wav),
                                             int(bool(mixture_consistency)), Bt, S, T, _table(lengths, "lengths", Bt),
                                             _lib.current_stream(dev))
    _lib.check(rc, "srf_bias_rescale_ragged")
    return est


# ---- the training step's own kernels (csrc/srf_original_train.hip).  Parameter gradients are ACCUMULATED into the tensors given.
def gln_c_bwd(gout, x, sums, gamma, beta, slopes=None, gout2=None, gx=None, accumulate=False, dgamma=None, dbeta=None, dslope=None):
    """Backward of gln_apply_c: gout (+ gout2) is the gradient w.r.t. [PReLU_c](GlobLN(x)); returns gx [groups, C, L] (given and
    accumulate: added to); dgamma, dbeta, dslope [C] += their sums where given."""
    dev = _chk(gout, x, sums, gamma, beta, slopes, gout2, gx, dgamma, dbeta, dslope)
    groups, channels, length = x.shape
    lib = _lib.load()
    if gx is None:
        if accumulate:
            raise _lib.SrfError("gln_c_bwd: accumulate needs the gx to add to")
        gx = torch.empty_like(x)
    scratch = torch.empty(lib.srf_gln_c_bwd_scratch_bytes(groups, channels, length), dtype=torch.uint8, device=dev)
    rc = lib.srf_gln_c_bwd(_lib.ptr(gout), _lib.ptr(gout2), _lib.ptr(x), _norm(sums, gamma, beta, None), _lib.ptr(slopes), groups,
                           channels, length, _lib.ptr(gx), int(bool(accumulate)), _lib.ptr(dgamma), _lib.ptr(dbeta), _lib.ptr(dslope),
                           _lib.ptr(scratch), _lib.current_stream(dev))
    _lib.check(rc, "srf_gln_c_bwd")
    return gx


def softmax_mask_bwd(z, enc, gv, sources, gz=None, genc=None, accumulate_genc=False):
    """Backward of softmax_mask from the logits: (gz [Bt, S N, L] -- may be gv --, genc [Bt, N, L])."""
    dev = _chk(z, enc, gv, gz, genc)
    Bt, SN, L = z.shape
    N = enc.shape[1]
    if SN != sources * N or enc.shape != (Bt, N, L) or gv.shape != z.shape:
        raise _lib.SrfError("softmax_mask_bwd: z %s, gv %s and enc %s do not fit %d sources"
                            % (tuple(z.shape), tuple(gv.shape), tuple(enc.shape), sources))
    if gz is None:
        gz = torch.empty_like(z)
    if genc is None:
        if accumulate_genc:
            raise _lib.SrfError("softmax_mask_bwd: accumulate_genc needs the genc to add to")
        genc = torch.empty_like(enc)
    rc = _lib.load().srf_softmax_mask_bwd(_lib.ptr(z), _lib.ptr(enc), _lib.ptr(gv), _lib.ptr(gz), _lib.ptr(genc),
                                          int(bool(accumulate_genc)), Bt, sources, N, L, _lib.current_stream(dev))
    _lib.check(rc, "srf_softmax_mask_bwd")
    return gz, genc


def mask_weight_fold(dtz, drow, dm_weight, dm_bias):
    """dm_weight [S, 1, N + 1, 1] += the diagonals of dtz [S N, N]; dm_bias [S] += the sums of drow [S N].  In place."""
    dev = _chk(dtz, drow, dm_weight, dm_bias)
    S, N = dm_weight.shape[0], dm_weight.shape[2] - 1
    rc = _lib.load().srf_mask_weight_fold(_lib.ptr(dtz), _lib.ptr(drow), _lib.ptr(dm_weight), _lib.ptr(dm_bias), N, S,
                                          _lib.current_stream(dev))
    _lib.check(rc, "srf_mask_weight_fold")


def decoder_weight_contract(dwexp, dweight):
    """dweight [S N, 1, K] += the diagonal blocks of dwexp [S N, S, K].  In place."""
    dev = _chk(dwexp, dweight)
    SN, S, K = dwexp.shape
    rc = _lib.load().srf_decoder_weight_contract(_lib.ptr(dwexp), _lib.ptr(dweight), SN // S, S, K, _lib.current_stream(dev))
    _lib.check(rc, "srf_decoder_weight_contract")


def decoder_bias_grad(grad_out, dbias):
    """dbias [S] += grad_out [Bt, S, T] summed over batch and time.  In place."""
    dev = _chk(grad_out, dbias)
    Bt, S, T = grad_out.shape
    lib = _lib.load()
    scratch = torch.empty(lib.srf_decoder_bias_grad_scratch_floats(S), dtype=torch.float32, device=dev)
    rc = lib.srf_decoder_bias_grad(_lib.ptr(grad_out), _lib.ptr(dbias), Bt, S, T, _lib.ptr(scratch), _lib.current_stream(dev))
    _lib.check(rc, "srf_decoder_bias_grad")


def relu_gate(g, s):
    """g = 0 where the saved post-ReLU output s is not positive.  In place; returns g."""
    dev = _chk(g, s)
    rc = _lib.load().srf_relu_gate(_lib.ptr(g), _lib.ptr(s), g.numel(), _lib.current_stream(dev))
    _lib.check(rc, "srf_relu_gate")
    return g
