"""Ragged-batch forms of the kernels: one launch over examples of unequal length (include/sudormrf_hip.h, "Ragged forms").

The tensors keep their uniform layout -- [batch, channels, L] with L the row stride -- and every example brings its own length
in a host-side list.  What lies at or past an example's end is never read and may hold anything; outputs that carry GlobLN
statistics are exact zeros there, and the statistics count the example's own elements only, so every example is treated as
its own batch-1 call would treat it.  The lists travel in the launch arguments: nothing is uploaded, nothing synchronises.

The ragged forms of the original model's own kernels (gln_apply_c, encoder_bias_relu, softmax_mask, bias_rescale) live next to
their uniform twins in ``original``; that model pads a row to a multiple of lcm(K // 2, 2^depth) (``original.padded_frames``), not
to the Improved model's (K // 2) * 2^depth (``padded_frames`` below)."""
import ctypes as C

import torch

from . import _lib
from .ops import _chk

MAX_BATCH = _lib.RAGGED_MAX_BATCH


def _table(values, what):
    if isinstance(values, torch.Tensor) and values.device.type != "cpu":
        raise _lib.SrfError("%s must be a list or a CPU tensor (reading a device tensor would synchronise)" % what)
    vals = [int(v) for v in (values.tolist() if isinstance(values, torch.Tensor) else values)]
    return (C.c_int * len(vals))(*vals), len(vals)


def padded_frames(length, kernel_size, depth):
    """Frames of one example of `length` samples as its own batch-1 forward would have them: the length padded up to a
    multiple of (K // 2) * 2^depth (at least one), in hops (improved_sudormrf.py:244,303-314)."""
    h = kernel_size // 2
    n = h << depth
    return max(n, -(-int(length) // n) * n) // h


def frames_ok(frames, L, D):
    """Whether an example of a ragged pyramid call may be `frames` long under row stride L (no GPU needed)."""
    return bool(_lib.load().srf_pyramid_ragged_frames_ok(int(frames), int(L), int(D)))


def wav_stats(wav, lengths):
    """srf_wav_stats_ragged: wav [rows, T] or [rows, 1, T] (row b valid up to lengths[b]; nothing at or past it is read) ->
    stats [rows, 2] = {mean, unbiased std} of wav[b, :lengths[b]] (fp64 sums in a fixed order: a row's two numbers do not
    depend on the other rows)."""
    dev = _chk(wav)
    if wav.dtype != torch.float32 or wav.dim() not in (2, 3) or (wav.dim() == 3 and wav.shape[1] != 1):
        raise _lib.SrfError("srf_wav_stats_ragged: expected a float32 tensor [rows, T] or [rows, 1, T], got %s %s"
                            % (wav.dtype, tuple(wav.shape)))
    rows, T = wav.shape[0], wav.shape[-1]
    lens, n = _table(lengths, "lengths")
    if n != rows:
        raise _lib.SrfError("srf_wav_stats_ragged: %d lengths for %d rows" % (n, rows))
    stats = torch.empty((rows, 2), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().srf_wav_stats_ragged(_lib.ptr(wav), lens, _lib.ptr(stats), rows, T, _lib.current_stream(dev)),
               "srf_wav_stats_ragged")
    return stats


def wav_gather(utterances, T):
    """srf_wav_gather_ragged: a list of 1-D contiguous float32 tensors on one GPU (any element-aligned address: views into a
    larger buffer are fine) -> (wav [batch, 1, T] from torch.empty, lengths).  Row b holds utterance b in [0, lengths[b]);
    what lies past it is NOT written -- no ragged kernel reads it.  One launch; the pointers travel in its arguments."""
    utterances = list(utterances)
    if not utterances:
        raise _lib.SrfError("srf_wav_gather_ragged: empty list of utterances")
    for i, u in enumerate(utterances):
        if not isinstance(u, torch.Tensor) or u.dim() != 1 or u.dtype != torch.float32 or u.numel() == 0:
            raise _lib.SrfError("srf_wav_gather_ragged: utterance %d must be a non-empty 1-D float32 tensor, got %s %s"
                                % (i, getattr(u, "dtype", type(u).__name__), tuple(getattr(u, "shape", ()))))
        if u.device != utterances[0].device:
            raise _lib.SrfError("srf_wav_gather_ragged: utterance %d is on %s, utterance 0 on %s" % (i, u.device, utterances[0].device))
    dev = _chk(*utterances)
    batch = len(utterances)
    lengths = [u.numel() for u in utterances]
    lens, _ = _table(lengths, "lengths")
    rows = (C.c_void_p * batch)(*[u.data_ptr() for u in utterances])
    wav = torch.empty((batch, 1, int(T)), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().srf_wav_gather_ragged(rows, lens, _lib.ptr(wav), batch, int(T), _lib.current_stream(dev)),
               "srf_wav_gather_ragged")
    return wav, lengths


def encoder(wav, weight, L, lengths, frames, sums=None, in_stats=None):
    """srf_encoder_ragged: wav [Bt,1,T] (row b valid up to lengths[b]), weight [N,1,21] -> [Bt,N,L], zeros from frames[b] on.
    in_stats [Bt,2] = {mean, std} per row (wav_stats): the row is normalised on load, (x - mean) / (std + 1e-9), and the zero
    padding past lengths[b] applies to the normalised signal (srf_encoder_ragged_stats)."""
    dev = _chk(wav, weight, sums, in_stats)
    Bt, A, T = wav.shape
    N, A2, K = weight.shape
    assert A == A2
    lens, n1 = _table(lengths, "lengths")
    frs, n2 = _table(frames, "frames")
    if n1 != Bt or n2 != Bt:
        raise _lib.SrfError("srf_encoder_ragged: %d lengths / %d frames for a batch of %d" % (n1, n2, Bt))
    out = torch.empty((Bt, N, L), dtype=torch.float32, device=dev)
    if in_stats is not None:
        if in_stats.dtype != torch.float32 or tuple(in_stats.shape) != (Bt, 2):
            raise _lib.SrfError("srf_encoder_ragged_stats: in_stats must be float32 [%d, 2], got %s %s"
                                % (Bt, in_stats.dtype, tuple(in_stats.shape)))
        _lib.check(_lib.load().srf_encoder_ragged_stats(_lib.ptr(wav), _lib.ptr(weight), _lib.ptr(out), _lib.ptr(sums), Bt, A, T, N,
                                                        K, L, lens, frs, _lib.ptr(in_stats), _lib.current_stream(dev)),
                   "srf_encoder_ragged_stats")
        return out
    _lib.check(_lib.load().srf_encoder_ragged(_lib.ptr(wav), _lib.ptr(weight), _lib.ptr(out), _lib.ptr(sums), Bt, A, T, N, K, L,
                                              lens, frs, _lib.current_stream(dev)), "srf_encoder_ragged")
    return out


def pyramid(y1, in_sums, in_gamma, in_beta, in_prelu, weights, biases, gammas, betas, frames, out_sums=None, rows_per_example=1):
    """srf_pyramid_ragged: y1 [groups,C,L] (row g valid up to frames[g]) -> merged [groups,C,L], zeros from frames[g] on.
    rows_per_example > 1 (GroupComm's folded rows): groups = examples * rows_per_example GlobLN groups, `frames` holds one
    entry per EXAMPLE and group g is frames[g // rows_per_example] long (srf_pyramid_ragged_rows)."""
    dev = _chk(y1, in_sums, in_gamma, in_beta, in_prelu, *weights, *biases, *gammas, *betas, out_sums)
    groups, Cc, L = y1.shape
    D = len(weights)
    lib = _lib.load()
    frs, n = _table(frames, "frames")
    if n * int(rows_per_example) != groups:
        raise _lib.SrfError("srf_pyramid_ragged: %d frames for %d examples" % (n, groups // max(1, int(rows_per_example))))
    merged = torch.empty_like(y1)
    scratch = torch.empty(lib.srf_pyramid_scratch_bytes(groups, Cc, L, D), dtype=torch.uint8, device=dev)
    arr = lambda ts: (C.c_void_p * D)(*[t.data_ptr() for t in ts])
    nrm = _lib.make_norm(in_sums, in_gamma, in_beta, in_prelu)
    rc = lib.srf_pyramid_ragged_rows(_lib.ptr(y1), _lib.ptr(merged), C.byref(nrm), arr(weights), arr(biases), arr(gammas),
                                     arr(betas), groups, Cc, L, D, _lib.ptr(scratch), _lib.ptr(out_sums), frs,
                                     int(rows_per_example), _lib.current_stream(dev))
    _lib.check(rc, "srf_pyramid_ragged")
    return merged


def pw_conv(x, packed, bias, Cout, frames, in_sums=None, in_gamma=None, in_beta=None, in_prelu=None, residual=None,
            out_sums=None):
    """srf_pw_conv_packed_ragged: x [Bt,Cin,L] (row b valid up to frames[b]), packed = ops.pack_pw_weight(W [Cout,Cin]) ->
    [Bt,Cout,L].  With out_sums the output is exact zeros from frames[b] on; the residual form leaves it unspecified there."""
    dev = _chk(x, packed, bias, in_sums, in_gamma, in_beta, in_prelu, residual, out_sums)
    Bt, Cin, L = x.shape
    frs, n = _table(frames, "frames")
    if n != Bt:
        raise _lib.SrfError("srf_pw_conv_packed_ragged: %d frames for a batch of %d" % (n, Bt))
    y = torch.empty((Bt, Cout, L), dtype=torch.float32, device=dev)
    nrm = None if in_sums is None and in_prelu is None else C.byref(_lib.make_norm(in_sums, in_gamma, in_beta, in_prelu))
    rc = _lib.load().srf_pw_conv_packed_ragged(_lib.ptr(x), None, _lib.ptr(packed), _lib.ptr(bias), _lib.ptr(y), Bt, Cin, Cout, L,
                                               nrm, _lib.ptr(residual), _lib.ptr(out_sums), 0, None, 0, frs,
                                               _lib.current_stream(dev))
    _lib.check(rc, "srf_pw_conv_packed_ragged")
    return y


def pw_conv_supported(Bt, Cin, Cout, L, frames, *tensors):
    """Whether pw_conv (srf_pw_conv_packed_ragged) takes this call now: the library's own gate
    (srf_pw_conv_packed_ragged_supported: the 256 x 128 kernel's shape and reach, kernel mode, debug flags, every frames[b] a
    multiple of 4) and the 16-byte alignment of `tensors` (x, the residual; None entries allowed).  No GPU needed."""
    tab, n = _table(frames, "frames")
    return bool(n == Bt and _lib.load().srf_pw_conv_packed_ragged_supported(Bt, Cin, Cout, L, tab)
                and all(t is None or t.data_ptr() % 16 == 0 for t in tensors))


def pw_conv_mfma(x, weight, bias, frames, in_sums=None, in_gamma=None, in_beta=None, in_prelu=None, residual=None, out_sums=None):
    """srf_pw_conv_ragged (the 128 x 128 split-bf16 GEMM's ragged form): x [Bt,Cin,L] (row b valid up to frames[b], ANY count
    in 1..L), weight [Cout,Cin(,1)] fp32 -> y [Bt,Cout,L] from torch.empty.  A 128-column tile wholly past frames[b] is not
    written; in the tile that holds the example's end y is exact 0 from frames[b] on.  out_sums and the norm on load run over
    the example's own columns."""
    dev = _chk(x, weight, bias, in_sums, in_gamma, in_beta, in_prelu, residual, out_sums)
    Bt, Cin, L = x.shape
    Cout = weight.shape[0]
    frs, n = _table(frames, "frames")
    if n != Bt:
        raise _lib.SrfError("srf_pw_conv_ragged: %d frames for a batch of %d" % (n, Bt))
    y = torch.empty((Bt, Cout, L), dtype=torch.float32, device=dev)
    nrm = None if in_sums is None and in_prelu is None else C.byref(_lib.make_norm(in_sums, in_gamma, in_beta, in_prelu))
    rc = _lib.load().srf_pw_conv_ragged(_lib.ptr(x), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(y), Bt, Cin, Cout, L, nrm,
                                        _lib.ptr(residual), _lib.ptr(out_sums), frs, _lib.current_stream(dev))
    _lib.check(rc, "srf_pw_conv_ragged")
    return y


def pw_conv_mfma_supported(Bt, Cin, Cout, L, frames):
    """Whether pw_conv_mfma (srf_pw_conv_ragged) takes this call now: the library's own gate (srf_pw_conv_ragged_supported).
    No GPU needed."""
    tab, n = _table(frames, "frames")
    return bool(n == Bt and _lib.load().srf_pw_conv_ragged_supported(Bt, Cin, Cout, L, tab))


def pw_conv_pair_supported(Cin1, Cmid, Cout2, L):
    """Whether srf_pw_conv_pair_ragged serves these channel counts / this row stride (no GPU needed)."""
    return bool(_lib.load().srf_pw_conv_pair_ragged_supported(Cin1, Cmid, Cout2, L))


def pw_conv_pair(x, packed1, bias1, in_sums, in_gamma, in_beta, in_prelu, residual, packed2, bias2, Cmid, Cout2, frames,
                 out_sums2=None):
    """srf_pw_conv_pair_ragged: y = W1 f(x) + b1 (+ residual) (unspecified past frames[b]), y2 = W2 y + b2 (exact zeros past
    frames[b], statistics over the example's own columns).  Returns (y, y2)."""
    dev = _chk(x, packed1, bias1, in_sums, in_gamma, in_beta, in_prelu, residual, packed2, bias2, out_sums2)
    Bt, Cin1, L = x.shape
    frs, n = _table(frames, "frames")
    if n != Bt:
        raise _lib.SrfError("srf_pw_conv_pair_ragged: %d frames for a batch of %d" % (n, Bt))
    y = torch.empty((Bt, Cmid, L), dtype=torch.float32, device=dev)
    y2 = torch.empty((Bt, Cout2, L), dtype=torch.float32, device=dev)
    nrm = C.byref(_lib.make_norm(in_sums, in_gamma, in_beta, in_prelu)) if in_sums is not None else None
    rc = _lib.load().srf_pw_conv_pair_ragged(_lib.ptr(x), _lib.ptr(packed1), _lib.ptr(bias1), _lib.ptr(y), nrm,
                                             _lib.ptr(residual), _lib.ptr(packed2), _lib.ptr(bias2), _lib.ptr(y2),
                                             _lib.ptr(out_sums2), Bt, Cin1, Cmid, Cout2, L, frs, _lib.current_stream(dev))
    _lib.check(rc, "srf_pw_conv_pair_ragged")
    return y, y2


def tac(x, params, G, frames, out_sums=None):
    """srf_tac_ragged (the MFMA kernel: n = 16, G = 16): x [Bt, G*n, L] (row b valid up to frames[b]; what lies past it may hold
    anything), params = the 9 TAC tensors in state_dict order -> q [Bt, G*n, L] (pre-norm), exact zeros from frames[b] on;
    out_sums [Bt*G, 64, 2] += the sums of the stored q per (example, group)."""
    dev = _chk(x, *params, out_sums)
    Bt, Ctot, L = x.shape
    n = Ctot // G
    frs, cnt = _table(frames, "frames")
    if cnt != Bt:
        raise _lib.SrfError("srf_tac_ragged: %d frames for a batch of %d" % (cnt, Bt))
    q = torch.empty_like(x)
    arr = (C.c_void_p * 9)(*[p.data_ptr() for p in params])
    rc = _lib.load().srf_tac_ragged(_lib.ptr(x), _lib.ptr(q), arr, Bt, G, n, 3 * n, L, _lib.ptr(out_sums), frs,
                                    _lib.current_stream(dev))
    _lib.check(rc, "srf_tac_ragged")
    return q


def pw_conv_small_supported(Cin, Cout, L):
    """Whether srf_pw_conv_small_ragged serves these channel counts / this row stride (no GPU needed)."""
    return bool(_lib.load().srf_pw_conv_small_ragged_supported(Cin, Cout, L))


def pw_conv_small(x, weight, bias, frames, rows_per_example=1, in_sums=None, in_gamma=None, in_beta=None, in_prelu=None,
                  residual=None, out_sums=None, pre_q=None, pre_sums=None, pre_gamma=None, pre_beta=None):
    """srf_pw_conv_small_ragged: GroupComm's per-group 1x1 convolutions over folded rows.  x [rows, Cin, L] with
    rows = examples * rows_per_example, weight [Cout, Cin(, 1)], `frames` one entry per EXAMPLE.
    Pre-add form (pre_q, pre_sums, pre_gamma, pre_beta, out_sums): returns (y, u) -- u = x + GlobLN(pre_q) valid on the
    example's own columns, y = W u + bias exact zeros past them.  Residual form (in_sums, in_gamma, in_beta, in_prelu,
    residual): returns y, valid on the example's own columns only."""
    dev = _chk(x, weight, bias, in_sums, in_gamma, in_beta, in_prelu, residual, out_sums, pre_q, pre_sums, pre_gamma, pre_beta)
    rows, Cin, L = x.shape
    Cout = weight.shape[0]
    frs, n = _table(frames, "frames")
    if n * int(rows_per_example) != rows:
        raise _lib.SrfError("srf_pw_conv_small_ragged: %d frames for %d rows of %d per example" % (n, rows, rows_per_example))
    y = torch.empty((rows, Cout, L), dtype=torch.float32, device=dev)
    u = torch.empty_like(x) if pre_q is not None else None
    nrm = None if in_sums is None and in_prelu is None else C.byref(_lib.make_norm(in_sums, in_gamma, in_beta, in_prelu))
    pre = None if pre_q is None else C.byref(_lib.make_norm(pre_sums, pre_gamma, pre_beta, None))
    rc = _lib.load().srf_pw_conv_small_ragged(_lib.ptr(x), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(y), rows, Cin, Cout, L, nrm,
                                              _lib.ptr(residual), _lib.ptr(out_sums), _lib.ptr(pre_q), pre, _lib.ptr(u), frs,
                                              int(rows_per_example), _lib.current_stream(dev))
    _lib.check(rc, "srf_pw_conv_small_ragged")
    return (y, u) if pre_q is not None else y


# ---- the attentive block's kernels (include/sudormrf_hip.h, "Attentive block on a ragged batch") ----
def _frames_for(name, values, groups, what="frames"):
    tab, n = _table(values, what)
    if n != groups:
        raise _lib.SrfError("%s: %d %s for a batch of %d" % (name, n, what, groups))
    return tab


def dwconv5(x, weight, bias, stride, in_frames, in_sums=None, in_gamma=None, in_beta=None, in_prelu=None, out_sums=None):
    """srf_dwconv5_ragged: ops.dwconv5 on x [Bt,C,Lin] whose row b is valid up to in_frames[b] (even under stride 2): the norm on
    load counts C * in_frames[b], the taps meet zeros at the example's own end, y [Bt,C,Lout] is exact 0 from in_frames[b] //
    stride on and out_sums run over the example's own outputs."""
    dev = _chk(x, weight, bias, in_sums, in_gamma, in_beta, in_prelu, out_sums)
    Bt, Cc, Lin = x.shape
    frs = _frames_for("srf_dwconv5_ragged", in_frames, Bt, "in_frames")
    y = torch.empty((Bt, Cc, (Lin - 1) // stride + 1), dtype=torch.float32, device=dev)
    nrm = None if in_sums is None and in_prelu is None else C.byref(_lib.make_norm(in_sums, in_gamma, in_beta, in_prelu))
    rc = _lib.load().srf_dwconv5_ragged(_lib.ptr(x), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(y), Bt, Cc, Lin, stride, nrm,
                                        _lib.ptr(out_sums), frs, _lib.current_stream(dev))
    _lib.check(rc, "srf_dwconv5_ragged")
    return y


def merge(levels, sums, gammas, betas, frames, out_sums=None):
    """srf_merge_ragged: ops.merge on levels[k] [Bt,C,L>>k] whose row b is valid up to frames[b] >> k (frames[b] a multiple of
    2^(D-1)): level k's norm counts C * (frames[b] >> k), merged is exact 0 on [frames[b], L), out_sums run over own columns."""
    dev = _chk(*levels, *sums, *gammas, *betas, out_sums)
    D = len(levels)
    Bt, Cc, L = levels[0].shape
    frs = _frames_for("srf_merge_ragged", frames, Bt)
    y = torch.empty((Bt, Cc, L), dtype=torch.float32, device=dev)
    lv = (C.c_void_p * D)(*[t.data_ptr() for t in levels])
    norms = (_lib.srf_norm * D)(*[_lib.make_norm(s, g, b, None) for s, g, b in zip(sums, gammas, betas)])
    rc = _lib.load().srf_merge_ragged(lv, norms, D, _lib.ptr(y), Bt, Cc, L, _lib.ptr(out_sums), frs, _lib.current_stream(dev))
    _lib.check(rc, "srf_merge_ragged")
    return y


def gln_stats(x, frames):
    """srf_gln_stats_ragged: x [groups, C, L] -> sums [groups, STAT_BUCKETS, 2] over x[g, :, :frames[g]], written in a fixed order
    (no atomics: the same bits on every run, and a group's numbers do not depend on the other groups)."""
    dev = _chk(x)
    groups, Cc, L = x.shape
    frs = _frames_for("srf_gln_stats_ragged", frames, groups)
    sums = torch.empty((groups, _lib.STAT_BUCKETS, 2), dtype=torch.float64, device=dev)
    rc = _lib.load().srf_gln_stats_ragged(_lib.ptr(x), _lib.ptr(sums), groups, Cc, L, frs, _lib.current_stream(dev))
    _lib.check(rc, "srf_gln_stats_ragged")
    return sums


def gln_apply(x, sums, gamma, beta, frames, prelu=None):
    """srf_gln_apply_ragged: y = GlobLN(x) (+ PReLU) counting C * frames[g] per group, exact 0 from frames[g] on (any
    frames[g] >= 1); `sums` are the group's own-column sums."""
    dev = _chk(x, sums, gamma, beta, prelu)
    groups, Cc, L = x.shape
    frs = _frames_for("srf_gln_apply_ragged", frames, groups)
    y = torch.empty_like(x)
    n = _lib.make_norm(sums, gamma, beta, prelu)
    rc = _lib.load().srf_gln_apply_ragged(_lib.ptr(x), _lib.ptr(y), C.byref(n), groups, Cc, L, frs, _lib.current_stream(dev))
    _lib.check(rc, "srf_gln_apply_ragged")
    return y


def sums_scale(sums, L, frames):
    """srf_sums_scale_ragged: a copy of own-column `sums` scaled by L / frames[g] in double -- what a UNIFORM kernel's on-load
    norm takes on a ragged batch: with the count C * L it assumes, the example's own mean and variance."""
    dev = _chk(sums)
    groups = sums.shape[0]
    frs = _frames_for("srf_sums_scale_ragged", frames, groups)
    out = torch.empty_like(sums)
    rc = _lib.load().srf_sums_scale_ragged(_lib.ptr(sums), _lib.ptr(out), groups, int(L), frs, _lib.current_stream(dev))
    _lib.check(rc, "srf_sums_scale_ragged")
    return out
