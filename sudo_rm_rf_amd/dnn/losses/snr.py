"""Host-side mirror of the reference's ``sudo_rm_rf.dnn.losses.snr`` as its FUSS runner uses it:

    PermInvariantSNRwithZeroRefs(n_sources=max, zero_mean=False, backward_loss=True, inactivity_threshold=-40.)
                                                         losses/snr.py:13-142; experiments/run_fuss_separation.py:91-102,257-259

Same constructor, attributes, ``forward`` signature and return conventions; the arithmetic runs in csrc/srf_loss_fuss.hip
(one streaming pass + a finalize launch for the forward, one pass for the gradient; deterministic).  1..4 sources, FUSS's
maximum.  CPU tensors raise: there is no fallback.

``SimplerPermInvariantSNRwithZeroRefs`` (snr.py:145-262) is not mirrored: with ``backward_loss=True`` its ``compute_snr``
returns one value and the reference's own ``forward`` fails unpacking it, and with ``backward_loss=False`` it computes what
the class above computes.
"""
import ctypes as C
import itertools

import torch
from torch import nn

from ... import _lib

MAX_SOURCES = 4
_THRESH = 0.001      # compute_snr's default, which forward never overrides (snr.py:84,135)


class _ZeroRefSnr(torch.autograd.Function):
    """values [Bt] (individual) or loss = -mean(values) (scalar); the best permutations' indices ride along."""

    @staticmethod
    def forward(ctx, est, tgt, zero_mean, threshold_db, eps, individual):
        est_c = est.detach().to(torch.float32).contiguous()
        tgt_c = tgt.detach().to(torch.float32).contiguous()
        Bt, S, T = est_c.shape
        dev = est_c.device
        lib = _lib.load()
        with torch.cuda.device(dev):
            work = torch.empty(lib.srf_zeroref_snr_work_bytes(Bt, S, T), dtype=torch.uint8, device=dev)
            values = torch.empty(Bt, dtype=torch.float32, device=dev)
            perm = torch.empty(Bt, dtype=torch.int32, device=dev)
            loss = torch.empty(1, dtype=torch.float32, device=dev)
            rc = lib.srf_zeroref_snr_forward(_lib.ptr(est_c), _lib.ptr(tgt_c), Bt, S, T, 1 if zero_mean else 0,
                                             C.c_float(threshold_db), C.c_float(_THRESH), C.c_float(eps), _lib.ptr(work),
                                             _lib.ptr(values), _lib.ptr(perm), _lib.ptr(loss), _lib.current_stream(dev))
        _lib.check(rc, "srf_zeroref_snr_forward")
        ctx.save_for_backward(est_c, tgt_c, work)
        ctx.individual = individual
        ctx.in_dtype = est.dtype
        ctx.mark_non_differentiable(perm)
        return (values if individual else loss[0].clone()), perm

    @staticmethod
    def backward(ctx, grad_out, _grad_perm):
        est, tgt, work = ctx.saved_tensors
        Bt, S, T = est.shape
        up = grad_out.detach().to(torch.float32).reshape(Bt if ctx.individual else 1).contiguous()
        grad = torch.empty_like(est)
        with torch.cuda.device(est.device):
            rc = _lib.load().srf_zeroref_snr_backward(_lib.ptr(est), _lib.ptr(tgt), Bt, S, T, _lib.ptr(work), _lib.ptr(up),
                                                      1 if ctx.individual else 0, _lib.ptr(grad),
                                                      _lib.current_stream(est.device))
        _lib.check(rc, "srf_zeroref_snr_backward")
        return grad.to(ctx.in_dtype), None, None, None, None, None


class PermInvariantSNRwithZeroRefs(nn.Module):
    """SNR between reconstructed and target wavs with compensation for zero reference signals (losses/snr.py:13-142)."""

    def __init__(self, zero_mean=False, n_sources=None, backward_loss=True, inactivity_threshold=-40.,
                 return_individual_results=False):
        super().__init__()
        self.perform_zero_mean = zero_mean
        self.backward_loss = backward_loss
        self.permutations = list(itertools.permutations(torch.arange(n_sources)))
        self.permutations_tensor = torch.LongTensor(self.permutations)
        self.n_sources = n_sources
        self.inactivity_threshold = inactivity_threshold
        self.return_individual_results = return_individual_results

    def forward(self, pr_batch, t_batch, eps=1e-9, return_best_permutation=False):
        if pr_batch.dim() != 3 or t_batch.dim() != 3 or pr_batch.shape[:2] != t_batch.shape[:2]:
            raise RuntimeError("expected [batch, n_sources, time] estimates and targets, got %s and %s" %
                               (tuple(pr_batch.shape), tuple(t_batch.shape)))
        if pr_batch.shape[1] != self.n_sources:
            raise RuntimeError("constructed for %s sources, got %d" % (self.n_sources, pr_batch.shape[1]))
        if pr_batch.device.type != "cuda" or t_batch.device != pr_batch.device:
            raise _lib.SrfError("sudo_rm_rf_amd losses run on an MI355X only (estimates on %s, targets on %s); there "
                                "is deliberately no CPU fallback" % (pr_batch.device, t_batch.device))
        if self.n_sources > MAX_SOURCES:
            raise NotImplementedError("the HIP zero-reference SNR supports up to %d sources (FUSS's maximum), got %d" %
                                      (MAX_SOURCES, self.n_sources))
        if torch.is_grad_enabled() and t_batch.requires_grad:
            raise NotImplementedError("PermInvariantSNRwithZeroRefs on the HIP path has no gradient w.r.t. the targets")
        min_len = min(pr_batch.shape[-1], t_batch.shape[-1])              # normalize_input, snr.py:38-42
        pr, tg = pr_batch[:, :, :min_len], t_batch[:, :, :min_len]
        out, perm = _ZeroRefSnr.apply(pr, tg, bool(self.perform_zero_mean), float(self.inactivity_threshold), float(eps),
                                      bool(self.return_individual_results))
        # the kernel's scalar is -mean(values) and its vector is `values`: snr.py:111-116
        if self.return_individual_results:
            out = -out if self.backward_loss else out
        else:
            out = out if self.backward_loss else -out
        if return_best_permutation:
            return out, self.permutations_tensor[perm.long().cpu()]
        return out
