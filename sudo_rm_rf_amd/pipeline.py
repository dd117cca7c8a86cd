"""The reference's caller-side inference recipe as one call.

README.md:100-114 (and experiments/simple_whamr_evaluation.py:142-148) wrap every model() call in the same
lines: per-example mean/std normalisation of the mixture, the forward, rescaling of the estimates with the
mixture's statistics and -- for the GroupComm models -- mixture consistency.  On a GPU those are 5-7 extra
passes over [batch, sources, time] tensors in separate ATen kernels; here they are folded INTO the forward
(srf_separate): one statistics kernel over the raw mixture, the normalisation in the encoder's operand load, the
rescale and the mixture consistency in the decoder's overlap-add.  The stand-alone kernels (srf_wav_normalize /
srf_wav_denormalize, ``ops``) remain for callers that need the normalised mixture itself."""
import torch

from . import ops, ragged


def separate(model, mixture, mixture_consistency=None):
    """mixture: float tensor [batch, time] or [batch, 1, time] on the model's MI355X.
    Returns the estimated sources [batch, num_sources, time] in the mixture's own scale.

    mixture_consistency: None = apply it exactly when the model is a GroupCommSudoRmRf (what the README
    prescribes for the pre-trained GroupComm models), True / False to force."""
    if mixture.dim() == 2:
        mixture = mixture.unsqueeze(1)
    if mixture.dim() != 3 or mixture.shape[1] != 1:
        raise RuntimeError("separate() expects [batch, time] or [batch, 1, time], got %s" % (tuple(mixture.shape),))
    if mixture_consistency is None:
        mixture_consistency = type(model).__name__ == "GroupCommSudoRmRf"
    x = mixture.detach().to(torch.float32).contiguous()
    with torch.no_grad():
        # srf_separate has no causal form (it refuses that variant): the causal model takes the three-kernel form below, as the
        # multi-channel front ends do -- before, a one-channel CausalSuDORMRF fell into the refusal
        if getattr(model, "in_audio_channels", 1) == 1 and hasattr(model, "_engine") and type(model).__name__ != "CausalSuDORMRF":
            return model._engine().separate(model, x, bool(mixture_consistency))
        norm, stats = ops.wav_normalize(x)          # (multi-channel front ends, the causal model: the three-kernel form)
        est = model(norm)
        return ops.wav_denormalize(est, stats, norm if mixture_consistency else None)


# ---- lists of utterances of unequal length ----------------------------------------------------------------------------------
BUCKET = 4000      # a batch's padded length is rounded up to a multiple of this many samples (0.5 s at 8 kHz): a folder of files
                   # then re-uses a handful of (batch, T) plans instead of making one per distinct longest member


def ragged_batches(lengths, max_batch=32, bucket=BUCKET):
    """The batching of separate_list as a pure function.  lengths: the utterances' lengths in samples.  Returns a list of
    (indices, T): utterances sorted by length (ties by index) and cut into runs of at most max_batch; T = the run's longest
    member rounded up to the bucket grid.  Every index appears exactly once; neighbours in length share a batch, so the padding
    a batch carries is small and the tiles past an example's end few."""
    if max_batch < 1 or bucket < 1:
        raise ValueError("max_batch and bucket must be positive")
    order = sorted(range(len(lengths)), key=lambda i: (int(lengths[i]), i))
    out = []
    for k in range(0, len(order), max_batch):
        idx = order[k:k + max_batch]
        longest = int(lengths[idx[-1]])
        out.append((idx, -(-longest // bucket) * bucket))
    return out


def ragged_route(model, length=None):
    """Where separate_list sends an utterance, decided from the model's configuration alone (no GPU): "ragged" = a candidate
    for the ragged batch (the Improved model with one input channel, K = 21, 256 bottleneck channels; the GroupComm model with
    one input channel, K = 21, 16 groups of 16 -> 32 channels, i.e. 256 / 512 channels; with `length`, also long enough for
    the fused pyramid to take it as an example of its own; the original model after enable_ragged(), see
    SuDORMRF._ragged_route), "single" = the per-example path (the causal model, other configurations, too-short utterances).
    A candidate batch still falls back as a whole when the plan of its (batch, T) is refused (srf_plan_ragged_supported,
    srf_original_ragged_supported: small shapes)."""
    kind = type(model).__name__
    if kind not in ("SuDORMRF", "GroupCommSudoRmRf") or not hasattr(model, "separate_ragged"):
        return "single"
    if hasattr(model, "_ragged_route"):      # the original / attentive v2 model after enable_ragged(): its own shapes and padding rule
        return model._ragged_route(length)
    if getattr(model, "enc_kernel_size", 0) != 21 or getattr(model, "out_channels", 0) != 256:
        return "single"
    if kind == "GroupCommSudoRmRf" and (model.in_audio_channels != 1 or model._group_size() != 16 or model.in_channels != 512):
        return "single"
    if length is not None:
        D = model.upsampling_depth
        n_req = (model.enc_kernel_size // 2) << D
        frames = max(n_req, -(-int(length) // n_req) * n_req) // (model.enc_kernel_size // 2)
        chunk = 16 if D <= 5 else 32
        if D > 6 or (frames >> (D - 1)) < 8 or frames % chunk or frames // chunk < 4:
            return "single"
    return "ragged"


def separate_list(model, mixtures, mixture_consistency=None, max_batch=32):
    """separate() over a list of utterances of unequal length: mixtures = tensors [T_i] or [1, T_i] on the model's MI355X;
    returns the estimates [num_sources, T_i] in the caller's order.  The README recipe per utterance (mean / std over its own
    samples, forward, rescale; mixture consistency as in separate()), with a length-sorted batch run as ONE gather launch
    (ragged.wav_gather) and ONE separate_ragged call of the Improved / the GroupComm model -- the recipe folded into the ragged
    forward as separate() folds it into the uniform one; the results are then views of that call's output -- where the model and
    the batch allow it, and through separate() one by one where they do not -- so the answer is always the per-utterance one."""
    mixes = []
    for m in mixtures:
        if m.dim() == 2 and m.shape[0] == 1:
            m = m[0]
        if m.dim() != 1 or m.numel() == 0:
            raise RuntimeError("separate_list() expects tensors [time] or [1, time], got %s" % (tuple(m.shape),))
        mixes.append(m.detach().to(torch.float32).contiguous())
    if mixture_consistency is None:
        mixture_consistency = type(model).__name__ == "GroupCommSudoRmRf"
    results = [None] * len(mixes)
    routes = [ragged_route(model, m.numel()) for m in mixes]
    single = [i for i, r in enumerate(routes) if r == "single"]
    cand = [i for i, r in enumerate(routes) if r != "single"]
    with torch.no_grad():
        for idx, T in ragged_batches([mixes[i].numel() for i in cand], max_batch):
            idx = [cand[j] for j in idx]
            dev = mixes[idx[0]].device
            if len(idx) < 2 or not model._engine().ragged_plan_supported(len(idx), T, dev):
                single.extend(idx)
                continue
            # the whole recipe of the batch on the device: one gather launch from the utterances' own buffers into the padded
            # batch, then statistics over each row's own samples, normalise-on-load, the ragged forward, rescale and mixture
            # consistency in ONE separate_ragged call; the results are views of its output
            x, lens = ragged.wav_gather([mixes[i] for i in idx], T)
            est, _ = model.separate_ragged(x, lens, mixture_consistency)
            for r, i in enumerate(idx):
                results[i] = est[r, :, :lens[r]]
        for i in single:
            results[i] = separate(model, mixes[i].unsqueeze(0), mixture_consistency)[0]
    return results
