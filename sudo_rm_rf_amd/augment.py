"""On-GPU online remix augmentation: the lines the reference's training loops run right
before the forward (experiments/run_improved_sudormrf.py:150-164; run_fuss_separation.py:195-215 generalises them to
n sources), as three small HIP kernels instead of ~25 ATen ops; and the FUSS runner's own variant of those lines
(``fuss_online_augment``: no energy matching, random gains, only the mixture is normalised)."""
import torch

from . import _lib


def online_remix(clean_wavs, eps=1e-8):
    """clean_wavs: [batch, n_sources, time] float32 on the MI355X -> (mixtures [batch, time], sources [batch,
    n_sources, time]), both normalised per row exactly like the runner's normalize_tensor_wav (:127-131).

    Random numbers: one ``torch.randperm(n_sources)`` followed by one ``torch.randperm(batch)`` per source, from
    torch's default CPU generator -- the same calls, in the same order, as the runner makes, so a seeded run draws
    the same permutations."""
    if clean_wavs.dim() != 3:
        raise RuntimeError("expected [batch, n_sources, time], got %s" % (tuple(clean_wavs.shape),))
    if clean_wavs.device.type != "cuda":
        raise _lib.SrfError("sudo_rm_rf_amd.augment runs on an MI355X only (input on %s)" % clean_wavs.device)
    B, S, T = clean_wavs.shape
    x = clean_wavs.detach().to(torch.float32).contiguous()
    dev = x.device
    src_s = torch.randperm(S)
    src_b = torch.stack([torch.randperm(B) for _ in range(S)])
    src_s_d = src_s.to(torch.int32).to(dev)
    src_b_d = src_b.to(torch.int32).to(dev).contiguous()
    lib = _lib.load()
    mix = torch.empty((B, T), dtype=torch.float32, device=dev)
    out = torch.empty_like(x)
    scratch = torch.empty(lib.srf_online_remix_scratch_bytes(B, S), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = lib.srf_online_remix(_lib.ptr(x), _lib.ptr(src_b_d), _lib.ptr(src_s_d), B, S, T, float(eps), _lib.ptr(mix),
                                  _lib.ptr(out), _lib.ptr(scratch), _lib.current_stream(dev))
    _lib.check(rc, "srf_online_remix")
    return mix, out


def fuss_online_augment(clean_sources, eps=1e-9):
    """The FUSS runner's ``online_augment`` (experiments/run_fuss_separation.py:195-215) and the mixture normalisation its loop
    applies right after (:237-243).  clean_sources: [batch, n_sources, time] float32 on the MI355X, n_sources <= 4 ->
    (sources [B,S,T], mixture [B,1,T], mean [B,1,1], std [B,1,1]): new source i of example b = clean[perm_i[b], i], then the
    source axis permuted, then every row times its gain in [0.5, 1.5); mixture = (m - mean) / (std + eps) of m = the sum over
    sources, std unbiased.

    Random numbers: ``torch.randperm(batch)`` per source, ``torch.randperm(n_sources)``, ``torch.rand(batch, n_sources)`` from
    torch's default CPU generator -- the same calls in the same order as the runner makes, so a seeded run draws what it
    draws.  The index and gain tables are the only host-to-device traffic."""
    if clean_sources.dim() != 3:
        raise RuntimeError("expected [batch, n_sources, time], got %s" % (tuple(clean_sources.shape),))
    if clean_sources.device.type != "cuda":
        raise _lib.SrfError("sudo_rm_rf_amd.augment runs on an MI355X only (input on %s)" % clean_sources.device)
    B, S, T = clean_sources.shape
    return fuss_augment_with_draws(clean_sources, *fuss_draws(B, S), eps=eps)


def fuss_draws(batch, n_sources):
    """The random numbers of one ``online_augment`` call, drawn as run_fuss_separation.py:207-213 draws them: (src_b [S, B],
    src_s [S], gain [B, S])."""
    src_b = torch.stack([torch.randperm(batch) for _ in range(n_sources)])
    src_s = torch.randperm(n_sources)
    gain = torch.rand(batch, n_sources) + 0.5
    return src_b, src_s, gain


def fuss_augment_with_draws(clean_sources, src_b, src_s, gain, eps=1e-9):
    """``fuss_online_augment`` with the random draws given: src_b [S, B] (the batch permutation of every source), src_s [S]
    (the permutation of the source axis), gain [B, S] (applied after both)."""
    B, S, T = clean_sources.shape
    x = clean_sources.detach().to(torch.float32).contiguous()
    dev = x.device
    src_b_d = src_b.to(torch.int32).contiguous().to(dev)
    src_s_d = src_s.to(torch.int32).contiguous().to(dev)
    gain_d = gain.to(torch.float32).contiguous().to(dev)
    lib = _lib.load()
    out = torch.empty_like(x)
    mix = torch.empty((B, 1, T), dtype=torch.float32, device=dev)
    stats = torch.empty((B, 2), dtype=torch.float32, device=dev)
    scratch = torch.empty(lib.srf_fuss_augment_scratch_bytes(B, T), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = lib.srf_fuss_augment(_lib.ptr(x), _lib.ptr(src_b_d), _lib.ptr(src_s_d), _lib.ptr(gain_d), B, S, T, float(eps),
                                  _lib.ptr(out), _lib.ptr(mix), _lib.ptr(stats), _lib.ptr(scratch), _lib.current_stream(dev))
    _lib.check(rc, "srf_fuss_augment")
    return out, mix, stats[:, 0].reshape(B, 1, 1), stats[:, 1].reshape(B, 1, 1)
