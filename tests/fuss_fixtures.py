"""Seeded inputs and the fp64 torch restatement of the FUSS recipe's loss, metric and augmentation
(experiments/run_fuss_separation.py), shared by tools/make_golden_fuss.py (which runs the REFERENCE classes on these inputs
and stores what they return in tests/golden/fuss_*.npz) and by tests/test_fuss_host.py / tests/test_gpu_fuss.py (which
regenerate the inputs and compare).  No file here depends on the reference."""
import itertools
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
THRESH = 0.001      # compute_snr's default (snr.py:84)


def manifest():
    with open(os.path.join(GOLDEN, "FUSS_MANIFEST.json")) as f:
        return json.load(f)


def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


# ---------------------------------------------------------------------------------------------
# loss cases.  name: dict(batch, n_src, T, seed, zero_mean, silent = per example the number of exact-zero targets,
#   snr_db = level of the estimates' error, edge = per example (dB relative to the mixture) level of the LAST non-silent
#   target or None, order = "id" | "rev": how the estimates that belong to silent targets are laid out)
# ---------------------------------------------------------------------------------------------
LOSS_CASES = {
    "fuss_loss_all_active": dict(batch=3, n_src=4, T=4000, seed=1, zero_mean=False, silent=[0, 0, 0], snr_db=6.0),
    "fuss_loss_silent_mix": dict(batch=4, n_src=4, T=3001, seed=2, zero_mean=False, silent=[1, 2, 3, 4], snr_db=4.0),
    "fuss_loss_silent_mix_zm": dict(batch=4, n_src=4, T=2048, seed=3, zero_mean=True, silent=[3, 1, 4, 2], snr_db=8.0),
    "fuss_loss_threshold": dict(batch=2, n_src=4, T=4000, seed=4, zero_mean=False, silent=[0, 0], snr_db=5.0,
                                edge=[-40.5, -39.5]),
    "fuss_loss_near_exact": dict(batch=2, n_src=4, T=4000, seed=5, zero_mean=False, silent=[0, 1], snr_db=80.0),
    "fuss_loss_tie": dict(batch=3, n_src=4, T=1000, seed=6, zero_mean=False, silent=[2, 2, 3], snr_db=7.0, order="rev"),
    "fuss_loss_s3": dict(batch=3, n_src=3, T=1501, seed=7, zero_mean=True, silent=[0, 1, 2], snr_db=3.0),
    "fuss_loss_s2": dict(batch=4, n_src=2, T=800, seed=8, zero_mean=False, silent=[0, 1, 0, 2], snr_db=10.0),
    "fuss_loss_s1": dict(batch=3, n_src=1, T=515, seed=9, zero_mean=False, silent=[0, 1, 0], snr_db=12.0),
    "fuss_loss_recipe_len": dict(batch=2, n_src=4, T=160000, seed=10, zero_mean=False, silent=[1, 0], snr_db=9.0),
}


def make_loss_case(batch, n_src, T, seed, silent, snr_db, edge=None, order="id", **_):
    """(est, tgt) float32 [batch, n_src, T].  Targets: white noise at per-source levels with a DC offset, `silent[b]` of them
    (chosen by the seed) exactly zero.  Estimates: the targets in a seeded order plus white noise `snr_db` below every active
    target; the estimates that go with silent targets are low-level noise.  order = "rev": those are laid out so that the
    matching permutation which keeps them in ASCENDING order is not the one the data suggests -- all their arrangements tie."""
    rng = np.random.default_rng(1000 + seed)
    est = np.zeros((batch, n_src, T), np.float64)
    tgt = np.zeros((batch, n_src, T), np.float64)
    for b in range(batch):
        level = rng.uniform(0.2, 1.0, n_src)
        t = rng.standard_normal((n_src, T)) * level[:, None] + rng.uniform(-0.05, 0.05, n_src)[:, None]
        dead = rng.permutation(n_src)[:silent[b]]
        t[dead] = 0.0
        live = [j for j in range(n_src) if j not in set(dead.tolist())]
        if edge is not None and edge[b] is not None and len(live) > 1:
            j = live[-1]
            others = t[[k for k in live if k != j]].sum(0)
            scale = 1.0
            for _it in range(30):      # level of target j relative to the WHOLE mixture (which contains it)
                ratio = 10 * np.log10((t[j] ** 2).sum() * scale ** 2 / (((others + scale * t[j]) ** 2).sum()))
                scale *= 10 ** ((edge[b] - ratio) / 20)
            t[j] *= scale
        perm = rng.permutation(n_src)               # estimate perm[j] belongs to target j
        if order == "rev":
            slots = sorted(perm[dead].tolist(), reverse=True)
            for j, s_ in zip(sorted(dead.tolist()), slots):
                perm[j] = s_
        for j in range(n_src):
            p = float((t[j] ** 2).mean())
            sigma = np.sqrt(p) * 10 ** (-snr_db / 20) if p > 0 else 0.01
            est[b, perm[j]] = t[j] + sigma * rng.standard_normal(T)
        tgt[b] = t
    return est.astype(np.float32), tgt.astype(np.float32)


def zeroref_snr(est, tgt, zero_mean=False, threshold_db=-40.0, eps=1e-9, thresh=THRESH):
    """fp64 restatement of PermInvariantSNRwithZeroRefs (snr.py:38-116) on torch tensors [B,S,T]: (values [B], index of the
    best permutation [B], activity mask [B,S]); differentiable w.r.t. est.  value_b = max_perm n_act sum_j term(perm(j), j)."""
    est, tgt = est.double(), tgt.double()
    n = min(est.shape[-1], tgt.shape[-1])
    est, tgt = est[..., :n], tgt[..., :n]
    if zero_mean:
        est = est - est.mean(-1, keepdim=True)
        tgt = tgt - tgt.mean(-1, keepdim=True)
    S = tgt.shape[1]
    M = (tgt.sum(1) ** 2).sum(-1, keepdim=True)                    # [B,1]
    P = (tgt ** 2).sum(-1)                                          # [B,S]
    active = 10.0 * torch.log10(P / (M + eps)) >= threshold_db
    n_act = active.sum(-1)
    stab = thresh * torch.where(active, P, M.expand_as(P))
    D = ((est[:, :, None, :] - tgt[:, None, :, :]) ** 2).sum(-1)   # [B, i, j]
    term = 10.0 * active[:, None, :] * torch.log10((P + eps)[:, None, :] / (D + stab[:, None, :] + eps) + eps)
    perms = list(itertools.permutations(range(S)))
    vals = []
    for p in perms:
        v = term[:, p[0], 0]
        for j in range(1, S):
            v = v + term[:, p[j], j]
        vals.append(v * n_act)
    vals = torch.stack(vals, -1)
    best, idx = torch.max(vals, -1)
    return best, idx, active, vals


def zeroref_loss_and_grad(est_np, tgt_np, zero_mean=False, upstream=None, **kw):
    """(values [B], perm index [B], active [B,S], gradient of sum_b upstream[b] * values[b] w.r.t. est) in fp64."""
    est = torch.tensor(est_np, dtype=torch.float64, requires_grad=True)
    best, idx, active, _ = zeroref_snr(est, torch.tensor(tgt_np, dtype=torch.float64), zero_mean, **kw)
    up = torch.ones_like(best) if upstream is None else torch.as_tensor(upstream, dtype=torch.float64)
    (best * up).sum().backward()
    return best.detach().numpy(), idx.numpy(), active.numpy(), est.grad.numpy()


# ---------------------------------------------------------------------------------------------
# metric cases: every (n_est, n_act) with 1 <= n_act <= n_est <= 4; improvement = n_act > 1 and single_source = False as
# run_fuss_separation.py:110-131 sets them; zero_mean=True, backward_loss=False, return_individual_results=True
# ---------------------------------------------------------------------------------------------
METRIC_CASES = {
    "fuss_metric_e%d_a%d" % (ne, na): dict(batch=3, n_est=ne, n_act=na, T=2000 + 37 * ne + 4 * na, seed=20 + 4 * ne + na,
                                           snr_db=[2.0, 9.0, 15.0], improvement=na > 1)
    for ne in range(1, 5) for na in range(1, ne + 1)
}


def make_metric_case(batch, n_est, n_act, T, seed, snr_db, **_):
    """(pr [batch, n_est, T], tgt [batch, n_act, T]) float32: n_act of the estimates are targets plus noise at snr_db[b], the
    others unrelated noise, in a seeded order."""
    rng = np.random.default_rng(2000 + seed)
    pr = np.zeros((batch, n_est, T))
    tgt = np.zeros((batch, n_act, T))
    for b in range(batch):
        t = rng.standard_normal((n_act, T)) * rng.uniform(0.3, 1.0, n_act)[:, None] + rng.uniform(-0.1, 0.1, n_act)[:, None]
        slot = rng.permutation(n_est)
        pr[b] = 0.3 * rng.standard_normal((n_est, T))
        for j in range(n_act):
            sigma = t[j].std() * 10 ** (-(snr_db[b % len(snr_db)] + 1.5 * j) / 20)
            pr[b, slot[j]] = rng.uniform(0.5, 2.0) * t[j] + sigma * rng.standard_normal(T) + 0.02
        tgt[b] = t
    return pr.astype(np.float32), tgt.astype(np.float32)


def stabilized_sisdr(pr, tgt, zero_mean=True, single_source=False, improvement=False, eps=1e-9):
    """fp64 restatement of StabilizedPermInvSISDRMetric.forward (sisdr.py:497-576) with backward_loss=False and
    return_individual_results=True: (values [B], index [B] into itertools.permutations(range(n_est), r=n_act), all values)."""
    pr, tgt = pr.double(), tgt.double()
    if single_source:
        pr = pr.sum(-2, keepdim=True)
    if zero_mean:
        pr = pr - pr.mean(-1, keepdim=True)
        tgt = tgt - tgt.mean(-1, keepdim=True)
    n_est, n_act = pr.shape[1], tgt.shape[1]
    tt = (tgt ** 2).sum(-1)                                         # [B, j]

    def value(p, t, t_pow):
        rho = (p * t).sum(-1) ** 2 / ((p ** 2).sum(-1) * t_pow + eps)
        return 10.0 * torch.log10((rho + eps) / (1.0 - rho + eps))

    perms = list(itertools.permutations(range(n_est), r=n_act))
    allv = torch.stack([value(pr[:, list(p), :], tgt, tt).mean(-1) for p in perms], -1)
    best, idx = torch.max(allv, -1)
    if improvement:
        mix = tgt.sum(-2, keepdim=True)
        if zero_mean:
            mix = mix - mix.mean(-1, keepdim=True)
        best = best - value(mix.expand_as(tgt), tgt, tt).mean()
    return best, idx, allv


# ---------------------------------------------------------------------------------------------
# augmentation
# ---------------------------------------------------------------------------------------------
AUG_CASES = {"fuss_augment_b5_s4": dict(batch=5, n_src=4, T=515, seed=31),
             "fuss_augment_b3_s3": dict(batch=3, n_src=3, T=1024, seed=32)}


def make_clean(batch, n_src, T, seed, **_):
    rng = np.random.default_rng(3000 + seed)
    x = rng.standard_normal((batch, n_src, T)) * rng.uniform(0.1, 1.0, (batch, n_src, 1)) + rng.uniform(-0.1, 0.1, (batch, n_src, 1))
    x[rng.uniform(size=(batch, n_src)) < 0.25] = 0.0            # FUSS: some sources are silent
    return x.astype(np.float32)


def augment(clean, src_b, src_s, gain, eps=1e-9, dtype=torch.float64):
    """Restatement of online_augment (run_fuss_separation.py:195-215) with the draws given, plus the loop's mixture
    normalisation (:237-243): (sources [B,S,T], mixture [B,1,T], mean, std [B,1,1]).  The gain multiplies in the INPUT's
    precision (one float32 product in the reference), everything after it in `dtype`."""
    clean = torch.as_tensor(clean)
    S = clean.shape[1]
    aug = torch.stack([clean[torch.as_tensor(src_b[i]).long(), i] for i in range(S)], 1)
    aug = aug[:, torch.as_tensor(src_s).long()]
    aug = aug * torch.as_tensor(gain).to(clean.dtype).unsqueeze(-1)
    mix = aug.to(dtype).sum(-2, keepdim=True)
    std, mean = mix.std(-1, keepdim=True), mix.mean(-1, keepdim=True)
    return aug, (mix - mean) / (std + eps), mean, std


# ---------------------------------------------------------------------------------------------
# three steps of the FUSS loop (:232-265) at 4 sources
# ---------------------------------------------------------------------------------------------
TRAJ_STEPS = 3


def traj_configs():
    from oracle.schema import ModelConfig
    # name: (config, batch, T, weight seed, first data seed); T a multiple of n_least_samples_req (fp64 reference run)
    return {
        "fuss_improved_s4_traj": (ModelConfig("improved", 64, 128, 2, 4, 21, 64, 4), 2, 2400, 402, 502),
        "fuss_groupcomm_s4_traj": (ModelConfig("groupcomm", 32, 64, 2, 3, 21, 24, 4, 1, 4), 2, 800, 403, 513),
    }


def make_traj_batches(batch, n_src, T, seed):
    """[(clean [B,S,T] float32, src_b [S,B], src_s [S], gain [B,S])] per step: the loader's batch and FIXED augmentation draws."""
    out = []
    for s_ in range(TRAJ_STEPS):
        rng = np.random.default_rng(4000 + seed + s_)
        clean = make_clean(batch, n_src, T, 400 + seed + s_)
        src_b = np.stack([rng.permutation(batch) for _ in range(n_src)])
        src_s = rng.permutation(n_src)
        gain = (rng.uniform(size=(batch, n_src)) + 0.5).astype(np.float32)
        out.append((clean, src_b, src_s, gain))
    return out
