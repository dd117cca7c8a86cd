#!/usr/bin/env python3
"""Generate tests/golden/fuss_*.npz + FUSS_MANIFEST.json from the REAL reference (build container only): the FUSS recipe's
training loss, validation metric, augmentation and three steps of its training loop (experiments/run_fuss_separation.py).

Imports losses/snr.py, losses/sisdr.py, the two models and mixture_consistency.py from the reference by file path
(make_golden.load_ref_module); `online_augment` is defined inside the runner SCRIPT, which cannot be imported (it parses a
command line and opens an experiment at import), so its function definition alone is compiled from the script's syntax tree.
Inputs are regenerated from seeds by tests/fuss_fixtures.py; the files hold only what the reference returned.

Every loss / metric case is run by the reference in fp32 AND in fp64.  A case is accepted only if (asserted here, recorded in
the manifest) the reference's own fp32-vs-fp64 distance is at most HALF the bar the GPU test applies (loss and values 2e-5
relative, gradient 2e-5 of its largest entry, metric 2e-4 + 2e-5 |value| dB), and if in fp64 the best permutation is at
least 0.01 dB ahead of the best DIFFERENTLY VALUED one (permutation comparisons are exact).

    python tools/make_golden_fuss.py [--only loss,metric,augment,traj]
"""
import ast
import json
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden import REF, load_ref_module  # noqa: E402
from make_golden_train import sample  # noqa: E402
from oracle.weights import make_state_dict  # noqa: E402
from tests import fuss_fixtures as ff  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
GRAD_KEEP = 2000
MIN_GAP_DB = 0.01
SAMPLE = 2048


def gap_to_next_value(vals, best):
    """Smallest distance from the best value to a permutation value that is not (exactly) equal to it, per example."""
    gaps = []
    for v, b in zip(vals, best):
        other = v[v != b]
        gaps.append(float((b - other.max()).item()) if other.numel() else float("inf"))
    return gaps


def loss_cases(snr):
    man = {}
    for name, c in ff.LOSS_CASES.items():
        est_np, tgt_np = ff.make_loss_case(**c)
        res = {}
        for dt in (torch.float32, torch.float64):
            fn = snr.PermInvariantSNRwithZeroRefs(n_sources=c["n_src"], zero_mean=c["zero_mean"], backward_loss=True,
                                                  inactivity_threshold=-40., return_individual_results=True)
            est = torch.tensor(est_np, dtype=dt, requires_grad=True)
            vals, perms = fn(est, torch.tensor(tgt_np, dtype=dt), return_best_permutation=True)
            vals.mean().backward()              # = the runner's scalar loss (return_individual_results=False)
            res[dt] = (-vals.detach().double().numpy(), perms.numpy(), est.grad.double().numpy(), float(vals.detach().mean()))
        (v32, p32, g32, l32), (v64, p64, g64, l64) = res[torch.float32], res[torch.float64]
        assert (p32 == p64).all(), name
        # fp64 structure: gap of the best permutation, activity
        best, idx, active, allv = ff.zeroref_snr(torch.tensor(est_np), torch.tensor(tgt_np), c["zero_mean"])
        gaps = gap_to_next_value(allv, best)
        assert min(gaps) >= MIN_GAP_DB, (name, gaps)
        d_val = float(np.max(np.abs(v32 - v64) / np.maximum(1.0, np.abs(v64))))
        d_loss = abs(l32 - l64) / max(1.0, abs(l64))
        d_grad = float(np.abs(g32 - g64).max() / max(np.abs(g64).max(), 1e-300))
        assert d_val <= 1e-5 and d_loss <= 1e-5 and d_grad <= 1e-5, (name, d_val, d_loss, d_grad)
        perm_list = [list(map(int, p)) for p in __import__("itertools").permutations(range(c["n_src"]))]
        perm_index = np.array([perm_list.index(list(map(int, p))) for p in p32], np.int32)
        np.savez_compressed(os.path.join(OUT, name + ".npz"), loss=np.float32(l32), loss_fp64=np.float64(l64),
                            values=v32.astype(np.float32), values_fp64=v64, perms=p32.astype(np.int32), perm_index=perm_index,
                            grad_prefix=g32[..., :GRAD_KEEP].astype(np.float32), grad_sum=g32.sum(-1),
                            grad_sqsum=(g32 ** 2).sum(-1), grad_absmax=np.float64(np.abs(g32).max()))
        man[name] = dict(c, kind="loss", loss=l32, n_active=[int(a) for a in active.sum(-1)], perm_gap_db=gaps,
                         ref_fp32_vs_fp64=dict(values_rel=d_val, loss_rel=d_loss, grad_rel_to_max=d_grad))
        print(name, "loss %.6f" % l32, "active", man[name]["n_active"], "min gap %.3f dB" % min(gaps),
              "fp32-fp64: values %.1e loss %.1e grad %.1e" % (d_val, d_loss, d_grad), flush=True)
    return man


def metric_cases(sisdr):
    man = {}
    for name, c in ff.METRIC_CASES.items():
        pr_np, tgt_np = ff.make_metric_case(**c)
        res = {}
        for dt in (torch.float32, torch.float64):
            fn = sisdr.StabilizedPermInvSISDRMetric(zero_mean=True, single_source=False, n_estimated_sources=c["n_est"],
                                                    n_actual_sources=c["n_act"], backward_loss=False,
                                                    improvement=c["improvement"], return_individual_results=True)
            with torch.no_grad():
                v, p = fn(torch.tensor(pr_np, dtype=dt), torch.tensor(tgt_np, dtype=dt), return_best_permutation=True)
            res[dt] = (v.double().numpy(), p.numpy())
        (v32, p32), (v64, p64) = res[torch.float32], res[torch.float64]
        assert (p32 == p64).all(), name
        best, idx, allv = ff.stabilized_sisdr(torch.tensor(pr_np), torch.tensor(tgt_np), improvement=False)
        gaps = gap_to_next_value(allv, best)
        assert min(gaps) >= MIN_GAP_DB, (name, gaps)
        d = float(np.max(np.abs(v32 - v64) / (2e-4 + 2e-5 * np.abs(v64))))       # in units of the bar
        assert d <= 0.5, (name, d)
        np.savez_compressed(os.path.join(OUT, name + ".npz"), value=v32.astype(np.float32), value_fp64=v64,
                            perms=p32.astype(np.int32))
        man[name] = dict(c, kind="metric", values=[float(x) for x in v32], perm_gap_db=gaps,
                         ref_fp32_vs_fp64=dict(fraction_of_bar=d, abs_db=float(np.abs(v32 - v64).max())))
        print(name, v32, "min gap %.3f dB" % min(gaps), "fp32-fp64 %.2f of the bar" % d, flush=True)
    return man


def reference_online_augment():
    """The runner's `online_augment` function object, compiled from its definition in the script (nothing else of the script
    runs)."""
    path = os.path.join(REF, "sudo_rm_rf/dnn/experiments/run_fuss_separation.py")
    tree = ast.parse(open(path).read(), path)
    fdef = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "online_augment"]
    assert len(fdef) == 1
    ns = {"torch": torch}
    exec(compile(ast.Module(body=fdef, type_ignores=[]), path, "exec"), ns)
    return ns["online_augment"]


def augment_cases():
    aug = reference_online_augment()
    man = {}
    for name, c in ff.AUG_CASES.items():
        B, S = c["batch"], c["n_src"]
        # the draws, read off a coded input: row (b, i) = [1, code(b, i)] comes back as [gain, gain * code]
        code = torch.arange(1, B * S + 1, dtype=torch.float32).reshape(B, S)
        coded = torch.stack([torch.ones(B, S), code], -1)
        torch.manual_seed(c["seed"])
        got = aug(coded.clone())
        gain = got[..., 0]
        src = torch.round(got[..., 1] / gain).long() - 1                  # flat index b' * S + i of the row that arrived
        src_s = (src[0] % S)
        src_b = torch.zeros(S, B, dtype=torch.long)
        for k in range(S):
            assert ((src[:, k] % S) == src_s[k]).all()
            src_b[src_s[k]] = src[:, k] // S
        # ... and what the runner makes of a real batch under the same seed (:234-243)
        clean = torch.from_numpy(ff.make_clean(**c))
        torch.manual_seed(c["seed"])
        wavs = aug(clean.clone())
        mix = torch.sum(wavs, -2, keepdim=True)
        std, mean = mix.std(-1, keepdim=True), mix.mean(-1, keepdim=True)
        mixn = (mix - mean) / (std + 1e-9)
        mine = ff.augment(clean, src_b.numpy(), src_s.numpy(), gain.numpy(), dtype=torch.float32)
        assert torch.equal(mine[0], wavs), name                            # the decoded draws reproduce the reference's output
        np.savez_compressed(os.path.join(OUT, name + ".npz"), src_b=src_b.numpy().astype(np.int32),
                            src_s=src_s.numpy().astype(np.int32), gain=gain.numpy(), sources=wavs.numpy(), mixture=mixn.numpy(),
                            mean=mean.numpy(), std=std.numpy())
        man[name] = dict(c, kind="augment", src_s=[int(x) for x in src_s])
        print(name, "src_s", man[name]["src_s"], flush=True)
    return man


def run_traj(ref_model, ref_mc, loss_fn, cfg, sd, batches, dtype):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = ref_model(**cfg.ctor_kwargs())
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model.train()
    if dtype == torch.float64:
        model = model.double()
        model.pad_to_appropriate_length = lambda x: x      # (builds a float32 buffer whatever the input; T is a multiple)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    losses = []
    for clean, src_b, src_s, gain in batches:
        opt.zero_grad()
        # online_augment with the stored draws (float32 products, like the loader's float32 batch), then :237-243
        clean_wavs, _, _, _ = ff.augment(clean, src_b, src_s, gain, dtype=torch.float32)
        clean_wavs = clean_wavs.to(dtype)
        mix = torch.sum(clean_wavs, -2, keepdim=True)
        mix = (mix - mix.mean(-1, keepdim=True)) / (mix.std(-1, keepdim=True) + 1e-9)
        rec = ref_mc.apply(model(mix), mix)
        l = loss_fn(rec, clean_wavs)
        l.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 5.0)
        opt.step()
        losses.append(float(l.item()))
    return losses, {k: v.detach().numpy().astype(np.float64) for k, v in model.state_dict().items()}


def traj_cases(snr):
    ref_imp = load_ref_module("sudo_rm_rf/dnn/models/improved_sudormrf.py", "_ref_improved_sudormrf")
    ref_gc = load_ref_module("sudo_rm_rf/dnn/models/groupcomm_sudormrf_v2.py", "_ref_groupcomm_sudormrf_v2")
    ref_mc = load_ref_module("sudo_rm_rf/dnn/experiments/utils/mixture_consistency.py", "_ref_mixture_consistency")
    loss_fn = snr.PermInvariantSNRwithZeroRefs(n_sources=4, zero_mean=False, backward_loss=True, inactivity_threshold=-40.)
    man = {}
    for name, (cfg, batch, T, wseed, dseed) in ff.traj_configs().items():
        assert T % cfg.n_least_samples_req == 0 and cfg.num_sources == 4
        ref_model = ref_imp.SuDORMRF if cfg.variant == "improved" else ref_gc.GroupCommSudoRmRf
        sd = make_state_dict(cfg, wseed)
        batches = ff.make_traj_batches(batch, cfg.num_sources, T, dseed)
        l64, w64 = run_traj(ref_model, ref_mc, loss_fn, cfg, sd, batches, torch.float64)
        l32, w32 = run_traj(ref_model, ref_mc, loss_fn, cfg, sd, batches, torch.float32)
        arrays = {"losses": np.array(l64), "losses_fp32": np.array(l32)}
        for k, w in w64.items():
            w0 = sd[k].astype(np.float64)
            d64, d32 = w - w0, w32[k] - w0
            arrays["d:" + k] = np.float64(np.sqrt(((d32 - d64) ** 2).sum()) / max(np.sqrt((d64 ** 2).sum()), 1e-300))
            smp, step = sample(w, SAMPLE)
            arrays["w:" + k] = smp
            arrays["n:" + k] = np.array([step, float(np.sqrt((d64 ** 2).sum()))])
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **arrays)
        man[name] = dict(kind="traj", config=cfg.as_dict(), batch=batch, T=T, weight_seed=wseed, data_seed=dseed,
                         steps=ff.TRAJ_STEPS, losses=l64, losses_fp32=l32, reference_dtype="float64", lr=1e-3, clip_grad_norm=5.0)
        print(name, l64, l32, "worst fp32-vs-fp64 update deviation %.3g" % max(float(arrays[k]) for k in arrays if k.startswith("d:")),
              flush=True)
    return man


def main():
    only = set(sys.argv[sys.argv.index("--only") + 1].split(",")) if "--only" in sys.argv else {"loss", "metric", "augment", "traj"}
    snr = load_ref_module("sudo_rm_rf/dnn/losses/snr.py", "_ref_snr")
    sisdr = load_ref_module("sudo_rm_rf/dnn/losses/sisdr.py", "_ref_sisdr")
    mpath = os.path.join(OUT, "FUSS_MANIFEST.json")
    man = json.load(open(mpath)) if os.path.exists(mpath) else {}
    if "loss" in only:
        man.update(loss_cases(snr))
    if "metric" in only:
        man.update(metric_cases(sisdr))
    if "augment" in only:
        man.update(augment_cases())
    if "traj" in only:
        man.update(traj_cases(snr))
    json.dump(man, open(mpath, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
