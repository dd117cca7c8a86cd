#!/usr/bin/env python3
"""Generate the causal SuDoRM-RF (v3) TRAINING fixtures from the REAL reference (build host only).

Loads the unmodified reference modules by file path, as tools/make_golden_causal.py does, and stores
  tests/golden/causal_train_*.npz      gradients of the linear loss (model(x) * gout).sum() of tests/causal_train_ref.GRAD_CASES
                                      in the format of tools/make_golden_train.py: "g:" the reference's fp64 gradient (small
                                      tensors whole, large ones a strided sample), "n:" [stride, max |g|, sum g, sum g^2], "d:" the
                                      deviation of the reference's own fp32 backward from fp64, relative to max |g|
  tests/golden/causal_fuss_s4_traj.npz three steps of the FUSS loop body (experiments/run_fuss_separation.py, model_type
                                      'causal') in the format of the fuss_*_traj fixtures: losses, losses_fp32, "w:", "n:", "d:"
  tests/golden/CAUSAL_TRAIN_MANIFEST.json
The fp64 run replaces the reference's pad helper on the instance (it builds a float32 buffer whatever the input) by the same
zero padding in the input's dtype.  Asserted for every gradient case: the reference's fp32 gradients pass
check_grads_against_golden against its fp64 ones with the bars the GPU test applies.

    SRF_REFERENCE=<reference checkout> python tools/make_golden_causal_train.py
Regenerating is bit-identical.
"""
import importlib.util
import io
import json
import os
import sys
import warnings
import zipfile

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from tests import causal_fixtures as cf  # noqa: E402
from tests import causal_train_ref as ctr  # noqa: E402
from tests import fuss_fixtures as ff  # noqa: E402

REF = os.environ.get("SRF_REFERENCE", "")
SAMPLE = {"tiny": 2048, "default": 384}
TRAJ_SAMPLE = 2048


def load_ref(rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        spec.loader.exec_module(mod)
    return mod


def save_npz(path, arrays):
    """np.savez's layout with a fixed member timestamp (regenerating writes identical bytes); scalars stay 0-d."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_STORED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[k], order="C"), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


def sample(g, n):
    flat = g.reshape(-1)
    step = max(1, flat.size // n)
    return flat[::step][:n].copy(), step


def build(ref, cfg, sd, dtype):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(0)
        m = ref.CausalSuDORMRF(**cfg)
    assert [k for k, _ in cf.schema(cfg)] == list(m.state_dict())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m.train()
    if dtype == torch.float64:
        m = m.double()
        m.pad_to_appropriate_length = lambda x: F.pad(x, (0, ctr.padded_length(cfg, x.shape[-1]) - x.shape[-1]))
    return m


def grad_cases(ref):
    from test_oracle_golden import check_grads_against_golden
    man = {}
    for name, (cfg, batch, T, kind) in ctr.GRAD_CASES.items():
        _, sd, x, gout = ctr.grad_case(name)
        grads = {}
        for dtype in (torch.float64, torch.float32):
            m = build(ref, cfg, sd, dtype)
            out = m(torch.tensor(x, dtype=dtype))
            assert out.dtype == dtype
            (out * gout.to(dtype)).sum().backward()
            grads[dtype] = {k: p.grad.double().numpy() for k, p in m.state_dict(keep_vars=True).items()}
        arrays, worst = {}, 0.0
        for k, g in grads[torch.float64].items():
            gmax = float(np.abs(g).max())
            d = float(np.abs(grads[torch.float32][k] - g).max() / max(gmax, 1e-300))
            worst = max(worst, d)
            arrays["d:" + k] = np.float64(d)
            smp, step = sample(g, SAMPLE[kind])
            arrays["g:" + k] = smp.astype(np.float32)
            arrays["n:" + k] = np.array([step, gmax, float(g.sum()), float((g ** 2).sum())])
        save_npz(os.path.join(cf.GOLDEN, name + ".npz"), arrays)
        z = np.load(os.path.join(cf.GOLDEN, name + ".npz"))
        tol, yard, flips = ctr.GRAD_BARS[kind]
        check_grads_against_golden(list(grads[torch.float32].items()), z, tol, fp32_yardstick=yard, flip_budget=flips)
        man[name] = dict(kind="grad", bars=kind, config=cfg, batch=batch, T=T, weight_seed=ctr.WEIGHT_SEED, input_seed=ctr.INPUT_SEED,
                         gout_seed=ctr.GOUT_SEED, reference_dtype="float64", ref_fp32_vs_fp64_worst=worst)
        print("%-26s reference fp32 vs fp64: worst %.2e of a tensor's largest entry" % (name, worst), flush=True)
    return man


def run_traj(ref, ref_mc, loss_fn, cfg, sd, batches, dtype):
    model = build(ref, cfg, sd, dtype)
    opt = torch.optim.Adam(model.parameters(), lr=ctr.TRAJ_LR)
    losses = []
    for clean, src_b, src_s, gain in batches:
        opt.zero_grad()
        clean_wavs, _, _, _ = ff.augment(clean, src_b, src_s, gain, dtype=torch.float32)
        clean_wavs = clean_wavs.to(dtype)
        mix = torch.sum(clean_wavs, -2, keepdim=True)
        mix = (mix - mix.mean(-1, keepdim=True)) / (mix.std(-1, keepdim=True) + 1e-9)
        rec = ref_mc.apply(model(mix), mix)
        l = loss_fn(rec, clean_wavs)
        l.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), ctr.TRAJ_CLIP)
        opt.step()
        losses.append(float(l.item()))
    return losses, {k: v.detach().numpy().astype(np.float64) for k, v in model.state_dict().items()}


def traj_cases(ref):
    ref_mc = load_ref("sudo_rm_rf/dnn/experiments/utils/mixture_consistency.py", "_ref_mixture_consistency")
    snr = load_ref("sudo_rm_rf/dnn/losses/snr.py", "_ref_snr")
    man = {}
    for name, (cfg, batch, T, wseed, dseed) in ctr.TRAJ_CASES.items():
        S = cfg["num_sources"] * cfg["in_audio_channels"]
        loss_fn = snr.PermInvariantSNRwithZeroRefs(n_sources=S, zero_mean=False, backward_loss=True, inactivity_threshold=-40.)
        sd = cf.make_state_dict(cfg, wseed)
        batches = ff.make_traj_batches(batch, S, T, dseed)
        l64, w64 = run_traj(ref, ref_mc, loss_fn, cfg, sd, batches, torch.float64)
        l32, w32 = run_traj(ref, ref_mc, loss_fn, cfg, sd, batches, torch.float32)
        assert np.isfinite(l64).all() and np.isfinite(l32).all(), (l64, l32)
        arrays = {"losses": np.array(l64), "losses_fp32": np.array(l32)}
        for k, w in w64.items():
            w0 = sd[k].astype(np.float64)
            d64, d32 = w - w0, w32[k] - w0
            arrays["d:" + k] = np.float64(np.sqrt(((d32 - d64) ** 2).sum()) / max(np.sqrt((d64 ** 2).sum()), 1e-300))
            smp, step = sample(w, TRAJ_SAMPLE)
            arrays["w:" + k] = smp
            arrays["n:" + k] = np.array([step, float(np.sqrt((d64 ** 2).sum()))])
        save_npz(os.path.join(cf.GOLDEN, name + ".npz"), arrays)
        man[name] = dict(kind="traj", config=cfg, batch=batch, T=T, weight_seed=wseed, data_seed=dseed, steps=ff.TRAJ_STEPS,
                         losses=l64, losses_fp32=l32, reference_dtype="float64", lr=ctr.TRAJ_LR, clip_grad_norm=ctr.TRAJ_CLIP)
        print(name, l64, l32, "worst fp32-vs-fp64 update deviation %.3g" % max(float(arrays[k]) for k in arrays if k.startswith("d:")),
              flush=True)
    return man


def main():
    if not REF or not os.path.isdir(REF):
        raise SystemExit("set SRF_REFERENCE to a checkout of the reference implementation")
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    ref = load_ref("sudo_rm_rf/dnn/models/causal_improved_sudormrf_v3.py", "_ref_causal_improved_sudormrf_v3")
    man = {"generator": "tools/make_golden_causal_train.py", "cases": {}}
    man["cases"].update(grad_cases(ref))
    man["cases"].update(traj_cases(ref))
    with open(ctr.MANIFEST, "w") as f:
        json.dump(man, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", ctr.MANIFEST)


if __name__ == "__main__":
    main()
