#!/usr/bin/env python3
"""Generate the original SuDoRM-RF TRAINING fixtures from the REAL reference (build host only).

Loads the unmodified reference modules by file path, as tools/make_golden_original.py does, and stores
  tests/golden/orig_train_*.npz        gradients of the linear loss (model(x) * gout).sum() of tests/original_train_ref.GRAD_CASES
                                       in the format of tools/make_golden_train.py: "g:" the reference's fp64 gradient (small
                                       tensors whole, large ones a strided sample), "n:" [stride, max |g|, sum g, sum g^2], "d:" the
                                       deviation of the reference's own fp32 backward from fp64, relative to max |g|.  ln_mask_in.*
                                       has no entries: the reference's forward never reads it and its .grad stays None (asserted)
  tests/golden/orig_train_traj.npz     three steps of run_sudormrf.py's loop body -- PermInvariantSISDR(zero_mean=True,
                                       backward_loss=True, improvement=True) with initial_mixtures, clip_grad_norm_, Adam -- in
                                       the format of tools/make_golden_traj.py: losses, losses_fp32, "w:", "n:", "d:"
  tests/golden/ORIGINAL_TRAIN_MANIFEST.json
The fp64 run replaces the reference's pad helper on the instance (it builds a float32 buffer whatever the input) by the same
zero padding in the input's dtype.  Asserted for every gradient case: the reference's fp32 gradients pass
check_grads_against_golden against its fp64 ones with the bars the GPU test applies (a case that does not: change its seed, not
the bar).

    SRF_REFERENCE=<reference checkout> python tools/make_golden_original_train.py
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
from tests import original_fixtures as of  # noqa: E402
from tests import original_train_ref as otr  # noqa: E402

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
    torch.manual_seed(0)
    m = ref.SuDORMRF(**cfg)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == of.schema(cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m.train()
    if dtype == torch.float64:
        m = m.double()
        m.pad_to_appropriate_length = lambda x: F.pad(x, (0, of.padded_length(cfg, x.shape[-1]) - x.shape[-1]))
    return m


def grad_cases(ref):
    from test_oracle_golden import check_grads_against_golden
    man = {}
    for name, (cfg, batch, T, kind) in otr.GRAD_CASES.items():
        _, sd, x, gout = otr.grad_case(name)
        grads = {}
        for dtype in (torch.float64, torch.float32):
            m = build(ref, cfg, sd, dtype)
            out = m(torch.tensor(x, dtype=dtype))
            assert out.dtype == dtype and tuple(out.shape) == (batch, cfg["num_sources"], T)
            (out * gout.to(dtype)).sum().backward()
            named = m.state_dict(keep_vars=True)
            assert [k for k, p in named.items() if p.grad is None] == list(otr.NO_GRAD), name
            grads[dtype] = {k: p.grad.double().numpy() for k, p in named.items() if p.grad is not None}
        arrays, worst = {}, 0.0
        for k, g in grads[torch.float64].items():
            gmax = float(np.abs(g).max())
            d = float(np.abs(grads[torch.float32][k] - g).max() / max(gmax, 1e-300))
            worst = max(worst, d)
            arrays["d:" + k] = np.float64(d)
            smp, step = sample(g, SAMPLE[kind])
            arrays["g:" + k] = smp.astype(np.float32)
            arrays["n:" + k] = np.array([step, gmax, float(g.sum()), float((g ** 2).sum())])
        path = os.path.join(of.GOLDEN, name + ".npz")
        save_npz(path, arrays)
        assert os.path.getsize(path) <= (1 << 20), name
        z = np.load(path)
        tol, yard, flips = otr.GRAD_BARS[kind]
        check_grads_against_golden(list(grads[torch.float32].items()), z, tol, fp32_yardstick=yard, flip_budget=flips)
        man[name] = dict(kind="grad", bars=kind, config=cfg, batch=batch, T=T, weight_seed=otr.WEIGHT_SEED, input_seed=otr.INPUT_SEED,
                         gout_seed=otr.GOUT_SEED, reference_dtype="float64", ref_fp32_vs_fp64_worst=worst, frames=of.frames(cfg, T),
                         schema=[[k, list(s)] for k, s in of.schema(cfg)], no_grad=list(otr.NO_GRAD))
        print("%-24s reference fp32 vs fp64: worst %.2e of a tensor's largest entry" % (name, worst), flush=True)
    return man


def run_traj(ref, loss_fn, cfg, sd, batches, dtype):
    model = build(ref, cfg, sd, dtype)
    opt = torch.optim.Adam(model.parameters(), lr=otr.TRAJ_LR)
    losses = []
    for mix, clean in batches:
        opt.zero_grad()
        m1wavs, clean_wavs = mix.to(dtype), clean.to(dtype)
        rec_sources_wavs = model(m1wavs)
        l = loss_fn(rec_sources_wavs, clean_wavs, initial_mixtures=m1wavs)
        l.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), otr.TRAJ_CLIP)
        opt.step()
        losses.append(float(l.item()))
    return losses, {k: v.detach().numpy().astype(np.float64) for k, v in model.state_dict().items()}


def traj_cases(ref):
    sisdr = load_ref("sudo_rm_rf/dnn/losses/sisdr.py", "_ref_sisdr")
    man = {}
    for name, (cfg, batch, T, wseed, dseed) in otr.TRAJ_CASES.items():
        S = cfg["num_sources"]
        loss_fn = sisdr.PermInvariantSISDR(batch_size=batch, n_sources=S, zero_mean=True, backward_loss=True, improvement=True)
        sd = of.make_state_dict(cfg, wseed)
        batches = otr.make_traj_batches(batch, S, T, dseed)
        l64, w64 = run_traj(ref, loss_fn, cfg, sd, batches, torch.float64)
        l32, w32 = run_traj(ref, loss_fn, cfg, sd, batches, torch.float32)
        assert np.isfinite(l64).all() and np.isfinite(l32).all(), (l64, l32)
        assert l64[0] <= otr.TRAJ_MAX_FIRST_LOSS, (name, l64)          # (the conditioning the bars assume: original_train_ref.py)
        arrays = {"losses": np.array(l64), "losses_fp32": np.array(l32)}
        for k, w in w64.items():
            w0 = sd[k].astype(np.float64)
            d64, d32 = w - w0, w32[k] - w0
            arrays["d:" + k] = np.float64(np.sqrt(((d32 - d64) ** 2).sum()) / max(np.sqrt((d64 ** 2).sum()), 1e-300))
            smp, step = sample(w, TRAJ_SAMPLE)
            arrays["w:" + k] = smp
            arrays["n:" + k] = np.array([step, float(np.sqrt((d64 ** 2).sum()))])
        for k in otr.NO_GRAD:
            assert np.array_equal(w64[k], sd[k].astype(np.float64)), k      # (no gradient: Adam leaves them alone)
        save_npz(os.path.join(of.GOLDEN, name + ".npz"), arrays)
        # the reference's own fp32 trajectory passes the check the GPU test applies, decoder.bias (zero gradient: pure noise) aside
        from test_oracle_golden import check_trajectory_against_golden
        z = np.load(os.path.join(of.GOLDEN, name + ".npz"))
        check_trajectory_against_golden([(k, w) for k, w in w32.items() if k not in otr.TRAJ_NOISE_ONLY], sd, l32, z, otr.TRAJ_TOL)
        man[name] = dict(kind="traj", config=cfg, batch=batch, T=T, weight_seed=wseed, data_seed=dseed, steps=otr.TRAJ_STEPS,
                         losses=l64, losses_fp32=l32, reference_dtype="float64", lr=otr.TRAJ_LR, clip_grad_norm=otr.TRAJ_CLIP,
                         schema=[[k, list(s)] for k, s in of.schema(cfg)])
        print(name, l64, l32, "worst fp32-vs-fp64 update deviation %.3g" % max(float(arrays[k]) for k in arrays if k.startswith("d:")),
              flush=True)
    return man


def main():
    if not REF or not os.path.isdir(REF):
        raise SystemExit("set SRF_REFERENCE to a checkout of the reference implementation")
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    ref = load_ref("sudo_rm_rf/dnn/models/sudormrf.py", "_ref_sudormrf")
    man = {"generator": "tools/make_golden_original_train.py", "torch": torch.__version__, "cases": {}}
    man["cases"].update(grad_cases(ref))
    man["cases"].update(traj_cases(ref))
    with open(otr.MANIFEST, "w") as f:
        json.dump(man, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", otr.MANIFEST)


if __name__ == "__main__":
    main()
