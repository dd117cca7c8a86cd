#!/usr/bin/env python3
"""Generate the degenerate-signal goldens from the REAL reference (build host only).

Loads the six unmodified reference model modules (and its mixture consistency) by file path under private module names, puts the
fixture weights of each family's tiny case into them (tests/edge_signals.py), runs the reference forward on the CPU in fp32 on
every signal of tests/edge_signals.signals -- silence, DC, DC plus a small signal, loud, tiny, near-silent, half-silent, one
silent row, an impulse -- and stores:
  tests/golden/edge_<family>.npz     "<signal>": the reference's output; "separate_<signal>" / "separate_mc_<signal>": the README
                                     recipe around the reference model (normalise by mean / std + 1e-9, forward, rescale, and
                                     the reference's own mixture_consistency.apply) without / with mixture consistency, for the
                                     settings tests/edge_signals.FAMILIES lists
  tests/golden/EDGE_MANIFEST.json    per case: max |out|, the deviation of the reference's fp32 output from the repo's fp64
                                     restatement, and whether the output is identically zero
Every case is checked here against the restatement at 1e-5 (x max(1, max |out|)), the bar the other generators hold theirs to.

    SRF_REFERENCE=<reference checkout> python tools/make_golden_edges.py
The GPU box has no reference: tests there regenerate weights and signals from seeds.  Regenerating is bit-identical.
"""
import importlib.util
import json
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import edge_signals as es  # noqa: E402
from tests.attentive_fixtures import save_npz  # noqa: E402

REF = os.environ.get("SRF_REFERENCE", "")
MODELS = "sudo_rm_rf/dnn/models/"
# family -> (module file, class)
CLASSES = {"improved": ("improved_sudormrf.py", "SuDORMRF"), "groupcomm": ("groupcomm_sudormrf_v2.py", "GroupCommSudoRmRf"),
           "causal": ("causal_improved_sudormrf_v3.py", "CausalSuDORMRF"), "attn": ("attentive_sudormrf_v2.py", "SuDORMRF"),
           "attn3": ("attentive_sudormrf_v3.py", "SuDORMRF"), "orig": ("sudormrf.py", "SuDORMRF")}


def load_ref(rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        spec.loader.exec_module(mod)
    return mod


def build(family):
    fn, cls = CLASSES[family]
    mod = load_ref(MODELS + fn, "_ref_edge_" + family)
    cfg = es.config(family)
    kw = cfg.ctor_kwargs() if hasattr(cfg, "ctor_kwargs") else cfg
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(0)
        m = getattr(mod, cls)(**kw).eval()
    sd = es.state_dict(family)
    assert list(m.state_dict()) == list(sd), family
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m, sd


def readme_recipe(m, mc, x, with_mc):
    """README.md's lines around the model, on [batch, time], in x's dtype (the model's forward always in fp32)"""
    with torch.no_grad():
        mix = x[:, 0]
        std, mean = mix.std(-1, keepdim=True), mix.mean(-1, keepdim=True)
        norm = (mix - mean) / (std + 1e-9)
        est = m(norm.unsqueeze(1).float()).to(x.dtype) * std.unsqueeze(1) + mean.unsqueeze(1)
        if with_mc:
            est = mc.apply(est, norm.unsqueeze(1))
    return est.numpy()


def entry(out, want):
    amax = float(np.abs(out).max())
    dev = float(np.abs(out.astype(np.float64) - want.numpy()).max())
    assert np.isfinite(out).all()
    return {"max_abs_out": amax, "restatement_fp64_deviation": dev, "identically_zero": bool(not out.any())}, amax, dev


def main():
    if not REF or not os.path.isdir(REF):
        raise SystemExit("set SRF_REFERENCE to a checkout of the reference implementation")
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    mc = load_ref("sudo_rm_rf/dnn/experiments/utils/mixture_consistency.py", "_ref_edge_mixture_consistency")
    manifest = {"generator": "tools/make_golden_edges.py", "torch": torch.__version__, "signal_seed": es.SEED, "families": {}}
    for family, (batch, T, wseed, recipes) in es.FAMILIES.items():
        m, sd = build(family)
        arrays, cases = {}, {}
        for signal, wav in es.family_signals(family).items():
            x = torch.from_numpy(wav)
            with torch.no_grad():
                out = m(x).numpy()
            key = es.case_key(signal)
            arrays[key] = out
            cases[key], amax, dev = entry(out, es.restatement(family, sd, wav))
            assert dev <= es.RESTATEMENT_TOL * max(1.0, amax), (family, key, dev, amax)
            line = "%-9s %-15s max|out| %.3e fp32 ref - fp64 restatement %.2e" % (family, signal, amax, dev)
            for with_mc in recipes:
                key = es.case_key(signal, with_mc)
                want = es.recipe(family, sd, wav, with_mc)
                est = readme_recipe(m, mc, x, with_mc)
                cases[key], amax, dev = entry(est, want)
                if dev > es.RESTATEMENT_TOL * max(1.0, amax):
                    # The README's lines in fp32 are ill-conditioned here: the mean of a (nearly) constant mixture is rounded to
                    # fp32, and (mix - mean) / (std + 1e-9) multiplies that rounding by up to 1e9 before mixture consistency adds
                    # it to the estimates.  The stored array is then the same lines evaluated in fp64 around the reference model's
                    # fp32 forward (the model itself refuses fp64 input); the fp32 figure stays in the manifest.
                    est64 = readme_recipe(m, mc, x.double(), with_mc)
                    fp32_dev = dev
                    cases[key], amax, dev = entry(est64, want)
                    cases[key].update(stored="recipe lines in fp64 around the fp32 reference model", reference_fp32_recipe_deviation=fp32_dev)
                    est = est64
                assert dev <= es.RESTATEMENT_TOL * max(1.0, amax), (family, key, dev, amax)
                arrays[key] = est
                line += " | recipe%s %.2e%s" % (" mc" if with_mc else "", dev, " (lines in fp64)" if est.dtype == np.float64 else "")
            print(line, flush=True)
        path = os.path.join(es.GOLDEN, "edge_%s.npz" % family)
        save_npz(path, arrays)
        assert os.path.getsize(path) <= (1 << 20), path
        manifest["families"][family] = {"batch": batch, "T": T, "weight_seed": wseed, "recipes": list(recipes), "cases": cases}
    with open(es.MANIFEST, "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", es.MANIFEST)


if __name__ == "__main__":
    main()
