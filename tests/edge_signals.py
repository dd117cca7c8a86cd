"""Degenerate signals and the six model families they are pushed through -- shared by the generator of the edge goldens
(tools/make_golden_edges.py, which runs the reference on the build host), the host test that pins the fp64 restatements to those
goldens (tests/test_edge_golden.py) and the GPU tests (tests/test_gpu_edge_signals.py, test_degenerate_inputs_match_oracle of
tests/test_gpu_model.py, the ragged and the training tests).

On well-conditioned input the 1e-8 inside every GlobLN / GroupNorm, the 1e-9 of the waveform normalisation and of mixture
consistency, the clamp of a negative variance and the activations' subgradient at exactly 0 are numerically invisible.  They
decide the answer for silence, DC, near-silence, very loud input and exact zeros, which is what a separation model meets between
utterances, in zero-padded tails and on a muted stream.
"""
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = os.path.join(GOLDEN, "EDGE_MANIFEST.json")
SEED = 20240
NAMES = ("silence", "dc", "dc_plus_small", "loud", "tiny", "near_silent", "half_silent", "one_silent_row", "impulse")
RESTATEMENT_TOL = 1e-5      # what every golden generator holds its restatement to (x max(1, max |out|) for `loud`)


def signals(batch, channels, T, seed=SEED):
    """name -> float32 [batch, channels, T].  `noise` is one standard-normal draw shared by every signal that uses it."""
    rng = np.random.default_rng(seed)
    noise = rng.standard_normal(size=(batch, channels, T))
    out = {"silence": np.zeros_like(noise), "dc": np.full_like(noise, 0.37), "dc_plus_small": 0.37 + 1e-4 * noise,
           "loud": noise * 1e3, "tiny": noise * 1e-6, "near_silent": noise * 1e-8}
    half = noise.copy()
    half[..., T // 2:] = 0.0
    row = noise.copy()
    row[0] = 0.0
    imp = np.zeros_like(noise)
    for b in range(batch):
        for c in range(channels):
            imp[b, c, (T // 3 + 97 * b + 13 * c) % T] = 1.0          # a single 1.0 per row, at a different place in each
    out.update(half_silent=half, one_silent_row=row, impulse=imp)
    assert tuple(out) == NAMES
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in out.items()}


# ---- the families: smallest committed configuration and fixture weights of each ------------------------------------------------
def _improved():
    from oracle.schema import ModelConfig
    return ModelConfig("improved", 16, 32, 2, 3, 21, 24, 2)


def _groupcomm():
    from oracle.schema import ModelConfig
    return ModelConfig("groupcomm", 32, 64, 2, 3, 21, 24, 2, 1, 4)


# name -> (batch, T, weight seed, recipes): recipes = the mixture_consistency settings its `separate` recipe is pinned at and run
# with -- both for every family: pipeline.separate takes the flag for every model (the README prescribes it for GroupComm, the
# FUSS loop uses it with the causal model, whose recipe runs on the stand-alone wav_normalize / wav_denormalize kernels)
BOTH = (False, True)
FAMILIES = {
    "improved": (2, 1600, 8, BOTH),          # (the configuration, seed and length of test_degenerate_inputs_match_oracle)
    "groupcomm": (2, 1600, 8, BOTH),
    "causal": (2, 1001, 101, BOTH),          # causal_tiny
    "attn": (2, 1001, 201, BOTH),            # attn_tiny
    "attn3": (2, 1001, 301, BOTH),           # attn3_tiny
    "orig": (2, 1001, 401, BOTH),            # orig_tiny
}


def config(family):
    if family in ("improved", "groupcomm"):
        return _improved() if family == "improved" else _groupcomm()
    if family == "causal":
        from tests import causal_fixtures as cf
        return cf.TINY
    if family == "attn":
        from tests import attentive_fixtures as af
        return af.TINY
    if family == "attn3":
        from tests import attentive_v3_fixtures as af3
        return af3.TINY
    from tests import original_fixtures as of
    return of.TINY


def state_dict(family):
    """key -> float32 ndarray: the fixture weights of the family's tiny case"""
    seed = FAMILIES[family][2]
    cfg = config(family)
    if family in ("improved", "groupcomm"):
        from oracle import weights
        return weights.make_state_dict(cfg, seed=seed)
    mod = {"causal": "causal_fixtures", "attn": "attentive_fixtures", "attn3": "attentive_v3_fixtures", "orig": "original_fixtures"}
    import importlib
    return importlib.import_module("tests." + mod[family]).make_state_dict(cfg, seed)


def module_class(family):
    """The class the GPU tests build: the reference's import paths for the two models that have them, the package's own for the rest"""
    import importlib
    name, cls = {"improved": ("sudo_rm_rf.dnn.models.improved_sudormrf", "SuDORMRF"),          # (the reference's import paths)
                 "groupcomm": ("sudo_rm_rf.dnn.models.groupcomm_sudormrf_v2", "GroupCommSudoRmRf"),
                 "causal": ("sudo_rm_rf_amd.dnn.models.causal_improved_sudormrf_v3", "CausalSuDORMRF"),
                 "attn": ("sudo_rm_rf_amd.dnn.models.attentive_sudormrf_v2", "SuDORMRF"),
                 "attn3": ("sudo_rm_rf_amd.dnn.models.attentive_sudormrf_v3", "SuDORMRF"),
                 "orig": ("sudo_rm_rf_amd.dnn.models.sudormrf", "SuDORMRF")}[family]
    return getattr(importlib.import_module(name), cls)


def family_signals(family):
    batch, T = FAMILIES[family][:2]
    return signals(batch, 1, T)


def restatement(family, sd, wav, dtype=torch.float64):
    """The repo's plain-torch restatement of the family's forward: [batch, S, T] as a `dtype` tensor, no graph."""
    cfg = config(family)
    with torch.no_grad():
        if family in ("improved", "groupcomm"):
            from oracle import torch_oracle
            return torch_oracle.forward(cfg, {k: torch.as_tensor(v).to(dtype) for k, v in sd.items()}, torch.as_tensor(wav).to(dtype))
        if family == "causal":
            from tests import causal_train_ref as ctr
            return ctr.forward(cfg, {k: torch.as_tensor(v).to(dtype) for k, v in sd.items()}, torch.as_tensor(wav).to(dtype))
        mod = {"attn": "attentive_ref", "attn3": "attentive_v3_ref", "orig": "original_ref"}[family]
        import importlib
        return importlib.import_module("tests." + mod).forward(cfg, sd, wav, dtype)


def recipe(family, sd, mixture, mixture_consistency, dtype=torch.float64):
    """The caller-side recipe around the restatement: per-example mean / unbiased std (+ 1e-9), forward, rescale and, on request,
    mixture consistency (uniform weights) of the rescaled estimates against the normalised mixture, as srf_separate has it."""
    x = torch.as_tensor(mixture).to(dtype)
    m, sdev = x.mean(-1, keepdim=True), x.std(-1, keepdim=True)
    norm = (x - m) / (sdev + 1e-9)
    est = restatement(family, sd, norm, dtype) * sdev + m
    if mixture_consistency:
        est = est + (norm - est.sum(1, keepdim=True)) / est.shape[1]
    return est


def case_key(signal, mc=None):
    """The array's name inside tests/golden/edge_<family>.npz: the forward, or the recipe with / without mixture consistency"""
    return signal if mc is None else ("separate_mc_" if mc else "separate_") + signal


def load_manifest():
    with open(MANIFEST) as f:
        return json.load(f)


def load_golden(family):
    with np.load(os.path.join(GOLDEN, "edge_%s.npz" % family)) as z:
        return {k: z[k] for k in z.files}


# ---- the bars --------------------------------------------------------------------------------------------------------------
def inference_bar(want_max, reference_is_zero, reference_fp32_deviation=None):
    """The degenerate test's 2e-4 max|want| + 1e-6, tightened so that it cannot pass vacuously: no absolute term where
    max|want| < 1e-3 (`tiny` and `near_silent` through a mask-times-encoder model), and <= 1e-6 where the reference's own output
    is identically zero.  reference_fp32_deviation: only for a case listed in REFERENCE_LIMITED -- the bar is then 8 x the
    deviation of the reference's own fp32 output from the fp64 restatement (the rule of tests/test_gpu_original_kernels.py)."""
    if reference_fp32_deviation is not None:
        return 8.0 * reference_fp32_deviation
    if reference_is_zero:
        return 1e-6
    return 2e-4 * want_max + (1e-6 if want_max >= 1e-3 else 0.0)


# (family, signal): a case that misses inference_bar because the reference's own fp32 output deviates from fp64 by the larger
# part is listed here, with that deviation quoted, and held to 8 x the manifest's figure instead.  None so far.
REFERENCE_LIMITED = {}
_MANIFEST = []


def _manifest():
    if not _MANIFEST:
        _MANIFEST.append(load_manifest())
    return _MANIFEST[0]


def check_inference(family, signal, got, want, lines=None):
    """got (numpy, from the device) against the fp64 restatement under edge_signals.inference_bar"""
    meta = _manifest()["families"][family]["cases"][case_key(signal)]
    wmax = float(np.abs(want).max())
    bar = inference_bar(wmax, meta["identically_zero"],
                           meta["restatement_fp64_deviation"] if (family, signal) in REFERENCE_LIMITED else None)
    assert got.shape == want.shape and np.isfinite(got).all(), (family, signal)
    err = float(np.abs(got.astype(np.float64) - want).max())
    line = "%-9s %-15s err %.3e bar %.3e (max|want| %.3e, reference fp32 - fp64 %.2e)" % (
        family, signal, err, bar, wmax, meta["restatement_fp64_deviation"])
    print(line)
    if lines is not None:
        lines.append(line)
    if meta["identically_zero"]:
        assert wmax == 0.0
    assert err <= bar, line
    return err


def recipe_bar(mixture_row):
    """The existing recipe tests' 1e-4 max(1, std) per example (std = 0 for silence)"""
    return 1e-4 * max(1.0, float(np.std(mixture_row, ddof=1)))


def write_profile_lines(section, lines):
    """Measured figures of a GPU test go to $SRF_EDGE_REPORT/<section>.txt when that variable names a directory;
    profiles/edge_signals.txt was assembled from those files."""
    root = os.environ.get("SRF_EDGE_REPORT", "")
    if not root:
        return
    os.makedirs(root, exist_ok=True)
    with open(os.path.join(root, section + ".txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
