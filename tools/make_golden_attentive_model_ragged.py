#!/usr/bin/env python3
"""Generate the fixtures of the attentive v2 model's ragged forward from the REAL reference (build host only).

For every case of tests/attentive_model_ragged_cases.py: the unmodified reference SuDORMRF in eval() with the weights of
tests/attentive_fixtures.make_state_dict, run on EVERY ROW ALONE at its own length (CPU, fp32: the dtype and seeding scheme of
tools/make_golden_attentive.py).  Stored: tests/golden/attn_model_ragged_<case>.npz (lengths, out<b> [S, lengths[b]]) and
tests/golden/ATTN_MODEL_RAGGED_MANIFEST.json (config, lengths, seeds, frames, per-row max |out|).  Weights and mixtures are
regenerated from the seeds by the tests.  Every row's max |out| must be at least 100 x the tests' bar (1e-4), or the seeds are
refused: a row of near-silence would pass the bar whatever the kernels do.

    SRF_REFERENCE=<reference checkout> python tools/make_golden_attentive_model_ragged.py
"""
import json
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import attentive_fixtures as af  # noqa: E402
from tests import attentive_model_ragged_cases as mc  # noqa: E402
from tools.make_golden_attentive import load_ref  # noqa: E402


def main():
    import tools.make_golden_attentive as g
    if not g.REF or not os.path.isdir(g.REF):
        raise SystemExit("set SRF_REFERENCE to a checkout of the reference implementation")
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    ref = load_ref()
    manifest = {"generator": "tools/make_golden_attentive_model_ragged.py", "torch": torch.__version__, "bar": mc.BAR, "cases": {}}
    for name, (cfg, lengths, wseed, iseed) in mc.CASES.items():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            torch.manual_seed(0)
            m = ref.SuDORMRF(**cfg).eval()
        sd = af.make_state_dict(cfg, wseed)
        assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == af.schema(cfg)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        wav = torch.from_numpy(mc.make_wav(name))
        arrays = {"lengths": np.asarray(lengths, dtype=np.int32)}
        amax = []
        for b, n in enumerate(lengths):
            with torch.no_grad():
                out = m(wav[b:b + 1, :, :n])
            assert tuple(out.shape) == (1, cfg["num_sources"], n)
            arrays["out%d" % b] = out[0].numpy()
            amax.append(float(out.abs().max()))
            assert amax[-1] >= 100 * mc.BAR, "case %s row %d: max |out| = %g is below 100 x the bar; pick other seeds" % (name, b, amax[-1])
        af.save_npz(mc.path(name), arrays)
        manifest["cases"][name] = {"config": cfg, "lengths": list(lengths), "T": max(lengths), "weight_seed": wseed, "input_seed": iseed,
                                   "frames": [mc.frames(cfg, n) for n in lengths],
                                   "deepest": [mc.frames(cfg, n) >> (cfg["upsampling_depth"] - 1) for n in lengths],
                                   "max_abs_out": amax}
        print("%s lengths %s frames %s max|out| %s" % (name, list(lengths), manifest["cases"][name]["frames"],
                                                      ["%.3f" % a for a in amax]), flush=True)
    with open(mc.MANIFEST, "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", mc.MANIFEST)


if __name__ == "__main__":
    main()
