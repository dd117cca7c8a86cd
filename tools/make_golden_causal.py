#!/usr/bin/env python3
"""Generate the causal SuDoRM-RF (v3) fixtures from the REAL reference (build host only).

Loads the unmodified reference module by file path (under a private module name), puts the weights of
tests/causal_fixtures.py into it, runs the reference forward on CPU in fp32 and stores:
  tests/golden/<case>.npz          reference outputs ("out"; "enc" / "sep" = encoder / separation-module output)
  tests/golden/CAUSAL_MANIFEST.json the cases (config, batch, T, seeds, max |out|), the sha256 digests of the reference's
                                   state_dict under torch.manual_seed(1234) for two configs, and the pickle's description
  tests/golden/ref_causal_module.pt a whole-module pickle (torch.save) of a tiny reference CausalSuDORMRF

    SRF_REFERENCE=<reference checkout> python tools/make_golden_causal.py
The GPU box has no reference: tests there regenerate weights and inputs from (config, seed).  Regenerating is bit-identical.
"""
import hashlib
import importlib.util
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import causal_fixtures as cf  # noqa: E402

REF = os.environ.get("SRF_REFERENCE", "")
REL = "sudo_rm_rf/dnn/models/causal_improved_sudormrf_v3.py"


def load_ref():
    spec = importlib.util.spec_from_file_location("_ref_causal_improved_sudormrf_v3", os.path.join(REF, REL))
    mod = importlib.util.module_from_spec(spec)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        spec.loader.exec_module(mod)
    return mod


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def main():
    if not REF or not os.path.isdir(REF):
        raise SystemExit("set SRF_REFERENCE to a checkout of the reference implementation")
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    ref = load_ref()
    manifest = {"generator": "tools/make_golden_causal.py", "torch": torch.__version__, "cases": {}}
    for name, (cfg, batch, T, wseed, iseed, stored) in cf.CASES.items():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            torch.manual_seed(0)
            m = ref.CausalSuDORMRF(**cfg).eval()
        sd = cf.make_state_dict(cfg, wseed)
        assert [k for k, _ in cf.schema(cfg)] == list(m.state_dict())
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        grab = {}
        m.encoder.register_forward_hook(lambda mod, i, o: grab.__setitem__("enc", o.detach().clone()))
        m.sm.register_forward_hook(lambda mod, i, o: grab.__setitem__("sep", o.detach().clone()))
        wav = torch.from_numpy(cf.make_input(name))
        with torch.no_grad():
            out = m(wav)
        arrays = {"out": out.numpy()}
        for k in stored:
            if k != "out":
                arrays[k] = grab[k].numpy()
        amax = float(np.abs(arrays["out"]).max())
        assert 0.1 <= amax <= 10.0, (name, amax)
        cf.save_npz(os.path.join(cf.GOLDEN, name + ".npz"), arrays)
        manifest["cases"][name] = {"config": cfg, "batch": batch, "T": T, "weight_seed": wseed, "input_seed": iseed,
                                   "stored": list(stored), "max_abs_out": amax, "frames": int(grab["enc"].shape[-1]),
                                   "padded_length": int(grab["enc"].shape[-1]) * (cfg["enc_kernel_size"] // 2),
                                   "num_params": int(sum(v.size for v in sd.values()))}
        print("%-20s out %s max|out| %.3f" % (name, tuple(out.shape), amax), flush=True)
    host = {}
    for tag, cfg in cf.DIGEST_CONFIGS.items():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            torch.manual_seed(1234)
            m = ref.CausalSuDORMRF(**cfg)
        host[tag] = {"config": cfg, "seed": 1234,
                     "state_dict": [[k, list(v.shape), digest(v)] for k, v in m.state_dict().items()],
                     "attributes": {a: getattr(m, a) for a in cf.FIELDS + ("n_least_samples_req",)}}
    manifest["digests"] = host
    path = os.path.join(cf.GOLDEN, "ref_causal_module.pt")
    code = ("import sys, warnings, torch\nsys.path.insert(0, %r)\nwarnings.simplefilter('ignore')\n"
            "import sudo_rm_rf.dnn.models.causal_improved_sudormrf_v3 as c\ntorch.manual_seed(7)\n"
            "m = c.CausalSuDORMRF(**%r)\nassert type(m).__module__ == 'sudo_rm_rf.dnn.models.causal_improved_sudormrf_v3'\n"
            "torch.save(m, %r)\n" % (REF, cf.PICKLE_CONFIG, path))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=cf.GOLDEN, env=dict(os.environ, PYTHONPATH=""))
    manifest["pickle"] = {"file": os.path.basename(path), "config": cf.PICKLE_CONFIG, "seed": 7}
    with open(cf.MANIFEST, "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", cf.MANIFEST)


if __name__ == "__main__":
    main()
