#!/usr/bin/env python3
"""Generate the original SuDoRM-RF fixtures from the REAL reference (build host only).

Loads the unmodified reference module by file path (under a private module name), puts the weights of
tests/original_fixtures.py into it, runs the reference forward on CPU in fp32 and stores:
  tests/golden/<case>.npz              reference outputs ("out"; orig_tiny also "block0": the output of sm[0], and "z": the mask
                                       layer's output before the softmax, [batch, S, N, L])
  tests/golden/orig_pickle.npz         the output of the pickled module below on a seeded input
  tests/golden/ORIGINAL_MANIFEST.json  the cases (config, batch, T, seeds, max |out|, padded length, frames, number of tensors,
                                       the error of tests/original_ref.py in fp64), the state_dict keys and shapes, the sha256
                                       digests of the reference's state_dict under torch.manual_seed(1234) for two configs, and
                                       the pickle's description
  tests/golden/ref_original_module.pt  a whole-module pickle (torch.save) of a small reference SuDORMRF (data only)
Every case is checked here against tests/original_ref.py in fp64 (1e-5) and for max |out| in [0.1, 10]; the state_dict order is
asserted against tests/original_fixtures.schema.

    SRF_REFERENCE=<reference checkout> python tools/make_golden_original.py
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
from tests import original_fixtures as of  # noqa: E402
from tests import original_ref as orf  # noqa: E402

REF = os.environ.get("SRF_REFERENCE", "")
REL = "sudo_rm_rf/dnn/models/sudormrf.py"


def load_ref():
    spec = importlib.util.spec_from_file_location("_ref_sudormrf", os.path.join(REF, REL))
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
    manifest = {"generator": "tools/make_golden_original.py", "torch": torch.__version__, "cases": {}}
    for name, (cfg, batch, T, wseed, iseed) in of.CASES.items():
        torch.manual_seed(0)
        m = ref.SuDORMRF(**cfg).eval()
        sd = of.make_state_dict(cfg, wseed)
        assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == of.schema(cfg), name
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        grab = {}
        m.sm[0].register_forward_hook(lambda mod, i, o: grab.update(block0=o.detach().clone()))
        m.m.register_forward_hook(lambda mod, i, o: grab.update(z=o.detach().clone()))
        wav = torch.from_numpy(of.make_input(name))
        with torch.no_grad():
            out = m(wav)
        arrays = {"out": out.numpy()}
        if name == "orig_tiny":
            arrays.update({k: v.numpy() for k, v in grab.items()})
        amax = float(np.abs(arrays["out"]).max())
        assert 0.1 <= amax <= 10.0, (name, amax)
        taps = {}
        err = float(np.abs(orf.forward(cfg, sd, wav.numpy(), torch.float64, taps).numpy() - arrays["out"]).max())
        assert err <= 1e-5, (name, err)
        assert float((taps["block0"] - grab["block0"]).abs().max()) <= 1e-5 and float((taps["z"] - grab["z"]).abs().max()) <= 1e-5
        L = int(grab["z"].shape[-1])
        assert L == of.frames(cfg, T) and tuple(grab["z"].shape[1:3]) == (cfg["num_sources"], cfg["enc_num_basis"])
        of.save_npz(os.path.join(of.GOLDEN, name + ".npz"), arrays)
        manifest["cases"][name] = {"config": cfg, "batch": batch, "T": T, "weight_seed": wseed, "input_seed": iseed,
                                   "stored": sorted(arrays), "max_abs_out": amax, "padded_length": of.padded_length(cfg, T),
                                   "frames": L, "restatement_fp64_error": err, "num_tensors": len(sd),
                                   "schema": [[k, list(s)] for k, s in of.schema(cfg)],
                                   "num_params": int(sum(v.size for v in sd.values()))}
        print("%-18s out %s max|out| %.3f frames %d fp64 restatement %.2e" % (name, tuple(out.shape), amax, L, err), flush=True)
    host = {}
    for tag, cfg in of.DIGEST_CONFIGS.items():
        torch.manual_seed(1234)
        m = ref.SuDORMRF(**cfg)
        host[tag] = {"config": cfg, "seed": 1234,
                     "state_dict": [[k, list(v.shape), digest(v)] for k, v in m.state_dict().items()],
                     "attributes": {a: getattr(m, a) for a in ("in_channels", "out_channels", "num_blocks", "upsampling_depth",
                                                               "enc_kernel_size", "enc_num_basis", "num_sources", "lcm")}}
    manifest["digests"] = host
    path = os.path.join(of.GOLDEN, "ref_original_module.pt")
    wav = of.make_mixture(of.PICKLE_BATCH, of.PICKLE_T, of.PICKLE_INPUT_SEED)
    wav_path = os.path.join(of.GOLDEN, "_orig_pickle_in.npy")
    out_path = os.path.join(of.GOLDEN, "_orig_pickle_out.npy")
    np.save(wav_path, wav)
    # torch's default initialisers leave every GroupNorm at (1, 0) and every slope at 0.25: perturb them, seeded, before saving
    code = ("import sys, warnings, numpy, torch\nsys.path.insert(0, %r)\nwarnings.simplefilter('ignore')\n"
            "import sudo_rm_rf.dnn.models.sudormrf as c\ntorch.manual_seed(%d)\n"
            "m = c.SuDORMRF(**%r).eval()\nassert type(m).__module__ == 'sudo_rm_rf.dnn.models.sudormrf'\n"
            "with torch.no_grad():\n"
            "    for k, v in m.state_dict().items():\n"
            "        if '.norm.' in k or '.act.' in k or k.startswith('ln') or k.endswith('bias'):\n"
            "            v.add_(torch.rand_like(v) * 0.2 - 0.1)\n"
            "    m.decoder.weight.mul_(3.0)\n"
            "torch.save(m, %r)\n"
            "with torch.no_grad():\n    numpy.save(%r, m(torch.from_numpy(numpy.load(%r))).numpy())\n"
            % (REF, of.PICKLE_SEED, of.PICKLE, path, out_path, wav_path))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=of.GOLDEN, env=dict(os.environ, PYTHONPATH=""))
    out = np.load(out_path)
    os.remove(wav_path)
    os.remove(out_path)
    of.save_npz(os.path.join(of.GOLDEN, "orig_pickle.npz"), {"out": out})
    manifest["pickle"] = {"file": os.path.basename(path), "config": of.PICKLE, "seed": of.PICKLE_SEED, "batch": of.PICKLE_BATCH,
                          "T": of.PICKLE_T, "input_seed": of.PICKLE_INPUT_SEED, "golden": "orig_pickle.npz",
                          "max_abs_out": float(np.abs(out).max())}
    with open(of.MANIFEST, "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    for fn in sorted(os.listdir(of.GOLDEN)):
        if fn.startswith("orig_") or fn.startswith("ref_original") or fn == "ORIGINAL_MANIFEST.json":
            assert os.path.getsize(os.path.join(of.GOLDEN, fn)) <= (1 << 20), fn
    print("wrote", of.MANIFEST, "pickle bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
