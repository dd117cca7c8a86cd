#!/usr/bin/env python3
"""Generate the attentive SuDoRM-RF (v3) fixtures from the REAL reference (build host only).

Loads the unmodified reference module by file path (under a private module name), puts the weights of
tests/attentive_v3_fixtures.py into it, runs the reference forward on CPU in fp32 and stores:
  tests/golden/<case>.npz                 reference outputs ("out"; attn3_tiny also "res_q" / "res_v" / "res_out": the two
                                          inputs and the output of the first resampler block 0 runs, attentive_resamplers[0])
  tests/golden/attn3_pickle.npz           the output of the pickled module below on a seeded input
  tests/golden/ATTENTIVE_V3_MANIFEST.json the cases (config, batch, T, seeds, max |out|, positions of every level, the error of
                                          tests/attentive_v3_ref.py in fp64), the sha256 digests of the reference's state_dict
                                          under torch.manual_seed(1234) for two configs, and the pickle's description
  tests/golden/ref_attentive_v3_module.pt a whole-module pickle (torch.save) of a small reference SuDORMRF (data only)
Every case is checked here against tests/attentive_v3_ref.py in fp64 (1e-5) and for max |out| in [0.1, 10].

    SRF_REFERENCE=<reference checkout> python tools/make_golden_attentive_v3.py
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
from tests import attentive_v3_fixtures as af  # noqa: E402
from tests import attentive_v3_ref as ar  # noqa: E402

REF = os.environ.get("SRF_REFERENCE", "")
REL = "sudo_rm_rf/dnn/models/attentive_sudormrf_v3.py"


def load_ref():
    spec = importlib.util.spec_from_file_location("_ref_attentive_sudormrf_v3", os.path.join(REF, REL))
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
    manifest = {"generator": "tools/make_golden_attentive_v3.py", "torch": torch.__version__, "cases": {},
                "block_heads": af.HEADS, "block_att_dims": af.ATT_DIMS}
    for name, (cfg, batch, T, wseed, iseed) in af.CASES.items():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            torch.manual_seed(0)
            m = ref.SuDORMRF(**cfg).eval()
        sd = af.make_state_dict(cfg, wseed)
        assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == af.schema(cfg)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        grab, levels = {}, []
        if cfg["upsampling_depth"] > 1:
            m.sm[0].attentive_resamplers[0].register_forward_hook(
                lambda mod, args, kw, o: grab.update(res_q=kw["q"].detach().clone(), res_v=kw["v"].detach().clone(),
                                                     res_out=o.detach().clone()), with_kwargs=True)
        for dw in m.sm[0].spp_dw:
            dw.register_forward_hook(lambda mod, i, o: levels.append(int(o.shape[-1])))
        wav = torch.from_numpy(af.make_input(name))
        with torch.no_grad():
            out = m(wav)
        arrays = {"out": out.numpy()}
        if name == "attn3_tiny":
            arrays.update({k: v.numpy() for k, v in grab.items()})
        amax = float(np.abs(arrays["out"]).max())
        assert 0.1 <= amax <= 10.0, (name, amax)
        assert levels == af.level_lengths(cfg, T) == af.LEVELS[name], (name, levels)
        err = float(np.abs(ar.forward(cfg, sd, wav.numpy(), torch.float64).numpy() - arrays["out"]).max())
        assert err <= 1e-5, (name, err)
        af.save_npz(os.path.join(af.GOLDEN, name + ".npz"), arrays)
        manifest["cases"][name] = {"config": cfg, "batch": batch, "T": T, "weight_seed": wseed, "input_seed": iseed,
                                   "stored": sorted(arrays), "max_abs_out": amax, "padded_length": af.padded_length(cfg, T),
                                   "levels": levels, "restatement_fp64_error": err,
                                   "num_params": int(sum(v.size for v in sd.values()))}
        print("%-18s out %s max|out| %.3f levels %s fp64 restatement %.2e" % (name, tuple(out.shape), amax, levels, err), flush=True)
    host = {}
    for tag, cfg in af.DIGEST_CONFIGS.items():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            torch.manual_seed(1234)
            m = ref.SuDORMRF(**cfg)
        host[tag] = {"config": cfg, "seed": 1234,
                     "state_dict": [[k, list(v.shape), digest(v)] for k, v in m.state_dict().items()],
                     "attributes": {a: getattr(m, a) for a in ("in_channels", "out_channels", "num_blocks", "upsampling_depth",
                                                               "enc_kernel_size", "enc_num_basis", "num_sources", "lcm")}}
    manifest["digests"] = host
    path = os.path.join(af.GOLDEN, "ref_attentive_v3_module.pt")
    wav = af.make_mixture(af.PICKLE_BATCH, af.PICKLE_T, af.PICKLE_INPUT_SEED)
    wav_path = os.path.join(af.GOLDEN, "_attn3_pickle_in.npy")
    out_path = os.path.join(af.GOLDEN, "_attn3_pickle_out.npy")
    np.save(wav_path, wav)
    code = ("import sys, warnings, numpy, torch\nsys.path.insert(0, %r)\nwarnings.simplefilter('ignore')\n"
            "import sudo_rm_rf.dnn.models.attentive_sudormrf_v3 as c\ntorch.manual_seed(%d)\n"
            "m = c.SuDORMRF(**%r).eval()\nassert type(m).__module__ == 'sudo_rm_rf.dnn.models.attentive_sudormrf_v3'\n"
            "torch.save(m, %r)\n"
            "with torch.no_grad():\n    numpy.save(%r, m(torch.from_numpy(numpy.load(%r))).numpy())\n"
            % (REF, af.PICKLE_SEED, af.PICKLE, path, out_path, wav_path))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=af.GOLDEN, env=dict(os.environ, PYTHONPATH=""))
    out = np.load(out_path)
    os.remove(wav_path)
    os.remove(out_path)
    af.save_npz(os.path.join(af.GOLDEN, "attn3_pickle.npz"), {"out": out})
    manifest["pickle"] = {"file": os.path.basename(path), "config": af.PICKLE, "seed": af.PICKLE_SEED, "batch": af.PICKLE_BATCH,
                          "T": af.PICKLE_T, "input_seed": af.PICKLE_INPUT_SEED, "golden": "attn3_pickle.npz",
                          "max_abs_out": float(np.abs(out).max())}
    with open(af.MANIFEST, "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", af.MANIFEST, "pickle bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
