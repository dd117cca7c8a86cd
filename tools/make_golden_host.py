#!/usr/bin/env python3
"""Golden fixtures for tests/test_host_interface.py, made with the UNMODIFIED reference classes.

  HOST_MANIFEST.json            per small configuration: the state_dict the reference's constructor makes under
                                torch.manual_seed(1234) -- keys in order, shapes, dtypes, sha256 of every tensor's bytes --
                                and the public attributes the README recipe reads back
  ref_groupcomm_module.pt       a whole-module pickle (torch.save) of a reference GroupCommSudoRmRf, the form of the
                                published checkpoints

    SRF_REFERENCE=<reference checkout> python tools/make_golden_host.py
"""
import hashlib
import importlib.util
import json
import os
import subprocess
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.schema import ModelConfig  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
ATTRS = ("out_channels", "in_channels", "num_blocks", "upsampling_depth", "enc_kernel_size", "enc_num_basis", "num_sources",
         "n_least_samples_req")
# tests/test_host_interface.py: SMALL
SMALL = [ModelConfig("improved", 16, 32, 2, 3, 21, 24, 2),
         ModelConfig("improved", 128, 512, 2, 4, 21, 512, 2),
         ModelConfig("groupcomm", 32, 64, 2, 3, 21, 24, 2, 1, 4),
         ModelConfig("groupcomm", 32, 64, 1, 2, 11, 16, 2, 2, 8)]
PICKLE_CFG = SMALL[2]


def tensor_digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def main():
    ref = os.environ.get("SRF_REFERENCE")
    if not ref or not os.path.isdir(ref):
        raise SystemExit("set SRF_REFERENCE to a checkout of the reference implementation")
    cases = {}
    for i, cfg in enumerate(SMALL):
        rel = "sudo_rm_rf/dnn/models/" + ("improved_sudormrf.py" if cfg.variant == "improved" else "groupcomm_sudormrf_v2.py")
        spec = importlib.util.spec_from_file_location("_ref_%s_%d" % (cfg.variant, i), os.path.join(ref, rel))
        mod = importlib.util.module_from_spec(spec)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            spec.loader.exec_module(mod)
            cls = mod.SuDORMRF if cfg.variant == "improved" else mod.GroupCommSudoRmRf
            torch.manual_seed(1234)
            m = cls(**cfg.ctor_kwargs())
        sd = m.state_dict()
        cases["case%d" % i] = {"config": cfg.__dict__, "seed": 1234,
                               "state_dict": [[k, list(v.shape), str(v.dtype).replace("torch.", ""), tensor_digest(v)]
                                              for k, v in sd.items()],
                               "attributes": {a: getattr(m, a) for a in ATTRS}}
    # the pickle is made in a fresh interpreter with ONLY the reference on the path, as a user of the reference would
    path = os.path.join(GOLDEN, "ref_groupcomm_module.pt")
    code = ("import sys, warnings, torch\nsys.path.insert(0, %r)\nwarnings.simplefilter('ignore')\n"
            "import sudo_rm_rf.dnn.models.groupcomm_sudormrf_v2 as g\ntorch.manual_seed(7)\n"
            "m = g.GroupCommSudoRmRf(**%r)\nassert type(m).__module__ == 'sudo_rm_rf.dnn.models.groupcomm_sudormrf_v2'\n"
            "torch.save(m, %r)\n" % (ref, PICKLE_CFG.ctor_kwargs(), path))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=os.path.dirname(path), env=dict(os.environ, PYTHONPATH=""))
    manifest = {"generator": "tools/make_golden_host.py", "torch": torch.__version__, "cases": cases,
                "pickle": {"file": os.path.basename(path), "config": PICKLE_CFG.__dict__, "seed": 7}}
    with open(os.path.join(GOLDEN, "HOST_MANIFEST.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print("wrote", os.path.join(GOLDEN, "HOST_MANIFEST.json"), path)


if __name__ == "__main__":
    main()
