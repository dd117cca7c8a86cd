#!/usr/bin/env python3
"""Generate the fixtures of the ragged attentive layer / block tests from the REAL reference (build host only, CPU).

Loads the unmodified reference module by file path, builds ITS TransformerLayer / AttentiveUConvBlock in fp64 and eval() from
float32-representable random parameters (the first rows of pos_enc.pe random too), and runs every example of a ragged batch
ALONE, on its own slice x[b:b+1, :, :lengths[b]] -- the definition of a ragged call.  Writes
  tests/golden/attn_ragged_<case>.npz            x (the padded batch), parameters, pe[:Ld], lengths, the zero-padded outputs
  tests/golden/ATTENTIVE_RAGGED_MANIFEST.json    the cases (tests/attentive_ragged_cases.py)

    SRF_REFERENCE=<reference checkout> python tools/make_golden_attentive_ragged.py
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
from tests import attentive_ragged_cases as rc  # noqa: E402

REF = os.environ.get("SRF_REFERENCE", "")
REL = "sudo_rm_rf/dnn/models/attentive_sudormrf_v2.py"
MAX_FILE = 1 << 20


def load_ref():
    spec = importlib.util.spec_from_file_location("_ref_attentive_sudormrf_v2", os.path.join(REF, REL))
    mod = importlib.util.module_from_spec(spec)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        spec.loader.exec_module(mod)
    return mod


def f32(g, *shape, scale=1.0, shift=0.0):
    """float32-representable values as an fp64 tensor"""
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale + shift).float().double()


def randomise(module, g, Ld):
    """Every parameter random (norm gains around 1, PReLU slopes around 0.25, weights scaled by their fan-in), pe[:Ld] random."""
    with torch.no_grad():
        for name, prm in module.named_parameters():
            if name.endswith("gamma"):
                prm.copy_(f32(g, *prm.shape, scale=0.2, shift=1.0))
            elif name.endswith("beta") or name.endswith("bias"):
                prm.copy_(f32(g, *prm.shape, scale=0.2))
            elif name.endswith("act.weight"):
                prm.copy_(f32(g, *prm.shape, scale=0.05, shift=0.25))
            else:
                prm.copy_(f32(g, *prm.shape, scale=prm[0].numel() ** -0.5))
        for name, buf in module.named_buffers():
            assert name.endswith("pe")
            buf[0, :Ld] = f32(g, Ld, buf.shape[-1], scale=0.7)


def run_case(ref, name, c, index):
    g = torch.Generator().manual_seed(9400 + index)
    lengths, L, Bt = c["lengths"], c["L"], len(c["lengths"])
    norm = None
    if c["module"] == "layer":
        Ld, Cin = L, c["emb"]
        m = ref.TransformerLayer(c["emb"], c["d_model"], c["heads"]).double().eval()
        layer = m
        if c["lazy"]:
            norm = ref.GlobLN(c["emb"]).double().eval()
            randomise(norm, g, 0)
    else:
        Ld, Cin = L >> (c["depth"] - 1), c["out"]
        m = ref.AttentiveUConvBlock(c["out"], c["emb"], c["depth"], c["heads"], c["d_model"]).double().eval()
        layer = m.attention
    randomise(m, g, Ld)
    x = f32(g, Bt, Cin, L)
    out = torch.zeros(Bt, Cin, L, dtype=torch.float64)
    with torch.no_grad():
        for b, n in enumerate(lengths):
            xb = x[b:b + 1, :, :n]
            out[b:b + 1, :, :n] = m(norm(xb) if norm is not None else xb)
    arrays = dict(x=x.numpy().astype(np.float32), out=out.numpy(), lengths=np.asarray(lengths, dtype=np.int32),
                  pe=layer.pos_enc.pe[0, :Ld].numpy().astype(np.float32))
    named = list(m.named_parameters()) + ([("in_norm." + n, q) for n, q in norm.named_parameters()] if norm is not None else [])
    for n, q in named:
        arrays["param." + n] = q.detach().numpy().astype(np.float32)
        assert np.array_equal(arrays["param." + n].astype(np.float64), q.detach().numpy()), n   # float32-representable
    np.savez_compressed(rc.path(name), **arrays)
    size = os.path.getsize(rc.path(name))
    assert size < MAX_FILE, (name, size)
    info = dict(c, Ld=Ld, bytes=size, max_abs_out=float(out.abs().max()), stored=sorted(arrays))
    print("%-14s out %s max|out| %.3f, %d bytes" % (name, tuple(out.shape), info["max_abs_out"], size), flush=True)
    return info


def main():
    if not REF or not os.path.isdir(REF):
        raise SystemExit("set SRF_REFERENCE to a checkout of the reference implementation")
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    ref = load_ref()
    manifest = {"generator": "tools/make_golden_attentive_ragged.py", "torch": torch.__version__, "cases": {}}
    for index, (name, c) in enumerate(rc.CASES.items()):
        manifest["cases"][name] = run_case(ref, name, c, index)
    with open(rc.MANIFEST, "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", rc.MANIFEST)


if __name__ == "__main__":
    main()
