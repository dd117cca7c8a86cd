#!/usr/bin/env python3
"""Generate the attentive training fixtures (TransformerLayer / AttentiveUConvBlock, forward and every gradient) from the
REAL reference (build host only, CPU).

Loads the unmodified reference module by file path, builds ITS TransformerLayer / AttentiveUConvBlock in fp64 from
float32-representable random parameters (the first Ld rows of pos_enc.pe random too), and swaps ONE thing: the nn.Dropout
instance of pos_enc, for a module that multiplies by the keep mask of srf_posenc_apply_dropout for a
stored (seed, offset, p) -- computed by the numpy restatement tests/attentive_train_ref.py, transposed to the reference's
[batch, len, channel] layout and scaled by the fp32 1 / (1 - p).  Runs forward and backward on a stored random output gradient
and writes
  tests/golden/attn_train_<case>.npz            inputs, parameters, pe[:Ld], (seed, offset, p), the output and every gradient
                                                (float32: 6e-8 relative beside the tests' bar of 2e-4)
  tests/golden/ATTENTIVE_TRAIN_MANIFEST.json    the cases

    SRF_REFERENCE=<reference checkout> python tools/make_golden_attentive_train.py
"""
import importlib.util
import json
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import attentive_train_ref as tr  # noqa: E402

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


class MaskedDropout(nn.Module):
    """Stands where pos_enc.dropout stood: x [batch, len, channel] times keep * inv_keep of the [batch, channel, len] tensor."""

    def __init__(self, p, seed, offset):
        super().__init__()
        self.p, self.seed, self.offset = p, seed, offset

    def forward(self, x):
        B, L, C = x.shape
        return x * tr.keep_tensor((B, C, L), self.p, self.seed, self.offset).transpose(1, 2)


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
                fan_in = prm[0].numel()
                prm.copy_(f32(g, *prm.shape, scale=fan_in ** -0.5))
        for name, buf in module.named_buffers():
            assert name.endswith("pe")
            buf[0, :Ld] = f32(g, Ld, buf.shape[-1], scale=0.7)


def run_case(ref, name, c, index):
    g = torch.Generator().manual_seed(9000 + index)
    p = c["p"]
    seed = int(torch.randint(0, 2 ** 63 - 1, (1,), generator=g))
    offset = int(torch.randint(2 ** 32, 2 ** 63 - 1, (1,), generator=g))          # (an offset above 2^32: both halves in use)
    arrays = {"p": np.float32(p), "seed": np.uint64(seed), "offset": np.uint64(offset)}
    grab = {}
    if c["module"] == "layer":
        Ld, C = c["Ld"], c["emb"]
        m = ref.TransformerLayer(C, c["d_model"], c["heads"], dropout=p).double().train()
        layer, pre = m, ""
        x = f32(g, c["Bt"], C, Ld).requires_grad_()
        norm = None
        if c["lazy"]:
            norm = ref.GlobLN(C).double()
            randomise(norm, g, 0)
    else:
        D, C = c["depth"], c["emb"]
        Ld = c["L"] >> (D - 1)
        m = ref.AttentiveUConvBlock(c["out"], C, D, c["heads"], c["d_model"], att_dropout=p).double().train()
        layer, pre = m.attention, "attention."
        x = f32(g, c["Bt"], c["out"], c["L"]).requires_grad_()
        norm = None
    randomise(m, g, Ld)
    layer.pos_enc.dropout = MaskedDropout(p, seed, offset)                          # the ONE swap
    def keep_k(mod, inputs, output):
        output.retain_grad()
        grab["k"] = output

    layer.mha.K_proj.register_forward_hook(keep_k)
    out = m(norm(x) if norm is not None else x)
    gout = f32(g, *out.shape)
    out.backward(gout)
    arrays.update(x=x.detach().numpy().astype(np.float32), gout=gout.numpy().astype(np.float32),
                  out=out.detach().numpy(), pe=layer.pos_enc.pe[0, :Ld].numpy().astype(np.float32))
    arrays["grad.x"] = x.grad.numpy().astype(np.float32)
    named = list(m.named_parameters()) + ([("in_norm." + n, q) for n, q in norm.named_parameters()] if norm is not None else [])
    for n, q in named:
        assert q.grad is not None, n
        arrays["param." + n] = q.detach().numpy().astype(np.float32)
        arrays["grad." + n] = q.grad.numpy().astype(np.float32)
        assert np.array_equal(arrays["param." + n].astype(np.float64), q.detach().numpy()), n   # float32-representable
    # K_proj.bias: exactly zero by the softmax's shift invariance; what cancels there is sum_{b, l} gk[b, l, c]
    gk = grab["k"].grad                                                           # [batch, len, H d]
    arrays["k_bias_cancel"] = np.float64(gk.abs().sum(dim=(0, 1)).max().item())
    assert float(np.abs(arrays["grad." + pre + "mha.K_proj.bias"]).max()) <= 1e-12
    want = [pre + k for k in tr.LAYER_KEYS] if c["module"] == "layer" else tr.block_keys(c["depth"])
    assert sorted(n for n, _ in m.named_parameters()) == sorted(want), name
    path = os.path.join(tr.GOLDEN, "attn_train_%s.npz" % name)
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < MAX_FILE, (name, size)
    keep = tr.dropout_mask(c["Bt"] * C * Ld, p, seed, offset)
    info = dict(c, seed=seed, offset=offset, Ld=Ld, bytes=size, kept=int(keep.sum()), elements=int(keep.size),
                max_abs_out=float(out.abs().max()), stored=sorted(arrays))
    print("%-14s out %s max|out| %.3f kept %d / %d, %d bytes" % (name, tuple(out.shape), info["max_abs_out"], info["kept"],
                                                              info["elements"], size), flush=True)
    return info


def main():
    if not REF or not os.path.isdir(REF):
        raise SystemExit("set SRF_REFERENCE to a checkout of the reference implementation")
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    ref = load_ref()
    manifest = {"generator": "tools/make_golden_attentive_train.py", "torch": torch.__version__, "cases": {}}
    for index, (name, c) in enumerate(tr.CASES.items()):
        manifest["cases"][name] = run_case(ref, name, c, index)
    with open(tr.MANIFEST, "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", tr.MANIFEST)


if __name__ == "__main__":
    main()
