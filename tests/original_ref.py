"""Original SuDoRM-RF forward restated in plain torch on the CPU (fp32 or fp64), from the formulas of DESIGN.md section 18 --
the yardstick of the GPU tests at shapes that have no golden.  tests/test_original_host.py pins it to the reference's own outputs
(tests/golden/orig_*.npz).  The mask layer is written as the Toeplitz GEMM the HIP path runs (tests/original_fixtures.toeplitz,
itself pinned to torch's conv2d), the grouped decoder as S separate transposed convolutions.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests.original_fixtures import toeplitz


def gn(x, weight, bias):
    """GroupNorm(1, C, eps=1e-8): one mean / biased variance per example over (C, L)."""
    m = x.mean((1, 2), keepdim=True)
    v = ((x - m) ** 2).mean((1, 2), keepdim=True)
    return (x - m) / torch.sqrt(v + 1e-8) * weight[None, :, None] + bias[None, :, None]


def prelu_c(x, slopes):
    """Per-channel PReLU.  The value at 0 is 0 either way; under autograd the branch decides the subgradient there, and it is
    torch's own (F.prelu: the slope at x == 0 and at -0.0)."""
    return torch.where(x > 0, x, x * slopes[None, :, None])


def block(x, sd, p, D):
    g = lambda t, q: gn(t, sd[p + q + ".weight"], sd[p + q + ".bias"])
    C = sd[p + "proj_1x1.conv.weight"].shape[0]
    a = F.conv1d(x, sd[p + "proj_1x1.conv.weight"], sd[p + "proj_1x1.conv.bias"])
    y = prelu_c(g(a, "proj_1x1.norm"), sd[p + "proj_1x1.act.weight"])
    levels = []
    for k in range(D):
        q = "spp_dw.%d." % k
        y = F.conv1d(y, sd[p + q + "conv.weight"], sd[p + q + "conv.bias"], stride=1 if k == 0 else 2, padding=2, groups=C)
        y = g(y, q + "norm")
        levels.append(y)
    m = levels[-1]
    for k in range(D - 2, -1, -1):
        m = levels[k] + m.repeat_interleave(2, dim=-1)
    e = prelu_c(g(m, "final_norm.norm"), sd[p + "final_norm.act.weight"])
    gg = g(F.conv1d(e, sd[p + "conv_1x1_exp.conv.weight"], sd[p + "conv_1x1_exp.conv.bias"]), "conv_1x1_exp.norm")
    return prelu_c(g(gg + x, "module_act.norm"), sd[p + "module_act.act.weight"])


def forward(cfg, sd, wav, dtype=torch.float64, taps=None):
    """cfg: the constructor kwargs (tests/original_fixtures.py), sd: key -> ndarray / tensor, wav: [batch, 1, T].  Returns
    [batch, S, T] as a `dtype` tensor.  taps (a dict): receives "block0" (the first block's output) and "z" (the mask logits
    [batch, S, N, L] before the softmax)."""
    tz, tb = toeplitz(np.asarray(sd["m.weight"]), np.asarray(sd["m.bias"]))
    sd = {k: torch.as_tensor(v).to(dtype) for k, v in sd.items()}
    tz, tb = torch.as_tensor(tz).to(dtype), torch.as_tensor(tb).to(dtype)
    wav = torch.as_tensor(wav).to(dtype)
    K, D, U, N, S, B = (cfg[f] for f in ("enc_kernel_size", "upsampling_depth", "num_blocks", "enc_num_basis", "num_sources",
                                         "out_channels"))
    T = wav.shape[-1]
    lcm = math.lcm(K // 2, 2 ** D)
    if T % lcm:
        wav = F.pad(wav, (0, lcm - T % lcm))
    s = torch.relu(F.conv1d(wav, sd["encoder.0.weight"], sd["encoder.0.bias"], stride=K // 2, padding=K // 2))
    x = F.conv1d(gn(s, sd["ln.weight"], sd["ln.bias"]), sd["l1.weight"], sd["l1.bias"])
    for i in range(U):
        x = block(x, sd, "sm.%d." % i, D)
        if taps is not None and i == 0:
            taps["block0"] = x
    if B != N:
        x = F.conv1d(x, sd["reshape_before_masks.weight"], sd["reshape_before_masks.bias"])
    z = (torch.einsum("rn,bnl->brl", tz, x) + tb[None, :, None]).view(x.shape[0], S, N, -1)
    if taps is not None:
        taps["z"] = z
    p = torch.sigmoid(z) if S == 1 else torch.softmax(z, dim=1)
    v = p * s.unsqueeze(1)
    w = sd["decoder.weight"].view(S, N, 1, K)
    est = torch.cat([F.conv_transpose1d(v[:, j], w[j], sd["decoder.bias"][j:j + 1], stride=K // 2, padding=K // 2,
                                        output_padding=K // 2 - 1) for j in range(S)], dim=1)
    return est[..., :T]


def separate(cfg, sd, mixture, mixture_consistency=False, dtype=torch.float64):
    """The caller-side recipe around forward(): per-example mean / unbiased std, forward, rescale and, on request, mixture
    consistency (uniform weights) of the rescaled estimates against the normalised mixture -- the recipe as srf_separate has it
    for every variant.  mixture: [batch, 1, T]."""
    x = torch.as_tensor(mixture).to(dtype)
    m = x.mean(-1, keepdim=True)
    sdev = x.std(-1, keepdim=True)
    norm = (x - m) / (sdev + 1e-9)
    est = forward(cfg, sd, norm, dtype) * sdev + m
    if mixture_consistency:
        est = est + (norm - est.sum(1, keepdim=True)) / est.shape[1]
    return est
