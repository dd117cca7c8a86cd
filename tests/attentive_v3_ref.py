"""Attentive SuDoRM-RF (v3) forward restated in plain torch on the CPU (fp32 or fp64), from the formulas of DESIGN.md
section 17 -- the yardstick of the GPU tests at shapes that have no golden.  tests/test_attentive_v3_host.py pins it to the
reference's own outputs (tests/golden/attn3_*.npz).  `heads` is an argument (4 in every model the reference builds), the head
dimension follows from the weights.  The shared pieces (attention, GlobLN, PReLU) are those of tests/attentive_ref.py.
"""
import math

import torch
import torch.nn.functional as F

from tests.attentive_ref import attention, gln, prelu


def resampler(q, v, sd, p, heads):
    """q: [B, C, Lq], v: [B, C, Lk], both normalised; p: key prefix 'sm.i.attentive_resamplers.r.'.  The position table goes on
    v only; q is the residual."""
    Lk = v.shape[-1]
    vp = v + sd[p + "pos_enc.pe"][0, :Lk, :].t()[None]
    lin = lambda n, x: F.conv1d(x, sd[p + "mha.%s_proj.weight" % n][:, :, None], sd[p + "mha.%s_proj.bias" % n])
    o = attention(lin("Q", q), lin("K", vp), lin("V", vp), heads)
    y = q + F.conv1d(o, sd[p + "mha.O_proj.weight"][:, :, None], sd[p + "mha.O_proj.bias"])
    y = gln(y, sd[p + "out_mha_norm.gamma"], sd[p + "out_mha_norm.beta"])
    f = F.conv1d(y, sd[p + "ffn.conv.weight"], sd[p + "ffn.conv.bias"])
    f = prelu(gln(f, sd[p + "ffn.norm.gamma"], sd[p + "ffn.norm.beta"]), sd[p + "ffn.act.weight"])
    return gln(f + y, sd[p + "out_norm.gamma"], sd[p + "out_norm.beta"])


def block(x, sd, p, D, heads, taps=None):
    C = sd[p + "proj_1x1.conv.weight"].shape[0]
    y = F.conv1d(x, sd[p + "proj_1x1.conv.weight"], sd[p + "proj_1x1.conv.bias"])
    y = prelu(gln(y, sd[p + "proj_1x1.norm.gamma"], sd[p + "proj_1x1.norm.beta"]), sd[p + "proj_1x1.act.weight"])
    levels = []
    for k in range(D):
        q = p + "spp_dw.%d." % k
        y = F.conv1d(y, sd[q + "conv.weight"], sd[q + "conv.bias"], stride=1 if k == 0 else 2, padding=2, groups=C)
        y = gln(y, sd[q + "norm.gamma"], sd[q + "norm.beta"])
        levels.append(y)
    v = levels[D - 1]
    for r in range(D - 1):                      # resampler r: level D - 2 - r asks, the result so far answers
        q = levels[D - 2 - r]
        z = resampler(q, v, sd, p + "attentive_resamplers.%d." % r, heads)
        if taps is not None:
            taps.append((q, v, z))
        v = z
    e = prelu(gln(v, sd[p + "final_norm.norm.gamma"], sd[p + "final_norm.norm.beta"]), sd[p + "final_norm.act.weight"])
    return F.conv1d(e, sd[p + "res_conv.weight"], sd[p + "res_conv.bias"]) + x


def forward(cfg, sd, wav, dtype=torch.float64, taps=None, heads=4):
    """cfg: the constructor kwargs (tests/attentive_v3_fixtures.py), sd: key -> ndarray / tensor, wav: [batch, 1, T].
    Returns [batch, S, T] as a `dtype` tensor.  taps (a list): receives (q, v, output) of every resampler in the order they run."""
    sd = {k: torch.as_tensor(v).to(dtype) for k, v in sd.items()}
    wav = torch.as_tensor(wav).to(dtype)
    K, D, U, N, S = cfg["enc_kernel_size"], cfg["upsampling_depth"], cfg["num_blocks"], cfg["enc_num_basis"], cfg["num_sources"]
    T = wav.shape[-1]
    lcm = math.lcm(K // 2, 2 ** D)
    if T % lcm:
        wav = F.pad(wav, (0, lcm - T % lcm))
    s = F.conv1d(wav, sd["encoder.weight"], stride=K // 2, padding=K // 2)
    x = F.conv1d(gln(s, sd["ln.gamma"], sd["ln.beta"]), sd["bottleneck.weight"], sd["bottleneck.bias"])
    for i in range(U):
        x = block(x, sd, "sm.%d." % i, D, heads, taps)
    m = F.conv1d(prelu(x, sd["mask_net.0.weight"]), sd["mask_net.1.weight"], sd["mask_net.1.bias"])
    m = torch.relu(m.view(m.shape[0], S, N, -1)) * s.unsqueeze(1)
    est = F.conv_transpose1d(m.view(m.shape[0], S * N, -1), sd["decoder.weight"], stride=K // 2, padding=K // 2,
                             output_padding=K // 2 - 1)
    return est[..., :T]


def separate(cfg, sd, mixture, dtype=torch.float64, heads=4):
    """The caller-side recipe around forward(): per-example mean / unbiased std, forward, rescale.  mixture: [batch, 1, T]."""
    x = torch.as_tensor(mixture).to(dtype)
    m = x.mean(-1, keepdim=True)
    sdev = x.std(-1, keepdim=True)
    est = forward(cfg, sd, (x - m) / (sdev + 1e-9), dtype, heads=heads)
    return est * sdev + m
