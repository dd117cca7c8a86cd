"""Attentive SuDoRM-RF (v2) forward restated in plain torch on the CPU (fp32 or fp64), from the formulas of DESIGN.md
section 16 -- the yardstick of the GPU tests at shapes that have no golden.  tests/test_attentive_host.py pins it to the
reference's own outputs (tests/golden/attn_*.npz).  `heads` is an argument (4 in every model the reference builds), the head
dimension follows from the weights: any (H, d) runs.
"""
import math

import torch
import torch.nn.functional as F


def attention(q, k, v, heads, scale=None):
    """q: [B, H d, Lq], k, v: [B, H d, Lk] -> [B, H d, Lq]; channel h d + j belongs to head h."""
    B, HD, Lq = q.shape
    d = HD // heads
    scale = 1.0 / math.sqrt(d) if scale is None else scale
    qh = (q * scale).reshape(B, heads, d, Lq)
    kh = k.reshape(B, heads, d, -1)
    vh = v.reshape(B, heads, d, -1)
    a = torch.softmax(torch.einsum("bhdl,bhds->bhls", qh, kh), dim=-1)
    return torch.einsum("bhls,bhds->bhdl", a, vh).reshape(B, HD, Lq)


def gln(x, gamma, beta):
    mean = x.mean(dim=(1, 2), keepdim=True)
    var = ((x - mean) ** 2).mean(dim=(1, 2), keepdim=True)
    return gamma[None, :, None] * ((x - mean) / (var + 1e-8).sqrt()) + beta[None, :, None]


def prelu(x, a):
    return torch.where(x >= 0, x, a * x)


def transformer_layer(a, sd, p, heads):
    """a: [B, C, Ld], the normalised deepest level; p: key prefix 'sm.i.attention.'."""
    Ld = a.shape[-1]
    x = a + sd[p + "pos_enc.pe"][0, :Ld, :].t()[None]
    lin = lambda n: F.conv1d(x, sd[p + "mha.%s_proj.weight" % n][:, :, None], sd[p + "mha.%s_proj.bias" % n])
    o = attention(lin("Q"), lin("K"), lin("V"), heads)
    y = x + F.conv1d(o, sd[p + "mha.O_proj.weight"][:, :, None], sd[p + "mha.O_proj.bias"])
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
    z = transformer_layer(levels[-1], sd, p + "attention.", heads)
    if taps is not None:
        taps.append((levels[-1], z))
    levels[-1] = z
    for _ in range(D - 1):
        top = levels.pop()
        levels[-1] = levels[-1] + top.repeat_interleave(2, dim=-1)
    e = prelu(gln(levels[0], sd[p + "final_norm.norm.gamma"], sd[p + "final_norm.norm.beta"]), sd[p + "final_norm.act.weight"])
    return F.conv1d(e, sd[p + "res_conv.weight"], sd[p + "res_conv.bias"]) + x


def forward(cfg, sd, wav, dtype=torch.float64, taps=None, heads=4):
    """cfg: the constructor kwargs (tests/attentive_fixtures.py), sd: key -> ndarray / tensor, wav: [batch, 1, T].
    Returns [batch, S, T] as a `dtype` tensor.  taps (a list): receives (transformer input, output) of every block.
    heads: 4 in every model the reference's SuDORMRF builds (it ignores n_heads / att_dims); the head dimension follows from
    the weights."""
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
