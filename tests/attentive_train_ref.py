"""Training restatements for the attentive transformer layer and U-block.

1. The dropout mask of srf_posenc_apply_dropout in numpy: `dropout_mask(n, p, seed, offset)`.  Element i keeps word i & 3 of
   Philox4x32-10 with the key {lo32(seed), hi32(seed)} on the counter {lo32(i >> 2), hi32(i >> 2), lo32(offset), hi32(offset)},
   kept where word >= floor(p 2^32) (64-bit comparison; the threshold from float32(p) in double, as the library forms it).
2. `layer_forward` / `block_forward`: TransformerLayer.forward and AttentiveUConvBlock.forward in torch operators (any dtype,
   differentiable by autograd) with an EXPLICIT keep mask, and `layer_backward` / `block_backward`: the backward chain of
   DESIGN.md section 16.2 in the order the HIP path runs it, in closed-form torch operators.  tests/test_transformer_train_host.py
   holds the chain against fp64 autograd of the forward and both against the reference-generated tests/golden/attn_train_*.npz.

Parameters travel as a dict of tensors under the module's own state_dict() keys ("mha.Q_proj.weight", ..., "pos_enc.pe" for a
layer; "proj_1x1.conv.weight", ..., "attention.pos_enc.pe" for a block).
"""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests import attentive_ref as ar

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = os.path.join(GOLDEN, "ATTENTIVE_TRAIN_MANIFEST.json")
EPS = 1e-8

# name: (module, Bt, emb / in_channels, heads, d_model, Ld (layer) or L (block), p, lazy norm (layer) / out_channels, depth (block))
CASES = {
    "tl_tiny": dict(module="layer", Bt=2, emb=24, heads=3, d_model=16, Ld=26, p=0.0, lazy=False),
    "tl_tiny_drop": dict(module="layer", Bt=2, emb=24, heads=3, d_model=16, Ld=26, p=0.1, lazy=False),
    "tl_lazy_drop": dict(module="layer", Bt=2, emb=24, heads=3, d_model=16, Ld=13, p=0.5, lazy=True),
    "tl_generic": dict(module="layer", Bt=2, emb=24, heads=2, d_model=24, Ld=25, p=0.1, lazy=False),
    "tl_mfma": dict(module="layer", Bt=2, emb=128, heads=2, d_model=64, Ld=40, p=0.1, lazy=False),
    "ab_d2": dict(module="block", Bt=2, out=16, emb=32, depth=2, L=24, heads=2, d_model=16, p=0.1),
    "ab_d3_odd": dict(module="block", Bt=2, out=16, emb=32, depth=3, L=52, heads=2, d_model=16, p=0.5),
}
LAYER_KEYS = ["mha.%s_proj.%s" % (m, w) for m in "QKVO" for w in ("weight", "bias")] + [
    "out_norm.gamma", "out_norm.beta", "out_mha_norm.gamma", "out_mha_norm.beta", "ffn.conv.weight", "ffn.conv.bias",
    "ffn.norm.gamma", "ffn.norm.beta", "ffn.act.weight"]


def block_keys(D):
    keys = ["proj_1x1.conv.weight", "proj_1x1.conv.bias", "proj_1x1.norm.gamma", "proj_1x1.norm.beta", "proj_1x1.act.weight"]
    for k in range(D):
        keys += ["spp_dw.%d.%s" % (k, s) for s in ("conv.weight", "conv.bias", "norm.gamma", "norm.beta")]
    keys += ["final_norm.norm.gamma", "final_norm.norm.beta", "final_norm.act.weight", "res_conv.weight", "res_conv.bias"]
    return keys + ["attention." + k for k in LAYER_KEYS]


# ---- 1. the mask -----------------------------------------------------------------------------------------------------
M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
LO = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Counter words as uint64 arrays holding 32-bit values, key words as Python ints -> the four output words (uint64 arrays)."""
    for r in range(10):
        p0, p1 = M0 * c0, M1 * c2                       # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ np.uint64(k0), p1 & LO, (p0 >> S32) ^ c3 ^ np.uint64(k1), p0 & LO
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def threshold(p):
    return int(np.floor(np.float64(np.float32(p)) * 4294967296.0))


def dropout_words(n, seed, offset, start=0):
    """The 32-bit word of elements start .. start + n - 1 (uint64 array)."""
    i = np.arange(start, start + n, dtype=np.uint64)
    blk = i >> np.uint64(2)
    full = lambda v: np.full(n, v, dtype=np.uint64)
    w = philox4x32_10(blk & LO, blk >> S32, full(offset & 0xFFFFFFFF), full((offset >> 32) & 0xFFFFFFFF),
                      seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return np.choose((i & np.uint64(3)).astype(np.int64), w)


def dropout_mask(n, p, seed, offset, start=0):
    """keep[i] (bool) for elements start .. start + n - 1."""
    return dropout_words(n, seed, offset, start) >= np.uint64(threshold(p))


def inv_keep(p):
    """The library's scale: the fp32 expression 1.f / (1.f - p) (inf at p = 1, never applied to a dropped element)."""
    with np.errstate(divide="ignore"):
        return np.float32(1) / (np.float32(1) - np.float32(p))


def keep_tensor(shape, p, seed, offset, dtype=torch.float64):
    """The keep mask of a [Bt, C, L] tensor times inv_keep, as the multiplier the reference's dropout stand-in applies
    (dropped: exactly 0, also at p = 1)."""
    keep = dropout_mask(int(np.prod(shape)), p, seed, offset).reshape(shape)
    scale = np.where(keep, np.float64(inv_keep(p)) if p < 1 else 0.0, 0.0)
    return torch.from_numpy(scale).to(dtype)


# ---- 2. forward ------------------------------------------------------------------------------------------------------
def _gln_parts(x):
    mean = x.mean(dim=(1, 2), keepdim=True)
    rstd = 1.0 / (((x - mean) ** 2).mean(dim=(1, 2), keepdim=True) + EPS).sqrt()
    return (x - mean) * rstd, rstd


def layer_forward(a, P, heads, mult=None, in_norm=None, saved=None):
    """a [Bt, C, Ld]; mult: keep * inv_keep [Bt, C, Ld] or None (no dropout); in_norm = (gamma, beta) of the level's lazy
    GlobLN or None.  saved (a dict) receives the tensors the backward chain reads."""
    Ld = a.shape[-1]
    xn = ar.gln(a, *in_norm) if in_norm is not None else a
    xp = xn + P["pos_enc.pe"][0, :Ld, :].t()[None]
    if mult is not None:
        xp = xp * mult
    wqkv = torch.cat([P["mha.%s_proj.weight" % n] for n in "QKV"], 0)
    bqkv = torch.cat([P["mha.%s_proj.bias" % n] for n in "QKV"], 0)
    q, k, v = F.conv1d(xp, wqkv[:, :, None], bqkv).chunk(3, dim=1)
    o = ar.attention(q, k, v, heads)
    y = xp + F.conv1d(o, P["mha.O_proj.weight"][:, :, None], P["mha.O_proj.bias"])
    yn = ar.gln(y, P["out_mha_norm.gamma"], P["out_mha_norm.beta"])
    f = F.conv1d(yn, P["ffn.conv.weight"], P["ffn.conv.bias"])
    z = ar.prelu(ar.gln(f, P["ffn.norm.gamma"], P["ffn.norm.beta"]), P["ffn.act.weight"]) + yn
    if saved is not None:
        saved.update(a=a, xp=xp, q=q, k=k, v=v, o=o, y=y, yn=yn, f=f, z=z, mult=mult)
    return ar.gln(z, P["out_norm.gamma"], P["out_norm.beta"])


def block_forward(x, P, D, heads, mult=None, saved=None):
    """x [Bt, out_channels, L]; mult as in layer_forward, for the deepest level [Bt, in_channels, L >> (D - 1)]."""
    C = P["proj_1x1.conv.weight"].shape[0]
    y1 = F.conv1d(x, P["proj_1x1.conv.weight"], P["proj_1x1.conv.bias"])
    src = ar.prelu(ar.gln(y1, P["proj_1x1.norm.gamma"], P["proj_1x1.norm.beta"]), P["proj_1x1.act.weight"])
    pre, normed = [], []
    for k in range(D):
        q = "spp_dw.%d." % k
        d_k = F.conv1d(src, P[q + "conv.weight"], P[q + "conv.bias"], stride=1 if k == 0 else 2, padding=2, groups=C)
        pre.append(d_k)
        if k < D - 1:
            src = ar.gln(d_k, P[q + "norm.gamma"], P[q + "norm.beta"])
            normed.append(src)
    q = "spp_dw.%d." % (D - 1)
    lp = {k[len("attention."):]: v for k, v in P.items() if k.startswith("attention.")}
    lsaved = {} if saved is not None else None
    top = layer_forward(pre[-1], lp, heads, mult, (P[q + "norm.gamma"], P[q + "norm.beta"]), lsaved)
    for k in range(D - 2, -1, -1):
        top = normed[k] + top.repeat_interleave(2, dim=-1)
    e = ar.prelu(ar.gln(top, P["final_norm.norm.gamma"], P["final_norm.norm.beta"]), P["final_norm.act.weight"])
    if saved is not None:
        saved.update(x=x, y1=y1, pre=pre, merged=top, e=e, layer=lsaved)
    return F.conv1d(e, P["res_conv.weight"], P["res_conv.bias"]) + x


# ---- 3. the backward chain, in the HIP path's order ------------------------------------------------------------------------
def gln_bwd(gout, x, gamma, beta, slope=None, gout2=None):
    """srf_gln_bwd: gout (+ gout2) w.r.t. the normalised (activated) tensor -> (gx, dgamma, dbeta, dslope)."""
    g = gout if gout2 is None else gout + gout2
    xh, rstd = _gln_parts(x)
    dslope = None
    if slope is not None:
        yv = gamma[None, :, None] * xh + beta[None, :, None]
        dslope = (g * yv * (yv < 0)).sum().reshape(1)
        g = torch.where(yv >= 0, g, g * slope)
    dgamma, dbeta = (g * xh).sum(dim=(0, 2)), g.sum(dim=(0, 2))
    gh = g * gamma[None, :, None]
    gx = (gh - gh.mean(dim=(1, 2), keepdim=True) - xh * (gh * xh).mean(dim=(1, 2), keepdim=True)) * rstd
    return gx, dgamma, dbeta, dslope


def pw_bwd(g, x, w):
    """a 1x1 conv y = W x + b: -> (dW [Cout, Cin], db, W^T g)"""
    return torch.einsum("bml,bnl->mn", g, x), g.sum(dim=(0, 2)), torch.einsum("mn,bml->bnl", w.reshape(w.shape[0], -1), g)


def attention_bwd(q, k, v, go, heads):
    B, HD, Lq = q.shape
    d = HD // heads
    scale = d ** -0.5
    h = lambda t: t.reshape(B, heads, d, -1)
    qh, kh, vh, gh = h(q), h(k), h(v), h(go)
    P = torch.softmax(torch.einsum("bhdl,bhds->bhls", qh * scale, kh), dim=-1)
    gv = torch.einsum("bhls,bhdl->bhds", P, gh)
    dP = torch.einsum("bhdl,bhds->bhls", gh, vh)
    dS = P * (dP - (P * dP).sum(-1, keepdim=True))
    gq = scale * torch.einsum("bhls,bhds->bhdl", dS, kh)
    gk = scale * torch.einsum("bhls,bhdl->bhds", dS, qh)
    return gq.reshape(q.shape), gk.reshape(k.shape), gv.reshape(v.shape)


def layer_backward(g, P, heads, S, in_norm=None):
    """g: the gradient of layer_forward's output, S: its `saved` -> ({key: gradient}, gx, gn); with in_norm the dict also
    holds "in_norm.gamma" / "in_norm.beta".  gn is the gradient w.r.t. the normalised input (= gx without in_norm)."""
    G = {}
    gz, G["out_norm.gamma"], G["out_norm.beta"], _ = gln_bwd(g, S["z"], P["out_norm.gamma"], P["out_norm.beta"])
    gf, G["ffn.norm.gamma"], G["ffn.norm.beta"], G["ffn.act.weight"] = gln_bwd(
        gz, S["f"], P["ffn.norm.gamma"], P["ffn.norm.beta"], P["ffn.act.weight"])
    dw, G["ffn.conv.bias"], g_yn = pw_bwd(gf, S["yn"], P["ffn.conv.weight"])
    G["ffn.conv.weight"] = dw[:, :, None]
    gy, G["out_mha_norm.gamma"], G["out_mha_norm.beta"], _ = gln_bwd(gz, S["y"], P["out_mha_norm.gamma"],
                                                                     P["out_mha_norm.beta"], gout2=g_yn)
    G["mha.O_proj.weight"], G["mha.O_proj.bias"], go = pw_bwd(gy, S["o"], P["mha.O_proj.weight"])
    gqkv = torch.cat(attention_bwd(S["q"], S["k"], S["v"], go, heads), 1)
    wqkv = torch.cat([P["mha.%s_proj.weight" % n] for n in "QKV"], 0)
    dw, db, gxp = pw_bwd(gqkv, S["xp"], wqkv)
    for n, w, b in zip("QKV", dw.chunk(3, 0), db.chunk(3, 0)):
        G["mha.%s_proj.weight" % n], G["mha.%s_proj.bias" % n] = w, b
    gxp = gxp + gy
    gn = gxp if S["mult"] is None else gxp * S["mult"]
    gx = gn
    if in_norm is not None:
        gx, G["in_norm.gamma"], G["in_norm.beta"], _ = gln_bwd(gn, S["a"], *in_norm)
    return G, gx, gn


def dwconv5_bwd(gd, xin_act, w, stride):
    """-> (gradient w.r.t. the conv's (already normalised / activated) input, dw, dbias): the transposed convolution and the
    correlation, by the operators' own definitions"""
    C, Lin = w.shape[0], xin_act.shape[-1]
    gin = F.conv_transpose1d(gd, w, stride=stride, padding=2, groups=C, output_padding=Lin - ((gd.shape[-1] - 1) * stride + 1))
    xpad = F.pad(xin_act, (2, 2))
    dw = torch.stack([(gd * xpad[..., t:t + (gd.shape[-1] - 1) * stride + 1:stride]).sum(dim=(0, 2)) for t in range(5)], -1)
    return gin, dw[:, None, :], gd.sum(dim=(0, 2))


def block_backward(g, P, D, heads, S):
    """g: the gradient of block_forward's output, S: its `saved` -> ({key: gradient}, gx)"""
    G = {}
    dw, G["res_conv.bias"], ge = pw_bwd(g, S["e"], P["res_conv.weight"])
    G["res_conv.weight"] = dw[:, :, None]
    gm, G["final_norm.norm.gamma"], G["final_norm.norm.beta"], G["final_norm.act.weight"] = gln_bwd(
        ge, S["merged"], P["final_norm.norm.gamma"], P["final_norm.norm.beta"], P["final_norm.act.weight"])
    parts = [gm]
    for k in range(1, D):                                 # srf_merge_bwd: the chain of pair sums
        parts.append(parts[-1].reshape(*parts[-1].shape[:2], -1, 2).sum(-1))
    q = "spp_dw.%d." % (D - 1)
    lp = {k[len("attention."):]: v for k, v in P.items() if k.startswith("attention.")}
    LG, gd, _ = layer_backward(parts[D - 1], lp, heads, S["layer"], (P[q + "norm.gamma"], P[q + "norm.beta"]))
    G[q + "norm.gamma"], G[q + "norm.beta"] = LG.pop("in_norm.gamma"), LG.pop("in_norm.beta")
    G.update({"attention." + k: v for k, v in LG.items()})
    for k in range(D - 1, -1, -1):
        q = "spp_dw.%d." % k
        if k < D - 1:
            gd, G[q + "norm.gamma"], G[q + "norm.beta"], _ = gln_bwd(parts[k], S["pre"][k], P[q + "norm.gamma"],
                                                                     P[q + "norm.beta"], gout2=gin)
        if k:
            r = "spp_dw.%d." % (k - 1)
            xin = ar.gln(S["pre"][k - 1], P[r + "norm.gamma"], P[r + "norm.beta"])
        else:
            xin = ar.prelu(ar.gln(S["y1"], P["proj_1x1.norm.gamma"], P["proj_1x1.norm.beta"]), P["proj_1x1.act.weight"])
        gin, G[q + "conv.weight"], G[q + "conv.bias"] = dwconv5_bwd(gd, xin, P[q + "conv.weight"], 1 if k == 0 else 2)
    gy1, G["proj_1x1.norm.gamma"], G["proj_1x1.norm.beta"], G["proj_1x1.act.weight"] = gln_bwd(
        gin, S["y1"], P["proj_1x1.norm.gamma"], P["proj_1x1.norm.beta"], P["proj_1x1.act.weight"])
    dw, G["proj_1x1.conv.bias"], gx = pw_bwd(gy1, S["x"], P["proj_1x1.conv.weight"])
    G["proj_1x1.conv.weight"] = dw[:, :, None]
    return G, gx + g


# ---- 4. fixtures -------------------------------------------------------------------------------------------------------
def manifest():
    with open(MANIFEST) as f:
        return json.load(f)


def load_case(name):
    """-> {array name: ndarray}: "x" (the input), "gout", "out", "p", "seed", "offset", "pe" ([Ld, C]), "param.<key>",
    "grad.x", "grad.<key>" (float32-rounded; a lazy layer also "param.in_norm.gamma" / "...beta" and their gradients),
    "k_bias_cancel" (max_c sum_{b, l} |gk[b, c, l]| of the reference: the size of what cancels in K_proj.bias's exact zero)."""
    with np.load(os.path.join(GOLDEN, "attn_train_%s.npz" % name)) as z:
        return {k: z[k] for k in z.files}


def case_params(arrays, dtype=torch.float64, max_len=None):
    """The parameter dict of a fixture; pe: the stored rows first, NaN behind them up to max_len (a read past Ld shows)."""
    P = {k[len("param."):]: torch.from_numpy(v).to(dtype) for k, v in arrays.items() if k.startswith("param.")}
    rows = torch.from_numpy(arrays["pe"]).to(dtype)
    pe = torch.full((1, max_len or rows.shape[0], rows.shape[1]), float("nan"), dtype=dtype)
    pe[0, :rows.shape[0]] = rows
    key = "attention.pos_enc.pe" if any(k.startswith("attention.") for k in P) else "pos_enc.pe"
    P[key] = pe
    return P
