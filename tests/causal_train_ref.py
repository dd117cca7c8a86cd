"""A differentiable restatement of the causal SuDoRM-RF (v3) forward in plain torch (fp64 by default), and the cases of
tests/golden/CAUSAL_TRAIN_MANIFEST.json.  Shared by tools/make_golden_causal_train.py (which runs the REFERENCE on these cases
and stores its gradients) and by the tests: the CPU suite pins this restatement to the stored reference gradients, the GPU
suite then uses its autograd where no fixture exists (single kernels, fresh models, block scales).  Nothing here depends on the
reference.

Arithmetic (live taps only -- the reference multiplies the stored weights by causal_mask, so the masked taps get zero gradients
and are simply not read here):
  encoder    out[l] = sum_{a, k<K} w[n,a,k] x[a, h l + k - 2h],  h = K // 2, x zero-padded to a multiple of h 2^D
  block      u = W_p x / beta + b_p;  a_p = PReLU_p(u);  d_0 = dw_0 *_1 a_p + b_0;  d_k = dw_k *_2 a_{k-1} + b_k;  a_k = PReLU_k(d_k)
             (input index s j - 10 + t, t = 0..10, zero left of the row);  M[j] = a_0[j] + (a_1[j >> 1] + (...));
             x' = g alpha (W_r M + b_r) + x
  tail       m = W_m PReLU(x_U) + b_m;  out = conv_transpose(PReLU_c(m))[..., :T]
"""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests import causal_fixtures as cf

MANIFEST = os.path.join(cf.GOLDEN, "CAUSAL_TRAIN_MANIFEST.json")
DEFAULT_U8 = dict(cf.DEFAULTS, num_blocks=8)
TINY_S4 = dict(cf.TINY, num_sources=4)
WEIGHT_SEED, INPUT_SEED, GOUT_SEED = 7, 8, 13

# gradient fixtures: name -> (constructor kwargs, batch, T, kind); loss = (model(x) * gout).sum()
GRAD_CASES = {
    "causal_train_tiny": (cf.TINY, 2, 1001, "tiny"),
    "causal_train_a2_k11": (cf.TINY_A2, 3, 777, "tiny"),
    "causal_train_default_u8": (DEFAULT_U8, 2, 12000, "default"),
    # depth 8: 12001 samples pad to 1280 frames, two tiles of the fused backward; the first one's 1280-frame right halo of
    # g_merged is clipped at the end of the row
    "causal_train_tiny_d8": (cf.TINY_D8, 2, 12001, "tiny"),
}
# the bars of the GPU test per kind: check_grads_against_golden(tol, fp32_yardstick, flip_budget)
GRAD_BARS = {"tiny": (2e-4, 0.0, 0.0), "default": (2e-3, 4.0, 0.01)}
# trajectory fixture: name -> (constructor kwargs, batch, T, weight seed, first data seed); three steps of the FUSS loop body
TRAJ_CASES = {"causal_fuss_s4_traj": (TINY_S4, 2, 800, 7, 521)}
TRAJ_LR, TRAJ_CLIP = 1e-3, 5.0


def load_manifest():
    with open(MANIFEST) as f:
        return json.load(f)


def make_gout(shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(GOUT_SEED), dtype=torch.float64)


def grad_case(name):
    """(cfg, state dict (numpy float32), mixture (numpy float32), gout (torch float64)) of a gradient fixture."""
    from oracle.weights import make_mixture
    cfg, batch, T, _ = GRAD_CASES[name]
    sd = cf.make_state_dict(cfg, WEIGHT_SEED)
    x = make_mixture(batch, T, INPUT_SEED, channels=cfg["in_audio_channels"])
    return cfg, sd, x, make_gout((batch, cfg["num_sources"] * cfg["in_audio_channels"], T))


def padded_length(cfg, T):
    n = (cfg["enc_kernel_size"] // 2) * 2 ** cfg["upsampling_depth"]
    return n if T < n else -(-T // n) * n


def dwconv(x, w, b, stride):
    """Causal depthwise k = 21 conv on its 11 live taps: y[c, j] = b[c] + sum_{t<=10} w[c, 0, t] x[c, stride j - 10 + t]."""
    return F.conv1d(F.pad(x, (10, 0)), w[..., :11], b, stride=stride, groups=x.shape[1])


def pyramid(u, a_p, ws, bs, slopes):
    """merged [Bt, C, L] from proj_1x1's pre-activation u: the D levels and the bottom-up nearest-x2 upsample-and-add."""
    acts, src = [], F.prelu(u, a_p)
    for k, (w, b, a) in enumerate(zip(ws, bs, slopes)):
        src = F.prelu(dwconv(src, w, b, 1 if k == 0 else 2), a)
        acts.append(src)
    acc = acts[-1]
    for a in reversed(acts[:-1]):
        acc = a + acc.repeat_interleave(2, dim=-1)
    return acc


def forward(cfg, sd, wav, scales=None):
    """CausalSuDORMRF(**cfg).forward(wav) with the weights sd (name -> tensor, any float dtype, may require grad).
    scales: [(alpha, beta)] per block, default all 1."""
    A, B, C, U, D, K, N, S = (cfg[f] for f in cf.FIELDS)
    h, T = K // 2, wav.shape[-1]
    x = F.pad(wav, (2 * h, padded_length(cfg, T) - T))
    x = F.conv1d(x, sd["encoder.weight"][..., :K], stride=h)
    x = F.conv1d(x, sd["bottleneck.weight"], sd["bottleneck.bias"])
    for i in range(U):
        p = "sm.%d." % i
        alpha, beta = scales[i] if scales is not None else (1.0, 1.0)
        u = F.conv1d(x / beta, sd[p + "proj_1x1.conv.weight"], sd[p + "proj_1x1.conv.bias"])
        q = [p + "spp_dw.%d." % k for k in range(D)]
        merged = pyramid(u, sd[p + "proj_1x1.act.weight"], [sd[v + "conv.weight"] for v in q], [sd[v + "conv.bias"] for v in q],
                         [sd[v + "act.weight"] for v in q])
        x = F.conv1d(merged, sd[p + "res_conv.weight"], sd[p + "res_conv.bias"]) * sd[p + "skipinit_gain"] * alpha + x
    m = F.conv1d(F.prelu(x, sd["mask_net.0.weight"]), sd["mask_net.1.weight"], sd["mask_net.1.bias"])
    v = F.prelu(m, sd["mask_nl_class.weight"])
    out = F.conv_transpose1d(v, sd["decoder.weight"], stride=h, padding=h, output_padding=h - 1)
    return out[..., :T]


def leaves(sd_np, dtype=torch.float64):
    """name -> leaf tensor requiring grad, from a numpy state dict."""
    return {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in sd_np.items()}


def linear_loss_grads(cfg, sd_np, x_np, gout, dtype=torch.float64, scales=None):
    """(output, {name: gradient as float64 numpy}) of (forward(x) * gout).sum()."""
    sd = leaves(sd_np, dtype)
    out = forward(cfg, sd, torch.tensor(x_np, dtype=dtype), scales)
    (out * gout.to(dtype)).sum().backward()
    return out.detach(), {k: v.grad.double().numpy() for k, v in sd.items()}


def fuss_trajectory(cfg, sd_np, batches, dtype=torch.float64, lr=TRAJ_LR, clip=TRAJ_CLIP):
    """Three steps of the FUSS loop body on this restatement: the fixture's augmentation draws, mixture normalisation, forward,
    uniform mixture consistency, zero-reference SNR, clip_grad_norm_, Adam.  (losses, {name: final weights as numpy})."""
    from tests import fuss_fixtures as ff
    sd = leaves(sd_np, dtype)
    opt = torch.optim.Adam(list(sd.values()), lr=lr)
    losses = []
    for clean, src_b, src_s, gain in batches:
        opt.zero_grad()
        wavs, _, _, _ = ff.augment(clean, src_b, src_s, gain, dtype=torch.float32)
        wavs = wavs.to(dtype)
        mix = wavs.sum(-2, keepdim=True)
        mix = (mix - mix.mean(-1, keepdim=True)) / (mix.std(-1, keepdim=True) + 1e-9)
        rec = forward(cfg, sd, mix)
        rec = rec + (mix - rec.sum(1, keepdim=True)) / rec.shape[1]
        best, _, _, _ = ff.zeroref_snr(rec, wavs)
        loss = -best.mean()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(list(sd.values()), clip)
        opt.step()
        losses.append(float(loss.item()))
    return losses, {k: v.detach().double().numpy() for k, v in sd.items()}


def random_pyramid_case(Bt, C, L, D, seed, dtype=torch.float64):
    """Operands of one block's pyramid backward for the kernel tests: u (row 1 all zero), slopes of which one is negative and
    one exactly zero where the depth allows, weights with junk in the masked taps, channel 1's biases zero (so that every
    pre-activation of row 1 is exactly 0), and the upstream gradient g_merged."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    u = r(Bt, C, L)
    u[0, 1] = 0.0
    ws = [r(C, 1, 21) / 3.0 for _ in range(D)]
    bs = [0.2 * r(C) for _ in range(D)]
    for b in bs:
        b[1] = 0.0
    slopes = [torch.tensor([0.25 + 0.05 * k], dtype=torch.float64) for k in range(D)]
    slopes[0][0] = -0.3
    if D > 1:
        slopes[D - 1][0] = 0.0
    a_p = torch.tensor([0.2 if D > 1 else 0.0], dtype=torch.float64)
    gm = r(Bt, C, L)
    cast = lambda t: t.to(dtype)
    return cast(u), cast(a_p), [cast(w) for w in ws], [cast(b) for b in bs], [cast(s) for s in slopes], cast(gm)


def pyramid_grads(u, a_p, ws, bs, slopes, gm):
    """Autograd of (pyramid(...) * gm).sum(): dict with gu, da_p, dw[k], db[k], ds[k] (same dtype as the operands)."""
    u, a_p = u.clone().requires_grad_(), a_p.clone().requires_grad_()
    ws = [w.clone().requires_grad_() for w in ws]
    bs = [b.clone().requires_grad_() for b in bs]
    slopes = [s.clone().requires_grad_() for s in slopes]
    (pyramid(u, a_p, ws, bs, slopes) * gm).sum().backward()
    return {"gu": u.grad, "da_p": a_p.grad, "dw": [w.grad for w in ws], "db": [b.grad for b in bs], "ds": [s.grad for s in slopes]}


def levels(u, a_p, ws, bs, slopes):
    """The pre-activations d_k of the pyramid (what the training forward saves)."""
    out, src = [], F.prelu(u, a_p)
    for k, (w, b, a) in enumerate(zip(ws, bs, slopes)):
        d = dwconv(src, w, b, 1 if k == 0 else 2)
        out.append(d)
        src = F.prelu(d, a)
    return out
