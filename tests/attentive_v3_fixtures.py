"""Attentive SuDoRM-RF (v3) fixtures: the cases of tests/golden/ATTENTIVE_V3_MANIFEST.json and their weights / inputs.

Shared by the generator (tools/make_golden_attentive_v3.py, which runs the reference on the build host) and the tests (which
regenerate the same weights and inputs from (config, seed) and compare against the stored reference outputs).  Every
parameter is drawn at random as in tests/attentive_fixtures.py -- gammas, betas, PReLU slopes and biases included, so that no
norm is the identity; every resampler's position table ``pos_enc.pe`` too, each from its own stretch of the stream, so that a
kernel that recomputes sines, or reads another resampler's table, fails -- with scales that keep max |out| in [0.1, 10].
Q_proj / K_proj are drawn four times wider than the other linear layers: the logits then spread over several units and the
softmax is far from uniform.

The reference's ``SuDORMRF`` IGNORES its ``n_heads`` / ``att_dims`` arguments: every block is built with 4 heads of 256
channels (attentive_sudormrf_v3.py, ``SuDORMRF.__init__``).  HEADS / ATT_DIMS are what the blocks really have; the constructor
arguments of the cases are kept as the reference's callers would write them.
"""
import json
import os

import numpy as np

from tests.attentive_fixtures import (FIELDS, GAINS, GOLDEN, HEADS, ATT_DIMS, MAX_LEN, ROOT, make_distinct,  # noqa: F401
                                      make_mixture, padded_length, save_npz)

MANIFEST = os.path.join(GOLDEN, "ATTENTIVE_V3_MANIFEST.json")


def _cfg(B, C, U, D, N, H, d, S, K=21):
    return dict(out_channels=B, in_channels=C, num_blocks=U, upsampling_depth=D, enc_kernel_size=K, enc_num_basis=N,
                n_heads=H, att_dims=d, att_dropout=0.1, num_sources=S)


TINY = _cfg(32, 64, 2, 3, 64, 3, 16, 2)
TINY_K9 = dict(TINY, enc_kernel_size=9)
TINY_D1 = dict(TINY, upsampling_depth=1)
DEFAULT_U2 = _cfg(128, 512, 2, 4, 512, 4, 256, 2)
MAIN_U1 = _cfg(256, 512, 1, 5, 512, 3, 256, 4)           # the file's __main__ configuration with one block
# the whole-module pickle: 16 channels, one block, D = 2 -- one resampler, so one 5000 x 16 table (320 KB)
PICKLE = _cfg(16, 16, 1, 2, 32, 4, 256, 2)

# name -> (constructor kwargs, batch, T, weight seed, input seed)
CASES = {
    "attn3_tiny": (TINY, 2, 1001, 301, 301),
    "attn3_tiny_short": (TINY, 2, 50, 302, 302),
    "attn3_odd": (TINY_K9, 2, 100, 303, 303),
    "attn3_d1": (TINY_D1, 2, 333, 304, 304),
    "attn3_default_u2": (DEFAULT_U2, 2, 10400, 305, 305),
    "attn3_main_u1": (MAIN_U1, 1, 32079, 306, 306),
}
# positions of every level, as the issue pins them
LEVELS = {"attn3_tiny": [104, 52, 26], "attn3_tiny_short": [8, 4, 2], "attn3_odd": [26, 13, 7], "attn3_d1": [34],
          "attn3_default_u2": [1040, 520, 260, 130], "attn3_main_u1": [3216, 1608, 804, 402, 201]}
DIGEST_CONFIGS = {"tiny": TINY, "pickle": PICKLE}
PICKLE_SEED, PICKLE_BATCH, PICKLE_T, PICKLE_INPUT_SEED = 9, 2, 777, 307
DISTINCT_T, DISTINCT_SEED = 1001, 308                    # five distinct examples on the weights of attn3_tiny


def level_lengths(cfg, T):
    """Positions of level 0 .. D - 1: the encoder's frames, then the strided convolution's own ceil halving."""
    K = cfg["enc_kernel_size"]
    lv = [(padded_length(cfg, T) + 2 * (K // 2) - K) // (K // 2) + 1]
    for _ in range(1, cfg["upsampling_depth"]):
        lv.append((lv[-1] + 1) // 2)
    return lv


def schema(cfg):
    """[(state_dict key, shape)] of the attentive v3 SuDORMRF(**cfg), in state_dict order (buffers included)."""
    B, C, U, D, K, N = (cfg[f] for f in FIELDS[:6])
    S = cfg["num_sources"]
    HD = HEADS * ATT_DIMS
    out = [("encoder.weight", (N, 1, K)), ("ln.gamma", (N,)), ("ln.beta", (N,)), ("bottleneck.weight", (B, N, 1)),
           ("bottleneck.bias", (B,))]
    for i in range(U):
        p = "sm.%d." % i
        out += [(p + "proj_1x1.conv.weight", (C, B, 1)), (p + "proj_1x1.conv.bias", (C,)), (p + "proj_1x1.norm.gamma", (C,)),
                (p + "proj_1x1.norm.beta", (C,)), (p + "proj_1x1.act.weight", (1,))]
        for k in range(D):
            q = p + "spp_dw.%d." % k
            out += [(q + "conv.weight", (C, 1, 5)), (q + "conv.bias", (C,)), (q + "norm.gamma", (C,)), (q + "norm.beta", (C,))]
        out += [(p + "final_norm.norm.gamma", (C,)), (p + "final_norm.norm.beta", (C,)), (p + "final_norm.act.weight", (1,)),
                (p + "res_conv.weight", (B, C, 1)), (p + "res_conv.bias", (B,))]
        for r in range(D - 1):
            a = p + "attentive_resamplers.%d." % r
            for proj in "QKV":
                out += [(a + "mha.%s_proj.weight" % proj, (HD, C)), (a + "mha.%s_proj.bias" % proj, (HD,))]
            out += [(a + "mha.O_proj.weight", (C, HD)), (a + "mha.O_proj.bias", (C,)),
                    (a + "out_norm.gamma", (C,)), (a + "out_norm.beta", (C,)),
                    (a + "out_mha_norm.gamma", (C,)), (a + "out_mha_norm.beta", (C,)),
                    (a + "ffn.conv.weight", (C, C, 1)), (a + "ffn.conv.bias", (C,)), (a + "ffn.norm.gamma", (C,)),
                    (a + "ffn.norm.beta", (C,)), (a + "ffn.act.weight", (1,)), (a + "pos_enc.pe", (1, MAX_LEN, C))]
    out += [("mask_net.0.weight", (1,)), ("mask_net.1.weight", (S * N, B, 1)), ("mask_net.1.bias", (S * N,)),
            ("decoder.weight", (S * N, S, K))]
    return out


def make_state_dict(cfg, seed):
    """Ordered dict key -> float32 ndarray, every entry drawn from numpy's PCG64 stream of `seed` (so every resampler's table
    is a different stretch of it)."""
    rng = np.random.default_rng(seed)
    sd = {}
    for key, shape in schema(cfg):
        leaf = key.split(".")[-1]
        if leaf == "pe":
            w = rng.uniform(-1.0, 1.0, size=shape)
        elif leaf == "gamma":
            w = rng.uniform(0.5, 1.5, size=shape)
        elif leaf == "beta":
            w = rng.uniform(-0.3, 0.3, size=shape)
        elif shape == (1,):                                   # PReLU slopes
            w = rng.uniform(0.05, 0.45, size=shape)
        elif key in ("encoder.weight", "decoder.weight"):    # xavier-uniform (decoder: x 3, for max |out| >= 0.1 at every case)
            rf = shape[2]
            b = np.sqrt(6.0 / (shape[1] * rf + shape[0] * rf)) * (3.0 if key == "decoder.weight" else 1.0)
            w = rng.uniform(-b, b, size=shape)
        elif leaf == "weight":
            b = 1.0 / np.sqrt(float(np.prod(shape[1:])))
            if ".Q_proj." in key or ".K_proj." in key:
                b *= 4.0
            w = rng.uniform(-b, b, size=shape)
        elif leaf == "bias":
            w = rng.uniform(-0.2, 0.2, size=shape)
        else:
            raise KeyError(key)
        sd[key] = np.ascontiguousarray(w, dtype=np.float32)
    return sd


def make_input(name):
    _, batch, T, _, iseed = CASES[name]
    return make_mixture(batch, T, iseed)


def load_manifest():
    with open(MANIFEST) as f:
        return json.load(f)


def load_golden(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        return {k: z[k] for k in z.files}
