"""Attentive SuDoRM-RF (v2) fixtures: the cases of tests/golden/ATTENTIVE_MANIFEST.json and their weights / inputs.

Shared by the generator (tools/make_golden_attentive.py, which runs the reference on the build host) and the tests (which
regenerate the same weights and inputs from (config, seed) and compare against the stored reference outputs).  Every
parameter is drawn at random -- gammas, betas, PReLU slopes and biases included, so that no norm is the identity, and the
position tables ``pos_enc.pe`` too, so that a kernel that recomputes sines instead of reading the buffer fails -- with scales
that keep max |out| in [0.1, 10].  Q_proj / K_proj are drawn four times wider than the other linear layers: the logits then
spread over several units and the softmax is far from uniform.

The reference's ``SuDORMRF`` IGNORES its ``n_heads`` / ``att_dims`` arguments: every block is built with 4 heads of 256
channels (attentive_sudormrf_v2.py, ``SuDORMRF.__init__``).  HEADS / ATT_DIMS below are what the blocks really have; the
constructor arguments of the cases are kept as the reference's callers would write them.
"""
import io
import json
import os
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MANIFEST = os.path.join(GOLDEN, "ATTENTIVE_MANIFEST.json")

FIELDS = ("out_channels", "in_channels", "num_blocks", "upsampling_depth", "enc_kernel_size", "enc_num_basis", "n_heads",
          "att_dims", "att_dropout", "num_sources")
HEADS, ATT_DIMS, MAX_LEN = 4, 256, 5000     # what SuDORMRF builds whatever n_heads / att_dims say


def _cfg(B, C, U, D, N, H, d, S):
    return dict(out_channels=B, in_channels=C, num_blocks=U, upsampling_depth=D, enc_kernel_size=21, enc_num_basis=N,
                n_heads=H, att_dims=d, att_dropout=0.1, num_sources=S)


TINY = _cfg(32, 64, 2, 3, 64, 3, 16, 2)
DEFAULT_U2 = _cfg(128, 512, 2, 4, 512, 4, 256, 2)
MAIN_U2 = _cfg(256, 512, 2, 5, 512, 3, 256, 4)
# the whole-module pickle: one block of 16 channels, so that its two 5000-row tables stay inside a small committed file
PICKLE = _cfg(16, 16, 1, 3, 32, 4, 256, 2)

# name -> (constructor kwargs, batch, T, weight seed, input seed)
CASES = {
    "attn_tiny": (TINY, 2, 1001, 201, 201),
    "attn_tiny_short": (TINY, 2, 50, 202, 202),
    "attn_default_u2": (DEFAULT_U2, 4, 10400, 203, 203),
    "attn_main_u2": (MAIN_U2, 2, 32079, 204, 204),
}
# Deepest levels of Ld % 4 == 0 positions: only there do the transformer layer's three GEMMs (Q/K/V, O_proj, ffn: 1x1 convs of
# length Ld) leave the scalar kernel -- every case above but the 16-channel pickle has Ld % 4 != 0.  No goldens: the yardstick is
# tests/attentive_ref.py in fp64.
#   TINY (D = 3: Ld = Tp / 40) on the weights of attn_tiny: (T, batch, Ld, input seed) -- one position group | a multiple of 4
#   that is none of 8 (Tp = 1120) | 4 short of a 128-column tile | exactly one | one plus a 4-column tile | batch 1
TINY_GRID = ((160, 2, 4, 240), (1100, 2, 28, 241), (4960, 2, 124, 242), (5120, 2, 128, 243), (5280, 2, 132, 244),
             (1100, 1, 28, 245))
#   WIDE: the default model's channel counts (C = 512, 4 heads of 256) at D = 2, so that Ld = Tp / 20 and a batch that gives the
#   layer's GEMMs as many 256 x 128 tiles as the chip has CUs stays small: T = 2640 -> L = 264, Ld = 132 = 128 + 4
WIDE = _cfg(128, 512, 2, 2, 128, 4, 256, 2)
WIDE_T, WIDE_LD, WIDE_WSEED, WIDE_INPUT_SEED = 2640, 132, 206, 206
GAINS = (1.0, 0.5, 2.0, 1.5, 0.8)          # per-example gains of the distinct-example batches, cycled
DIGEST_CONFIGS = {"tiny": TINY, "pickle": PICKLE}
PICKLE_SEED, PICKLE_BATCH, PICKLE_T, PICKLE_INPUT_SEED = 7, 2, 777, 205


def padded_length(cfg, T):
    """pad_to_appropriate_length: up to a multiple of lcm(K // 2, 2^D), only when T is not one already."""
    lcm = int(np.lcm(cfg["enc_kernel_size"] // 2, 2 ** cfg["upsampling_depth"]))
    return T + lcm - T % lcm if T % lcm else T


def deepest_length(cfg, T):
    K = cfg["enc_kernel_size"]
    L = (padded_length(cfg, T) + 2 * (K // 2) - K) // (K // 2) + 1
    return L >> (cfg["upsampling_depth"] - 1)


def schema(cfg):
    """[(state_dict key, shape)] of the attentive SuDORMRF(**cfg), in state_dict order (buffers included)."""
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
        a = p + "attention."
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
    """Ordered dict key -> float32 ndarray, every entry drawn from numpy's PCG64 stream of `seed`."""
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


def make_mixture(batch, T, seed):
    """Synthetic mixtures [batch, 1, T], normalised per example (the stream of oracle.weights.make_mixture)."""
    rng = np.random.default_rng(1000003 * (seed + 1) + 17)
    x = rng.standard_normal(size=(batch, 1, T))
    if T > 1:
        x = (x - x.mean(-1, keepdims=True)) / (x.std(-1, ddof=1, keepdims=True) + 1e-9)
    return np.ascontiguousarray(x, dtype=np.float32)


def make_distinct(batch, T, seed):
    """make_mixture with example b scaled by GAINS[b % 5]: rows that differ in level as well as in content."""
    gains = np.array([GAINS[b % len(GAINS)] for b in range(batch)], dtype=np.float32)
    return make_mixture(batch, T, seed) * gains[:, None, None]


def make_input(name):
    _, batch, T, _, iseed = CASES[name]
    return make_mixture(batch, T, iseed)


def load_manifest():
    with open(MANIFEST) as f:
        return json.load(f)


def load_golden(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def save_npz(path, arrays):
    """np.savez's layout with a fixed member timestamp, so that regenerating writes identical bytes."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_STORED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())
