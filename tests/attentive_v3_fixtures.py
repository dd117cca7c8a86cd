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

# ---- configurations without a golden (reference: tests/attentive_v3_ref.py in fp64) -----------------------------------------------
# WIDE3: the default model's channel counts at D = 3, U = 2 (two resamplers in each of two blocks: block AND resampler index of
# every packed image vary); T = 5280 gives levels 528 / 264 / 132, all multiples of 4, so that every 1x1 conv of the walk can take
# the 256 x 128 packed-weight kernel once the batch fills the chip.  The fewest 256 x 128 tiles per example (O_proj and ffn of
# resampler 0: 2 m-tiles x 3 n-tiles) decide the batch: ceil(CUs / 6).
WIDE3 = _cfg(128, 512, 2, 3, 256, 4, 256, 2)
WIDE3_T, WIDE3_LEVELS, WIDE3_WSEED, WIDE3_INPUT_SEED, WIDE3_MIN_TILES = 5280, [528, 264, 132], 310, 310, 6
# 256 x 128 tiles per example of every conv the 256 x 128 kernel can take (Cout, L): resampler r asks with level 1 - r
WIDE3_TILES = {"proj_1x1": 10, "mask": 10, 0: {"Q": 12, "KV": 16, "O": 6, "ffn": 6}, 1: {"Q": 20, "KV": 24, "O": 10, "ffn": 10}}
# MANY: 6 blocks x (proj_1x1 + 4 resamplers x 4) = 102 packable weights -- more than one launch of the packing kernel holds (96) --
# run with 3 heads of 64 (with_heads); T = 640 gives levels 64 / 32 / 16 / 8 / 4.  Every packable conv is one 256 x 128 tile per
# example ([K; V]: two), so a batch of as many examples as the chip has CUs fills it at every level.
MANY = _cfg(128, 192, 6, 5, 64, 3, 64, 2)
MANY_T, MANY_LEVELS, MANY_HEADS, MANY_WSEED, MANY_INPUT_SEED, MANY_PACK_CHUNK = 640, [64, 32, 16, 8, 4], (3, 64), 311, 311, 96
# NARROW: off the grids -- 2 heads of 9 make 2 HD C = 720 and 2 HD = 36 (no multiples of 64: the concatenated [K; V] weight and
# bias sections are padded) and HD Lk = 126 / 234 (V's base inside the [K; V] projection is off the 16-byte grid), d = 9 takes the
# generic attention, 12 and 20 channels are below every MFMA GEMM's minimum; levels 26 / 13 / 7
NARROW = _cfg(12, 20, 2, 3, 24, 2, 9, 2, K=9)
NARROW_T, NARROW_LEVELS, NARROW_HEADS, NARROW_WSEED, NARROW_INPUT_SEED = 100, [26, 13, 7], (2, 9), 312, 312
# (heads, dims) -> the attention kernel and what of it the head dimension reaches
HEAD_SHAPES = (((3, 16), "mha_attention_mfma"),          # one 32-channel chunk, half full
               ((2, 48), "mha_attention_mfma"),          # two chunks, the second half full
               ((1, 80), "mha_attention_mfma"),          # the four-chunk instance with one chunk skipped
               ((1, 144), "mha_attention_mfma"),         # the eight-chunk instance with three skipped
               ((2, 24), "mha_attention_generic"),
               ((2, 9), "mha_attention_generic"))
HEADS_WSEED, HEADS_INPUT_SEED = 313, 313
# Levels of ONE position (K = 9: 4 samples per frame, ceil halving): (D, T) -> (levels, factor on decoder.weight).  One or two
# frames give the decoder so little to add up that max |out| of the fixtures' weights is 0.03 .. 0.1; the factor, chosen on the CPU
# from the fp64 restatement, brings every case (the other head shapes of (3, 8) included) back into [0.1, 10], where the 1e-4 bar
# means what it means for every other case.
ONE_POSITION = {(1, 3): ([1], 8.0), (2, 3): ([1, 1], 8.0), (3, 8): ([2, 1, 1], 4.0), (5, 30): ([8, 4, 2, 1, 1], 1.0)}
ONE_POSITION_WSEED, ONE_POSITION_INPUT_SEED = 314, 314
GRID_T, GRID_LEVELS, GRID_INPUT_SEED = 1120, [112, 56, 28], 315     # TINY on the MFMA grid at every level (kernel modes)


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


def with_heads(sd, cfg, heads, dims, seed):
    """The state dict of a model whose resamplers have `heads` heads of `dims` channels (what AttentiveUConvBlock and
    srf_attentive_v3_plan_create take and the reference's SuDORMRF cannot build): the first heads * dims rows of every Q / K / V
    projection, and O_proj.weight drawn anew as [C, heads * dims], uniform(-1, 1) / sqrt(heads * dims).  A new dict; sd is kept."""
    hd, C = heads * dims, cfg["in_channels"]
    assert hd <= HEADS * ATT_DIMS
    rng = np.random.default_rng(seed)
    out = dict(sd)
    for i in range(cfg["num_blocks"]):
        for r in range(cfg["upsampling_depth"] - 1):
            p = "sm.%d.attentive_resamplers.%d.mha." % (i, r)
            for n in "QKV":
                out[p + n + "_proj.weight"] = np.ascontiguousarray(sd[p + n + "_proj.weight"][:hd])
                out[p + n + "_proj.bias"] = np.ascontiguousarray(sd[p + n + "_proj.bias"][:hd])
            out[p + "O_proj.weight"] = (rng.uniform(-1, 1, size=(C, hd)) / np.sqrt(hd)).astype(np.float32)
    return out


def one_position_case(D, T):
    """(cfg, state dict for 4 heads of 256, input [2, 1, T]) of ONE_POSITION[(D, T)], decoder.weight times the case's factor"""
    cfg = dict(TINY_K9, upsampling_depth=D)
    sd = make_state_dict(cfg, ONE_POSITION_WSEED + D)
    sd["decoder.weight"] = sd["decoder.weight"] * np.float32(ONE_POSITION[(D, T)][1])
    return cfg, sd, make_mixture(2, T, ONE_POSITION_INPUT_SEED + D)


def tiles_256(batch, cout, length):
    """Tiles of a 256 x 128 launch: the left side of the library's "fills the chip" test (>= the CU count)"""
    return batch * -(-cout // 256) * -(-length // 128)


def make_input(name):
    _, batch, T, _, iseed = CASES[name]
    return make_mixture(batch, T, iseed)


def load_manifest():
    with open(MANIFEST) as f:
        return json.load(f)


def load_golden(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        return {k: z[k] for k in z.files}
