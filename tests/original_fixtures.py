"""Original SuDoRM-RF fixtures: the cases of tests/golden/ORIGINAL_MANIFEST.json and their weights / inputs.

Shared by the generator (tools/make_golden_original.py, which runs the reference on the build host) and the tests (which
regenerate the same weights and inputs from (config, seed) and compare against the stored reference outputs).  Every parameter
is drawn at random -- GroupNorm weights and biases, the per-channel PReLU slopes in (0.05, 0.45) and every bias included, so that
no norm or slope is an identity or a constant (a kernel that reads slope 0 for every channel fails) -- with scales that keep
max |out| in [0.1, 10].  ``ln_mask_in`` is drawn too: it is in the state_dict and must change nothing.
"""
import json
import os

import numpy as np

from tests.attentive_fixtures import GAINS, GOLDEN, ROOT, make_distinct, make_mixture, save_npz  # noqa: F401

MANIFEST = os.path.join(GOLDEN, "ORIGINAL_MANIFEST.json")
FIELDS = ("out_channels", "in_channels", "num_blocks", "upsampling_depth", "enc_kernel_size", "enc_num_basis", "num_sources")


def _cfg(B, C, U, D, N, S, K=21):
    return dict(out_channels=B, in_channels=C, num_blocks=U, upsampling_depth=D, enc_kernel_size=K, enc_num_basis=N, num_sources=S)


TINY = _cfg(32, 64, 2, 3, 64, 2)
SAME = _cfg(32, 64, 2, 3, 32, 2)                 # B == N: no reshape_before_masks
S1 = dict(TINY, num_sources=1)                   # sigmoid
S3_K9 = _cfg(32, 64, 2, 3, 64, 3, K=9)
D1 = dict(TINY, upsampling_depth=1)
DEFAULT_U2 = _cfg(128, 512, 2, 4, 512, 2)        # the file's defaults with two blocks
RECIPE_U1 = _cfg(256, 512, 1, 5, 512, 2)         # the README recipe with one block
RECIPE = _cfg(256, 512, 16, 5, 512, 2)           # -X 5 -N 512 -B 256 -H 512 -L 21 -R 16 (tools/original_bench.py)
PICKLE = _cfg(16, 16, 1, 2, 32, 2)

# name -> (constructor kwargs, batch, T, weight seed, input seed)
CASES = {
    "orig_tiny": (TINY, 2, 1001, 401, 401),
    "orig_tiny_short": (TINY, 2, 50, 402, 402),
    "orig_same": (SAME, 2, 333, 403, 403),
    "orig_s1": (S1, 2, 333, 404, 404),
    "orig_s3_k9": (S3_K9, 2, 108, 405, 405),           # (T = 100: see S3_K9_REFUSED_T)
    "orig_d1": (D1, 2, 333, 406, 406),
    "orig_default_u2": (DEFAULT_U2, 2, 10400, 407, 407),
    "orig_recipe_u1": (RECIPE_U1, 1, 32079, 408, 408),
}
# K = 9, D = 3 at T = 100 pads to 104 samples = 26 frames, no multiple of 2^(D-1) = 4: the reference's own upsample-and-add raises
# there (13 against 14 positions), so there is no output to compare with; the plan refuses it, and the golden sits at the next
# length that pads to a multiple of 16 samples (108 -> 112 = 28 frames)
S3_K9_REFUSED_T = 100
DIGEST_CONFIGS = {"tiny": TINY, "same": SAME}
PICKLE_SEED, PICKLE_BATCH, PICKLE_T, PICKLE_INPUT_SEED = 11, 2, 777, 409
DISTINCT_T, DISTINCT_SEED = 1001, 410                    # five distinct examples on the weights of orig_tiny
# WIDE: the recipe's channel counts (B = 256, C = N = 512) at D = 3, U = 2.  With the file's default B = 128 conv_1x1_exp has 128
# output channels, below the 192 the 256 x 128 kernel asks for, so that configuration can never run it there; at B = 256 every 1x1
# conv of the walk qualifies.  T = 5120 gives 512 frames = four 128-column tiles; per example l1 and conv_1x1_exp (256 rows) make
# 1 x 4 tiles, proj_1x1 and reshape_before_masks (512 rows) 2 x 4, the mask GEMM (1024 rows) 4 x 4.  The fewest (4) decide the
# batch that fills the chip: ceil(CUs / 4).
WIDE = _cfg(256, 512, 2, 3, 512, 2)
WIDE_T, WIDE_WSEED, WIDE_INPUT_SEED, WIDE_MIN_TILES = 5120, 411, 411, 4


def padded_length(cfg, T):
    """pad_to_appropriate_length: up to a multiple of lcm(K // 2, 2^D), only when T is not one already."""
    lcm = int(np.lcm(cfg["enc_kernel_size"] // 2, 2 ** cfg["upsampling_depth"]))
    return T + lcm - T % lcm if T % lcm else T


def frames(cfg, T):
    K = cfg["enc_kernel_size"]
    return (padded_length(cfg, T) + 2 * (K // 2) - K) // (K // 2) + 1


def schema(cfg):
    """[(state_dict key, shape)] of the original SuDORMRF(**cfg), in state_dict order."""
    B, C, U, D, K, N, S = (cfg[f] for f in FIELDS)
    out = [("encoder.0.weight", (N, 1, K)), ("encoder.0.bias", (N,)), ("ln.weight", (N,)), ("ln.bias", (N,)),
           ("l1.weight", (B, N, 1)), ("l1.bias", (B,))]
    for i in range(U):
        p = "sm.%d." % i
        out += [(p + "proj_1x1.conv.weight", (C, B, 1)), (p + "proj_1x1.conv.bias", (C,)), (p + "proj_1x1.norm.weight", (C,)),
                (p + "proj_1x1.norm.bias", (C,)), (p + "proj_1x1.act.weight", (C,))]
        for k in range(D):
            q = p + "spp_dw.%d." % k
            out += [(q + "conv.weight", (C, 1, 5)), (q + "conv.bias", (C,)), (q + "norm.weight", (C,)), (q + "norm.bias", (C,))]
        out += [(p + "conv_1x1_exp.conv.weight", (B, C, 1)), (p + "conv_1x1_exp.conv.bias", (B,)),
                (p + "conv_1x1_exp.norm.weight", (B,)), (p + "conv_1x1_exp.norm.bias", (B,)),
                (p + "final_norm.norm.weight", (C,)), (p + "final_norm.norm.bias", (C,)), (p + "final_norm.act.weight", (C,)),
                (p + "module_act.norm.weight", (B,)), (p + "module_act.norm.bias", (B,)), (p + "module_act.act.weight", (B,))]
    if B != N:
        out += [("reshape_before_masks.weight", (N, B, 1)), ("reshape_before_masks.bias", (N,))]
    out += [("m.weight", (S, 1, N + 1, 1)), ("m.bias", (S,)), ("decoder.weight", (S * N, 1, K)), ("decoder.bias", (S,)),
            ("ln_mask_in.weight", (N,)), ("ln_mask_in.bias", (N,))]
    return out


def make_state_dict(cfg, seed):
    """Ordered dict key -> float32 ndarray, every entry drawn from numpy's PCG64 stream of `seed`."""
    rng = np.random.default_rng(seed)
    N, K = cfg["enc_num_basis"], cfg["enc_kernel_size"]
    sd = {}
    for key, shape in schema(cfg):
        leaf = key.split(".")[-1]
        if ".norm." in key or key.startswith("ln"):           # GroupNorm
            w = rng.uniform(0.5, 1.5, size=shape) if leaf == "weight" else rng.uniform(-0.3, 0.3, size=shape)
        elif ".act." in key:                                  # per-channel PReLU slopes
            w = rng.uniform(0.05, 0.45, size=shape)
        elif key == "encoder.0.weight":                       # xavier-uniform
            w = rng.uniform(-1, 1, size=shape) * np.sqrt(6.0 / (K + N * K))
        elif key == "encoder.0.bias":                         # small next to the filter outputs: the ReLU cuts about half of them
            w = rng.uniform(-0.05, 0.05, size=shape)
        elif key == "decoder.weight":                         # (x 3, as the other variants' fixtures: max |out| >= 0.1 everywhere)
            w = rng.uniform(-1, 1, size=shape) * 3.0 * np.sqrt(6.0 / (K + N * K))
        elif key == "m.weight":                               # logits that spread over a few units: a softmax far from uniform
            w = rng.uniform(-1, 1, size=shape) * 4.0 / np.sqrt(N + 1.0)
        elif leaf == "weight":
            w = rng.uniform(-1, 1, size=shape) / np.sqrt(float(np.prod(shape[1:])))
        elif leaf == "bias":
            w = rng.uniform(-0.2, 0.2, size=shape)
        else:
            raise KeyError(key)
        sd[key] = np.ascontiguousarray(w, dtype=np.float32)
    return sd


def toeplitz(m_weight, m_bias):
    """The mask layer Conv2d(1 -> S, (N + 1, 1), padding (N - N // 2, 0)) as a GEMM (the issue's formula, N even):
    (Tz [S N, N], row bias [S N]) with Tz[s N + i, n] = m.weight[s, 0, n - i + pad, 0] where 0 <= n - i + pad <= N, else 0.
    Dtype of m_weight is kept: a copy, no arithmetic."""
    w = np.asarray(m_weight)
    S, N = w.shape[0], w.shape[2] - 1
    pad = N - N // 2
    tz = np.zeros((S * N, N), dtype=w.dtype)
    for s in range(S):
        for i in range(N):
            n = np.arange(N)
            j = n - i + pad
            ok = (j >= 0) & (j <= N)
            tz[s * N + i, n[ok]] = w[s, 0, j[ok], 0]
    return tz, np.repeat(np.asarray(m_bias), N)


def expand_decoder(weight, S):
    """decoder.weight [S N, 1, K] of the grouped ConvTranspose1d -> block-diagonal [S N, S, K]."""
    w = np.asarray(weight)
    SN, _, K = w.shape
    N = SN // S
    out = np.zeros((SN, S, K), dtype=w.dtype)
    for c in range(SN):
        out[c, c // N] = w[c, 0]
    return out


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
