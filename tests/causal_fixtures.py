"""Causal SuDoRM-RF (v3) fixtures: the cases of tests/golden/CAUSAL_MANIFEST.json and their weights / inputs.

Shared by the generator (tools/make_golden_causal.py, which runs the reference on the build host) and the tests (which
regenerate the same weights and inputs from (config, seed) and compare against the stored reference outputs).  Every
parameter is drawn at random -- skipinit_gain included, so that no block is the identity, and the causally masked taps of
the encoder / depthwise weights, so that a kernel that reads them fails -- with scales that keep max |out| in [0.1, 10].
"""
import io
import json
import os
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MANIFEST = os.path.join(GOLDEN, "CAUSAL_MANIFEST.json")

FIELDS = ("in_audio_channels", "out_channels", "in_channels", "num_blocks", "upsampling_depth", "enc_kernel_size",
          "enc_num_basis", "num_sources")
DEFAULTS = dict(in_audio_channels=1, out_channels=128, in_channels=512, num_blocks=16, upsampling_depth=4,
                enc_kernel_size=21, enc_num_basis=512, num_sources=2)
MAIN = dict(in_audio_channels=2, out_channels=256, in_channels=512, num_blocks=4, upsampling_depth=5, enc_kernel_size=21,
            enc_num_basis=512, num_sources=2)
TINY = dict(in_audio_channels=1, out_channels=32, in_channels=64, num_blocks=2, upsampling_depth=3, enc_kernel_size=21,
            enc_num_basis=64, num_sources=2)
TINY_A2 = dict(in_audio_channels=2, out_channels=32, in_channels=64, num_blocks=2, upsampling_depth=2, enc_kernel_size=11,
               enc_num_basis=64, num_sources=3)
# depth 8 (the deepest the library takes): one block, 16 channels; 23001 samples pad to 2304 frames = three 1024-frame tiles of
# the fused pyramid, the third one's 1280-frame left halo reaching into the first
TINY_D8 = dict(in_audio_channels=1, out_channels=8, in_channels=16, num_blocks=1, upsampling_depth=8, enc_kernel_size=21,
               enc_num_basis=16, num_sources=2)

# name -> (constructor kwargs, batch, T, weight seed, input seed, stored arrays)
CASES = {
    "causal_tiny": (TINY, 2, 1001, 101, 101, ("enc", "sep", "out")),
    "causal_tiny_a2_k11": (TINY_A2, 3, 777, 102, 102, ("out",)),
    "causal_tiny_short": (TINY, 2, 50, 103, 103, ("out",)),
    "causal_default": (DEFAULTS, 4, 32000, 104, 104, ("out",)),
    "causal_main": (MAIN, 1, 44100, 105, 105, ("out",)),
    "causal_tiny_d8": (TINY_D8, 2, 23001, 107, 107, ("out",)),
}
# configurations whose seeded reference state_dict is pinned by sha256 digests (CPU test)
DIGEST_CONFIGS = {"tiny": TINY, "main": MAIN}
PICKLE_CONFIG = TINY_A2


def schema(cfg):
    """[(state_dict key, shape)] of CausalSuDORMRF(**cfg), in state_dict order."""
    A, B, C, U, D, K, N, S = (cfg[f] for f in FIELDS)
    out = [("encoder.weight", (N, A, 2 * K - 1)), ("bottleneck.weight", (B, N, 1)), ("bottleneck.bias", (B,))]
    for i in range(U):
        p = "sm.%d." % i
        out += [(p + "skipinit_gain", ()), (p + "proj_1x1.conv.weight", (C, B, 1)), (p + "proj_1x1.conv.bias", (C,)),
                (p + "proj_1x1.act.weight", (1,))]
        for k in range(D):
            q = p + "spp_dw.%d." % k
            out += [(q + "conv.weight", (C, 1, 21)), (q + "conv.bias", (C,)), (q + "act.weight", (1,))]
        out += [(p + "res_conv.weight", (B, C, 1)), (p + "res_conv.bias", (B,))]
    out += [("mask_net.0.weight", (1,)), ("mask_net.1.weight", (S * N * A, B, 1)), ("mask_net.1.bias", (S * N * A,)),
            ("decoder.weight", (S * N * A, S * A, K)), ("mask_nl_class.weight", (1,))]
    return out


def make_state_dict(cfg, seed):
    """Ordered dict key -> float32 ndarray, every entry drawn from numpy's PCG64 stream of `seed`."""
    rng = np.random.default_rng(seed)
    sd = {}
    for key, shape in schema(cfg):
        leaf = key.split(".")[-1]
        if key.endswith("skipinit_gain"):
            w = rng.uniform(0.2, 0.6, size=shape)
        elif shape == (1,):                                   # PReLU slopes
            w = rng.uniform(0.05, 0.45, size=shape)
        elif key in ("encoder.weight", "decoder.weight"):    # xavier-uniform, all taps (masked ones too)
            rf = shape[2]
            b = np.sqrt(6.0 / (shape[1] * rf + shape[0] * rf))
            w = rng.uniform(-b, b, size=shape)
        elif ".spp_dw." in key and leaf == "weight":          # depthwise: scaled for its 11 live taps, all 21 drawn
            w = rng.uniform(-0.5, 0.5, size=shape) / np.sqrt(11.0)
        elif leaf == "weight":
            w = rng.uniform(-1, 1, size=shape) / np.sqrt(float(np.prod(shape[1:])))
        elif leaf == "bias":
            w = rng.uniform(-0.2, 0.2, size=shape)
        else:
            raise KeyError(key)
        sd[key] = np.ascontiguousarray(w, dtype=np.float32)
    return sd


def make_input(name):
    from oracle.weights import make_mixture
    cfg, batch, T, _, iseed, _ = CASES[name]
    return make_mixture(batch, T, iseed, channels=cfg["in_audio_channels"])


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
