"""Ragged-batch fixtures of the original SuDoRM-RF: tests/golden/orig_ragged_*.npz.

Every case is one padded batch [rows, 1, T] with its lengths and, per row, the output of the UNMODIFIED reference model on that row
alone at its own length (batch 1) -- written by tools/make_golden_original_ragged.py on the build host.  The weights come from
tests/original_fixtures.make_state_dict(config, seed), as everywhere; the mixtures are stored (rows are read up to their length,
what lies past it belongs to the test to overwrite).

The configurations are the smallest that pass srf_original_ragged_supported -- every 1x1 convolution a shape of the 256 x 128
GEMM -- and between them take both tails of the walk (with and without reshape_before_masks), two and three sources, and the
recipe's depth.  The lengths put every row on the pyramid's 16-frame chunk grid under the model's own padding rule, lcm(10, 2^D)
samples: one row at the batch's T, one that pads up to it, rows in the middle, and the shortest the pyramid takes."""
import os

import numpy as np

from tests.original_fixtures import GOLDEN, _cfg, frames, make_mixture, make_state_dict, save_npz  # noqa: F401

# name -> (constructor kwargs, T, lengths, weight seed, input seed)
CASES = {
    # reshape_before_masks present; D = 3 pads to multiples of 40 samples = 4 frames, so the lengths are chosen on the 16 grid
    "rg_a": (_cfg(192, 256, 2, 3, 256, 2), 2560, (2560, 2399, 1900, 1280, 950, 640), 501, 501),
    # the recipe's depth and channels, one block: D = 5 pads to multiples of 160 samples = 16 frames
    "rg_b": (_cfg(256, 512, 1, 5, 512, 2), 2560, (2560, 2401, 2400, 1921, 1441, 1280), 502, 502),
    # B = N: no reshape_before_masks; three sources
    "rg_c": (_cfg(256, 256, 1, 3, 256, 3), 2560, (2560, 2240, 1600, 960, 800, 640), 503, 503),
}
OFF_GRID = ("rg_a", 641)          # 641 samples pad to 680 = 68 frames: off the 16-frame grid at D = 3
RECIPE_BATCH, RECIPE_T = 32, 32000


def path(name):
    return os.path.join(GOLDEN, "orig_ragged_%s.npz" % name[3:])


def make_wav(name):
    _, T, lengths, _, iseed = CASES[name]
    return make_mixture(len(lengths), T, iseed)


def row_frames(name):
    cfg, _, lengths, _, _ = CASES[name]
    return [frames(cfg, n) for n in lengths]


def load(name):
    """{"wav" [rows, 1, T], "lengths" [rows], "out" [the reference's per-row outputs, each [S, lengths[b]]]}"""
    with np.load(path(name)) as z:
        lengths = [int(n) for n in z["lengths"]]
        return {"wav": z["wav"], "lengths": lengths, "out": [z["out%d" % b] for b in range(len(lengths))]}
