"""Attentive SuDoRM-RF (v2), whole-model ragged forward: the cases of tests/golden/ATTN_MODEL_RAGGED_MANIFEST.json.

Shared by the generator (tools/make_golden_attentive_model_ragged.py: the reference model in eval(), every row alone at its own
length) and the tests, which regenerate weights and mixtures from (config, seed) with tests/attentive_fixtures.py; the fixtures
hold outputs, lengths and metadata only.  All K = 21.  Frames = padded length / 10, the deepest level has frames >> (D - 1).
"""
import json
import os

import numpy as np

from tests import attentive_fixtures as af

MANIFEST = os.path.join(af.GOLDEN, "ATTN_MODEL_RAGGED_MANIFEST.json")
BAR = 1e-4

# name -> (constructor kwargs, lengths, weight seed, input seed); T = max(lengths)
CASES = {
    # attn_tiny's config: frames 104 / 64 / 12, deepest level 26 / 16 / 3 (row stride 26: off the grid of 4); the unfused tail
    "a": (af.TINY, (1001, 640, 90), 301, 301),
    # frames 200 / 130 / 42: two column tiles and two lengths off the grid of 4; every GEMM of the walk on the 128 x 128 ragged kernel
    "b": (af._cfg(64, 128, 2, 2, 64, 4, 256, 2), (2000, 1300, 410), 302, 302),
    # frames 128 / 80 / 36, deepest level 32 / 20 / 9
    "c": (af._cfg(256, 256, 1, 3, 256, 4, 256, 2), (1280, 800, 330), 303, 303),
    # the reference defaults with two blocks: frames 1040 / 520
    "d": (af.DEFAULT_U2, (10400, 5200), 304, 304),
}


def model(cfg):
    """the HIP attentive v2 SuDORMRF(**cfg), parameters as the constructor left them, on the CPU"""
    from sudo_rm_rf_amd.dnn.models.attentive_sudormrf_v2 import SuDORMRF
    return SuDORMRF(**cfg)


def plan(cfg, batch, T):
    """an attentive plan made without a GPU (the blocks' real 4 heads of 256 channels)"""
    import torch
    from sudo_rm_rf_amd.engine import Plan
    tup = ("attentive", 1) + tuple(cfg[f] for f in af.FIELDS[:6]) + (cfg["num_sources"], 1, (af.HEADS, af.ATT_DIMS))
    return Plan(tup, batch, T, torch.device("cpu"))


def frames(cfg, n):
    return af.padded_length(cfg, n) // (cfg["enc_kernel_size"] // 2)


def path(name):
    return os.path.join(af.GOLDEN, "attn_model_ragged_%s.npz" % name)


def make_wav(name):
    """[batch, 1, T] float32: the rows of make_distinct (different content and level per row); row b is used up to lengths[b]"""
    cfg, lengths, _, iseed = CASES[name]
    return af.make_distinct(len(lengths), max(lengths), iseed)


def load(name):
    """-> {"lengths": [...], "out": [per row [S, lengths[b]] float32]}"""
    with np.load(path(name)) as z:
        lengths = [int(n) for n in z["lengths"]]
        return {"lengths": lengths, "out": [z["out%d" % b] for b in range(len(lengths))]}


def load_manifest():
    with open(MANIFEST) as f:
        return json.load(f)
