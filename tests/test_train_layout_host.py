"""The `saved` and `scratch` layouts of the three training steps, pinned as byte totals.  No GPU needed.

The six layout functions (srf_train.hip, srf_causal_train.hip, srf_original_train.hip) carve their slices with one shared
helper; these totals, asked through the C size queries, were recorded on commit 4711e9b, the commit BEFORE the helper replaced
the six hand-written carving lambdas.  A total moves when any slice before the end changes its size or its alignment."""
import pytest
import torch

from tests import causal_fixtures as cf
from tests import original_fixtures as of
from test_gpu_launch_sequence import TRAIN_SHAPES


def _improved(name):
    c, batch, T = TRAIN_SHAPES[name]
    return (c.variant, c.in_audio_channels, c.out_channels, c.in_channels, c.num_blocks, c.upsampling_depth, c.enc_kernel_size,
            c.enc_num_basis, c.num_sources, c.group_size), batch, T


def _causal(cfg, batch, T):
    return ("causal",) + tuple(cfg[f] for f in cf.FIELDS) + (1,), batch, T


def _original(cfg, batch, T):
    return ("original", 1) + tuple(cfg[f] for f in of.FIELDS) + (1,), batch, T


# name: ((configuration tuple, batch, T), size queries, (saved bytes, scratch bytes))
CASES = {
    "improved_d5": (_improved("improved_d5"), "srf_train", (23184384, 12706816)),
    "improved_d1": (_improved("improved_d1"), "srf_train", (295936, 370688)),
    "groupcomm_d4": (_improved("groupcomm_d4"), "srf_train", (5754880, 6335488)),
    "causal_tiny": (_causal(cf.TINY, 2, 1001), "srf_causal_train", (638976, 705792)),
    "orig_tiny": (_original(of.TINY, 2, 1001), "srf_original_train", (829440, 1122816)),
    "orig_same": (_original(of.SAME, 2, 333), "srf_original_train", (261120, 357376)),          # no reshape_before_masks slice
    "orig_d1": (_original(of.D1, 2, 333), "srf_original_train", (257536, 587264)),              # 34 frames: the padg / padx slices
}


def sizes(name):
    from sudo_rm_rf_amd import _lib
    from sudo_rm_rf_amd.engine import Plan
    lib = _lib.load()
    (tup, batch, T), query, _ = CASES[name]
    plan = Plan(tup, batch, T, torch.device("cpu"))
    return getattr(lib, query + "_saved_bytes")(plan.handle), getattr(lib, query + "_scratch_bytes")(plan.handle), plan


@pytest.mark.parametrize("name", list(CASES))
def test_saved_and_scratch_totals_are_what_they_were(name):
    saved, scratch, plan = sizes(name)
    assert (saved, scratch) == CASES[name][2]
    assert plan.train_sizes() == (saved, scratch)          # (the plan asks its own family's queries)
    if name == "orig_d1":
        assert plan.frames == 34
