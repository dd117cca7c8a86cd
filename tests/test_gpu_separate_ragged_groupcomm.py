"""separate_ragged of the GroupComm model on the GPU: cfg 3 weights, batch 32, T = 10400 (the setup of
tests/test_gpu_ragged_groupcomm.py), RAW rows of very different level and offset.  Mixture consistency -- what the README
prescribes for this model -- is on by default.  Every row against the oracle recipe of that row alone (normalised over its own
length, oracle.torch_oracle.forward at that length, rescaled, made mixture consistent in torch) within TOL * max(1, std_i);
then isolation and separate_list end to end.  The helpers are those of tests/test_gpu_separate_ragged.py."""
import pytest
import torch

from test_gpu_separate_ragged import (BATCH, DEV, T, check_against_the_oracle, check_degenerate_rows_recipe, check_isolation,
                                      check_separate_list, recipe_setup)

pytestmark = pytest.mark.gpu

CASE = "cfg3_groupcomm_u8"


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    from sudo_rm_rf_amd import _lib, ops
    _lib.load()
    ops.set_kernel_mode(0)


@pytest.fixture(scope="module")
def setup(manifest):
    return recipe_setup(manifest, CASE, 9150)


def test_separate_ragged_matches_the_oracle_recipe_row_by_row(setup):
    """the default (mixture consistency on) and both explicit settings, from ONE oracle forward per row"""
    cfg, model, x, lens, want, st = setup
    assert model._engine().ragged_plan_supported(BATCH, T, torch.device(DEV))
    check_against_the_oracle(model, x, lens, want, st, True)
    check_against_the_oracle(model, x, lens, want, st, True, mixture_consistency=True)
    check_against_the_oracle(model, x, lens, want, st, False, mixture_consistency=False)


def test_separate_ragged_with_silent_dc_and_near_silent_rows(manifest, setup):
    """mixture consistency on, as the README prescribes for this model (the helper and its bars: tests/test_gpu_separate_ragged.py)"""
    check_degenerate_rows_recipe(manifest, CASE, setup, True)


def test_separate_ragged_launch_set(setup):
    """what test_gpu_ragged_groupcomm.py pins for forward_ragged, plus exactly one wav_stats_ragged"""
    from sudo_rm_rf_amd import ops
    cfg, model, x, lens, _, _ = setup
    with torch.no_grad(), ops.kernel_trace(DEV) as tr:
        model.separate_ragged(x.to(DEV), lens)
    U = cfg.num_blocks
    count = {n: sum(1 for k, _ in tr.launches if k == n) for n in tr.names}
    print("separate_ragged dispatched", sorted(count.items()))
    assert count == {"wav_stats_ragged": 1, "zero_fill": 1, "pack_pw_weights": 1, "encoder_ragged": 1, "pw_conv_x3w_ragged<1>": 1,
                     "tac_mfma_ragged": U, "pw_conv_small_ragged": 2 * U, "pyramid_moments_ragged": U, "pyramid_finalize_ragged": U,
                     "pyramid_merge_ragged": U, "pack_decoder": 1, "pw_mask_decode": 1, "overlap_add_ragged": 1}


@pytest.mark.parametrize("keep", [0, 1], ids=["even-rows", "odd-rows"])
def test_separate_ragged_rows_are_isolated(setup, keep):
    cfg, model, x, lens, _, st = setup
    check_isolation(model, x, lens, st, keep, 9151)


def test_separate_list_is_one_gather_and_one_call_per_batch(setup):
    cfg, model, _, _, _, _ = setup
    check_separate_list(model, cfg, 80, 9800)
