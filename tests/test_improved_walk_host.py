"""The Improved / GroupComm walk on the host, pinned as literals: what a plan reports -- workspace bytes, launches, frames, padded
length, the training step's `saved` and `scratch` bytes -- and the exact text and return code of every refusal of
srf_forward_train that fake pointers reach (a refusal comes before any launch): the entry checks in their order, L % 4, the TAC
size limits.  No GPU needed.

Recorded on commit 2377517, the commit BEFORE the inference walk and the training forward of these two models became one walk
(srf_improved_walk.h)."""
import ctypes as C
import json
import os

import pytest
import torch

from conftest import GOLDEN
from oracle.schema import ModelConfig
from tests.test_gpu_launch_sequence import BATCH, T, TRAIN_SHAPES

# name: (workspace bytes, launches, frames, padded length, saved bytes, scratch bytes); the shapes: the two golden cases at their
# own batch and T, TRAIN_SHAPES (improved_pairs among them), cfg 2 and cfg 3 at batch 32, T = 10400
FIGURES = {
    "tiny_improved": (135936, 20, 56, 560, 205312, 259072),
    "tiny_groupcomm": (355840, 24, 72, 720, 581120, 755456),
    "improved_d5": (10344704, 32, 800, 8000, 23184384, 12706816),
    "improved_d2": (824832, 18, 256, 2560, 1182720, 1300480),
    "improved_d2_l36": (71936, 13, 36, 180, 71424, 148480),
    "improved_d1": (221184, 16, 100, 1000, 295936, 370688),
    "groupcomm_d4": (3341312, 26, 400, 4000, 5754880, 6335488),
    "improved_pairs": (237982208, 18, 4000, 40000, 409673728, 276468992),
    "cfg2_improved_u16": (599115520, 136, 1056, 10560, 5297963008, 813191424),
    "cfg3_groupcomm_u8": (665166080, 88, 1056, 10560, 3425173504, 1073500928),
}
EINVAL = -1


def _lib():
    from sudo_rm_rf_amd import _lib
    return _lib.load()


def _plan(cfg, batch, T_):
    from sudo_rm_rf_amd.engine import Plan
    return Plan((cfg.variant, cfg.in_audio_channels, cfg.out_channels, cfg.in_channels, cfg.num_blocks, cfg.upsampling_depth,
                 cfg.enc_kernel_size, cfg.enc_num_basis, cfg.num_sources, cfg.group_size), batch, T_, torch.device("cpu"))


def _shape(name):
    if name in TRAIN_SHAPES:
        return TRAIN_SHAPES[name]
    with open(os.path.join(GOLDEN, "MANIFEST.json")) as f:
        meta = json.load(f)["cases"][name]
    big = name.startswith("cfg")
    return ModelConfig(**meta["config"]), BATCH if big else meta["batch"], T if big else meta["T"]


@pytest.mark.parametrize("name", list(FIGURES))
def test_plan_figures_are_what_they_were(name):
    lib = _lib()
    plan = _plan(*_shape(name))      # (alive while its handle is in use)
    h = plan.handle
    got = (lib.srf_plan_workspace_bytes(h), lib.srf_plan_num_launches(h), lib.srf_plan_frames(h), lib.srf_plan_padded_length(h),
           lib.srf_train_saved_bytes(h), lib.srf_train_scratch_bytes(h))
    assert got == FIGURES[name]


def _forward_train(lib, plan, num_params=None, null_at=None, wav=256, out=256, saved=256, saved_bytes=None, scratch=256,
                   scratch_bytes=None):
    """(return code, srf_last_error()) of srf_forward_train with fake non-null pointers and buffers of the needed size"""
    n = plan.num_params if num_params is None else num_params
    entries = [256] * max(n, 1)
    if null_at is not None:
        entries[null_at] = None
    table = (C.c_void_p * max(n, 1))(*entries)
    need_saved, need_scratch = plan.train_sizes()
    rc = lib.srf_forward_train(plan.handle, table, n, C.c_void_p(wav), C.c_void_p(out), C.c_void_p(saved),
                               need_saved if saved_bytes is None else saved_bytes, C.c_void_p(scratch),
                               need_scratch if scratch_bytes is None else scratch_bytes, None)
    return rc, lib.srf_last_error().decode()


def test_forward_train_entry_refusals_are_what_they_were():
    lib = _lib()
    p = _plan(*_shape("tiny_improved"))
    assert (p.num_params, p.train_sizes()) == (53, (205312, 259072))
    who = "srf_forward_train: "
    for kwargs, text in (
            (dict(wav=None), "null pointer"),
            (dict(out=None), "null pointer"),
            (dict(saved=None), "null pointer"),
            (dict(scratch=None), "null pointer"),
            (dict(num_params=52), "expected 53 parameter tensors, got 52"),
            (dict(null_at=3), "parameter 3 is null"),
            (dict(saved_bytes=205311), "saved buffer too small (205311 bytes, needs 205312)"),
            (dict(scratch_bytes=259071), "scratch buffer too small (259071 bytes, needs 259072)"),
            (dict(saved=384), "saved and scratch must be 256-byte aligned"),
            (dict(scratch=128), "saved and scratch must be 256-byte aligned"),
            # the order of the checks: the parameter count, a null parameter, `saved`, `scratch`, the alignment
            (dict(num_params=52, saved_bytes=0, saved=384), "expected 53 parameter tensors, got 52"),
            (dict(null_at=0, saved_bytes=0), "parameter 0 is null"),
            (dict(saved_bytes=0, scratch_bytes=0, saved=384), "saved buffer too small (0 bytes, needs 205312)"),
            (dict(scratch_bytes=0, scratch=384), "scratch buffer too small (0 bytes, needs 259072)")):
        assert _forward_train(lib, p, **kwargs) == (EINVAL, who + text)


@pytest.mark.parametrize("cfg,T_,frames,text", [
    (ModelConfig("improved", 16, 24, 2, 1, 21, 32, 2), 1010, 102, "L=102 must be a multiple of 4"),
    (ModelConfig("improved", 16, 24, 2, 1, 21, 32, 2), 90, 10, "L=10 must be a multiple of 4"),
    (ModelConfig("groupcomm", 64, 128, 2, 4, 21, 64, 2, 1, 2), 4000, 400,
     "TAC backward supports out_channels/group_size in {2,4,8,16} and group_size in {2,4,8,16} (got 32, 2)"),
    # (the TAC limit comes before L % 4)
    (ModelConfig("groupcomm", 64, 128, 2, 1, 21, 64, 2, 1, 2), 1010, 102,
     "TAC backward supports out_channels/group_size in {2,4,8,16} and group_size in {2,4,8,16} (got 32, 2)"),
    (ModelConfig("groupcomm", 64, 128, 2, 4, 21, 64, 2, 1, 32), 4000, 400,
     "TAC backward supports out_channels/group_size in {2,4,8,16} and group_size in {2,4,8,16} (got 2, 32)"),
], ids=["L_102", "L_10", "tac_n_32", "tac_n_32_L_102", "tac_G_32"])
def test_forward_train_shape_refusals_are_what_they_were(cfg, T_, frames, text):
    lib = _lib()
    p = _plan(cfg, 2, T_)
    assert p.frames == frames
    assert _forward_train(lib, p) == (EINVAL, "srf_forward_train: " + text)
    # ... and after the entry checks
    assert _forward_train(lib, p, saved=384) == (EINVAL, "srf_forward_train: saved and scratch must be 256-byte aligned")
