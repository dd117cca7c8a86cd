"""The original SuDoRM-RF's walk on the host, pinned as literals: what a plan reports -- workspace bytes, launches, frames, padded
length, the training step's `saved` and `scratch` bytes -- and the exact text and return code of every entry-check refusal of the
two ragged entry points (fake pointers: a refusal comes before any launch).  No GPU needed.

Recorded on commit 30e11c2, the commit BEFORE the inference walk and the training forward became one walk, the two spellings of the
padding rule one function and the ragged entry's copy of the argument checks a call of the forward's."""
import ctypes as C

import pytest

from tests import original_fixtures as of
from tests import original_ragged_fixtures as rf
from tests.test_original_host import _plan

RG_C = rf.CASES["rg_c"]
# name: (constructor kwargs, batch, T)
SHAPES = {
    "TINY": (of.TINY,) + of.CASES["orig_tiny"][1:3],
    "SAME": (of.SAME,) + of.CASES["orig_same"][1:3],
    "D1": (of.D1,) + of.CASES["orig_d1"][1:3],
    "S3_K9": (of.S3_K9,) + of.CASES["orig_s3_k9"][1:3],
    "rg_c": (RG_C[0], len(RG_C[2]), RG_C[1]),
}
# name: (workspace bytes, launches, frames, padded length, saved bytes, scratch bytes)
FIGURES = {
    "TINY": (741376, 33, 104, 1040, 829440, 1122816),
    "SAME": (216064, 32, 36, 360, 261120, 357376),
    "D1": (293376, 29, 34, 340, 257536, 587264),
    "S3_K9": (318464, 33, 28, 112, 260096, 626944),
    "rg_c": (28143104, 22, 256, 2560, 18530304, 44814080),
}
EINVAL, EWORKSPACE = -1, -3


def _lib():
    from sudo_rm_rf_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("name", list(SHAPES))
def test_plan_figures_are_what_they_were(name):
    lib = _lib()
    plan = _plan(*SHAPES[name])
    h = plan.handle
    got = (lib.srf_plan_workspace_bytes(h), lib.srf_plan_num_launches(h), lib.srf_plan_frames(h), lib.srf_plan_padded_length(h),
           lib.srf_original_train_saved_bytes(h), lib.srf_original_train_scratch_bytes(h))
    assert got == FIGURES[name]


def _ragged_call(lib, which, plan, lengths, num_params=None, workspace=256, workspace_bytes=1 << 40, null_at=None):
    """(return code, srf_last_error()) of srf_original_forward_ragged / _separate_ragged with fake non-null pointers"""
    n = plan.num_params if num_params is None else num_params
    entries = [256] * max(n, 1)
    if null_at is not None:
        entries[null_at] = None
    table = (C.c_void_p * max(n, 1))(*entries)
    lens = (C.c_int * len(lengths))(*lengths)
    one, ws = C.c_void_p(256), C.c_void_p(workspace)
    if which == "forward":
        rc = lib.srf_original_forward_ragged(plan.handle, table, n, one, lens, one, ws, workspace_bytes, None)
    else:
        rc = lib.srf_original_separate_ragged(plan.handle, table, n, one, lens, one, one, 0, ws, workspace_bytes, None)
    return rc, lib.srf_last_error().decode()


@pytest.mark.parametrize("which", ["forward", "separate"])
def test_ragged_entry_refusals_are_what_they_were(which):
    cfg, T, lengths, _, _ = RG_C
    assert (T, len(lengths)) == (2560, 6)
    p = _plan(cfg, len(lengths), T)
    assert (p.num_params, p.workspace_bytes) == (39, 28143104)
    lib = _lib()
    who = "srf_original_%s_ragged (original): " % which
    zero, over = list(lengths), list(lengths)
    zero[2], over[4] = 0, T + 1
    for kwargs, lens, rc, text in (
            (dict(num_params=38), lengths, EINVAL, "expected 39 parameter tensors, got 38"),
            (dict(workspace_bytes=28143103), lengths, EWORKSPACE, "workspace too small (28143103 < 28143104 bytes)"),
            (dict(workspace=384), lengths, EINVAL, "workspace must be 256-byte aligned"),
            (dict(null_at=3), lengths, EINVAL, "parameter 3 is null"),
            (dict(), zero, EINVAL, "example 2 has length 0 (allowed: 1..2560)"),
            (dict(), over, EINVAL, "example 4 has length 2561 (allowed: 1..2560)")):
        assert _ragged_call(lib, which, p, lens, **kwargs) == (rc, who + text)
    # the order of the checks: the parameter count before the workspace, the workspace's size before its alignment, a null
    # parameter before the lengths
    assert _ragged_call(lib, which, p, zero, num_params=38, workspace_bytes=0)[1] == who + "expected 39 parameter tensors, got 38"
    assert _ragged_call(lib, which, p, zero, workspace=384, workspace_bytes=0)[0] == EWORKSPACE
    assert _ragged_call(lib, which, p, zero, null_at=0)[1] == who + "parameter 0 is null"
