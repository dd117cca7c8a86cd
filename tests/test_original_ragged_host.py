"""The original SuDoRM-RF's opt-in ragged forward on the host: exported symbols, the gate, the refusals before any launch (fake
pointers: nothing is launched), the fixtures of tools/make_golden_original_ragged.py, and SuDORMRF.enable_ragged() -- what it
switches on and that everything pinned for a model without it stays as it was.  No GPU needed."""
import ctypes as C
import pickle

import numpy as np
import pytest
import torch

from tests import original_fixtures as of
from tests import original_ragged_fixtures as rf
from tests import original_ref as orf
from tests.test_original_host import _model, _plan

NEW_SYMBOLS = ("srf_gln_apply_c_ragged", "srf_encoder_bias_relu_ragged", "srf_softmax_mask_ragged", "srf_bias_rescale_ragged",
               "srf_original_ragged_supported", "srf_original_ragged_workspace_bytes", "srf_original_forward_ragged",
               "srf_original_separate_ragged")
RECIPE_U16 = of.RECIPE


def _lib():
    from sudo_rm_rf_amd import _lib
    return _lib.load()


def _call(lib, which, plan, lengths, num_params=None):
    """srf_original_forward_ragged / _separate_ragged with fake (non-null, 256-byte aligned) pointers: refusals come first."""
    n = plan.num_params if num_params is None else num_params
    table = (C.c_void_p * max(n, 1))(*([256] * max(n, 1)))
    lens = (C.c_int * len(lengths))(*lengths)
    one = C.c_void_p(256)
    if which == "forward":
        return lib.srf_original_forward_ragged(plan.handle, table, n, one, lens, one, one, 1 << 40, None)
    return lib.srf_original_separate_ragged(plan.handle, table, n, one, lens, one, one, 0, one, 1 << 40, None)


def test_every_declared_symbol_is_exported_and_bound():
    from sudo_rm_rf_amd import _lib
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and getattr(lib, name) is not None, name
    header = open(__import__("os").path.join(of.ROOT, "include", "sudormrf_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in header, name
    assert lib.srf_abi_version() == 19


@pytest.mark.parametrize("name", sorted(rf.CASES))
def test_the_gate_takes_the_three_cases(name):
    cfg, T, lengths, _, _ = rf.CASES[name]
    p = _plan(cfg, len(lengths), T)
    lib = _lib()
    assert p.original_ragged_supported and lib.srf_original_ragged_supported(p.handle) == 1
    assert lib.srf_original_ragged_workspace_bytes(p.handle) == p.workspace_bytes > 0
    # the general entry points keep refusing the plan
    assert not p.ragged_supported and lib.srf_plan_ragged_supported(p.handle) == 0 and lib.srf_plan_ragged_workspace_bytes(p.handle) == 0


def test_the_gate_takes_the_recipe_at_batch_32():
    p = _plan(RECIPE_U16, rf.RECIPE_BATCH, rf.RECIPE_T)
    assert p.original_ragged_supported and not p.ragged_supported
    assert _lib().srf_original_ragged_workspace_bytes(p.handle) == p.workspace_bytes


@pytest.mark.parametrize("cfg,T", [(of.TINY, 2560), (of.DEFAULT_U2, 2560), (of.S3_K9, 1008)], ids=["tiny", "default_u2_B128", "s3_k9"])
def test_the_gate_refuses_small_and_foreign_shapes(cfg, T):
    p = _plan(cfg, 6, T)
    lib = _lib()
    assert not p.original_ragged_supported and lib.srf_original_ragged_workspace_bytes(p.handle) == 0
    assert lib.srf_plan_ragged_supported(p.handle) == 0
    rc = _call(lib, "forward", p, [T] * 6)
    assert rc == -1 and b"original" in lib.srf_last_error() and b"not supported" in lib.srf_last_error()


def test_the_gate_is_closed_under_kernel_mode_1():
    cfg, T, lengths, _, _ = rf.CASES["rg_a"]
    p = _plan(cfg, len(lengths), T)
    lib = _lib()
    assert p.original_ragged_supported
    lib.srf_set_kernel_mode(1)
    try:
        assert not p.original_ragged_supported and lib.srf_original_ragged_workspace_bytes(p.handle) == 0
        assert lib.srf_plan_ragged_supported(p.handle) == 0
        assert _call(lib, "separate", p, list(lengths)) == -1 and b"original" in lib.srf_last_error()
    finally:
        lib.srf_set_kernel_mode(0)
    assert p.original_ragged_supported


@pytest.mark.parametrize("which", ["forward", "separate"])
def test_refusals_come_before_any_launch_and_name_the_example(which):
    cfg, T, lengths, _, _ = rf.CASES["rg_a"]
    p = _plan(cfg, len(lengths), T)
    lib = _lib()
    for bad, at, word in ((0, 2, b"length 0"), (T + 1, 4, b"length %d" % (T + 1)), (rf.OFF_GRID[1], 5, b"68 frames")):
        lens = list(lengths)
        lens[at] = bad
        rc = _call(lib, which, p, lens)
        msg = lib.srf_last_error()
        assert rc == -1 and b"original" in msg and (b"example %d" % at) in msg and word in msg, msg
    # the number of parameter tensors, a null pointer
    assert _call(lib, which, p, list(lengths), num_params=p.num_params - 1) == -1 and b"original" in lib.srf_last_error()
    lens = (C.c_int * len(lengths))(*lengths)
    assert lib.srf_original_forward_ragged(p.handle, None, 0, None, lens, None, None, 0, None) == -1
    assert b"original" in lib.srf_last_error() and b"null" in lib.srf_last_error()


def test_a_plan_of_another_model_is_refused():
    from sudo_rm_rf_amd.engine import Plan
    p = Plan(("improved", 1, 256, 512, 2, 5, 21, 512, 2, 1), 4, 32000, torch.device("cpu"))
    lib = _lib()
    assert lib.srf_original_ragged_supported(p.handle) == 0 and lib.srf_original_ragged_workspace_bytes(p.handle) == 0
    for which in ("forward", "separate"):
        rc = _call(lib, which, p, [32000] * 4)
        assert rc == -1 and b"original" in lib.srf_last_error() and b"srf_original_plan_create" in lib.srf_last_error()


def test_the_kernel_entries_refuse_bad_tables_before_the_launch():
    lib = _lib()
    one = C.c_void_p(256)
    from sudo_rm_rf_amd._lib import srf_norm
    nrm = srf_norm(sums=256, gamma=256, beta=256, prelu=None)
    fr = (C.c_int * 2)(128, 130)
    assert lib.srf_gln_apply_c_ragged(one, C.byref(nrm), None, None, C.c_void_p(1 << 20), None, 2, 4, 132, fr, None) == -1
    assert b"example 1" in lib.srf_last_error() and b"multiple of 4" in lib.srf_last_error()
    fr = (C.c_int * 2)(128, 136)
    assert lib.srf_gln_apply_c_ragged(one, C.byref(nrm), None, None, C.c_void_p(1 << 20), None, 2, 4, 132, fr, None) == -1
    assert b"example 1" in lib.srf_last_error()
    lens, frames = (C.c_int * 2)(2000, 651), (C.c_int * 2)(200, 65)
    rc = lib.srf_encoder_bias_relu_ragged(one, one, one, one, None, 2, 2000, 64, 21, 200, lens, frames, None, None)
    assert rc == -1 and b"example 1" in lib.srf_last_error()
    rc = lib.srf_encoder_bias_relu_ragged(one, one, one, one, None, 2, 2000, 64, 9, 200, lens, frames, None, None)
    assert rc == -1 and b"K = 21" in lib.srf_last_error()
    assert lib.srf_softmax_mask_ragged(one, one, C.c_void_p(512), 2, 2, 8, 200, (C.c_int * 2)(200, 201), None) == -1
    assert b"example 1" in lib.srf_last_error()
    assert lib.srf_bias_rescale_ragged(one, one, None, None, 0, 2, 2, 1000, (C.c_int * 2)(0, 5), None) == -1
    assert b"example 0" in lib.srf_last_error()


@pytest.mark.parametrize("name", sorted(rf.CASES))
def test_fixtures_are_what_the_restatement_gives_row_by_row(name):
    cfg, T, lengths, wseed, _ = rf.CASES[name]
    fx = rf.load(name)
    assert fx["lengths"] == list(lengths) and fx["wav"].shape == (len(lengths), 1, T)
    assert np.array_equal(fx["wav"], rf.make_wav(name))
    sd = of.make_state_dict(cfg, wseed)
    from sudo_rm_rf_amd import original
    for b, n in enumerate(lengths):
        assert fx["out"][b].shape == (cfg["num_sources"], n)
        assert 0.1 <= float(np.abs(fx["out"][b]).max()) <= 10.0
        fr = of.frames(cfg, n)
        assert fr == original.padded_frames(n, 21, cfg["upsampling_depth"]) and fr % 16 == 0 and fr >= 64
    for b in (0, len(lengths) - 1):          # (the generator has asserted every row; two are re-run here)
        got = orf.forward(cfg, sd, fx["wav"][b:b + 1, :, :lengths[b]]).numpy()[0]
        assert np.abs(got - fx["out"][b]).max() <= 1e-5


def test_a_model_that_has_not_opted_in_is_what_it_was():
    from sudo_rm_rf_amd import pipeline
    cfg = rf.CASES["rg_b"][0]
    m = _model(cfg).eval()
    assert not hasattr(m, "separate_ragged") and "_srf_ragged" not in m.__dict__
    assert pipeline.ragged_route(m, 32000) == "single" and pipeline.ragged_route(m) == "single"
    with torch.no_grad(), pytest.raises(NotImplementedError, match="ragged"):
        m.forward_ragged(torch.zeros(2, 1, 2560), [2560, 1280])
    assert not m._engine().original_ragged
    assert "_srf_ragged" not in m.state_dict() and all("ragged" not in k for k in m.state_dict())


def test_enable_ragged_routes_by_configuration_and_length():
    from sudo_rm_rf_amd import pipeline
    cfg_b, cfg_a = rf.CASES["rg_b"][0], rf.CASES["rg_a"][0]
    m = _model(cfg_b).eval()
    assert m.enable_ragged() is m and hasattr(m, "separate_ragged") and callable(m.separate_ragged)
    assert m._engine().original_ragged
    assert pipeline.ragged_route(m) == "ragged"
    # D = 5: multiples of 160 samples = 16 frames; every length from 1280 samples on passes, shorter ones have < 8 positions on
    # the deepest level
    for n in (1280, 1281, 1441, 2401, 32000, 31999):
        assert pipeline.ragged_route(m, n) == "ragged", n
    for n in (1, 640, 1120):
        assert pipeline.ragged_route(m, n) == "single", n
    # D = 3: multiples of 40 samples = 4 frames; only the lengths whose frame count is on the 16-frame chunk grid
    a = _model(cfg_a).eval().enable_ragged()
    for n, want in ((640, "ragged"), (641, "single"), (950, "ragged"), (1900, "ragged"), (2399, "ragged"), (2000, "single"), (600, "single")):
        assert pipeline.ragged_route(a, n) == want, n
    # configurations the gate does not take stay on the per-utterance path, opted in or not
    for cfg in (of.TINY, of.DEFAULT_U2, of.S3_K9):
        assert pipeline.ragged_route(_model(cfg).enable_ragged(), 32000) == "single"
    # the Python rule is the library's: every routed length is one the entry points take
    p = _plan(cfg_a, 6, 2560)          # (batch 2 would have fewer than 8 tiles: the gate)
    lib = _lib()
    from sudo_rm_rf_amd import original
    for n in range(600, 2561, 7):
        ok = lib.srf_pyramid_ragged_frames_ok(original.padded_frames(n, 21, 3), p.frames, 3) == 1
        assert (pipeline.ragged_route(a, n) == "ragged") == ok, n
        # (only refusals are run with fake pointers: a length that passes would launch)
        if not ok:
            assert _call(lib, "forward", p, [2560, n] + [2560] * 4) == -1 and b"example 1" in lib.srf_last_error(), n


def test_the_opt_in_is_not_in_pickles_and_can_be_taken_back():
    from sudo_rm_rf_amd import pipeline
    m = _model(rf.CASES["rg_c"][0]).eval().enable_ragged()
    keys = list(m.state_dict())
    assert all("ragged" not in k for k in keys)
    back = pickle.loads(pickle.dumps(m))
    assert not hasattr(back, "separate_ragged") and pipeline.ragged_route(back, 2560) == "single"
    assert list(back.state_dict()) == keys
    assert m.enable_ragged(False) is m and not hasattr(m, "separate_ragged")
    assert pipeline.ragged_route(m, 2560) == "single" and not m._engine().original_ragged
    with torch.no_grad(), pytest.raises(NotImplementedError, match="ragged"):
        m.forward_ragged(torch.zeros(2, 1, 2560), [2560, 1280])
    with pytest.raises(AttributeError):
        m.no_such_attribute


def test_the_opted_in_model_keeps_the_ragged_checks_of_the_engine():
    from sudo_rm_rf_amd._lib import SrfError
    m = _model(rf.CASES["rg_c"][0]).eval().enable_ragged()
    with torch.no_grad():
        with pytest.raises(SrfError, match="MI355X"):
            m.forward_ragged(torch.zeros(2, 1, 2560), [2560, 1280])
        with pytest.raises(RuntimeError, match=r"\[batch, 1, time\]"):
            m.separate_ragged(torch.zeros(2, 2, 2560), [2560, 1280])
