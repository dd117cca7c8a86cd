"""Attentive v2, whole-model ragged forward on the host: exported symbols, the opt-in and what stays
pinned without it, the two gates, the refusals before any launch (fake pointers: nothing is launched) and the fixtures of
tools/make_golden_attentive_model_ragged.py.  No GPU needed."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest
import torch

from tests import attentive_fixtures as af
from tests import attentive_model_ragged_cases as mc

_model, _plan = mc.model, mc.plan

NEW_SYMBOLS = ("srf_pw_conv_ragged_supported", "srf_pw_conv_ragged", "srf_attentive_ragged_supported",
               "srf_attentive_ragged_workspace_bytes", "srf_attentive_forward_ragged", "srf_attentive_separate_ragged")
MODEL_CASES = ("a", "b", "c")


def _lib():
    from sudo_rm_rf_amd import _lib
    return _lib.load()


def _call(lib, which, plan, lengths, num_params=None):
    """srf_attentive_forward_ragged / _separate_ragged with fake (non-null, 256-byte aligned) pointers: refusals come first."""
    n = plan.num_params if num_params is None else num_params
    table = (C.c_void_p * max(n, 1))(*([256] * max(n, 1)))
    lens = (C.c_int * len(lengths))(*lengths)
    one = C.c_void_p(256)
    if which == "forward":
        return lib.srf_attentive_forward_ragged(plan.handle, table, n, one, lens, one, one, 1 << 40, None)
    return lib.srf_attentive_separate_ragged(plan.handle, table, n, one, lens, one, one, 0, one, 1 << 40, None)


def test_abi_19_and_every_new_symbol_is_declared_exported_and_bound():
    from sudo_rm_rf_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(af.ROOT, "include", "sudormrf_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and getattr(lib, name) is not None, name
        assert name + "(" in header, name
    assert lib.srf_abi_version() == 19 and _lib.ABI_VERSION == 19


def test_enable_ragged_exists_on_v2_and_not_on_v3():
    from sudo_rm_rf_amd.dnn.models import attentive_sudormrf_v2 as v2, attentive_sudormrf_v3 as v3
    assert callable(getattr(v2.SuDORMRF, "enable_ragged", None))
    assert not hasattr(v3.SuDORMRF, "enable_ragged")
    from sudo_rm_rf_amd import ragged
    assert callable(ragged.pw_conv_mfma) and callable(ragged.pw_conv_mfma_supported)


def test_separate_ragged_and_the_route_follow_the_opt_in():
    from sudo_rm_rf_amd import pipeline
    m = _model(af.TINY).eval()
    keys = list(m.state_dict())
    # before: everything pinned for the model without ragged kernels
    assert not hasattr(m, "separate_ragged") and "_srf_ragged" not in m.__dict__
    assert pipeline.ragged_route(m) == "single" and pipeline.ragged_route(m, 1001) == "single"
    assert not m._engine().attentive_ragged and not m._engine().original_ragged
    with torch.no_grad(), pytest.raises(NotImplementedError, match="no ragged kernels"):
        m.forward_ragged(torch.zeros(2, 1, 200), [200, 100])
    # after
    assert m.enable_ragged() is m and hasattr(m, "separate_ragged") and callable(m.separate_ragged)
    assert m._engine().attentive_ragged and not m._engine().original_ragged
    for n in (None, 1, 90, 1001, 32000):
        assert pipeline.ragged_route(m, n) == "ragged", n
    assert list(m.state_dict()) == keys
    back = pickle.loads(pickle.dumps(m))
    assert not hasattr(back, "separate_ragged") and pipeline.ragged_route(back, 1001) == "single"
    # and taken back
    assert m.enable_ragged(False) is m and not hasattr(m, "separate_ragged") and "_srf_ragged" not in m.__dict__
    assert pipeline.ragged_route(m) == "single" and pipeline.ragged_route(m, 1001) == "single" and not m._engine().attentive_ragged
    with torch.no_grad(), pytest.raises(NotImplementedError, match="no ragged kernels"):
        m.forward_ragged(torch.zeros(2, 1, 200), [200, 100])
    with pytest.raises(AttributeError):
        m.no_such_attribute
    # K = 9: opted in or not, the per-utterance path
    k9 = _model(dict(af.TINY, enc_kernel_size=9)).enable_ragged()
    assert pipeline.ragged_route(k9, 1001) == "single"


def test_the_opted_in_model_keeps_the_engines_checks():
    from sudo_rm_rf_amd._lib import SrfError
    m = _model(af.TINY).eval().enable_ragged()
    with torch.no_grad():
        with pytest.raises(SrfError, match="MI355X"):
            m.forward_ragged(torch.zeros(2, 1, 200), [200, 100])
        with pytest.raises(RuntimeError, match=r"\[batch, 1, time\]"):
            m.separate_ragged(torch.zeros(2, 2, 200), [200, 100])


@pytest.mark.parametrize("name", MODEL_CASES)
def test_the_models_gate_takes_the_cases_and_the_general_gate_stays_closed(name):
    cfg, lengths, _, _ = mc.CASES[name]
    p = _plan(cfg, len(lengths), max(lengths))
    lib = _lib()
    assert p.attentive_ragged_supported and lib.srf_attentive_ragged_supported(p.handle) == 1
    assert lib.srf_attentive_ragged_workspace_bytes(p.handle) == p.workspace_bytes > 0
    assert not p.ragged_supported and lib.srf_plan_ragged_supported(p.handle) == 0 and lib.srf_plan_ragged_workspace_bytes(p.handle) == 0


def test_the_models_gate_refuses_k9_v3_other_models_and_kernel_mode_1():
    from sudo_rm_rf_amd.engine import Plan
    lib = _lib()
    k9 = _plan(dict(af.TINY, enc_kernel_size=9), 3, 1008)
    assert lib.srf_attentive_ragged_supported(k9.handle) == 0 and lib.srf_attentive_ragged_workspace_bytes(k9.handle) == 0
    assert lib.srf_plan_ragged_supported(k9.handle) == 0
    assert _call(lib, "forward", k9, [1008] * 3) == -1 and b"K = 21" in lib.srf_last_error()
    tup = ("attentive_v3", 1) + tuple(af.TINY[f] for f in af.FIELDS[:6]) + (2, 1, (af.HEADS, af.ATT_DIMS))
    for other in (Plan(tup, 3, 1000, torch.device("cpu")), Plan(("improved", 1, 256, 512, 2, 5, 21, 512, 2, 1), 4, 32000, torch.device("cpu"))):
        assert lib.srf_attentive_ragged_supported(other.handle) == 0
        assert _call(lib, "separate", other, [1000] * other.batch) == -1 and b"srf_attentive_plan_create" in lib.srf_last_error()
    # a model whose masked tensor (sources x basis x frames floats) cannot hold the one statistics slot the walk keeps in it
    small = _plan(dict(af.TINY, enc_num_basis=8, upsampling_depth=2), 2, 20)
    assert small.frames == 2 and lib.srf_attentive_ragged_supported(small.handle) == 0
    assert _call(lib, "forward", small, [20, 10]) == -1 and b"too small" in lib.srf_last_error()
    p = _plan(af.TINY, 3, 1001)
    assert p.attentive_ragged_supported
    lib.srf_set_kernel_mode(1)
    try:
        assert not p.attentive_ragged_supported and lib.srf_attentive_ragged_workspace_bytes(p.handle) == 0
    finally:
        lib.srf_set_kernel_mode(0)
    assert p.attentive_ragged_supported


@pytest.mark.parametrize("which", ["forward", "separate"])
def test_model_refusals_come_before_any_launch_and_name_the_example(which):
    cfg, lengths, _, _ = mc.CASES["a"]
    T = max(lengths)
    p = _plan(cfg, len(lengths), T)
    lib = _lib()
    for bad, at, word in ((0, 1, b"length 0"), (T + 1, 2, b"length %d" % (T + 1)), (-5, 0, b"length -5")):
        lens = list(lengths)
        lens[at] = bad
        rc = _call(lib, which, p, lens)
        msg = lib.srf_last_error()
        assert rc == -1 and (b"example %d" % at) in msg and word in msg, msg
    assert _call(lib, which, p, list(lengths), num_params=p.num_params - 1) == -1
    lens = (C.c_int * len(lengths))(*lengths)
    assert lib.srf_attentive_forward_ragged(p.handle, None, 0, None, lens, None, None, 0, None) == -1 and b"null" in lib.srf_last_error()
    # the general entry points keep refusing the plan
    table = (C.c_void_p * p.num_params)(*([256] * p.num_params))
    one = C.c_void_p(256)
    assert lib.srf_forward_ragged(p.handle, table, p.num_params, one, lens, one, one, 1 << 40, None) == -1
    assert b"attentive" in lib.srf_last_error()


@pytest.mark.parametrize("Cin", [48, 64])
@pytest.mark.parametrize("Cout", [16, 32])
@pytest.mark.parametrize("L", [130, 132])
def test_truth_table_of_the_kernels_gate(Cin, Cout, L):
    lib = _lib()
    shape_ok = Cin == 64 and Cout == 32 and L == 132
    fr = lambda *v: (C.c_int * len(v))(*v)
    assert lib.srf_pw_conv_ragged_supported(3, Cin, Cout, L, fr(L, L - 3, 1)) == int(shape_ok)
    assert lib.srf_pw_conv_ragged_supported(3, Cin, Cout, L, fr(L, 0, 1)) == 0
    assert lib.srf_pw_conv_ragged_supported(3, Cin, Cout, L, fr(L, 5, L + 1)) == 0
    assert lib.srf_pw_conv_ragged_supported(3, Cin, Cout, L, None) == 0
    assert lib.srf_pw_conv_ragged_supported(0, Cin, Cout, L, fr(L)) == 0
    from sudo_rm_rf_amd import ragged
    assert ragged.pw_conv_mfma_supported(3, Cin, Cout, L, [L, L - 3, 1]) == shape_ok
    assert not ragged.pw_conv_mfma_supported(2, Cin, Cout, L, [L, L - 3, 1])          # (a table of another batch)
    if shape_ok:
        lib.srf_set_kernel_mode(2)
        try:
            assert lib.srf_pw_conv_ragged_supported(3, Cin, Cout, L, fr(L, L - 3, 1)) == 0
        finally:
            lib.srf_set_kernel_mode(0)
        assert lib.srf_pw_conv_ragged_supported(129, Cin, Cout, L, (C.c_int * 129)(*([L] * 129))) == 0
        # the 32-bit reach of the buffer loads: 2 x 8192 x 32768 floats = 2 GB
        assert lib.srf_pw_conv_ragged_supported(2, 8192, 32, 32768, fr(32768, 4)) == 0
        assert lib.srf_pw_conv_ragged_supported(1, 8192, 32, 32768, fr(32768)) == 1


def test_the_kernel_entry_refuses_before_any_launch_naming_the_example():
    lib = _lib()
    one, y = C.c_void_p(256), C.c_void_p(1 << 20)
    fr = lambda *v: (C.c_int * len(v))(*v)
    call = lambda x, w, frames, Bt=3, Cin=64, Cout=32, L=132, res=None: lib.srf_pw_conv_ragged(
        x, w, one, y, Bt, Cin, Cout, L, None, res, None, frames, None)
    assert call(one, one, fr(132, 0, 1)) == -1 and b"example 1" in lib.srf_last_error() and b"0 frames" in lib.srf_last_error()
    assert call(one, one, fr(132, 5, 133)) == -1 and b"example 2" in lib.srf_last_error() and b"133 frames" in lib.srf_last_error()
    assert call(one, one, None) == -1 and b"null" in lib.srf_last_error()
    assert call(None, one, fr(132, 5, 1)) == -1 and b"null pointer" in lib.srf_last_error()
    assert call(one, one, fr(48, 5, 1), Cin=48) == -1 and b"does not take" in lib.srf_last_error()
    assert call(one, one, fr(130, 5, 1), L=130) == -1 and b"does not take" in lib.srf_last_error()
    assert call(one, one, fr(132, 5, 1), Cout=16) == -1 and b"does not take" in lib.srf_last_error()
    assert call(C.c_void_p(260), one, fr(132, 5, 1)) == -1 and b"'x'" in lib.srf_last_error() and b"16-byte" in lib.srf_last_error()
    assert call(one, C.c_void_p(264), fr(132, 5, 1)) == -1 and b"'w'" in lib.srf_last_error()
    assert call(one, one, fr(132, 5, 1), res=C.c_void_p(260)) == -1 and b"'residual'" in lib.srf_last_error()


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_fixtures_hold_every_row_alone_and_no_row_is_near_silence(name):
    cfg, lengths, wseed, iseed = mc.CASES[name]
    fx, meta = mc.load(name), mc.load_manifest()["cases"][name]
    assert fx["lengths"] == list(lengths) == meta["lengths"] and meta["config"] == cfg
    assert (meta["weight_seed"], meta["input_seed"]) == (wseed, iseed)
    D = cfg["upsampling_depth"]
    for b, n in enumerate(lengths):
        assert fx["out"][b].shape == (cfg["num_sources"], n) and fx["out"][b].dtype == np.float32
        amax = float(np.abs(fx["out"][b]).max())
        assert amax == pytest.approx(meta["max_abs_out"][b], rel=1e-6) and amax >= 100 * mc.BAR, (name, b, amax)
        fr = mc.frames(cfg, n)
        assert fr == meta["frames"][b] and fr % (1 << (D - 1)) == 0 and fr <= mc.frames(cfg, max(lengths))
    expect = {"a": ([104, 64, 12], [26, 16, 3]), "b": ([200, 130, 42], [100, 65, 21]), "c": ([128, 80, 36], [32, 20, 9]),
              "d": ([1040, 520], [130, 65])}[name]
    assert (meta["frames"], meta["deepest"]) == (expect[0], expect[1])
    assert os.path.getsize(mc.path(name)) < (1 << 20)


def test_fixture_a_is_what_the_restatement_gives_on_the_row_alone():
    """tests/attentive_ref.py (fp64) on rows 0 and 2 of case a, at their own lengths, against the reference's stored outputs"""
    from tests import attentive_ref as ar
    cfg, lengths, wseed, _ = mc.CASES["a"]
    sd = {k: torch.from_numpy(v).double() for k, v in af.make_state_dict(cfg, wseed).items()}
    wav, fx = mc.make_wav("a"), mc.load("a")
    for b in (0, 2):
        got = ar.forward(cfg, sd, torch.from_numpy(wav[b:b + 1, :, :lengths[b]]).double())
        assert np.abs(got[0].numpy() - fx["out"][b]).max() <= 1e-5
