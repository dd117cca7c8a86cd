"""Causal SuDoRM-RF (v3) on the host: module schema, seeded weights and pickles against fixtures made by the reference
(tools/make_golden_causal.py), plan geometry, the refusals and every byte count / launch count of a plan and of a streaming
session as literals.  No GPU needed."""
import ctypes as C
import hashlib
import os

import pytest
import torch

from tests import causal_fixtures as cf


@pytest.fixture(scope="module")
def man():
    return cf.load_manifest()


def _model(cfg):
    from sudo_rm_rf_amd.dnn.models.causal_improved_sudormrf_v3 import CausalSuDORMRF
    return CausalSuDORMRF(**cfg)


def _plan(cfg, batch, T, group_size=1):
    from sudo_rm_rf_amd.engine import Plan
    tup = ("causal",) + tuple(cfg[f] for f in cf.FIELDS) + (group_size,)
    return Plan(tup, batch, T, torch.device("cpu"))


@pytest.mark.parametrize("name", sorted(cf.CASES))
def test_schema_and_order_match_manifest(man, name):
    meta = man["cases"][name]
    cfg = meta["config"]
    sd = _model(cfg).state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, tuple(s)) for k, s in cf.schema(cfg)]
    U, D = cfg["num_blocks"], cfg["upsampling_depth"]
    assert len(sd) == 3 + U * (6 + 3 * D) + 5
    assert sum(v.numel() for v in sd.values()) == meta["num_params"]


def test_parameter_counts_of_the_reference_configs():
    assert sum(v.numel() for v in _model(cf.DEFAULTS).state_dict().values()) == 3090146
    assert sum(v.numel() for v in _model(cf.MAIN).state_dict().values()) == 2148638


@pytest.mark.parametrize("tag", ["tiny", "main"])
def test_same_seed_gives_the_reference_weights(man, tag):
    ref = man["digests"][tag]
    torch.manual_seed(ref["seed"])
    m = _model(ref["config"])
    got = [[k, list(v.shape), hashlib.sha256(v.detach().contiguous().numpy().tobytes()).hexdigest()]
           for k, v in m.state_dict().items()]
    assert got == ref["state_dict"]
    for a, v in ref["attributes"].items():
        assert getattr(m, a) == v, a
    enc = m.encoder
    K = ref["config"]["enc_kernel_size"]
    assert torch.equal(enc.causal_mask[..., :K], torch.ones_like(enc.causal_mask[..., :K]))
    assert not enc.causal_mask[..., K:].any()
    assert all(b.alpha == 1.0 and b.beta == 1.0 for b in m.sm)


def test_both_import_paths_resolve():
    import sudo_rm_rf.dnn.models.causal_improved_sudormrf_v3 as shim
    import sudo_rm_rf_amd.dnn.models.causal_improved_sudormrf_v3 as ours
    for n in ("ScaledWSConv1d", "ConvAct", "UConvBlock", "CausalSuDORMRF"):
        assert getattr(shim, n) is getattr(ours, n)


def test_reference_pickle_unpickles_into_our_classes(man):
    from sudo_rm_rf_amd.dnn.models.causal_improved_sudormrf_v3 import CausalSuDORMRF, ScaledWSConv1d, UConvBlock
    meta = man["pickle"]
    m = torch.load(os.path.join(cf.GOLDEN, meta["file"]), weights_only=False)
    assert type(m) is CausalSuDORMRF
    assert isinstance(m.encoder, ScaledWSConv1d) and isinstance(m.sm[0], UConvBlock)
    torch.manual_seed(meta["seed"])
    want = _model(meta["config"]).state_dict()
    got = m.state_dict()
    assert list(got) == list(want)
    assert all(torch.equal(got[k], want[k]) for k in want)
    assert m.sm[0].alpha == 1.0 and m.sm[0].beta == 1.0
    assert m.encoder.causal_mask.shape == m.encoder.weight.shape
    assert m._config_tuple()[0] == "causal"


@pytest.mark.parametrize("name", sorted(cf.CASES))
def test_plan_geometry_follows_the_padding_rule(man, name):
    meta = man["cases"][name]
    cfg = meta["config"]
    p = _plan(cfg, meta["batch"], meta["T"])
    h = cfg["enc_kernel_size"] // 2
    n = h * 2 ** cfg["upsampling_depth"]
    T = meta["T"]
    Tp = n if T < n else -(-T // n) * n
    assert (p.padded_length, p.frames) == (Tp, Tp // h) == (meta["padded_length"], meta["frames"])
    assert p.num_params == len(cf.schema(cfg))
    assert _model(cfg).n_least_samples_req == n


def test_cpu_input_fails_loudly():
    from sudo_rm_rf_amd._lib import SrfError
    m = _model(cf.TINY).eval()
    with torch.no_grad(), pytest.raises(SrfError, match="MI355X"):
        m(torch.zeros(1, 1, 200))


def test_invalid_configs_are_refused():
    from sudo_rm_rf_amd._lib import SrfError
    with pytest.raises(AssertionError):
        _model(dict(cf.TINY, enc_kernel_size=20))
    with pytest.raises(SrfError, match="odd"):
        _plan(dict(cf.TINY, enc_kernel_size=20), 1, 1000)
    with pytest.raises(SrfError, match="group_size"):
        _plan(cf.TINY, 1, 1000, group_size=2)


def test_training_is_refused_before_anything_runs():
    from sudo_rm_rf_amd import _lib
    m = _model(cf.TINY)
    with pytest.raises(NotImplementedError, match="forward-only"):
        m(torch.zeros(1, 1, 200))
    p = _plan(cf.TINY, 1, 1000)
    lib = _lib.load()
    assert lib.srf_train_saved_bytes(p.handle) == 0 and lib.srf_train_scratch_bytes(p.handle) == 0
    rc = lib.srf_forward_train(p.handle, None, 0, None, None, None, 0, None, 0, None)
    assert rc == -1 and b"causal" in lib.srf_last_error()
    for fn in ("srf_backward", "srf_backward_wav"):
        args = [p.handle, None, None, 0, None, None, None, 0, None, 0] + ([C.c_void_p(16)] if fn.endswith("wav") else []) + [None]
        assert getattr(lib, fn)(*args) == -1 and b"causal" in lib.srf_last_error()
    rc = lib.srf_separate(p.handle, None, 0, C.c_void_p(16), None, C.c_void_p(16), 0, None, 0, None)
    assert rc == -1 and b"causal" in lib.srf_last_error()


# ---- byte and count literals ------------------------------------------------------------------------------------------------
# Recorded on commit 13ee426, the commit BEFORE causal_plan_create, the training layouts and srf_stream_create took the causal
# parameter layout from srf_plan.h: whatever spells the layout, these numbers stay.
SIZE_CASES = ("causal_tiny", "causal_tiny_a2_k11", "causal_default", "causal_main")      # TINY, TINY_A2, DEFAULTS, MAIN
PLAN_SIZES = {      # (workspace bytes, parameters, launches, frames, training saved bytes, training scratch bytes)
    "causal_tiny": (502784, 38, 15, 104, 638976, 705792),
    "causal_tiny_a2_k11": (1636608, 32, 15, 156, 1857024, 2754816),
    "causal_default": (213487872, 296, 57, 3200, 1815347200, 237105408),
    "causal_main": (109876736, 92, 21, 4416, 210272256, 138257920),
}
STREAM_SIZES = {      # (weights, state, workspace) bytes of a session at the case's batch, max_chunk_samples = 4 granules
    "causal_tiny": (128000, 31232, 54528),
    "causal_tiny_a2_k11": (230144, 31488, 67840),
    "causal_default": (12385280, 5243904, 1463296),
    "causal_main": (8602112, 410112, 1070080),
}


def plan_sizes(name):
    """(workspace bytes, parameters, launches, frames, training saved bytes, training scratch bytes) at the case's batch and T"""
    from sudo_rm_rf_amd import _lib
    cfg, batch, T = cf.CASES[name][:3]
    p = _plan(cfg, batch, T)
    lib = _lib.load()
    return (p.workspace_bytes, p.num_params, p.num_launches, p.frames, lib.srf_causal_train_saved_bytes(p.handle),
            lib.srf_causal_train_scratch_bytes(p.handle))


def stream_sizes(name):
    """(weights, state, workspace) bytes of a session of the case's configuration and batch at max_chunk_samples = 4 granules"""
    from sudo_rm_rf_amd.streaming import _Session
    cfg, batch = cf.CASES[name][:2]
    g = (cfg["enc_kernel_size"] // 2) << (cfg["upsampling_depth"] - 1)
    s = _Session(("causal",) + tuple(cfg[f] for f in cf.FIELDS) + (1,), batch, 4 * g)
    assert s.granule == g
    return s.weights_bytes, s.state_bytes, s.workspace_bytes


@pytest.mark.parametrize("name", SIZE_CASES)
def test_plan_and_training_sizes_are_what_they_were(name):
    assert plan_sizes(name) == PLAN_SIZES[name]


@pytest.mark.parametrize("name", SIZE_CASES)
def test_stream_session_sizes_are_what_they_were(name):
    assert stream_sizes(name) == STREAM_SIZES[name]
