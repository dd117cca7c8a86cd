"""What dnn/models/_base.py gives the six top-level models (CPU, nothing is launched): the engine plumbing, what stays out of
pickles and copies, which classes have an enable_hip_training(), the reference's two pad_to_appropriate_length rules and the
input refusals of every forward."""
import copy
import inspect
import math
import pickle

import pytest
import torch

from tests import attentive_fixtures, attentive_v3_fixtures, causal_fixtures, original_fixtures

MODULES = ("improved_sudormrf", "groupcomm_sudormrf_v2", "causal_improved_sudormrf_v3", "sudormrf", "attentive_sudormrf_v2",
           "attentive_sudormrf_v3")
# name: (module, class, smallest fixture configuration, pad rule, single stream only)
MODELS = {
    "improved": ("improved_sudormrf", "SuDORMRF", dict(out_channels=16, in_channels=32, num_blocks=2, upsampling_depth=3,
                                                       enc_kernel_size=21, enc_num_basis=24, num_sources=2), "n_req", False),
    "groupcomm": ("groupcomm_sudormrf_v2", "GroupCommSudoRmRf",
                  dict(in_audio_channels=2, out_channels=32, in_channels=64, num_blocks=1, upsampling_depth=2,
                       enc_kernel_size=11, enc_num_basis=16, num_sources=2, group_size=8), "n_req", False),
    "causal": ("causal_improved_sudormrf_v3", "CausalSuDORMRF", causal_fixtures.TINY_A2, "n_req", False),
    "original": ("sudormrf", "SuDORMRF", original_fixtures.PICKLE, "lcm", True),
    "attentive_v2": ("attentive_sudormrf_v2", "SuDORMRF", attentive_fixtures.PICKLE, "lcm", True),
    "attentive_v3": ("attentive_sudormrf_v3", "SuDORMRF", attentive_v3_fixtures.PICKLE, "lcm", True),
}
OPT_IN = {("causal_improved_sudormrf_v3", "CausalSuDORMRF"), ("sudormrf", "SuDORMRF"), ("attentive_sudormrf_v2", "PositionalEncoding"),
          ("attentive_sudormrf_v2", "MHAttentionLayer"), ("attentive_sudormrf_v2", "TransformerLayer"),
          ("attentive_sudormrf_v2", "AttentiveUConvBlock")}


def _module(name):
    return __import__("sudo_rm_rf_amd.dnn.models." + name, fromlist=[name])


def _model(name):
    mod, cls, cfg, _, _ = MODELS[name]
    return getattr(_module(mod), cls)(**cfg)


def _all_opted_in(name):
    """A model after everything that leaves an _srf_* key behind: the engine and every opt-in the class has."""
    m = _model(name)
    m._engine()
    for opt_in in ("enable_hip_training", "enable_ragged"):
        if hasattr(m, opt_in):
            assert getattr(m, opt_in)() is m
    assert any(k.startswith("_srf_") for k in m.__dict__)
    return m


def _srf_keys(module):
    return sorted(k for m in module.modules() for k in m.__dict__ if k.startswith("_srf_"))


@pytest.mark.parametrize("name", sorted(MODELS))
def test_nothing_of_the_engine_layer_is_pickled_or_copied(name):
    m = _all_opted_in(name)
    for clone in (pickle.loads(pickle.dumps(m)), copy.deepcopy(m)):
        assert type(clone) is type(m) and _srf_keys(clone) == []
        assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), clone.state_dict().values()))
        assert clone._engine() is not m._engine() and clone._engine().cfg_tuple == m._engine().cfg_tuple
    assert _srf_keys(m) != []                      # (the original keeps what it had)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_state_dict_keys_are_those_of_a_fresh_model(name):
    torch.manual_seed(7)
    fresh = _model(name)
    torch.manual_seed(7)
    m = _all_opted_in(name)
    assert list(m.state_dict().keys()) == list(fresh.state_dict().keys())
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), fresh.state_dict().values()))


@pytest.mark.parametrize("name", sorted(MODELS))
def test_engine_is_cached_until_the_configuration_changes(name):
    m = _model(name)
    eng = m._engine()
    assert m._engine() is eng and eng.cfg_tuple == m._config_tuple()
    assert eng.multi_stream == (not MODELS[name][4])
    m.num_sources += 1
    new = m._engine()
    assert new is not eng and new.cfg_tuple == m._config_tuple() != eng.cfg_tuple
    assert m._engine() is new and new.multi_stream == eng.multi_stream


def test_single_stream_models_are_exactly_the_original_and_the_attentive_ones():
    assert sorted(n for n in MODELS if not _model(n)._engine().multi_stream) == ["attentive_v2", "attentive_v3", "original"]


def test_original_ragged_follows_the_flag_on_every_engine_call():
    m = _model("original")
    eng = m._engine()
    assert not eng.original_ragged
    m.enable_ragged()
    assert m._engine() is eng and eng.original_ragged and hasattr(m, "separate_ragged")
    m.enable_ragged(False)
    assert m._engine() is eng and not eng.original_ragged and not hasattr(m, "separate_ragged")
    assert not _model("causal")._engine().original_ragged


def test_classes_with_an_opt_in_are_exactly_the_six():
    classes = {}
    for mod in MODULES:
        for cls_name, cls in inspect.getmembers(_module(mod), inspect.isclass):
            if issubclass(cls, torch.nn.Module) and cls.__module__.startswith("sudo_rm_rf_amd.dnn.models."):
                classes[(cls.__module__.rsplit(".", 1)[1], cls.__name__)] = cls
    assert {mod for mod, _ in classes} >= set(MODULES) and len(classes) > 20
    assert {key for key, cls in classes.items() if hasattr(cls, "enable_hip_training")} == OPT_IN
    for name in ("improved", "groupcomm", "attentive_v2", "attentive_v3"):
        assert not hasattr(_model(name), "enable_hip_training")
    assert not hasattr(_module("attentive_sudormrf_v3").ConditionalTransformerLayer, "enable_hip_training")
    assert not hasattr(_module("attentive_sudormrf_v3").AttentiveUConvBlock, "enable_hip_training")


@pytest.mark.parametrize("key", sorted(OPT_IN))
def test_opt_in_flag_is_set_cleared_and_dropped(key):
    cls = getattr(_module(key[0]), key[1])
    top = [n for n, v in MODELS.items() if v[:2] == key]
    m = _model(top[0]) if top else {"PositionalEncoding": lambda: cls(8, 0.1, 16), "MHAttentionLayer": lambda: cls(8, 4, 2),
                                    "TransformerLayer": lambda: cls(8, 4, 2, max_len=16),
                                    "AttentiveUConvBlock": lambda: cls(8, 8, 2, 2, 4)}[key[1]]()
    probe = torch.zeros(1, requires_grad=True)
    assert "_srf_hip_training" not in m.__dict__ and not m._wants_grad(probe)
    assert m.enable_hip_training() is m and m.__dict__["_srf_hip_training"] is True
    assert m._wants_grad(None, probe)
    # (nothing passed in: the module's own parameters count; PositionalEncoding has a buffer and no parameter)
    assert m._wants_grad(None, probe.detach()) == (len(list(m.parameters())) > 0)
    with torch.no_grad():
        assert not m._wants_grad(probe)
    owned = [s for s in m.modules() if hasattr(s, "enable_hip_training")]
    assert all(s.__dict__.get("_srf_hip_training") for s in owned)
    assert "_srf_hip_training" not in m.state_dict()
    assert _srf_keys(pickle.loads(pickle.dumps(m))) == [] and _srf_keys(copy.deepcopy(m)) == []
    assert m.enable_hip_training(False) is m and _srf_keys(m) in ([], ["_srf_engine"])


def _reference_padded_length(rule, cfg, length):
    """The reference's two formulas (improved_sudormrf.py: up to a multiple of n_least_samples_req, at least one; sudormrf.py:
    up to a multiple of lcm, only when the length is not one)."""
    hop, span = cfg["enc_kernel_size"] // 2, 2 ** cfg["upsampling_depth"]
    if rule == "n_req":
        n = hop * span
        return n if length < n else (length // n + (1 if length % n else 0)) * n
    lcm = abs(hop * span) // math.gcd(hop, span)
    return length + lcm - length % lcm if length % lcm else length


@pytest.mark.parametrize("name", sorted(MODELS))
def test_pad_to_appropriate_length_follows_the_reference_rule(name):
    _, _, cfg, rule, _ = MODELS[name]
    m = _model(name)
    unit = m.n_least_samples_req if rule == "n_req" else m.lcm
    assert unit == _reference_padded_length(rule, cfg, 1)
    for length in (unit - 1, unit, unit + 1):
        x = torch.arange(1, 2 * length + 1, dtype=torch.float64).reshape(2, 1, length)
        padded = m.pad_to_appropriate_length(x)
        want = _reference_padded_length(rule, cfg, length)
        assert tuple(padded.shape) == (2, 1, want), (length, tuple(padded.shape))
        assert torch.equal(padded[..., :length].double(), x) and not padded[..., length:].any()
        # (the lcm rule hands a length that fits back as it is; every other result is a fresh float32 tensor)
        assert padded is x if (rule == "lcm" and want == length) else padded.dtype == torch.float32
        assert torch.equal(m.remove_trailing_zeros(padded, x).double(), x)
        assert torch.equal(type(m).remove_trailing_zeros(padded, x).double(), x)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_forward_refuses_cpu_tensors_wrong_ranks_and_non_tensors(name):
    from sudo_rm_rf_amd._lib import SrfError
    m = _model(name).eval()
    channels = getattr(m, "in_audio_channels", 1)
    with torch.no_grad():
        with pytest.raises(SrfError, match="no CPU"):
            m(torch.zeros(1, channels, 400))
        with pytest.raises(RuntimeError, match="expected input of shape"):
            m(torch.zeros(1, 400))
        with pytest.raises(TypeError, match="must be a torch.Tensor"):
            m([0.0] * 400)
    assert m._engine().last_plan is None
