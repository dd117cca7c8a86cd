"""The fp64 restatements against the reference's own outputs on degenerate signals (tests/golden/edge_<family>.npz, written by
tools/make_golden_edges.py from the unmodified reference): silence, DC, near-silence, loud input and exact zeros are where the
1e-8 of a norm, the 1e-9 of the waveform normalisation and a misplaced epsilon decide the answer, so the yardsticks the GPU tests
use are pinned there too.  Bar: 1e-5, the one every generator holds its restatement to (x max(1, max |out|) for loud outputs).
No GPU."""
import numpy as np
import pytest

from tests import edge_signals as es


@pytest.fixture(scope="module")
def manifest():
    return es.load_manifest()


def test_signal_set_is_what_the_manifest_was_made_from(manifest):
    assert manifest["signal_seed"] == es.SEED and sorted(manifest["families"]) == sorted(es.FAMILIES)
    s = es.signals(3, 2, 1001)
    assert tuple(s) == es.NAMES and all(v.shape == (3, 2, 1001) and v.dtype == np.float32 for v in s.values())
    assert not s["silence"].any() and (s["dc"] == np.float32(0.37)).all()
    assert not s["half_silent"][..., 500:].any() and s["half_silent"][..., :500].all()
    assert not s["one_silent_row"][0].any() and s["one_silent_row"][1:].all()
    assert (s["impulse"].sum(-1) == 1.0).all() and (np.count_nonzero(s["impulse"], axis=-1) == 1).all()
    assert 1e-9 < np.abs(s["near_silent"]).max() < 1e-7 and 1e-7 < np.abs(s["tiny"]).max() < 1e-5
    assert np.abs(s["loud"]).max() > 1e3
    again = es.signals(3, 2, 1001)
    assert all(np.array_equal(s[k], again[k]) for k in s)
    for family, (batch, T, wseed, recipes) in es.FAMILIES.items():
        meta = manifest["families"][family]
        assert (meta["batch"], meta["T"], meta["weight_seed"], tuple(meta["recipes"])) == (batch, T, wseed, recipes)
        keys = [es.case_key(n) for n in es.NAMES] + [es.case_key(n, mc) for n in es.NAMES for mc in recipes]
        assert sorted(meta["cases"]) == sorted(keys)


@pytest.mark.parametrize("family", sorted(es.FAMILIES))
def test_restatement_matches_the_reference_on_every_signal(manifest, family):
    gold, meta = es.load_golden(family), manifest["families"][family]["cases"]
    sd = es.state_dict(family)
    recipes = es.FAMILIES[family][3]
    for signal, wav in es.family_signals(family).items():
        runs = [(es.case_key(signal), lambda: es.restatement(family, sd, wav))]
        runs += [(es.case_key(signal, mc), lambda mc=mc: es.recipe(family, sd, wav, mc)) for mc in recipes]
        for key, fn in runs:
            want, m = gold[key], meta[key]
            got = fn().numpy()
            assert got.shape == want.shape and np.isfinite(got).all(), key
            amax = float(np.abs(want).max())
            err = float(np.abs(got - want.astype(np.float64)).max())
            print("%s %s: max|restatement - reference| %.3e (max|ref| %.3e)" % (family, key, err, amax))
            assert amax == m["max_abs_out"] and bool(not want.any()) == m["identically_zero"], key
            assert err <= es.RESTATEMENT_TOL * max(1.0, amax), (family, key, err)
            if m["identically_zero"]:
                assert not got.any(), key


@pytest.mark.parametrize("family", ["attn", "attn3", "orig"])
def test_named_recipe_restatements_match_the_reference(manifest, family):
    """attentive_ref.separate, attentive_v3_ref.separate and original_ref.separate -- the recipe yardsticks of the families' own
    GPU tests -- against the same goldens (the attentive ones have no mixture consistency; the original one has both settings)."""
    import importlib
    mod = importlib.import_module("tests." + {"attn": "attentive_ref", "attn3": "attentive_v3_ref", "orig": "original_ref"}[family])
    gold, cfg, sd = es.load_golden(family), es.config(family), es.state_dict(family)
    for signal, wav in es.family_signals(family).items():
        for mc in ((False, True) if family == "orig" else (False,)):
            got = (mod.separate(cfg, sd, wav, mixture_consistency=mc) if family == "orig" else mod.separate(cfg, sd, wav)).numpy()
            want = gold[es.case_key(signal, mc)].astype(np.float64)
            err = float(np.abs(got - want).max())
            assert np.isfinite(got).all() and err <= es.RESTATEMENT_TOL * max(1.0, float(np.abs(want).max())), (family, signal, mc, err)


def test_silence_is_identically_zero_only_where_nothing_adds_a_bias(manifest):
    """Mask times encoder with no encoder bias: silence in, exact zeros out (improved, GroupComm, both attentive models); the
    causal model's decoder sees its mask net's biases, the original model's encoder has a bias: their silence is not zero."""
    zero = {f: manifest["families"][f]["cases"]["silence"]["identically_zero"] for f in es.FAMILIES}
    assert zero == {"improved": True, "groupcomm": True, "attn": True, "attn3": True, "causal": False, "orig": False}
    for f, meta in manifest["families"].items():
        for key, m in meta["cases"].items():
            # the recipe gives silence back as exact zeros whatever the model: it multiplies by std = 0 and adds mean = 0.  (With
            # mixture consistency DC comes back as zeros as well: mean + (0 - S mean) / S, the consistency being taken against
            # the NORMALISED mixture, as the README has it.)
            if key in ("separate_silence", "separate_mc_silence", "separate_mc_dc"):
                assert m["identically_zero"], (f, key)
            elif key != "silence":
                assert not m["identically_zero"], (f, key)


def test_bars():
    assert es.inference_bar(0.25, False) == 2e-4 * 0.25 + 1e-6
    assert es.inference_bar(1e-7, False) == 2e-4 * 1e-7               # no absolute term below 1e-3
    assert es.inference_bar(0.0, True) == 1e-6
    assert es.inference_bar(0.25, False, 1e-4) == 8e-4
    assert es.recipe_bar(np.zeros(100, np.float32)) == 1e-4 and es.recipe_bar(np.arange(100.0)) > 1e-3
