"""Silence, DC and extreme levels through the models on the GPU (tests/edge_signals.py has the signal set, the families and the
bars): the inference forward of the causal, the two attentive and the original model, pipeline.separate of every family with and
without mixture consistency, and the causal model's streaming sessions.  (The improved and the GroupComm forward run the same signals in
test_degenerate_inputs_match_oracle of tests/test_gpu_model.py, the ragged paths in tests/test_gpu_ragged*.py and
tests/test_gpu_separate_ragged*.py, the training steps in tests/test_gpu_edge_train.py.)

Reference: the fp64 restatement of each family, pinned to the reference's own outputs on these very signals by
tests/test_edge_golden.py.  Bars: edge_signals.inference_bar and edge_signals.recipe_bar.  Every figure is printed before it is
asserted; profiles/edge_signals.txt holds the ones measured on an MI355X."""
import functools

import numpy as np
import pytest
import torch

from tests import edge_signals as es
from tests.causal_stream_ref import schedule_chunks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_LINES = {"inference": [], "recipe": [], "stream": []}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    from sudo_rm_rf_amd import _lib, ops
    _lib.load()
    ops.set_kernel_mode(0)
    ops.set_debug_flags(0)
    yield
    for section, lines in _LINES.items():
        if lines:
            es.write_profile_lines(section, lines)


@functools.lru_cache(maxsize=None)
def family_model(family):
    """(model on the GPU in eval mode, state dict): made once, shared, never written to"""
    cfg, sd = es.config(family), es.state_dict(family)
    torch.manual_seed(0)
    m = es.module_class(family)(**(cfg.ctor_kwargs() if hasattr(cfg, "ctor_kwargs") else cfg))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(DEV).eval(), sd


@functools.lru_cache(maxsize=None)
def references(family):
    """signal -> fp64 restatement output (numpy): computed once per family"""
    _, sd = family_model(family)
    return {name: es.restatement(family, sd, wav).numpy() for name, wav in es.family_signals(family).items()}


@pytest.mark.parametrize("signal", es.NAMES)
@pytest.mark.parametrize("family", ["causal", "attn", "attn3", "orig"])
def test_inference_forward(family, signal):
    m, _ = family_model(family)
    wav = es.family_signals(family)[signal]
    with torch.no_grad():
        got = m(torch.from_numpy(wav).to(DEV))
    torch.cuda.synchronize()
    es.check_inference(family, signal, got.cpu().numpy(), references(family)[signal], _LINES["inference"])


RECIPES = [(f, mc) for f in es.FAMILIES for mc in es.FAMILIES[f][3]]


@pytest.mark.parametrize("signal", es.NAMES)
@pytest.mark.parametrize("family,mc", RECIPES, ids=["%s%s" % (f, "_mc" if mc else "") for f, mc in RECIPES])
def test_separate_recipe(family, mc, signal):
    """pipeline.separate against the recipe restatement: 1e-4 max(1, std) per example.  Silence comes back finite (and, its std
    being 0 against the 1e-9, as the zeros the restatement gives); the listed form of each row is held to the same bar."""
    from sudo_rm_rf_amd import pipeline
    m, sd = family_model(family)
    wav = es.family_signals(family)[signal]
    want = es.recipe(family, sd, wav, mc).numpy()
    x = torch.from_numpy(wav).to(DEV)
    got = pipeline.separate(m, x, mixture_consistency=mc).cpu().numpy()
    listed = pipeline.separate_list(m, [x[b, 0] for b in range(x.shape[0])], mixture_consistency=mc)
    assert got.shape == want.shape and np.isfinite(got).all(), (family, signal)
    for b in range(wav.shape[0]):
        bar = es.recipe_bar(wav[b])
        err = float(np.abs(got[b] - want[b]).max())
        err_l = float(np.abs(listed[b].cpu().numpy() - want[b]).max())
        line = "%-9s mc=%-5s %-15s row %d err %.3e listed %.3e bar %.3e (max|want| %.3e)" % (
            family, mc, signal, b, err, err_l, bar, float(np.abs(want[b]).max()))
        print(line)
        _LINES["recipe"].append(line)
        assert err <= bar and err_l <= bar, line


# ---- the causal model's streaming sessions ------------------------------------------------------------------------------------
RAGGED_CHUNKS = (7, 133, 1, 64, 250, 3, 415, 2000)       # the ragged schedule of tests/test_gpu_causal_stream.py


def _stream_all(s, x, sizes):
    outs = [s.push(x[..., a:b]) for a, b in schedule_chunks(x.shape[-1], sizes)]
    outs.append(s.finish())
    torch.cuda.synchronize()
    return torch.cat(outs, dim=-1)


@pytest.mark.parametrize("signal", es.NAMES)
def test_causal_stream_schedules(signal):
    """stream() in granule-sized and ragged chunks, held to what tests/test_gpu_causal_stream.py requires of ordinary signals: the
    schedules give the same bits (the invariance rule), and those are the whole-signal forward's samples within the bar -- not
    its bits: a session runs its 1x1 convs in exact fp32, the forward in split bf16 (measured on an MI355X: 6e-7 .. 1e-6 apart
    at max|out| 0.13, 3e-4 at 44 for `loud`, on these signals as on the fixtures')."""
    m, _ = family_model("causal")
    x = torch.from_numpy(es.family_signals("causal")[signal]).to(DEV)
    with torch.no_grad():
        whole = m(x)
        s = m.stream(batch=x.shape[0])
        outs = []
        for sizes in ((s.granule,), RAGGED_CHUNKS):
            s.reset()
            outs.append(_stream_all(s, x, sizes))
    assert torch.isfinite(whole).all() and outs[0].shape == whole.shape
    diff = float((outs[0] - whole).abs().max())
    line = "causal stream %-15s max|stream - whole forward| %.3e, schedules equal: %s" % (signal, diff, torch.equal(outs[0], outs[1]))
    print(line)
    _LINES["stream"].append(line)
    assert torch.equal(outs[0], outs[1]), "the granule and the ragged schedule differ"
    want = references("causal")[signal]
    es.check_inference("causal", signal, outs[0].cpu().numpy(), want, _LINES["stream"])
    assert diff <= 2 * es.inference_bar(float(np.abs(want).max()), False), line           # both are within the bar of fp64


def _private(m, x, cuts):
    """x [A, T] through a batch-1 session of its own, cut as `cuts` -> [S*A, T]"""
    s = m.stream(batch=1)
    outs = [s.push(x[None, :, a:b]) for a, b in cuts]
    outs.append(s.finish())
    return torch.cat(outs, dim=-1)[0]


def test_causal_stream_pool_with_a_silent_and_a_fading_stream():
    """Three streams of one pool, pushed in chunks of their own: one is silent throughout, one falls silent half-way, one is loud.
    Each gets the bits of a private batch-1 session fed the same chunks (what tests/test_gpu_causal_stream_pool.py requires: nothing
    of a neighbour's level reaches it), and the fp64 restatement of its own signal within the bar."""
    m, sd = family_model("causal")
    names = ("silence", "half_silent", "loud")
    sig = es.signals(1, 1, 1001)
    xs = [torch.from_numpy(sig[n][0]).to(DEV) for n in names]
    with torch.no_grad():
        pool = m.stream_pool(3)
        g = pool.granule
        cuts = [schedule_chunks(1001, sizes) for sizes in ((g,), RAGGED_CHUNKS, (4 * g,))]
        want = [_private(m, x, c) for x, c in zip(xs, cuts)]
        sids = [pool.open() for _ in xs]
        outs = [[] for _ in xs]
        for tick in range(max(len(c) for c in cuts)):
            chunks = {sids[i]: xs[i][:, cuts[i][tick][0]:cuts[i][tick][1]] for i in range(3) if tick < len(cuts[i])}
            for sid, y in pool.push(chunks).items():
                outs[sids.index(sid)].append(y)
        for i, sid in enumerate(sids):
            outs[i].append(pool.close(sid))
        torch.cuda.synchronize()
    for i, name in enumerate(names):
        got = torch.cat(outs[i], dim=-1)
        assert got.shape == want[i].shape and torch.isfinite(got).all(), name
        assert torch.equal(got, want[i]), "stream %s differs from its private session" % name
        ref = es.restatement("causal", sd, sig[name]).numpy()
        wmax = float(np.abs(ref).max())
        err = float(np.abs(got.cpu().numpy()[None] - ref).max())
        line = "causal pool   %-15s err %.3e bar %.3e (max|want| %.3e)" % (name, err, es.inference_bar(wmax, False), wmax)
        print(line)
        _LINES["stream"].append(line)
        assert err <= es.inference_bar(wmax, False), line
