"""The inference forward AT THE BENCH BATCH on examples that all differ -- in content, level and offset -- against references
that share no code with the library.

Every other bench-batch inference test fills the batch with copies of one or two golden waveforms (or scales every row by
the same factor), so every row, every GlobLN statistic and every {mean, std} of the separate() recipe is the same: a
batch-index slip in the whole-model wiring (a statistics slot of example b + 2 handed to a prologue, a sub-batch workspace
offset, the tile -> example map of the paired-block GEMM, a pyramid / TAC tile that straddles two examples, stats[b + 1] in
the rescale) reads equal values and passes.  Here row i is  raw[i] = g_i * m_i + o_i  with 32 different mixtures m_i, gains
g_i log-spaced over 0.05 .. 20 in shuffled order and offsets o_i in +-0.5; the model sees the per-example normalised rows
(so the OUTPUT scale is that of the goldens and the north-star bar applies unchanged), separate() sees the raw ones.

References (both treat examples independently -- tests/test_oracle_golden.py::test_torch_oracle_treats_examples_independently
-- so the reference of a subset of rows is computed from that subset alone):
  * Improved / GroupComm: oracle.torch_oracle.forward in fp32 on the CPU, the reference's own ATen op sequence, pinned to the
    stored reference outputs to 2e-6 by the CPU golden tests;
  * causal: tests/causal_stream_ref.StreamRef in fp32 (written from the arithmetic alone, pinned by
    tests/test_causal_stream_host.py), run as cat(push(x), finish()).
"""
import gc
import time

import numpy as np
import pytest
import torch

from conftest import load_case
from oracle import torch_oracle, weights
from test_gpu_causal import assert_bench_dispatch as assert_causal_bench_dispatch
from test_gpu_model import _BENCH_BATCH, DEV, TOL, assert_bench_dispatch, build
from tests import causal_fixtures as cf
from tests.causal_stream_ref import StreamRef

pytestmark = pytest.mark.gpu

T_SHORT = 10400      # the shortest length at which batch 32 (cfg 5: 16) still dispatches the bench kernel set, see test 1
CASE_IDS = [c for c, _, _ in _BENCH_BATCH]
BENCH_T = {"cfg2_improved_u16": 32000, "cfg3_groupcomm_u8": 32000, "cfg4_improved_u36_n2048": 32000,
           "cfg5_improved_u36_n4096": 128000}                       # the lengths bench.py times
INPUT_SEED = {"cfg2_improved_u16": 9020, "cfg3_groupcomm_u8": 9030, "cfg4_improved_u36_n2048": 9040,
              "cfg5_improved_u36_n4096": 9050, "causal": 9104}      # (no golden is made from any of them)
# rows on both sides of every cut the engine may make: 16|16, 20|12, 18|14 (batch 16: 8|8, 10|6, 9|7); not periodic
ROWS_32 = [0, 11, 15, 16, 19, 31]
ROWS_16 = [0, 8, 9, 15]
ROWS_CAUSAL = [0, 15, 16, 19, 31]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    from sudo_rm_rf_amd import ops
    ops.set_kernel_mode(0)


def _free_gpu():
    gc.collect()
    torch.cuda.empty_cache()


def distinct_batch(batch, T, seed, channels=1):
    """(raw, norm, mean, std, gain): raw[i] = gain[i] * mixture_i + offset_i, norm = the callers' per-example normalisation of
    raw (README recipe, as in test_separate_pipeline_matches_reference_recipe).  CPU float32 tensors [batch, channels, T]."""
    m = weights.make_mixture(batch, T, seed, channels=channels)
    rng = np.random.default_rng(seed)
    gain = np.geomspace(0.05, 20.0, batch)[rng.permutation(batch)]
    assert (np.diff(gain) > 0).any() and (np.diff(gain) < 0).any(), "the gains must not be monotone in the row index"
    offset = rng.uniform(-0.5, 0.5, batch)
    raw = torch.from_numpy((gain[:, None, None] * m + offset[:, None, None]).astype(np.float32))
    std, mean = raw.std(-1, keepdim=True), raw.mean(-1, keepdim=True)
    norm = (raw - mean) / (std + 1e-9)
    return raw, norm, mean, std, gain


def oracle_rows(cfg, sdt, x):
    """torch_oracle.forward of the rows of x (fp32, CPU), a few rows at a time where the masked tensor of all of them would
    take more than 1 GiB (the rows are independent)."""
    SA = cfg.num_sources * (cfg.in_audio_channels if cfg.variant == "groupcomm" else 1)
    frames = cfg.padded_length(x.shape[-1]) // (cfg.enc_kernel_size // 2)
    chunk = max(1, (1 << 28) // (SA * cfg.enc_num_basis * frames))
    t0 = time.time()
    with torch.no_grad():
        out = torch.cat([torch_oracle.forward(cfg, sdt, x[i:i + chunk].contiguous()) for i in range(0, x.shape[0], chunk)])
    return out, time.time() - t0


def per_example_error(got, want):
    """max |got - want| per example, as a float64 array."""
    got = got.detach().cpu() if isinstance(got, torch.Tensor) else got
    return (got - want).abs().flatten(1).max(1).values.double().numpy()


def report(what, err, bar, labels=None):
    """Print the worst example and its error, then assert every example against its bar (a scalar or one bar per example)."""
    bar = np.broadcast_to(np.asarray(bar, dtype=np.float64), err.shape)
    labels = list(range(len(err))) if labels is None else labels
    w = int(np.argmax(err / bar))
    print("%s: worst example %d: max abs err %.3e (bar %.1e); median over examples %.3e" %
          (what, labels[w], err[w], bar[w], float(np.median(err))))
    over = [(labels[i], float("%.3g" % err[i])) for i in range(len(err)) if not err[i] <= bar[i]]
    assert not over, "%s: examples over their bar (example, max abs err): %s" % (what, over)


# ---------------------------------------------------------------------------------------------------------------------------
# test 1: single stream, bench kernel set, every example against the oracle
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,batch,families", _BENCH_BATCH, ids=CASE_IDS)
def test_every_distinct_example_matches_the_oracle_on_the_bench_kernels(manifest, case, batch, families):
    """Batch 32 (cfg 5: 16) distinct examples at T = 10400, single stream: the forward must dispatch the SAME kernel families
    with the SAME launch counts that test_bench_batch_examples_match_reference_golden asserts at T = 32000, and every example
    must match the CPU fp32 oracle within the north-star 1e-4; for cfg 2 / cfg 3 also through engine.separate (statistics,
    normalise-on-load, rescale and -- GroupComm -- mixture consistency folded into the overlap-add, fused mask + decoder tail)
    against the README recipe written out with the oracle, within 1e-4 * max(1, g_i) (the rescale multiplies the model's
    error by std ~ g_i).

    Why 10400: the oracle costs CPU time per sample, so the length is the shortest that keeps the bench dispatch.  The padded
    length is 10400 (D = 5) / 10560 (D = 6), i.e. 1040 / 1056 frames = 9 tiles of 128: the pair gate is 32 * 9 = 288 >= 256 CUs,
    the 256 x 128 GEMM / fused-tail gates are Bt * 2 * 9 >= 256, and the register pyramid's L % 16 (D = 6: % 32) holds.
    If a dispatch change ever makes the trace at this length differ from the T = 32000 one, the length is wrong, not the
    assertion: take the next multiple of 320 at which they agree.

    Cost: nearly all of it is the CPU oracle (measured on 8 host threads: 6 s for cfg 3, about 10 s for the 16 rows of cfg 5);
    the GPU part is two forwards."""
    from sudo_rm_rf_amd import ops
    cfg, sd, _, _ = load_case(manifest, case)
    raw, norm, mean, std, gain = distinct_batch(batch, T_SHORT, INPUT_SEED[case])
    est, secs = oracle_rows(cfg, torch_oracle.to_torch(sd), norm)
    print("%s batch %d T %d: oracle (CPU fp32) %.1f s, output abs max %.3f" % (case, batch, T_SHORT, secs, float(est.abs().max())))
    model = build(cfg, sd)
    eng = model._engine()
    try:
        eng.multi_stream = False
        with torch.no_grad(), ops.kernel_trace(DEV) as tr:
            out = model(norm.to(DEV))
        count = assert_bench_dispatch(cfg, tr, families)
        print("%s: dispatched %s" % (case, sorted(count.items())))
        report("%s model(norm) vs oracle" % case, per_example_error(out, est), TOL)
        if case in ("cfg2_improved_u16", "cfg3_groupcomm_u8"):
            mc = cfg.variant == "groupcomm"
            want = est * std + mean
            if mc:
                want = want + (norm - want.sum(1, keepdim=True)) / want.shape[1]
            with torch.no_grad(), ops.kernel_trace(DEV) as tr:
                got = eng.separate(model, raw.to(DEV), mc)
            assert "pw_mask_decode" in tr.names, sorted(tr.names)
            report("%s separate(raw, mixture_consistency=%s) vs recipe" % (case, mc), per_example_error(got, want),
                   TOL * np.maximum(1.0, gain))
    finally:
        eng.multi_stream = True
        del model, eng
        _free_gpu()


# ---------------------------------------------------------------------------------------------------------------------------
# test 2: bench length, every split the engine may pick
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,batch", [(c, b) for c, b, _ in _BENCH_BATCH], ids=CASE_IDS)
def test_every_split_of_a_distinct_bench_batch_equals_the_single_stream_forward(manifest, monkeypatch, case, batch):
    """At the length bench.py times (T = 32000; cfg 5: 128000 -- only there do the sub-batches of 12 / 6 examples keep the bench
    kernel set) and with all examples distinct: every explicit split the engine may pick (halves, 5 : 3, 9 : 7) through
    _forward_split and the public path once the auto-tuner has run give every example within 2e-6 max-abs of the single-stream
    forward (the bar of test_split_forward_stress, whose docstring says why it is not bit equality); and the single-stream
    forward matches the CPU fp32 oracle within 1e-4 on a fixed, non-periodic subset of rows that lie on both sides of every
    cut (the oracle runs on those rows alone)."""
    from sudo_rm_rf_amd import engine as engine_mod
    cfg, sd, _, _ = load_case(manifest, case)
    T = BENCH_T[case]
    _, norm, _, _, _ = distinct_batch(batch, T, INPUT_SEED[case] + 1)
    rows = ROWS_32 if batch == 32 else ROWS_16
    model = build(cfg, sd)
    eng = model._engine()
    monkeypatch.setattr(engine_mod, "_SPLIT_MODE", "auto")
    try:
        x = norm.to(DEV)
        with torch.no_grad():
            eng.multi_stream = False
            ref = model(x).cpu()
            eng.multi_stream = True
            cands = eng._split_candidates(batch)
            assert cands[0] == (batch,) and len(cands) == 4, cands
            params = [p.detach() for p in model.state_dict(keep_vars=True).values()]
            for parts in cands[1:]:
                out = torch.full(ref.shape, float("nan"), device=x.device)
                with torch.cuda.device(x.device), eng._run_lock(x.device):
                    eng._forward_split(parts, x, out, eng._param_table(params, x.device))
                torch.cuda.synchronize()
                report("%s split %s vs single stream" % (case, parts), per_example_error(out, ref), 2e-6)
            for _ in range(engine_mod._TUNE_AFTER + 1):
                out = model(x)
            choice = eng._split_choice.get((x.device.index, batch, T))
            assert choice is not None, "the split auto-tune did not run"
            report("%s auto-tuned %s vs single stream" % (case, choice), per_example_error(out, ref), 2e-6)
        del out, x
        est, secs = oracle_rows(cfg, torch_oracle.to_torch(sd), norm[rows].contiguous())
        print("%s T %d: oracle (CPU fp32) of rows %s %.1f s" % (case, T, rows, secs))
        report("%s single stream vs oracle, rows %s" % (case, rows), per_example_error(ref[rows], est), TOL, labels=rows)
    finally:
        eng.multi_stream = True
        del model, eng
        _free_gpu()


# ---------------------------------------------------------------------------------------------------------------------------
# test 3: the causal model
# ---------------------------------------------------------------------------------------------------------------------------
def _causal_model():
    from test_gpu_causal import _model
    return _model("causal_default", torch.device(DEV))      # causal_fixtures.DEFAULTS, weight seed 104


def _stream_ref(x):
    sd = cf.make_state_dict(cf.DEFAULTS, cf.CASES["causal_default"][3])
    ref = StreamRef(cf.DEFAULTS, sd, x.shape[0], dtype=torch.float32)
    t0 = time.time()
    with torch.no_grad():
        y = torch.cat([ref.push(x), ref.finish()], dim=-1)
    return y, time.time() - t0


def test_causal_every_distinct_example_matches_the_stream_reference_on_the_bench_kernels():
    """The causal model (causal_fixtures.DEFAULTS, weight seed 104) at batch 32 distinct, T = 10400 (D = 4: already a multiple
    of 80; 1040 frames clear the same 32 * 2 * 9 >= 256 gate as cfg 2), single stream: the launch counts
    test_bench_shape_dispatch_and_parity asserts at T = 32000, and every example within 1e-4 of StreamRef (fp32, CPU)."""
    from sudo_rm_rf_amd import ops
    x = torch.from_numpy(weights.make_mixture(32, T_SHORT, INPUT_SEED["causal"]))
    want, secs = _stream_ref(x)
    print("causal batch 32 T %d: StreamRef (CPU fp32) %.1f s, output abs max %.3f" % (T_SHORT, secs, float(want.abs().max())))
    m = _causal_model()
    eng = m._engine()
    try:
        eng.multi_stream = False
        with torch.no_grad(), ops.kernel_trace(DEV) as tr:
            out = m(x.to(DEV))
        torch.cuda.synchronize()
        count = assert_causal_bench_dispatch(tr, m.num_blocks)
        print("causal: dispatched %s" % (sorted(count.items()),))
        assert out.shape == want.shape
        report("causal model(x) vs StreamRef", per_example_error(out, want), TOL)
    finally:
        eng.multi_stream = True
        del m, eng
        _free_gpu()


def test_causal_every_split_of_a_distinct_bench_batch_equals_the_single_stream_forward(monkeypatch):
    """The causal model at the bench shape (batch 32, T = 32000), all examples distinct: the splits "half", "5:3" and "auto"
    each within 1e-6 of the single-stream forward (the bar of test_batch_independence_and_two_stream_split), and rows
    [0, 15, 16, 19, 31] of the single-stream forward within 1e-4 of StreamRef run on those rows alone."""
    from sudo_rm_rf_amd import engine as engine_mod
    x = torch.from_numpy(weights.make_mixture(32, 32000, INPUT_SEED["causal"] + 1))
    m = _causal_model()
    eng = m._engine()
    try:
        xd = x.to(DEV)
        with torch.no_grad():
            eng.multi_stream = False
            ref = m(xd).cpu()
            eng.multi_stream = True
            for mode in ("half", "5:3", "auto"):
                monkeypatch.setattr(engine_mod, "_SPLIT_MODE", mode)
                eng._split_choice.clear()
                eng._seen.clear()
                for _ in range(engine_mod._TUNE_AFTER + 1):
                    out = m(xd)
                choice = eng._split_choice.get((xd.device.index, 32, 32000))
                assert choice is not None and (mode == "auto" or len(choice) == 2), (mode, choice)
                report("causal split %s %s vs single stream" % (mode, choice), per_example_error(out, ref), 1e-6)
        want, secs = _stream_ref(x[ROWS_CAUSAL].contiguous())
        print("causal T 32000: StreamRef (CPU fp32) of rows %s %.1f s" % (ROWS_CAUSAL, secs))
        report("causal single stream vs StreamRef, rows %s" % (ROWS_CAUSAL,), per_example_error(ref[ROWS_CAUSAL], want), TOL,
               labels=ROWS_CAUSAL)
    finally:
        eng.multi_stream = True
        del m, eng
        _free_gpu()
