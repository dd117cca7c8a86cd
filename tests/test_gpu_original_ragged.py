"""The original SuDoRM-RF's opt-in ragged forward on the GPU: SuDORMRF.enable_ragged() -> forward_ragged / separate_ragged /
pipeline.separate_list, for the three cases of tests/original_ragged_fixtures.py.

References: the UNMODIFIED reference model's output for every row alone at its own length (tests/golden/orig_ragged_*.npz,
tools/make_golden_original_ragged.py) and, for the recipe, tests/original_ref.separate of the row alone in fp64.  Bar: the
project's 1e-4 max-abs (x max(1, std) of the row for the recipe, whose rescale multiplies the model's error by it).

Row isolation: the same call with NaN past every length, the workspace and the output pre-filled with 0xFF and every other row's
content replaced.  GlobLN statistics are accumulated with fp64 atomics into 64 buckets per example, in whatever order the blocks
finish: two runs of the SAME input may differ in the last bit of a sum, so the kept rows are held to 1e-6 of their first result
(the figure is printed; a cross-row leak is orders of magnitude larger) rather than to equal bits.
Measured on an MI355X: forward_ragged against the reference per row <= 1.5e-6 (all three cases); all lengths = T against the
uniform forward <= 5.2e-7; separate_ragged <= 2.7e-5 at a row of std 20.4 (bar 2.0e-3), <= 9.9e-6 elsewhere; the kept rows of the
isolation runs came back with equal bits in all six runs."""
import functools

import numpy as np
import pytest
import torch

from tests import original_fixtures as of
from tests import original_ragged_fixtures as rf
from tests import original_ref as orf
from tests.placement import poisoned_allocations

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4
ISOLATION_TOL = 1e-6
RAGGED_KERNELS = {"encoder_bias_relu_ragged", "gln_apply_c_ragged", "softmax_mask_ragged", "bias_rescale_ragged", "overlap_add_ragged",
                  "pyramid_moments_ragged", "pyramid_finalize_ragged", "pyramid_merge_ragged"}
UNIFORM_TWINS = {"gln_apply_c", "gln_apply_c_scalar", "encoder_bias_relu", "softmax_mask", "bias_rescale", "overlap_add", "encoder",
                 "pyramid_moments", "pyramid_finalize", "pyramid_merge"}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    from sudo_rm_rf_amd import _lib, ops
    _lib.load()
    ops.set_kernel_mode(0)
    ops.set_debug_flags(0)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(opted-in model on the GPU, state dict, fixture) of a case: made once, shared, never written to"""
    from sudo_rm_rf_amd.dnn.models.sudormrf import SuDORMRF
    cfg, _, _, wseed, _ = rf.CASES[name]
    sd = of.make_state_dict(cfg, wseed)
    m = SuDORMRF(**cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(DEV).eval().enable_ragged(), sd, rf.load(name)


def _zeros_past(out, lengths, what):
    for b, n in enumerate(lengths):
        assert bool((out[b, :, n:] == 0).all()), "%s: row %d is not exactly zero past its length %d" % (what, b, n)


@pytest.mark.parametrize("name", sorted(rf.CASES))
def test_forward_ragged_is_the_reference_row_by_row(name):
    from sudo_rm_rf_amd import engine as engine_mod, ops
    m, _, fx = _case(name)
    lens = fx["lengths"]
    wav = torch.from_numpy(fx["wav"]).to(DEV)
    with torch.no_grad(), poisoned_allocations(engine_mod), ops.kernel_trace(DEV) as tr:
        out = m.forward_ragged(wav, lens)
    torch.cuda.synchronize()
    assert out.shape == (len(lens), rf.CASES[name][0]["num_sources"], wav.shape[-1]) and torch.isfinite(out).all()
    got = out.cpu().numpy()
    err = [float(np.abs(got[b, :, :n] - fx["out"][b]).max()) for b, n in enumerate(lens)]
    print("%s forward_ragged vs the reference per row: %s" % (name, " ".join("%.2e" % e for e in err)))
    assert max(err) <= TOL
    _zeros_past(out, lens, name)
    # the launch trace: the ragged kernels, none of their uniform twins
    names = tr.names
    assert RAGGED_KERNELS <= names, sorted(RAGGED_KERNELS - names)
    assert not (UNIFORM_TWINS & names), sorted(UNIFORM_TWINS & names)
    assert {n for n in names if n.startswith("pw_conv_x3w")} <= {"pw_conv_x3w_ragged<0>", "pw_conv_x3w_ragged<1>"}
    assert m._engine().last_plan.original_ragged_supported and not m._engine().last_plan.ragged_supported


@pytest.mark.parametrize("keep", [0, 1], ids=["even-rows", "odd-rows"])
@pytest.mark.parametrize("name", sorted(rf.CASES))
def test_rows_are_isolated(name, keep):
    from sudo_rm_rf_amd import engine as engine_mod
    m, _, fx = _case(name)
    lens = fx["lengths"]
    x = torch.from_numpy(fx["wav"])
    with torch.no_grad():
        first = m.forward_ragged(x.to(DEV), lens).cpu()
    other = torch.from_numpy(of.make_mixture(len(lens), x.shape[-1], 9121 + keep)) * 3.0 + 0.25
    x2 = x.clone()
    for i, n in enumerate(lens):
        if i % 2 != keep:
            x2[i] = other[i]
        x2[i, :, n:] = float("nan")
    m._engine().last_plan.workspace.fill_(0xFF)
    with torch.no_grad(), poisoned_allocations(engine_mod):
        out = m.forward_ragged(x2.to(DEV), lens).cpu()
    kept = [i for i in range(len(lens)) if i % 2 == keep]
    assert torch.isfinite(out).all()
    diff = [float((out[i, :, :lens[i]] - first[i, :, :lens[i]]).abs().max()) for i in kept]
    same = [bool(torch.equal(out[i], first[i])) for i in kept]
    print("%s kept rows %s vs their first result: max diff %s, equal bits %s" % (name, kept, ["%.1e" % d for d in diff], same))
    assert max(diff) <= ISOLATION_TOL
    changed = [i for i in range(len(lens)) if i % 2 != keep]
    assert all(float((out[i, :, :lens[i]] - first[i, :, :lens[i]]).abs().max()) > 1e-3 for i in changed)      # (they did change)
    _zeros_past(out, lens, name)


@pytest.mark.parametrize("name", sorted(rf.CASES))
def test_all_lengths_equal_to_T_is_the_uniform_forward(name):
    m, _, fx = _case(name)
    wav = torch.from_numpy(fx["wav"]).to(DEV)
    T = wav.shape[-1]
    with torch.no_grad():
        a = m.forward_ragged(wav, [T] * wav.shape[0])
        b = m(wav)
    err = float((a - b).abs().max())
    print("%s forward_ragged(all lengths = T) vs the uniform forward: %.2e" % (name, err))
    assert torch.isfinite(a).all() and err <= TOL


@functools.lru_cache(maxsize=None)
def _raw_rows(name):
    """the fixture's rows at other levels and offsets: gains over geomspace(0.05, 20), offsets in +-0.5"""
    fx = rf.load(name)
    rng = np.random.default_rng(31)
    n = len(fx["lengths"])
    gain = np.geomspace(0.05, 20.0, n)[rng.permutation(n)].astype(np.float32)
    off = rng.uniform(-0.5, 0.5, n).astype(np.float32)
    return np.ascontiguousarray(fx["wav"] * gain[:, None, None] + off[:, None, None], dtype=np.float32)


@pytest.mark.parametrize("mc", [False, True], ids=["plain", "mixture_consistency"])
@pytest.mark.parametrize("name", sorted(rf.CASES))
def test_separate_ragged_is_the_recipe_row_by_row(name, mc):
    from sudo_rm_rf_amd import ops
    m, sd, fx = _case(name)
    cfg, lens = rf.CASES[name][0], fx["lengths"]
    raw = _raw_rows(name)
    x = torch.from_numpy(raw).clone()
    for b, n in enumerate(lens):
        x[b, :, n:] = float("nan")
    with torch.no_grad(), ops.kernel_trace(DEV) as tr:
        est, stats = m.separate_ragged(x.to(DEV), lens, mixture_consistency=mc)
    torch.cuda.synchronize()
    assert "wav_stats_ragged" in tr.names and "bias_rescale_ragged" in tr.names and torch.isfinite(est).all()
    est, stats = est.cpu().numpy(), stats.cpu().numpy()
    for b, n in enumerate(lens):
        row = raw[b:b + 1, :, :n]
        want = orf.separate(cfg, sd, row, mixture_consistency=mc).numpy()[0]
        mean, std = float(row.astype(np.float64).mean()), float(row.astype(np.float64).std(ddof=1))
        err = float(np.abs(est[b, :, :n] - want).max())
        print("%s row %d (std %.3f): separate_ragged err %.2e, bar %.2e" % (name, b, std, err, TOL * max(1.0, std)))
        assert err <= TOL * max(1.0, std)
        assert abs(stats[b, 0] - mean) <= 1e-6 * max(1.0, abs(mean)) and abs(stats[b, 1] - std) <= 1e-6 * max(1.0, abs(std))
    _zeros_past(torch.from_numpy(est), lens, name)


def test_separate_list_batches_what_the_gate_takes_and_keeps_the_order():
    """10 utterances at the lengths of rg_b plus two that are too short for the pyramid: one gather and one separate_ragged call
    for the ragged batch, the short ones through separate(), the results in the caller's order."""
    from sudo_rm_rf_amd import ops, pipeline
    m, sd, fx = _case("rg_b")
    cfg = rf.CASES["rg_b"][0]
    lens = [2560, 640, 2401, 1280, 2400, 1921, 1441, 1120, 2000, 1600, 2240, 1290]
    short = {640, 1120}
    rng = np.random.default_rng(5)
    mixes = [(of.make_mixture(1, n, 700 + i)[0, 0] * rng.uniform(0.3, 3.0) + rng.uniform(-0.3, 0.3)).astype(np.float32) for i, n in enumerate(lens)]
    assert [pipeline.ragged_route(m, n) for n in lens] == ["single" if n in short else "ragged" for n in lens]
    with ops.kernel_trace(DEV) as tr:
        got = pipeline.separate_list(m, [torch.from_numpy(x).to(DEV) for x in mixes])
    torch.cuda.synchronize()
    count = lambda k: sum(1 for name, _ in tr.launches if name == k)
    assert count("wav_gather_ragged") == 1 and count("wav_stats_ragged") == 1 and count("bias_rescale_ragged") == 1
    assert count("encoder_bias_relu_ragged") == 1 and count("encoder_bias_relu") == len(short) == count("bias_rescale")
    for i, (x, n) in enumerate(zip(mixes, lens)):
        want = orf.separate(cfg, sd, x[None, None, :]).numpy()[0]
        assert tuple(got[i].shape) == (cfg["num_sources"], n)
        err = float(np.abs(got[i].cpu().numpy() - want).max())
        assert err <= TOL * max(1.0, float(x.std(ddof=1))), (i, n, err)
    # a model that has not opted in: utterance by utterance, no ragged kernel
    m.enable_ragged(False)
    try:
        with ops.kernel_trace(DEV) as tr:
            again = pipeline.separate_list(m, [torch.from_numpy(x).to(DEV) for x in mixes[:3]])
        assert not any(n.endswith("_ragged") or "_ragged<" in n for n in tr.names), tr.names
        assert all(float((a - g).abs().max()) <= 2 * TOL * max(1.0, float(x.std(ddof=1))) for a, g, x in zip(again, got, mixes))
    finally:
        m.enable_ragged()


def test_ragged_forward_is_inference_only_and_refuses_an_off_grid_row():
    from sudo_rm_rf_amd._lib import SrfError
    m, _, fx = _case("rg_a")
    wav = torch.from_numpy(fx["wav"]).to(DEV)
    with pytest.raises(NotImplementedError):
        m.forward_ragged(wav, fx["lengths"])            # (grad mode on, parameters require grad)
    lens = list(fx["lengths"])
    lens[3] = rf.OFF_GRID[1]
    with torch.no_grad(), pytest.raises(SrfError, match=r"original.*example 3"):
        m.forward_ragged(wav, lens)
