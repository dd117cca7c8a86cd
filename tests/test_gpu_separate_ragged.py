"""separate_ragged on the GPU: the caller-side recipe of a ragged batch -- statistics over each row's own samples, normalise
on load, the ragged forward, rescale, mixture consistency -- in one call, and the two small kernels beside it.

Per kernel first (wav_stats_ragged, wav_gather_ragged, the ragged encoder with statistics) against fp64 restatements written
here; then the whole model (cfg 2 weights, batch 32, T = 10400: the shapes tests/test_gpu_ragged.py establishes as the
smallest that keep the ragged kernel set) on RAW rows of very different level and offset, every row against
oracle.torch_oracle.forward of that row ALONE, normalised over its own length, rescaled (and made mixture consistent) in
torch -- a swapped or missing statistic shows at once.  The oracle fixture costs CPU time once per module."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_case
from oracle import torch_oracle, weights
from test_gpu_ragged import (DEGENERATE_ROWS, ORDER_TOL, TOL, _check_rows, _check_sums_rows, build, degenerate_batch,
                             ragged_lengths, report)
from tests.placement import SENTINEL_WORD, poisoned_allocations
from tests.test_gpu_ops import DEV, dev32, rnd

pytestmark = pytest.mark.gpu

CASE, BATCH, T = "cfg2_improved_u16", 32, 10400
STATS_RTOL = 1e-6          # |got - fp64| <= 1e-6 * max(1, |value|): the bar test_gpu_placement.py holds wav_normalize's statistics to


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    from sudo_rm_rf_amd import _lib, ops
    _lib.load()
    ops.set_kernel_mode(0)


def stats64(x, lens):
    """fp64 {mean, unbiased std} of x[r, :lens[r]] -> [rows, 2]; a lone sample has std 0 (the kernel's max(len - 1, 1))"""
    x = x.reshape(x.shape[0], -1)
    out = torch.zeros(len(lens), 2, dtype=torch.float64)
    for r, n in enumerate(lens):
        v = x[r, :n].double()
        out[r, 0] = v.mean()
        out[r, 1] = ((v - v.mean()) ** 2).sum().div(max(n - 1, 1)).sqrt()
    return out


def check_stats(got, want, what):
    got = got.detach().cpu().double()
    assert got.shape == want.shape and torch.isfinite(got).all(), what
    err, bar = (got - want).abs(), STATS_RTOL * want.abs().clamp(min=1.0)
    print("%s: worst |stats - fp64| / bar = %.3f" % (what, float((err / bar).max())))
    assert (err <= bar).all(), "%s: %s over %s" % (what, err.max().item(), STATS_RTOL)


def nan_tails(x, lens):
    x = x.clone()
    for r, n in enumerate(lens):
        x[r].reshape(-1)[n:] = float("nan")
    return x


def at_offset(x, off):
    """x on the device at a base `off` floats past a 16-byte boundary"""
    flat = torch.empty(x.numel() + 8, dtype=torch.float32, device=DEV)
    assert flat.data_ptr() % 16 == 0
    view = flat[off:off + x.numel()].view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 16 == 4 * off and view.is_contiguous()
    return view


# ---- statistics ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "one-float-off"])
@pytest.mark.parametrize("rows,T_,lens", [(3, 77, [77, 1, 40]), (2, 32000, [32000, 12345])], ids=["T77", "T32000"])
def test_wav_stats_ragged(rows, T_, lens, off):
    from sudo_rm_rf_amd import ops, ragged
    x = rnd(rows, 1, T_, seed=95, scale=3.0, shift=0.7).float()
    want = stats64(x, lens)
    xd = at_offset(nan_tails(x, lens), off)
    with poisoned_allocations(ragged), ops.kernel_trace(DEV) as tr:
        got = ragged.wav_stats(xd, lens)
    assert [n for n, _ in tr.launches] == ["wav_stats_ragged"]
    check_stats(got, want, "wav_stats_ragged")
    for r, n in enumerate(lens):
        if n == 1:
            assert got[r, 1].item() == 0.0, "a lone sample has a standard deviation of exactly 0"
            assert got[r, 0].item() == x[r, 0, 0].item()
    # a row's two numbers are the same bits when every OTHER row changes
    other = rnd(rows, 1, T_, seed=96, scale=0.5, shift=-2.0).float()
    for keep in range(rows):
        x2 = other.clone()
        x2[keep] = x[keep]
        got2 = ragged.wav_stats(at_offset(nan_tails(x2, lens), off), lens)
        assert torch.equal(got2[keep], got[keep]), "row %d depends on the other rows" % keep
    # the 2-D form [rows, T] is the same call
    assert torch.equal(ragged.wav_stats(xd.view(rows, T_), lens), got)


# ---- gather -------------------------------------------------------------------------------------------------------------------
def test_wav_gather_ragged():
    """Sources are views at odd element offsets of one buffer of random BIT PATTERNS (NaNs with payloads, denormals, -0.0 among
    them); the destination comes pre-filled with 0xFF bytes: [0, len) must equal the source bit for bit, every other word must
    still hold the sentinel."""
    from sudo_rm_rf_amd import ops, ragged
    lens, Tg = [5, 77, 1], 80
    g = torch.Generator().manual_seed(7)
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (200,), generator=g, dtype=torch.int64).to(torch.int32)
    bits[bits == SENTINEL_WORD] = 0
    buf = bits.to(DEV).view(torch.float32)
    starts = [1, 11, 93]
    srcs = [buf[s:s + n] for s, n in zip(starts, lens)]
    assert all(s.data_ptr() % 8 == 4 for s in srcs)
    with poisoned_allocations(ragged), ops.kernel_trace(DEV) as tr:
        wav, got_lens = ragged.wav_gather(srcs, Tg)
    assert [n for n, _ in tr.launches] == ["wav_gather_ragged"]
    assert got_lens == lens and wav.shape == (3, 1, Tg) and wav.dtype == torch.float32
    words = wav.view(torch.int32).cpu()
    for b, (s, n) in enumerate(zip(starts, lens)):
        assert torch.equal(words[b, 0, :n], bits[s:s + n]), "row %d is not its source bit for bit" % b
        assert (words[b, 0, n:] == SENTINEL_WORD).all(), "row %d was written at or past its length %d" % (b, n)


# ---- encoder with normalise-on-load -----------------------------------------------------------------------------------------------
def test_encoder_ragged_with_statistics():
    """N = 64, batch 3, T = 2600, D = 4: the encoder of a RAW row given its statistics is the fp64 convolution of the row
    normalised over its own length and zero padded (bar 2e-5: test_encoder_ragged's); frames past frames[b] exactly 0."""
    from sudo_rm_rf_amd import ops, ragged
    N, Te, D, lens = 64, 2600, 4, [2600, 1281, 1]
    frames = [ragged.padded_frames(n, 21, D) for n in lens]
    L = frames[0]
    assert frames == [272, 144, 16]
    x, w = rnd(3, 1, Te, seed=11, scale=3.0, shift=0.7).float(), rnd(N, 1, 21, seed=12, scale=0.3)
    st = stats64(x, lens)
    want = []
    for b, n in enumerate(lens):
        xp = torch.zeros(1, 1, frames[b] * 10, dtype=torch.float64)
        xp[0, 0, :n] = (x[b, 0, :n].double() - st[b, 0]) / (st[b, 1] + 1e-9)
        want.append(F.conv1d(xp, w, None, stride=10, padding=10)[0])
    xd = nan_tails(x, lens).to(DEV)
    stats = ragged.wav_stats(xd, lens)
    sums = ops.new_sums(3, DEV)
    with poisoned_allocations(ragged), ops.kernel_trace(DEV) as tr:
        got = ragged.encoder(xd, dev32(w), L, lens, frames, sums, in_stats=stats)
    assert [n for n, _ in tr.launches] == ["encoder_ragged"]
    _check_rows(got, want, frames, 2e-5, "encoder_ragged with statistics")
    _check_sums_rows(sums, want, "encoder_ragged with statistics, sums")
    # without statistics the same entry point is the plain ragged encoder of the raw row
    plain = ragged.encoder(xd, dev32(w), L, lens, frames)
    assert not torch.equal(plain, got)


# ======================================================================================================================
# whole model
# ======================================================================================================================
def recipe_setup(manifest, case, seed):
    """(cfg, model, raw x [BATCH, 1, T], lens, {False: rows, True: rows with mixture consistency}, fp64 stats): the reference of
    every row is computed ONCE -- normalised over its own length, torch_oracle.forward at that length, rescaled."""
    cfg, sd, _, _ = load_case(manifest, case)
    lens = ragged_lengths(cfg)
    rng = np.random.default_rng(seed)
    gain = np.geomspace(0.05, 20.0, BATCH)[rng.permutation(BATCH)]
    offs = rng.uniform(-0.5, 0.5, BATCH)
    x = torch.from_numpy((weights.make_mixture(BATCH, T, seed) * gain[:, None, None] + offs[:, None, None]).astype(np.float32))
    st = stats64(x, lens)
    assert float(st[:, 1].max() / st[:, 1].min()) > 100, "the rows must differ in level"
    sdt = torch_oracle.to_torch(sd)
    want = {False: [], True: []}
    with torch.no_grad():
        for i, n in enumerate(lens):
            mean, std = st[i, 0], st[i, 1]
            norm = ((x[i:i + 1, :, :n].double() - mean) / (std + 1e-9)).float().contiguous()
            est = torch_oracle.forward(cfg, sdt, norm)[0].double() * std + mean
            want[False].append(est.float())
            want[True].append((est + (norm[0].double() - est.sum(0, keepdim=True)) / est.shape[0]).float())
    model = build(cfg, sd)
    model._engine().multi_stream = False
    return cfg, model, x, lens, want, st


@pytest.fixture(scope="module")
def setup(manifest):
    return recipe_setup(manifest, CASE, 9140)


def row_errors(out, rows, lens):
    out = out.detach().cpu()
    return np.array([float((out[i, :, :lens[i]] - rows[i]).abs().max()) for i in range(len(lens))])


def row_bars(tol, st):
    return tol * np.maximum(1.0, st[:, 1].numpy())


def check_against_the_oracle(model, x, lens, want, st, mc, **kw):
    """separate_ragged(..., **kw) against the rows of `want[mc]`: TOL * max(1, std_i) per row, exact zeros past every length,
    the statistics at their own bar"""
    with torch.no_grad():
        out, stats = model.separate_ragged(nan_tails(x, lens).to(DEV), lens, **kw)
    assert out.shape == (BATCH, want[mc][0].shape[0], T) and torch.isfinite(out).all()
    check_stats(stats, st, "separate_ragged stats")
    report("separate_ragged(mixture_consistency=%s) vs the oracle recipe at each row's own length" % mc,
           row_errors(out, want[mc], lens), row_bars(TOL, st))
    for i, n in enumerate(lens):
        assert (out[i, :, n:] == 0).all(), "row %d is not exactly zero past its length %d" % (i, n)
    return out


@pytest.mark.parametrize("mc", [False, True], ids=["plain", "mixture-consistency"])
def test_separate_ragged_matches_the_oracle_recipe_row_by_row(setup, mc):
    cfg, model, x, lens, want, st = setup
    assert model._engine().ragged_plan_supported(BATCH, T, torch.device(DEV))
    if not mc:          # the Improved model's default is no mixture consistency
        check_against_the_oracle(model, x, lens, want, st, False)
    check_against_the_oracle(model, x, lens, want, st, mc, mixture_consistency=mc)


def check_degenerate_rows_recipe(manifest, case, setup, mc):
    """separate_ragged and separate_list on a batch that contains a silent, a DC and a near-silent utterance (the rows of
    test_gpu_ragged.DEGENERATE_ROWS) among the raw ordinary ones: each of the three against the fp64 recipe of that row alone at
    its own length -- mean / unbiased std over its own samples, (x - mean) / (std + 1e-9), the oracle forward, rescale, mixture
    consistency on request -- within 1e-4 max(1, std_i); the other rows against the references they had; finite everywhere
    (std = 0 meets the 1e-9 in the silent and the DC row); exactly zero past every end."""
    from sudo_rm_rf_amd import pipeline
    cfg, model, x, lens, want, st = setup
    _, sd, _, _ = load_case(manifest, case)
    sd64 = {k: v.double() for k, v in torch_oracle.to_torch(sd).items()}
    x2 = degenerate_batch(x, lens)
    with torch.no_grad():
        out, _ = model.separate_ragged(nan_tails(x2, lens).to(DEV), lens, mixture_consistency=mc)
        listed = pipeline.separate_list(model, [x2[i, 0, :n].to(DEV) for i, n in enumerate(lens)], mixture_consistency=mc)
    out = out.cpu()
    assert torch.isfinite(out).all() and all(torch.isfinite(y).all() for y in listed)
    for r, name in DEGENERATE_ROWS.items():
        n = lens[r]
        row = x2[r:r + 1, :, :n].double()
        mean, std = row.mean(), row.std()
        norm = (row - mean) / (std + 1e-9)
        with torch.no_grad():
            ref = torch_oracle.forward(cfg, sd64, norm)[0] * std + mean
        if mc:
            ref = ref + (norm[0] - ref.sum(0, keepdim=True)) / ref.shape[0]
        bar = TOL * max(1.0, float(std))
        err = float((out[r, :, :n].double() - ref).abs().max())
        err_l = float((listed[r].cpu().double() - ref).abs().max())
        print("separate_ragged(mc=%s) row %d (%s, %d samples): err %.3e, separate_list %.3e, bar %.3e (max|want| %.3e)"
              % (mc, r, name, n, err, err_l, bar, float(ref.abs().max())))
        assert err <= bar and err_l <= bar, (name, err, err_l, bar)
    others = [i for i in range(BATCH) if i not in DEGENERATE_ROWS]
    report("separate_ragged(mc=%s), the ordinary rows beside the degenerate ones" % mc,
           row_errors(out, want[mc], lens)[others], row_bars(TOL, st)[others], labels=others)
    for i, n in enumerate(lens):
        assert (out[i, :, n:] == 0).all(), "row %d is not exactly zero past its length %d" % (i, n)


@pytest.mark.parametrize("mc", [False, True], ids=["plain", "mixture-consistency"])
def test_separate_ragged_with_silent_dc_and_near_silent_rows(manifest, setup, mc):
    check_degenerate_rows_recipe(manifest, CASE, setup, mc)


def test_separate_ragged_launch_set(setup):
    """what test_ragged_forward_matches_the_oracle_row_by_row pins for forward_ragged, plus exactly one wav_stats_ragged"""
    from sudo_rm_rf_amd import ops
    cfg, model, x, lens, _, _ = setup
    with torch.no_grad(), ops.kernel_trace(DEV) as tr:
        model.separate_ragged(x.to(DEV), lens, mixture_consistency=True)
    U = cfg.num_blocks
    count = {n: sum(1 for k, _ in tr.launches if k == n) for n in tr.names}
    print("separate_ragged dispatched", sorted(count.items()))
    assert count == {"wav_stats_ragged": 1, "zero_fill": 1, "pack_pw_weights": 1, "encoder_ragged": 1, "pw_pair_x3f_ragged<1>": 1,
                     "pw_pair_x3f_ragged<2>": U - 1, "pyramid_moments_ragged": U, "pyramid_finalize_ragged": U,
                     "pyramid_merge_ragged": U, "pw_conv_x3w_ragged<2>": 1, "pack_decoder": 1, "pw_mask_decode": 1,
                     "overlap_add_ragged": 1}


def check_isolation(model, x, lens, st, keep, seed, **kw):
    """Same call again with everything a row must not depend on changed: the input past every length NaN, the workspace and the
    output buffers filled with 0xFF bytes beforehand, the CONTENT of every other row replaced.  Kept rows: finite, within
    ORDER_TOL * max(1, std_i) of their first result, their statistics the same bits; every row exactly zero past its length."""
    from sudo_rm_rf_amd import engine as engine_mod
    with torch.no_grad():
        first, stats1 = model.separate_ragged(x.to(DEV), lens, **kw)
    first, stats1 = first.cpu(), stats1.cpu()
    other = torch.from_numpy(weights.make_mixture(BATCH, T, seed + keep).astype(np.float32)) * 3.0 + 0.25
    x2 = x.clone()
    for i in range(BATCH):
        if i % 2 != keep:
            x2[i] = other[i]
    x2 = nan_tails(x2, lens)
    model._engine().last_plan.workspace.fill_(0xFF)
    with torch.no_grad(), poisoned_allocations(engine_mod):
        out, stats2 = model.separate_ragged(x2.to(DEV), lens, **kw)
    out, stats2 = out.cpu(), stats2.cpu()
    kept = [i for i in range(BATCH) if i % 2 == keep]
    for i in kept:
        assert torch.isfinite(out[i]).all(), "row %d is not finite" % i
        assert torch.equal(stats2[i], stats1[i]), "the statistics of row %d depend on something outside the row" % i
    err = np.array([float((out[i, :, :lens[i]] - first[i, :, :lens[i]]).abs().max()) for i in kept])
    report("kept rows vs their first result", err, row_bars(ORDER_TOL, st)[kept], labels=kept)
    for i, n in enumerate(lens):
        assert (out[i, :, n:] == 0).all(), "row %d is not exactly zero past its length %d" % (i, n)


@pytest.mark.parametrize("keep", [0, 1], ids=["even-rows", "odd-rows"])
def test_separate_ragged_rows_are_isolated(setup, keep):
    cfg, model, x, lens, _, st = setup
    check_isolation(model, x, lens, st, keep, 9141, mixture_consistency=True)


@pytest.mark.parametrize("mc", [False, True], ids=["plain", "mixture-consistency"])
def test_separate_ragged_with_equal_lengths_is_separate(setup, mc):
    from sudo_rm_rf_amd import pipeline
    cfg, model, x, _, _, _ = setup
    rows = x.to(DEV)
    with torch.no_grad():
        a, stats = model.separate_ragged(rows, [T] * BATCH, mixture_consistency=mc)
        b = pipeline.separate(model, rows, mixture_consistency=mc)
    full = stats64(x, [T] * BATCH)
    check_stats(stats, full, "separate_ragged stats, all lengths = T")
    err = (a - b).abs().flatten(1).max(1).values.double().cpu().numpy()
    report("separate_ragged(all lengths = T) vs pipeline.separate", err, row_bars(ORDER_TOL, full))


def test_separate_ragged_is_inference_only(setup):
    cfg, model, x, lens, _, _ = setup
    with pytest.raises(NotImplementedError):
        model.separate_ragged(x.to(DEV), lens)            # (grad mode on, parameters require grad)


def check_separate_list(model, cfg, seed, data_seed):
    """40 utterances of mixed length, level and offset in batches of 20: ONE gather launch and ONE separate_ragged call per
    ragged batch, the results views [num_sources, T_i] of that call's output, each within TOL * max(1, std_i) of
    pipeline.separate of that utterance alone."""
    from sudo_rm_rf_amd import ops, pipeline
    rng = np.random.default_rng(seed)
    n = 40
    lens = [int(v) for v in rng.integers(3000, T + 1, n)]
    gain = np.geomspace(0.05, 20.0, n)[rng.permutation(n)]
    mixes = [torch.from_numpy((gain[i] * weights.make_mixture(1, lens[i], data_seed + i)[0, 0] + rng.uniform(-0.5, 0.5)).astype(np.float32)).to(DEV)
             for i in range(n)]
    calls, inner = [], model.separate_ragged

    def counted(wav, lengths, mixture_consistency):
        calls.append(len(lengths))
        return inner(wav, lengths, mixture_consistency)

    model.__dict__["separate_ragged"] = counted          # (an instance attribute in front of the method, for this call only)
    try:
        with ops.kernel_trace(DEV) as tr:
            got = pipeline.separate_list(model, [m if i % 2 else m.unsqueeze(0) for i, m in enumerate(mixes)], max_batch=20)
    finally:
        del model.__dict__["separate_ragged"]
    assert calls == [20, 20], "one separate_ragged call per ragged batch"
    count = {k: sum(1 for name, _ in tr.launches if name == k) for k in ("wav_gather_ragged", "wav_stats_ragged", "overlap_add_ragged")}
    assert count == {"wav_gather_ragged": 2, "wav_stats_ragged": 2, "overlap_add_ragged": 2}, count
    err, bar = [], []
    for i, m in enumerate(mixes):
        want = pipeline.separate(model, m.unsqueeze(0))[0]
        assert got[i].shape == want.shape == (cfg.num_sources, lens[i])
        assert got[i]._base is not None and got[i]._base.shape[-1] % pipeline.BUCKET == 0, "utterance %d is not a view of its batch" % i
        err.append(float((got[i] - want).abs().max()))
        bar.append(TOL * max(1.0, float(m.std())))
    report("separate_list vs separate per utterance", np.array(err), np.array(bar))


def test_separate_list_is_one_gather_and_one_call_per_batch(setup):
    cfg, model, _, _, _, _ = setup
    check_separate_list(model, cfg, 79, 9700)
