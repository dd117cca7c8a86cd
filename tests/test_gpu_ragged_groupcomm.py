"""Ragged batch for the GroupComm model on the GPU.

First half, one test per ragged form that is GroupComm's own (TAC, the two thin-conv forms, the pyramid over folded rows):
the scheme of tests/test_gpu_ragged.py -- an fp64 reference per example on the example's own columns, outputs and scratch
pre-filled with 0xFF bytes (tests/placement.py) so that "exactly zero past the end" proves the kernel wrote it, then the same
call with NaN past every end must give the same bits; and with all lengths equal to the row stride every form is bit for
bit its uniform twin.  Bars: those tests/test_gpu_ops.py holds the uniform twins to (test_tac 2e-5, test_pw_conv 5e-5,
test_fused_pyramid 5e-5).

Second half, the whole model: cfg 3 weights (golden cfg3_groupcomm_u8), batch 32, T = 10400, rows of unequal length in ONE
call (GroupCommSudoRmRf.forward_ragged), every row against oracle.torch_oracle.forward of that row ALONE at its own length,
and pipeline.separate_list against pipeline.separate per utterance."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_case
from oracle import torch_oracle, weights
from oracle.schema import ModelConfig
from test_gpu_batch_distinct import per_example_error, report
from test_gpu_model import TOL, build
from test_gpu_ragged import (ORDER_TOL, check_degenerate_rows_forward, PW_FRAMES, PW_L, PYR_CASES, _check_rows, _check_sums_rows, _nan_tail, _pyramid_ref,
                             _sums64_valid, ragged_lengths)
from tests.placement import poisoned_allocations
from tests.test_gpu_ops import DEV, check, check_sums, dev32, gln64, rnd, sums64

pytestmark = pytest.mark.gpu

G, NB, NC = 16, 16, 32          # groups, channels per group outside / inside the U-block (cfg 3: 256 / 512 channels)


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    from sudo_rm_rf_amd import _lib, ops
    _lib.load()
    ops.set_kernel_mode(0)


def _fold_frames(frames, rows_per_example):
    """one entry per folded row"""
    return [n for n in frames for _ in range(rows_per_example)]


# ---- TAC ------------------------------------------------------------------------------------------------------------------
def _tac_params(n):
    H = 3 * n
    return [rnd(H, n, seed=81, scale=n ** -0.5), rnd(H, seed=82, scale=0.2), torch.tensor([0.2], dtype=torch.float64),
            rnd(H, H, seed=83, scale=H ** -0.5), rnd(H, seed=84, scale=0.2), torch.tensor([0.3], dtype=torch.float64),
            rnd(n, 2 * H, seed=85, scale=(2 * H) ** -0.5), rnd(n, seed=86, scale=0.2), torch.tensor([0.15], dtype=torch.float64)]


def _tac_ref(x, P, n):
    """groupcomm_sudormrf_v2.py:356-377 in fp64 on ONE example x [G, n, cols] -> [G, n, cols] (pre-norm)"""
    H, cols = 3 * n, x.shape[-1]
    pr = lambda t, a: torch.where(t >= 0, t, a * t)
    rows = x.permute(2, 0, 1).reshape(-1, n)
    z = pr(rows @ P[0].T + P[1], P[2]).view(cols, G, H)
    q = pr(z.mean(1) @ P[3].T + P[4], P[5])
    cat = torch.cat([z, q.unsqueeze(1).expand(cols, G, H)], 2).reshape(-1, 2 * H)
    return pr(cat @ P[6].T + P[7], P[8]).view(cols, G, n).permute(1, 2, 0).contiguous()


def test_tac_ragged():
    from sudo_rm_rf_amd import ops, ragged
    frames, L, Bt = PW_FRAMES, PW_L, len(PW_FRAMES)
    x = rnd(Bt, G * NB, L, seed=80)
    P = _tac_params(NB)
    want = [_tac_ref(x[b].view(G, NB, L)[..., :n], P, NB).reshape(G * NB, n) for b, n in enumerate(frames)]
    Pd = [dev32(p) for p in P]

    def run(xx):
        sums = ops.new_sums(Bt * G, DEV)
        with poisoned_allocations(ragged), ops.kernel_trace(DEV) as tr:
            q = ragged.tac(dev32(xx), Pd, G, frames, out_sums=sums)
        assert [n for n, _ in tr.launches] == ["tac_mfma_ragged"]
        return q, sums

    q, sums = run(x)
    _check_rows(q, want, frames, 2e-5, "tac_ragged")
    stored = q.double().cpu().view(Bt * G, NB, L)
    rows = [stored[r, :, :n] for r, n in enumerate(_fold_frames(frames, G))]
    _check_sums_rows(sums, rows, "tac_ragged sums")
    q2, sums2 = run(_nan_tail(x, frames))
    assert torch.equal(q2, q), "tac_ragged: the result depends on x past an example's end"
    _check_sums_rows(sums2, rows, "tac_ragged sums (NaN tail)")


def test_tac_ragged_equal_lengths_is_the_uniform_tac():
    from sudo_rm_rf_amd import ops, ragged
    Bt, L = 3, PW_L
    x, Pd = dev32(rnd(Bt, G * NB, L, seed=80)), [dev32(p) for p in _tac_params(NB)]
    sa, sb = ops.new_sums(Bt * G, DEV), ops.new_sums(Bt * G, DEV)
    with ops.kernel_trace(DEV) as tr:
        b = ops.tac(x.view(Bt, G, NB, L), Pd, out_sums=sb)
    assert tr.names == {"tac_mfma"}, tr.names
    a = ragged.tac(x, Pd, G, [L] * Bt, out_sums=sa)
    assert torch.equal(a, b.view(Bt, G * NB, L))
    assert torch.allclose(sa.sum(1), sb.sum(1), rtol=1e-12, atol=0)          # (same partials; the fp64 atomic order may differ)


# ---- thin convolutions: 5 examples x 16 folded rows, row stride 400 ------------------------------------------------------------
def test_pw_conv_small_ragged_preadd():
    """proj_1x1 with u = x + GlobLN(q) folded into its load: 16 -> 32 channels"""
    from sudo_rm_rf_amd import ops, ragged
    frames, L, Bt = PW_FRAMES, PW_L, len(PW_FRAMES)
    rows, fr = Bt * G, _fold_frames(PW_FRAMES, G)
    x, q = rnd(rows, NB, L, seed=60, scale=1.3, shift=0.2), rnd(rows, NB, L, seed=61, scale=0.7, shift=-0.1)
    w, bias = rnd(NC, NB, 1, seed=62, scale=NB ** -0.5), rnd(NC, seed=63, scale=0.2)
    gam, bet = rnd(NB, seed=64, scale=0.2, shift=1.0), rnd(NB, seed=65, scale=0.2)
    want_u = [x[r:r + 1, :, :n] + gln64(q[r:r + 1, :, :n], gam, bet) for r, n in enumerate(fr)]
    want_y = [F.conv1d(u, w, bias)[0] for u in want_u]
    qsums = _sums64_valid(q, fr).to(DEV)

    def run(xx, qq):
        sums = ops.new_sums(rows, DEV)
        with poisoned_allocations(ragged), ops.kernel_trace(DEV) as tr:
            y, u = ragged.pw_conv_small(dev32(xx), dev32(w), dev32(bias), frames, G, out_sums=sums, pre_q=dev32(qq),
                                        pre_sums=qsums, pre_gamma=dev32(gam), pre_beta=dev32(bet))
        assert [n for n, _ in tr.launches] == ["pw_conv_small_ragged"]
        return y, u, sums

    y, u, sums = run(x, q)
    _check_rows(y, want_y, fr, 5e-5, "pw_conv_small_ragged (pre-add) y")
    for r, n in enumerate(fr):
        check(u[r, :, :n], want_u[r][0], 3e-5, "pw_conv_small_ragged (pre-add) u, row %d" % r)
    stored = [y[r, :, :n].double().cpu() for r, n in enumerate(fr)]
    _check_sums_rows(sums, stored, "pw_conv_small_ragged (pre-add) sums")
    y2, u2, sums2 = run(_nan_tail(x, fr), _nan_tail(q, fr))
    assert torch.equal(y2, y), "y depends on x / q past an example's end"
    for r, n in enumerate(fr):
        assert torch.equal(u2[r, :, :n], u[r, :, :n]), "u of row %d depends on x / q past its end" % r
    _check_sums_rows(sums2, stored, "pw_conv_small_ragged (pre-add) sums (NaN tail)")


def test_pw_conv_small_ragged_residual():
    """res_conv: GlobLN + PReLU on load, + residual: 32 -> 16 channels; the output is block stream -- valid columns only"""
    from sudo_rm_rf_amd import ops, ragged
    frames, L, Bt = PW_FRAMES, PW_L, len(PW_FRAMES)
    rows, fr = Bt * G, _fold_frames(PW_FRAMES, G)
    x, res = rnd(rows, NC, L, seed=70, scale=1.5, shift=0.3), rnd(rows, NB, L, seed=71)
    w, bias = rnd(NB, NC, 1, seed=72, scale=NC ** -0.5), rnd(NB, seed=73, scale=0.2)
    gam, bet = rnd(NC, seed=74, scale=0.3, shift=1.0), rnd(NC, seed=75, scale=0.3)
    slope = torch.tensor([0.17], dtype=torch.float64)
    want = []
    for r, n in enumerate(fr):
        v = gln64(x[r:r + 1, :, :n], gam, bet)
        want.append(F.conv1d(torch.where(v >= 0, v, slope * v), w, bias)[0] + res[r, :, :n])
    in_sums = _sums64_valid(x, fr).to(DEV)

    def run(xx):
        with poisoned_allocations(ragged), ops.kernel_trace(DEV) as tr:
            y = ragged.pw_conv_small(dev32(xx), dev32(w), dev32(bias), frames, G, in_sums=in_sums, in_gamma=dev32(gam),
                                     in_beta=dev32(bet), in_prelu=dev32(slope), residual=dev32(res))
        assert [n for n, _ in tr.launches] == ["pw_conv_small_ragged"]
        return y

    y = run(x)
    for r, n in enumerate(fr):
        check(y[r, :, :n], want[r], 5e-5, "pw_conv_small_ragged (residual), row %d" % r)
    y2 = run(_nan_tail(x, fr))
    for r, n in enumerate(fr):
        assert torch.equal(y2[r, :, :n], y[r, :, :n]), "row %d depends on x past its end" % r


def test_pw_conv_small_ragged_equal_lengths_is_the_uniform_kernel():
    from sudo_rm_rf_amd import ops, ragged
    Bt, L = 3, PW_L
    rows = Bt * G
    # pre-add form: the uniform forward's unfused pair of launches computes the same bits (srf_pwconv_small.hip)
    x, q = dev32(rnd(rows, NB, L, seed=60, scale=1.3, shift=0.2)), dev32(rnd(rows, NB, L, seed=61, scale=0.7, shift=-0.1))
    w, bias = dev32(rnd(NC, NB, 1, seed=62, scale=NB ** -0.5)), dev32(rnd(NC, seed=63, scale=0.2))
    gam, bet = dev32(rnd(NB, seed=64, scale=0.2, shift=1.0)), dev32(rnd(NB, seed=65, scale=0.2))
    qsums = sums64(q.double().cpu()).to(DEV)
    sa, sb = ops.new_sums(rows, DEV), ops.new_sums(rows, DEV)
    y, u = ragged.pw_conv_small(x, w, bias, [L] * Bt, G, out_sums=sa, pre_q=q, pre_sums=qsums, pre_gamma=gam, pre_beta=bet)
    u_t = ops.gln_apply(q, qsums, gam, bet, residual=x)
    with ops.kernel_trace(DEV) as tr:
        y_t = ops.pw_conv(u_t, w, bias, out_sums=sb)
    assert tr.names == {"pw_conv_small"}, tr.names
    assert torch.equal(u, u_t) and torch.equal(y, y_t) and torch.allclose(sa.sum(1), sb.sum(1), rtol=1e-12, atol=0)
    # residual form
    x, res = dev32(rnd(rows, NC, L, seed=70, scale=1.5, shift=0.3)), dev32(rnd(rows, NB, L, seed=71))
    w, bias = dev32(rnd(NB, NC, 1, seed=72, scale=NC ** -0.5)), dev32(rnd(NB, seed=73, scale=0.2))
    kw = dict(in_sums=sums64(x.double().cpu()).to(DEV), in_gamma=dev32(rnd(NC, seed=74, scale=0.3, shift=1.0)),
              in_beta=dev32(rnd(NC, seed=75, scale=0.3)), in_prelu=dev32(torch.tensor([0.17])), residual=res)
    assert torch.equal(ragged.pw_conv_small(x, w, bias, [L] * Bt, G, **kw), ops.pw_conv(x, w, bias, **kw))


# ---- pyramid over folded rows: 3 rows per example (not a power of two: a shift in place of the division would show) --------
def test_pyramid_ragged_three_rows_per_example():
    from sudo_rm_rf_amd import ops, ragged
    C_, D, L, frames = PYR_CASES[0]
    assert D == 4
    RPE = 3
    fr = _fold_frames(frames, RPE)
    groups = len(fr)
    y1 = rnd(groups, C_, L, seed=200, scale=1.4, shift=0.2)           # every row its own data
    g_in, b_in = rnd(C_, seed=101, scale=0.3, shift=1.0), rnd(C_, seed=102, scale=0.3)
    slope = torch.tensor([0.23], dtype=torch.float64)
    W = [rnd(C_, 1, 5, seed=110 + k, scale=0.5) for k in range(D)]
    Bi = [rnd(C_, seed=120 + k, scale=0.2) for k in range(D)]
    Ga = [rnd(C_, seed=130 + k, scale=0.3, shift=1.0) for k in range(D)]
    Be = [rnd(C_, seed=140 + k, scale=0.3) for k in range(D)]
    want = [_pyramid_ref(y1[g:g + 1, :, :n], g_in, b_in, slope, W, Bi, Ga, Be) for g, n in enumerate(fr)]
    in_sums = _sums64_valid(y1, fr).to(DEV)
    dl = lambda ts: [dev32(t) for t in ts]

    def run(y):
        osums = ops.new_sums(groups, DEV)
        with poisoned_allocations(ragged), ops.kernel_trace(DEV) as tr:
            got = ragged.pyramid(dev32(y), in_sums, dev32(g_in), dev32(b_in), dev32(slope), dl(W), dl(Bi), dl(Ga), dl(Be),
                                 frames, out_sums=osums, rows_per_example=RPE)
        assert [n for n, _ in tr.launches] == ["pyramid_moments_ragged", "pyramid_finalize_ragged", "pyramid_merge_ragged"]
        return got, osums

    got, osums = run(y1)
    _check_rows(got, want, fr, 5e-5, "pyramid_ragged (3 rows per example)")
    _check_sums_rows(osums, want, "pyramid_ragged (3 rows per example) sums")
    got2, osums2 = run(_nan_tail(y1, fr))
    assert torch.equal(got2, got), "pyramid_ragged: the result depends on y1 past an example's end"
    _check_sums_rows(osums2, want, "pyramid_ragged (3 rows per example) sums (NaN tail)")
    # all lengths equal to the row stride: the uniform pyramid over the same 6 groups
    a = ragged.pyramid(dev32(y1[:6]), sums64(y1[:6]).to(DEV), dev32(g_in), dev32(b_in), dev32(slope), dl(W), dl(Bi), dl(Ga), dl(Be),
                       [L, L], rows_per_example=RPE)
    b = ops.pyramid(dev32(y1[:6]), sums64(y1[:6]).to(DEV), dev32(g_in), dev32(b_in), dev32(slope), dl(W), dl(Bi), dl(Ga), dl(Be))
    assert torch.equal(a, b)


# ======================================================================================================================
# whole model
# ======================================================================================================================
CASE, BATCH, T = "cfg3_groupcomm_u8", 32, 10400      # the length at which test_gpu_batch_distinct asserts cfg 3's bench dispatch


@pytest.fixture(scope="module")
def setup(manifest):
    cfg, sd, _, _ = load_case(manifest, CASE)
    assert (cfg.upsampling_depth, cfg.enc_kernel_size) == (5, 21)
    lens = ragged_lengths(cfg)
    assert min(lens) == 961 and {10240, 10241, 1280, 1281} <= set(lens)
    x = torch.from_numpy(weights.make_mixture(BATCH, T, 9130).astype(np.float32))
    x = (x - x.mean(-1, keepdim=True)) / (x.std(-1, keepdim=True) + 1e-9)
    sdt = torch_oracle.to_torch(sd)
    with torch.no_grad():            # the reference, ONCE, row by row at the row's own length
        want = [torch_oracle.forward(cfg, sdt, x[i:i + 1, :, :n].contiguous())[0] for i, n in enumerate(lens)]
    model = build(cfg, sd)
    model._engine().multi_stream = False
    return cfg, model, x, lens, want


def _row_errors(out, rows, lens):
    out = out.detach().cpu()
    return np.array([float((out[i, :, :lens[i]] - rows[i]).abs().max()) for i in range(len(lens))])


def test_ragged_forward_with_silent_dc_and_near_silent_rows(manifest, setup):
    """(the helper and its bars: tests/test_gpu_ragged.py)"""
    check_degenerate_rows_forward(manifest, CASE, setup)


def test_ragged_forward_matches_the_oracle_row_by_row(setup):
    from sudo_rm_rf_amd import ops
    cfg, model, x, lens, want = setup
    eng = model._engine()
    assert eng.ragged_plan_supported(BATCH, T, torch.device(DEV)), "zero examples may take the fallback"
    with torch.no_grad(), ops.kernel_trace(DEV) as tr:
        out = model.forward_ragged(x.to(DEV), lens)
    U = cfg.num_blocks
    count = {n: sum(1 for k, _ in tr.launches if k == n) for n in tr.names}
    print("ragged forward dispatched", sorted(count.items()))
    assert count == {"zero_fill": 1, "pack_pw_weights": 1, "encoder_ragged": 1, "pw_conv_x3w_ragged<1>": 1, "tac_mfma_ragged": U,
                     "pw_conv_small_ragged": 2 * U, "pyramid_moments_ragged": U, "pyramid_finalize_ragged": U,
                     "pyramid_merge_ragged": U, "pack_decoder": 1, "pw_mask_decode": 1, "overlap_add_ragged": 1}
    assert out.shape == (BATCH, cfg.num_sources, T) and torch.isfinite(out).all()
    report("forward_ragged vs oracle at each row's own length", _row_errors(out, want, lens), TOL)
    for i, n in enumerate(lens):
        assert (out[i, :, n:] == 0).all(), "row %d is not exactly zero past its length %d" % (i, n)


@pytest.mark.parametrize("keep", [0, 1], ids=["even-rows", "odd-rows"])
def test_ragged_rows_are_isolated(setup, keep):
    """Same call again with everything a row must not depend on changed: the input past every length NaN, the workspace and
    the output buffer filled with 0xFF bytes beforehand, and the CONTENT of every other row replaced.  The kept rows must be
    finite and within 2e-6 of their first result (only the fp64 atomic order differs); every row exactly zero past its length."""
    from sudo_rm_rf_amd import engine as engine_mod
    cfg, model, x, lens, _ = setup
    with torch.no_grad():
        first = model.forward_ragged(x.to(DEV), lens).cpu()
    other = torch.from_numpy(weights.make_mixture(BATCH, T, 9131 + keep).astype(np.float32)) * 3.0 + 0.25
    x2 = x.clone()
    for i, n in enumerate(lens):
        if i % 2 != keep:
            x2[i] = other[i]
        x2[i, :, n:] = float("nan")
    eng = model._engine()
    eng.last_plan.workspace.fill_(0xFF)
    with torch.no_grad(), poisoned_allocations(engine_mod):
        out = model.forward_ragged(x2.to(DEV), lens).cpu()
    kept = [i for i in range(BATCH) if i % 2 == keep]
    for i in kept:
        assert torch.isfinite(out[i]).all(), "row %d is not finite" % i
    err = np.array([float((out[i, :, :lens[i]] - first[i, :, :lens[i]]).abs().max()) for i in kept])
    report("kept rows vs their first result", err, ORDER_TOL, labels=kept)
    for i, n in enumerate(lens):
        assert (out[i, :, n:] == 0).all(), "row %d is not exactly zero past its length %d" % (i, n)


def test_ragged_forward_with_equal_lengths_is_the_uniform_forward(setup):
    cfg, model, x, _, _ = setup
    rows = x[:BATCH].to(DEV)
    with torch.no_grad():
        a = model.forward_ragged(rows, [T] * BATCH)
        b = model(rows)
    report("forward_ragged(all lengths = T) vs model(x)", per_example_error(a, b.cpu()), ORDER_TOL)


def test_ragged_forward_is_inference_only(setup):
    cfg, model, x, lens, _ = setup
    with pytest.raises(NotImplementedError):
        model.forward_ragged(x.to(DEV), lens)            # (grad mode on, parameters require grad)


def test_separate_list_matches_separate_per_utterance(setup):
    """40 utterances of mixed length, level and offset: each result against pipeline.separate of that tensor alone (mixture
    consistency on by default for this model), within TOL * max(1, std_i); the whole list costs at most two plans and runs
    the ragged kernels."""
    from sudo_rm_rf_amd import ops, pipeline
    cfg, model, _, _, _ = setup
    rng = np.random.default_rng(78)
    n = 40
    lens = [int(v) for v in rng.integers(3000, T + 1, n)]
    gain = np.geomspace(0.05, 20.0, n)[rng.permutation(n)]
    mixes = [torch.from_numpy((gain[i] * weights.make_mixture(1, lens[i], 9600 + i)[0, 0] + rng.uniform(-0.5, 0.5)).astype(np.float32)).to(DEV)
             for i in range(n)]
    assert all(pipeline.ragged_route(model, m.numel()) == "ragged" for m in mixes)
    eng = model._engine()
    before = set(eng._plans)
    with ops.kernel_trace(DEV) as tr:
        got = pipeline.separate_list(model, [m if i % 2 else m.unsqueeze(0) for i, m in enumerate(mixes)], max_batch=20)
    made = set(eng._plans) - before
    print("separate_list: %d utterances, %d plans created: %s" % (n, len(made), sorted((k[1], k[2]) for k in made)))
    assert len(made) <= 2 < n
    assert {"tac_mfma_ragged", "pw_conv_small_ragged", "pyramid_merge_ragged", "overlap_add_ragged"} <= tr.names, tr.names
    err, bar = [], []
    for i, m in enumerate(mixes):
        want = pipeline.separate(model, m.unsqueeze(0))[0]
        assert got[i].shape == want.shape == (cfg.num_sources, lens[i])
        err.append(float((got[i] - want).abs().max()))
        bar.append(TOL * max(1.0, float(m.std())))
    report("separate_list vs separate per utterance", np.array(err), np.array(bar))


def test_separate_list_falls_back_for_other_groupcomm_models():
    """A 2-channel GroupComm model and a G = 8 model -- both otherwise of cfg 3's shape -- still go per utterance, with no
    ragged launch.  (separate() is defined for one-channel mixtures, so the 2-channel model shows its route and its plan.)"""
    from sudo_rm_rf_amd import ops, pipeline
    lens = [6500, 5800, 7100]
    for gcfg in (ModelConfig("groupcomm", 256, 512, 2, 5, 21, 512, 2, 2, 16), ModelConfig("groupcomm", 256, 512, 2, 5, 21, 512, 2, 1, 8)):
        mdl = build(gcfg, weights.make_state_dict(gcfg, seed=3))
        assert pipeline.ragged_route(mdl, lens[0]) == "single" and pipeline.ragged_route(mdl, T) == "single"
        assert not mdl._engine().ragged_plan_supported(BATCH, T, torch.device(DEV))
        if gcfg.in_audio_channels != 1:
            continue
        mixes = [torch.from_numpy(weights.make_mixture(1, n, 9300 + n)[0, 0].astype(np.float32) * 2.0 + 0.1).to(DEV) for n in lens]
        with ops.kernel_trace(DEV) as tr:
            got = pipeline.separate_list(mdl, mixes)
        assert not any(n.endswith("_ragged") or "_ragged<" in n for n in tr.names), tr.names
        for g, m in zip(got, mixes):
            want = pipeline.separate(mdl, m.unsqueeze(0))[0]
            assert g.shape == want.shape and float((g - want).abs().max()) <= TOL * max(1.0, float(m.std()))
