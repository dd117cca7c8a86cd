"""GPU parity of the FUSS recipe (csrc/srf_loss_fuss.hip) through the reference's own import paths: the zero-reference PIT-SNR
loss and its gradient, the stabilized SI-SDR metric with fewer targets than estimates, the online augmentation, and three steps
of the FUSS training loop at 4 sources -- against what the reference classes returned (tools/make_golden_fuss.py) and, on
shapes without fixtures, the fp64 restatement of tests/fuss_fixtures.py.

Bars (the ones tests/test_gpu_loss.py uses for the same kinds of quantity): loss and per-example values 2e-5 relative,
gradient 2e-5 of the fixture's largest gradient entry, metric 2e-4 + 2e-5 |value| dB, permutations exact.  The reference's own
fp32-vs-fp64 distance on every fixture is at most half of these (FUSS_MANIFEST.json, asserted in tests/test_fuss_host.py)."""
import itertools

import numpy as np
import pytest
import torch

from tests import fuss_fixtures as ff

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAN = ff.manifest()
LOSS = sorted(k for k, v in MAN.items() if v["kind"] == "loss")
METRIC = sorted(k for k, v in MAN.items() if v["kind"] == "metric")
AUG = sorted(k for k, v in MAN.items() if v["kind"] == "augment")
TRAJ = sorted(k for k, v in MAN.items() if v["kind"] == "traj")


def _snr(**kw):
    import sudo_rm_rf.dnn.losses.snr as snr_lib                             # the reference's import path
    return snr_lib.PermInvariantSNRwithZeroRefs(**kw)


def _runner_loss(n):                                                       # run_fuss_separation.py:97-101
    return _snr(n_sources=n, zero_mean=False, backward_loss=True, inactivity_threshold=-40.)


@pytest.mark.parametrize("name", LOSS)
def test_zeroref_snr_matches_reference_golden(name):
    c, z = MAN[name], ff.load(name)
    est_np, tgt_np = ff.make_loss_case(**c)
    S, B = c["n_src"], c["batch"]
    tgt = torch.tensor(tgt_np, device=DEV)
    est = torch.tensor(est_np, device=DEV, requires_grad=True)
    fn = _snr(n_sources=S, zero_mean=c["zero_mean"], backward_loss=True, inactivity_threshold=-40.)
    l, perms = fn(est, tgt, return_best_permutation=True)
    l.backward()
    print("%s: loss %.7f (reference %.7f)" % (name, l.item(), float(z["loss"])))
    assert l.shape == () and abs(l.item() - float(z["loss"])) <= 2e-5 * max(1.0, abs(float(z["loss"])))
    assert perms.dtype == torch.int64 and (perms.numpy() == z["perms"]).all()
    g = est.grad.cpu().numpy()
    k = z["grad_prefix"].shape[-1]
    scale = max(float(z["grad_absmax"]), 1e-12)
    err = np.abs(g[..., :k] - z["grad_prefix"]).max()
    print("%s: gradient error %.3e of the largest entry" % (name, err / scale))
    assert err <= 2e-5 * scale
    assert np.abs(g.sum(-1) - z["grad_sum"]).max() <= 1e-5 * max(1.0, np.abs(z["grad_sum"]).max())
    assert np.abs((g.astype(np.float64) ** 2).sum(-1) - z["grad_sqsum"]).max() <= 1e-4 * max(z["grad_sqsum"].max(), 1e-12)
    # per-example values, both signs
    ind = _snr(n_sources=S, zero_mean=c["zero_mean"], backward_loss=False, return_individual_results=True)
    vals = ind(est.detach(), tgt).cpu().numpy()
    assert vals.shape == (B,) and (np.abs(vals - z["values"]) <= 2e-5 * np.maximum(1.0, np.abs(z["values"]))).all()
    neg = _snr(n_sources=S, zero_mean=c["zero_mean"], backward_loss=True, return_individual_results=True)
    assert np.array_equal(neg(est.detach(), tgt).cpu().numpy(), -vals)
    pos = _snr(n_sources=S, zero_mean=c["zero_mean"], backward_loss=False)
    assert pos(est.detach(), tgt).item() == -l.item()
    # estimates matched with inactive targets: gradient rows EXACTLY zero; an all-silent example contributes 0
    plist = list(itertools.permutations(range(S)))
    _, _, active, _ = ff.zeroref_snr(torch.tensor(est_np), torch.tensor(tgt_np), c["zero_mean"])
    n_zero_rows = 0
    for b in range(B):
        for j in range(S):
            if not active[b, j]:
                assert (g[b, plist[int(z["perm_index"][b])][j]] == 0).all()
                n_zero_rows += 1
        if not active[b].any():
            assert vals[b] == 0
    assert n_zero_rows == B * S - sum(c["n_active"])


def test_tie_goes_to_the_itertools_first_permutation():
    c, z = MAN["fuss_loss_tie"], ff.load("fuss_loss_tie")
    est_np, tgt_np = ff.make_loss_case(**c)
    _, perms = _runner_loss(4)(torch.tensor(est_np, device=DEV), torch.tensor(tgt_np, device=DEV), return_best_permutation=True)
    assert (perms.numpy() == z["perms"]).all()
    for b in range(c["batch"]):
        dead = [j for j in range(4) if not np.any(tgt_np[b, j])]
        assert len(dead) >= 2
        got = [int(perms[b][j]) for j in dead]
        assert got == sorted(got)


def _random_case(B, S, T, seed, offset=0.0):
    rng = np.random.default_rng(seed)
    tgt = rng.standard_normal((B, S, T)) * rng.uniform(0.2, 1.0, (B, S, 1)) + offset
    tgt[rng.uniform(size=(B, S)) < 0.3] = 0.0
    est = np.take_along_axis(tgt, np.stack([rng.permutation(S) for _ in range(B)])[:, :, None], 1) + \
        0.2 * rng.standard_normal((B, S, T))
    return est.astype(np.float32), tgt.astype(np.float32)


@pytest.mark.parametrize("zero_mean", [False, True])
@pytest.mark.parametrize("B,S,T", [(3, 4, 1), (2, 4, 3), (3, 4, 515), (2, 4, 160000), (5, 1, 64), (4, 2, 1001), (3, 3, 4096),
                                   (2, 3, 4097), (300, 2, 40)])
def test_zeroref_snr_matches_fp64_restatement(B, S, T, zero_mean):
    """Shapes without fixtures: T = 1, 3 (scalar loads only), 515 and 1001 (rows not 16-byte aligned), 4096 / 4097 (one block /
    one sample into the second), the recipe's 160000; S = 1..4; more examples than the finalize block has threads; a scalar
    upstream gradient != 1 and a per-example upstream."""
    est_np, tgt_np = _random_case(B, S, T, 7 * B + S + T, offset=0.05 if zero_mean else 0.0)
    up = np.linspace(0.5, 2.0, B)
    v64, i64, _, g64 = ff.zeroref_loss_and_grad(est_np, tgt_np, zero_mean, upstream=up)
    gap = []
    _, _, _, allv = ff.zeroref_snr(torch.tensor(est_np), torch.tensor(tgt_np), zero_mean)
    for b in range(B):
        other = allv[b][allv[b] != v64[b]]
        gap.append(float(v64[b] - other.max()) if other.numel() else np.inf)
    tgt = torch.tensor(tgt_np, device=DEV)
    est = torch.tensor(est_np, device=DEV, requires_grad=True)
    ind = _snr(n_sources=S, zero_mean=zero_mean, backward_loss=False, return_individual_results=True)
    vals, perms = ind(est, tgt, return_best_permutation=True)
    (vals * torch.tensor(up, device=DEV, dtype=torch.float32)).sum().backward()          # [Bt] upstream, on the device
    assert (np.abs(vals.detach().cpu().numpy() - v64) <= 2e-5 * np.maximum(1.0, np.abs(v64))).all()
    plist = list(itertools.permutations(range(S)))
    for b in range(B):
        if gap[b] >= 0.01:
            assert tuple(int(x) for x in perms[b]) == plist[i64[b]]
    g = est.grad.cpu().numpy()
    clear = np.array(gap) >= 0.01
    assert np.abs(g - g64)[clear].max(initial=0.0) <= 2e-5 * max(np.abs(g64).max(), 1e-12)
    # mean reduction with a scalar upstream != 1
    est2 = torch.tensor(est_np, device=DEV, requires_grad=True)
    l = _snr(n_sources=S, zero_mean=zero_mean)(est2, tgt)
    (2.5 * l).backward()
    assert abs(l.item() + v64.mean()) <= 2e-5 * max(1.0, abs(v64.mean()))
    _, _, _, gm = ff.zeroref_loss_and_grad(est_np, tgt_np, zero_mean, upstream=np.full(B, -2.5 / B))
    assert np.abs(est2.grad.cpu().numpy() - gm)[clear].max(initial=0.0) <= 2e-5 * max(np.abs(gm).max(), 1e-12)


def test_zeroref_snr_crops_to_the_shorter_input_and_takes_views():
    est_np, tgt_np = _random_case(2, 4, 700, 77)
    want, _, _, g64 = ff.zeroref_loss_and_grad(est_np[..., :601], tgt_np[..., :601])
    big = torch.tensor(est_np, device=DEV)
    est = big[..., :650].requires_grad_()                     # a view whose rows are not contiguous
    ind = _snr(n_sources=4, backward_loss=False, return_individual_results=True)
    vals = ind(est, torch.tensor(tgt_np[..., :601], device=DEV))
    vals.sum().backward()
    assert (np.abs(vals.detach().cpu().numpy() - want) <= 2e-5 * np.maximum(1.0, np.abs(want))).all()
    g = est.grad.cpu().numpy()
    assert g.shape == (2, 4, 650) and (g[..., 601:] == 0).all()
    assert np.abs(g[..., :601] - g64).max() <= 2e-5 * np.abs(g64).max()


def test_zeroref_snr_rows_off_the_16_byte_grid():
    """T % 4 == 0 but the tensors start 4 bytes into their allocation: contiguous, not 16-byte aligned -> the scalar-load kernels;
    same values and gradient as the fp64 restatement, and the metric and the augmentation take such tensors too."""
    import sudo_rm_rf.dnn.losses.sisdr as sisdr_lib
    from sudo_rm_rf_amd import augment
    B, S, T = 3, 4, 2048
    est_np, tgt_np = _random_case(B, S, T, 99)
    v64, i64, _, g64 = ff.zeroref_loss_and_grad(est_np, tgt_np)

    def shifted(a):
        buf = torch.empty(a.size + 1, dtype=torch.float32, device=DEV)
        buf[1:] = torch.tensor(a.reshape(-1), device=DEV)
        t = buf[1:].view(a.shape)
        assert t.is_contiguous() and t.data_ptr() % 16 == 4
        return t

    est, tgt = shifted(est_np).requires_grad_(), shifted(tgt_np)
    ind = _snr(n_sources=S, backward_loss=False, return_individual_results=True)
    vals = ind(est, tgt)
    vals.sum().backward()
    assert (np.abs(vals.detach().cpu().numpy() - v64) <= 2e-5 * np.maximum(1.0, np.abs(v64))).all()
    assert np.abs(est.grad.cpu().numpy() - g64).max() <= 2e-5 * np.abs(g64).max()
    fn = sisdr_lib.StabilizedPermInvSISDRMetric(zero_mean=True, n_estimated_sources=4, n_actual_sources=2, backward_loss=False,
                                                improvement=True, return_individual_results=True)
    want, _, _ = ff.stabilized_sisdr(torch.tensor(est_np), torch.tensor(tgt_np[:, :2]), improvement=True)
    with torch.no_grad():
        got = fn(est.detach(), shifted(np.ascontiguousarray(tgt_np[:, :2])))
    ok = np.abs(want.numpy()) < 30
    assert (np.abs(got.cpu().numpy() - want.numpy())[ok] <= 2e-4 + 2e-5 * np.abs(want.numpy()[ok])).all()
    src_b, src_s, gain = augment.fuss_draws(B, S)
    src, mix, _, _ = augment.fuss_augment_with_draws(tgt, src_b, src_s, gain)
    w_src, w_mix, _, _ = ff.augment(tgt_np, src_b.numpy(), src_s.numpy(), gain.numpy())
    assert np.array_equal(src.cpu().numpy(), w_src.numpy()) and np.abs(mix.cpu().numpy() - w_mix.numpy()).max() <= 2e-5


@pytest.mark.parametrize("name", METRIC)
def test_stabilized_metric_matches_reference_golden(name):
    import sudo_rm_rf.dnn.losses.sisdr as sisdr_lib
    c, z = MAN[name], ff.load(name)
    pr_np, tgt_np = ff.make_metric_case(**c)
    fn = sisdr_lib.StabilizedPermInvSISDRMetric(zero_mean=True, single_source=False, n_estimated_sources=c["n_est"],
                                                n_actual_sources=c["n_act"], backward_loss=False, improvement=c["improvement"],
                                                return_individual_results=True)          # run_fuss_separation.py:123-131
    with torch.no_grad():
        val, perms = fn(torch.tensor(pr_np, device=DEV), torch.tensor(tgt_np, device=DEV), return_best_permutation=True)
        only = fn(torch.tensor(pr_np, device=DEV), torch.tensor(tgt_np, device=DEV))
    got = val.cpu().numpy()
    print("%s: max |value - reference| = %.3e dB" % (name, np.abs(got - z["value"]).max()))
    assert got.shape == z["value"].shape
    assert (np.abs(got - z["value"]) <= 2e-4 + 2e-5 * np.abs(z["value"])).all()
    assert perms.shape == (c["batch"], c["n_act"]) and (perms.numpy() == z["perms"]).all()
    assert torch.equal(only, val)


@pytest.mark.parametrize("n_est,n_act,T,zero_mean,improvement,single", [
    (4, 2, 515, False, True, False), (3, 3, 1, False, False, False), (4, 4, 160000, True, True, False),
    (1, 1, 4096, True, False, True), (2, 1, 3, True, False, False), (4, 3, 8192, True, True, False)])
def test_stabilized_metric_matches_fp64_restatement(n_est, n_act, T, zero_mean, improvement, single):
    import sudo_rm_rf.dnn.losses.sisdr as sisdr_lib
    B = 300 if T == 3 else 3
    pr_np, tgt_np = ff.make_metric_case(B, 3 if single else n_est, n_act, T, 90 + n_est + n_act, [3.0, 8.0, 12.0])
    if T <= 3:      # (a handful of samples: rho^2 is within rounding of 1 for some pairs; keep them apart)
        rng = np.random.default_rng(5)
        pr_np, tgt_np = rng.standard_normal(pr_np.shape).astype(np.float32), rng.standard_normal(tgt_np.shape).astype(np.float32)
    want, idx, allv = ff.stabilized_sisdr(torch.tensor(pr_np), torch.tensor(tgt_np), zero_mean, single, improvement)
    raw = want if not improvement else ff.stabilized_sisdr(torch.tensor(pr_np), torch.tensor(tgt_np), zero_mean, single)[0]
    fn = sisdr_lib.StabilizedPermInvSISDRMetric(zero_mean=zero_mean, single_source=single, n_estimated_sources=n_est,
                                                n_actual_sources=n_act, backward_loss=True, improvement=improvement,
                                                return_individual_results=True)
    with torch.no_grad():
        val, perms = fn(torch.tensor(pr_np, device=DEV), torch.tensor(tgt_np, device=DEV), return_best_permutation=True)
    got = -val.cpu().numpy()
    # 1 - rho^2 loses digits as rho^2 -> 1 (and rho^2 as it -> 0): only examples at moderate values are judged at the metric's bar
    ok = (raw.numpy() < 30) & (raw.numpy() > -30) if T > 3 else np.zeros(B, bool)
    assert (np.abs(got - want.numpy())[ok] <= 2e-4 + 2e-5 * np.abs(want.numpy()[ok])).all()
    assert np.isfinite(got).all()
    plist = list(itertools.permutations(range(n_est), r=n_act))
    for b in range(B):
        other = allv[b][allv[b] != allv[b].max()]
        if ok[b] and (not other.numel() or float(allv[b].max() - other.max()) >= 0.01):
            assert tuple(int(x) for x in perms[b]) == plist[idx[b]]


@pytest.mark.parametrize("name", AUG)
def test_fuss_augmentation_matches_reference_draws_and_restatement(name):
    from sudo_rm_rf_amd import augment
    c, z = MAN[name], ff.load(name)
    clean = ff.make_clean(**c)
    torch.manual_seed(c["seed"])
    src, mix, mean, std = augment.fuss_online_augment(torch.tensor(clean, device=DEV))
    B, S, T = clean.shape
    assert src.shape == (B, S, T) and mix.shape == (B, 1, T) and mean.shape == (B, 1, 1) and std.shape == (B, 1, 1)
    assert np.array_equal(src.cpu().numpy(), z["sources"])              # same draws, one float32 product: bit for bit
    w_src, w_mix, w_mean, w_std = ff.augment(clean, z["src_b"], z["src_s"], z["gain"])
    assert np.abs(mix.cpu().numpy() - w_mix.numpy()).max() <= 2e-5       # normalised mixture, O(1) values, fp32
    assert np.abs(mean.cpu().numpy() - w_mean.numpy()).max() <= 1e-6
    assert np.abs(std.cpu().numpy() / w_std.numpy() - 1).max() <= 1e-5
    assert np.abs(mix.cpu().numpy() - z["mixture"]).max() <= 2e-5
    again = augment.fuss_augment_with_draws(torch.tensor(clean, device=DEV), torch.tensor(z["src_b"]), torch.tensor(z["src_s"]),
                                            torch.tensor(z["gain"]))
    for a, b in zip(again, (src, mix, mean, std)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("B,S,T", [(2, 4, 160000), (3, 1, 3), (4, 2, 4097)])
def test_fuss_augmentation_other_shapes(B, S, T):
    from sudo_rm_rf_amd import augment
    clean = ff.make_clean(B, S, T, 60 + S)
    torch.manual_seed(B + S)
    src_b, src_s, gain = augment.fuss_draws(B, S)
    torch.manual_seed(B + S)
    src, mix, mean, std = augment.fuss_online_augment(torch.tensor(clean, device=DEV))
    w_src, w_mix, w_mean, w_std = ff.augment(clean, src_b.numpy(), src_s.numpy(), gain.numpy())
    assert np.array_equal(src.cpu().numpy(), w_src.numpy())
    live = (w_std.numpy() > 0).reshape(-1)
    assert np.abs(mix.cpu().numpy() - w_mix.numpy())[live].max(initial=0.0) <= 2e-5
    assert (mix.cpu().numpy()[~live] == 0).all()
    assert np.abs(mean.cpu().numpy() - w_mean.numpy()).max() <= 1e-6


def _build(cfg, sd):
    import sudo_rm_rf.dnn.models.groupcomm_sudormrf_v2 as sudormrf_gc_v2
    import sudo_rm_rf.dnn.models.improved_sudormrf as improved_sudormrf
    cls = improved_sudormrf.SuDORMRF if cfg.variant == "improved" else sudormrf_gc_v2.GroupCommSudoRmRf
    m = cls(**cfg.ctor_kwargs())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(DEV)


@pytest.mark.parametrize("name", TRAJ)
def test_fuss_training_trajectory_matches_reference_loop(name):
    """THREE steps of the FUSS loop body (run_fuss_separation.py:232-265: online_augment with the fixture's draws, mixture
    normalisation, model, mixture_consistency.apply, zero-reference SNR, clip_grad_norm_(5.0), Adam(lr=1e-3)) for a 4-source
    Improved and a 4-source GroupComm model, through the public modules only, against the trajectory the reference modules
    produced; same checker and tolerance as the existing small-model trajectory."""
    import sudo_rm_rf.dnn.experiments.utils.mixture_consistency as mixture_consistency
    from oracle.weights import make_state_dict
    from sudo_rm_rf_amd import augment, optim
    from test_oracle_golden import check_trajectory_against_golden
    c, z = MAN[name], ff.load(name)
    cfg, batch, T, wseed, dseed = ff.traj_configs()[name]
    assert cfg.as_dict() == c["config"] and cfg.num_sources == 4
    sd = make_state_dict(cfg, wseed)
    model = _build(cfg, sd).train()
    opt = optim.FusedClipAdam(model.parameters(), lr=c["lr"], clip_grad_norm=c["clip_grad_norm"])
    loss_fn = _runner_loss(4)
    losses = []
    for clean, src_b, src_s, gain in ff.make_traj_batches(batch, 4, T, dseed):
        opt.zero_grad()
        clean_wavs, input_mixture, _, _ = augment.fuss_augment_with_draws(
            torch.tensor(clean, device=DEV), torch.tensor(src_b), torch.tensor(src_s), torch.tensor(gain))
        rec = mixture_consistency.apply(model(input_mixture), input_mixture)
        l = loss_fn(rec, clean_wavs)
        l.backward()
        opt.step()
        losses.append(l.item())
    print(name, "losses", losses, "reference", list(z["losses"]))
    check_trajectory_against_golden([(k, p.detach().cpu().numpy()) for k, p in model.state_dict(keep_vars=True).items()], sd, losses,
                                    z, 2e-3)


@pytest.mark.parametrize("T", [515, 160000])
def test_dispatch_and_determinism(T):
    """A loss forward + backward is exactly three launches, the same at every length, and two runs on the
    same inputs give identical bits (the block sums are written and added in block order, not accumulated atomically)."""
    from sudo_rm_rf_amd import ops
    est_np, tgt_np = _random_case(4, 4, T, 123)
    tgt = torch.tensor(tgt_np, device=DEV)
    runs = []
    for _ in range(2):
        est = torch.tensor(est_np, device=DEV, requires_grad=True)
        with ops.kernel_trace(DEV) as tr:
            l = _runner_loss(4)(est, tgt)
            l.backward()
        assert [n for n, _ in tr.launches] == ["zeroref_snr_stats", "zeroref_snr_finalize", "zeroref_snr_grad"]
        runs.append((l.detach().clone(), est.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    import sudo_rm_rf.dnn.losses.sisdr as sisdr_lib
    from sudo_rm_rf_amd import augment
    fn = sisdr_lib.StabilizedPermInvSISDRMetric(zero_mean=True, n_estimated_sources=4, n_actual_sources=3, backward_loss=False,
                                                improvement=True, return_individual_results=True)
    with torch.no_grad(), ops.kernel_trace(DEV) as tr:
        a = fn(torch.tensor(est_np, device=DEV), tgt[:, :3].contiguous())
        torch.manual_seed(1)
        s1 = augment.fuss_online_augment(tgt)
    assert [n for n, _ in tr.launches] == ["stab_sisdr_stats", "stab_sisdr_finalize", "fuss_augment_gather",
                                          "fuss_augment_normalize"]
    with torch.no_grad():
        b = fn(torch.tensor(est_np, device=DEV), tgt[:, :3].contiguous())
        torch.manual_seed(1)
        s2 = augment.fuss_online_augment(tgt)
    assert torch.equal(a, b) and all(torch.equal(x, y) for x, y in zip(s1, s2))
