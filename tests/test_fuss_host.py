"""The FUSS recipe (zero-reference SNR loss, stabilized SI-SDR metric, online augmentation), host side (no GPU): the fp64
restatements of tests/fuss_fixtures.py against what the reference classes returned (tools/make_golden_fuss.py), the
reference's import path and constructors, and the refusals, which must all come back before anything is launched."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest
import torch

from tests import fuss_fixtures as ff

MAN = ff.manifest()
LOSS = sorted(k for k, v in MAN.items() if v["kind"] == "loss")
METRIC = sorted(k for k, v in MAN.items() if v["kind"] == "metric")
AUG = sorted(k for k, v in MAN.items() if v["kind"] == "augment")


def test_manifest_covers_what_the_checks_need():
    assert set(LOSS) == set(ff.LOSS_CASES) and set(METRIC) == set(ff.METRIC_CASES) and set(AUG) == set(ff.AUG_CASES)
    n_active = {(MAN[k]["n_src"], n) for k in LOSS for n in MAN[k]["n_active"]}
    assert {(4, n) for n in range(5)} <= n_active                      # 4, 3, 2, 1 and 0 of 4 active
    assert MAN["fuss_loss_threshold"]["n_active"] == [3, 4]            # one non-zero target just below, one just above -40 dB
    assert {(MAN[k]["n_est"], MAN[k]["n_act"]) for k in METRIC} == {(e, a) for e in range(1, 5) for a in range(1, e + 1)}
    for k in LOSS + METRIC:
        assert min(MAN[k]["perm_gap_db"]) >= 0.01
    for k in LOSS:      # the reference's own fp32-vs-fp64 distance is at most half the bar of the GPU test (2e-5)
        assert max(MAN[k]["ref_fp32_vs_fp64"].values()) <= 1e-5
    for k in METRIC:
        assert MAN[k]["ref_fp32_vs_fp64"]["fraction_of_bar"] <= 0.5


@pytest.mark.parametrize("name", LOSS)
def test_zeroref_snr_restatement_reproduces_the_reference(name):
    c, z = MAN[name], ff.load(name)
    est, tgt = ff.make_loss_case(**c)
    B = c["batch"]
    vals, idx, active, grad = ff.zeroref_loss_and_grad(est, tgt, c["zero_mean"], upstream=np.full(B, -1.0 / B))
    assert [int(a) for a in active.sum(-1)] == c["n_active"]
    assert (np.abs(vals - z["values"]) <= 2e-5 * np.maximum(1.0, np.abs(vals))).all()
    assert abs(-vals.mean() - float(z["loss"])) <= 2e-5 * max(1.0, abs(vals.mean()))
    perms = list(itertools.permutations(range(c["n_src"])))
    assert (idx == z["perm_index"]).all() and (np.array([perms[i] for i in idx]) == z["perms"]).all()
    k = z["grad_prefix"].shape[-1]
    scale = float(z["grad_absmax"])
    assert np.abs(grad[..., :k] - z["grad_prefix"]).max() <= 2e-5 * max(scale, 1e-12)
    assert np.abs(grad.sum(-1) - z["grad_sum"]).max() <= 1e-5 * max(1.0, np.abs(z["grad_sum"]).max())
    # an estimate matched with an inactive target gets no gradient -- in the reference's own output
    for b in range(B):
        for j in range(c["n_src"]):
            if not active[b, j]:
                i = perms[idx[b]][j]
                assert (z["grad_prefix"][b, i] == 0).all() and z["grad_sqsum"][b, i] == 0


def test_tie_case_returns_the_itertools_first_permutation():
    """Permutations that differ only in which estimates go to inactive targets have EXACTLY the same value; the reference returns
    the first in itertools order, i.e. the inactive targets take their estimates in ascending order."""
    c, z = MAN["fuss_loss_tie"], ff.load("fuss_loss_tie")
    est, tgt = ff.make_loss_case(**c)
    best, idx, active, allv = ff.zeroref_snr(torch.tensor(est), torch.tensor(tgt))
    for b in range(c["batch"]):
        ties = (allv[b] == best[b]).nonzero().flatten().tolist()
        assert len(ties) == math.factorial(4 - c["n_active"][b]) and len(ties) >= 2
        assert int(z["perm_index"][b]) == ties[0]
        dead = [j for j in range(4) if not active[b, j]]
        assigned = [int(z["perms"][b][j]) for j in dead]
        assert assigned == sorted(assigned)


@pytest.mark.parametrize("name", METRIC)
def test_stabilized_metric_restatement_reproduces_the_reference(name):
    c, z = MAN[name], ff.load(name)
    pr, tgt = ff.make_metric_case(**c)
    best, idx, _ = ff.stabilized_sisdr(torch.tensor(pr), torch.tensor(tgt), improvement=c["improvement"])
    assert (np.abs(best.numpy() - z["value"]) <= 2e-4 + 2e-5 * np.abs(z["value"])).all()
    perms = list(itertools.permutations(range(c["n_est"]), r=c["n_act"]))
    assert (np.array([perms[i] for i in idx]) == z["perms"]).all()


@pytest.mark.parametrize("name", AUG)
def test_augmentation_restatement_and_draws_reproduce_the_reference(name):
    from sudo_rm_rf_amd import augment
    c, z = MAN[name], ff.load(name)
    torch.manual_seed(c["seed"])
    src_b, src_s, gain = augment.fuss_draws(c["batch"], c["n_src"])      # the library's draws == the reference's
    assert (src_b.numpy() == z["src_b"]).all() and (src_s.numpy() == z["src_s"]).all()
    assert np.array_equal(gain.numpy(), z["gain"])
    clean = ff.make_clean(**c)
    src, mix, mean, std = ff.augment(clean, z["src_b"], z["src_s"], z["gain"])
    assert np.array_equal(src.numpy(), z["sources"])
    assert np.abs(mix.numpy() - z["mixture"]).max() <= 1e-5
    assert np.abs(mean.numpy() - z["mean"]).max() <= 1e-6 and np.abs(std.numpy() / z["std"] - 1).max() <= 1e-5


def test_reference_import_path_and_constructors():
    import sudo_rm_rf.dnn.losses.sisdr as sisdr_lib
    import sudo_rm_rf.dnn.losses.snr as snr_lib
    fn = snr_lib.PermInvariantSNRwithZeroRefs(n_sources=4, zero_mean=False, backward_loss=True, inactivity_threshold=-40.)
    assert (fn.n_sources, fn.perform_zero_mean, fn.backward_loss, fn.inactivity_threshold, fn.return_individual_results) == \
        (4, False, True, -40., False)
    assert len(fn.permutations) == 24 and fn.permutations_tensor.shape == (24, 4) and fn.permutations_tensor.dtype == torch.int64
    assert [int(x) for x in fn.permutations[1]] == [0, 1, 3, 2]
    assert not hasattr(snr_lib, "SimplerPermInvariantSNRwithZeroRefs")
    m = sisdr_lib.StabilizedPermInvSISDRMetric(zero_mean=True, n_estimated_sources=4, n_actual_sources=2, backward_loss=False,
                                               improvement=True, return_individual_results=True)
    assert m.permutations_tensor.shape == (12, 2) and [int(x) for x in m.permutations[3]] == [1, 0]
    assert (m.perform_zero_mean, m.single_source, m.improvement, m.backward_loss) == (True, False, True, False)
    with pytest.raises(AssertionError, match="Estimates need to be at least"):
        sisdr_lib.StabilizedPermInvSISDRMetric(n_estimated_sources=2, n_actual_sources=3)
    with pytest.raises(AssertionError):
        sisdr_lib.StabilizedPermInvSISDRMetric(single_source=True, n_estimated_sources=2, n_actual_sources=2)


def test_cpu_tensors_and_wrong_shapes_are_refused():
    import sudo_rm_rf.dnn.losses.sisdr as sisdr_lib
    import sudo_rm_rf.dnn.losses.snr as snr_lib
    from sudo_rm_rf_amd import augment
    from sudo_rm_rf_amd._lib import SrfError
    fn = snr_lib.PermInvariantSNRwithZeroRefs(n_sources=4)
    with pytest.raises(SrfError, match="MI355X only"):
        fn(torch.randn(2, 4, 100), torch.randn(2, 4, 100))
    with pytest.raises(RuntimeError, match="constructed for 4 sources, got 3"):
        fn(torch.randn(2, 3, 100), torch.randn(2, 3, 100))
    m = sisdr_lib.StabilizedPermInvSISDRMetric(zero_mean=True, n_estimated_sources=4, n_actual_sources=2)
    with torch.no_grad():
        with pytest.raises(SrfError, match="MI355X only"):
            m(torch.randn(2, 4, 100), torch.randn(2, 2, 100))
        with pytest.raises(AssertionError):
            m(torch.randn(2, 4, 100), torch.randn(2, 3, 100))            # sisdr.py:521
        with pytest.raises(RuntimeError, match="constructed for 4 estimated"):
            m(torch.randn(2, 3, 100), torch.randn(2, 2, 100))
    with pytest.raises(NotImplementedError):
        m(torch.randn(2, 4, 100, requires_grad=True), torch.randn(2, 2, 100))
    with pytest.raises(SrfError, match="MI355X only"):
        augment.fuss_online_augment(torch.randn(2, 4, 100))


def _err(lib):
    return lib.srf_last_error().decode()


def test_library_refusals_come_before_any_launch():
    """Fake (aligned, never dereferenced) device pointers on a machine without a GPU: every refusal must return before the first
    launch, or this test would crash instead of reading an error message."""
    from sudo_rm_rf_amd import _lib
    lib = _lib.load()
    p = lambda k: C.c_void_p(4096 * k)
    f = C.c_float

    def fwd(S, Bt=2, T=100, work=p(3)):
        return lib.srf_zeroref_snr_forward(p(1), p(2), Bt, S, T, 0, f(-40.), f(1e-3), f(1e-9), work, p(4), p(5), p(6), None)

    def bwd(S, Bt=2, T=100, grad=p(5)):
        return lib.srf_zeroref_snr_backward(p(1), p(2), Bt, S, T, p(3), None, 0, grad, None)

    for call in (fwd, bwd):
        assert call(5) == -1 and "5 sources" in _err(lib) and "limit is 4" in _err(lib)
        assert call(0) == -1 and "0 sources" in _err(lib)
        assert call(4, Bt=0) == -1 and "Bt = 0" in _err(lib)
        assert call(4, T=0) == -1 and "T = 0" in _err(lib)
        assert call(4, Bt=70000) == -1 and "70000" in _err(lib)
    assert fwd(4, work=None) == -1 and "null" in _err(lib)
    assert fwd(4, work=C.c_void_p(4096 * 3 + 4)) == -1 and "aligned" in _err(lib)
    assert bwd(4, grad=None) == -1 and "null" in _err(lib)
    assert lib.srf_zeroref_snr_work_bytes(2, 5, 100) == 0 and lib.srf_zeroref_snr_work_bytes(2, 4, 100) > 0
    # work = per block of 4096 samples and per example S^2 + 3 S + 1 doubles, the totals, 2 floats + 1 int per estimate
    assert lib.srf_zeroref_snr_work_bytes(3, 4, 8193) == 3 * ((3 + 1) * 29 * 8 + 4 * 8 + 4 * 4)

    def metric(rows, ne, na, Bt=2, T=100):
        return lib.srf_stab_sisdr(p(1), p(2), Bt, rows, ne, na, T, 1, 1, C.c_double(1e-9), p(3), p(4), p(5), None)

    assert metric(2, 2, 3) == -1 and "3 actual sources with 2 estimated" in _err(lib)
    assert metric(5, 5, 2) == -1 and "5 estimated sources" in _err(lib) and "limit is 4" in _err(lib)
    assert metric(4, 4, 0) == -1 and "0 actual" in _err(lib)
    assert metric(3, 4, 2) == -1 and "3 estimate rows for 4" in _err(lib)
    assert metric(4, 4, 2, T=0) == -1 and "T = 0" in _err(lib)

    def aug(S, B=2, T=100, out=p(5)):
        return lib.srf_fuss_augment(p(1), p(2), p(3), p(4), B, S, T, f(1e-9), out, p(6), p(7), p(8), None)

    assert aug(5) == -1 and "limit is 4" in _err(lib)
    assert aug(4, B=0) == -1 and "B = 0" in _err(lib)
    assert aug(4, out=p(1)) == -1 and "alias" in _err(lib)
    assert lib.srf_fuss_augment_scratch_bytes(3, 8193) == 3 * 3 * 16
