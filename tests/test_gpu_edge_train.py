"""Training steps on batches that contain degenerate rows (tests/edge_signals.py): the improved and the GroupComm model
(srf_forward_train / srf_backward; GroupComm with mixture consistency between the model and the loss, as its runner has it), the
causal and the original model (enable_hip_training()).

Per family and case -- a batch with one silent row, one that falls silent half-way, DC, a tiny level, an all-silent batch, and a
near-silent row behind a first norm whose beta is 0 (as at initialisation: the first GEMM's operand level is then set by the raw
signal, where the two-fp16-part GEMM's lower limit is reachable) -- the parameter gradients of sum(out * g), g seeded, against fp64
autograd of the family's restatement.  Bar: the families' tiny-case bar, 2e-4 of each tensor's largest reference entry; a tensor
whose fp64 gradient is identically zero must be exactly zero; everything finite.  Improved / GroupComm: the gradient with respect
to the waveform too (srf_backward_wav).  Then one step of each family's own loss and FusedClipAdam on the all-silent batch."""
import numpy as np
import pytest
import torch

from tests import edge_signals as es

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BATCH, T = 2, 1001
TOL = 2e-4
FAMILIES = ("improved", "groupcomm", "causal", "orig")
CASES = ("one_silent_row", "half_silent", "dc", "tiny", "silence", "near_silent_row_beta0")
# (the causal model has no norm at all: its case is the near-silent row alone, which differs from one_silent_row only by the 1e-8
# noise in row 0 and gives the same figures -- kept so that every family has the case)
FIRST_NORM_BETA = {"improved": "ln.beta", "groupcomm": "ln.beta", "orig": "ln.bias"}
_LINES = []


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    from sudo_rm_rf_amd import _lib, ops
    _lib.load()
    ops.set_kernel_mode(0)
    ops.set_debug_flags(0)
    yield
    if _LINES:
        es.write_profile_lines("gradients", _LINES)


def case_input(family, case):
    """(state dict, mixture [BATCH, 1, T] float32)"""
    sd = dict(es.state_dict(family))
    sig = es.signals(BATCH, 1, T)
    if case != "near_silent_row_beta0":
        return sd, sig[case]
    if family in FIRST_NORM_BETA:
        sd[FIRST_NORM_BETA[family]] = np.zeros_like(sd[FIRST_NORM_BETA[family]])
    x = sig["one_silent_row"].copy()
    x[0] = sig["near_silent"][0]
    return sd, x


def gout(family):
    S = 2
    return torch.randn(BATCH, S, T, generator=torch.Generator().manual_seed(77), dtype=torch.float64)


def reference_grads(family, sd, x):
    """fp64 autograd of sum(out * g) through the restatement: ({name: gradient}, d / d mixture or None)"""
    cfg, g = es.config(family), gout(family)
    if family in ("improved", "groupcomm"):
        from oracle import torch_oracle
        leaves = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in sd.items()}
        x64 = torch.tensor(x, dtype=torch.float64, requires_grad=True)
        out = torch_oracle.forward(cfg, leaves, x64)
        if family == "groupcomm":
            out = out + (x64 - out.sum(1, keepdim=True)) / out.shape[1]
        (out * g).sum().backward()
        return {k: v.grad.numpy() for k, v in leaves.items() if v.grad is not None}, x64.grad.numpy()
    if family == "causal":
        from tests import causal_train_ref as ctr
        return ctr.linear_loss_grads(cfg, sd, x, g)[1], None
    from tests import original_train_ref as otr
    return otr.restatement_grads(cfg, sd, x, g)[1], None


def train_model(family, sd):
    cfg = es.config(family)
    torch.manual_seed(0)
    m = es.module_class(family)(**(cfg.ctor_kwargs() if hasattr(cfg, "ctor_kwargs") else cfg))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.to(DEV).train()
    return m.enable_hip_training() if family in ("causal", "orig") else m


def forward(family, m, x):
    out = m(x)
    if family == "groupcomm":
        import sudo_rm_rf.dnn.experiments.utils.mixture_consistency as mixture_consistency
        out = mixture_consistency.apply(out, x)
    return out


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("family", FAMILIES)
def test_gradients_on_degenerate_batches(family, case):
    """Measured on an MI355X (profiles/edge_signals.txt): worst tensor per case 3.7e-7 .. 9.3e-5 of its largest entry, bar 2e-4;
    every tensor that is identically zero in fp64 is exactly zero.  causal-half_silent is the case that moved the causal
    backward's small data-gradient GEMMs into the exact-fp32 class (csrc/srf_causal_train.hip): mask_net.0.weight, one sum of
    3104 terms that cancels to 6e-4 of their size, was 4.4e-4 of its value off with the on-the-fly split-bf16 kernels."""
    sd, x = case_input(family, case)
    want, want_wav = reference_grads(family, sd, x)
    m = train_model(family, sd)
    xd = torch.from_numpy(x).to(DEV)
    if want_wav is not None:
        xd.requires_grad_()
    out = forward(family, m, xd)
    (out * gout(family).float().to(DEV)).sum().backward()
    torch.cuda.synchronize()
    got = {k: p.grad.detach().cpu().numpy() for k, p in m.state_dict(keep_vars=True).items() if getattr(p, "grad", None) is not None}
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    if want_wav is not None:
        got["d/d mixture"], want["d/d mixture"] = xd.grad.cpu().numpy(), want_wav
    worst, zeros, failed = ("", 0.0), 0, []
    for k, w in want.items():
        g = got[k]
        assert g.size == w.size and np.isfinite(g).all(), (family, case, k)
        g = g.reshape(w.shape)                    # (the causal model's skipinit_gain: a 0-d parameter, [1] in the restatement)
        wmax = float(np.abs(w).max())
        if wmax == 0.0:
            zeros += 1
            if g.any():
                failed.append("%s: reference identically zero, got max %.3e" % (k, float(np.abs(g).max())))
            continue
        rel = float(np.abs(g.astype(np.float64) - w).max()) / wmax
        if rel > worst[1]:
            worst = (k, rel)
        if rel > TOL:
            failed.append("%s: %.3e of its largest entry %.3e" % (k, rel, wmax))
    line = "%-9s %-22s worst %.3e (%s) bar %.1e; %d of %d tensors identically zero in fp64" % (
        family, case, worst[1], worst[0], TOL, zeros, len(want))
    print(line)
    _LINES.append(line)
    assert not failed, (line, failed)
    if case == "silence":
        enc = [k for k in want if k.startswith("encoder") and k.endswith("weight")]
        assert enc and all(not want[k].any() and not got[k].any() for k in enc), "the encoder weight sees only zeros under silence"


@pytest.mark.parametrize("family", FAMILIES)
def test_one_optimizer_step_on_an_all_silent_batch_leaves_every_parameter_finite(family):
    """The family's own loss (PIT-SI-SDR, clamped, as the runners have it; the FUSS zero-reference SNR for the causal model; the
    original runner's PermInvariantSISDR with the improvement term) on silent mixtures and silent targets, then the fused clip +
    Adam step: whatever the loss makes of 0 / (0 + eps), no parameter may turn non-finite.  The original runner's loss IS NaN
    there, in the reference as here (log10(0 / eps) - log10(0 / eps), with non-finite gradients): what keeps the parameters is
    FusedClipAdam, which leaves a step whose gradient norm is not finite unapplied and reports it through check_finite()."""
    import sudo_rm_rf.dnn.losses.sisdr as sisdr_lib
    import sudo_rm_rf.dnn.losses.snr as snr_lib
    from sudo_rm_rf_amd import optim
    sd = es.state_dict(family)
    m = train_model(family, sd)
    opt = optim.FusedClipAdam(m.parameters(), lr=1e-3, clip_grad_norm=5.0)
    mix = torch.zeros(BATCH, 1, T, device=DEV)
    clean = torch.zeros(BATCH, 2, T, device=DEV)
    opt.zero_grad()
    rec = forward(family, m, mix)
    if family in ("improved", "groupcomm"):
        loss = torch.clamp(sisdr_lib.PITLossWrapper(sisdr_lib.PairwiseNegSDR("sisdr"), pit_from="pw_mtx")(rec, clean), min=-30., max=+30.)
    elif family == "causal":
        import sudo_rm_rf.dnn.experiments.utils.mixture_consistency as mixture_consistency
        rec = mixture_consistency.apply(rec, mix)
        loss = snr_lib.PermInvariantSNRwithZeroRefs(n_sources=2, zero_mean=False, backward_loss=True, inactivity_threshold=-40.)(rec, clean)
    else:
        loss = sisdr_lib.PermInvariantSISDR(batch_size=BATCH, n_sources=2, zero_mean=True, backward_loss=True,
                                            improvement=True)(rec, clean, initial_mixtures=mix)
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    print("%s: loss on the all-silent batch %r" % (family, loss.item()))
    bad = [k for k, p in m.state_dict().items() if not torch.isfinite(p).all()]
    assert not bad, (family, loss.item(), bad)
