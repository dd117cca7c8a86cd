"""Depths 7 and 8 at model level: Improved and GroupComm inference on each pyramid path a deep model can take, against the fp64
CPU oracle (oracle/np_oracle.py, pinned to the reference's goldens, main_groupcomm_d7_k91 among them), and one training step
against gradients the reference itself produced (tools/make_golden_train.py: train_tiny_improved_d7, train_tiny_improved_d8,
train_tiny_groupcomm_d7).  The causal model's depth-8 fixtures (causal_tiny_d8, causal_train_tiny_d8) run through the
parametrisations of tests/test_gpu_causal.py, test_gpu_causal_stream.py and test_gpu_causal_train.py.

Above depth 6 the register-resident pyramid does not exist: inference runs the LDS kernels of csrc/srf_pyramid.hip (block per
row, or wave per 512-frame tile) or, where they refuse the length, one kernel per level; the training forward always runs level
by level, and the backward folds the merge backward of ALL levels -- 6 and 7 included, reachable from nowhere else -- into the
apply pass of final_norm's GlobLN backward."""
import numpy as np
import pytest
import torch

from oracle import np_oracle, weights
from oracle.schema import ModelConfig
from sudo_rm_rf_amd.ops import DebugFlag
from test_gpu_model import TOL, build

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    from sudo_rm_rf_amd import ops
    ops.set_kernel_mode(0)
    yield
    ops.set_kernel_mode(0)


# ---- inference -------------------------------------------------------------------------------------------------------------------
def _config(variant, D):
    if variant == "improved":
        return ModelConfig("improved", 8, 16, 2, D, 21, 16, 2)
    return ModelConfig("groupcomm", 16, 16, 1, D, 21, 16, 2, 1, 4)       # 4 groups of 4 channels


# (D, T, frames, path): T pads to frames * 10 samples (the reference's rule: a multiple of 10 * 2^D)
INFER = [(7, 5000, 512, "lds-rows"), (7, 10000, 1024, "lds-tiles"), (8, 10000, 1024, "lds-tiles"), (8, 12500, 1280, "per-level")]
PYRAMID = ("pyramid_moments", "pyramid_finalize", "pyramid_merge")


@pytest.mark.parametrize("D,T,frames,path", INFER, ids=["d%d-L%d-%s" % (d, f, p) for d, _, f, p in INFER])
@pytest.mark.parametrize("variant", ["improved", "groupcomm"])
def test_inference_at_depth_7_and_8(variant, D, T, frames, path):
    """Batch 3, rows at three levels.  The dispatch, from the in-library trace of a single-stream forward: one fused pyramid per
    block -- with the tiled form's own stats_finalize launch, or without it on the block-per-row form -- or, at 1280 frames,
    which srf_pyramid refuses at depth 8, D depthwise launches and one merge per block."""
    from sudo_rm_rf_amd import ops
    cfg = _config(variant, D)
    U = cfg.num_blocks
    sd = weights.make_state_dict(cfg, seed=70 + D)
    wav = weights.make_mixture(3, T, seed=80 + D) * np.array([0.3, 1.0, 3.0], dtype=np.float32)[:, None, None]
    want = np_oracle.forward(cfg, sd, wav, dtype=np.float64)
    model = build(cfg, sd)
    eng = model._engine()
    eng.multi_stream = False
    x = torch.from_numpy(wav).to(DEV)
    plan = eng.plan_for(3, T, torch.device(DEV))
    assert plan.frames == frames == cfg.frames(T)
    with torch.no_grad(), ops.kernel_trace(DEV) as tr:
        out = model(x)
    torch.cuda.synchronize()
    names = [n for n, _ in tr.launches]
    count = lambda n: names.count(n)
    levels = sum(1 for n in names if n.startswith("dwconv5"))
    merges = sum(1 for n in names if n.startswith("merge"))
    if path == "per-level":
        assert not any(n.startswith("pyramid") or n == "stats_finalize" for n in names), names
        assert (levels, merges) == (U * D, U), names
    else:
        assert [count(n) for n in PYRAMID] == [U, U, U] and (levels, merges) == (0, 0), names
        assert count("stats_finalize") == (U if path == "lds-tiles" else 0), names
    err = np.abs(out.cpu().numpy().astype(np.float64) - want).reshape(3, -1).max(1)
    print("deep %s D=%d L=%d %s: max abs err per row %s (bar %.0e), max|ref| per row %s" %
          (variant, D, frames, path, ["%.2e" % e for e in err], TOL, ["%.2f" % v for v in np.abs(want).reshape(3, -1).max(1)]))
    assert out.shape == want.shape and (err <= TOL).all(), err


# ---- training --------------------------------------------------------------------------------------------------------------------
# (fixture, kernel mode, debug flags)
TRAIN = [("train_tiny_improved_d7", 0, 0), ("train_tiny_improved_d7", 1, 0),
         ("train_tiny_improved_d8", 0, 0), ("train_tiny_improved_d8", 1, 0), ("train_tiny_improved_d8", 0, DebugFlag.BWD_NO_FUSED_HEAD),
         ("train_tiny_groupcomm_d7", 0, 0), ("train_tiny_groupcomm_d7", 1, 0)]
# L / 2^D: even, odd, odd.  Odd: the deepest level's input has 4 * odd frames, Lin % 8 == 4, which srf_dwconv5_bwd_form sends
# to the chunked kernel while the other levels stay on the row kernels.
TRAIN_FRAMES = {"train_tiny_improved_d7": (512, 4), "train_tiny_improved_d8": (768, 3), "train_tiny_groupcomm_d7": (384, 3)}
HEAD = ("bwd_l0p_reduce", "bwd_l0p_apply", "bwd_l1h")


@pytest.mark.parametrize("name,mode,flags", TRAIN, ids=["%s-mode%d-flags%d" % (n, m, int(f)) for n, m, f in TRAIN])
def test_training_step_at_depth_7_and_8(name, mode, flags):
    """The runner's step against the reference's own gradients, the gradient with respect to the input waveform included, at
    the bars of the tiny fixtures (tests/test_gpu_train.py: 2e-4 of a tensor's largest entry, loss within 1e-3)."""
    import sudo_rm_rf.dnn.experiments.utils.mixture_consistency as mixture_consistency
    import sudo_rm_rf.dnn.losses.sisdr as sisdr_lib
    from sudo_rm_rf_amd import ops
    from test_gpu_train import build as build_train
    from test_oracle_golden import check_grads_against_golden, train_case
    cfg, sd, mix, tgt, z = train_case(name)
    D, U = cfg.upsampling_depth, cfg.num_blocks
    L, ratio = TRAIN_FRAMES[name]
    assert cfg.frames(mix.shape[-1]) == L and L == ratio << D and D in (7, 8)
    model = build_train(cfg, sd).train()
    loss_fn = sisdr_lib.PITLossWrapper(sisdr_lib.PairwiseNegSDR("sisdr"), pit_from='pw_mtx')
    x = mix.to(DEV).requires_grad_()
    try:
        ops.set_kernel_mode(mode)
        with ops.debug_flags(flags), ops.kernel_trace(DEV) as tr:
            rec = model(x)
            if cfg.variant == "groupcomm":
                rec = mixture_consistency.apply(rec, x)
            l = torch.clamp(loss_fn(rec, tgt.to(DEV)), min=-30., max=+30.)
            l.backward()
        torch.cuda.synchronize()
    finally:
        ops.set_kernel_mode(0)
    names = [n for n, _ in tr.launches]
    assert model._engine().last_plan.frames == L
    # forward: no fused pyramid above depth 6 in training, every level a launch of its own
    assert not any(n.startswith("pyramid") for n in names), names
    assert sum(1 for n in names if n.startswith("dwconv5_s") or n == "dwconv5_generic") == U * D, names
    # backward: on the fast kernels the merge backward rides on gln_bwd_apply (no launch of its own, with or without the fused
    # head); the generic kernels (mode 1) run it stand-alone, which also shows that the trace would have named it
    if mode == 0:
        assert "merge_bwd" not in names and "gln_bwd_apply" in names, names
    else:
        assert "merge_bwd" in names, names
    if flags & DebugFlag.BWD_NO_FUSED_HEAD:
        assert not any(n in HEAD for n in names), names
    print("deep train %s mode %d flags %d: loss %.6f (golden %.6f); backward families: %s" %
          (name, mode, int(flags), l.item(), float(z["loss"]), sorted({n for n in names if "bwd" in n})))
    assert abs(l.item() - float(z["loss"])) <= 1e-3
    assert float(z["loss"]) < 29.0                                      # (not clamped: the gradients are not all zero)
    want = torch.from_numpy(z["gwav"])
    assert x.grad is not None and x.grad.shape == want.shape
    gerr = ((x.grad.cpu() - want).abs().max() / want.abs().max()).item()
    print("deep train %s mode %d flags %d: input gradient rel err %.3e (bar 2e-4)" % (name, mode, int(flags), gerr))
    assert gerr <= 2e-4
    check_grads_against_golden([(k, p.grad.cpu().numpy()) for k, p in model.state_dict(keep_vars=True).items()], z, 2e-4)
