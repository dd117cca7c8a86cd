"""Training the causal SuDoRM-RF (v3), host side: the fp64 restatement (tests/causal_train_ref.py) against the gradients and
the FUSS trajectory the REFERENCE produced (tools/make_golden_causal_train.py), the opt-in flag, and the refusals of the new
entry points.  No GPU needed."""
import ctypes as C
import io
import pickle

import numpy as np
import pytest
import torch

from tests import causal_fixtures as cf
from tests import causal_train_ref as ctr
from tests import fuss_fixtures as ff


def _model(cfg):
    from sudo_rm_rf_amd.dnn.models.causal_improved_sudormrf_v3 import CausalSuDORMRF
    return CausalSuDORMRF(**cfg)


def _plan(variant, cfg, batch, T):
    from sudo_rm_rf_amd.engine import Plan
    return Plan((variant,) + tuple(cfg[f] for f in cf.FIELDS) + (1,), batch, T, torch.device("cpu"))


@pytest.mark.parametrize("name", sorted(ctr.GRAD_CASES))
def test_restatement_reproduces_the_reference_gradients(name):
    """fp64 autograd over the restatement against the reference's fp64 gradients: both are exact up to fp64 rounding and the
    float32 storage of the fixture (2^-24 per entry), so 1e-6 of a tensor's largest entry is a wide bar."""
    from test_oracle_golden import check_grads_against_golden
    man = ctr.load_manifest()["cases"][name]
    cfg, sd, x, gout = ctr.grad_case(name)
    assert man["config"] == cfg and (man["batch"], man["T"]) == ctr.GRAD_CASES[name][1:3]
    z = cf.load_golden(name)
    out, grads = ctr.linear_loss_grads(cfg, sd, x, gout)
    assert out.shape == gout.shape
    check_grads_against_golden([(k, grads[k]) for k, _ in cf.schema(cfg)], z, 1e-6)
    K = cfg["enc_kernel_size"]
    assert not grads["encoder.weight"][..., K:].any()
    assert not any(g[..., 11:].any() for k, g in grads.items() if ".spp_dw." in k and k.endswith("conv.weight"))


def test_restatement_reproduces_the_reference_trajectory():
    from test_oracle_golden import check_trajectory_against_golden
    name = "causal_fuss_s4_traj"
    cfg, batch, T, wseed, dseed = ctr.TRAJ_CASES[name]
    man, z = ctr.load_manifest()["cases"][name], cf.load_golden(name)
    assert man["config"] == cfg and man["steps"] == ff.TRAJ_STEPS == len(z["losses"])
    sd = cf.make_state_dict(cfg, wseed)
    losses, final = ctr.fuss_trajectory(cfg, sd, ff.make_traj_batches(batch, 4, T, dseed))
    assert np.abs(np.array(losses) - z["losses"]).max() <= 1e-8 * max(1.0, np.abs(z["losses"]).max())
    check_trajectory_against_golden([(k, final[k]) for k, _ in cf.schema(cfg)], sd, losses, z, 1e-6, yardstick=0.0)


def test_opt_in_flag_is_not_state_and_a_fresh_model_still_refuses():
    torch.manual_seed(3)
    m = _model(cf.TINY)
    keys, blob = list(m.state_dict()), pickle.dumps(m)
    buf = io.BytesIO()
    torch.save(m, buf)
    assert m.enable_hip_training() is m
    assert list(m.state_dict()) == keys and pickle.dumps(m) == blob
    buf2 = io.BytesIO()
    torch.save(m, buf2)
    assert buf2.getvalue() == buf.getvalue()
    assert "_srf_hip_training" not in pickle.loads(pickle.dumps(m)).__dict__
    # opted in: autograd reaches the engine, which has no CPU path; a mixture that requires grad is refused by name
    from sudo_rm_rf_amd._lib import SrfError
    with pytest.raises(SrfError, match="MI355X"):
        m(torch.zeros(1, 1, 200))
    with pytest.raises(NotImplementedError, match="mixture"):
        m(torch.zeros(1, 1, 200, requires_grad=True))
    # sub-modules, streams and pools keep refusing; opting out restores the refusal of the model itself
    for what in (lambda: m.sm[0](torch.zeros(1, 32, 8)), lambda: m.stream(), lambda: m.stream_pool(2)):
        with pytest.raises(NotImplementedError, match="forward-only"):
            what()
    m.enable_hip_training(False)
    assert "_srf_hip_training" not in m.__dict__
    for fresh in (m, _model(cf.TINY), pickle.loads(pickle.dumps(_model(cf.TINY).enable_hip_training()))):
        with pytest.raises(NotImplementedError, match="forward-only"):
            fresh(torch.zeros(1, 1, 200))


def test_new_entry_points_refuse_before_any_launch():
    from sudo_rm_rf_amd import _lib
    lib = _lib.load()
    causal = _plan("causal", cf.TINY, 1, 1000)
    other = _plan("improved", dict(cf.TINY, in_audio_channels=1), 1, 1000)
    saved, scratch = lib.srf_causal_train_saved_bytes(causal.handle), lib.srf_causal_train_scratch_bytes(causal.handle)
    assert saved > 0 and scratch > 0 and saved % 256 == 0
    assert lib.srf_train_saved_bytes(causal.handle) == 0 and lib.srf_train_scratch_bytes(causal.handle) == 0
    assert lib.srf_causal_train_saved_bytes(other.handle) == 0 and lib.srf_causal_train_scratch_bytes(other.handle) == 0
    assert lib.srf_causal_train_saved_bytes(None) == 0
    # the saved layout of DESIGN.md 11.1: enc | x_0..x_U | per block u, d_k, merged | m, every slice 256-byte aligned
    A, B, Cc, U, D, K, N, S = (cf.TINY[f] for f in cf.FIELDS)
    L = causal.frames
    al = lambda n: -(-4 * n // 256) * 256
    assert saved == al(N * L) + (U + 1) * al(B * L) + U * (2 * al(Cc * L) + sum(al(Cc * (L >> k)) for k in range(D))) + al(S * A * N * L)
    n = causal.num_params
    fake = C.c_void_p(256)
    tab = (C.c_void_p * n)(*[256] * n)
    fwd, bwd = lib.srf_causal_forward_train, lib.srf_causal_backward
    cases = [
        (fwd, (other.handle, tab, n, fake, fake, fake, saved, fake, scratch, None), b"causal"),
        (bwd, (other.handle, tab, tab, n, fake, fake, fake, saved, fake, scratch, None), b"causal"),
        (fwd, (None, tab, n, fake, fake, fake, saved, fake, scratch, None), b"null"),
        (fwd, (causal.handle, None, n, fake, fake, fake, saved, fake, scratch, None), b"null"),
        (fwd, (causal.handle, tab, n, None, fake, fake, saved, fake, scratch, None), b"null"),
        (fwd, (causal.handle, tab, n, fake, fake, None, saved, fake, scratch, None), b"null"),
        (bwd, (causal.handle, tab, None, n, fake, fake, fake, saved, fake, scratch, None), b"null"),
        (bwd, (causal.handle, tab, tab, n, fake, None, fake, saved, fake, scratch, None), b"null"),
        (fwd, (causal.handle, tab, n - 1, fake, fake, fake, saved, fake, scratch, None), b"parameter tensors"),
        (bwd, (causal.handle, tab, tab, n + 1, fake, fake, fake, saved, fake, scratch, None), b"parameter tensors"),
        (fwd, (causal.handle, tab, n, fake, fake, fake, saved - 1, fake, scratch, None), b"too small"),
        (fwd, (causal.handle, tab, n, fake, fake, fake, saved, fake, scratch - 1, None), b"too small"),
        (bwd, (causal.handle, tab, tab, n, fake, fake, fake, saved - 1, fake, scratch, None), b"too small"),
        (bwd, (causal.handle, tab, tab, n, fake, fake, fake, saved, fake, scratch - 1, None), b"too small"),
        (fwd, (causal.handle, tab, n, fake, fake, C.c_void_p(260), saved, fake, scratch, None), b"aligned"),
    ]
    for fn, args, text in cases:
        assert fn(*args) == -1 and text in lib.srf_last_error(), (args, lib.srf_last_error())
    # kernel level: null pointers, bad shapes and aliasing are refused too
    ptrs = (C.c_void_p * 8)(*[256] * 8)
    assert lib.srf_causal_pyramid_bwd_tile() % (1 << 7) == 0
    assert lib.srf_causal_pyramid_bwd_supported(5, 24, 3) == 1 and lib.srf_causal_pyramid_bwd_supported(5, 22, 3) == 0
    assert lib.srf_causal_pyramid_bwd_supported(5, 24, 9) == 0 and lib.srf_causal_pyramid_bwd_scratch_bytes(2, 5, 22, 3) == 0
    assert lib.srf_causal_pyramid_bwd_scratch_bytes(2, 5, 24, 3) > 0 and lib.srf_causal_dwconv_bwd_scratch_bytes(2, 5, 24) > 0
    pyr = lib.srf_causal_pyramid_bwd
    assert pyr(None, fake, ptrs, fake, ptrs, ptrs, fake, ptrs, ptrs, ptrs, fake, 2, 5, 24, 3, fake, None) == -1
    assert pyr(fake, fake, ptrs, fake, ptrs, ptrs, C.c_void_p(512), ptrs, ptrs, ptrs, fake, 2, 5, 22, 3, fake, None) == -1
    assert b"not supported" in lib.srf_last_error()
    assert pyr(fake, fake, ptrs, fake, ptrs, ptrs, fake, ptrs, ptrs, ptrs, fake, 2, 5, 24, 3, fake, None) == -1
    assert b"alias" in lib.srf_last_error()
    dwb = lib.srf_causal_dwconv_bwd
    a, b_, c_, d_ = (C.c_void_p(256 * i) for i in range(1, 5))
    assert dwb(a, 0, None, None, 2, b_, fake, c_, fake, 1, None, fake, fake, fake, 2, 5, 24, fake, None) == -1
    assert dwb(None, 0, None, None, 2, b_, fake, c_, fake, 1, d_, fake, fake, fake, 2, 5, 24, fake, None) == -1
    assert dwb(a, 8, None, None, 2, b_, fake, c_, fake, 1, d_, fake, fake, fake, 2, 5, 24, fake, None) == -1
    assert dwb(a, 1, a, fake, 2, b_, fake, c_, fake, 2, d_, fake, fake, fake, 2, 5, 23, fake, None) == -1
    assert dwb(a, 0, None, None, 2, b_, fake, c_, fake, 3, d_, fake, fake, fake, 2, 5, 24, fake, None) == -1
    assert dwb(a, 0, None, None, 2, b_, fake, None, None, 1, d_, fake, None, fake, 2, 5, 24, fake, None) == -1
    assert dwb(a, 0, None, None, 2, b_, fake, c_, fake, 1, a, fake, fake, fake, 2, 5, 24, fake, None) == -1
    assert b"alias" in lib.srf_last_error()
