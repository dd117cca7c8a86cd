"""Training the original SuDoRM-RF, host side: the new symbols, the size queries, the refusals of the two walks and of the six
kernel entry points (all before any launch), the opt-in flag, the fixtures' manifest, and the differentiable restatement
(tests/original_train_ref.forward) against the reference's stored forward outputs and gradients.  No GPU needed."""
import ctypes as C
import io
import pickle

import numpy as np
import pytest
import torch

from tests import original_fixtures as of
from tests import original_train_ref as otr

WALKS = ("srf_original_train_saved_bytes", "srf_original_train_scratch_bytes", "srf_original_forward_train", "srf_original_backward")
KERNELS = ("srf_gln_c_bwd", "srf_softmax_mask_bwd", "srf_mask_weight_fold", "srf_decoder_weight_contract", "srf_decoder_bias_grad",
           "srf_relu_gate")


def _model(cfg):
    from sudo_rm_rf_amd.dnn.models.sudormrf import SuDORMRF
    return SuDORMRF(**cfg)


def _plan(cfg, batch, T, variant="original"):
    from sudo_rm_rf_amd.engine import Plan
    tup = (variant, 1, cfg["out_channels"], cfg["in_channels"], cfg["num_blocks"], cfg["upsampling_depth"], cfg["enc_kernel_size"],
           cfg["enc_num_basis"], cfg["num_sources"], 1)
    return Plan(tup, batch, T, torch.device("cpu"))


def test_symbols_exist():
    from sudo_rm_rf_amd import _lib
    lib = _lib.load()
    for name in WALKS + KERNELS + ("srf_gln_c_bwd_scratch_bytes", "srf_decoder_bias_grad_scratch_floats", "srf_perm_inv_sisdr_backward"):
        assert name in _lib.EXPORTED_SYMBOLS and getattr(lib, name) is not None, name
    assert lib.srf_abi_version() == _lib.ABI_VERSION


@pytest.mark.parametrize("name", sorted(otr.GRAD_CASES))
def test_size_queries(name):
    """Positive for every golden plan, and the saved layout is the one DESIGN.md 18.1 gives: statistics | s | x_0 .. x_U | per
    block y1, the D levels, m, g, g + x | reshape_before_masks' output (B != N) | z, every slice 256-byte aligned."""
    from sudo_rm_rf_amd import _lib
    lib = _lib.load()
    cfg, batch, T, _ = otr.GRAD_CASES[name]
    p = _plan(cfg, batch, T)
    saved, scratch = lib.srf_original_train_saved_bytes(p.handle), lib.srf_original_train_scratch_bytes(p.handle)
    assert saved > 0 and scratch > 0 and saved % 256 == 0 and scratch % 256 == 0
    assert p.train_sizes() == (saved, scratch)
    B, C_, U, D, K, N, S = (cfg[f] for f in of.FIELDS)
    L = p.frames
    assert L == of.frames(cfg, T)
    al = lambda nbytes: -(-nbytes // 256) * 256
    stats = (1 + U * (D + 4)) * batch * _lib.STAT_BUCKETS * 2 * 8
    per_block = 2 * al(4 * batch * C_ * L) + sum(al(4 * batch * C_ * (L >> k)) for k in range(D)) + 2 * al(4 * batch * B * L)
    want = al(stats) + al(4 * batch * N * L) + (U + 1) * al(4 * batch * B * L) + U * per_block + \
        (al(4 * batch * N * L) if B != N else 0) + al(4 * batch * S * N * L)
    assert saved == want


def test_size_queries_are_zero_for_other_plans():
    from sudo_rm_rf_amd import _lib
    lib = _lib.load()
    other = _plan(of.TINY, 1, 1000, variant="improved")
    assert lib.srf_original_train_saved_bytes(other.handle) == 0 and lib.srf_original_train_scratch_bytes(other.handle) == 0
    assert lib.srf_original_train_saved_bytes(None) == 0 and lib.srf_original_train_scratch_bytes(None) == 0
    # ... and the general training entry points keep refusing the original plan
    p = _plan(of.TINY, 2, 1000)
    assert lib.srf_train_saved_bytes(p.handle) == 0 and lib.srf_train_scratch_bytes(p.handle) == 0
    assert lib.srf_forward_train(p.handle, None, 0, None, None, None, 0, None, 0, None) == -1 and b"original" in lib.srf_last_error()


def test_walks_refuse_before_any_launch():
    from sudo_rm_rf_amd import _lib
    lib = _lib.load()
    orig = _plan(of.TINY, 1, 1000)
    other = _plan(of.TINY, 1, 1000, variant="improved")
    saved, scratch = orig.train_sizes()
    n = orig.num_params
    assert n == len(of.schema(of.TINY))
    fake = C.c_void_p(256)
    tab = (C.c_void_p * n)(*[256] * n)
    holes = (C.c_void_p * n)(*([256] * (n - 3) + [None, 256, 256]))          # a live gradient missing
    no_mask_in = (C.c_void_p * n)(*([256] * (n - 2) + [None, None]))        # ln_mask_in.*: allowed, checked below
    fwd, bwd = lib.srf_original_forward_train, lib.srf_original_backward
    cases = [
        (fwd, (other.handle, tab, n, fake, fake, fake, saved, fake, scratch, None), b"original plans only"),
        (bwd, (other.handle, tab, tab, n, fake, fake, fake, saved, fake, scratch, None), b"original plans only"),
        (fwd, (None, tab, n, fake, fake, fake, saved, fake, scratch, None), b"null plan"),
        (bwd, (None, tab, tab, n, fake, fake, fake, saved, fake, scratch, None), b"null plan"),
        (fwd, (orig.handle, None, n, fake, fake, fake, saved, fake, scratch, None), b"null"),
        (fwd, (orig.handle, tab, n, None, fake, fake, saved, fake, scratch, None), b"null"),
        (fwd, (orig.handle, tab, n, fake, None, fake, saved, fake, scratch, None), b"null"),
        (fwd, (orig.handle, tab, n, fake, fake, None, saved, fake, scratch, None), b"null"),
        (fwd, (orig.handle, tab, n, fake, fake, fake, saved, None, scratch, None), b"null"),
        (bwd, (orig.handle, tab, None, n, fake, fake, fake, saved, fake, scratch, None), b"null"),
        (bwd, (orig.handle, tab, tab, n, fake, None, fake, saved, fake, scratch, None), b"null"),
        (bwd, (orig.handle, tab, tab, n, None, fake, fake, saved, fake, scratch, None), b"null"),
        (bwd, (orig.handle, tab, holes, n, fake, fake, fake, saved, fake, scratch, None), b"gradient %d is null" % (n - 3)),
        (fwd, (orig.handle, no_mask_in, n, fake, fake, fake, saved, fake, scratch, None), b"parameter %d is null" % (n - 2)),
        (fwd, (orig.handle, tab, n - 1, fake, fake, fake, saved, fake, scratch, None), b"parameter tensors"),
        (bwd, (orig.handle, tab, tab, n + 1, fake, fake, fake, saved, fake, scratch, None), b"parameter tensors"),
        (fwd, (orig.handle, tab, n, fake, fake, fake, saved - 1, fake, scratch, None), b"saved buffer too small"),
        (fwd, (orig.handle, tab, n, fake, fake, fake, saved, fake, scratch - 1, None), b"scratch buffer too small"),
        (bwd, (orig.handle, tab, tab, n, fake, fake, fake, saved - 1, fake, scratch, None), b"saved buffer too small"),
        (bwd, (orig.handle, tab, tab, n, fake, fake, fake, saved, fake, scratch - 1, None), b"scratch buffer too small"),
        (fwd, (orig.handle, tab, n, fake, fake, C.c_void_p(260), saved, fake, scratch, None), b"256-byte aligned"),
        (bwd, (orig.handle, tab, tab, n, fake, fake, fake, saved, C.c_void_p(384 + 64), scratch, None), b"256-byte aligned"),
        # (ln_mask_in's gradients may be missing: the call gets past them to the next check)
        (bwd, (orig.handle, tab, no_mask_in, n, fake, fake, fake, saved - 1, fake, scratch, None), b"saved buffer too small"),
    ]
    for fn, args, text in cases:
        assert fn(*args) == -1 and text in lib.srf_last_error(), (text, lib.srf_last_error())


def test_kernel_entries_refuse_null_and_misaligned_arguments():
    from sudo_rm_rf_amd import _lib
    lib = _lib.load()
    a, b, c, d, e = (C.c_void_p(4096 * i) for i in range(1, 6))
    odd = C.c_void_p(4096 + 2)          # not float-aligned
    off4 = C.c_void_p(4096 + 4)         # float-aligned, off the 16-byte grid
    err = lambda: lib.srf_last_error()
    nrm = _lib.srf_norm()
    nrm.sums, nrm.gamma, nrm.beta, nrm.prelu = 4096, 8192, 12288, None
    good = C.byref(nrm)
    glnc = lib.srf_gln_c_bwd
    assert lib.srf_gln_c_bwd_scratch_bytes(2, 5, 4500) == 4 * 4 * 2 * 5 * 3 and lib.srf_gln_c_bwd_scratch_bytes(0, 5, 7) == 0
    assert glnc(None, None, b, good, None, 2, 5, 7, d, 0, None, None, None, e, None) == -1 and b"null" in err()
    assert glnc(a, None, None, good, None, 2, 5, 7, d, 0, None, None, None, e, None) == -1 and b"null" in err()
    assert glnc(a, None, b, None, None, 2, 5, 7, d, 0, None, None, None, e, None) == -1 and b"null" in err()
    assert glnc(a, None, b, good, None, 2, 5, 7, None, 0, None, None, None, e, None) == -1 and b"null" in err()
    assert glnc(a, None, b, good, None, 2, 5, 7, d, 0, None, None, None, None, None) == -1 and b"null" in err()
    assert glnc(a, None, b, good, None, 2, 0, 7, d, 0, None, None, None, e, None) == -1 and b"bad sizes" in err()
    bad = _lib.srf_norm()
    bad.sums, bad.gamma, bad.beta, bad.prelu = 4096, None, 12288, None
    assert glnc(a, None, b, C.byref(bad), None, 2, 5, 7, d, 0, None, None, None, e, None) == -1 and b"gamma" in err()
    bad.sums, bad.gamma = 4096 + 8, 8192
    assert glnc(a, None, b, C.byref(bad), None, 2, 5, 7, d, 0, None, None, None, e, None) == -1 and b"norm.sums" in err()
    assert glnc(a, None, b, good, None, 2, 5, 7, d, 0, None, None, None, off4, None) == -1 and b"scratch" in err()
    for args in ((odd, None, b, d), (a, odd, b, d), (a, None, odd, d), (a, None, b, odd)):
        assert glnc(args[0], args[1], args[2], good, None, 2, 5, 7, args[3], 0, None, None, None, e, None) == -1
        assert b"float-aligned" in err()
    assert glnc(a, None, b, good, None, 2, 5, 7, d, 0, odd, None, None, e, None) == -1 and b"float-aligned" in err()
    smb = lib.srf_softmax_mask_bwd
    for hole in range(5):
        args = [a, b, c, d, e]
        args[hole] = None
        assert smb(*args, 0, 2, 2, 6, 37, None) == -1 and b"null" in err()
        args[hole] = odd
        assert smb(*args, 0, 2, 2, 6, 37, None) == -1 and b"float-aligned" in err()
    assert smb(a, b, c, d, e, 0, 2, 0, 6, 37, None) == -1 and b"num_sources" in err()
    assert smb(a, b, c, d, e, 0, 2, 17, 6, 37, None) == -1 and b"num_sources" in err()
    assert smb(a, b, c, d, e, 0, 0, 2, 6, 37, None) == -1 and b"bad sizes" in err()
    assert smb(a, b, c, a, e, 0, 2, 2, 6, 37, None) == -1 and b"gz must not be z" in err()
    assert smb(a, b, c, d, c, 0, 2, 2, 6, 37, None) == -1 and b"genc" in err()
    fold = lib.srf_mask_weight_fold
    for hole in range(4):
        args = [a, b, c, d]
        args[hole] = None
        assert fold(*args, 6, 2, None) == -1 and b"null" in err()
        args[hole] = odd
        assert fold(*args, 6, 2, None) == -1 and b"float-aligned" in err()
    assert fold(a, b, c, d, 7, 2, None) == -1 and b"even" in err()
    assert fold(a, b, c, d, 6, 0, None) == -1 and b"num_sources" in err()
    con = lib.srf_decoder_weight_contract
    assert con(None, b, 6, 2, 21, None) == -1 and b"null" in err()
    assert con(a, None, 6, 2, 21, None) == -1 and b"null" in err()
    assert con(odd, b, 6, 2, 21, None) == -1 and b"float-aligned" in err()
    assert con(a, b, 0, 2, 21, None) == -1 and b"bad sizes" in err()
    bg = lib.srf_decoder_bias_grad
    assert lib.srf_decoder_bias_grad_scratch_floats(3) > 0 and lib.srf_decoder_bias_grad_scratch_floats(0) == 0
    assert bg(None, b, 2, 2, 100, c, None) == -1 and b"null" in err()
    assert bg(a, None, 2, 2, 100, c, None) == -1 and b"null" in err()
    assert bg(a, b, 2, 2, 100, None, None) == -1 and b"null" in err()
    assert bg(a, odd, 2, 2, 100, c, None) == -1 and b"float-aligned" in err()
    assert bg(a, b, 2, 0, 100, c, None) == -1 and b"bad sizes" in err()
    pib = lib.srf_perm_inv_sisdr_backward
    assert pib(None, b, 2, 2, 100, 1, 1e-9, c, d, e, a, None) == -1 and b"null" in err()
    assert pib(a, b, 2, 2, 100, 1, 1e-9, c, d, None, e, None) == -1 and b"null" in err()
    assert pib(a, b, 2, 10, 100, 1, 1e-9, c, d, e, C.c_void_p(4096 * 6), None) == -1 and b"sources" in err()
    assert pib(a, b, 2, 2, 100, 1, 1e-9, c, d, e, a, None) == -1 and b"must not be" in err()
    assert pib(a, b, 2, 2, 100, 1, 1e-9, c, d, e, odd, None) == -1 and b"misaligned" in err()
    gate = lib.srf_relu_gate
    assert gate(None, b, 10, None) == -1 and b"null" in err()
    assert gate(a, None, 10, None) == -1 and b"null" in err()
    assert gate(a, odd, 10, None) == -1 and b"float-aligned" in err()
    assert gate(a, b, 0, None) == -1 and b"bad size" in err()
    assert gate(a, a, 10, None) == -1 and b"must not be s" in err()


def test_opt_in_flag_returns_self_toggles_and_is_not_pickled():
    from sudo_rm_rf_amd._lib import SrfError
    torch.manual_seed(3)
    m = _model(of.PICKLE)
    keys, blob = list(m.state_dict()), pickle.dumps(m)
    buf = io.BytesIO()
    torch.save(m, buf)
    assert m.enable_hip_training() is m and m.__dict__.get("_srf_hip_training") is True
    assert list(m.state_dict()) == keys and pickle.dumps(m) == blob
    buf2 = io.BytesIO()
    torch.save(m, buf2)
    assert buf2.getvalue() == buf.getvalue()
    assert "_srf_hip_training" not in pickle.loads(pickle.dumps(m)).__dict__
    x = torch.zeros(1, 1, 200)
    # opted in: autograd reaches the engine, which has no CPU path -- in train() and in eval() mode alike; a mixture that
    # requires grad is refused by name
    for mode in (m.train, m.eval):
        mode()
        with pytest.raises(SrfError, match="MI355X"):
            m(x)
        with pytest.raises(NotImplementedError, match="mixture"):
            m(torch.zeros(1, 1, 200, requires_grad=True))
    # the sub-module forwards are untouched: an MI355X tensor or nothing
    with pytest.raises(RuntimeError, match="MI355X only"):
        m.sm[0](torch.zeros(1, of.PICKLE["out_channels"], 8))
    assert m.enable_hip_training(False) is m and "_srf_hip_training" not in m.__dict__
    # without the flag the refusals read as they always did
    for fresh in (m, _model(of.PICKLE), pickle.loads(pickle.dumps(_model(of.PICKLE).enable_hip_training()))):
        for mode in (fresh.train, fresh.eval):
            mode()
            with pytest.raises(RuntimeError, match=r"inference forward only \(no backward kernels\): run it under torch\.no_grad\(\)"):
                fresh(x)
        with torch.no_grad(), pytest.raises(SrfError, match="MI355X"):
            fresh(x)


def test_manifest_matches_the_schema_and_the_case_table():
    man = otr.load_manifest()
    assert man["generator"] == "tools/make_golden_original_train.py"
    assert sorted(man["cases"]) == sorted(list(otr.GRAD_CASES) + list(otr.TRAJ_CASES))
    for name, (cfg, batch, T, kind) in otr.GRAD_CASES.items():
        c = man["cases"][name]
        assert c["config"] == cfg and (c["batch"], c["T"], c["bars"]) == (batch, T, kind) and c["frames"] == of.frames(cfg, T)
        assert [(k, tuple(s)) for k, s in c["schema"]] == of.schema(cfg)
        assert (c["weight_seed"], c["input_seed"], c["gout_seed"]) == (otr.WEIGHT_SEED, otr.INPUT_SEED, otr.GOUT_SEED)
        assert tuple(c["no_grad"]) == otr.NO_GRAD
        z = of.load_golden(name)
        live = [k for k, _ in of.schema(cfg) if k not in otr.NO_GRAD]
        assert sorted(z) == sorted(p + k for k in live for p in ("g:", "n:", "d:"))
        # the reference's own fp32 backward is inside the bars it sets for the HIP one
        tol, yard, _ = otr.GRAD_BARS[kind]
        assert c["ref_fp32_vs_fp64_worst"] <= (tol if yard == 0 else 1e-2)
    for name, (cfg, batch, T, wseed, dseed) in otr.TRAJ_CASES.items():
        c = man["cases"][name]
        assert c["config"] == cfg and (c["batch"], c["T"], c["weight_seed"], c["data_seed"]) == (batch, T, wseed, dseed)
        assert (c["steps"], c["lr"], c["clip_grad_norm"]) == (otr.TRAJ_STEPS, otr.TRAJ_LR, otr.TRAJ_CLIP)
        z = of.load_golden(name)
        assert len(z["losses"]) == otr.TRAJ_STEPS and sorted(k[2:] for k in z if k.startswith("w:")) == sorted(k for k, _ in of.schema(cfg))


@pytest.mark.parametrize("name", ["orig_tiny", "orig_s1", "orig_s3_k9"])
def test_differentiable_restatement_reproduces_the_reference_forward(name):
    cfg, _, _, wseed, _ = of.CASES[name]
    out = otr.forward(cfg, of.make_state_dict(cfg, wseed), of.make_input(name))
    assert float(np.abs(out.numpy() - of.load_golden(name)["out"]).max()) <= 1e-5


@pytest.mark.parametrize("name", [n for n in sorted(otr.GRAD_CASES) if otr.GRAD_CASES[n][3] == "tiny"])
def test_differentiable_restatement_reproduces_the_reference_gradients(name):
    """fp64 autograd over the restatement against the reference's fp64 gradients: both exact up to fp64 rounding and the float32
    storage of the fixture (2^-24 per entry), so 1e-6 of a tensor's largest entry is a wide bar.  ln_mask_in gets nothing."""
    from test_oracle_golden import check_grads_against_golden
    cfg, sd, x, gout = otr.grad_case(name)
    out, grads = otr.restatement_grads(cfg, sd, x, gout)
    assert out.shape == gout.shape and not any(k in grads for k in otr.NO_GRAD)
    check_grads_against_golden([(k, grads[k]) for k, _ in of.schema(cfg) if k not in otr.NO_GRAD], of.load_golden(name), 1e-6)


def test_toeplitz_index_is_the_map_of_the_fill():
    S, N = 3, 6
    w = np.arange(1.0, S * (N + 1) + 1).reshape(S, 1, N + 1, 1)
    tz, _ = of.toeplitz(w, np.zeros(S))
    idx = otr.toeplitz_index(S, N)
    assert idx.shape == (S * N, N) and np.array_equal(np.concatenate([[0.0], w.reshape(-1)])[idx], tz)
