"""Training the original SuDoRM-RF on the MI355X (opt-in, SuDORMRF.enable_hip_training): every gradient fixture of
tests/original_train_ref.py through the C ABI and through the module + autograd against the reference's stored gradients with the
project's bars, the training forward's output, accumulation and repeatability, three steps of run_sudormrf.py's loop body, the
recipe's channel counts on the packed GEMM paths against fp64 autograd over the restatement, one step inside a poisoned arena, and
the refusals."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import original_fixtures as of
from tests import original_train_ref as otr
from tests import placement as pl

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4          # the output bar of tests/test_gpu_original.py


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    from sudo_rm_rf_amd import _lib, ops
    _lib.load()
    ops.set_kernel_mode(0)
    ops.set_debug_flags(0)


def _model(cfg, sd, train=True):
    from sudo_rm_rf_amd.dnn.models.sudormrf import SuDORMRF
    m = SuDORMRF(**cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.to(DEV)
    return (m.train() if train else m.eval()).enable_hip_training()


def _config(cfg):
    from sudo_rm_rf_amd import _lib
    return _lib.srf_config(variant=_lib.VARIANT_ORIGINAL, in_audio_channels=1, out_channels=cfg["out_channels"],
                           in_channels=cfg["in_channels"], num_blocks=cfg["num_blocks"], upsampling_depth=cfg["upsampling_depth"],
                           enc_kernel_size=cfg["enc_kernel_size"], enc_num_basis=cfg["enc_num_basis"],
                           num_sources=cfg["num_sources"], group_size=1)


def _raw_step(cfg, sd, wav, gout, arena=None, backwards=1):
    """srf_original_plan_create + srf_original_forward_train + srf_original_backward through ctypes, the gradients zeroed first
    and ln_mask_in's entries NULL.  arena: every buffer inside it, off the 16-byte grid where the ABI allows, saved and scratch
    poisoned.  Returns (out, [(key, gradient)]) as numpy."""
    from sudo_rm_rf_amd import _lib
    lib = _lib.load()
    c = _config(cfg)
    batch, _, T = wav.shape
    h = C.c_void_p()
    _lib.check(lib.srf_original_plan_create(C.byref(c), batch, T, C.byref(h)), "srf_original_plan_create")
    try:
        keys = list(sd)
        n = len(keys)
        assert lib.srf_plan_num_params(h) == n
        saved_bytes, scratch_bytes = lib.srf_original_train_saved_bytes(h), lib.srf_original_train_scratch_bytes(h)
        if arena is None:
            params = [torch.from_numpy(v).to(DEV) for v in sd.values()]
            grads = [torch.zeros_like(p) for p in params[:-2]]
            x, go = torch.from_numpy(wav).to(DEV), gout.float().to(DEV)
            out = torch.full((batch, cfg["num_sources"], T), float("nan"), device=DEV)
            saved = torch.full((saved_bytes,), 0xFF, dtype=torch.uint8, device=DEV)
            scratch = torch.full((scratch_bytes,), 0xFF, dtype=torch.uint8, device=DEV)
        else:
            params = [arena.put(torch.from_numpy(v), shift_floats=(1, 3, 0, 2)[i % 4], name=k) for i, (k, v) in enumerate(sd.items())]
            grads = [arena.put(torch.zeros(v.shape), shift_floats=(3, 1, 2, 0)[i % 4], name="grad:" + k)
                     for i, (k, v) in enumerate(list(sd.items())[:-2])]
            x = arena.put(torch.from_numpy(wav), shift_floats=1, name="wav")
            go = arena.put(gout.float(), shift_floats=3, name="grad_out")
            out = arena.place((batch, cfg["num_sources"], T), shift_floats=3, name="out")
            saved = arena.place((saved_bytes,), torch.uint8, name="saved")          # poisoned: 0xFF throughout
            scratch = arena.place((scratch_bytes,), torch.uint8, name="scratch")
        assert saved.data_ptr() % 256 == 0 and scratch.data_ptr() % 256 == 0
        ptab = (C.c_void_p * n)(*[p.data_ptr() for p in params])
        gtab = (C.c_void_p * n)(*([g.data_ptr() for g in grads] + [None, None]))
        st = _lib.current_stream(torch.device(DEV))
        if arena is not None:       # refused calls first: nothing may be written
            assert lib.srf_original_forward_train(h, ptab, n, _lib.ptr(x), _lib.ptr(out), _lib.ptr(saved), saved_bytes - 1,
                                                  _lib.ptr(scratch), scratch_bytes, st) == -1
            assert lib.srf_original_backward(h, ptab, gtab, n - 1, _lib.ptr(x), _lib.ptr(go), _lib.ptr(saved), saved_bytes,
                                             _lib.ptr(scratch), scratch_bytes, st) == -1
            torch.cuda.synchronize()
            arena.check()
            for t in (out, saved, scratch):
                arena.assert_untouched(t)
        _lib.check(lib.srf_original_forward_train(h, ptab, n, _lib.ptr(x), _lib.ptr(out), _lib.ptr(saved), saved_bytes,
                                                  _lib.ptr(scratch), scratch_bytes, st), "srf_original_forward_train")
        if arena is not None:       # `scratch` may be reused by anything between the two calls
            torch.cuda.synchronize()
            scratch.fill_(0xFF)
        for _ in range(backwards):
            _lib.check(lib.srf_original_backward(h, ptab, gtab, n, _lib.ptr(x), _lib.ptr(go), _lib.ptr(saved), saved_bytes,
                                                 _lib.ptr(scratch), scratch_bytes, st), "srf_original_backward")
        torch.cuda.synchronize()
        if arena is not None:
            arena.check()                                        # no guard word changed
            arena.assert_written(out)
            for t in [out] + grads:
                arena.assert_clean(t)                            # no poison reached an output
        return out.cpu().numpy(), [(k, g.cpu().numpy()) for k, g in zip(keys, grads)]
    finally:
        lib.srf_plan_destroy(h)


def _check(name, grads, z):
    from test_oracle_golden import check_grads_against_golden
    tol, yard, flips = otr.GRAD_BARS[otr.GRAD_CASES[name][3]]
    check_grads_against_golden(grads, z, tol, fp32_yardstick=yard, flip_budget=flips)


@pytest.mark.parametrize("name", sorted(otr.GRAD_CASES))
def test_gradients_match_the_reference_through_the_c_abi(name):
    cfg, sd, x, gout = otr.grad_case(name)
    _, grads = _raw_step(cfg, sd, x, gout)
    assert [k for k, _ in grads] == [k for k, _ in of.schema(cfg)][:-2]
    _check(name, grads, of.load_golden(name))


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("name", sorted(otr.GRAD_CASES))
def test_gradients_match_the_reference_through_autograd(name, mode):
    """enable_hip_training() + autograd, in train() and in eval() mode (GroupNorm does not differ between them);
    ln_mask_in.* keeps .grad None, as under the reference's autograd."""
    cfg, sd, x, gout = otr.grad_case(name)
    m = _model(cfg, sd, train=mode == "train")
    out = m(torch.from_numpy(x).to(DEV))
    assert out.requires_grad and out.grad_fn is not None
    (out * gout.float().to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert m.ln_mask_in.weight.grad is None and m.ln_mask_in.bias.grad is None
    grads = otr.named_grads(m)
    assert [k for k, _ in grads] == [k for k, _ in of.schema(cfg)][:-2]
    _check(name, grads, of.load_golden(name))


@pytest.mark.parametrize("name", sorted(otr.FORWARD_TWINS))
def test_training_forward_output(name):
    """On the weights and the input of the forward golden that shares the case's config, batch and T: the training forward
    within 1e-4 of the reference's stored output and of the same model's inference forward."""
    twin = otr.FORWARD_TWINS[name]
    cfg, batch, T, wseed, _ = of.CASES[twin]
    assert (cfg, batch, T) == otr.GRAD_CASES[name][:3]
    m = _model(cfg, of.make_state_dict(cfg, wseed))
    x = torch.from_numpy(of.make_input(twin)).to(DEV)
    out = m(x)
    assert out.requires_grad
    with torch.no_grad():
        plain = m(x)
    gold = of.load_golden(twin)["out"]
    e1 = float(np.abs(out.detach().cpu().numpy() - gold).max())
    e2 = float((out.detach() - plain).abs().max())
    print("%s: training forward vs reference %.3e, vs the inference forward %.3e" % (name, e1, e2))
    assert e1 <= TOL and e2 <= TOL


def test_s3_k9_training_forward_output():
    """(the case without a twin: three examples where the forward golden has two) against the model's own inference forward"""
    cfg, sd, x, _ = otr.grad_case("orig_train_s3_k9")
    m = _model(cfg, sd)
    xd = torch.from_numpy(x).to(DEV)
    out = m(xd)
    with torch.no_grad():
        assert float((out.detach() - m(xd)).abs().max()) <= TOL


def test_backward_accumulates_repeats_and_refuses_input_gradients():
    """A second backward without zeroing doubles the gradients; two backwards over one saved step give the same bits wherever
    only this feature's kernels and the ordered weight-gradient GEMM produce them (decoder, mask layer) and the same values to
    1e-6 of a tensor's largest entry everywhere else (the GlobLN backward of the pyramid levels adds its example sums with fp64
    atomics, whose order is not fixed)."""
    cfg, sd, x, gout = otr.grad_case("orig_train_tiny")
    m = _model(cfg, sd)
    m._engine().keep_saved_for_repeat = True
    xd, g = torch.from_numpy(x).to(DEV), gout.float().to(DEV)
    loss = (m(xd) * g).sum()
    named = [(k, p) for k, p in m.state_dict(keep_vars=True).items() if k not in otr.NO_GRAD]
    params = [p for _, p in named]
    first = torch.autograd.grad(loss, params, retain_graph=True)
    second = torch.autograd.grad(loss, params)
    for (k, _), a, b in zip(named, first, second):
        if k.split(".")[0] in ("decoder", "m"):
            assert torch.equal(a, b), k
        assert float((a - b).abs().max()) <= 1e-6 * float(a.abs().max()), k
    m._engine().keep_saved_for_repeat = False
    for _ in range(2):
        (m(xd) * g).sum().backward()
    torch.cuda.synchronize()
    for (k, p), a in zip(named, first):
        assert float((p.grad - 2 * a).abs().max()) <= 2e-6 * float(a.abs().max()), k
    assert m.ln_mask_in.weight.grad is None
    # through the C ABI: two backwards into the same gradient buffers
    _, once = _raw_step(cfg, sd, x, gout)
    _, twice = _raw_step(cfg, sd, x, gout, backwards=2)
    for (k, a), (_, b) in zip(once, twice):
        assert float(np.abs(b - 2 * a).max()) <= 2e-6 * float(np.abs(a).max()), k
    with pytest.raises(NotImplementedError, match="mixture"):
        m(xd.clone().requires_grad_())
    # without autograd the opted-in model runs the inference path, bit for bit what a model that never opted in returns
    from sudo_rm_rf_amd.dnn.models.sudormrf import SuDORMRF
    plain = SuDORMRF(**cfg)
    plain.load_state_dict(m.state_dict())
    plain = plain.to(DEV).eval()
    with torch.no_grad():
        assert torch.equal(m(xd), plain(xd))


def test_refusals_without_the_opt_in_read_as_before():
    from sudo_rm_rf_amd.dnn.models.sudormrf import SuDORMRF
    cfg, sd, x, _ = otr.grad_case("orig_train_tiny")
    m = SuDORMRF(**cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.to(DEV)
    xd = torch.from_numpy(x).to(DEV)
    for mode in (m.eval, m.train):
        mode()
        with pytest.raises(RuntimeError, match=r"inference forward only \(no backward kernels\): run it under torch\.no_grad\(\)"):
            m(xd)
    m.enable_hip_training().enable_hip_training(False)
    with pytest.raises(RuntimeError, match=r"inference forward only"):
        m(xd)
    # the sub-module forwards never join the training step
    m.enable_hip_training()
    y = m.sm[0](torch.zeros(1, cfg["out_channels"], 8, device=DEV))
    assert not y.requires_grad


def test_training_trajectory_matches_reference_runner_loop():
    """Three steps of run_sudormrf.py's loop body -- its own loss, PermInvariantSISDR(zero_mean, backward_loss, improvement) with
    initial_mixtures, differentiated on HIP (srf_perm_inv_sisdr_backward) -- with the fused HIP clip + Adam step against the
    trajectory the reference itself produced; decoder.bias apart (tests/original_train_ref.TRAJ_NOISE_ONLY).  Measured: losses within 1.7e-5 dB, worst tensor
    sm.1.spp_dw.2.norm.bias at 0.32 of its bar, whole-model update 3.9e-5 (bar 2e-3).  That tensor has an entry whose clipped
    first-step gradient (4.0e-8) lies inside Adam's eps, where the step follows the gradient's size: it is what made the walk keep
    the decoder's frame GEMMs and every GEMM launch without a packed image in the exact-fp32 class."""
    import sudo_rm_rf.dnn.losses.sisdr as sisdr_lib
    from sudo_rm_rf_amd import optim
    from test_oracle_golden import check_trajectory_against_golden
    name = "orig_train_traj"
    cfg, batch, T, wseed, dseed = otr.TRAJ_CASES[name]
    c, z = otr.load_manifest()["cases"][name], of.load_golden(name)
    sd = of.make_state_dict(cfg, wseed)
    model = _model(cfg, sd)
    opt = optim.FusedClipAdam(model.parameters(), lr=c["lr"], clip_grad_norm=c["clip_grad_norm"])
    back_loss_tr_loss = sisdr_lib.PermInvariantSISDR(batch_size=batch, n_sources=cfg["num_sources"], zero_mean=True, backward_loss=True,
                                          improvement=True)
    losses = []
    for mix, clean in otr.make_traj_batches(batch, cfg["num_sources"], T, dseed):
        opt.zero_grad()
        m1wavs, clean_wavs = mix.to(DEV), clean.to(DEV)
        rec_sources_wavs = model(m1wavs)
        l = back_loss_tr_loss(rec_sources_wavs, clean_wavs, initial_mixtures=m1wavs)
        l.backward()
        opt.step()
        losses.append(l.item())
    print(name, "losses", losses, "reference", list(z["losses"]))
    final = [(k, p.detach().cpu().numpy()) for k, p in model.state_dict(keep_vars=True).items()]
    for k, w in final:
        if k in otr.TRAJ_NOISE_ONLY:      # a zero gradient's rounding noise: at most Adam's full step per step (original_train_ref.py)
            assert float(np.abs(w - sd[k]).max()) <= otr.TRAJ_STEPS * c["lr"] * 1.001, k
        if k in otr.NO_GRAD:
            assert np.array_equal(w, sd[k]), k
    check_trajectory_against_golden([(k, w) for k, w in final if k not in otr.TRAJ_NOISE_ONLY], sd, losses, z, otr.TRAJ_TOL)


@functools.lru_cache(maxsize=None)
def _wide_reference(nb):
    """fp64 and fp32 autograd over the restatement for the wide case, in slices of 8 examples (the loss is a sum over examples),
    as a golden-shaped dict for check_grads_against_golden: every entry stored (stride 1), "d:" the restatement's own fp32
    deviation from fp64."""
    cfg = of.WIDE
    sd = of.make_state_dict(cfg, of.WIDE_WSEED)
    wav = of.make_distinct(nb, of.WIDE_T, of.WIDE_INPUT_SEED)
    gout = otr.make_gout((nb, cfg["num_sources"], of.WIDE_T))
    acc = {}
    for dt in (torch.float64, torch.float32):
        tot = None
        for b0 in range(0, nb, 8):
            _, g = otr.restatement_grads(cfg, sd, wav[b0:b0 + 8], gout[b0:b0 + 8], dt)
            tot = g if tot is None else {k: tot[k] + g[k] for k in g}
        acc[dt] = tot
    z = {}
    for k, g in acc[torch.float64].items():
        gmax = float(np.abs(g).max())
        z["g:" + k] = g.reshape(-1)
        z["n:" + k] = np.array([1, gmax, float(g.sum()), float((g ** 2).sum())])
        z["d:" + k] = np.float64(np.abs(acc[torch.float32][k] - g).max() / max(gmax, 1e-300))
    return cfg, sd, wav, gout, z


def test_wide_configuration_trains_on_the_packed_gemm_paths():
    """The recipe's channel counts (256 / 512 / N 512, U 2, D 3, 512 frames) at ceil(CUs / 4) examples: the training forward's 1x1
    convolutions run the 256 x 128 kernel from their exact-class images, the backward's data-gradient GEMMs from the packed
    transposes (the Toeplitz weight's among them), asserted from the trace; gradients against fp64 autograd over the
    restatement on the host with the bars of the default-shape fixtures."""
    from sudo_rm_rf_amd import ops
    from test_oracle_golden import check_grads_against_golden
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nb = -(-cus // of.WIDE_MIN_TILES)
    cfg, sd, wav, gout, z = _wide_reference(nb)
    U = cfg["num_blocks"]
    m = _model(cfg, sd)
    with ops.kernel_trace(DEV) as tr:
        out = m(torch.from_numpy(wav).to(DEV))
    torch.cuda.synchronize()
    fwd = [n for n, _ in tr.launches]
    with ops.kernel_trace(DEV) as tr:
        (out * gout.float().to(DEV)).sum().backward()
    torch.cuda.synchronize()
    bwd = [n for n, _ in tr.launches]
    print("wide: batch %d on %d CUs\nforward: %s\nbackward: %s" % (nb, cus, fwd, bwd))
    # forward: l1 (GlobLN on load) | per block proj_1x1, conv_1x1_exp | reshape_before_masks | the mask GEMM: the 256 x 128 kernel on
    # THREE bf16 parts per operand (24 mantissa bits; not the two-fp16-part form srf_forward_train defaults to), from ONE pack
    # launch; every other GEMM is the decoder's
    exact = [n for n in fwd if n.startswith("pw_conv_x3w")]
    assert exact == ["pw_conv_x3w3<1>"] + ["pw_conv_x3w3<0>"] * (2 * U + 2) and fwd.count("pack_pw_weights3") == 1, fwd
    assert sum(n.startswith("pw_conv") for n in fwd) == len(exact) + 1
    assert fwd.count("gln_apply_c") == 4 * U and fwd.count("softmax_mask") == 1 and fwd[-1] == "bias_rescale"
    assert sum(n.startswith("dwconv5") for n in fwd) == U * cfg["upsampling_depth"] and fwd.count("merge_fast") == U
    big = lambda n: n.startswith("pw_conv_x3p<") or n.startswith("pw_conv_x3w<")
    # backward: the mask GEMM's, reshape_before_masks', per block conv_1x1_exp's and proj_1x1's, and l1's data gradients
    assert sum(big(n) for n in bwd) == 2 + 2 * U + 1 and "pack_pw_weights" in bwd, bwd
    assert not any(n.startswith("transpose") for n in bwd)
    assert bwd.count("gln_c_bwd_reduce") == bwd.count("gln_c_bwd_apply") == 4 * U and bwd.count("gln_apply_c") == 2 * U
    assert bwd.count("softmax_mask_bwd") == bwd.count("mask_weight_fold") == bwd.count("decoder_weight_contract") == 1
    assert bwd.count("relu_gate") == bwd.count("decoder_bias_fold") == 1
    grads = otr.named_grads(m)
    assert [k for k, _ in grads] == [k for k, _ in of.schema(cfg)][:-2]
    tol, yard, flips = otr.GRAD_BARS["default"]
    check_grads_against_golden(grads, z, tol, fp32_yardstick=yard, flip_budget=flips)


def test_one_step_inside_a_guarded_arena():
    """One forward-train + backward at TINY with parameters, gradients, saved, scratch, wav, grad_out and out inside a poisoned
    arena: no guard word changes, no poison reaches an output, refused calls write nothing; and the gradients are the
    fixture's."""
    cfg, sd, x, gout = otr.grad_case("orig_train_tiny")
    from sudo_rm_rf_amd import _lib
    p_bytes = sum(v.nbytes for v in sd.values())
    lib = _lib.load()
    h = C.c_void_p()
    c = _config(cfg)
    _lib.check(lib.srf_original_plan_create(C.byref(c), x.shape[0], x.shape[2], C.byref(h)), "srf_original_plan_create")
    need = lib.srf_original_train_saved_bytes(h) + lib.srf_original_train_scratch_bytes(h)
    lib.srf_plan_destroy(h)
    a = pl.Arena(DEV, need + 2 * p_bytes + (16 << 20))
    out, grads = _raw_step(cfg, sd, x, gout, arena=a)
    gold = of.load_golden("orig_tiny")["out"]
    assert out.shape == gold.shape and np.isfinite(out).all()
    _check("orig_train_tiny", grads, of.load_golden("orig_train_tiny"))
