"""Training the causal SuDoRM-RF (v3) on the MI355X (opt-in, CausalSuDORMRF.enable_hip_training): the pyramid-backward kernels
against autograd over the restatement (tests/causal_train_ref.py, pinned to the reference by tests/test_causal_train_host.py),
their operand placement, the model's gradients against the reference's (tests/golden/causal_train_*.npz), the train-mode
output, fresh models, block scales, three steps of the FUSS loop, determinism and accumulation."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import causal_fixtures as cf
from tests import causal_train_ref as ctr
from tests import fuss_fixtures as ff

pytestmark = pytest.mark.gpu
TOL = 1e-4          # the output bar of tests/test_gpu_causal.py
SMALL_TOL = 2e-4    # the gradient bar of the tiny fixtures, for the tiny cases that have no fixture


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


class _kernel_mode:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from sudo_rm_rf_amd import ops
        ops.set_kernel_mode(self.mode)

    def __exit__(self, *exc):
        from sudo_rm_rf_amd import ops
        ops.set_kernel_mode(0)
        return False


def _lib():
    from sudo_rm_rf_amd import _lib
    return _lib


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(dev):
    return _lib().current_stream(dev)


# ---- op level -------------------------------------------------------------------------------------------------------
def _tile():
    return _lib().load().srf_causal_pyramid_bwd_tile()


def _lengths(D):
    """Multiples of the granule q = 2^(D-1).  Up to D = 6 the last length is two tiles plus 11 granules; at D = 7 and 8 it is
    2432 (two tiles plus 6 and 3 granules: a third, partial tile whose frames lie inside the right halo, 10 * 2^(D-1) = 640 and
    1280 frames, of BOTH earlier tiles).  At D = 8 the list is 128 and 896 (below a tile), 1024, 1152 (a tile plus 128), 2432."""
    q, t = 1 << (D - 1), _tile()
    last = 2 * t + 11 * q if D <= 6 else 2432
    assert last % q == 0 and last > 2 * t
    return sorted({q, 8 * q, t - q, t, t + q, last})


_REF_CACHE = {}


def _pyr_reference(D, L):
    """Operands rounded to float32 (what the kernels see), fp64 autograd over the restatement on exactly those, torch's own
    float32 CPU autograd on the same case (the yardstick) and the float32 pre-activations d_k."""
    key = (D, L)
    if key not in _REF_CACHE:
        ops64 = [t for t in ctr.random_pyramid_case(2, 5, L, D, 100 * D + L % 97)]
        rnd = lambda t: [v.float().double() for v in t] if isinstance(t, list) else t.float().double()
        ops64 = [rnd(t) for t in ops64]
        ops32 = [[v.float() for v in t] if isinstance(t, list) else t.float() for t in ops64]
        u, a_p, ws, bs, slopes, gm = ops64
        ref = ctr.pyramid_grads(*ops64)
        f32 = ctr.pyramid_grads(*ops32)
        d = [v.float() for v in ctr.levels(u, a_p, ws, bs, slopes)]
        assert not any(v[0, 1].any() for v in d)          # row (0, 1): every pre-activation exactly 0
        _REF_CACHE[key] = (ops32, d, ref, f32)
    return _REF_CACHE[key]


def _run_per_level(lib, dev, u, a_p, ws, slopes, gm, d, out):
    Bt, Cc, L = u.shape
    D = len(ws)
    scratch = torch.empty(lib.srf_causal_dwconv_bwd_scratch_bytes(Bt, Cc, L), dtype=torch.uint8, device=dev)
    gd = [torch.empty_like(v) for v in d]
    for k in range(D - 1, -1, -1):
        rc = lib.srf_causal_dwconv_bwd(_p(gm), k, _p(gd[k + 1]) if k < D - 1 else None, _p(ws[k + 1]) if k < D - 1 else None, 2,
                                       _p(d[k]), _p(slopes[k]), _p(u if k == 0 else d[k - 1]), _p(a_p if k == 0 else slopes[k - 1]),
                                       1 if k == 0 else 2, _p(gd[k]), _p(out["dw"][k]), _p(out["db"][k]), _p(out["ds"][k]), Bt, Cc,
                                       L >> k, _p(scratch), _stream(dev))
        _lib().check(rc, "srf_causal_dwconv_bwd")
    rc = lib.srf_causal_dwconv_bwd(None, 0, _p(gd[0]), _p(ws[0]), 1, _p(u), _p(a_p), None, None, 1, _p(out["gu"]), None, None,
                                   _p(out["da_p"]), Bt, Cc, L, _p(scratch), _stream(dev))
    _lib().check(rc, "srf_causal_dwconv_bwd")


def _run_fused(lib, dev, u, a_p, ws, slopes, gm, d, out):
    Bt, Cc, L = u.shape
    D = len(ws)
    scratch = torch.empty(lib.srf_causal_pyramid_bwd_scratch_bytes(Bt, Cc, L, D), dtype=torch.uint8, device=dev)
    rc = lib.srf_causal_pyramid_bwd(_p(gm), _p(u), _ptrs(d), _p(a_p), _ptrs(ws), _ptrs(slopes), _p(out["gu"]), _ptrs(out["dw"]),
                                    _ptrs(out["db"]), _ptrs(out["ds"]), _p(out["da_p"]), Bt, Cc, L, D, _p(scratch), _stream(dev))
    _lib().check(rc, "srf_causal_pyramid_bwd")


def _outputs(dev, u, ws):
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    D = len(ws)
    return {"gu": nan(*u.shape), "da_p": nan(1), "dw": [nan(*w.shape) for w in ws], "db": [nan(w.shape[0]) for w in ws],
            "ds": [nan(1) for _ in range(D)]}


def _flat(out):
    return [out["gu"], out["da_p"]] + out["dw"] + out["db"] + out["ds"]


@pytest.mark.parametrize("D", [1, 3, 5, 6, 7, 8])
def test_pyramid_backward_kernels_match_autograd(dev, D):
    """Both forms on Bt = 2, C = 5 at every length where the fused kernel's tiling changes: a fraction of a tile, one tile less /
    exactly / more than a granule, and two tiles plus more than the deepest level's right halo.  One slope negative, one zero,
    one row whose pre-activations are all exactly 0, junk in the masked taps.  Bar per tensor, relative to its largest entry:
    max(1e-5, 4 x the error of torch's float32 CPU autograd on the same case)."""
    lib = _lib().load()
    for L in _lengths(D):
        ops32, d, ref, f32 = _pyr_reference(D, L)
        u, a_p, ws, bs, slopes, gm = [[v.to(dev) for v in t] if isinstance(t, list) else t.to(dev) for t in ops32]
        dd = [v.to(dev) for v in d]
        runs = {}
        for form, fn in (("per_level", _run_per_level), ("fused", _run_fused)):
            outs = []
            for _ in range(2):
                out = _outputs(dev, u, ws)
                fn(lib, dev, u, a_p, ws, slopes, gm, dd, out)
                outs.append(out)
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(_flat(outs[0]), _flat(outs[1]))), (form, L, "second run differs")
            runs[form] = outs[0]
            named = [("gu", out["gu"], ref["gu"], f32["gu"]), ("da_p", out["da_p"], ref["da_p"], f32["da_p"])]
            for k in range(D):
                named += [("dw%d" % k, out["dw"][k], ref["dw"][k], f32["dw"][k]), ("db%d" % k, out["db"][k], ref["db"][k], f32["db"][k]),
                          ("ds%d" % k, out["ds"][k], ref["ds"][k], f32["ds"][k])]
                assert not out["dw"][k][..., 11:].any(), (form, L, k, "masked taps")
            worst = ("", 0.0, 0.0)
            for name, got, want, yard in named:
                scale = max(float(want.abs().max()), 1e-30)
                err = float((got.cpu().double() - want).abs().max()) / scale
                bar = max(1e-5, 4.0 * float((yard.double() - want).abs().max()) / scale)
                if err / bar >= worst[1] / max(worst[2], 1e-30):
                    worst = (name, err, bar)
                assert err <= bar, (form, D, L, name, err, bar)
            print("D=%d L=%d %-9s worst %s: %.2e (bar %.1e)" % (D, L, form, worst[0], worst[1], worst[2]))
        assert torch.equal(runs["per_level"]["gu"], runs["fused"]["gu"]), (D, L, "gu differs between the two forms")


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_pyramid_backward_kernels_off_the_16_byte_grid(dev, shift):
    """srf_causal_dwconv_bwd and srf_causal_pyramid_bwd with every operand `shift` floats behind a 256-byte boundary inside
    poisoned guard bands: every output word written, no poison read, guards untouched; a refused call writes nothing."""
    from tests.placement import Arena
    lib = _lib().load()
    D, L = 3, _tile() + 4
    ops32, d, ref, f32 = _pyr_reference(D, L)
    u0, a0, ws0, _, sl0, gm0 = ops32
    Bt, Cc, _ = u0.shape

    def close(got, want, yard):
        scale = float(want.abs().max())
        return float((got.cpu().double() - want).abs().max()) <= max(1e-5, 4.0 * float((yard.double() - want).abs().max()) / scale) * scale
    arena = Arena(dev, 8 << 20)
    put = lambda t, n: arena.put(t, shift_floats=shift, name=n)
    u, a_p, gm = put(u0, "u"), put(a0, "a_p"), put(gm0, "gm")
    ws = [put(w, "w%d" % k) for k, w in enumerate(ws0)]
    slopes = [put(s, "slope%d" % k) for k, s in enumerate(sl0)]
    dd = [put(v, "d%d" % k) for k, v in enumerate(d)]
    place = lambda shape, n: arena.place(shape, shift_floats=shift, name=n)
    out = {"gu": place(u0.shape, "gu"), "da_p": place((1,), "da_p"), "dw": [place(w.shape, "dw%d" % k) for k, w in enumerate(ws0)],
           "db": [place((Cc,), "db%d" % k) for k in range(D)], "ds": [place((1,), "ds%d" % k) for k in range(D)]}
    scratch = place((lib.srf_causal_pyramid_bwd_scratch_bytes(Bt, Cc, L, D) // 4,), "scratch")
    # refused (gu aliases u): nothing is written
    rc = lib.srf_causal_pyramid_bwd(_p(gm), _p(u), _ptrs(dd), _p(a_p), _ptrs(ws), _ptrs(slopes), _p(u), _ptrs(out["dw"]),
                                    _ptrs(out["db"]), _ptrs(out["ds"]), _p(out["da_p"]), Bt, Cc, L, D, _p(scratch), _stream(dev))
    assert rc == -1
    torch.cuda.synchronize()
    for t in _flat(out) + [scratch]:
        arena.assert_untouched(t)
    rc = lib.srf_causal_pyramid_bwd(_p(gm), _p(u), _ptrs(dd), _p(a_p), _ptrs(ws), _ptrs(slopes), _p(out["gu"]), _ptrs(out["dw"]),
                                    _ptrs(out["db"]), _ptrs(out["ds"]), _p(out["da_p"]), Bt, Cc, L, D, _p(scratch), _stream(dev))
    _lib().check(rc, "srf_causal_pyramid_bwd")
    torch.cuda.synchronize()
    arena.check()
    for t in _flat(out):
        arena.assert_written(t)
        arena.assert_clean(t)
    assert close(out["gu"], ref["gu"], f32["gu"]) and close(out["dw"][1], ref["dw"][1], f32["dw"][1])
    # one level (k = 1: pooled g_merged, the next level's taps, weight gradient with a stride-2 input), then proj_1x1's PReLU
    gd2 = place(dd[2].shape, "gd2")
    gd1 = place(dd[1].shape, "gd1")
    o1 = {"dw": place(ws0[1].shape, "l_dw"), "db": place((Cc,), "l_db"), "ds": place((1,), "l_ds")}
    sc1 = place((lib.srf_causal_dwconv_bwd_scratch_bytes(Bt, Cc, L) // 4,), "l_scratch")
    rc = lib.srf_causal_dwconv_bwd(_p(gm), 1, None, None, 2, _p(dd[1]), _p(slopes[1]), _p(dd[0]), _p(slopes[0]), 3, _p(gd1), _p(o1["dw"]),
                                   _p(o1["db"]), _p(o1["ds"]), Bt, Cc, L >> 1, _p(sc1), _stream(dev))
    assert rc == -1                      # stride 3: refused
    torch.cuda.synchronize()
    for t in (gd1, o1["dw"], o1["db"], o1["ds"], sc1):
        arena.assert_untouched(t)
    tmp = {"dw": place(ws0[2].shape, "t_dw"), "db": place((Cc,), "t_db"), "ds": place((1,), "t_ds")}
    rc = lib.srf_causal_dwconv_bwd(_p(gm), 2, None, None, 2, _p(dd[2]), _p(slopes[2]), _p(dd[1]), _p(slopes[1]), 2, _p(gd2), _p(tmp["dw"]),
                                   _p(tmp["db"]), _p(tmp["ds"]), Bt, Cc, L >> 2, _p(sc1), _stream(dev))
    _lib().check(rc, "srf_causal_dwconv_bwd")
    rc = lib.srf_causal_dwconv_bwd(_p(gm), 1, _p(gd2), _p(ws[2]), 2, _p(dd[1]), _p(slopes[1]), _p(dd[0]), _p(slopes[0]), 2, _p(gd1),
                                   _p(o1["dw"]), _p(o1["db"]), _p(o1["ds"]), Bt, Cc, L >> 1, _p(sc1), _stream(dev))
    _lib().check(rc, "srf_causal_dwconv_bwd")
    torch.cuda.synchronize()
    arena.check()
    for t in (gd2, gd1, o1["dw"], o1["db"], o1["ds"], tmp["dw"], tmp["db"], tmp["ds"]):
        arena.assert_written(t)
        arena.assert_clean(t)
    assert close(o1["dw"], ref["dw"][1], f32["dw"][1]) and close(o1["db"], ref["db"][1], f32["db"][1])


# ---- model level ----------------------------------------------------------------------------------------------------
def _train_model(dev, cfg, sd=None, seed=0):
    from sudo_rm_rf_amd.dnn.models.causal_improved_sudormrf_v3 import CausalSuDORMRF
    torch.manual_seed(seed)
    m = CausalSuDORMRF(**cfg)
    if sd is not None:
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(dev).train().enable_hip_training()


def _named_grads(m):
    return [(k, p.grad.detach().cpu().numpy()) for k, p in m.state_dict(keep_vars=True).items()]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", sorted(ctr.GRAD_CASES))
def test_model_gradients_match_the_reference(dev, name, mode):
    from test_oracle_golden import check_grads_against_golden
    cfg, sd, x, gout = ctr.grad_case(name)
    z = cf.load_golden(name)
    m = _train_model(dev, cfg, sd)
    with _kernel_mode(mode):
        out = m(torch.from_numpy(x).to(dev))
        (out * gout.float().to(dev)).sum().backward()
        torch.cuda.synchronize()
    grads = _named_grads(m)
    K = cfg["enc_kernel_size"]
    assert not dict(grads)["encoder.weight"][..., K:].any()
    assert not any(g[..., 11:].any() for k, g in grads if ".spp_dw." in k and k.endswith("conv.weight"))
    tol, yard, flips = ctr.GRAD_BARS[ctr.GRAD_CASES[name][3]]
    check_grads_against_golden(grads, z, tol, fp32_yardstick=yard, flip_budget=flips)


@pytest.mark.parametrize("name", ["causal_tiny", "causal_tiny_a2_k11"])
def test_train_mode_output_matches_the_reference_forward(dev, name):
    cfg, _, _, wseed, _, _ = cf.CASES[name]
    m = _train_model(dev, cfg, cf.make_state_dict(cfg, wseed))
    out = m(torch.from_numpy(cf.make_input(name)).to(dev))
    assert out.requires_grad and out.grad_fn is not None
    err = float(np.abs(out.detach().cpu().numpy() - cf.load_golden(name)["out"]).max())
    print("%s: train-mode max|hip - reference| %.3e" % (name, err))
    assert err <= TOL


def _against_restatement(dev, m, cfg, T, scales=None, batch=2):
    """Gradients of the linear loss against fp64 autograd over the restatement, for cases that have no fixture.  Tensors: within
    SMALL_TOL of their largest entry, the bar of the tiny fixtures.  Scalars (PReLU slopes, gains) are signed sums over every
    element of a tensor: their rounding error scales with the sum of the terms' magnitudes, not with the net value, which
    cancellation can make ten times smaller than its neighbours' (sm.1.spp_dw.1.act.weight of the block-scales case: 1.8e-3
    beside 1.5e-2 .. 6e-2).  So, as check_grads_against_golden and check_trajectory_against_golden do, they are judged as ONE
    vector: relative L2 error of all scalar gradients within SMALL_TOL."""
    from oracle.weights import make_mixture
    x = make_mixture(batch, T, 31, channels=cfg["in_audio_channels"])
    gout = ctr.make_gout((batch, cfg["num_sources"] * cfg["in_audio_channels"], T))
    sd = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    _, ref = ctr.linear_loss_grads(cfg, sd, x, gout, scales=scales)
    out = m(torch.from_numpy(x).to(dev))
    (out * gout.float().to(dev)).sum().backward()
    torch.cuda.synchronize()
    got = dict(_named_grads(m))
    num = den = 0.0
    for k, want in ref.items():
        scale = float(np.abs(want).max())
        err = float(np.abs(got[k] - want).max())
        if want.size == 1:
            num, den = num + err ** 2, den + scale ** 2
        else:
            assert err <= SMALL_TOL * scale or (scale == 0.0 and err == 0.0), (k, err, scale)
    print("scalar gradients: relative L2 error of the whole vector %.2e" % ((num / den) ** 0.5))
    assert num <= SMALL_TOL ** 2 * den, (num, den)
    return got, ref


def test_fresh_model_trains_its_gains_first(dev):
    """Every skipinit_gain of a freshly constructed model is 0: the blocks are the identity, every block parameter but the gains
    has an exactly zero gradient, and the gains' gradients are what the restatement gives."""
    m = _train_model(dev, cf.TINY, seed=5)
    assert all(float(b.skipinit_gain.detach()) == 0.0 for b in m.sm)
    got, ref = _against_restatement(dev, m, cf.TINY, 1001)
    for k, g in got.items():
        if k.startswith("sm."):
            if k.endswith("skipinit_gain"):
                assert g != 0.0 and abs(float(g) - float(ref[k])) <= SMALL_TOL * abs(float(ref[k])), (k, g, ref[k])
            else:
                assert not g.any(), k


def test_block_scales_are_honoured(dev):
    m = _train_model(dev, cf.TINY, cf.make_state_dict(cf.TINY, 11))
    m.sm[0].alpha, m.sm[0].beta = 0.7, 1.3
    m.sm[1].alpha, m.sm[1].beta = 1.2, 0.8
    _against_restatement(dev, m, cf.TINY, 640, scales=[(0.7, 1.3), (1.2, 0.8)])


def test_fuss_training_trajectory_matches_reference_loop(dev):
    """The loop of tests/test_gpu_fuss.py::test_fuss_training_trajectory_matches_reference_loop with the opted-in causal model."""
    import sudo_rm_rf.dnn.experiments.utils.mixture_consistency as mixture_consistency
    import sudo_rm_rf.dnn.losses.snr as snr_lib
    from sudo_rm_rf_amd import augment, optim
    from test_oracle_golden import check_trajectory_against_golden
    name = "causal_fuss_s4_traj"
    cfg, batch, T, wseed, dseed = ctr.TRAJ_CASES[name]
    c, z = ctr.load_manifest()["cases"][name], cf.load_golden(name)
    sd = cf.make_state_dict(cfg, wseed)
    model = _train_model(dev, cfg, sd)
    opt = optim.FusedClipAdam(model.parameters(), lr=c["lr"], clip_grad_norm=c["clip_grad_norm"])
    loss_fn = snr_lib.PermInvariantSNRwithZeroRefs(n_sources=4, zero_mean=False, backward_loss=True, inactivity_threshold=-40.)
    losses = []
    for clean, src_b, src_s, gain in ff.make_traj_batches(batch, 4, T, dseed):
        opt.zero_grad()
        clean_wavs, input_mixture, _, _ = augment.fuss_augment_with_draws(
            torch.tensor(clean, device=dev), torch.tensor(src_b), torch.tensor(src_s), torch.tensor(gain))
        rec = mixture_consistency.apply(model(input_mixture), input_mixture)
        l = loss_fn(rec, clean_wavs)
        l.backward()
        opt.step()
        losses.append(l.item())
    print(name, "losses", losses, "reference", list(z["losses"]))
    check_trajectory_against_golden([(k, p.detach().cpu().numpy()) for k, p in model.state_dict(keep_vars=True).items()], sd, losses,
                                    z, 2e-3)


def test_backward_is_deterministic_accumulates_and_refuses_input_gradients(dev):
    cfg, sd, x, gout = ctr.grad_case("causal_train_tiny")
    m = _train_model(dev, cfg, sd)
    m._engine().keep_saved_for_repeat = True
    xd, g = torch.from_numpy(x).to(dev), gout.float().to(dev)
    loss = (m(xd) * g).sum()
    params = list(m.parameters())
    first = torch.autograd.grad(loss, params, retain_graph=True)
    second = torch.autograd.grad(loss, params)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    m._engine().keep_saved_for_repeat = False
    for _ in range(2):
        (m(xd) * g).sum().backward()
    torch.cuda.synchronize()
    assert all(torch.equal(p.grad, 2 * a) for p, a in zip(params, first))
    with pytest.raises(NotImplementedError, match="mixture"):
        m(xd.clone().requires_grad_())
    # without autograd the opted-in model runs the inference path, bit for bit what a model that never opted in returns
    from sudo_rm_rf_amd.dnn.models.causal_improved_sudormrf_v3 import CausalSuDORMRF
    plain = CausalSuDORMRF(**cfg)
    plain.load_state_dict(m.state_dict())
    plain = plain.to(dev).eval()
    with torch.no_grad():
        assert torch.equal(m(xd), plain(xd))
