"""Attentive SuDoRM-RF (v3) on the GPU: the reference's goldens through the module and through the raw C ABI, the stored
resampler of attn3_tiny, the reference's pickle, a batch of distinct examples, the separate() recipe, the kernels
attn3_default_u2 runs at batch 2 (the kernels that split the fp32 weight on the fly; the batch-32 kernels of the published
profile are covered by the WIDE3 and MANY tests of tests/test_gpu_attentive_v3_walk.py), the refusals, and srf_gln_apply_stats
against fp64.  References: the stored reference outputs
(tests/golden/attn3_*.npz) and, where there is no golden, tests/attentive_v3_ref.py in fp64 (pinned to the goldens within 1e-5
by tests/test_attentive_v3_host.py).  Bar: the project's 1e-4 max-abs.
Measured on an MI355X: goldens 1.8e-7 .. 2.4e-6 (module and C ABI alike), stored resampler 2.1e-5 at max |ref| 11.7, pickle
5.2e-8, distinct examples <= 4.2e-6, separate <= 4.5e-6, a block alone 9.9e-7; srf_gln_apply_stats value <= 6.2e-7, its
statistics <= 1.8e-16 relative to the fp64 sums of the stored output."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from tests import attentive_ref as ar2
from tests import attentive_v3_fixtures as af
from tests import attentive_v3_ref as ar
from tests import placement as pl

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    from sudo_rm_rf_amd import _lib, ops
    _lib.load()
    ops.set_kernel_mode(0)
    ops.set_debug_flags(0)


def _model(cfg, sd):
    from sudo_rm_rf_amd.dnn.models.attentive_sudormrf_v3 import SuDORMRF
    m = SuDORMRF(**cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _case(name):
    """(model on the GPU, state dict) of a golden case: made once, shared, never written to"""
    cfg, _, _, wseed, _ = af.CASES[name]
    sd = af.make_state_dict(cfg, wseed)
    return _model(cfg, sd), sd


def _raw_forward(cfg, sd, wav, heads=af.HEADS, dims=af.ATT_DIMS, poison=None):
    """srf_attentive_v3_plan_create + srf_forward through ctypes; poison: a byte to fill the workspace with first"""
    from sudo_rm_rf_amd import _lib
    lib = _lib.load()
    c = _lib.srf_config(variant=_lib.VARIANT_ATTENTIVE_V3, in_audio_channels=1, out_channels=cfg["out_channels"],
                        in_channels=cfg["in_channels"], num_blocks=cfg["num_blocks"], upsampling_depth=cfg["upsampling_depth"],
                        enc_kernel_size=cfg["enc_kernel_size"], enc_num_basis=cfg["enc_num_basis"],
                        num_sources=cfg["num_sources"], group_size=1)
    batch, _, T = wav.shape
    h = C.c_void_p()
    _lib.check(lib.srf_attentive_v3_plan_create(C.byref(c), heads, dims, batch, T, C.byref(h)), "srf_attentive_v3_plan_create")
    try:
        assert all(v.dtype == np.float32 for v in sd.values())
        params = [torch.from_numpy(v).to(DEV) for v in sd.values()]
        assert lib.srf_plan_num_params(h) == len(params)
        table = (C.c_void_p * len(params))(*[p.data_ptr() for p in params])
        nbytes = lib.srf_plan_workspace_bytes(h)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        assert ws.data_ptr() % 256 == 0
        if poison is not None:
            ws.fill_(poison)
        x = torch.from_numpy(wav).to(DEV)
        out = torch.full((batch, cfg["num_sources"], T), float("nan"), device=DEV)
        _lib.check(lib.srf_forward(h, table, len(params), _lib.ptr(x), _lib.ptr(out), _lib.ptr(ws), nbytes,
                                   _lib.current_stream(x.device)), "srf_forward")
        torch.cuda.synchronize()
        return out.cpu().numpy()
    finally:
        lib.srf_plan_destroy(h)


@pytest.mark.parametrize("name", sorted(af.CASES))
def test_goldens_through_the_module_and_the_c_abi(name):
    gold = af.load_golden(name)["out"]
    m, sd = _case(name)
    wav = af.make_input(name)
    with torch.no_grad():
        out = m(torch.from_numpy(wav).to(DEV)).cpu().numpy()
    raw = _raw_forward(af.CASES[name][0], sd, wav, poison=0xFF)
    e1, e2 = float(np.abs(out - gold).max()), float(np.abs(raw - gold).max())
    print("%s: max|model - reference| = %.3e, max|C ABI - reference| = %.3e (max|ref| %.3f)" % (name, e1, e2, np.abs(gold).max()))
    assert out.shape == gold.shape and e1 <= TOL and e2 <= TOL


def test_first_resampler_of_the_tiny_case():
    """attentive_resamplers[0] of block 0 on the reference's own inputs: 52 positions ask 26 (Lq != Lk)."""
    gold = af.load_golden("attn3_tiny")
    m, _ = _case("attn3_tiny")
    assert gold["res_q"].shape[-1] == 52 and gold["res_v"].shape[-1] == 26
    with torch.no_grad():
        z = m.sm[0].attentive_resamplers[0](torch.from_numpy(gold["res_q"]).to(DEV), torch.from_numpy(gold["res_v"]).to(DEV))
    err = float(np.abs(z.cpu().numpy() - gold["res_out"]).max())
    print("resampler 0: max|hip - reference| = %.3e (max|ref| %.3f)" % (err, np.abs(gold["res_out"]).max()))
    assert z.shape == gold["res_out"].shape and err <= TOL


def test_block_forward_is_the_walk():
    """AttentiveUConvBlock.forward (the stand-alone kernel sequence) against the restatement's block on a random input, at the
    ceil-halving lengths of attn3_odd (26 / 13 / 7)."""
    m, sd = _case("attn3_odd")
    cfg = af.TINY_K9
    x = np.random.default_rng(26).standard_normal(size=(2, cfg["out_channels"], 26)).astype(np.float32)
    sd64 = {k: torch.from_numpy(v).double() for k, v in sd.items()}
    want = ar.block(torch.from_numpy(x).double(), sd64, "sm.1.", cfg["upsampling_depth"], af.HEADS).numpy()
    with torch.no_grad():
        got = m.sm[1](torch.from_numpy(x).to(DEV)).cpu().numpy()
    err = float(np.abs(got - want).max())
    print("block 1 alone: max|hip - attentive_v3_ref| = %.3e (max|ref| %.3f)" % (err, np.abs(want).max()))
    assert got.shape == want.shape and err <= TOL


def test_reference_pickle_runs():
    from sudo_rm_rf_amd.dnn.models.attentive_sudormrf_v3 import SuDORMRF
    meta = af.load_manifest()["pickle"]
    m = torch.load(os.path.join(af.GOLDEN, meta["file"]), weights_only=False)
    assert type(m) is SuDORMRF
    m = m.to(DEV).eval()
    wav = af.make_mixture(meta["batch"], meta["T"], meta["input_seed"])
    with torch.no_grad():
        out = m(torch.from_numpy(wav).to(DEV)).cpu().numpy()
    gold = af.load_golden("attn3_pickle")["out"]
    err = float(np.abs(out - gold).max())
    print("pickle: max|hip - reference| = %.3e (max|ref| %.3f)" % (err, np.abs(gold).max()))
    assert out.shape == gold.shape and err <= TOL


def test_five_distinct_examples_match_their_own_forward():
    """Row b of a batch of 5 against attentive_v3_ref on example b ALONE: attention or statistics that cross an example's
    boundary cannot pass."""
    m, sd = _case("attn3_tiny")
    wav = af.make_distinct(5, af.DISTINCT_T, af.DISTINCT_SEED)
    with torch.no_grad():
        out = m(torch.from_numpy(wav).to(DEV)).cpu().numpy()
    for b in range(5):
        want = ar.forward(af.TINY, sd, wav[b:b + 1], torch.float64).numpy()
        err = float(np.abs(out[b:b + 1] - want).max())
        print("example %d: max|hip - attentive_v3_ref| = %.3e (max|ref| %.3f)" % (b, err, np.abs(want).max()))
        assert err <= TOL


def test_separate_recipe():
    from sudo_rm_rf_amd import pipeline
    m, sd = _case("attn3_tiny")
    raw = af.make_mixture(3, 1001, 330) * np.array([0.3, 2.0, 1.0], dtype=np.float32)[:, None, None] + 0.05
    want = ar.separate(af.TINY, sd, raw, torch.float64).numpy()
    got = pipeline.separate(m, torch.from_numpy(raw).to(DEV)).cpu().numpy()
    listed = pipeline.separate_list(m, [torch.from_numpy(raw[b, 0]).to(DEV) for b in range(3)])
    for b in range(3):
        bar = TOL * max(1.0, float(raw[b].std(ddof=1)))
        err = float(np.abs(got[b] - want[b]).max())
        print("separate, example %d: err %.3e, bar %.3e" % (b, err, bar))
        assert err <= bar
        assert float(np.abs(listed[b].cpu().numpy() - want[b]).max()) <= bar


def test_default_configuration_runs_the_mfma_kernels_where_the_level_qualifies():
    """attn3_default_u2: levels 1040 / 520 / 260 / 130.  Every resampler's attention is the MFMA kernel; a 1x1 conv is an MFMA
    GEMM on the levels of a multiple of 4 positions, and ONE per block -- the [K; V] projection of level 3, 130 positions --
    takes the scalar kernel.  Read from the in-library trace."""
    from sudo_rm_rf_amd import ops
    m, _ = _case("attn3_default_u2")
    cfg = af.DEFAULT_U2
    U, D = cfg["num_blocks"], cfg["upsampling_depth"]
    with torch.no_grad(), ops.kernel_trace(DEV) as tr:
        m(torch.from_numpy(af.make_input("attn3_default_u2")).to(DEV))
    torch.cuda.synchronize()
    names = [n for n, _ in tr.launches]
    print("attn3_default_u2 launches:", names)
    count = names.count
    assert count("mha_attention_mfma") == U * (D - 1) and count("mha_attention_generic") == 0
    assert count("posenc_apply") == count("gln_apply2_add") == U * (D - 1)
    assert count("gln_apply_stats") == U * D                      # norm(q) per resampler, final_norm's input per block
    assert count("pw_conv_generic") == U, [n for n in names if n.startswith("pw_")]
    for i, n in enumerate(names):
        if n == "mha_attention_mfma":
            # [K; V] and Q before the attention; norm(q), O_proj and ffn after it
            assert names[i - 2].startswith("pw_conv_") and names[i - 1].startswith("pw_conv_") and names[i - 3] == "posenc_apply"
            assert names[i + 1] == "gln_apply_stats" and names[i + 4] == "gln_apply2_add"
            for g in (names[i - 1], names[i + 2], names[i + 3]):          # the asking side: 260, 520 or 1040 positions
                assert g.startswith("pw_conv_") and g != "pw_conv_generic", (i, g)
    kv = [names[i - 2] for i, n in enumerate(names) if n == "mha_attention_mfma"]
    assert [g == "pw_conv_generic" for g in kv] == [True, False, False] * U, kv


def test_refusals():
    from sudo_rm_rf_amd._lib import SrfError
    from sudo_rm_rf_amd.dnn.models.attentive_sudormrf_v3 import SuDORMRF
    m, sd = _case("attn3_tiny")
    wav = af.make_input("attn3_tiny")
    x = torch.from_numpy(wav).to(DEV)
    with pytest.raises(RuntimeError, match=r"torch\.no_grad\(\)"):
        m(x)
    m.train()
    try:
        with torch.no_grad(), pytest.raises(RuntimeError, match="dropout"):
            m(x)
    finally:
        m.eval()
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="ragged"):
            m.forward_ragged(x, [1001, 900])
        with pytest.raises(SrfError, match="MI355X"):
            m(torch.from_numpy(wav))
        with pytest.raises(SrfError, match=r"5001 positions on level 1"):
            SuDORMRF(**dict(af.TINY, upsampling_depth=2, num_blocks=1)).to(DEV).eval()(torch.zeros(1, 1, 100020, device=DEV))
        assert np.isfinite(m(x).cpu().numpy()).all()


# ---- srf_gln_apply_stats ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def arena():
    return pl.Arena(DEV, 16 << 20)


def _sums(x64):
    xf = x64.reshape(x64.shape[0], -1)
    s = torch.zeros(x64.shape[0], 64, 2, dtype=torch.float64)
    s[:, 0, 0] = xf.sum(1)
    s[:, 5, 1] = (xf * xf).sum(1)          # (any bucket: the statistic is the total over the buckets)
    return s


# the issue's three shapes and one of more than a 1024-position chunk per row
@pytest.mark.parametrize("Bt,C,L", [(3, 5, 7), (2, 64, 130), (2, 512, 26), (1, 7, 1500)])
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("act", [False, True], ids=["plain", "prelu"])
def test_gln_apply_stats(arena, Bt, C, L, shift, act):
    """Value bar: y = fma(x, gamma rstd, beta - mean gamma rstd) in fp32 from fp64 statistics -- the roundings of rstd, of the two
    products, of the difference and of the fma, each 2^-24 relative to an intermediate of at most 16 here (|x - mean| <= 5 sigma,
    gamma <= 1.5, |beta| <= 0.5): 5 x 6e-8 x 16 = 4.8e-6, rounded up to 1e-5.
    Statistics: out_sums are fp64 sums of the STORED fp32 values (float -> double and the square of a float are exact in
    fp64), so against the same sums of the stored output taken on the host only the order of n additions differs:
    |error| <= n 2^-52 sum|term|.  Against the fp64 reference they differ by the outputs' fp32 rounding: the 4e-6 relative of
    tests/test_gpu_ops.py check_sums."""
    from sudo_rm_rf_amd import attention
    g = torch.Generator().manual_seed(5 * C + L)
    x = (torch.randn(Bt, C, L, generator=g, dtype=torch.float64) * 2 + 0.3).float()
    gamma = (torch.rand(C, generator=g) + 0.5).float()
    beta = (torch.rand(C, generator=g) - 0.5).float()
    slope = torch.tensor([0.2])
    want = ar2.gln(x.double(), gamma.double(), beta.double())
    if act:
        want = ar2.prelu(want, 0.2)
    arena.reset()
    dx = arena.put(x, shift_floats=shift, name="x")
    dg, db = arena.put(gamma, shift_floats=shift * 2, name="gamma"), arena.put(beta, shift_floats=shift * 3, name="beta")
    dsl = arena.put(slope, shift_floats=shift, name="slope") if act else None
    ds = arena.put(_sums(x.double()), dtype=torch.float64, name="sums")
    so = arena.place((Bt, 64, 2), dtype=torch.float64, name="out_sums", zero=True)
    y = arena.place(x.shape, shift_floats=(shift * 3) % 4, name="y")
    y2 = arena.place(x.shape, shift_floats=shift * 2, name="y_without_sums")
    y.fill_(float("nan"))
    y2.fill_(float("nan"))
    attention.gln_apply_stats(dx, ds, dg, db, dsl, out_sums=so, out=y)
    attention.gln_apply_stats(dx, ds, dg, db, dsl, out=y2)               # out_sums = NULL: the residual form
    torch.cuda.synchronize()
    arena.check()
    arena.assert_clean(y)
    arena.assert_clean(y2)
    got = y.double().cpu()
    err = (got - want).abs().max().item()
    print("gln_apply_stats (%d, %d, %d) shift %d %s: value err %.3e, bar 1e-5" % (Bt, C, L, shift, "prelu" if act else "plain", err))
    assert err <= 1e-5 and torch.equal(y2.cpu(), y.cpu())
    sums = so.cpu().sum(1)
    gf, wf, n = got.reshape(Bt, -1), want.reshape(Bt, -1), C * L
    e_s = (sums[:, 0] - gf.sum(1)).abs() / gf.abs().sum(1)
    e_q = (sums[:, 1] - (gf * gf).sum(1)).abs() / (gf * gf).sum(1)
    print("   statistics of the stored y: sum %.3e, sumsq %.3e relative; bar %.3e" % (e_s.max(), e_q.max(), n * 2.0 ** -52))
    assert (e_s <= n * 2.0 ** -52).all() and (e_q <= n * 2.0 ** -52).all()
    assert ((sums[:, 0] - wf.sum(1)).abs() <= 4e-6 * wf.abs().sum(1) + 1e-9).all()
    assert ((sums[:, 1] - (wf * wf).sum(1)).abs() <= 4e-6 * (wf * wf).sum(1) + 1e-9).all()
    # a second call ADDS to out_sums
    attention.gln_apply_stats(dx, ds, dg, db, dsl, out_sums=so, out=y)
    torch.cuda.synchronize()
    assert torch.allclose(so.cpu().sum(1), 2 * sums, rtol=1e-12, atol=0)


def test_gln_apply_stats_refusals():
    from sudo_rm_rf_amd import attention, ops
    from sudo_rm_rf_amd._lib import SrfError
    x = torch.zeros(1, 4, 8, device=DEV)
    s = ops.new_sums(1, DEV)
    gb = torch.ones(4, device=DEV)
    with pytest.raises(SrfError, match="statistics, gamma and beta"):
        attention.gln_apply_stats(x, s, None, gb)
    with pytest.raises(SrfError, match="must not be norm.sums"):
        attention.gln_apply_stats(x, s, gb, gb, out_sums=s)
