"""Attentive SuDoRM-RF (v2) on the GPU: the reference's goldens through the module and through the raw C ABI, the reference's
pickle, a batch of distinct examples, a poisoned workspace, the separate() recipe and the refusals.  References: the stored
reference outputs (tests/golden/attn_*.npz) and, where there is no golden, tests/attentive_ref.py in fp64 (pinned to the
goldens by tests/test_attentive_host.py).  Bar: the project's 1e-4 max-abs.
Second half: deepest levels of Ld % 4 == 0 positions, where the transformer layer's GEMMs run the MFMA kernels (the goldens'
cases run them on the scalar one), with the kernel each GEMM was given read from the in-library trace."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from tests import attentive_fixtures as af
from tests import attentive_ref as ar

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
    from sudo_rm_rf_amd.dnn.models.attentive_sudormrf_v2 import SuDORMRF
    m = SuDORMRF(**cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def models():
    """name -> (model on the GPU, state dict); one model per configuration and weight seed"""
    out = {}
    for name, (cfg, _, _, wseed, _) in af.CASES.items():
        sd = af.make_state_dict(cfg, wseed)
        out[name] = (_model(cfg, sd), sd)
    return out


def _raw_forward(cfg, sd, wav, heads=af.HEADS, dims=af.ATT_DIMS, poison=None):
    """srf_attentive_plan_create + srf_forward through ctypes; poison: a byte to fill the workspace with first"""
    from sudo_rm_rf_amd import _lib
    lib = _lib.load()
    c = _lib.srf_config(variant=_lib.VARIANT_ATTENTIVE, in_audio_channels=1, out_channels=cfg["out_channels"],
                        in_channels=cfg["in_channels"], num_blocks=cfg["num_blocks"], upsampling_depth=cfg["upsampling_depth"],
                        enc_kernel_size=cfg["enc_kernel_size"], enc_num_basis=cfg["enc_num_basis"],
                        num_sources=cfg["num_sources"], group_size=1)
    batch, _, T = wav.shape
    h = C.c_void_p()
    _lib.check(lib.srf_attentive_plan_create(C.byref(c), heads, dims, batch, T, C.byref(h)), "srf_attentive_plan_create")
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
def test_goldens_through_the_module_and_the_c_abi(models, name):
    gold = af.load_golden(name)["out"]
    m, sd = models[name]
    wav = af.make_input(name)
    with torch.no_grad():
        out = m(torch.from_numpy(wav).to(DEV)).cpu().numpy()
    raw = _raw_forward(af.CASES[name][0], sd, wav)
    e1, e2 = float(np.abs(out - gold).max()), float(np.abs(raw - gold).max())
    print("%s: max|model - reference| = %.3e, max|C ABI - reference| = %.3e (max|ref| %.3f)" % (name, e1, e2, np.abs(gold).max()))
    assert out.shape == gold.shape and e1 <= TOL and e2 <= TOL


def test_transformer_layer_of_the_tiny_case(models):
    gold = af.load_golden("attn_tiny")
    m, _ = models["attn_tiny"]
    with torch.no_grad():
        z = m.sm[0].attention(torch.from_numpy(gold["att_in"]).to(DEV)).cpu().numpy()
    err = float(np.abs(z - gold["att_out"]).max())
    print("transformer layer: max|hip - reference| = %.3e (max|ref| %.3f)" % (err, np.abs(gold["att_out"]).max()))
    assert err <= TOL


def test_other_heads_and_head_dimensions_through_the_c_abi():
    """What the reference's SuDORMRF cannot build but its blocks (and srf_attentive_plan_create) can: 3 heads of 16 channels
    (MFMA form) and 2 heads of 24 (generic form), against attentive_ref in fp64."""
    for heads, dims in ((3, 16), (2, 24)):
        cfg = af.TINY
        sd = af.make_state_dict(cfg, 210 + heads)
        C_ = cfg["in_channels"]
        rng = np.random.default_rng(heads)
        for i in range(cfg["num_blocks"]):
            p = "sm.%d.attention.mha." % i
            for n in "QKV":
                sd[p + n + "_proj.weight"] = np.ascontiguousarray(sd[p + n + "_proj.weight"][:heads * dims])
                sd[p + n + "_proj.bias"] = np.ascontiguousarray(sd[p + n + "_proj.bias"][:heads * dims])
            sd[p + "O_proj.weight"] = (rng.uniform(-1, 1, size=(C_, heads * dims)) / np.sqrt(heads * dims)).astype(np.float32)
        wav = af.make_mixture(2, 1001, 211)
        want = ar.forward(cfg, sd, wav, torch.float64, heads=heads).numpy()
        got = _raw_forward(cfg, sd, wav, heads, dims)
        err = float(np.abs(got - want).max())
        print("H %d, d %d: max|hip - attentive_ref| = %.3e" % (heads, dims, err))
        assert err <= TOL


def test_reference_pickle_runs():
    from sudo_rm_rf_amd.dnn.models.attentive_sudormrf_v2 import SuDORMRF
    meta = af.load_manifest()["pickle"]
    m = torch.load(os.path.join(af.GOLDEN, meta["file"]), weights_only=False)
    assert type(m) is SuDORMRF
    m = m.to(DEV).eval()
    wav = af.make_mixture(meta["batch"], meta["T"], meta["input_seed"])
    out, tr = _traced(m, wav)
    gold = af.load_golden("attn_pickle")["out"]
    err = float(np.abs(out - gold).max())
    # (Ld = 20 is on the MFMA grid, but 16 channels are below every MFMA GEMM's minimum: the trace says what served the layer)
    print("pickle: max|hip - reference| = %.3e; layer (Q/K/V, O_proj, ffn) %s" % (err, _layer_gemms(tr)))
    assert out.shape == gold.shape and err <= TOL


def test_five_distinct_examples_match_their_own_forward(models):
    """Row b of a batch of 5 against attentive_ref on example b ALONE: attention or statistics that cross an example's
    boundary cannot pass."""
    cfg = af.DEFAULT_U2
    m, sd = models["attn_default_u2"]
    wav = af.make_mixture(5, 10400, 220) * np.array([1.0, 0.5, 2.0, 1.5, 0.8], dtype=np.float32)[:, None, None]
    with torch.no_grad():
        out = m(torch.from_numpy(wav).to(DEV)).cpu().numpy()
    for b in range(5):
        want = ar.forward(cfg, sd, wav[b:b + 1], torch.float64).numpy()
        err = float(np.abs(out[b:b + 1] - want).max())
        print("example %d: max|hip - attentive_ref| = %.3e" % (b, err))
        assert err <= TOL


def test_poisoned_workspace_changes_nothing(models):
    _, sd = models["attn_tiny"]
    wav = af.make_input("attn_tiny")
    clean = _raw_forward(af.TINY, sd, wav, poison=0x00)
    dirty = _raw_forward(af.TINY, sd, wav, poison=0xFF)
    assert not np.isnan(dirty).any() and np.array_equal(clean, dirty)


def test_separate_recipe(models):
    from sudo_rm_rf_amd import pipeline
    m, sd = models["attn_tiny"]
    raw = af.make_mixture(3, 1001, 230) * np.array([0.3, 2.0, 1.0], dtype=np.float32)[:, None, None] + 0.05
    want = ar.separate(af.TINY, sd, raw, torch.float64).numpy()
    got = pipeline.separate(m, torch.from_numpy(raw).to(DEV)).cpu().numpy()
    listed = pipeline.separate_list(m, [torch.from_numpy(raw[b, 0]).to(DEV) for b in range(3)])
    for b in range(3):
        bar = TOL * max(1.0, float(raw[b].std(ddof=1)))
        err = float(np.abs(got[b] - want[b]).max())
        print("separate, example %d: err %.3e, bar %.3e" % (b, err, bar))
        assert err <= bar
        assert float(np.abs(listed[b].cpu().numpy() - want[b]).max()) <= bar


def test_refusals(models):
    from sudo_rm_rf_amd._lib import SrfError
    from sudo_rm_rf_amd.dnn.models.attentive_sudormrf_v2 import SuDORMRF
    m, sd = models["attn_tiny"]
    x = torch.from_numpy(af.make_input("attn_tiny")).to(DEV)
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
        shallow = SuDORMRF(**dict(af.TINY, upsampling_depth=1)).to(DEV).eval()
        with pytest.raises(SrfError, match="upsampling_depth = 1"):
            shallow(x)
        with pytest.raises(SrfError, match=r"Ld = 5001"):
            SuDORMRF(**dict(af.TINY, upsampling_depth=2, num_blocks=1)).to(DEV).eval()(torch.zeros(1, 1, 100020, device=DEV))
        assert np.isfinite(m(x).cpu().numpy()).all()


# ---- Ld % 4 == 0: the transformer layer on its MFMA GEMMs -------------------------------------------------------------------
# Every case above but the 16-channel pickle has Ld % 4 != 0, where srf_pw_conv_packed sends the layer's Q/K/V, O_proj and ffn
# convs to the scalar kernel.  Below, the lengths at which they run the kernels of the published profile; which kernel is read
# from the in-library trace, never assumed.  Reference: tests/attentive_ref.py in fp64 (no length-dependent path).
def _traced(m, wav):
    from sudo_rm_rf_amd import ops
    with torch.no_grad(), ops.kernel_trace(DEV) as tr:
        out = m(torch.from_numpy(wav).to(DEV))
    torch.cuda.synchronize()
    return out.cpu().numpy(), tr


def _gemms(tr):
    return sorted(n for n in tr.names if n.startswith("pw_"))


def _layer_gemms(tr):
    """[(Q/K/V, O_proj, ffn)] launch names per block: the GEMM before the attention kernel and the two after it"""
    names = [n for n, _ in tr.launches]
    return [(names[i - 1], names[i + 1], names[i + 2]) for i, n in enumerate(names) if n.startswith("mha_attention")]


@functools.lru_cache(maxsize=None)
def _tiny_grid_case(i):
    """(input, fp64 reference) of af.TINY_GRID[i] on the weights of attn_tiny: computed once, shared, never written to"""
    T, batch, _, iseed = af.TINY_GRID[i]
    wav = af.make_mixture(batch, T, iseed)
    return wav, ar.forward(af.TINY, af.make_state_dict(af.TINY, af.CASES["attn_tiny"][3]), wav, torch.float64).numpy()


@pytest.mark.parametrize("i", range(len(af.TINY_GRID)), ids=["T%d_B%d_Ld%d" % c[:3] for c in af.TINY_GRID])
def test_tiny_model_on_the_mfma_grid(models, i):
    T, batch, Ld, _ = af.TINY_GRID[i]
    assert af.deepest_length(af.TINY, T) == Ld and Ld % 4 == 0
    m, _ = models["attn_tiny"]
    wav, want = _tiny_grid_case(i)
    out, tr = _traced(m, wav)
    err = float(np.abs(out - want).max())
    print("TINY T %d, batch %d, Ld %d: max|hip - attentive_ref| = %.3e, bar %.1e (max|ref| %.3f); GEMMs %s; layer (Q/K/V, O_proj, "
          "ffn) %s" % (T, batch, Ld, err, TOL, np.abs(want).max(), _gemms(tr), sorted(set(_layer_gemms(tr)))))
    assert "pw_conv_generic" not in tr.names, _gemms(tr)
    layer = _layer_gemms(tr)
    assert len(layer) == af.TINY["num_blocks"] and all(n.startswith("pw_conv_") for blk in layer for n in blk), layer
    assert out.shape == want.shape and err <= TOL


@pytest.fixture(scope="module")
def wide():
    """The WIDE model, a batch of distinct examples that gives O_proj (C / 256 = 2 m-tiles x 2 n-tiles per example) at least as
    many 256 x 128 tiles as the device has CUs -- 64 examples on 256 CUs: exactly as many -- and its fp64 reference, computed
    once for the whole batch (the model is per-example independent: rows 0 .. n - 1 are the reference of every smaller batch)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nb = -(-cus // 4)
    sd = af.make_state_dict(af.WIDE, af.WIDE_WSEED)
    wav = af.make_distinct(nb, af.WIDE_T, af.WIDE_INPUT_SEED)
    want = ar.forward(af.WIDE, sd, wav, torch.float64).numpy()
    return dict(model=_model(af.WIDE, sd), sd=sd, wav=wav, want=want, nb=nb, cus=cus)


X3_LAYER = ("pw_conv_x3p<0>", "pw_conv_x3w<0>", "pw_conv_x3p<1>")


@pytest.mark.parametrize("batch", [1, 8, "chip"])
def test_wide_model_on_the_bench_kernels(wide, batch):
    """Batch 1: the 64 x 64-tile kernel; batch 8: the 128 x 128 ones; a batch that fills the chip: the 256 x 128 kernels of
    profiles/attentive_forward.txt -- Q/K/V and ffn in the paired-block form, O_proj (residual AND statistics) in the other."""
    n = wide["nb"] if batch == "chip" else batch
    assert af.deepest_length(af.WIDE, af.WIDE_T) == af.WIDE_LD == 132
    out, tr = _traced(wide["model"], wide["wav"][:n])
    errs = np.abs(out - wide["want"][:n]).max(axis=(1, 2))
    layer = _layer_gemms(tr)
    print("WIDE batch %d (%d CUs): max|hip - attentive_ref| = %.3e (example %d), bar %.1e (max|ref| %.3f); GEMMs %s; layer (Q/K/V, "
          "O_proj, ffn) %s" % (n, wide["cus"], errs.max(), errs.argmax(), TOL, np.abs(wide["want"][:n]).max(), _gemms(tr),
                                sorted(set(layer))))
    assert "pw_conv_generic" not in tr.names, _gemms(tr)
    assert len(layer) == af.WIDE["num_blocks"]
    if batch == "chip":
        # tiles of 256 x 128: Q/K/V n * 12 * 2, O_proj and ffn n * 2 * 2 (= the CU count at 64 examples on 256 CUs), proj_1x1 n * 2 * 3
        assert n * 2 * 2 >= wide["cus"]
        assert all(blk == X3_LAYER for blk in layer), layer
        assert [x for x, _ in tr.launches].count("pw_conv_x3p<0>") == 2 * af.WIDE["num_blocks"]      # Q/K/V and proj_1x1
    elif batch == 1:
        assert all(blk == ("pw_conv_bf16x3_w4",) * 3 for blk in layer), layer
    else:
        assert all(blk[0].startswith("pw_conv_bf16x3_p8<") or blk[0] == "pw_conv_bf16x3_w8" for blk in layer), layer
    assert out.shape == (n, 2, af.WIDE_T) and errs.max() <= TOL


def test_wide_model_through_the_c_abi_with_a_poisoned_workspace(wide):
    clean = _raw_forward(af.WIDE, wide["sd"], wide["wav"], poison=0x00)
    dirty = _raw_forward(af.WIDE, wide["sd"], wide["wav"], poison=0xFF)
    err = float(np.abs(clean - wide["want"]).max())
    print("WIDE batch %d through the C ABI: max|hip - attentive_ref| = %.3e, bar %.1e" % (wide["nb"], err, TOL))
    assert not np.isnan(dirty).any() and np.array_equal(clean, dirty)
    assert err <= TOL


@pytest.mark.parametrize("which,batch,Ld", [("tiny", 2, 28), ("tiny", 2, 132), ("wide", "chip", 132)])
def test_transformer_layer_alone_on_the_mfma_grid(models, wide, which, batch, Ld):
    """m.sm[0].attention on a random normalised input against ar.transformer_layer in fp64: places a model-level failure inside
    or outside the layer.  (The stand-alone layer calls ops.pw_conv without packed weights: the kernels are printed.)
    Measured on an MI355X: 3.2e-5, 3.3e-5 and 8.0e-5 -- ten times the model-level errors and torch's own fp32 deviation on these
    inputs (2.7e-6, 6.3e-6, 9.1e-6): white noise through the fixtures' four-times-wider Q / K weights makes sharp softmaxes, which
    pass on the split-bf16 GEMMs' error on q and k (3e-5 at op level) undamped."""
    m, sd = models["attn_tiny"] if which == "tiny" else (wide["model"], wide["sd"])
    n = wide["nb"] if batch == "chip" else batch
    C_ = (af.TINY if which == "tiny" else af.WIDE)["in_channels"]
    x = np.random.default_rng(1000 * Ld + C_).standard_normal(size=(n, C_, Ld))
    x = ((x - x.mean(axis=(1, 2), keepdims=True)) / x.std(axis=(1, 2), keepdims=True)).astype(np.float32)
    sd64 = {k: torch.from_numpy(v).double() for k, v in sd.items() if k.startswith("sm.0.attention.")}
    want = ar.transformer_layer(torch.from_numpy(x).double(), sd64, "sm.0.attention.", af.HEADS).numpy()
    from sudo_rm_rf_amd import ops
    with torch.no_grad(), ops.kernel_trace(DEV) as tr:
        z = m.sm[0].attention(torch.from_numpy(x).to(DEV))
    torch.cuda.synchronize()
    err = float(np.abs(z.cpu().numpy() - want).max())
    print("transformer layer, %s, batch %d, Ld %d: max|hip - attentive_ref| = %.3e, bar %.1e (max|ref| %.3f); GEMMs %s"
          % (which, n, Ld, err, TOL, np.abs(want).max(), _gemms(tr)))
    assert "pw_conv_generic" not in tr.names, _gemms(tr)
    assert z.shape == want.shape and err <= TOL


@pytest.mark.parametrize("mode", [1, 2])
def test_attentive_walk_in_the_other_kernel_modes(models, mode):
    """Kernel mode 1 (generic kernels only) and 2 (exact-fp32 MFMA GEMMs) on a case off the MFMA grid (attn_tiny, against the
    reference's golden) and one on it (TINY T = 1100, against attentive_ref in fp64)."""
    from sudo_rm_rf_amd import ops
    m, _ = models["attn_tiny"]
    wav, want = _tiny_grid_case(1)
    assert wav.shape == (2, 1, 1100)
    gold = af.load_golden("attn_tiny")["out"]
    ops.set_kernel_mode(mode)
    try:
        out_a, tr_a = _traced(m, af.make_input("attn_tiny"))
        out_b, tr_b = _traced(m, wav)
    finally:
        ops.set_kernel_mode(0)
    e_a, e_b = float(np.abs(out_a - gold).max()), float(np.abs(out_b - want).max())
    print("kernel mode %d: attn_tiny err %.3e, TINY T 1100 err %.3e, bar %.1e; GEMMs %s | %s" % (mode, e_a, e_b, TOL, _gemms(tr_a),
                                                                                              _gemms(tr_b)))
    for tr in (tr_a, tr_b):
        if mode == 1:
            assert "mha_attention_generic" in tr.names and "mha_attention_mfma" not in tr.names
            assert set(_gemms(tr)) == {"pw_conv_generic"}, _gemms(tr)      # no MFMA GEMM of any family
        else:
            assert "mha_attention_mfma" in tr.names
    assert e_a <= TOL and e_b <= TOL
