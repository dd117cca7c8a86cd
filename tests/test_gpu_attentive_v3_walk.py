"""Attentive SuDoRM-RF (v3) on the GPU, second part: the walk on the kernels of the published profile and at its edges.  The
goldens of tests/test_gpu_attentive_v3.py are the reference's own models (4 heads of 256, batch 1 or 2): no launch of theirs has
as many 256 x 128 tiles as the chip has CUs, so every 1x1 conv of theirs splits its fp32 weight on the fly and the packed images
srf_attentive_v3_forward makes are never read.  Here:
  WIDE3 (levels 528 / 264 / 132, two blocks of two resamplers) at a batch that fills the chip at every conv -- the packed-weight
    kernels, the [K; V] image hung on K_proj.weight's index, the fused mask + decoder tail -- through the module, the C ABI with a
    poisoned workspace, pipeline.separate, and each resampler alone;
  MANY: 102 packed images, more than one launch of the packing kernel holds, read from the second launch's share;
  other heads and head dimensions (every instance of the MFMA attention, the generic one, padded [K; V] sections);
  levels of ONE position; kernel modes 1 and 2; and guard bands around every operand of the C-ABI call, the workspace included.
Reference: tests/attentive_v3_ref.py in fp64 (pinned to the reference's goldens by tests/test_attentive_v3_host.py, which also
asserts the conditions on the fixtures that these tests rest on).  Bar: the project's 1e-4 max-abs, max |ref| printed next to
every error.  Which kernel served is read from the in-library trace, never assumed.
Measured on an MI355X (256 CUs):
  test_wide3_on_the_bench_kernels: batch 1 1.9e-6 (pw_conv_bf16x3_w4 throughout), batch 8 3.7e-6 (pw_conv_bf16x3_w8 / _w4), batch
    43 3.9e-6 at max |ref| 0.51 with every resampler (pw_conv_x3p<0>, pw_conv_x3p<1>, pw_conv_x3w<0>, pw_conv_x3p<1>) for ([K; V],
    Q, O_proj, ffn), pw_mask_decode, pack_pw_weights;
  test_wide3_without_packed_weights: 4.1e-6 (pw_conv_bf16x3_p8<0>, _p8<1>, _w8), 2.2e-6 from the packed run;
  test_wide3_through_the_c_abi_with_a_poisoned_workspace: 3.9e-6, 0x00 and 0xFF bit-identical;
  test_wide3_separate_recipe: worst error 2.3 % of its bar (pw_mask_decode with the mixture's statistics);
  test_wide3_resampler_alone: 7.0e-5, 6.7e-5, 9.5e-5, 6.3e-5 at max |ref| 12.6, 11.6, 14.3, 16.3 (pw_conv_bf16x3_w8, _p8<0>;
    mha_attention_mfma) -- relative to max |ref| as the model-level errors are;
  test_many_reads_images_of_the_second_packing_launch: 1.6e-5 at max |ref| 1.32, two pack_pw_weights launches, every resampler of
    every block on the same four pw_conv_x3 kernels as WIDE3's;
  test_other_heads_and_head_dimensions_through_the_c_abi: TINY 2.4e-6 .. 3.1e-6, TINY_K9 1.3e-7 .. 2.7e-7, the attention kernel
    of the table; test_narrow_model_with_padded_kv_sections: 1.3e-7 (2 x 9), 1.9e-7 (1 x 16), pw_conv_generic throughout;
    test_block_with_other_heads_stands_alone: 9.1e-7 at max |ref| 3.8;
  test_levels_of_one_position: 1.5e-7, 1.8e-7, 2.9e-7 (C ABI 3 x 16: 2.5e-7, 2 x 24: 1.6e-7), 1.5e-6;
  test_v3_walk_in_the_other_kernel_modes: mode 1 1.8e-7 / 1.4e-7 (pw_conv_generic, mha_attention_generic), mode 2 1.8e-7 /
    1.4e-7 (pw_conv_mfma, pw_conv_small; off the grid pw_conv_generic as well);
  test_the_walk_stays_inside_its_operands: guard bands intact, 1.3e-7, 2.9e-7, 2.2e-7.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

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


def _raw_forward(cfg, sd, wav, heads=af.HEADS, dims=af.ATT_DIMS, poison=None, arena=None):
    """srf_attentive_v3_plan_create + srf_forward through ctypes.  poison: a byte to fill the workspace with first.  arena: a
    placement.Arena that then holds the input, the output (NaN), every parameter and a workspace of exactly
    srf_plan_workspace_bytes() bytes; returns (output, the device views by name) for the caller's checks."""
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
        nbytes = lib.srf_plan_workspace_bytes(h)
        assert lib.srf_plan_num_params(h) == len(sd)
        if arena is None:
            params = [torch.from_numpy(v).to(DEV) for v in sd.values()]
            ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
            if poison is not None:
                ws.fill_(poison)
            x = torch.from_numpy(wav).to(DEV)
            out = torch.full((batch, cfg["num_sources"], T), float("nan"), device=DEV)
        else:
            arena.reset()
            x = arena.put(torch.from_numpy(wav), name="input")
            out = arena.place((batch, cfg["num_sources"], T), name="output")
            out.fill_(float("nan"))
            params = [arena.put(torch.from_numpy(v), name=k) for k, v in sd.items()]
            ws = arena.place((nbytes,), dtype=torch.uint8, name="workspace")          # (stays 0xFF: poisoned)
            assert ws.numel() == nbytes
        assert ws.data_ptr() % 256 == 0
        table = (C.c_void_p * len(params))(*[p.data_ptr() for p in params])
        _lib.check(lib.srf_forward(h, table, len(params), _lib.ptr(x), _lib.ptr(out), _lib.ptr(ws), nbytes,
                                   _lib.current_stream(x.device)), "srf_forward")
        torch.cuda.synchronize()
        if arena is None:
            return out.cpu().numpy()
        return out.cpu().numpy(), dict(input=x, output=out, params=params)
    finally:
        lib.srf_plan_destroy(h)


def _traced(fn):
    """(fn(), launch names in order) with the in-library trace on torch's current stream"""
    from sudo_rm_rf_amd import ops
    with torch.no_grad(), ops.kernel_trace(DEV) as tr:
        out = fn()
    torch.cuda.synchronize()
    return out, [n for n, _ in tr.launches]


def _module_forward(m, wav):
    return lambda: m(torch.from_numpy(wav).to(DEV)).cpu().numpy()


def _gemms(names):
    return sorted(set(n for n in names if n.startswith("pw_")))


def _resampler_gemms(names):
    """[(K; V, Q, O_proj, ffn)] launch names per attention launch: posenc, [K; V], Q, attention, norm(q), O_proj, ffn, add"""
    out = []
    for i, n in enumerate(names):
        if n.startswith("mha_attention"):
            assert names[i - 3] == "posenc_apply" and names[i + 1] == "gln_apply_stats" and names[i + 4] == "gln_apply2_add", \
                names[i - 3:i + 5]
            out.append((names[i - 2], names[i - 1], names[i + 2], names[i + 3]))
    return out


def _report(tag, got, want):
    """prints max |got - want| next to max |want| and returns the per-example errors"""
    assert got.shape == want.shape, (got.shape, want.shape)
    errs = np.abs(got - want).reshape(got.shape[0], -1).max(axis=1)
    print("%s: max|hip - attentive_v3_ref| = %.3e (example %d), bar %.1e (max|ref| %.3f)"
          % (tag, errs.max(), errs.argmax(), TOL, np.abs(want).max()))
    return errs


# ---- WIDE3: the kernels of the published profile --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide3():
    """The WIDE3 model, a batch of distinct examples that gives EVERY packable conv of the walk at least as many 256 x 128 tiles
    as the device has CUs (O_proj / ffn of resampler 0 have the fewest: 6 per example; 43 examples on 256 CUs), and its fp64
    reference with every resampler's (q, v, output), computed once (the model is per-example independent: rows 0 .. n - 1 are
    the reference of every smaller batch)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nb = -(-cus // af.WIDE3_MIN_TILES)
    sd = af.make_state_dict(af.WIDE3, af.WIDE3_WSEED)
    wav = af.make_distinct(nb, af.WIDE3_T, af.WIDE3_INPUT_SEED)
    taps = []
    want = ar.forward(af.WIDE3, sd, wav, torch.float64, taps).numpy()
    taps = [(q.float(), v.float(), z.numpy()) for q, v, z in taps]
    return dict(model=_model(af.WIDE3, sd), sd=sd, wav=wav, want=want, taps=taps, nb=nb, cus=cus)


# (K; V, Q, O_proj, ffn) at a batch that fills the chip: the 256 x 128 kernels of profiles/attentive_v3_forward.txt -- the
# paired-block form for [K; V] (no prologue) and for Q and ffn (norm on load), the one-block form for O_proj (residual AND
# statistics, which the paired form does not take)
X3_RESAMPLER = ("pw_conv_x3p<0>", "pw_conv_x3p<1>", "pw_conv_x3w<0>", "pw_conv_x3p<1>")


@pytest.mark.parametrize("batch", [1, 8, "chip"])
def test_wide3_on_the_bench_kernels(wide3, batch):
    cfg = af.WIDE3
    U, D = cfg["num_blocks"], cfg["upsampling_depth"]
    n = wide3["nb"] if batch == "chip" else batch
    out, names = _traced(_module_forward(wide3["model"], wide3["wav"][:n]))
    errs = _report("WIDE3 batch %d (%d CUs)" % (n, wide3["cus"]), out, wide3["want"][:n])
    layer = _resampler_gemms(names)
    print("   GEMMs %s; resamplers (K; V, Q, O_proj, ffn) %s" % (_gemms(names), layer))
    assert "pw_conv_generic" not in names, _gemms(names)
    assert names.count("mha_attention_mfma") == len(layer) == U * (D - 1)
    if batch == "chip":
        assert n * af.WIDE3_MIN_TILES >= wide3["cus"]
        for blk in layer:
            assert all(g.startswith("pw_conv_x3p<") or g.startswith("pw_conv_x3w<") for g in blk), layer
        assert "pw_mask_decode" in names and "pack_pw_weights" in names
        assert all(blk == X3_RESAMPLER for blk in layer), layer
    assert errs.max() <= TOL


def test_wide3_without_packed_weights(wide3):
    """The same batch with the images switched off (the kernels that split the fp32 weight themselves): the same bar.  A defect
    in an image -- the wrong source behind K_proj.weight's index, say -- shows as the packed run failing while this one passes."""
    from sudo_rm_rf_amd import ops
    with ops.debug_flags(ops.DebugFlag.NO_PACKED_WEIGHTS):          # (puts the flags back in a finally)
        out, names = _traced(_module_forward(wide3["model"], wide3["wav"]))
    errs = _report("WIDE3 batch %d, no packed weights" % wide3["nb"], out, wide3["want"])
    with torch.no_grad():
        packed = _module_forward(wide3["model"], wide3["wav"])()
    print("   GEMMs %s; max|packed - unpacked| = %.3e" % (_gemms(names), np.abs(out - packed).max()))
    assert "pack_pw_weights" not in names and "pw_mask_decode" not in names and "pw_conv_generic" not in names
    assert not any(g.startswith("pw_conv_x3") for g in names), _gemms(names)
    assert errs.max() <= TOL


def test_wide3_through_the_c_abi_with_a_poisoned_workspace(wide3):
    clean = _raw_forward(af.WIDE3, wide3["sd"], wide3["wav"], poison=0x00)
    dirty = _raw_forward(af.WIDE3, wide3["sd"], wide3["wav"], poison=0xFF)
    errs = _report("WIDE3 batch %d through the C ABI" % wide3["nb"], clean, wide3["want"])
    assert not np.isnan(clean).any() and not np.isnan(dirty).any() and np.array_equal(clean, dirty)
    assert errs.max() <= TOL


def test_wide3_separate_recipe(wide3):
    """pipeline.separate at the chip batch: the fused mask + decoder tail with the per-example statistics of the mixture."""
    from sudo_rm_rf_amd import pipeline
    nb = wide3["nb"]
    raw = af.make_distinct(nb, af.WIDE3_T, af.WIDE3_INPUT_SEED + 1) * np.float32(1.7) + np.float32(0.05)
    want = ar.separate(af.WIDE3, wide3["sd"], raw, torch.float64).numpy()
    got, names = _traced(lambda: pipeline.separate(wide3["model"], torch.from_numpy(raw).to(DEV)).cpu().numpy())
    assert "pw_mask_decode" in names, _gemms(names)
    worst = 0.0
    for b in range(nb):
        bar = TOL * max(1.0, float(raw[b].std(ddof=1)))
        err = float(np.abs(got[b] - want[b]).max())
        worst = max(worst, err / bar)
        assert err <= bar, (b, err, bar)
    print("WIDE3 separate, batch %d: worst err / bar = %.3f (bars %.1e .. %.1e, max|ref| %.3f)"
          % (nb, worst, TOL, TOL * max(1.0, float(raw.std(axis=-1, ddof=1).max())), np.abs(want).max()))


@pytest.mark.parametrize("i,r", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_wide3_resampler_alone(wide3, i, r):
    """m.sm[i].attentive_resamplers[r] on the (q, v) the fp64 restatement recorded for it inside the model -- the model's own
    activations, not white noise -- against the recorded output: places a model-level failure inside or outside a resampler.
    (The stand-alone layer calls ops.pw_conv without packed weights: the kernels are printed.)"""
    cfg = af.WIDE3
    q, v, z = wide3["taps"][i * (cfg["upsampling_depth"] - 1) + r]
    lv = af.WIDE3_LEVELS
    assert q.shape[-1] == lv[1 - r] and v.shape[-1] == lv[2 - r] and q.shape[0] == wide3["nb"]
    got, names = _traced(lambda: wide3["model"].sm[i].attentive_resamplers[r](q.to(DEV), v.to(DEV)).cpu().numpy())
    errs = _report("WIDE3 block %d resampler %d alone (%d ask %d), batch %d" % (i, r, q.shape[-1], v.shape[-1], q.shape[0]), got, z)
    print("   GEMMs %s, attention %s" % (_gemms(names), sorted(n for n in set(names) if n.startswith("mha_"))))
    assert "pw_conv_generic" not in names and "mha_attention_mfma" in names
    assert errs.max() <= TOL


# ---- MANY: more packed images than one launch of the packing kernel holds --------------------------------------------------------
def test_many_reads_images_of_the_second_packing_launch():
    cfg, (heads, dims) = af.MANY, af.MANY_HEADS
    U, R = cfg["num_blocks"], cfg["upsampling_depth"] - 1
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    sd = af.with_heads(af.make_state_dict(cfg, af.MANY_WSEED), cfg, heads, dims, af.MANY_WSEED)
    wav = af.make_distinct(cus, af.MANY_T, af.MANY_INPUT_SEED)
    want = ar.forward(cfg, sd, wav, torch.float64, heads=heads).numpy()
    out, names = _traced(lambda: _raw_forward(cfg, sd, wav, heads, dims, poison=0xFF))
    errs = _report("MANY batch %d, %d x %d" % (cus, heads, dims), out, want)
    layer = _resampler_gemms(names)
    print("   GEMMs %s; last block's resamplers (K; V, Q, O_proj, ffn) %s" % (_gemms(names), layer[-R:]))
    assert (U - 1) * (1 + 4 * R) + 1 + 4 * (R - 1) >= af.MANY_PACK_CHUNK          # the last resampler's first image: index 98
    assert names.count("pack_pw_weights") == 2 and "pw_conv_generic" not in names
    assert names.count("mha_attention_mfma") == len(layer) == U * R
    # the pw_conv_x3 kernels read the packed image only; images 96 .. 101 -- O_proj and ffn of the last block's third resampler
    # and all four of its fourth -- come from the second packing launch
    assert all(g.startswith("pw_conv_x3") for blk in layer for g in blk), layer
    assert errs.max() <= TOL


# ---- other heads and head dimensions ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["TINY", "TINY_K9"])
@pytest.mark.parametrize("shape", af.HEAD_SHAPES, ids=["%dx%d" % s for s, _ in af.HEAD_SHAPES])
def test_other_heads_and_head_dimensions_through_the_c_abi(which, shape):
    """What the reference's SuDORMRF cannot build but its blocks (and srf_attentive_v3_plan_create) can."""
    (heads, dims), kernel = shape
    cfg, T = (af.TINY, 1001) if which == "TINY" else (af.TINY_K9, 100)
    sd = af.with_heads(af.make_state_dict(cfg, af.HEADS_WSEED), cfg, heads, dims, af.HEADS_WSEED + heads * dims)
    wav = af.make_mixture(2, T, af.HEADS_INPUT_SEED)
    want = ar.forward(cfg, sd, wav, torch.float64, heads=heads).numpy()
    out, names = _traced(lambda: _raw_forward(cfg, sd, wav, heads, dims, poison=0xFF))
    errs = _report("%s T %d, %d x %d (%s)" % (which, T, heads, dims, kernel), out, want)
    att = [n for n in names if n.startswith("mha_attention")]
    assert att == [kernel] * (cfg["num_blocks"] * (cfg["upsampling_depth"] - 1)), att
    assert errs.max() <= TOL


@pytest.mark.parametrize("heads,dims,kernel", [(2, 9, "mha_attention_generic"), (1, 16, "mha_attention_mfma")])
def test_narrow_model_with_padded_kv_sections(heads, dims, kernel):
    cfg = af.NARROW
    sd = af.with_heads(af.make_state_dict(cfg, af.NARROW_WSEED), cfg, heads, dims, af.NARROW_WSEED + heads * dims)
    wav = af.make_mixture(2, af.NARROW_T, af.NARROW_INPUT_SEED)
    want = ar.forward(cfg, sd, wav, torch.float64, heads=heads).numpy()
    out, names = _traced(lambda: _raw_forward(cfg, sd, wav, heads, dims, poison=0xFF))
    errs = _report("NARROW T %d, %d x %d" % (af.NARROW_T, heads, dims), out, want)
    print("   GEMMs %s" % _gemms(names))
    assert set(n for n in names if n.startswith("mha_attention")) == {kernel}
    assert errs.max() <= TOL


def test_block_with_other_heads_stands_alone():
    """AttentiveUConvBlock(n_heads=2, att_dims=24) as a module of its own against the restatement's block."""
    from sudo_rm_rf_amd.dnn.models.attentive_sudormrf_v3 import AttentiveUConvBlock
    cfg, heads, dims = af.TINY_K9, 2, 24
    sd = af.with_heads(af.make_state_dict(cfg, af.HEADS_WSEED), cfg, heads, dims, af.HEADS_WSEED + heads * dims)
    blk = AttentiveUConvBlock(cfg["out_channels"], cfg["in_channels"], cfg["upsampling_depth"], n_heads=heads, att_dims=dims)
    blk.load_state_dict({k[len("sm.1."):]: torch.from_numpy(v) for k, v in sd.items() if k.startswith("sm.1.")})
    blk = blk.to(DEV).eval()
    x = np.random.default_rng(27).standard_normal(size=(2, cfg["out_channels"], 26)).astype(np.float32)
    sd64 = {k: torch.from_numpy(v).double() for k, v in sd.items()}
    want = ar.block(torch.from_numpy(x).double(), sd64, "sm.1.", cfg["upsampling_depth"], heads).numpy()
    got, names = _traced(lambda: blk(torch.from_numpy(x).to(DEV)).cpu().numpy())
    errs = _report("block of 2 x 24 alone, levels 26 / 13 / 7", got, want)
    assert names.count("mha_attention_generic") == cfg["upsampling_depth"] - 1 and "mha_attention_mfma" not in names
    assert errs.max() <= TOL


# ---- levels of one position -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,T", sorted(af.ONE_POSITION))
def test_levels_of_one_position(D, T):
    """Attention with Lq = Lk = 1, GlobLN over C x 1, a stride-2 depthwise conv on one input, an encoder with T < K, a decoder of
    one frame.  Through the module (4 x 256); the [2, 1, 1] case through the C ABI with 3 x 16 and 2 x 24 as well."""
    levels, _ = af.ONE_POSITION[(D, T)]
    cfg, sd, wav = af.one_position_case(D, T)
    assert af.level_lengths(cfg, T) == levels
    want = ar.forward(cfg, sd, wav, torch.float64).numpy()
    out, names = _traced(_module_forward(_model(cfg, sd), wav))
    errs = _report("levels %s (T %d), module" % (levels, T), out, want)
    assert names.count("mha_attention_mfma") == cfg["num_blocks"] * (D - 1)
    assert np.isfinite(out).all() and errs.max() <= TOL
    if (D, T) == (3, 8):
        for heads, dims in ((3, 16), (2, 24)):
            w = af.with_heads(sd, cfg, heads, dims, af.ONE_POSITION_WSEED + heads)
            want = ar.forward(cfg, w, wav, torch.float64, heads=heads).numpy()
            raw = _raw_forward(cfg, w, wav, heads, dims, poison=0xFF)
            errs = _report("levels %s (T %d), C ABI, %d x %d" % (levels, T, heads, dims), raw, want)
            assert np.isfinite(raw).all() and errs.max() <= TOL


# ---- the other kernel modes -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tiny():
    sd = af.make_state_dict(af.TINY, af.CASES["attn3_tiny"][3])
    return _model(af.TINY, sd), sd


@pytest.mark.parametrize("mode", [1, 2])
def test_v3_walk_in_the_other_kernel_modes(mode):
    """Kernel mode 1 (generic kernels only) and 2 (exact-fp32 MFMA GEMMs) on a case off the MFMA grid (attn3_tiny: 104 / 52 / 26,
    against the reference's golden) and one on it at every level (TINY T = 1120: 112 / 56 / 28, against the restatement)."""
    from sudo_rm_rf_amd import ops
    m, sd = _tiny()
    wav = af.make_mixture(2, af.GRID_T, af.GRID_INPUT_SEED)
    want = ar.forward(af.TINY, sd, wav, torch.float64).numpy()
    gold = af.load_golden("attn3_tiny")["out"]
    ops.set_kernel_mode(mode)
    try:
        out_a, names_a = _traced(_module_forward(m, af.make_input("attn3_tiny")))
        out_b, names_b = _traced(_module_forward(m, wav))
    finally:
        ops.set_kernel_mode(0)
    e_a = _report("kernel mode %d, attn3_tiny (golden)" % mode, out_a, gold)
    e_b = _report("kernel mode %d, TINY T %d" % (mode, af.GRID_T), out_b, want)
    print("   GEMMs %s | %s" % (_gemms(names_a), _gemms(names_b)))
    for names in (names_a, names_b):
        if mode == 1:
            assert "mha_attention_generic" in names and "mha_attention_mfma" not in names
            assert set(n for n in names if n.startswith("pw_")) == {"pw_conv_generic"}, _gemms(names)
        else:
            assert "mha_attention_mfma" in names and "mha_attention_generic" not in names
    if mode == 2:
        assert "pw_conv_generic" not in names_b, _gemms(names_b)
    assert e_a.max() <= TOL and e_b.max() <= TOL


# ---- guard bands around the whole C-ABI call -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def arena():
    return pl.Arena(DEV, 64 << 20)


def _guarded_cases():
    def narrow():
        heads, dims = af.NARROW_HEADS
        sd = af.with_heads(af.make_state_dict(af.NARROW, af.NARROW_WSEED), af.NARROW, heads, dims, af.NARROW_WSEED + heads * dims)
        wav = af.make_mixture(2, af.NARROW_T, af.NARROW_INPUT_SEED)
        return af.NARROW, sd, wav, heads, dims, ar.forward(af.NARROW, sd, wav, torch.float64, heads=heads).numpy()

    def one_position():
        cfg, sd, wav = af.one_position_case(3, 8)
        return cfg, sd, wav, af.HEADS, af.ATT_DIMS, ar.forward(cfg, sd, wav, torch.float64).numpy()

    def odd():
        cfg, _, _, wseed, _ = af.CASES["attn3_odd"]
        return cfg, af.make_state_dict(cfg, wseed), af.make_input("attn3_odd"), af.HEADS, af.ATT_DIMS, af.load_golden("attn3_odd")["out"]
    return {"narrow_2x9": narrow, "levels_2_1_1": one_position, "attn3_odd": odd}


@pytest.mark.parametrize("which", ["narrow_2x9", "levels_2_1_1", "attn3_odd"])
def test_the_walk_stays_inside_its_operands(arena, which):
    """Input, output (NaN), every parameter and a workspace of EXACTLY srf_plan_workspace_bytes() bytes lie in one arena of 0xFF
    with guard bands between them: nothing outside a payload is written, no poison reaches the output, the inputs are unchanged."""
    cfg, sd, wav, heads, dims, want = _guarded_cases()[which]()
    out, views = _raw_forward(cfg, sd, wav, heads, dims, arena=arena)
    arena.check()
    arena.assert_clean(views["output"])
    assert torch.equal(views["input"].cpu(), torch.from_numpy(wav))
    for (k, v), p in zip(sd.items(), views["params"]):
        assert torch.equal(p.cpu(), torch.from_numpy(v)), k
    errs = _report("%s inside guard bands, workspace of the plan's exact size" % which, out, want)
    assert errs.max() <= TOL
