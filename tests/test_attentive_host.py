"""Attentive SuDoRM-RF (v2) on the host: module schema, seeded weights and the reference's pickle against fixtures made by the
reference (tools/make_golden_attentive.py), the library's new symbols, the plan's geometry and refusals, and the torch
restatement tests/attentive_ref.py against every golden.  No GPU needed."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest
import torch

from tests import attentive_fixtures as af
from tests import attentive_ref as ar


@pytest.fixture(scope="module")
def man():
    return af.load_manifest()


def _model(cfg):
    from sudo_rm_rf_amd.dnn.models.attentive_sudormrf_v2 import SuDORMRF
    return SuDORMRF(**cfg)


def _plan(cfg, batch, T, heads=af.HEADS, dims=af.ATT_DIMS):
    from sudo_rm_rf_amd.engine import Plan
    tup = ("attentive", 1) + tuple(cfg[f] for f in af.FIELDS[:6]) + (cfg["num_sources"], 1, (heads, dims))
    return Plan(tup, batch, T, torch.device("cpu"))


@pytest.mark.parametrize("name", sorted(af.CASES))
def test_schema_and_order_match_manifest(man, name):
    meta = man["cases"][name]
    cfg = meta["config"]
    assert cfg == af.CASES[name][0]
    sd = _model(cfg).state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == af.schema(cfg)
    U, D = cfg["num_blocks"], cfg["upsampling_depth"]
    assert len(sd) == 5 + U * (10 + 4 * D + 18) + 4
    assert sum(v.numel() for v in sd.values()) == meta["num_params"]
    assert af.deepest_length(cfg, meta["T"]) == meta["deepest_length"]


@pytest.mark.parametrize("tag", sorted(af.DIGEST_CONFIGS))
def test_same_seed_gives_the_reference_weights(man, tag):
    ref = man["digests"][tag]
    torch.manual_seed(ref["seed"])
    m = _model(ref["config"])
    got = [[k, list(v.shape), hashlib.sha256(v.detach().contiguous().numpy().tobytes()).hexdigest()]
           for k, v in m.state_dict().items()]
    assert got == ref["state_dict"]
    for a, v in ref["attributes"].items():
        assert getattr(m, a) == v, a
    # as the reference: the blocks are built with 4 heads of 256 channels whatever the constructor was given
    mha = m.sm[0].attention.mha
    assert (mha.n_heads, mha.d_model) == (man["block_heads"], man["block_att_dims"]) == (4, 256)
    assert m._config_tuple()[0] == "attentive" and m._config_tuple()[10] == (4, 256)


def test_both_import_paths_resolve():
    import sudo_rm_rf.dnn.models.attentive_sudormrf_v2 as shim
    import sudo_rm_rf_amd.dnn.models.attentive_sudormrf_v2 as ours
    for n in ("_LayerNorm", "GlobLN", "ConvNormAct", "ConvNorm", "NormAct", "DilatedConv", "DilatedConvNorm", "PositionalEncoding",
              "MHAttentionLayer", "TransformerLayer", "AttentiveUConvBlock", "SuDORMRF"):
        assert getattr(shim, n) is getattr(ours, n)
    assert not hasattr(ours, "MHANormLayer")      # dead code in the reference: neither built nor mirrored


def test_reference_pickle_unpickles_into_our_classes(man):
    from sudo_rm_rf_amd.dnn.models.attentive_sudormrf_v2 import AttentiveUConvBlock, SuDORMRF, TransformerLayer
    meta = man["pickle"]
    path = os.path.join(af.GOLDEN, meta["file"])
    assert os.path.getsize(path) < (1 << 20)
    m = torch.load(path, weights_only=False)
    assert type(m) is SuDORMRF
    assert isinstance(m.sm[0], AttentiveUConvBlock) and isinstance(m.sm[0].attention, TransformerLayer)
    torch.manual_seed(meta["seed"])
    want = _model(meta["config"]).state_dict()
    got = m.state_dict()
    assert list(got) == list(want)
    assert all(torch.equal(got[k], want[k]) for k in want)
    assert m._config_tuple()[0] == "attentive" and not m.training
    # the pickle's own forward, restated: the golden the GPU test holds the unpickled module to
    gold = af.load_golden("attn_pickle")["out"]
    wav = af.make_mixture(meta["batch"], meta["T"], meta["input_seed"])
    out = ar.forward(meta["config"], {k: v.numpy() for k, v in got.items()}, wav).numpy()
    assert np.abs(out - gold).max() <= 1e-4


def test_the_separate_list_route_is_per_utterance():
    from sudo_rm_rf_amd import pipeline
    m = _model(dict(af.TINY, out_channels=256))
    assert type(m).__name__ == "SuDORMRF" and not hasattr(m, "separate_ragged")
    assert pipeline.ragged_route(m, 32000) == "single"


def test_library_exports_the_new_symbols_and_keeps_its_abi():
    from sudo_rm_rf_amd import _lib, ops
    lib = _lib.load()
    assert lib.srf_abi_version() == 19 == _lib.ABI_VERSION
    for name in ("srf_attentive_plan_create", "srf_mha_attention", "srf_mha_attention_mfma_supported", "srf_posenc_apply",
                 "srf_gln_apply2_add"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert C.sizeof(_lib.srf_config) == 10 * C.sizeof(C.c_int)      # the config did not grow
    assert _lib.VARIANT_ATTENTIVE == 3
    for name in ("mha_attention", "posenc_apply", "gln_apply2_add"):
        assert not hasattr(ops, name)
    # the dispatch test of the attention kernel: MFMA for d % 16 == 0 in 16..256, the VALU form otherwise
    assert [d for d in range(1, 300) if lib.srf_mha_attention_mfma_supported(d)] == list(range(16, 257, 16))


@pytest.mark.parametrize("name", sorted(af.CASES))
def test_plan_geometry_follows_the_padding_rule(man, name):
    meta = man["cases"][name]
    cfg = meta["config"]
    p = _plan(cfg, meta["batch"], meta["T"])
    assert p.padded_length == meta["padded_length"] == af.padded_length(cfg, meta["T"])
    assert p.frames == meta["padded_length"] // (cfg["enc_kernel_size"] // 2)
    assert p.frames >> (cfg["upsampling_depth"] - 1) == meta["deepest_length"]
    assert p.num_params == len(af.schema(cfg))
    assert p.workspace_bytes > 0 and not p.ragged_supported
    assert _model(cfg).lcm == np.lcm(cfg["enc_kernel_size"] // 2, 2 ** cfg["upsampling_depth"])


def test_plan_refusals_name_their_argument():
    from sudo_rm_rf_amd import _lib
    from sudo_rm_rf_amd._lib import SrfError
    with pytest.raises(SrfError, match="upsampling_depth = 1"):
        _plan(dict(af.TINY, upsampling_depth=1), 1, 1000)
    # D = 2, K = 21: Ld = frames / 2 = T / 20
    assert _plan(dict(af.TINY, upsampling_depth=2), 1, 100000).frames == 10000
    with pytest.raises(SrfError, match=r"Ld = 5001 .* 5000"):
        _plan(dict(af.TINY, upsampling_depth=2), 1, 100020)
    with pytest.raises(SrfError, match="n_heads = 0"):
        _plan(af.TINY, 1, 1000, heads=0)
    with pytest.raises(SrfError, match="att_dims = -1"):
        _plan(af.TINY, 1, 1000, dims=-1)
    with pytest.raises(SrfError, match="enc_kernel_size must be odd"):
        _plan(dict(af.TINY, enc_kernel_size=20), 1, 1000)
    with pytest.raises(SrfError, match="multiple of 2"):          # K = 9, D = 4: 4 m frames, not a multiple of 8
        _plan(dict(af.TINY, enc_kernel_size=9, upsampling_depth=4), 1, 16)
    lib = _lib.load()
    cfg = _lib.srf_config(variant=_lib.VARIANT_ATTENTIVE, in_audio_channels=1, out_channels=32, in_channels=64, num_blocks=2,
                          upsampling_depth=3, enc_kernel_size=21, enc_num_basis=64, num_sources=2, group_size=1)
    h = C.c_void_p()
    assert lib.srf_plan_create(C.byref(cfg), 1, 1000, C.byref(h)) == -1 and b"srf_attentive_plan_create" in lib.srf_last_error()
    cfg.in_audio_channels = 2
    assert lib.srf_attentive_plan_create(C.byref(cfg), 4, 256, 1, 1000, C.byref(h)) == -1
    assert b"in_audio_channels" in lib.srf_last_error()


def test_training_and_ragged_entry_points_refuse_the_plan():
    from sudo_rm_rf_amd import _lib
    p = _plan(af.TINY, 2, 1000)
    lib = _lib.load()
    assert lib.srf_plan_ragged_supported(p.handle) == 0 and lib.srf_plan_ragged_workspace_bytes(p.handle) == 0
    assert lib.srf_train_saved_bytes(p.handle) == 0 and lib.srf_train_scratch_bytes(p.handle) == 0
    rc = lib.srf_forward_train(p.handle, None, 0, None, None, None, 0, None, 0, None)
    assert rc == -1 and b"attentive" in lib.srf_last_error()
    for fn in ("srf_backward", "srf_backward_wav"):
        args = [p.handle, None, None, 0, None, None, None, 0, None, 0] + ([C.c_void_p(16)] if fn.endswith("wav") else []) + [None]
        assert getattr(lib, fn)(*args) == -1 and b"attentive" in lib.srf_last_error()
    lens = (C.c_int * 2)(1000, 900)
    table = (C.c_void_p * 1)(16)
    one = C.c_void_p(256)
    rc = lib.srf_forward_ragged(p.handle, table, 1, one, lens, one, one, 0, None)
    assert rc == -1 and b"attentive" in lib.srf_last_error()
    rc = lib.srf_separate_ragged(p.handle, table, 1, one, lens, one, one, 0, one, 0, None)
    assert rc == -1 and b"attentive" in lib.srf_last_error()


def test_python_refusals_need_no_gpu():
    from sudo_rm_rf_amd._lib import SrfError
    m = _model(af.TINY)
    with pytest.raises(RuntimeError, match="dropout"):                    # train() mode, att_dropout 0.1
        m(torch.zeros(1, 1, 200))
    m.eval()
    with pytest.raises(RuntimeError, match=r"torch\.no_grad\(\)"):        # autograd would need a backward
        m(torch.zeros(1, 1, 200))
    with torch.no_grad():
        with pytest.raises(SrfError, match="MI355X"):
            m(torch.zeros(1, 1, 200))
        with pytest.raises(NotImplementedError, match="ragged"):
            m.forward_ragged(torch.zeros(2, 1, 200), [200, 100])


@pytest.fixture(scope="module")
def restated(man):
    """name -> (fp64 output, transformer taps) of tests/attentive_ref.py on the golden's weights and input"""
    out = {}
    for name, (cfg, _, _, wseed, _) in af.CASES.items():
        taps = []
        y = ar.forward(cfg, af.make_state_dict(cfg, wseed), af.make_input(name), torch.float64, taps)
        out[name] = (y.numpy(), taps)
    return out


@pytest.mark.parametrize("name", sorted(af.CASES))
def test_restatement_agrees_with_the_reference(restated, name):
    gold = af.load_golden(name)
    y, taps = restated[name]
    err = float(np.abs(y - gold["out"]).max())
    print("%s: max|attentive_ref fp64 - reference fp32| = %.3e" % (name, err))
    assert y.shape == gold["out"].shape and err <= 1e-4
    if name == "attn_tiny":
        a, z = taps[0]
        assert np.abs(a.numpy() - gold["att_in"]).max() <= 1e-4 and np.abs(z.numpy() - gold["att_out"]).max() <= 1e-4


# ---- the Ld % 4 == 0 cases of tests/test_gpu_attentive.py and tests/test_gpu_ops.py ---------------------------------------
def test_the_named_cases_sit_where_the_gpu_tests_need_them():
    """The deepest-level length decides which GEMM kernel the transformer layer runs (an MFMA one only for Ld % 4 == 0): a change
    to the padding rule must not quietly move a case on or off that grid."""
    named = [(af.TINY, 1001, 26), (af.TINY, 50, 2), (af.DEFAULT_U2, 10400, 130), (af.MAIN_U2, 32079, 201), (af.PICKLE, 777, 20),
             (af.WIDE, af.WIDE_T, af.WIDE_LD)] + [(af.TINY, T, Ld) for T, _, Ld, _ in af.TINY_GRID]
    assert [af.deepest_length(cfg, T) for cfg, T, _ in named] == [Ld for _, _, Ld in named]
    assert [Ld for _, _, Ld in named[:5]] == [26, 2, 130, 201, 20] and af.WIDE_LD == 132
    assert [Ld for _, _, Ld, _ in af.TINY_GRID] == [4, 28, 124, 128, 132, 28]
    # the goldens' cases keep off the grid (the pickle apart), the new ones are on it
    assert [Ld % 4 == 0 for _, _, Ld in named] == [False] * 4 + [True] * (2 + len(af.TINY_GRID))
    for (cfg, _, T, _, _), Ld in zip((af.CASES[n] for n in ("attn_tiny", "attn_tiny_short", "attn_default_u2", "attn_main_u2")),
                                     (26, 2, 130, 201)):
        assert af.deepest_length(cfg, T) == Ld
    assert _plan(af.WIDE, 1, af.WIDE_T).frames == 2 * af.WIDE_LD


def test_restatement_in_fp32_leaves_headroom_under_the_gpu_bar():
    """attentive_ref in fp32 against itself in fp64 on the TINY T = 1100 case: a tenth of the 1e-4 the GPU is held to."""
    T, batch, _, iseed = af.TINY_GRID[1]
    assert (T, batch) == (1100, 2)
    sd, wav = af.make_state_dict(af.TINY, af.CASES["attn_tiny"][3]), af.make_mixture(batch, T, iseed)
    y64 = ar.forward(af.TINY, sd, wav, torch.float64)
    y32 = ar.forward(af.TINY, sd, wav, torch.float32)
    err = float((y32.double() - y64).abs().max())
    print("TINY T = 1100: max|attentive_ref fp32 - fp64| = %.3e (max|ref| %.3f), bar %.1e" % (err, float(y64.abs().max()), 1e-4 / 10))
    assert y32.dtype == torch.float32 and err <= 1e-4 / 10


def test_wide_reference_for_64_examples_is_affordable():
    """The GPU test of the WIDE model computes this once per module: under a minute on at most 16 threads."""
    import time
    sd = af.make_state_dict(af.WIDE, af.WIDE_WSEED)
    wav = af.make_distinct(64, af.WIDE_T, af.WIDE_INPUT_SEED)
    before = torch.get_num_threads()
    torch.set_num_threads(min(16, before))
    try:
        t0 = time.perf_counter()
        y = ar.forward(af.WIDE, sd, wav, torch.float64)
        dt = time.perf_counter() - t0
    finally:
        torch.set_num_threads(before)
    peak = y.abs().amax(dim=(1, 2))
    print("WIDE fp64 reference, 64 examples: %.1f s on %d threads; max|ref| per example %.3f .. %.3f"
          % (dt, min(16, before), float(peak.min()), float(peak.max())))
    assert y.shape == (64, 2, af.WIDE_T) and bool(torch.isfinite(y).all())
    assert float(peak.max()) >= 0.1          # (the outputs are of a size at which 1e-4 absolute means something)
    assert dt < 60.0


# ---- byte and count literals --------------------------------------------------------------------------------------------------
# (workspace bytes, parameters, launches) of the plans of the two fixtures, recorded on commit 13ee426: the commit BEFORE the
# attentive plan constructor took plan_add_pack from srf_plan.h and the walk the shared pack helpers and tail.
SIZE_CASES = {"tiny": (af.TINY, 2, 1001), "wide": (af.WIDE, 8, af.WIDE_T)}
PLAN_SIZES = {"tiny": (2940416, 89, 34), "wide": (92263168, 81, 32)}


def plan_sizes(name):
    p = _plan(*SIZE_CASES[name])
    return p.workspace_bytes, p.num_params, p.num_launches


@pytest.mark.parametrize("name", sorted(SIZE_CASES))
def test_plan_sizes_are_what_they_were(name):
    assert plan_sizes(name) == PLAN_SIZES[name]
