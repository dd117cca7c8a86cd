"""Attentive SuDoRM-RF (v3) on the host: module schema, seeded weights and the reference's pickle against fixtures made by the
reference (tools/make_golden_attentive_v3.py), the library's new symbols, the plan's geometry and refusals, and the torch
restatement tests/attentive_v3_ref.py against every golden.  No GPU needed.

One refusal of srf_attentive_v3_plan_create has no test: "a level with fewer than 1 position".  The padding rule leaves at
least one frame and ceil halving keeps every level at one or more, so no argument reaches it; the check stays as a guard
(levels of exactly ONE position are reached and tested: ONE_POSITION).

Last part: the configurations that have no golden (WIDE3, MANY, NARROW, the other head shapes, the one-position levels) -- the
conditions on them that the GPU tests of tests/test_gpu_attentive_v3_walk.py rest on, so that a later edit of a fixture cannot
hollow those out."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest
import torch

from tests import attentive_v3_fixtures as af
from tests import attentive_v3_ref as ar


@pytest.fixture(scope="module")
def man():
    return af.load_manifest()


def _model(cfg):
    from sudo_rm_rf_amd.dnn.models.attentive_sudormrf_v3 import SuDORMRF
    return SuDORMRF(**cfg)


def _plan(cfg, batch, T, heads=af.HEADS, dims=af.ATT_DIMS):
    from sudo_rm_rf_amd.engine import Plan
    tup = ("attentive_v3", 1) + tuple(cfg[f] for f in af.FIELDS[:6]) + (cfg["num_sources"], 1, (heads, dims))
    return Plan(tup, batch, T, torch.device("cpu"))


@pytest.mark.parametrize("name", sorted(af.CASES))
def test_schema_and_order_match_manifest(man, name):
    meta = man["cases"][name]
    cfg = meta["config"]
    assert cfg == af.CASES[name][0]
    sd = _model(cfg).state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == af.schema(cfg)
    U, D = cfg["num_blocks"], cfg["upsampling_depth"]
    assert len(sd) == 5 + U * (10 + 4 * D + 18 * (D - 1)) + 4
    assert sum(v.numel() for v in sd.values()) == meta["num_params"]
    assert af.level_lengths(cfg, meta["T"]) == meta["levels"] == af.LEVELS[name]


def test_every_resampler_has_a_table_of_its_own():
    sd = af.make_state_dict(af.TINY, af.CASES["attn3_tiny"][3])
    tables = [v for k, v in sd.items() if k.endswith("pos_enc.pe")]
    assert len(tables) == af.TINY["num_blocks"] * (af.TINY["upsampling_depth"] - 1) == 4
    assert all(not np.array_equal(a, b) for i, a in enumerate(tables) for b in tables[i + 1:])
    q, o = sd["sm.0.attentive_resamplers.0.mha.Q_proj.weight"], sd["sm.0.attentive_resamplers.0.mha.V_proj.weight"]
    assert 3.5 <= np.abs(q).max() / np.abs(o).max() <= 4.5          # Q / K four times wider than the other linear layers


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
    mha = m.sm[0].attentive_resamplers[0].mha
    assert (mha.n_heads, mha.d_model) == (man["block_heads"], man["block_att_dims"]) == (4, 256)
    assert m._config_tuple()[0] == "attentive_v3" and m._config_tuple()[10] == (4, 256)
    assert len(m.sm[0].attentive_resamplers) == ref["config"]["upsampling_depth"] - 1


def test_both_import_paths_resolve():
    import sudo_rm_rf.dnn.models.attentive_sudormrf_v3 as shim
    import sudo_rm_rf_amd.dnn.models.attentive_sudormrf_v3 as ours
    for n in ("_LayerNorm", "GlobLN", "ConvNormAct", "ConvNorm", "NormAct", "DilatedConv", "DilatedConvNorm", "PositionalEncoding",
              "MHAttentionLayer", "TransformerLayer", "ConditionalTransformerLayer", "AttentiveUConvBlock", "SuDORMRF"):
        assert getattr(shim, n) is getattr(ours, n)
    assert not hasattr(ours, "MHANormLayer")      # dead code in the reference: neither built nor mirrored
    import sudo_rm_rf_amd.dnn.models.attentive_sudormrf_v2 as v2
    assert ours.SuDORMRF is not v2.SuDORMRF and ours.AttentiveUConvBlock is not v2.AttentiveUConvBlock


def test_reference_pickle_unpickles_into_our_classes(man):
    from sudo_rm_rf_amd.dnn.models.attentive_sudormrf_v3 import AttentiveUConvBlock, ConditionalTransformerLayer, SuDORMRF
    meta = man["pickle"]
    path = os.path.join(af.GOLDEN, meta["file"])
    assert os.path.getsize(path) < (1 << 20)
    m = torch.load(path, weights_only=False)
    assert type(m) is SuDORMRF
    assert isinstance(m.sm[0], AttentiveUConvBlock) and isinstance(m.sm[0].attentive_resamplers[0], ConditionalTransformerLayer)
    torch.manual_seed(meta["seed"])
    want = _model(meta["config"]).state_dict()
    got = m.state_dict()
    assert list(got) == list(want)
    assert all(torch.equal(got[k], want[k]) for k in want)
    assert m._config_tuple()[0] == "attentive_v3" and not m.training
    # the pickle's own forward, restated: the golden the GPU test holds the unpickled module to
    gold = af.load_golden("attn3_pickle")["out"]
    wav = af.make_mixture(meta["batch"], meta["T"], meta["input_seed"])
    out = ar.forward(meta["config"], {k: v.numpy() for k, v in got.items()}, wav).numpy()
    assert np.abs(out - gold).max() <= 1e-5


def test_the_separate_list_route_is_per_utterance():
    from sudo_rm_rf_amd import pipeline
    m = _model(dict(af.TINY, out_channels=256))
    assert type(m).__name__ == "SuDORMRF" and not hasattr(m, "separate_ragged")
    assert pipeline.ragged_route(m, 32000) == "single"


def test_library_exports_the_new_symbols_and_keeps_its_abi():
    from sudo_rm_rf_amd import _lib, attention, ops
    lib = _lib.load()
    assert lib.srf_abi_version() == 19 == _lib.ABI_VERSION
    for name in ("srf_attentive_v3_plan_create", "srf_gln_apply_stats"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert C.sizeof(_lib.srf_config) == 10 * C.sizeof(C.c_int)      # the config did not grow
    assert _lib.VARIANT_ATTENTIVE == 3 and _lib.VARIANT_ATTENTIVE_V3 == 4
    assert hasattr(attention, "gln_apply_stats") and not hasattr(ops, "gln_apply_stats")


@pytest.mark.parametrize("name", sorted(af.CASES))
def test_plan_geometry_follows_the_padding_rule_and_the_convs_own_halving(man, name):
    meta = man["cases"][name]
    cfg = meta["config"]
    p = _plan(cfg, meta["batch"], meta["T"])
    assert p.padded_length == meta["padded_length"] == af.padded_length(cfg, meta["T"])
    assert p.frames == meta["padded_length"] // (cfg["enc_kernel_size"] // 2) == meta["levels"][0]
    assert p.num_params == len(af.schema(cfg))
    assert p.workspace_bytes > 0 and not p.ragged_supported
    assert _model(cfg).lcm == np.lcm(cfg["enc_kernel_size"] // 2, 2 ** cfg["upsampling_depth"])
    # every level length, as the reference's strided convolutions made them when the golden was generated: ceil halving
    lv = meta["levels"]
    assert len(lv) == cfg["upsampling_depth"] and all(lv[k + 1] == -(-lv[k] // 2) for k in range(len(lv) - 1))


def test_lengths_the_v2_plan_refuses_are_taken():
    """K = 9, D = 3: 26 frames are no multiple of 4 -- v2's upsample-and-add cannot run there, v3 has none."""
    from sudo_rm_rf_amd.engine import Plan
    from sudo_rm_rf_amd._lib import SrfError
    cfg = af.TINY_K9
    tail = tuple(cfg[f] for f in af.FIELDS[:6]) + (cfg["num_sources"], 1, (4, 256))
    with pytest.raises(SrfError, match="multiple of 2"):
        Plan(("attentive", 1) + tail, 2, 100, torch.device("cpu"))
    assert Plan(("attentive_v3", 1) + tail, 2, 100, torch.device("cpu")).frames == 26
    assert _plan(af.TINY_D1, 2, 333).frames == 34                       # depth 1 is legal


def test_plan_refusals_name_their_argument():
    from sudo_rm_rf_amd import _lib
    from sudo_rm_rf_amd._lib import SrfError
    # D = 2, K = 21: level 1 = ceil(frames / 2) = ceil(T / 20); the table is added to the ANSWERING side, so 10000 frames pass
    assert _plan(dict(af.TINY, upsampling_depth=2), 1, 100000).frames == 10000
    with pytest.raises(SrfError, match=r"5001 positions on level 1.* 5000"):
        _plan(dict(af.TINY, upsampling_depth=2), 1, 100020)
    assert _plan(af.TINY_D1, 1, 100020).frames == 10002                 # (no resampler, no table, no limit)
    with pytest.raises(SrfError, match="n_heads = 0"):
        _plan(af.TINY, 1, 1000, heads=0)
    with pytest.raises(SrfError, match="att_dims = -1"):
        _plan(af.TINY, 1, 1000, dims=-1)
    with pytest.raises(SrfError, match="enc_kernel_size must be odd"):
        _plan(dict(af.TINY, enc_kernel_size=20), 1, 1000)
    with pytest.raises(SrfError, match="upsampling_depth 9 unsupported"):
        _plan(dict(af.TINY, upsampling_depth=9), 1, 100000)
    with pytest.raises(SrfError, match="upsampling_depth 0 unsupported"):
        _plan(dict(af.TINY, upsampling_depth=0), 1, 1000)
    lib = _lib.load()
    cfg = _lib.srf_config(variant=_lib.VARIANT_ATTENTIVE_V3, in_audio_channels=1, out_channels=32, in_channels=64, num_blocks=2,
                          upsampling_depth=3, enc_kernel_size=21, enc_num_basis=64, num_sources=2, group_size=1)
    h = C.c_void_p()
    assert lib.srf_plan_create(C.byref(cfg), 1, 1000, C.byref(h)) == -1 and b"srf_attentive_v3_plan_create" in lib.srf_last_error()
    cfg.in_audio_channels = 2
    assert lib.srf_attentive_v3_plan_create(C.byref(cfg), 4, 256, 1, 1000, C.byref(h)) == -1
    assert b"in_audio_channels" in lib.srf_last_error() and not h.value
    cfg.in_audio_channels, cfg.group_size = 1, 16
    assert lib.srf_attentive_v3_plan_create(C.byref(cfg), 4, 256, 1, 1000, C.byref(h)) == -1
    assert b"group_size" in lib.srf_last_error() and not h.value
    cfg.group_size = 1
    assert lib.srf_attentive_v3_plan_create(C.byref(cfg), 4, 256, 0, 1000, C.byref(h)) == -1 and b"batch" in lib.srf_last_error()


def test_training_and_ragged_entry_points_refuse_the_plan():
    from sudo_rm_rf_amd import _lib
    p = _plan(af.TINY, 2, 1000)
    lib = _lib.load()
    assert lib.srf_plan_ragged_supported(p.handle) == 0 and lib.srf_plan_ragged_workspace_bytes(p.handle) == 0
    assert lib.srf_train_saved_bytes(p.handle) == 0 and lib.srf_train_scratch_bytes(p.handle) == 0
    rc = lib.srf_forward_train(p.handle, None, 0, None, None, None, 0, None, 0, None)
    assert rc == -1 and b"attentive v3" in lib.srf_last_error()
    for fn in ("srf_backward", "srf_backward_wav"):
        args = [p.handle, None, None, 0, None, None, None, 0, None, 0] + ([C.c_void_p(16)] if fn.endswith("wav") else []) + [None]
        assert getattr(lib, fn)(*args) == -1 and b"attentive v3" in lib.srf_last_error()
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
        # depth 1 has no resampler, hence no dropout to refuse: train() mode gets as far as the device check
        with pytest.raises(SrfError, match="MI355X"):
            _model(af.TINY_D1)(torch.zeros(1, 1, 200))


@pytest.fixture(scope="module")
def restated():
    """name -> (fp64 output, resampler taps) of tests/attentive_v3_ref.py on the golden's weights and input"""
    out = {}
    for name, (cfg, _, _, wseed, _) in af.CASES.items():
        taps = []
        y = ar.forward(cfg, af.make_state_dict(cfg, wseed), af.make_input(name), torch.float64, taps)
        out[name] = (y.numpy(), taps)
    return out


@pytest.mark.parametrize("name", sorted(af.CASES))
def test_restatement_agrees_with_the_reference(man, restated, name):
    gold = af.load_golden(name)
    y, taps = restated[name]
    err = float(np.abs(y - gold["out"]).max())
    amax = float(np.abs(gold["out"]).max())
    print("%s: max|attentive_v3_ref fp64 - reference fp32| = %.3e, max|out| %.3f" % (name, err, amax))
    assert y.shape == gold["out"].shape and err <= 1e-5
    assert 0.1 <= amax <= 10.0 and amax == man["cases"][name]["max_abs_out"]
    cfg = af.CASES[name][0]
    assert len(taps) == cfg["num_blocks"] * (cfg["upsampling_depth"] - 1)
    if name == "attn3_tiny":
        # the first resampler block 0 runs is attentive_resamplers[0]: the DEEPEST pair, 52 positions ask 26
        q, v, z = taps[0]
        assert q.shape[-1] == 52 and v.shape[-1] == 26
        for got, key in ((q, "res_q"), (v, "res_v"), (z, "res_out")):
            assert got.shape == gold[key].shape and np.abs(got.numpy() - gold[key]).max() <= 1e-5


# ---- the configurations without a golden: the conditions the GPU tests of tests/test_gpu_attentive_v3_walk.py rest on ------------
def _packable(lib, cfg, heads, dims):
    """(Cout, Cin) of every 1x1 weight srf_attentive_v3_plan_create gives a packed image, in the order it adds them"""
    B, C, N, S = cfg["out_channels"], cfg["in_channels"], cfg["enc_num_basis"], cfg["num_sources"]
    hd = heads * dims
    shapes = [(B, N)]
    for _ in range(cfg["num_blocks"]):
        shapes += [(C, B), (B, C)]
        shapes += [(hd, C), (2 * hd, C), (C, hd), (C, C)] * (cfg["upsampling_depth"] - 1)
    shapes.append((S * N, B))
    return [s for s in shapes if lib.srf_packed_pw_weight_bytes(*s) > 0]


def test_wide3_levels_and_tile_counts():
    cfg, lv = af.WIDE3, af.level_lengths(af.WIDE3, af.WIDE3_T)
    assert lv == af.WIDE3_LEVELS == [528, 264, 132] and all(n % 4 == 0 for n in lv)
    assert cfg["num_blocks"] >= 2 and cfg["upsampling_depth"] >= 3          # block index and resampler index both vary
    C_, B, hd = cfg["in_channels"], cfg["out_channels"], af.HEADS * af.ATT_DIMS
    # the library's test (srf_pwconv.hip, pw256_fills_chip): Bt * ceil(Cout / 256) * ceil(L / 128) >= CUs
    tiles = lambda cout, n: -(-cout // 256) * -(-n // 128)
    got = {"proj_1x1": tiles(C_, lv[0]), "mask": tiles(cfg["num_sources"] * cfg["enc_num_basis"], lv[0])}
    for r in range(2):                                                       # resampler r: level 1 - r asks level 2 - r
        lq, lk = lv[1 - r], lv[2 - r]
        got[r] = {"Q": tiles(hd, lq), "KV": tiles(2 * hd, lk), "O": tiles(C_, lq), "ffn": tiles(C_, lq)}
    assert got == af.WIDE3_TILES
    assert got[0] == {"Q": 12, "KV": 16, "O": 6, "ffn": 6} and got[1] == {"Q": 20, "KV": 24, "O": 10, "ffn": 10}
    assert min(min(got[0].values()), min(got[1].values()), got["proj_1x1"], got["mask"]) == af.WIDE3_MIN_TILES == 6
    assert all(af.tiles_256(1, c, n) == tiles(c, n) for c in (192, 256, 512, 2048) for n in lv)
    assert -(-256 // af.WIDE3_MIN_TILES) == 43                                # the chip batch on 256 CUs
    from sudo_rm_rf_amd import _lib
    assert len(_packable(_lib.load(), cfg, af.HEADS, af.ATT_DIMS)) == 2 * (1 + 4 * 2) + 1       # every one but B-row outputs


def test_many_has_more_packable_weights_than_one_packing_launch_holds():
    from sudo_rm_rf_amd import _lib
    cfg, (heads, dims) = af.MANY, af.MANY_HEADS
    lv = af.level_lengths(cfg, af.MANY_T)
    assert lv == af.MANY_LEVELS == [64, 32, 16, 8, 4] and all(n % 4 == 0 for n in lv)
    packs = _packable(_lib.load(), cfg, heads, dims)
    per_block = 1 + 4 * (cfg["upsampling_depth"] - 1)
    assert len(packs) == cfg["num_blocks"] * per_block == 102 > af.MANY_PACK_CHUNK == 96
    # the first launch is full; the second holds images 96 .. 101: all four of the last block's last resampler (from index 98) and
    # O_proj and ffn of the one before
    assert af.MANY_PACK_CHUNK < len(packs) <= 2 * af.MANY_PACK_CHUNK
    assert (cfg["num_blocks"] - 1) * per_block + 1 + 4 * (cfg["upsampling_depth"] - 2) == 98 >= af.MANY_PACK_CHUNK
    # one 256 x 128 tile per example ([K; V]: two) at every level: a batch of as many examples as CUs fills the chip
    assert all(af.tiles_256(1, cout, n) == (2 if cout == 2 * heads * dims else 1) for cout, _ in packs for n in lv)


def test_narrow_is_off_every_grid():
    cfg, (heads, dims) = af.NARROW, af.NARROW_HEADS
    hd, C_ = heads * dims, cfg["in_channels"]
    assert af.level_lengths(cfg, af.NARROW_T) == af.NARROW_LEVELS == [26, 13, 7]
    assert (2 * hd * C_) % 64 != 0 and (2 * hd) % 64 != 0          # padded [K; V] weight and bias sections
    assert (hd * 7) % 4 != 0 and (hd * 13) % 4 != 0                 # V's base kv + HD Lk is off the 16-byte grid
    assert C_ < 32 and cfg["out_channels"] < 32                      # below every MFMA GEMM's minimum: the scalar conv kernel
    assert dims % 16 != 0                                                    # the generic attention
    assert (2 * 16) % 64 != 0 and (16 * 7) % 4 == 0                          # (1, 16): a padded bias section, MFMA attention


@pytest.mark.parametrize("which", ["WIDE3", "MANY", "NARROW", "NARROW_1x16"])
def test_plans_of_the_new_configurations(which):
    from sudo_rm_rf_amd import _lib
    cfg, T, (heads, dims), wseed = {"WIDE3": (af.WIDE3, af.WIDE3_T, (af.HEADS, af.ATT_DIMS), af.WIDE3_WSEED),
                                    "MANY": (af.MANY, af.MANY_T, af.MANY_HEADS, af.MANY_WSEED),
                                    "NARROW": (af.NARROW, af.NARROW_T, af.NARROW_HEADS, af.NARROW_WSEED),
                                    "NARROW_1x16": (af.NARROW, af.NARROW_T, (1, 16), af.NARROW_WSEED)}[which]
    sd = af.with_heads(af.make_state_dict(cfg, wseed), cfg, heads, dims, wseed)
    p = _plan(cfg, 3, T, heads, dims)
    assert p.num_params == _lib.load().srf_plan_num_params(p.handle) == len(sd) == len(af.schema(cfg))
    assert p.frames == af.level_lengths(cfg, T)[0] and p.workspace_bytes > 0
    a = "sm.1.attentive_resamplers.1.mha."
    assert sd[a + "K_proj.weight"].shape == (heads * dims, cfg["in_channels"]) and sd[a + "V_proj.bias"].shape == (heads * dims,)
    assert sd[a + "O_proj.weight"].shape == (cfg["in_channels"], heads * dims)
    assert np.abs(sd[a + "O_proj.weight"]).max() <= 1.0 / np.sqrt(heads * dims)


def test_with_heads_cuts_rows_and_keeps_the_rest():
    sd = af.make_state_dict(af.TINY, 5)
    cut = af.with_heads(sd, af.TINY, 2, 24, 6)
    assert list(cut) == list(sd)
    for k in sd:
        if ".mha.O_proj.weight" in k:
            assert cut[k].shape == (64, 48) and cut[k].dtype == np.float32
        elif ".mha." in k and "O_proj" not in k:
            assert np.array_equal(cut[k], sd[k][:48]) and cut[k].flags["C_CONTIGUOUS"]
        else:
            assert cut[k] is sd[k]
    assert sd["sm.0.attentive_resamplers.0.mha.Q_proj.weight"].shape == (1024, 64)          # the source is untouched
    a, b = (af.with_heads(sd, af.TINY, 2, 24, s)["sm.1.attentive_resamplers.0.mha.O_proj.weight"] for s in (6, 6))
    assert np.array_equal(a, b)
    o = [v for k, v in cut.items() if k.endswith("O_proj.weight")]
    assert all(not np.array_equal(x, y) for i, x in enumerate(o) for y in o[i + 1:])


@pytest.mark.parametrize("D,T", sorted(af.ONE_POSITION))
def test_levels_of_one_position(D, T):
    """T < K and one or two frames: the plan takes them, the level list ends in 1s, and the restatement is finite with
    max |out| inside the fixtures' [0.1, 10] (the decoder factor of the fixture)."""
    levels, factor = af.ONE_POSITION[(D, T)]
    cfg, sd, wav = af.one_position_case(D, T)
    assert af.level_lengths(cfg, T) == levels and levels[-1] == 1 and T < cfg["enc_kernel_size"] * 4
    variants = [(af.HEADS, af.ATT_DIMS, sd)]
    if (D, T) == (3, 8):
        variants += [(h, d, af.with_heads(sd, cfg, h, d, af.ONE_POSITION_WSEED + h)) for h, d in ((3, 16), (2, 24))]
    for heads, dims, w in variants:
        p = _plan(cfg, 2, T, heads, dims)
        assert p.frames == levels[0] and p.num_params == len(w)
        y = ar.forward(cfg, w, wav, torch.float64, heads=heads).numpy()
        amax = float(np.abs(y).max())
        print("D %d, T %d, %d x %d, decoder x %g: max|out| %.3f" % (D, T, heads, dims, factor, amax))
        assert y.shape == (2, 2, T) and np.isfinite(y).all() and 0.1 <= amax <= 10.0


def test_grid_case_of_the_kernel_modes_is_on_the_mfma_grid():
    lv = af.level_lengths(af.TINY, af.GRID_T)
    assert lv == af.GRID_LEVELS == [112, 56, 28] and all(n % 4 == 0 for n in lv)
