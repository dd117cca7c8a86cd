"""Original SuDoRM-RF on the host: module schema, seeded weights and the reference's pickle against fixtures made by the reference
(tools/make_golden_original.py), the Toeplitz form of the mask layer against torch's conv2d, the library's new symbols, the
plan's geometry and refusals, and the torch restatement tests/original_ref.py against every golden.  No GPU needed."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import original_fixtures as of
from tests import original_ref as orf


@pytest.fixture(scope="module")
def man():
    return of.load_manifest()


def _model(cfg):
    from sudo_rm_rf_amd.dnn.models.sudormrf import SuDORMRF
    return SuDORMRF(**cfg)


def _plan(cfg, batch, T):
    from sudo_rm_rf_amd.engine import Plan
    tup = ("original", 1, cfg["out_channels"], cfg["in_channels"], cfg["num_blocks"], cfg["upsampling_depth"], cfg["enc_kernel_size"],
           cfg["enc_num_basis"], cfg["num_sources"], 1)
    return Plan(tup, batch, T, torch.device("cpu"))


@pytest.mark.parametrize("name", sorted(of.CASES))
def test_schema_and_order_match_manifest(man, name):
    meta = man["cases"][name]
    cfg = meta["config"]
    assert cfg == of.CASES[name][0] and (meta["batch"], meta["T"]) == of.CASES[name][1:3]
    sd = _model(cfg).state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == of.schema(cfg) == [(k, tuple(s)) for k, s in meta["schema"]]
    U, D = cfg["num_blocks"], cfg["upsampling_depth"]
    reshape = cfg["out_channels"] != cfg["enc_num_basis"]
    assert len(sd) == 6 + U * (15 + 4 * D) + (2 if reshape else 0) + 6 == meta["num_tensors"]
    assert ("reshape_before_masks.weight" in sd) == reshape
    assert list(sd)[-2:] == ["ln_mask_in.weight", "ln_mask_in.bias"]
    assert sum(v.numel() for v in sd.values()) == meta["num_params"]


def test_the_case_without_reshape_is_two_tensors_shorter():
    assert len(of.schema(of.SAME)) == len(of.schema(of.TINY)) - 2
    m = _model(of.SAME)
    assert not hasattr(m, "reshape_before_masks") and hasattr(_model(of.TINY), "reshape_before_masks")
    assert hasattr(m, "ln_mask_in") and m.sm[0].proj_1x1.act.weight.shape == (64,)      # one slope per channel


def test_fixture_weights_leave_no_identity():
    sd = of.make_state_dict(of.TINY, of.CASES["orig_tiny"][3])
    for k, v in sd.items():
        assert v.dtype == np.float32 and np.unique(v).size > 1 or v.size == 1, k
        if ".act." in k:
            assert 0.05 < v.min() and v.max() < 0.45 and v.size in (32, 64)


@pytest.mark.parametrize("tag", sorted(of.DIGEST_CONFIGS))
def test_same_seed_gives_the_reference_weights(man, tag):
    ref = man["digests"][tag]
    torch.manual_seed(ref["seed"])
    m = _model(ref["config"])
    got = [[k, list(v.shape), hashlib.sha256(v.detach().contiguous().numpy().tobytes()).hexdigest()]
           for k, v in m.state_dict().items()]
    assert got == ref["state_dict"]
    for a, v in ref["attributes"].items():
        assert getattr(m, a) == v, a
    assert m._config_tuple()[0] == "original"


def test_both_import_paths_resolve():
    import sudo_rm_rf.dnn.models.sudormrf as shim
    import sudo_rm_rf_amd.dnn.models.sudormrf as ours
    for n in ("ConvNormAct", "ConvNorm", "NormAct", "DilatedConv", "DilatedConvNorm", "UBlock", "SuDORMRF"):
        assert getattr(shim, n) is getattr(ours, n)
    import sudo_rm_rf_amd.dnn.models.improved_sudormrf as improved
    assert ours.SuDORMRF is not improved.SuDORMRF


def test_state_dict_round_trip_keeps_ln_mask_in():
    sd = {k: torch.from_numpy(v) for k, v in of.make_state_dict(of.TINY, 5).items()}
    m = _model(of.TINY)
    m.load_state_dict(sd)                                   # strict: every key of the checkpoint, ln_mask_in included
    back = m.state_dict()
    assert list(back) == list(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    with pytest.raises(RuntimeError, match="reshape_before_masks"):
        _model(of.SAME).load_state_dict({k: torch.from_numpy(v) for k, v in of.make_state_dict(of.TINY, 5).items()})


def test_reference_pickle_unpickles_into_our_classes(man):
    from sudo_rm_rf_amd.dnn.models.sudormrf import SuDORMRF, UBlock
    meta = man["pickle"]
    path = os.path.join(of.GOLDEN, meta["file"])
    assert os.path.getsize(path) < (1 << 20)
    m = torch.load(path, weights_only=False)
    assert type(m) is SuDORMRF and isinstance(m.sm[0], UBlock)
    got = m.state_dict()
    assert [(k, tuple(v.shape)) for k, v in got.items()] == of.schema(meta["config"])
    assert "ln_mask_in.weight" in got and m._config_tuple()[0] == "original" and not m.training
    # the pickle's own forward, restated: the golden the GPU test holds the unpickled module to
    gold = of.load_golden("orig_pickle")["out"]
    wav = of.make_mixture(meta["batch"], meta["T"], meta["input_seed"])
    out = orf.forward(meta["config"], {k: v.numpy() for k, v in got.items()}, wav).numpy()
    assert np.abs(out - gold).max() <= 1e-5
    assert 0.1 <= meta["max_abs_out"] <= 10.0


def test_the_separate_list_route_is_per_utterance():
    from sudo_rm_rf_amd import pipeline
    m = _model(dict(of.TINY, out_channels=256))
    assert type(m).__name__ == "SuDORMRF" and not hasattr(m, "separate_ragged")
    assert pipeline.ragged_route(m, 32000) == "single"


@pytest.mark.parametrize("N", [4, 6, 64])
@pytest.mark.parametrize("S", [1, 2, 3])
def test_toeplitz_weight_is_the_mask_convolution(N, S):
    rng = np.random.default_rng(100 * N + S)
    w = rng.standard_normal((S, 1, N + 1, 1))
    b = rng.standard_normal((S,))
    x = rng.standard_normal((3, N, 7))
    want = F.conv2d(torch.from_numpy(x).unsqueeze(1), torch.from_numpy(w), torch.from_numpy(b), padding=(N - N // 2, 0)).numpy()
    assert want.shape == (3, S, N, 7)                       # N rows for even N
    tz, tb = of.toeplitz(w, b)
    assert tz.shape == (S * N, N) and tz.dtype == np.float64 and tb.shape == (S * N,)
    got = (np.einsum("rn,bnl->brl", tz, x) + tb[None, :, None]).reshape(3, S, N, 7)
    assert np.abs(got - want).max() <= 1e-12
    assert all(np.all(np.diag(tz[s * N:(s + 1) * N]) == w[s, 0, N - N // 2, 0]) for s in range(S))      # a copy of the taps


def test_odd_basis_gives_the_reference_one_row_too_many():
    """why odd enc_num_basis is refused: the mask layer then has N + 1 rows and `p * s` cannot broadcast"""
    z = F.conv2d(torch.zeros(1, 1, 5, 3), torch.zeros(2, 1, 6, 1), padding=(5 - 5 // 2, 0))
    assert z.shape[2] == 6


def test_expanded_decoder_weight_is_the_grouped_transposed_convolution():
    rng = np.random.default_rng(3)
    S, N, K = 3, 4, 9
    w = rng.standard_normal((S * N, 1, K))
    v = torch.from_numpy(rng.standard_normal((2, S * N, 6)))
    want = F.conv_transpose1d(v, torch.from_numpy(w), stride=K // 2, padding=K // 2, output_padding=K // 2 - 1, groups=S)
    got = F.conv_transpose1d(v, torch.from_numpy(of.expand_decoder(w, S)), stride=K // 2, padding=K // 2, output_padding=K // 2 - 1)
    assert (got - want).abs().max() <= 1e-12


def test_library_exports_the_new_symbols_and_keeps_its_abi():
    from sudo_rm_rf_amd import _lib, ops, original
    lib = _lib.load()
    assert lib.srf_abi_version() == 19 == _lib.ABI_VERSION
    for name in ("srf_original_plan_create", "srf_gln_apply_c", "srf_encoder_bias_relu", "srf_mask_weight_fill", "srf_softmax_mask",
                 "srf_decoder_weight_expand", "srf_bias_rescale"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert C.sizeof(_lib.srf_config) == 10 * C.sizeof(C.c_int)      # the config did not grow
    assert _lib.VARIANT_ORIGINAL == 5 and _lib.VARIANT_ATTENTIVE_V3 == 4
    assert hasattr(original, "gln_apply_c") and not hasattr(ops, "gln_apply_c")
    assert original.MAX_SOURCES >= 9


@pytest.mark.parametrize("name", sorted(of.CASES))
def test_plan_geometry_follows_the_padding_rule(man, name):
    meta = man["cases"][name]
    cfg = meta["config"]
    p = _plan(cfg, meta["batch"], meta["T"])
    assert p.padded_length == meta["padded_length"] == of.padded_length(cfg, meta["T"])
    assert p.frames == meta["frames"] == of.frames(cfg, meta["T"]) == meta["padded_length"] // (cfg["enc_kernel_size"] // 2)
    assert p.num_params == len(of.schema(cfg)) == meta["num_tensors"]
    assert p.workspace_bytes > 0 and not p.ragged_supported
    assert _model(cfg).lcm == np.lcm(cfg["enc_kernel_size"] // 2, 2 ** cfg["upsampling_depth"])
    U, D = cfg["num_blocks"], cfg["upsampling_depth"]
    reshape = cfg["out_channels"] != cfg["enc_num_basis"]
    lib = __import__("sudo_rm_rf_amd._lib", fromlist=["x"]).load()
    N, B, C_, S = cfg["enc_num_basis"], cfg["out_channels"], cfg["in_channels"], cfg["num_sources"]
    pack = any(lib.srf_packed_pw_weight_bytes(*s) for s in ((B, N), (C_, B), (B, C_), (N, B), (S * N, N)))
    # zero | mask weight, decoder weight | [pack] | encoder, l1 | per block 6 + the pyramid (3 launches fused, D + 1 level by level)
    # | [reshape] | mask GEMM, softmax | decoder (4) | bias
    pyr = 3 if lib.srf_pyramid_supported(C_, p.frames, D) else D + 1
    assert p.num_launches == 3 + (1 if pack else 0) + 2 + U * (pyr + 6) + (1 if reshape else 0) + 2 + 4 + 1
    assert bool(lib.srf_pyramid_supported(C_, p.frames, D)) == (name in ("orig_default_u2", "orig_recipe_u1"))
    assert p.frames % (1 << (D - 1)) == 0


def test_a_length_that_is_already_a_multiple_is_not_padded():
    assert _plan(of.TINY, 1, 1040).padded_length == 1040 and _plan(of.TINY, 1, 1041).padded_length == 1080
    assert _plan(of.D1, 2, 333).frames == 34                            # depth 1 is legal


def test_plan_refusals_name_their_argument():
    from sudo_rm_rf_amd import _lib
    from sudo_rm_rf_amd._lib import SrfError
    with pytest.raises(SrfError, match=r"enc_num_basis = 63 is odd.*reference"):
        _plan(dict(of.TINY, enc_num_basis=63), 1, 1000)
    with pytest.raises(SrfError, match="enc_kernel_size must be odd"):
        _plan(dict(of.TINY, enc_kernel_size=20), 1, 1000)
    with pytest.raises(SrfError, match=r"enc_kernel_size must be odd and >= 3 \(got 1\)"):
        _plan(dict(of.TINY, enc_kernel_size=1), 1, 1000)
    with pytest.raises(SrfError, match="upsampling_depth 9 unsupported"):
        _plan(dict(of.TINY, upsampling_depth=9), 1, 100000)
    with pytest.raises(SrfError, match="upsampling_depth 0 unsupported"):
        _plan(dict(of.TINY, upsampling_depth=0), 1, 1000)
    # K = 9, D = 3, T = 100: 26 frames; the reference's own upsample-and-add raises there (tests/original_fixtures.py)
    with pytest.raises(SrfError, match=r"26 frames are not a multiple of 2\^\(D-1\)"):
        _plan(of.S3_K9, 2, of.S3_K9_REFUSED_T)
    assert _plan(of.S3_K9, 2, 108).frames == 28
    with pytest.raises(SrfError, match=r"num_sources = 17 exceeds SRF_SOFTMAX_MASK_MAX_SOURCES"):
        _plan(dict(of.TINY, num_sources=17), 1, 1000)
    assert _plan(dict(of.TINY, num_sources=9), 1, 1000).num_params == len(of.schema(of.TINY))
    with pytest.raises(SrfError, match="batch 65536 too large"):
        _plan(of.TINY, 65536, 1000)
    lib = _lib.load()
    cfg = _lib.srf_config(variant=_lib.VARIANT_ORIGINAL, in_audio_channels=1, out_channels=32, in_channels=64, num_blocks=2,
                          upsampling_depth=3, enc_kernel_size=21, enc_num_basis=64, num_sources=2, group_size=1)
    h = C.c_void_p()
    assert lib.srf_plan_create(C.byref(cfg), 1, 1000, C.byref(h)) == -1 and b"srf_original_plan_create" in lib.srf_last_error()
    cfg.in_audio_channels = 2
    assert lib.srf_original_plan_create(C.byref(cfg), 1, 1000, C.byref(h)) == -1
    assert b"in_audio_channels" in lib.srf_last_error() and not h.value
    cfg.in_audio_channels, cfg.group_size = 1, 16
    assert lib.srf_original_plan_create(C.byref(cfg), 1, 1000, C.byref(h)) == -1
    assert b"group_size" in lib.srf_last_error() and not h.value
    cfg.group_size = 1
    assert lib.srf_original_plan_create(C.byref(cfg), 0, 1000, C.byref(h)) == -1 and b"batch" in lib.srf_last_error()


def test_training_and_ragged_entry_points_refuse_the_plan():
    from sudo_rm_rf_amd import _lib
    p = _plan(of.TINY, 2, 1000)
    lib = _lib.load()
    assert lib.srf_plan_ragged_supported(p.handle) == 0 and lib.srf_plan_ragged_workspace_bytes(p.handle) == 0
    assert lib.srf_train_saved_bytes(p.handle) == 0 and lib.srf_train_scratch_bytes(p.handle) == 0
    rc = lib.srf_forward_train(p.handle, None, 0, None, None, None, 0, None, 0, None)
    assert rc == -1 and b"original" in lib.srf_last_error()
    for fn in ("srf_backward", "srf_backward_wav"):
        args = [p.handle, None, None, 0, None, None, None, 0, None, 0] + ([C.c_void_p(16)] if fn.endswith("wav") else []) + [None]
        assert getattr(lib, fn)(*args) == -1 and b"original" in lib.srf_last_error()
    lens = (C.c_int * 2)(1000, 900)
    table = (C.c_void_p * 1)(16)
    one = C.c_void_p(256)
    rc = lib.srf_forward_ragged(p.handle, table, 1, one, lens, one, one, 0, None)
    assert rc == -1 and b"original" in lib.srf_last_error()
    rc = lib.srf_separate_ragged(p.handle, table, 1, one, lens, one, one, 0, one, 0, None)
    assert rc == -1 and b"original" in lib.srf_last_error()


def test_kernel_entry_points_refuse_before_any_launch():
    """argument checks that come before a kernel's launch need no GPU: bad pointers and ranges never reach the device"""
    from sudo_rm_rf_amd import _lib
    lib = _lib.load()
    one, two = C.c_void_p(256), C.c_void_p(512)
    assert lib.srf_softmax_mask(one, two, C.c_void_p(1024), 1, 17, 4, 4, None) == -1 and b"num_sources = 17" in lib.srf_last_error()
    assert lib.srf_softmax_mask(one, two, C.c_void_p(1024), 1, 0, 4, 4, None) == -1
    assert lib.srf_softmax_mask(one, two, two, 1, 2, 4, 4, None) == -1 and b"must not be enc" in lib.srf_last_error()
    assert lib.srf_mask_weight_fill(one, one, two, two, 5, 2, None) == -1 and b"even" in lib.srf_last_error()
    assert lib.srf_encoder_bias_relu(one, one, one, two, None, 1, 100, 4, 8, 10, None, None) == -1 and b"odd" in lib.srf_last_error()
    n = _lib.srf_norm()
    n.sums, n.gamma, n.beta = 256, 256, 256
    assert lib.srf_gln_apply_c(one, C.byref(n), None, None, one, None, 1, 4, 4, None) == -1 and b"y must not overlap" in lib.srf_last_error()
    # a y that overlaps x only partly (16 floats each, 8 floats apart), and one that overlaps the addend
    assert lib.srf_gln_apply_c(one, C.byref(n), None, None, C.c_void_p(256 + 32), None, 1, 4, 4, None) == -1
    assert b"y must not overlap" in lib.srf_last_error()
    assert lib.srf_gln_apply_c(one, C.byref(n), None, C.c_void_p(1024 + 60), C.c_void_p(1024), None, 1, 4, 4, None) == -1
    assert b"y must not overlap" in lib.srf_last_error()
    assert lib.srf_gln_apply_c(C.c_void_p(258), C.byref(n), None, None, two, None, 1, 4, 4, None) == -1
    assert b"float-aligned" in lib.srf_last_error()
    n.sums = None
    assert lib.srf_gln_apply_c(one, C.byref(n), None, None, two, None, 1, 4, 4, None) == -1 and b"statistics" in lib.srf_last_error()
    assert lib.srf_bias_rescale(one, None, None, None, 0, 1, 2, 10, None) == -1


def test_python_refusals_need_no_gpu():
    from sudo_rm_rf_amd._lib import SrfError
    m = _model(of.TINY)
    with pytest.raises(RuntimeError, match=r"torch\.no_grad\(\)"):        # train() mode with gradients: would need a backward
        m(torch.zeros(1, 1, 200))
    m.eval()
    with pytest.raises(RuntimeError, match=r"inference forward only.*torch\.no_grad\(\)"):
        m(torch.zeros(1, 1, 200))
    with torch.no_grad():
        with pytest.raises(SrfError, match="MI355X"):
            m(torch.zeros(1, 1, 200))
        with pytest.raises(NotImplementedError, match="ragged"):
            m.forward_ragged(torch.zeros(2, 1, 200), [200, 100])
        with pytest.raises(RuntimeError, match=r"\[batch, 1, time\]"):
            m(torch.zeros(1, 2, 200))
        with pytest.raises(RuntimeError, match="MI355X"):
            m.sm[0](torch.zeros(1, 32, 8))


@pytest.fixture(scope="module")
def restated():
    out = {}
    for name, (cfg, _, _, wseed, _) in of.CASES.items():
        taps = {}
        y = orf.forward(cfg, of.make_state_dict(cfg, wseed), of.make_input(name), torch.float64, taps)
        out[name] = (y.numpy(), taps)
    return out


@pytest.mark.parametrize("name", sorted(of.CASES))
def test_restatement_agrees_with_the_reference(man, restated, name):
    gold = of.load_golden(name)
    y, taps = restated[name]
    err = float(np.abs(y - gold["out"]).max())
    amax = float(np.abs(gold["out"]).max())
    print("%s: max|original_ref fp64 - reference fp32| = %.3e, max|out| %.3f" % (name, err, amax))
    assert y.shape == gold["out"].shape and err <= 1e-5
    assert 0.1 <= amax <= 10.0 and amax == man["cases"][name]["max_abs_out"]
    if name == "orig_tiny":
        assert sorted(gold) == ["block0", "out", "z"]
        assert taps["block0"].shape == gold["block0"].shape == (2, 32, 104)
        assert np.abs(taps["block0"].numpy() - gold["block0"]).max() <= 1e-5
        assert taps["z"].shape == gold["z"].shape == (2, 2, 64, 104) and np.abs(taps["z"].numpy() - gold["z"]).max() <= 1e-5


def test_ln_mask_in_changes_nothing():
    cfg, _, _, wseed, _ = of.CASES["orig_tiny_short"]
    sd = of.make_state_dict(cfg, wseed)
    wav = of.make_input("orig_tiny_short")
    a = orf.forward(cfg, sd, wav)
    sd2 = dict(sd, **{"ln_mask_in.weight": sd["ln_mask_in.weight"] * 3, "ln_mask_in.bias": sd["ln_mask_in.bias"] + 1})
    assert torch.equal(a, orf.forward(cfg, sd2, wav))


def test_separate_recipe_of_the_restatement():
    cfg, _, _, wseed, _ = of.CASES["orig_tiny_short"]
    sd = of.make_state_dict(cfg, wseed)
    mix = of.make_mixture(2, 50, 77) * 3.0 + 0.5
    est = orf.separate(cfg, sd, mix, mixture_consistency=True)
    x = torch.from_numpy(mix).double()
    norm = (x - x.mean(-1, keepdim=True)) / (x.std(-1, keepdim=True) + 1e-9)
    assert (est.sum(1, keepdim=True) - norm).abs().max() <= 1e-12          # what mixture consistency promises
