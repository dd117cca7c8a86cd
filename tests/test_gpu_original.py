"""Original SuDoRM-RF on the GPU: the reference's goldens through the module and through the raw C ABI, the stored block output
and mask logits of orig_tiny, the reference's pickle, a batch of distinct examples, the separate() recipe with and without mixture
consistency, a configuration whose 1x1 convs take the 256 x 128 MFMA kernel, a guarded-arena run of srf_forward, and the refusals.
References: the stored reference outputs (tests/golden/orig_*.npz) and, where there is no golden, tests/original_ref.py in fp64
(pinned to the goldens within 1e-5 by tests/test_original_host.py).  Bar: the project's 1e-4 max-abs.
Measured on an MI355X (256 CUs): goldens 1.2e-7 .. 2.5e-6 (module and C ABI alike; orig_default_u2 1.2e-6 with the fused pyramid,
1.3e-6 level by level), block 0 of orig_tiny 4.8e-5 through the walk / 3.8e-5 through UBlock.forward at max |ref| 4.9, its mask
logits 3.3e-5 at max |z| 5.5, pickle 4.8e-7, distinct examples <= 3.9e-6, separate <= 4.1e-6 with and without mixture consistency,
the wide case at batch 64 2.4e-6 with every conv but the decoder's frame GEMM on pw_conv_x3p, the arena runs 2.4e-6 / 1.0e-6."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from tests import original_fixtures as of
from tests import original_ref as orf
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
    from sudo_rm_rf_amd.dnn.models.sudormrf import SuDORMRF
    m = SuDORMRF(**cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _case(name):
    """(model on the GPU, state dict) of a golden case: made once, shared, never written to"""
    cfg, _, _, wseed, _ = of.CASES[name]
    sd = of.make_state_dict(cfg, wseed)
    return _model(cfg, sd), sd


def _config(cfg):
    from sudo_rm_rf_amd import _lib
    return _lib.srf_config(variant=_lib.VARIANT_ORIGINAL, in_audio_channels=1, out_channels=cfg["out_channels"],
                           in_channels=cfg["in_channels"], num_blocks=cfg["num_blocks"], upsampling_depth=cfg["upsampling_depth"],
                           enc_kernel_size=cfg["enc_kernel_size"], enc_num_basis=cfg["enc_num_basis"],
                           num_sources=cfg["num_sources"], group_size=1)


def _raw_forward(cfg, sd, wav, poison=None, fetch=None):
    """srf_original_plan_create + srf_forward through ctypes; poison: a byte to fill the workspace with first; fetch: a
    srf_debug_fetch selector and shape to return next to the output"""
    from sudo_rm_rf_amd import _lib
    lib = _lib.load()
    c = _config(cfg)
    batch, _, T = wav.shape
    h = C.c_void_p()
    _lib.check(lib.srf_original_plan_create(C.byref(c), batch, T, C.byref(h)), "srf_original_plan_create")
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
        got = None
        if fetch is not None:
            got = torch.empty(fetch[1], dtype=torch.float32, device=DEV)
            _lib.check(lib.srf_debug_fetch(h, _lib.ptr(ws), fetch[0], _lib.ptr(got), got.numel(), _lib.current_stream(x.device)),
                       "srf_debug_fetch")
        torch.cuda.synchronize()
        return out.cpu().numpy() if fetch is None else (out.cpu().numpy(), got.cpu().numpy())
    finally:
        lib.srf_plan_destroy(h)


@pytest.mark.parametrize("name", sorted(of.CASES))
def test_goldens_through_the_module_and_the_c_abi(name):
    from sudo_rm_rf_amd import ops
    gold = of.load_golden(name)["out"]
    m, sd = _case(name)
    wav = of.make_input(name)
    with torch.no_grad(), ops.kernel_trace(DEV) as tr:
        out = m(torch.from_numpy(wav).to(DEV))
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    raw = _raw_forward(of.CASES[name][0], sd, wav, poison=0xFF)
    e1, e2 = float(np.abs(out - gold).max()), float(np.abs(raw - gold).max())
    print("%s: max|model - reference| = %.3e, max|C ABI - reference| = %.3e (max|ref| %.3f)" % (name, e1, e2, np.abs(gold).max()))
    assert out.shape == gold.shape and e1 <= TOL and e2 <= TOL
    # the launch count the plan states is the count of the forward that ran
    plan = m._engine().last_plan
    names = [n for n, _ in tr.launches]
    assert len(names) == plan.num_launches, names
    cfg = of.CASES[name][0]
    assert names.count("gln_apply_c") + names.count("gln_apply_c_scalar") == 4 * cfg["num_blocks"]
    assert names.count("encoder_bias_relu") == names.count("mask_weight_fill") == names.count("softmax_mask") == 1
    assert names.count("decoder_weight_expand") == names.count("bias_rescale") == 1 and names[-2:] == ["overlap_add", "bias_rescale"]


def test_fused_and_per_level_pyramid_agree():
    """orig_default_u2 (1040 frames, D = 4) runs the fused pyramid on the materialised activation, with no input norm; under the
    per-level switch the same forward runs srf_dwconv5 x D + srf_merge, as the small cases do.  Both against the reference."""
    from sudo_rm_rf_amd import ops
    name = "orig_default_u2"
    gold = of.load_golden(name)["out"]
    m, _ = _case(name)
    x = torch.from_numpy(of.make_input(name)).to(DEV)
    outs, traces = [], []
    for flags in (0, ops.DebugFlag.PYR_PER_LEVEL):
        with torch.no_grad(), ops.debug_flags(flags), ops.kernel_trace(DEV) as tr:
            outs.append(m(x))
        torch.cuda.synchronize()
        traces.append([n for n, _ in tr.launches])
    U, D = of.DEFAULT_U2["num_blocks"], of.DEFAULT_U2["upsampling_depth"]
    assert traces[0].count("pyramid_moments") == traces[0].count("pyramid_finalize") == traces[0].count("pyramid_merge") == U
    assert not any(n.startswith("dwconv5") or n.startswith("merge") for n in traces[0])
    assert sum(n.startswith("dwconv5") for n in traces[1]) == U * D and traces[1].count("merge_fast") == U
    assert not any(n.startswith("pyramid") for n in traces[1]) and len(traces[1]) - len(traces[0]) == U * (D + 1 - 3)
    errs = [float(np.abs(o.cpu().numpy() - gold).max()) for o in outs]
    print("orig_default_u2: fused pyramid %.3e, per-level %.3e, between them %.3e"
          % (errs[0], errs[1], float((outs[0] - outs[1]).abs().max())))
    assert max(errs) <= TOL


def test_stored_block_output_and_mask_logits_of_the_tiny_case():
    """block 0 alone (UBlock.forward, the stand-alone kernel sequence, and a one-block model's separation module through
    srf_debug_fetch) and the mask layer's output before the softmax (selector 3) against what the reference stored"""
    gold = of.load_golden("orig_tiny")
    m, sd = _case("orig_tiny")
    cfg = of.TINY
    wav = of.make_input("orig_tiny")
    L = of.frames(cfg, 1001)
    _, z = _raw_forward(cfg, sd, wav, poison=0xFF, fetch=(3, (2, cfg["num_sources"] * cfg["enc_num_basis"], L)))
    ez = float(np.abs(z.reshape(gold["z"].shape) - gold["z"]).max())
    # one block: the state dict of orig_tiny without sm.1
    cfg1 = dict(cfg, num_blocks=1)
    sd1 = {k: v for k, v in sd.items() if not k.startswith("sm.1.")}
    assert [k for k, _ in of.schema(cfg1)] == list(sd1)
    _, b0 = _raw_forward(cfg1, sd1, wav, poison=0xFF, fetch=(1, (2, cfg["out_channels"], L)))
    eb = float(np.abs(b0 - gold["block0"]).max())
    # UBlock.forward on the reference's own block input: l1(ln(s)) restated in fp64
    sd64 = {k: torch.from_numpy(v).double() for k, v in sd.items()}
    s = torch.relu(torch.nn.functional.conv1d(torch.nn.functional.pad(torch.from_numpy(wav).double(), (0, 1040 - 1001)),
                                              sd64["encoder.0.weight"], sd64["encoder.0.bias"], stride=10, padding=10))
    x0 = torch.nn.functional.conv1d(orf.gn(s, sd64["ln.weight"], sd64["ln.bias"]), sd64["l1.weight"], sd64["l1.bias"])
    with torch.no_grad():
        blk = m.sm[0](x0.float().to(DEV)).cpu().numpy()
    eu = float(np.abs(blk - gold["block0"]).max())
    print("orig_tiny: z err %.3e (max|z| %.2f), block 0 through the walk %.3e, UBlock.forward %.3e (max|ref| %.2f)"
          % (ez, np.abs(gold["z"]).max(), eb, eu, np.abs(gold["block0"]).max()))
    assert eb <= TOL and eu <= TOL and ez <= TOL


def test_reference_pickle_runs():
    from sudo_rm_rf_amd.dnn.models.sudormrf import SuDORMRF
    meta = of.load_manifest()["pickle"]
    m = torch.load(os.path.join(of.GOLDEN, meta["file"]), weights_only=False)
    assert type(m) is SuDORMRF
    m = m.to(DEV).eval()
    wav = of.make_mixture(meta["batch"], meta["T"], meta["input_seed"])
    with torch.no_grad():
        out = m(torch.from_numpy(wav).to(DEV)).cpu().numpy()
    gold = of.load_golden("orig_pickle")["out"]
    err = float(np.abs(out - gold).max())
    print("pickle: max|hip - reference| = %.3e (max|ref| %.3f)" % (err, np.abs(gold).max()))
    assert out.shape == gold.shape and err <= TOL


def test_five_distinct_examples_match_their_own_forward():
    """Row b of a batch of 5 against original_ref on example b ALONE: statistics or a softmax that cross an example's boundary
    cannot pass."""
    m, sd = _case("orig_tiny")
    wav = of.make_distinct(5, of.DISTINCT_T, of.DISTINCT_SEED)
    with torch.no_grad():
        out = m(torch.from_numpy(wav).to(DEV)).cpu().numpy()
    for b in range(5):
        want = orf.forward(of.TINY, sd, wav[b:b + 1], torch.float64).numpy()
        err = float(np.abs(out[b:b + 1] - want).max())
        print("example %d: max|hip - original_ref| = %.3e (max|ref| %.3f)" % (b, err, np.abs(want).max()))
        assert err <= TOL


@pytest.mark.parametrize("mc", [False, True], ids=["plain", "mixture_consistency"])
def test_separate_recipe(mc):
    from sudo_rm_rf_amd import pipeline
    m, sd = _case("orig_tiny")
    raw = of.make_mixture(3, 1001, 430) * np.array([0.3, 2.0, 1.0], dtype=np.float32)[:, None, None] + 0.05
    want = orf.separate(of.TINY, sd, raw, mixture_consistency=mc).numpy()
    got = pipeline.separate(m, torch.from_numpy(raw).to(DEV), mixture_consistency=mc).cpu().numpy()
    listed = pipeline.separate_list(m, [torch.from_numpy(raw[b, 0]).to(DEV) for b in range(3)], mixture_consistency=mc)
    assert pipeline.ragged_route(m, 1001) == "single"
    for b in range(3):
        bar = TOL * max(1.0, float(raw[b].std(ddof=1)))
        err = float(np.abs(got[b] - want[b]).max())
        print("separate (mc %s), example %d: err %.3e, bar %.3e" % (mc, b, err, bar))
        assert err <= bar
        assert float(np.abs(listed[b].cpu().numpy() - want[b]).max()) <= bar


def test_wide_configuration_runs_the_256x128_kernel():
    """The recipe's channel counts at a batch sized from the CU count: l1, proj_1x1, conv_1x1_exp, reshape_before_masks and the
    mask GEMM all take the 256 x 128 split-precision kernel, from packed images (the Toeplitz weight's among them)."""
    from sudo_rm_rf_amd import ops
    cfg = of.WIDE
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nb = -(-cus // of.WIDE_MIN_TILES)
    L = of.frames(cfg, of.WIDE_T)
    assert L == 512 and of.tiles_256(nb, cfg["out_channels"], L) >= cus
    sd = of.make_state_dict(cfg, of.WIDE_WSEED)
    wav = of.make_distinct(nb, of.WIDE_T, of.WIDE_INPUT_SEED)
    m = _model(cfg, sd)
    with torch.no_grad(), ops.kernel_trace(DEV) as tr:
        out = m(torch.from_numpy(wav).to(DEV))
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    names = [n for n, _ in tr.launches]
    print("wide: batch %d on %d CUs, launches: %s" % (nb, cus, names))
    assert len(names) == m._engine().last_plan.num_launches and "pack_pw_weights" in names
    big = lambda n: n.startswith("pw_conv_x3p<") or n.startswith("pw_conv_x3w<")
    gemms = [n for n in names if n.startswith("pw_conv")]
    # l1 | per block proj_1x1, conv_1x1_exp | reshape_before_masks | the mask GEMM | the decoder's frame GEMM (thin: not this kernel)
    assert len(gemms) == 1 + 2 * cfg["num_blocks"] + 1 + 1 + 1 and all(big(n) for n in gemms[:-1]), gemms
    i = names.index("softmax_mask")
    assert big(names[i - 1]) and big(names[i - 2])           # the mask GEMM and reshape_before_masks
    assert names.count("pyramid_moments") == names.count("pyramid_merge") == cfg["num_blocks"] and "merge_fast" not in names
    for j, n in enumerate(names):
        if n == "pyramid_moments":
            assert names[j - 1] == "gln_apply_c" and big(names[j - 2])      # proj_1x1, then a
        if n == "pyramid_merge":
            assert names[j + 1] == "gln_apply_c" and big(names[j + 2]) and names[j + 3:j + 5] == ["gln_apply_c"] * 2
    errs = []
    for b0 in range(0, nb, 8):                               # (per-example independent: the fp64 restatement in slices)
        want = orf.forward(cfg, sd, wav[b0:b0 + 8], torch.float64).numpy()
        errs.append(float(np.abs(out[b0:b0 + 8] - want).max()))
    print("wide: max|hip - original_ref| = %.3e (max|out| %.3f)" % (max(errs), np.abs(out).max()))
    assert 0.1 <= np.abs(out).max() <= 10.0 and max(errs) <= TOL


# ---- one srf_forward with wav, out and the workspace inside a poisoned arena with guard words ---------------------------------------
@pytest.mark.parametrize("name", ["orig_tiny", "orig_s3_k9"])
def test_forward_inside_a_guarded_arena(name):
    from sudo_rm_rf_amd import _lib
    lib = _lib.load()
    cfg, batch, T, wseed, _ = of.CASES[name]
    sd = of.make_state_dict(cfg, wseed)
    wav = of.make_input(name)
    gold = of.load_golden(name)["out"]
    c = _config(cfg)
    h = C.c_void_p()
    _lib.check(lib.srf_original_plan_create(C.byref(c), batch, T, C.byref(h)), "srf_original_plan_create")
    try:
        nbytes = lib.srf_plan_workspace_bytes(h)
        a = pl.Arena(DEV, nbytes + (4 << 20))
        params = [a.put(torch.from_numpy(v), shift_floats=(1, 3, 0, 2)[i % 4], name=k) for i, (k, v) in enumerate(sd.items())]
        table = (C.c_void_p * len(params))(*[p.data_ptr() for p in params])
        x = a.put(torch.from_numpy(wav), shift_floats=1, name="wav")
        out = a.place((batch, cfg["num_sources"], T), shift_floats=3, name="out")
        ws = a.place((nbytes,), torch.uint8, name="workspace")          # poisoned: 0xFF throughout
        assert ws.data_ptr() % 256 == 0
        st = _lib.current_stream(torch.device(DEV))
        # refused calls first: nothing may be written (a short workspace, a wrong table length, a misaligned workspace)
        assert lib.srf_forward(h, table, len(params), _lib.ptr(x), _lib.ptr(out), _lib.ptr(ws), nbytes - 1, st) == -3
        assert lib.srf_forward(h, table, len(params) - 1, _lib.ptr(x), _lib.ptr(out), _lib.ptr(ws), nbytes, st) == -1
        assert lib.srf_forward(h, table, len(params), _lib.ptr(x), _lib.ptr(out), C.c_void_p(ws.data_ptr() + 4), nbytes, st) == -1
        torch.cuda.synchronize()
        a.check()
        a.assert_untouched(out)
        a.assert_untouched(ws)
        _lib.check(lib.srf_forward(h, table, len(params), _lib.ptr(x), _lib.ptr(out), _lib.ptr(ws), nbytes, st), "srf_forward")
        torch.cuda.synchronize()
        a.check()                                            # no guard word changed
        a.assert_written(out)
        a.assert_clean(out)                                  # no poison reached the output
        err = float(np.abs(out.cpu().numpy() - gold).max())
        print("%s in the arena: max|hip - reference| = %.3e" % (name, err))
        assert err <= TOL
    finally:
        lib.srf_plan_destroy(h)


def test_refusals():
    from sudo_rm_rf_amd._lib import SrfError
    from sudo_rm_rf_amd.dnn.models.sudormrf import SuDORMRF
    m, sd = _case("orig_tiny")
    wav = of.make_input("orig_tiny")
    x = torch.from_numpy(wav).to(DEV)
    with pytest.raises(RuntimeError, match=r"torch\.no_grad\(\)"):
        m(x)
    m.train()
    try:
        with pytest.raises(RuntimeError, match=r"inference forward only"):
            m(x)
    finally:
        m.eval()
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="ragged"):
            m.forward_ragged(x, [1001, 900])
        with pytest.raises(SrfError, match="MI355X"):
            m(torch.from_numpy(wav))
        with pytest.raises(SrfError, match=r"26 frames are not a multiple of 2\^\(D-1\)"):
            SuDORMRF(**of.S3_K9).to(DEV).eval()(torch.zeros(2, 1, of.S3_K9_REFUSED_T, device=DEV))
        with pytest.raises(SrfError, match="enc_num_basis = 63 is odd"):
            SuDORMRF(**dict(of.TINY, enc_num_basis=63)).to(DEV).eval()(torch.zeros(1, 1, 1000, device=DEV))
        with pytest.raises(SrfError, match="SRF_SOFTMAX_MASK_MAX_SOURCES"):
            SuDORMRF(**dict(of.TINY, num_sources=17, num_blocks=1)).to(DEV).eval()(torch.zeros(1, 1, 1000, device=DEV))
        assert np.isfinite(m(x).cpu().numpy()).all()
