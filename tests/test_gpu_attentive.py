"""Attentive SuDoRM-RF (v2) on the GPU: the reference's goldens through the module and through the raw C ABI, the reference's
pickle, a batch of distinct examples, a poisoned workspace, the separate() recipe and the refusals.  References: the stored
reference outputs (tests/golden/attn_*.npz) and, where there is no golden, tests/attentive_ref.py in fp64 (pinned to the
goldens by tests/test_attentive_host.py).  Bar: the project's 1e-4 max-abs."""
import ctypes as C
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
    with torch.no_grad():
        out = m(torch.from_numpy(wav).to(DEV)).cpu().numpy()
    gold = af.load_golden("attn_pickle")["out"]
    err = float(np.abs(out - gold).max())
    print("pickle: max|hip - reference| = %.3e" % err)
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
