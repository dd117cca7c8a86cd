"""attentive_sudormrf_v2.SuDORMRF after enable_ragged() on the GPU: forward_ragged / separate_ragged /
pipeline.separate_list on unequal-length rows in one set of launches.  Every row is held to 1e-4 max-abs -- the project's bar for
forward outputs -- against the reference model run on that row ALONE at its own length (tests/golden/attn_model_ragged_*.npz,
tools/make_golden_attentive_model_ragged.py) and against the model's own batch-1 HIP forward on the row; weights and mixtures are
regenerated from the cases' seeds.  Worst errors measured on an MI355X: profiles/ragged_forward_attentive.txt."""
import numpy as np
import pytest
import torch

from tests import attentive_fixtures as af
from tests import attentive_model_ragged_cases as mc

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR = mc.BAR
NAMES = sorted(mc.CASES)


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    from sudo_rm_rf_amd import _lib, ops
    _lib.load()
    ops.set_kernel_mode(0)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _model(name, opt_in=True):
    from sudo_rm_rf_amd.dnn.models.attentive_sudormrf_v2 import SuDORMRF
    cfg, _, wseed, _ = mc.CASES[name]
    m = SuDORMRF(**cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in af.make_state_dict(cfg, wseed).items()})
    m = m.to(DEV).eval()
    return m.enable_ragged() if opt_in else m


_CACHE = {}


def _case(name):
    """-> dict(model, wav [B, 1, T] host, lengths, out: the ragged forward's output (host), names: its launches, single: per row
    the model's own batch-1 forward on the row (host)).  Built once per case and shared; nothing in it is modified."""
    if name in _CACHE:
        return _CACHE[name]
    from sudo_rm_rf_amd import ops
    cfg, lengths, _, _ = mc.CASES[name]
    lengths = list(lengths)
    m = _model(name)
    wav = torch.from_numpy(mc.make_wav(name))
    with torch.no_grad():
        with ops.kernel_trace(DEV) as tr:
            out = m.forward_ragged(wav.to(DEV), lengths)
        single = [m(wav[b:b + 1, :, :n].to(DEV).contiguous())[0].cpu() for b, n in enumerate(lengths)]
    torch.cuda.synchronize()
    _CACHE[name] = dict(model=m, wav=wav, lengths=lengths, out=out.cpu(), names=[n for n, _ in tr.launches], single=single, cfg=cfg)
    return _CACHE[name]


@pytest.mark.parametrize("name", NAMES)
def test_every_row_is_its_own_forward(name):
    c = _case(name)
    fx = mc.load(name)
    assert fx["lengths"] == c["lengths"] and tuple(c["out"].shape) == (len(c["lengths"]), c["cfg"]["num_sources"], max(c["lengths"]))
    worst_ref = worst_hip = 0.0
    for b, n in enumerate(c["lengths"]):
        got = c["out"][b, :, :n].double()
        assert torch.isfinite(got).all()
        e_ref = (got - torch.from_numpy(fx["out"][b]).double()).abs().max().item()
        e_hip = (got - c["single"][b].double()).abs().max().item()
        print("  case %s row %d (%d samples): max-abs error vs the reference %.3g, vs the batch-1 HIP forward %.3g" % (name, b, n, e_ref, e_hip))
        worst_ref, worst_hip = max(worst_ref, e_ref), max(worst_hip, e_hip)
        tail = c["out"][b, :, n:]
        assert tail.numel() == 0 or (_bits(tail) == 0).all(), "case %s: row %d is not exact +0 past its end" % (name, b)
    print("  case %s: worst %.3g (reference) %.3g (batch-1 HIP)" % (name, worst_ref, worst_hip))
    assert worst_ref <= BAR and worst_hip <= BAR, (name, worst_ref, worst_hip)


def _gemm_shapes(cfg, T):
    """(Cin, Cout, level) of every 1x1 convolution of the walk in launch order: level 0 = full length, 1 = the deepest level"""
    B, C, N, U = cfg["out_channels"], cfg["in_channels"], cfg["enc_num_basis"], cfg["num_blocks"]
    HD = af.HEADS * af.ATT_DIMS
    return [(N, B, 0)] + U * [(B, C, 0), (C, 3 * HD, 1), (HD, C, 1), (C, C, 1), (C, B, 0)]


@pytest.mark.parametrize("name", NAMES)
def test_the_launches_are_the_ragged_ones(name):
    from sudo_rm_rf_amd import ragged
    c = _case(name)
    cfg, names, lengths = c["cfg"], c["names"], c["lengths"]
    D, U = cfg["upsampling_depth"], cfg["num_blocks"]
    print("  case %s: %s" % (name, sorted(set(names))))
    assert "zero_past" not in names and not any("zero_past" in n for n in names), names
    assert sum(n.startswith("dwconv5_") and n.endswith("_ragged") for n in names) == U * D, names
    assert names.count("posenc_apply_ragged") == U and names.count("gln_apply2_add_ragged") == U, names
    assert sum(n.startswith("merge_") and n.endswith("_ragged") for n in names) == U, names
    assert sum(n.startswith("mha_attention") and n.endswith("_ragged") for n in names) == U, names
    assert any(n.startswith("encoder") and n.endswith("_ragged") for n in names), names
    assert any(n.startswith("overlap_add") and n.endswith("_ragged") for n in names), names
    # per launch: where a ragged gate passes, a ragged GEMM ran -- count the walk's convolutions that neither gate takes
    # (those, the mask GEMM and the decoder's frame GEMM are the uniform launches that remain)
    L = mc.frames(cfg, max(lengths))
    fr = [[mc.frames(cfg, n) >> k for n in lengths] for k in (0, D - 1)]
    Bt = len(lengths)
    fallback = 0
    for Cin, Cout, lv in _gemm_shapes(cfg, max(lengths)):
        len_lv = L >> ((D - 1) * lv)
        if not (ragged.pw_conv_mfma_supported(Bt, Cin, Cout, len_lv, fr[lv]) or ragged.pw_conv_supported(Bt, Cin, Cout, len_lv, fr[lv])):
            fallback += 1
    rg = [n for n in names if n.startswith("pw_conv_") and "_ragged" in n]
    uniform = [n for n in names if n.startswith("pw_conv_") and "_ragged" not in n]
    fused_tail = "pw_mask_decode" in names
    print("  case %s: %d ragged GEMM launches, %d uniform (%d fall-backs of the walk), tail %s" % (
        name, len(rg), len(uniform), fallback, "fused" if fused_tail else "unfused"))
    assert len(rg) == 1 + 5 * U - fallback, (names, fallback)
    assert len(uniform) == fallback + (0 if fused_tail else 2), (names, fallback)          # + mask GEMM, decoder frame GEMM
    if name == "a":
        assert not fused_tail and fallback > 0
    if name == "b":             # every GEMM of the walk on the new kernel
        assert fallback == 0 and all(n.startswith("pw_conv_bf16x3_ragged") for n in rg) and len(rg) == 1 + 5 * U, names
    if name == "c":             # the deepest level (32 / 20 / 9 positions) on the new kernel
        assert sum(n.startswith("pw_conv_bf16x3_ragged") for n in rg) >= 3 * U, names
    if name == "d":             # proj_1x1 (128 -> 512 at 1040 / 520 frames) on the packed ragged kernel, bottleneck and res_conv on the new one
        assert sum(n.startswith("pw_conv_x3w_ragged") for n in rg) == U and sum(n.startswith("pw_conv_bf16x3_ragged") for n in rg) >= 1 + U, names


@pytest.mark.parametrize("name", NAMES)
def test_nan_padding_and_other_rows_change_no_bit(name):
    c = _case(name)
    m, lengths = c["model"], c["lengths"]
    wav = c["wav"].clone()
    for b, n in enumerate(lengths):
        wav[b, :, n:] = float("nan")
    with torch.no_grad():
        out = m.forward_ragged(wav.to(DEV), lengths).cpu()
    assert torch.equal(_bits(out), _bits(c["out"])), "case %s: NaN past the lengths changed the output" % name
    # other rows' content (their lengths held fixed: dispatch is per launch)
    g = torch.Generator().manual_seed(11)
    other = c["wav"].clone()
    other[1:] = torch.randn(other[1:].shape, generator=g) * 0.7
    with torch.no_grad():
        out = m.forward_ragged(other.to(DEV), lengths).cpu()
    assert torch.equal(_bits(out[0]), _bits(c["out"][0])), "case %s: row 0 changed with the other rows' content" % name
    other = c["wav"].clone()
    other[:-1] = torch.randn(other[:-1].shape, generator=g) * 0.7
    with torch.no_grad():
        out = m.forward_ragged(other.to(DEV), lengths).cpu()
    assert torch.equal(_bits(out[-1]), _bits(c["out"][-1])), "case %s: the last row changed with the other rows' content" % name


@pytest.mark.parametrize("name", NAMES)
def test_equal_lengths_are_the_uniform_forward_within_the_bar(name):
    c = _case(name)
    m, T = c["model"], max(c["lengths"])
    x = c["wav"].to(DEV)
    with torch.no_grad():
        got = m.forward_ragged(x, [T] * x.shape[0]).cpu()
        want = m(x).cpu()
    err = (got.double() - want.double()).abs().max().item()
    print("  case %s: equal lengths vs the uniform forward: max-abs %.3g" % (name, err))
    assert err <= BAR, (name, err)


@pytest.mark.parametrize("mcons", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_separate_ragged_and_separate_list_are_separate_per_utterance(name, mcons):
    from sudo_rm_rf_amd import pipeline
    c = _case(name)
    m, lengths = c["model"], c["lengths"]
    gains = torch.tensor([0.05, 3.0, 0.7])[:len(lengths), None, None]
    raw = (c["wav"] * gains + 0.01).to(DEV)             # un-normalised mixtures with an offset
    rows = [raw[b, 0, :n].contiguous() for b, n in enumerate(lengths)]
    with torch.no_grad():
        est, stats = m.separate_ragged(raw, lengths, mcons)
        listed = pipeline.separate_list(m, rows, mixture_consistency=mcons)
        want = [pipeline.separate(m, r[None, None], mcons)[0] for r in rows]
    assert tuple(stats.shape) == (len(lengths), 2)
    for b, n in enumerate(lengths):
        tol = BAR * max(1.0, float(rows[b].std()))
        e1 = (est[b, :, :n] - want[b]).abs().max().item()
        e2 = (listed[b] - want[b]).abs().max().item()
        print("  case %s mc=%s row %d: separate_ragged %.3g, separate_list %.3g (tolerance %.3g)" % (name, mcons, b, e1, e2, tol))
        assert tuple(listed[b].shape) == tuple(want[b].shape) and e1 <= tol and e2 <= tol, (name, b, e1, e2, tol)
        assert n == est.shape[-1] or (_bits(est[b, :, n:]) == 0).all()
        assert abs(float(stats[b, 0]) - float(rows[b].mean())) <= 1e-5 and abs(float(stats[b, 1]) - float(rows[b].std())) <= 1e-4 * float(rows[b].std())
    # the list went through ONE ragged plan (the whole batch)
    assert any(k[1] == len(lengths) for k in m._engine()._plans)


def test_separate_list_without_the_opt_in_makes_one_plan_per_utterance():
    from sudo_rm_rf_amd import ops, pipeline
    c = _case("a")
    plain = _model("a", opt_in=False)
    assert not hasattr(plain, "separate_ragged") and pipeline.ragged_route(plain, 1001) == "single"
    rows = [c["wav"][b, 0, :n].to(DEV).contiguous() for b, n in enumerate(c["lengths"])]
    with torch.no_grad(), ops.kernel_trace(DEV) as tr:
        got = pipeline.separate_list(plain, rows, mixture_consistency=False)
    plans = list(plain._engine()._plans)
    assert len(plans) == len(rows) and all(k[1] == 1 for k in plans), plans
    assert not any(n.endswith("_ragged") or "_ragged<" in n for n, _ in tr.launches)
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="no ragged kernels"):
            plain.forward_ragged(c["wav"].to(DEV), c["lengths"])
        want = pipeline.separate_list(c["model"], rows, mixture_consistency=False)
    for a, b in zip(got, want):
        assert (a - b).abs().max().item() <= BAR


def test_the_ragged_call_raises_under_autograd_and_in_train_mode():
    c = _case("a")
    m = _model("a")
    x = c["wav"].to(DEV)
    with pytest.raises(NotImplementedError, match="inference path"):
        m.forward_ragged(x, c["lengths"])               # grad mode on, parameters require grad
    with pytest.raises(NotImplementedError, match="inference path"):
        m.separate_ragged(x, c["lengths"])
    m.train()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="inference path"):
        m.forward_ragged(x, c["lengths"])
    m.eval()
    with torch.no_grad():
        assert torch.equal(_bits(m.forward_ragged(x, c["lengths"])), _bits(c["out"]))
