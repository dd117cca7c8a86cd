"""TransformerLayer.forward(..., lengths=) and AttentiveUConvBlock.forward(x, lengths) on a ragged batch.
Per example the output is compared with tests.attentive_ref on the example's own slice (fp64) and, for the small cases, with
the reference's own modules (tests/golden/attn_ragged_*.npz, tools/make_golden_attentive_ragged.py): 1e-4 max-abs, the project's
bar for forward outputs.  Every case: exact zeros past the lengths, NaN padding in x, a row's bits unchanged under other rows
and lengths, equal bits on a second run, lengths=None the call without the keyword, the refusals under autograd and in train().
Worst errors measured on an MI355X: profiles/attentive_block_ragged.txt."""
import numpy as np
import pytest
import torch

from tests import attentive_ragged_cases as rc
from tests import attentive_ref as ar

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR = 1e-4

# the cases without a fixture (the reference restated in fp64 is the yardstick): the MFMA GEMM paths of the layer, and a block
# whose two 1x1 convolutions take the packed ragged GEMM
BIG = {
    "layer_mfma_gemm": dict(module="layer", emb=128, heads=2, d_model=64, L=40, lengths=[40, 17], lazy=False),
    "block_packed": dict(module="block", out=256, emb=512, depth=3, heads=2, d_model=32, L=512, lengths=[512, 260]),
}
ALL = dict(rc.CASES, **BIG)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _nan_tail(x, lengths):
    x = x.clone()
    for b, n in enumerate(lengths):
        x[b, :, n:] = float("nan")
    return x


def _own_sums(x, lengths):
    s = torch.zeros(x.shape[0], 64, 2, dtype=torch.float64)
    for b, n in enumerate(lengths):
        own = x[b, :, :n].double()
        s[b, 0, 0], s[b, 0, 1] = own.sum(), (own * own).sum()
    return s.to(DEV)


_CACHE = {}


def _case(name):
    """-> (module on the GPU in eval(), x [Bt, C, L] host fp32, extra keyword tensors for a lazy layer, want: per example the
    fp64 reference on its own slice, c).  Built once per case and shared; nothing in it is modified."""
    if name in _CACHE:
        return _CACHE[name]
    from sudo_rm_rf_amd.dnn.models import attentive_sudormrf_v2 as m2
    c = ALL[name]
    Ld = c["L"] >> (c.get("depth", 1) - 1)
    torch.manual_seed(4100 + len(name))
    if c["module"] == "layer":
        mod = m2.TransformerLayer(c["emb"], c["d_model"], c["heads"])
        layer, Cin = mod, c["emb"]
    else:
        mod = m2.AttentiveUConvBlock(c["out"], c["emb"], c["depth"], c["heads"], c["d_model"])
        layer, Cin = mod.attention, c["out"]
    in_norm = None
    if name in rc.CASES:
        z = np.load(rc.path(name))
        with torch.no_grad():
            for n, p in mod.named_parameters():
                p.copy_(torch.as_tensor(z["param." + n]))
            layer.pos_enc.pe[0, :Ld] = torch.as_tensor(z["pe"])
        x = torch.as_tensor(z["x"])
        if c.get("lazy"):
            in_norm = (torch.as_tensor(z["param.in_norm.gamma"]), torch.as_tensor(z["param.in_norm.beta"]))
        golden = torch.as_tensor(z["out"])
    else:
        g = torch.Generator().manual_seed(77)
        with torch.no_grad():
            for n, p in mod.named_parameters():          # gains around 1, small shifts: every norm and slope takes part
                if n.endswith("gamma"):
                    p.copy_(torch.randn(p.shape, generator=g) * 0.2 + 1.0)
                elif n.endswith("beta") or n.endswith("bias"):
                    p.copy_(torch.randn(p.shape, generator=g) * 0.2)
        x = torch.randn(len(c["lengths"]), Cin, c["L"], generator=g)
        golden = None
    mod = mod.to(DEV).eval()
    sd = {"m." + k: v.detach().double().cpu() for k, v in mod.state_dict().items()}
    want = []
    for b, n in enumerate(c["lengths"]):
        xb = x[b:b + 1, :, :n].double()
        if c["module"] == "block":
            w = ar.block(xb, sd, "m.", c["depth"], c["heads"])
        else:
            a = ar.gln(xb, in_norm[0].double(), in_norm[1].double()) if in_norm else xb
            w = ar.transformer_layer(a, sd, "m.", c["heads"])
        want.append(w[0])
        if golden is not None:      # the restatement and the reference's own module agree on the slice (fp64 both)
            assert (w[0] - golden[b, :, :n]).abs().max().item() <= 1e-10
    _CACHE[name] = (mod, x, in_norm, want, c)
    return _CACHE[name]


def _run(name, x, lengths, trace=None):
    from sudo_rm_rf_amd import ops
    mod, _, in_norm, _, c = _case(name)
    kw = {}
    if in_norm:
        kw = dict(in_sums=_own_sums(x, lengths), in_gamma=in_norm[0].to(DEV), in_beta=in_norm[1].to(DEV))
    with torch.no_grad(), ops.kernel_trace(DEV) as tr:
        y = mod(x.to(DEV), lengths=lengths, **kw)
    if trace is not None:
        trace.extend(n for n, _ in tr.launches)
    return y


@pytest.mark.parametrize("name", list(ALL))
def test_ragged_call_is_every_example_alone_on_its_slice(name):
    from sudo_rm_rf_amd import attention
    mod, x, in_norm, want, c = _case(name)
    lengths = c["lengths"]
    names = []
    y = _run(name, x, lengths, names)
    got = y.cpu()
    worst = 0.0
    for b, n in enumerate(lengths):
        err = (got[b, :, :n].double() - want[b]).abs().max().item()
        worst = max(worst, err)
        print("  %s example %d (%d of %d): max-abs error %.3g" % (name, b, n, c["L"], err))
        tail = got[b, :, n:]
        assert tail.numel() == 0 or (_bits(tail) == 0).all(), "%s: example %d is not exact +0 past its end" % (name, b)
    print("  %s: worst max-abs error %.3g; kernels %s" % (name, worst, sorted(set(names))))
    assert worst <= BAR, (name, worst)
    # ---- the kernels: ragged forms where there are any, the dispatch the case is about
    assert "posenc_apply_ragged" in names and "gln_apply2_add_ragged" in names and names.count("gln_stats_ragged") >= 2, names
    assert any(n.startswith("mha_attention") and n.endswith("_ragged") for n in names), names
    assert "mha_attention_%s_ragged" % ("mfma" if attention.mha_attention_mfma_supported(c["d_model"]) else "generic") in names
    if name == "layer_valu24":
        assert "mha_attention_generic_ragged" in names
    if name in ("layer_mfma16", "layer_mfma_gemm"):
        assert "mha_attention_mfma_ragged" in names
    if name == "layer_mfma_gemm":
        assert "pw_conv_generic" not in names and any(n.startswith("pw_conv_bf16x3") for n in names), names
    if c["module"] == "layer":
        assert names[-1] == "gln_apply_ragged"
    else:
        assert any(n.startswith("merge_") and n.endswith("_ragged") for n in names), names
        assert sum(n.startswith("dwconv5_") and n.endswith("_ragged") for n in names) == c["depth"], names
        packed = [n for n in names if n.startswith("pw_conv_x3w_ragged")]
        if name == "block_packed":      # proj_1x1 (with statistics) and res_conv (GlobLN + PReLU + residual) on the packed ragged GEMM
            assert len(packed) == 2 and names[-1] == packed[1], names
            assert names.count("gln_stats_ragged") == 2 and names.count("sums_scale_ragged") == 1, names
        else:                            # the fallback: uniform GEMMs between the statistics pass and the scaled sums
            assert not packed and names.count("gln_stats_ragged") == 3 and names.count("sums_scale_ragged") == 2, names


@pytest.mark.parametrize("name", list(ALL))
def test_padding_other_rows_and_a_second_run_change_no_bit(name):
    mod, x, in_norm, want, c = _case(name)
    lengths = c["lengths"]
    y = _run(name, x, lengths)
    assert torch.equal(_bits(y), _bits(_run(name, x, lengths))), "two runs differ"
    names = []
    y_nan = _run(name, _nan_tail(x, lengths), lengths, names)
    assert torch.equal(_bits(y), _bits(y_nan)), "NaN past the lengths changed the output"
    if name == "block_d2":      # (the NaN-padded block on the uniform-GEMM fallback: the padding really flows through the GEMMs)
        assert not [n for n in names if n.startswith("pw_conv_x3w_ragged")] and any(n.startswith("pw_conv") for n in names)
    # example 1 keeps content and length; the others change both (lengths stay legal for the case)
    unit = 1 << (c.get("depth", 1) - 1)
    other = torch.randn(x.shape, generator=torch.Generator().manual_seed(5)) * 2.0
    other[1] = x[1]
    other_len = [max(unit, (n // 2) // unit * unit) for n in lengths]
    other_len[1] = lengths[1]
    if name == "block_packed":
        other_len = [256, lengths[1]]                      # (multiples of 4: the same GEMM -- the contract holds while the batch
                                                           #  stays on the same kernels)
    y_o = _run(name, other, other_len)
    assert torch.equal(_bits(y[1]), _bits(y_o[1])), "example 1 changed with the other rows (lengths %s)" % other_len


@pytest.mark.parametrize("name", list(ALL))
def test_lengths_none_is_the_call_without_the_keyword(name):
    mod, x, in_norm, _, c = _case(name)
    full = [c["L"]] * x.shape[0]
    args = (_own_sums(x, full), in_norm[0].to(DEV), in_norm[1].to(DEV)) if in_norm else ()
    with torch.no_grad():
        a = mod(x.to(DEV), *args)
        b = mod(x.to(DEV), *args, lengths=None)
        r = mod(x.to(DEV), *args, lengths=full)
    assert torch.equal(_bits(a), _bits(b))
    assert (a - r).abs().max().item() <= BAR               # full lengths: the uniform call within the bar


@pytest.mark.parametrize("name", list(ALL))
def test_refusals_under_autograd_and_in_train_mode(name):
    import copy
    mod, x, _, _, c = _case(name)
    mod = copy.deepcopy(mod)
    lengths = c["lengths"]
    xd = x.to(DEV)
    mod.enable_hip_training()
    with pytest.raises(NotImplementedError, match="no ragged training"):
        mod(xd.clone().requires_grad_(), lengths=lengths)
    with torch.no_grad():                                  # (opted in, but nothing to differentiate: the inference path)
        assert mod(xd, lengths=lengths).shape == xd.shape
    mod.train()
    with torch.no_grad(), pytest.raises(RuntimeError, match="dropout"):
        mod(xd, lengths=lengths)
    mod.enable_hip_training(False)
    with torch.no_grad(), pytest.raises(RuntimeError, match="dropout"):
        mod(xd, lengths=lengths)
    with pytest.raises(Exception, match="list or a CPU tensor"):
        with torch.no_grad():
            mod.eval()(xd, lengths=torch.tensor(lengths, device=DEV))
