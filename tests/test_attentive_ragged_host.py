"""The ragged attentive layer / block without a GPU: the seven new symbols' declarations against their
ctypes bindings, the keyword defaults, the refusals that come before any launch, and -- in fp64 torch -- the definition the GPU
tests rely on: tests.attentive_ref.block / transformer_layer on an example's own slice is the reference's module on that slice
(the fixtures, every example run alone), and sums scaled by L / len under the count C * L give the slice's own mean and variance."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import attentive_ragged_cases as rc
from tests import attentive_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("srf_dwconv5_ragged", "srf_merge_ragged", "srf_posenc_apply_ragged", "srf_gln_apply2_add_ragged",
               "srf_gln_apply_ragged", "srf_gln_stats_ragged", "srf_sums_scale_ragged", "srf_pw_conv_packed_ragged_supported")
UNIFORM_TWIN = {"srf_dwconv5_ragged": "srf_dwconv5", "srf_merge_ragged": "srf_merge", "srf_posenc_apply_ragged": "srf_posenc_apply",
                "srf_gln_apply2_add_ragged": "srf_gln_apply2_add", "srf_gln_apply_ragged": "srf_gln_apply"}


def _header_arity(name):
    text = open(os.path.join(ROOT, "include", "sudormrf_hip.h")).read()
    m = re.search(r"^(?:int|size_t)\s+%s\(([^;]*)\);" % name, text, re.M | re.S)
    assert m, "%s is not declared in include/sudormrf_hip.h" % name
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_header_declares_and_lib_binds_the_new_symbols(name):
    from sudo_rm_rf_amd import _lib
    lib = _lib.load()
    assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert len(getattr(lib, name).argtypes) == _header_arity(name)
    if name in UNIFORM_TWIN:
        assert _header_arity(name) == _header_arity(UNIFORM_TWIN[name]) + 1          # + the table
    assert lib.srf_abi_version() == 19 == _lib.ABI_VERSION
    assert _lib.RAGGED_MAX_BATCH == 128


def test_lengths_default_to_none_everywhere():
    from sudo_rm_rf_amd import attention, ragged
    from sudo_rm_rf_amd.dnn.models import attentive_sudormrf_v2 as m
    for fn in (m.TransformerLayer.forward, m.AttentiveUConvBlock.forward, m._transformer_tail, attention.posenc_apply,
               attention.gln_apply2_add):
        assert inspect.signature(fn).parameters["lengths"].default is None, fn
    assert list(inspect.signature(m.TransformerLayer.forward).parameters) == ["self", "x", "in_sums", "in_gamma", "in_beta", "lengths"]
    for name in ("dwconv5", "merge", "gln_stats", "gln_apply", "sums_scale"):
        assert callable(getattr(ragged, name)), name
    assert "lengths" not in inspect.signature(m.MHAttentionLayer.forward).parameters      # (its own two keywords stay)
    from sudo_rm_rf_amd.dnn.models import attentive_sudormrf_v3 as m3
    assert "lengths" not in inspect.signature(m3.ConditionalTransformerLayer.forward).parameters


def test_a_device_tensor_as_lengths_is_refused_by_the_table_convention():
    from sudo_rm_rf_amd import _lib, ragged

    class FakeCuda(torch.Tensor):
        """a CPU tensor that says it lives on a GPU: ragged._table must refuse it without reading it"""
        @property
        def device(self):
            return torch.device("cuda", 0)

    t = torch.tensor([4, 2]).as_subclass(FakeCuda)
    with pytest.raises(_lib.SrfError, match="list or a CPU tensor"):
        ragged._frames_for("srf_gln_stats_ragged", t, 2)
    with pytest.raises(_lib.SrfError, match="3 frames for a batch of 2"):
        ragged._frames_for("srf_gln_stats_ragged", [1, 2, 3], 2)


def test_bad_tables_are_refused_by_the_c_entry_points_before_any_launch():
    """(never-dereferenced dummy pointers: every call below returns SRF_EINVAL from its argument checks)"""
    from sudo_rm_rf_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(0x1000)
    tab = lambda *v: (C.c_int * len(v))(*v)
    nrm = _lib.srf_norm()
    nrm.sums = nrm.gamma = nrm.beta = 0x1000
    nrm.prelu = None
    norms = (_lib.srf_norm * 3)(nrm, nrm, nrm)
    lv = (C.c_void_p * 3)(0x1000, 0x1000, 0x1000)
    Bt, Cc, L = 3, 8, 24

    def calls(t, Bt=Bt, stride=1, D=3):
        yield "srf_dwconv5_ragged", lib.srf_dwconv5_ragged(p, p, p, p, Bt, Cc, L, stride, C.byref(nrm), None, t, None)
        yield "srf_merge_ragged", lib.srf_merge_ragged(lv, norms, D, p, Bt, Cc, L, None, t, None)
        yield "srf_posenc_apply_ragged", lib.srf_posenc_apply_ragged(p, C.byref(nrm), p, p, Bt, Cc, L, 5000, t, None)
        yield "srf_gln_apply2_add_ragged", lib.srf_gln_apply2_add_ragged(p, C.byref(nrm), p, C.byref(nrm), p, None, Bt, Cc, L, t, None)
        yield "srf_gln_apply_ragged", lib.srf_gln_apply_ragged(p, p, C.byref(nrm), Bt, Cc, L, t, None)
        yield "srf_gln_stats_ragged", lib.srf_gln_stats_ragged(p, p, Bt, Cc, L, t, None)
        yield "srf_sums_scale_ragged", lib.srf_sums_scale_ragged(p, C.c_void_p(0x2000), Bt, L, t, None)

    def refused(t, pattern, only=None, **kw):
        seen = 0
        for name, rc_ in calls(t, **kw):
            msg = lib.srf_last_error().decode()
            if only is not None and name not in only:
                continue
            seen += 1
            assert rc_ == -1, (name, rc_, msg)          # SRF_EINVAL
            assert msg.startswith(name) and re.search(pattern, msg), (name, msg)
        assert seen == (7 if only is None else len(only))

    refused(None, r"null frames table")
    refused(tab(24, 0, 4), r"example 1 has 0 frames \(allowed: 1\.\.24\)")
    refused(tab(24, 4, 28), r"example 2 has 28 frames \(allowed: 1\.\.24\)")
    refused(tab(8, -4, 4), r"example 1 has -4 frames")
    refused(tab(*([4] * 129)), r"1\.\.128 examples \(got 129\)", Bt=129)
    refused(tab(24, 7, 4), r"example 1 has 7 input frames: stride 2 needs an even count", only=("srf_dwconv5_ragged",), stride=2)
    refused(tab(24, 8, 6), r"example 2 has 6 frames: not a multiple of 2\^\(D-1\) = 4", only=("srf_merge_ragged",))
    # ... and what the uniform twins refuse
    assert lib.srf_dwconv5_ragged(p, p, p, p, Bt, Cc, L, 3, None, None, tab(4, 4, 4), None) == -1
    assert "stride must be 1 or 2" in lib.srf_last_error().decode()
    assert lib.srf_merge_ragged(lv, norms, 3, p, Bt, Cc, 26, None, tab(4, 4, 4), None) == -1
    assert "not divisible by 2^(D-1)" in lib.srf_last_error().decode()
    assert lib.srf_posenc_apply_ragged(p, None, p, p, Bt, Cc, L, 20, tab(4, 4, 4), None) == -1
    assert "exceed the table's max_len" in lib.srf_last_error().decode()


def test_block_refuses_bad_lengths_naming_the_example():
    """(the block's own checks come before the device check: CPU tensors reach them)"""
    from sudo_rm_rf_amd.dnn.models.attentive_sudormrf_v2 import AttentiveUConvBlock
    blk = AttentiveUConvBlock(8, 16, 3, 2, 8).eval()
    x = torch.zeros(3, 8, 24)
    with torch.no_grad():
        for lengths, pattern in (([24, 6, 4], "example 1 has length 6"), ([24, 8, 0], "example 2 has length 0"),
                                 ([28, 8, 4], "example 0 has length 28"), ([24, 8], "2 lengths for a batch of 3")):
            with pytest.raises(RuntimeError, match=pattern):
                blk(x, lengths)


def test_models_forward_ragged_keeps_raising_and_points_to_the_blocks():
    from sudo_rm_rf_amd.dnn.models.attentive_sudormrf_v2 import SuDORMRF
    m = SuDORMRF(out_channels=8, in_channels=16, num_blocks=1, upsampling_depth=2, enc_kernel_size=5, enc_num_basis=8)
    with pytest.raises(NotImplementedError, match=r"AttentiveUConvBlock\.forward\(x, lengths\)"):
        m.forward_ragged(torch.zeros(2, 1, 64), [64, 32])


# ---- the definition, in fp64 torch -----------------------------------------------------------------------------------------------
def _sd(name, prefix):
    z = np.load(rc.path(name))
    sd = {prefix + k[len("param."):]: torch.as_tensor(z[k]).double() for k in z.files if k.startswith("param.")}
    c = rc.CASES[name]
    Ld = c["L"] >> (c.get("depth", 1) - 1)
    pe = torch.zeros(1, Ld + 7, c["emb"], dtype=torch.float64)
    pe[0, :Ld] = torch.as_tensor(z["pe"]).double()
    pe[0, Ld:] = float("nan")
    sd[prefix + ("attention." if c["module"] == "block" else "") + "pos_enc.pe"] = pe
    return z, sd, c


@pytest.mark.parametrize("name", list(rc.CASES))
def test_reference_restated_on_a_slice_matches_the_fixture(name):
    z, sd, c = _sd(name, "m.")
    x = torch.as_tensor(z["x"]).double()
    want = torch.as_tensor(z["out"])
    for b, n in enumerate(c["lengths"]):
        xb = x[b:b + 1, :, :n]
        if c["module"] == "block":
            got = ar.block(xb, sd, "m.", c["depth"], c["heads"])
        else:
            a = ar.gln(xb, sd["m.in_norm.gamma"], sd["m.in_norm.beta"]) if c["lazy"] else xb
            got = ar.transformer_layer(a, sd, "m.", c["heads"])
        err = (got - want[b:b + 1, :, :n]).abs().max().item()
        assert err <= 1e-10, (name, b, err)          # the restatement IS the reference's module on the slice
        assert want[b, :, n:].abs().sum().item() == 0.0


@pytest.mark.parametrize("Cc,L,n", [(24, 26, 13), (24, 26, 5), (32, 13, 1), (512, 400, 201)])
def test_scaled_sums_under_the_row_stride_count_give_the_slices_own_moments(Cc, L, n):
    g = torch.Generator().manual_seed(Cc + 31 * L + n)
    x = torch.randn(Cc, L, generator=g, dtype=torch.float64) * 3 + 1.5
    own = x[:, :n]
    s, q = own.sum() * (L / n), (own * own).sum() * (L / n)
    inv = 1.0 / (Cc * L)                      # the count a uniform kernel assumes
    mean = s * inv
    var = q * inv - mean * mean
    assert abs(mean.item() - own.mean().item()) <= 1e-12
    assert abs(var.item() - own.var(unbiased=False).item()) <= 1e-12


def test_the_packed_ragged_gemm_gate_is_the_librarys_own():
    """ragged.pw_conv_supported asks srf_pw_conv_packed_ragged_supported (no GPU needed) and adds the tensors' 16-byte alignment"""
    from sudo_rm_rf_amd import _lib, ragged
    assert ragged.pw_conv_supported(2, 256, 512, 512, [512, 260])
    assert ragged.pw_conv_supported(2, 512, 256, 512, [512, 260])
    assert not ragged.pw_conv_supported(2, 512, 128, 512, [512, 260])          # fewer than 192 outputs: the v2 default's res_conv
    assert not ragged.pw_conv_supported(2, 256, 512, 512, [512, 258])          # an example off the grid of 4
    assert not ragged.pw_conv_supported(2, 256, 512, 510, [508, 260])          # the row stride off it
    assert not ragged.pw_conv_supported(2, 256, 512, 512, [516, 260])          # an example above the row stride
    assert not ragged.pw_conv_supported(3, 256, 512, 512, [512, 260])          # a table of another size
    assert not ragged.pw_conv_supported(128, 4096, 512, 4096, [4096] * 128)    # beyond the kernel's 32-bit reach
    buf = torch.zeros(64)
    assert ragged.pw_conv_supported(2, 256, 512, 512, [512, 260], buf[4:], None)
    assert not ragged.pw_conv_supported(2, 256, 512, 512, [512, 260], buf[4:], buf[5:])
    lib = _lib.load()
    lib.srf_set_kernel_mode(1)
    try:
        assert not ragged.pw_conv_supported(2, 256, 512, 512, [512, 260])      # generic kernels only: the uniform fallback
    finally:
        lib.srf_set_kernel_mode(0)
