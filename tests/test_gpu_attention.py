"""srf_mha_attention and the transformer layer's two glue kernels against fp64 restatements on the same inputs.

Tolerance of the attention kernel: not invented -- the same attention computed by torch in fp32 on the CPU deviates from the
fp64 one by some max-abs amount; the kernel may deviate by 8 times that, relative to max |ref| (the factor allows for another
summation order over up to 256 channels and 321 keys).  Dispatch is asserted by profiler name; placement runs the op off the
16-byte grid inside the guard-banded arena of tests/placement.py with the output pre-filled with NaN."""
import functools
import math

import pytest
import torch

from tests import attentive_ref as ar
from tests import placement as pl

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (Bt, H, d, Lq, Lk): smallest MFMA shape | fewer keys than a tile | one key | two past a 128 boundary | the __main__ shapes
# (201 positions, and the issue's 202) | several key tiles + a remainder | generic form, odd rows | Lq != Lk
# | head dimensions that are no multiple of 32, so that a 32-channel chunk of the MFMA form is half full or skipped (with
# d in {16, 32, 64, 256} "c * 32 < d" never prunes a chunk and "c * 32 + 2 r < d" never goes false past the first):
# NCH = 2, second chunk half full | NCH = 4, third half full, fourth skipped | NCH = 8, fifth half full, three skipped
SHAPES = [(2, 3, 16, 26, 26), (3, 1, 64, 2, 2), (1, 4, 256, 1, 1), (2, 4, 256, 130, 130), (1, 3, 256, 202, 202),
          (1, 3, 256, 201, 201), (1, 2, 32, 321, 321), (2, 3, 24, 25, 25), (2, 1, 64, 70, 45),
          (1, 2, 48, 33, 33), (1, 1, 80, 5, 37), (1, 1, 144, 40, 70)]
LARGE = (2, 4, 256, 130, 130)          # run once more with logits of +-80


def _id(s):
    return "B%d_H%d_d%d_Lq%d_Lk%d" % s


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    from sudo_rm_rf_amd import _lib, ops
    _lib.load()
    ops.set_kernel_mode(0)
    ops.set_debug_flags(0)
    yield
    ops.set_kernel_mode(0)


@functools.lru_cache(maxsize=None)
def case(shape, q_gain=1.0):
    """(q, k, v in fp32, fp64 reference, bar): computed once per shape, shared by the tests, never written to"""
    Bt, H, d, Lq, Lk = shape
    g = torch.Generator().manual_seed(1000 * d + Lq + 7 * Lk)
    q = (torch.randn(Bt, H * d, Lq, generator=g, dtype=torch.float64) * q_gain).float()
    k = torch.randn(Bt, H * d, Lk, generator=g, dtype=torch.float64).float()
    v = torch.randn(Bt, H * d, Lk, generator=g, dtype=torch.float64).float()
    ref = ar.attention(q.double(), k.double(), v.double(), H)
    fp32 = ar.attention(q, k, v, H).double()
    dev32 = (fp32 - ref).abs().max().item()
    return q, k, v, ref, dev32


def check(out, shape, q_gain=1.0):
    q, k, v, ref, dev32 = case(shape, q_gain)
    assert out.shape == ref.shape
    assert torch.isfinite(out).all()
    scale = ref.abs().max().item()
    err = (out.double().cpu() - ref).abs().max().item()
    print("%s gain %g: kernel err %.3e, torch fp32 dev %.3e, bar %.3e (relative to max|ref| = %.3f: %.3e vs %.3e)"
          % (_id(shape), q_gain, err, dev32, 8 * dev32, scale, err / scale, 8 * dev32 / scale))
    assert err / scale <= 8 * dev32 / scale


def run(shape, q_gain=1.0):
    from sudo_rm_rf_amd import attention, ops
    q, k, v, _, _ = case(shape, q_gain)
    with ops.kernel_trace(DEV) as tr:
        out = attention.mha_attention(q.to(DEV), k.to(DEV), v.to(DEV), shape[1])
    torch.cuda.synchronize()
    return out, tr


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_attention_matches_fp64_and_dispatch(shape):
    from sudo_rm_rf_amd import attention
    out, tr = run(shape)
    d = shape[2]
    mfma = d % 16 == 0 and 16 <= d <= 256
    assert attention.mha_attention_mfma_supported(d) == mfma
    assert [n for n, _ in tr.launches] == ["mha_attention_mfma" if mfma else "mha_attention_generic"]
    check(out, shape)


def test_attention_large_logits_stay_finite_and_correct():
    q, k, _, _, _ = case(LARGE, 20.0)
    logits = torch.einsum("bhdl,bhds->bhls", q.double().reshape(2, 4, 256, -1), k.double().reshape(2, 4, 256, -1)) / 16.0
    assert logits.abs().max().item() >= 80.0
    out, tr = run(LARGE, 20.0)
    assert tr.names == {"mha_attention_mfma"}
    check(out, LARGE, 20.0)


def test_attention_generic_kernel_serves_mfma_shapes_in_kernel_mode_1():
    from sudo_rm_rf_amd import attention, ops
    shape = (2, 3, 16, 26, 26)
    ops.set_kernel_mode(1)
    try:
        assert not attention.mha_attention_mfma_supported(16)
        out, tr = run(shape)
    finally:
        ops.set_kernel_mode(0)
    assert tr.names == {"mha_attention_generic"}
    check(out, shape)


def test_attention_refuses_bad_arguments_before_launching():
    from sudo_rm_rf_amd import attention
    from sudo_rm_rf_amd._lib import SrfError
    q = torch.zeros(1, 2 * 1040, 3, device=DEV)
    with pytest.raises(SrfError, match="d = 1040"):
        attention.mha_attention(q, q, q, 2)
    with pytest.raises(SrfError, match="heads"):
        attention.mha_attention(q, q, q, 7)


@pytest.fixture(scope="module")
def arena():
    return pl.Arena(DEV, 64 << 20)


@pytest.mark.parametrize("shape", [(2, 3, 16, 26, 26), (2, 4, 256, 130, 130), (2, 3, 24, 25, 25), (2, 1, 64, 70, 45),
                                   (1, 2, 48, 33, 33)], ids=_id)
@pytest.mark.parametrize("shifts", [(0, 0, 0, 0), (1, 2, 3, 1), (3, 1, 2, 3)], ids=lambda s: "shift%d%d%d%d" % s)
def test_attention_off_the_16_byte_grid_with_guard_bands(arena, shape, shifts):
    from sudo_rm_rf_amd import attention
    q, k, v, _, _ = case(shape)
    arena.reset()
    dq = arena.put(q, shift_floats=shifts[0], name="q")
    dk = arena.put(k, shift_floats=shifts[1], name="k")
    dv = arena.put(v, shift_floats=shifts[2], name="v")
    o = arena.place(q.shape, shift_floats=shifts[3], name="o")
    o.fill_(float("nan"))
    attention.mha_attention(dq, dk, dv, shape[1], out=o)
    torch.cuda.synchronize()
    arena.check()
    arena.assert_clean(o)
    for t, h in ((dq, q), (dk, k), (dv, v)):
        assert torch.equal(t.cpu(), h)
    check(o, shape)


# ---- the glue kernels -------------------------------------------------------------------------------------------------
def _sums(x64):
    xf = x64.reshape(x64.shape[0], -1)
    s = torch.zeros(x64.shape[0], 64, 2, dtype=torch.float64)
    s[:, 0, 0] = xf.sum(1)
    s[:, 5, 1] = (xf * xf).sum(1)          # (any bucket: the statistic is the total over the buckets)
    return s


@pytest.mark.parametrize("Bt,C,L", [(2, 64, 26), (3, 33, 2), (1, 70, 131)])
@pytest.mark.parametrize("shift", [0, 1])
def test_posenc_apply(arena, Bt, C, L, shift):
    from sudo_rm_rf_amd import attention
    g = torch.Generator().manual_seed(C + L)
    a = torch.randn(Bt, C, L, generator=g, dtype=torch.float64).float()
    pe = torch.randn(1, 150, C, generator=g, dtype=torch.float64).float()
    gamma = (torch.rand(C, generator=g) + 0.5).float()
    beta = (torch.rand(C, generator=g) - 0.5).float()
    want = ar.gln(a.double(), gamma.double(), beta.double()) + pe[0, :L].double().t()[None]
    arena.reset()
    da, dpe = arena.put(a, shift_floats=shift, name="a"), arena.put(pe, shift_floats=(shift * 3) % 4, name="pe")
    dg, db = arena.put(gamma, shift_floats=shift * 2, name="gamma"), arena.put(beta, shift_floats=shift, name="beta")
    ds = arena.put(_sums(a.double()), dtype=torch.float64, name="sums")
    x = arena.place(a.shape, shift_floats=shift * 3, name="x")
    x.fill_(float("nan"))
    attention.posenc_apply(da, dpe, ds, dg, db, out=x)
    plain = attention.posenc_apply(da, dpe)
    torch.cuda.synchronize()
    arena.check()
    arena.assert_clean(x)
    assert (x.double().cpu() - want).abs().max().item() <= 1e-5
    assert (plain.double().cpu() - (a.double() + pe[0, :L].double().t()[None])).abs().max().item() <= 1e-6
    from sudo_rm_rf_amd._lib import SrfError
    with pytest.raises(SrfError, match="max_len = 150"):
        attention.posenc_apply(torch.zeros(1, C, 151, device=DEV), dpe)


@pytest.mark.parametrize("Bt,C,L", [(2, 64, 26), (3, 5, 2), (1, 7, 1500)])
@pytest.mark.parametrize("shift", [0, 1])
def test_gln_apply2_add(arena, Bt, C, L, shift):
    from sudo_rm_rf_amd import attention
    g = torch.Generator().manual_seed(3 * C + L)
    f = (torch.randn(Bt, C, L, generator=g, dtype=torch.float64) * 2 + 0.3).float()
    y = (torch.randn(Bt, C, L, generator=g, dtype=torch.float64) - 0.2).float()
    par = [(torch.rand(C, generator=g) + 0.5).float() for _ in range(2)] + [(torch.rand(C, generator=g) - 0.5).float() for _ in range(2)]
    slope = torch.tensor([0.2])
    want = ar.prelu(ar.gln(f.double(), par[0].double(), par[2].double()), 0.2) + ar.gln(y.double(), par[1].double(), par[3].double())
    arena.reset()
    df, dy = arena.put(f, shift_floats=shift, name="f"), arena.put(y, shift_floats=shift * 2, name="y")
    dp = [arena.put(t, shift_floats=(shift * (i + 1)) % 4, name="p%d" % i) for i, t in enumerate(par)]
    dsl = arena.put(slope, shift_floats=shift, name="slope")
    sf = arena.put(_sums(f.double()), dtype=torch.float64, name="f_sums")
    sy = arena.put(_sums(y.double()), dtype=torch.float64, name="y_sums")
    so = arena.place((Bt, 64, 2), dtype=torch.float64, name="out_sums", zero=True)
    z = arena.place(f.shape, shift_floats=shift * 3, name="z")
    z.fill_(float("nan"))
    attention.gln_apply2_add(df, sf, dp[0], dp[2], dsl, dy, sy, dp[1], dp[3], out_sums=so, out=z)
    torch.cuda.synchronize()
    arena.check()
    arena.assert_clean(z)
    assert (z.double().cpu() - want).abs().max().item() <= 2e-5
    got = so.cpu().sum(1)
    wf = want.reshape(Bt, -1)
    assert ((got[:, 0] - wf.sum(1)).abs() <= 4e-6 * wf.abs().sum(1) + 1e-9).all()
    assert ((got[:, 1] - (wf * wf).sum(1)).abs() <= 4e-6 * (wf * wf).sum(1) + 1e-9).all()
