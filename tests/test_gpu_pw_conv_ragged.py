"""srf_pw_conv_ragged on the GPU: the ragged form of the 128 x 128 split-bf16 GEMM, in the four forms
the attentive walk uses, against an fp64 restatement on each example's own slice.  Bar: 1e-4 max-abs, the project's own for the
split-bf16 GEMMs.  The output is allocated inside a poisoned arena (tests/placement.py): guard bands around y, exact zeros from
frames[b] to the end of the tile that holds own columns, and a skipped tile still holding the poison -- nothing was stored there.
Worst errors measured on an MI355X: profiles/ragged_forward_attentive.txt."""
import pytest
import torch

from tests.placement import SENTINEL_WORD, Arena
from tests.test_gpu_ops import check_sums

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR = 1e-4
TILE = 128

# Cin, Cout, L, frames
CASES = {
    # two column tiles, the second 4 wide; a length off the grid of 4; an example whose second tile lies wholly past its end
    "c1": (64, 32, 132, [132, 129, 1]),
    # a partial second row tile (160 = 128 + 32); an end exactly on a tile boundary; one just past it; a length below 4
    "c2": (128, 160, 256, [256, 128, 130, 3]),
}
# form -> (prologue, residual, out_sums): what the walk runs -- plain (Q/K/V), the O projection, the FFN / bottleneck, res_conv
FORMS = {"pro0": (0, False, False), "pro0_res_sums": (0, True, True), "pro1_sums": (1, False, True), "pro2_res": (2, True, False)}


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    from sudo_rm_rf_amd import _lib, ops
    _lib.load()
    ops.set_kernel_mode(0)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


_CACHE = {}


def _case(name):
    """Operands (host, fp32) of a case, drawn once and shared; nothing in it is modified."""
    if name not in _CACHE:
        Cin, Cout, L, frames = CASES[name]
        g = torch.Generator().manual_seed(900 + len(name) + Cin)
        Bt = len(frames)
        r = lambda *s, scale=1.0, shift=0.0: torch.randn(*s, generator=g) * scale + shift
        _CACHE[name] = dict(x=r(Bt, Cin, L, scale=1.5, shift=0.3), w=r(Cout, Cin, scale=Cin ** -0.5), bias=r(Cout, scale=0.2),
                            res=r(Bt, Cout, L), gamma=r(Cin, scale=0.2, shift=1.0), beta=r(Cin, scale=0.2),
                            prelu=torch.tensor([0.25]))
    return _CACHE[name]


def _own_sums(x, frames):
    s = torch.zeros(x.shape[0], 64, 2, dtype=torch.float64)
    for b, n in enumerate(frames):
        own = x[b, :, :n].double()
        s[b, 0, 0], s[b, 0, 1] = own.sum(), (own * own).sum()
    return s


def _want(c, frames, pro, with_res):
    """fp64, per example on its own slice: y[b] [Cout, frames[b]]"""
    out = []
    for b, n in enumerate(frames):
        x = c["x"][b, :, :n].double()
        if pro in (1, 2):
            mu = x.mean()
            var = ((x - mu) ** 2).mean()
            x = c["gamma"].double()[:, None] * (x - mu) / (var + 1e-8).sqrt() + c["beta"].double()[:, None]
        if pro == 2:
            x = torch.where(x >= 0, x, c["prelu"].double() * x)
        y = c["w"].double() @ x + c["bias"].double()[:, None]
        if with_res:
            y = y + c["res"][b, :, :n].double()
        out.append(y)
    return out


def _run(name, form, x, res, trace=None, arena=None):
    """-> (y, out_sums or None); arena: y is allocated inside it"""
    import contextlib

    from sudo_rm_rf_amd import ops, ragged
    c = _case(name)
    Cin, Cout, L, frames = CASES[name]
    pro, with_res, with_sums = FORMS[form]
    d = lambda t: t.to(DEV).contiguous()
    kw = {}
    if pro in (1, 2):
        kw.update(in_sums=_own_sums(c["x"], frames).to(DEV), in_gamma=d(c["gamma"]), in_beta=d(c["beta"]))
    if pro == 2:
        kw.update(in_prelu=d(c["prelu"]))
    if with_res:
        kw.update(residual=d(res))
    sums = ops.new_sums(len(frames), DEV) if with_sums else None
    with (arena.allocating(ragged, names=("y",)) if arena else contextlib.nullcontext()), ops.kernel_trace(DEV) as tr:
        y = ragged.pw_conv_mfma(d(x), d(c["w"]), d(c["bias"]), frames, out_sums=sums, **kw)
    torch.cuda.synchronize()
    if trace is not None:
        trace.extend(n for n, _ in tr.launches)
    return y, sums


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(CASES))
def test_every_example_alone_on_its_slice(name, form):
    from sudo_rm_rf_amd import ragged
    c = _case(name)
    Cin, Cout, L, frames = CASES[name]
    pro, with_res, with_sums = FORMS[form]
    assert ragged.pw_conv_mfma_supported(len(frames), Cin, Cout, L, frames)
    arena = Arena(DEV, 4 << 20)
    names = []
    y, sums = _run(name, form, c["x"], c["res"], names, arena)
    arena.check()                                            # guard bands around y untouched
    assert names == ["pw_conv_bf16x3_ragged<%d>" % pro], names
    want = _want(c, frames, pro, with_res)
    got, raw = y.cpu(), _bits(y)
    worst = 0.0
    for b, n in enumerate(frames):
        err = (got[b, :, :n].double() - want[b]).abs().max().item()
        worst = max(worst, err)
        end = min(L, -(-n // TILE) * TILE)                   # the end of the tile that holds the last own column
        assert (raw[b, :, n:end] == 0).all(), "%s %s: example %d is not exact +0 on [%d, %d)" % (name, form, b, n, end)
        assert (raw[b, :, end:] == SENTINEL_WORD).all(), "%s %s: example %d: a skipped tile was written" % (name, form, b)
        assert torch.isfinite(got[b, :, :n]).all()
    print("  %s %s: worst max-abs error %.3g" % (name, form, worst))
    assert worst <= BAR, (name, form, worst)
    if with_sums:
        # the sums of the kernel's own fp32 outputs over own columns (what the next norm needs), to check_sums' rounding bound
        for b, n in enumerate(frames):
            check_sums(sums[b:b + 1], got[b:b + 1, :, :n].double(), "%s %s example %d" % (name, form, b))


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(CASES))
def test_nan_padding_and_other_rows_change_no_bit(name, form):
    c = _case(name)
    Cin, Cout, L, frames = CASES[name]
    y0, s0 = _run(name, form, c["x"], c["res"])
    # NaN past every length, in x and in the residual
    x, res = c["x"].clone(), c["res"].clone()
    for b, n in enumerate(frames):
        x[b, :, n:] = float("nan")
        res[b, :, n:] = float("nan")
    y1, s1 = _run(name, form, x, res)
    # other rows' content: rows 1.. replaced, row 0 must keep its bits; then row 0 replaced, the last row must keep its own
    g = torch.Generator().manual_seed(5)
    xa, xb = c["x"].clone(), c["x"].clone()
    xa[1:] = torch.randn(xa[1:].shape, generator=g) * 3
    xb[0] = torch.randn(xb[0].shape, generator=g) * 3
    for b, n in enumerate(frames):
        end = min(L, -(-n // TILE) * TILE)
        assert torch.equal(_bits(y0)[b, :, :end], _bits(y1)[b, :, :end]), "%s %s: NaN padding changed example %d" % (name, form, b)
    if s0 is not None:
        assert torch.equal(s0.cpu(), s1.cpu()) and torch.isfinite(s1).all()
    # (the statistics of a norm on load are those of the unchanged rows' own content: _run builds them from the case's x)
    ya, sa = _run(name, form, xa, c["res"])
    yb, sb = _run(name, form, xb, c["res"])
    assert torch.equal(_bits(y0)[0, :, :frames[0]], _bits(ya)[0, :, :frames[0]]), "%s %s: row 0 changed with the other rows" % (name, form)
    assert torch.equal(_bits(y0)[-1, :, :frames[-1]], _bits(yb)[-1, :, :frames[-1]]), "%s %s: the last row changed with the others" % (name, form)
    if s0 is not None:      # ... and so are the row's own out_sums buckets
        assert torch.equal(s0[0].cpu(), sa[0].cpu()) and torch.equal(s0[-1].cpu(), sb[-1].cpu())


def test_the_entry_refuses_an_unaligned_x_and_a_bad_table():
    from sudo_rm_rf_amd import _lib, ragged
    c = _case("c1")
    Cin, Cout, L, frames = CASES["c1"]
    d = lambda t: t.to(DEV).contiguous()
    flat = torch.zeros(len(frames) * Cin * L + 4, device=DEV)
    x_off = flat[1:1 + len(frames) * Cin * L].view(len(frames), Cin, L)        # float aligned, off the 16-byte grid
    assert x_off.data_ptr() % 16 == 4
    with pytest.raises(_lib.SrfError, match="'x' is not 16-byte aligned"):
        ragged.pw_conv_mfma(x_off, d(c["w"]), d(c["bias"]), frames)
    with pytest.raises(_lib.SrfError, match="example 1 has 133 frames"):
        ragged.pw_conv_mfma(d(c["x"]), d(c["w"]), d(c["bias"]), [132, 133, 1])
    with pytest.raises(_lib.SrfError, match="example 2 has 0 frames"):
        ragged.pw_conv_mfma(d(c["x"]), d(c["w"]), d(c["bias"]), [132, 129, 0])
