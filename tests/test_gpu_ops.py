"""Per-kernel parity: every C-ABI entry point vs an fp64 torch/numpy reference of the same op.

Tolerances are for fp32 arithmetic with re-association (no reduced-precision operands anywhere)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from sudo_rm_rf_amd.ops import DebugFlag

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    from sudo_rm_rf_amd import _lib
    _lib.load()
    yield
    from sudo_rm_rf_amd import ops
    ops.set_kernel_mode(0)


@pytest.fixture(params=[0, 1], ids=["fast", "generic"])
def mode(request):
    from sudo_rm_rf_amd import ops
    ops.set_kernel_mode(request.param)
    yield request.param
    ops.set_kernel_mode(0)


def rnd(*shape, seed=0, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale + shift)


def dev32(t):
    return t.to(torch.float32).to(DEV).contiguous()


def gln64(x, gamma, beta):
    dims = list(range(1, x.dim()))
    mu = x.mean(dim=dims, keepdim=True)
    var = ((x - mu) ** 2).mean(dim=dims, keepdim=True)
    shape = [1, -1] + [1] * (x.dim() - 2)
    return gamma.view(shape) * (x - mu) / (var + 1e-8).sqrt() + beta.view(shape)


def sums64(x):
    """exact fp64 {sum, sumsq} per group in the library's bucketed layout [groups, 64, 2] (bucket 0)."""
    xf = x.reshape(x.shape[0], -1)
    out = torch.zeros(x.shape[0], 64, 2, dtype=torch.float64)
    out[:, 0, 0] = xf.sum(1)
    out[:, 0, 1] = (xf * xf).sum(1)
    return out


def check(got, want, atol, what=""):
    got = got.detach().cpu().to(torch.float64)
    err = (got - want).abs().max().item()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert err <= atol, f"{what}: max abs err {err:.3e} > {atol:.1e}"


def check_sums(got, x64, what=""):
    """bucketed fp64 sums of the kernel's own fp32 outputs vs the fp64 reference tensor: the only
    differences are the outputs' fp32 rounding, so bound them by eps * sum|x| and eps * sum x^2."""
    xf = x64.reshape(x64.shape[0], -1)
    got = got.cpu().sum(1)                       # total over buckets -> [groups, 2]
    assert ((got[:, 0] - xf.sum(1)).abs() <= 4e-6 * xf.abs().sum(1) + 1e-9).all(), f"{what}: sum"
    assert ((got[:, 1] - (xf * xf).sum(1)).abs() <= 4e-6 * (xf * xf).sum(1) + 1e-9).all(), f"{what}: sumsq"


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,K,T,N,Bt", [(1, 21, 32000, 96, 2), (1, 21, 1237, 33, 3), (2, 11, 700, 16, 2),
                                        (1, 5, 64, 8, 1)])
def test_encoder(mode, A, K, T, N, Bt):
    from sudo_rm_rf_amd import ops
    h = K // 2
    D = 3
    nls = h * 2 ** D
    Tp = nls if T < nls else (T // nls + (1 if T % nls else 0)) * nls
    L = (Tp + 2 * h - K) // h + 1
    x, w = rnd(Bt, A, T, seed=1), rnd(N, A, K, seed=2, scale=0.3)
    xp = torch.zeros(Bt, A, Tp, dtype=torch.float64)
    xp[..., :T] = x
    want = F.conv1d(xp, w, None, stride=h, padding=h)
    sums = ops.new_sums(Bt, DEV)
    got = ops.encoder(dev32(x), dev32(w), L, sums)
    check(got, want, 2e-5, "encoder")
    check_sums(sums, want, "encoder sums")


def test_gln_standalone():
    from sudo_rm_rf_amd import ops
    x, g, b = rnd(3, 40, 333, seed=3, scale=2.0, shift=0.7), rnd(40, seed=4), rnd(40, seed=5)
    got = ops.glob_ln(dev32(x), dev32(g), dev32(b))
    check(got, gln64(x, g, b), 2e-5, "glob_ln")


# ---------------------------------------------------------------------------------------------
PW_SHAPES = [  # Bt, Cin, Cout, L
    (2, 256, 512, 3200),   # proj_1x1 of cfg2
    (2, 512, 256, 800),    # res_conv-like
    (1, 64, 42, 200),      # partial M tile (decoder frame GEMM shape), partial N tile
    (3, 48, 160, 132),     # nothing a multiple of the tile
    (4, 16, 32, 404),      # GroupComm per-group shapes (register-resident streaming kernel)
    (3, 32, 16, 1000),
    (2, 8, 64, 64),
    (2, 32, 64, 260),
    (2, 16, 32, 402),      # same channels, L % 4 != 0 -> generic kernel
    (2, 24, 20, 50),       # generic: Cin not multiple of 16, L not multiple of 4
]


@pytest.mark.parametrize("Bt,Cin,Cout,L", PW_SHAPES)
@pytest.mark.parametrize("pro", [0, 1, 2, 3])
def test_pw_conv(mode, Bt, Cin, Cout, L, pro):
    from sudo_rm_rf_amd import ops
    x = rnd(Bt, Cin, L, seed=10, scale=1.5, shift=0.3)
    w = rnd(Cout, Cin, 1, seed=11, scale=Cin ** -0.5)
    bias = rnd(Cout, seed=12, scale=0.2)
    gamma, beta = rnd(Cin, seed=13, scale=0.3, shift=1.0), rnd(Cin, seed=14, scale=0.3)
    slope = torch.tensor([0.17], dtype=torch.float64)
    res = rnd(Bt, Cout, L, seed=15)
    xin = x
    kw = {}
    if pro in (1, 2):
        xin = gln64(x, gamma, beta)
        kw.update(in_sums=sums64(x).to(DEV), in_gamma=dev32(gamma), in_beta=dev32(beta))
    if pro in (2, 3):
        xin = torch.where(xin >= 0, xin, slope * xin)
        kw.update(in_prelu=dev32(slope))
    want = F.conv1d(xin, w, bias) + res
    osums = ops.new_sums(Bt, DEV)
    got = ops.pw_conv(dev32(x), dev32(w), dev32(bias), residual=dev32(res), out_sums=osums, **kw)
    # the sums handed in are exact fp64 sums of the fp64 tensor -> only fp32 arithmetic error remains
    check(got, want, 5e-5, f"pw_conv pro={pro}")
    check_sums(osums, want, "pw_conv sums")


@pytest.mark.parametrize("Bt,Cin,Cout,L", [(32, 64, 200, 3300),   # 1664 tiles: persistent kernel, partial M and N tiles
                                          (3, 128, 72, 333)])     # one tile per block
@pytest.mark.parametrize("pro", [0, 2])
def test_pw_conv_buffer_and_pointer_loads_agree(Bt, Cin, Cout, L, pro):
    """The split-bf16 GEMMs fetch their operands with buffer loads (out-of-range rows read 0); debug flag 1<<27 selects
    the 64-bit pointer form kept for tensors beyond 2 GB.  Same arithmetic -> bit-identical results."""
    from sudo_rm_rf_amd import ops
    ops.set_kernel_mode(0)
    x, w, bias = dev32(rnd(Bt, Cin, L, seed=30)), dev32(rnd(Cout, Cin, 1, seed=31, scale=0.1)), dev32(rnd(Cout, seed=32))
    kw = {}
    if pro == 2:
        kw = dict(in_sums=sums64(x.double().cpu()).to(DEV), in_gamma=dev32(rnd(Cin, seed=33, shift=1.0)),
                  in_beta=dev32(rnd(Cin, seed=34)), in_prelu=dev32(torch.tensor([0.2], dtype=torch.float64)))
    want = F.conv1d(x.double().cpu(), w.double().cpu(), bias.double().cpu()) if pro == 0 else None
    a = ops.pw_conv(x, w, bias, **kw)
    with ops.debug_flags(DebugFlag.GEMM_128_POINTER_LOADS):
        b = ops.pw_conv(x, w, bias, **kw)
    assert torch.equal(a, b)
    if want is not None:
        check(a, want, 5e-5, "pw_conv buffer loads")


@pytest.mark.parametrize("Bt,Cin,Cout,L", [(32, 512, 256, 1600), (16, 256, 512, 3200),     # 1664 / 1600 tiles: persistent
                                           (1, 512, 256, 3200), (2, 256, 512, 1632), (1, 128, 1024, 416)])   # small: quarter tiles
@pytest.mark.parametrize("pro", [0, 1, 2, 3])
def test_pw_conv_persistent_variants(Bt, Cin, Cout, L, pro):
    """Every prologue instantiation of the persistent split-bf16 GEMM at model-sized K, in the form that is dispatched
    (buffer loads), the pointer form (flag 1<<27) and the one-tile-per-block kernel (flag 2048): all against an fp64
    reference and against each other.  (The whole-model tests auto-tune a batch split, so they do not necessarily run
    the persistent kernel for every conv.)"""
    from sudo_rm_rf_amd import ops
    ops.set_kernel_mode(0)
    x = dev32(rnd(Bt, Cin, L, seed=40, scale=1.3, shift=0.2))
    w, bias = dev32(rnd(Cout, Cin, 1, seed=41, scale=Cin ** -0.5)), dev32(rnd(Cout, seed=42, scale=0.2))
    res = dev32(rnd(Bt, Cout, L, seed=43))
    kw, xin = {}, x.double().cpu()
    if pro in (1, 2):
        gamma, beta = rnd(Cin, seed=44, scale=0.3, shift=1.0), rnd(Cin, seed=45, scale=0.3)
        kw.update(in_sums=sums64(xin).to(DEV), in_gamma=dev32(gamma), in_beta=dev32(beta))
        xin = gln64(xin, gamma, beta)
    if pro in (2, 3):
        kw.update(in_prelu=dev32(torch.tensor([0.17], dtype=torch.float64)))
        xin = torch.where(xin >= 0, xin, 0.17 * xin)
    want = F.conv1d(xin, w.double().cpu(), bias.double().cpu()) + res.double().cpu()
    outs = {}
    for name, flags in (("dispatched", 0), ("pointer loads", DebugFlag.GEMM_128_POINTER_LOADS),
                        ("one tile per block", DebugFlag.GEMM_128_ONE_TILE_PER_BLOCK)):
        with ops.debug_flags(flags):
            outs[name] = ops.pw_conv(x, w, bias, residual=res, **kw)
    # the 256 x 128 kernel with pre-split weights (what srf_forward dispatches: srf_pwconv_x3w.hip)
    packed = ops.pack_pw_weight(w)
    assert packed is not None
    outs["packed 256x128"] = ops.pw_conv(x, w, bias, residual=res, packed=packed, **kw)
    with ops.debug_flags(DebugFlag.GEMM_256_SWAP_FORMS):   # (round 4) the paired-block form, what srf_forward runs: two co-resident blocks per CU
        outs["packed 256x128, two blocks per CU"] = ops.pw_conv(x, w, bias, residual=res, packed=packed, **kw)
    assert torch.equal(outs["packed 256x128"], outs["packed 256x128, two blocks per CU"])
    for name, got in outs.items():
        check(got, want, 1e-4, "persistent pw_conv pro=%d (%s)" % (pro, name))
    assert torch.equal(outs["dispatched"], outs["pointer loads"])
    # same arithmetic (same splits, same per-accumulator summation order over k): bitwise equal to the 128 x 128 kernels
    assert torch.equal(outs["packed 256x128"], outs["dispatched"])


# ---- the attentive transformer layer's three GEMM forms (srf_attentive.hip), at deepest-level lengths Ld % 4 == 0 ----------
# (a) O_proj: no prologue, residual AND statistics -- srf_x3p_supported refuses that pair, so the 256 x 128 launch is the x3w form
#     under either setting of GEMM_256_SWAP_FORMS; (b) ffn: GlobLN on load, statistics; (c) Q/K/V as one conv: nothing.
# Operands scaled as in test_pw_conv_persistent_variants (w by Cin ** -0.5): neither the outputs nor the random-sign rounding
# error grow with K, so its bars hold at K = 1024 unchanged.
LAYER_FORMS = {"O_proj": (0, True, True), "ffn": (1, False, True), "qkv": (0, False, False)}    # prologue, residual, statistics
MFMA_GEMMS = ("pw_conv_bf16x3", "pw_conv_x3w<", "pw_conv_x3p<", "pw_conv_mfma")


def _layer_form_case(form, Bt, Cin, Cout, L):
    """(x, w, bias, keyword operands, fp64 reference, whether statistics are taken) of one form at one shape"""
    pro, with_res, with_sums = LAYER_FORMS[form]
    x = dev32(rnd(Bt, Cin, L, seed=40, scale=1.3, shift=0.2))
    w, bias = dev32(rnd(Cout, Cin, 1, seed=41, scale=Cin ** -0.5)), dev32(rnd(Cout, seed=42, scale=0.2))
    kw, xin = {}, x.double().cpu()
    if pro == 1:
        gamma, beta = rnd(Cin, seed=44, scale=0.3, shift=1.0), rnd(Cin, seed=45, scale=0.3)
        kw.update(in_sums=sums64(xin).to(DEV), in_gamma=dev32(gamma), in_beta=dev32(beta))
        xin = gln64(xin, gamma, beta)
    want = F.conv1d(xin, w.double().cpu(), bias.double().cpu())
    if with_res:
        kw.update(residual=dev32(rnd(Bt, Cout, L, seed=43)))
        want = want + kw["residual"].double().cpu()
    return x, w, bias, kw, want, with_sums


def _run_layer_form(x, w, bias, kw, with_sums, packed, flags=0):
    from sudo_rm_rf_amd import ops
    sums = ops.new_sums(x.shape[0], DEV) if with_sums else None
    with ops.debug_flags(flags), ops.kernel_trace(DEV) as tr:
        y = ops.pw_conv(x, w, bias, out_sums=sums, packed=packed, **kw)
    torch.cuda.synchronize()
    return y, sums, tr.names


def _report(what, got, want, sums):
    """measured errors, printed before anything is asserted: output max-abs, and the statistics relative to their bars"""
    err = (got.double().cpu() - want).abs().max().item()
    msg = "%s: max abs err %.3e (bar 1.0e-04, max|want| %.2f)" % (what, err, want.abs().max().item())
    if sums is not None:
        wf, tot = want.reshape(want.shape[0], -1), sums.cpu().sum(1)
        e0 = ((tot[:, 0] - wf.sum(1)).abs() / wf.abs().sum(1)).max().item()
        e1 = ((tot[:, 1] - (wf * wf).sum(1)).abs() / (wf * wf).sum(1)).max().item()
        msg += "; sum err %.2e of sum|y|, sumsq err %.2e of sum y^2 (bars 4e-06)" % (e0, e1)
    print(msg)


@pytest.mark.parametrize("form,Bt,Cin,Cout,L", [("O_proj", 32, 1024, 1024, 132),     # 256 tiles: one full n-tile + 4 columns
                                                ("ffn", 32, 1024, 1024, 132),
                                                ("O_proj", 32, 1024, 512, 400),      # the bench shape's O_proj: 256 tiles
                                                ("qkv", 11, 128, 3072, 132)])        # 264 tiles, 12 m-tiles
def test_pw_conv_attentive_layer_forms(form, Bt, Cin, Cout, L):
    """The 256 x 128 kernels at the shapes the attentive layer gives them when the launch fills the chip: as dispatched, under
    GEMM_256_SWAP_FORMS (the form srf_forward prefers) and without the packed image (the 128 x 128 kernels) -- each against fp64
    F.conv1d and its statistics against the fp64 sums, the three bitwise equal (same splits, same summation order over k)."""
    from sudo_rm_rf_amd import ops
    ops.set_kernel_mode(0)
    pro = LAYER_FORMS[form][0]
    x, w, bias, kw, want, with_sums = _layer_form_case(form, Bt, Cin, Cout, L)
    packed = ops.pack_pw_weight(w)
    assert packed is not None
    runs = {"dispatched": _run_layer_form(x, w, bias, kw, with_sums, packed),
            "swapped forms": _run_layer_form(x, w, bias, kw, with_sums, packed, DebugFlag.GEMM_256_SWAP_FORMS),
            "no packed image": _run_layer_form(x, w, bias, kw, with_sums, None)}
    for name, (y, sums, names) in runs.items():
        _report("%s %s (%s, %s)" % (form, (Bt, Cin, Cout, L), name, sorted(names)), y, want, sums)
    assert runs["dispatched"][2] == {"pw_conv_x3w<%d>" % pro}, runs["dispatched"][2]
    # the paired-block form takes every epilogue but residual + statistics
    assert runs["swapped forms"][2] == {"pw_conv_x3w<0>" if form == "O_proj" else "pw_conv_x3p<%d>" % pro}, runs["swapped forms"][2]
    assert all(n.startswith("pw_conv_bf16x3") for n in runs["no packed image"][2]), runs["no packed image"][2]
    for name, (y, sums, _) in runs.items():
        check(y, want, 1e-4, "%s (%s)" % (form, name))
        if with_sums:
            check_sums(sums, want, "%s statistics (%s)" % (form, name))
    assert torch.equal(runs["dispatched"][0], runs["swapped forms"][0])
    assert torch.equal(runs["dispatched"][0], runs["no packed image"][0])


@pytest.mark.parametrize("Cin,Cout", [(64, 3072), (1024, 64), (64, 64),      # the tiny layer's Q/K/V, O_proj, ffn
                                      (512, 3072), (1024, 512)])             # the default model's Q/K/V and O_proj
@pytest.mark.parametrize("L", [4, 28, 124])
def test_pw_conv_attentive_layer_forms_shorter_than_a_tile(Cin, Cout, L):
    """Lengths below one tile of any MFMA GEMM (the attentive layer asks for every Ld >= 4 that is a multiple of 4), batches 1 and
    3, all three forms: an MFMA kernel serves them -- named by the trace -- and is right."""
    from sudo_rm_rf_amd import ops
    ops.set_kernel_mode(0)
    for Bt in (1, 3):
        for form in LAYER_FORMS:
            x, w, bias, kw, want, with_sums = _layer_form_case(form, Bt, Cin, Cout, L)
            y, sums, names = _run_layer_form(x, w, bias, kw, with_sums, ops.pack_pw_weight(w))
            what = "%s %s" % (form, (Bt, Cin, Cout, L))
            _report("%s (%s)" % (what, sorted(names)), y, want, sums)
            assert len(names) == 1 and all(n.startswith(MFMA_GEMMS) for n in names), (what, names)
            check(y, want, 1e-4, what)
            if with_sums:
                check_sums(sums, want, what + " statistics")


def test_pw_conv_o_proj_form_inside_guard_bands():
    """O_proj's form (residual + statistics on the 256 x 128 kernel) with x, residual, bias and the output inside the guard-banded
    arena of tests/placement.py, on the 16-byte grid, the output pre-filled with NaN: the 4-column last tile stores nothing outside
    the output (arena.check) and leaves no element unwritten (assert_clean); a store past column 132 of a row lands in the next
    row and fails the comparison."""
    from sudo_rm_rf_amd import ops
    from tests import placement as pl
    ops.set_kernel_mode(0)
    Bt, Cin, Cout, L = 32, 1024, 1024, 132
    x, w, bias, kw, want, _ = _layer_form_case("O_proj", Bt, Cin, Cout, L)
    packed = ops.pack_pw_weight(w)
    sums = ops.new_sums(Bt, DEV)
    arena = pl.Arena(DEV, 64 << 20)
    ax, ab = arena.put(x, name="x"), arena.put(bias, name="bias")
    ares = arena.put(kw["residual"], name="residual")
    with arena.allocating(ops, names=("y",)) as made, ops.kernel_trace(DEV) as tr:
        y = ops.pw_conv(ax, w, ab, residual=ares, out_sums=sums, packed=packed)
    torch.cuda.synchronize()
    assert [n for n, _ in made] == ["y"] and arena.owns(y) and y.data_ptr() % 16 == 0 and ares.data_ptr() % 16 == 0
    assert tr.names == {"pw_conv_x3w<0>"}, tr.names
    arena.check()
    arena.assert_clean(y)
    assert torch.equal(ares, kw["residual"]) and torch.equal(ax, x)
    _report("O_proj %s in the arena" % ((Bt, Cin, Cout, L),), y, want, sums)
    check(y, want, 1e-4, "O_proj in the arena")
    check_sums(sums, want, "O_proj in the arena: statistics")


@pytest.mark.parametrize("Bt,Cin1,Cout2,L", [(32, 512, 512, 3200),      # cfg 2: res_conv -> proj_1x1 (800 tiles on 512 blocks: two rounds)
                                             (12, 512, 512, 3200),      # a sub-batch of the stream split: one round, blocks with one tile
                                             (24, 256, 384, 1604),      # ragged last tile (L % 128 = 68), three passes of conv 2, K1 = 256
                                             (40, 128, 128, 1000)])     # shortest k loop (8 steps), one pass, ragged
@pytest.mark.parametrize("pro", [0, 1, 2])
def test_pw_conv_pair_is_bitwise_the_two_launches(Bt, Cin1, Cout2, L, pro):
    """srf_pw_conv_pair (round 5: res_conv / bottleneck + the next block's proj_1x1 in one launch, the 256-channel tensor handed
    over in registers) against the two srf_pw_conv_packed launches it replaces -- BIT FOR BIT on both outputs -- against an fp64
    reference, its statistics against the fp64 sums; the form with full-drain waits (flag 1 << 23) must agree bitwise too (a
    difference = a miscounted vmcnt in the DMA pipeline), and so must the persistent-block form (flag 1 << 21: several tiles per
    block, the operand pipeline running across tile boundaries -- what launches beyond 16 rounds of the chip get).
    pro 0 = no prologue, with residual: the backward's data-gradient pair (W_proj^T g + skip gradient, then W_res^T of it)."""
    from sudo_rm_rf_amd import ops
    ops.set_kernel_mode(0)
    Cmid = 256
    if not ops.pw_conv_pair_supported(Bt, Cin1, Cmid, Cout2, L):
        pytest.skip("shape not served on this device")
    x = dev32(rnd(Bt, Cin1, L, seed=50, scale=1.3, shift=0.2))
    w1, b1 = dev32(rnd(Cmid, Cin1, 1, seed=51, scale=Cin1 ** -0.5)), dev32(rnd(Cmid, seed=52, scale=0.2))
    w2, b2 = dev32(rnd(Cout2, Cmid, 1, seed=53, scale=Cmid ** -0.5)), dev32(rnd(Cout2, seed=54, scale=0.2))
    res = dev32(rnd(Bt, Cmid, L, seed=55)) if pro != 1 else None
    gamma, beta = rnd(Cin1, seed=56, scale=0.3, shift=1.0), rnd(Cin1, seed=57, scale=0.3)
    xin = x.double().cpu()
    kw = dict(in_sums=None, in_gamma=None, in_beta=None)
    if pro != 0:
        kw = dict(in_sums=sums64(xin).to(DEV), in_gamma=dev32(gamma), in_beta=dev32(beta))
        xin = gln64(xin, gamma, beta)
    slope = None
    if pro == 2:
        slope = dev32(torch.tensor([0.17], dtype=torch.float64))
        kw.update(in_prelu=slope)
        xin = torch.where(xin >= 0, xin, 0.17 * xin)
    want1 = F.conv1d(xin, w1.double().cpu(), b1.double().cpu())
    if res is not None:
        want1 = want1 + res.double().cpu()
    p1, p2 = ops.pack_pw_weight(w1), ops.pack_pw_weight(w2)
    assert p1 is not None and p2 is not None
    # the two launches
    y_ref = ops.pw_conv(x, w1, b1, residual=res, packed=p1, **kw)
    sums_ref = ops.new_sums(Bt, DEV)
    y2_ref = ops.pw_conv(y_ref, w2, b2, out_sums=sums_ref, packed=p2)
    want2 = F.conv1d(y_ref.double().cpu(), w2.double().cpu(), b2.double().cpu())
    outs = {}
    for name, flags in (("counted waits", 0), ("full drains", DebugFlag.PAIR_FULL_DRAIN), ("persistent blocks", DebugFlag.PAIR_PERSISTENT)):
        with ops.debug_flags(flags):
            sums = ops.new_sums(Bt, DEV)
            y, y2 = ops.pw_conv_pair(x, p1, b1, kw["in_sums"], kw["in_gamma"], kw["in_beta"], slope, res, p2, b2, Cmid, Cout2, out_sums2=sums)
            outs[name] = (y, y2, sums)
    def where(got, ref):      # a failure report that shows the pattern (which examples / row blocks / column phases)
        bad = (got != ref) | torch.isnan(got)
        if not bad.any():
            return ""
        idx = bad.nonzero().cpu()
        return ("%d of %d values differ (max |d| %.3e, nan %d); examples %s; rows/32 %s; columns %% 128 / 32 %s; first %s" %
                (idx.shape[0], got.numel(), (got - ref).abs().nan_to_num(0).max().item(), int(torch.isnan(got).sum()),
                 sorted(set(idx[:, 0].tolist()))[:8], sorted(set((idx[:, 1] // 32).tolist())),
                 sorted(set(((idx[:, 2] % 128) // 32).tolist())), idx[0].tolist()))
    for name, (y, y2, sums) in outs.items():
        msg = where(y, y_ref)
        assert not msg, "pair conv 1 (%s) vs the separate launch: %s" % (name, msg)
        msg = where(y2, y2_ref)
        assert not msg, "pair conv 2 (%s) vs the separate launch: %s" % (name, msg)
        check(y, want1, 1e-4, "pair conv 1 (%s)" % name)
        check(y2, want2, 1e-4, "pair conv 2 (%s)" % name)
        check_sums(sums, y2.double().cpu(), "pair statistics (%s)" % name)
    # twice in a row on the same buffers: a persistent pipeline that leaves state behind would show here
    y, y2, _ = outs["counted waits"]
    ya, y2a = ops.pw_conv_pair(x, p1, b1, kw["in_sums"], kw["in_gamma"], kw["in_beta"], slope, res, p2, b2, Cmid, Cout2)
    assert torch.equal(ya, y) and torch.equal(y2a, y2)


@pytest.mark.parametrize("Bt,Cin,Cout,L", [(1, 256, 512, 3200), (1, 512, 256, 3200), (1, 256, 1024, 1600), (2, 128, 200, 708),
                                           (1, 512, 512, 1600)])
@pytest.mark.parametrize("pro", [0, 1, 2, 3])
@pytest.mark.parametrize("epi", ["sums", "residual", "mask"])
def test_pw_conv_narrow_tiles_for_small_launches(Bt, Cin, Cout, L, pro, epi):
    """Launches that cannot fill the chip with 128 x 128 tiles (a batch-1 forward: README.md:100-106, SURVEY.md §8 cfg 1) run
    the 64 x 64-tile kernel (srf_pwconv_w4.hip): the profiler proves the dispatch, the result is checked against an fp64
    reference and is BITWISE the 128 x 128 kernel's (debug flag 2048 = the one-tile-per-block 128 x 128 kernel): same splits, same
    summation order.  Ragged edges: Cout = 200 (rows beyond Cout), L = 708 (columns beyond L)."""
    from sudo_rm_rf_amd import ops
    ops.set_kernel_mode(0)
    x = dev32(rnd(Bt, Cin, L, seed=50, scale=1.3, shift=0.2))
    w, bias = dev32(rnd(Cout, Cin, 1, seed=51, scale=Cin ** -0.5)), dev32(rnd(Cout, seed=52, scale=0.2))
    kw, xin = {}, x.double().cpu()
    if pro in (1, 2):
        gamma, beta = rnd(Cin, seed=54, scale=0.3, shift=1.0), rnd(Cin, seed=55, scale=0.3)
        kw.update(in_sums=sums64(xin).to(DEV), in_gamma=dev32(gamma), in_beta=dev32(beta))
        xin = gln64(xin, gamma, beta)
    if pro in (2, 3):
        kw.update(in_prelu=dev32(torch.tensor([0.17], dtype=torch.float64)))
        xin = torch.where(xin >= 0, xin, 0.17 * xin)
    want = F.conv1d(xin, w.double().cpu(), bias.double().cpu())
    if epi == "residual":
        res = dev32(rnd(Bt, Cout, L, seed=53))
        kw.update(residual=res)
        want = want + res.double().cpu()
    elif epi == "mask":
        mc = 8 if Cout % 8 == 0 else Cout
        mul = dev32(rnd(Bt, mc, L, seed=56))
        kw.update(mask_mul=mul)
        want = torch.relu(want) * mul.double().cpu().repeat(1, Cout // mc, 1)
    got_sums = ops.new_sums(Bt, DEV) if epi == "sums" else None
    with ops.kernel_trace(DEV) as tr:
        got = ops.pw_conv(x, w, bias, out_sums=got_sums, **kw)
    assert tr.names == {"pw_conv_bf16x3_w4"}, tr.names
    with ops.debug_flags(DebugFlag.GEMM_128_ONE_TILE_PER_BLOCK):
        with ops.kernel_trace(DEV) as tr:
            ref = ops.pw_conv(x, w, bias, out_sums=ops.new_sums(Bt, DEV) if epi == "sums" else None, **kw)
        assert "pw_conv_bf16x3_w4" not in tr.names, tr.names
    if epi == "sums":
        tot = got_sums.double().sum(dim=1).cpu()              # [Bt][buckets][2] -> per-example {sum, sumsq}
        exp = torch.stack([want.sum(dim=(1, 2)), (want * want).sum(dim=(1, 2))], dim=1)
        assert torch.allclose(tot, exp, rtol=1e-5, atol=1e-6 * want[0].numel()), (tot, exp)   # (fp32 partial sums per thread)
    check(got, want, 1e-4, "narrow-tile pw_conv pro=%d epi=%s" % (pro, epi))
    assert torch.equal(got, ref)


@pytest.mark.parametrize("Bt,Cin,Cout,L", [(16, 256, 512, 3200), (16, 512, 256, 3200), (8, 512, 1024, 3200), (3, 2048, 512, 12800),
                                           (12, 512, 512, 1632)])
@pytest.mark.parametrize("pro", [0, 1, 2, 3])
@pytest.mark.parametrize("parts", ["fp16x2", "bf16x3"])
def test_pw_conv_three_part_split(Bt, Cin, Cout, L, pro, parts):
    """The training forward's GEMM (srf_pw_conv_packed3) in both of its forms -- two fp16 parts per operand, three MFMAs per
    product block (round 4, the default) and three bf16 parts, six MFMAs (round 3, debug flag 16384): the profiler proves the
    256 x 128 kernel of that form served the launch; against an fp64 reference its error must be in the exact-fp32 MFMA kernel's
    class (kernel mode 2 on the same inputs), far below the two-part bf16 kernel's; statistics epilogue checked for the forms
    that have one.  Forms as the training forward uses them: pro 2 with the residual, the others without."""
    from sudo_rm_rf_amd import ops
    ops.set_kernel_mode(0)
    ops.set_debug_flags(DebugFlag.TRAIN_BF16X3 if parts == "bf16x3" else 0)
    g = torch.Generator(device=DEV).manual_seed(700 + Cin + Cout + L + pro)
    x = torch.randn(Bt, Cin, L, generator=g, device=DEV) * 1.3 + 0.2
    w = torch.randn(Cout, Cin, 1, generator=g, device=DEV) * Cin ** -0.5
    bias = torch.randn(Cout, generator=g, device=DEV) * 0.2
    kw, xin = {}, x.double()
    if pro in (1, 2):
        gamma = (torch.randn(Cin, generator=g, device=DEV) * 0.3 + 1.0)
        beta = torch.randn(Cin, generator=g, device=DEV) * 0.3
        sums = ops.new_sums(Bt, DEV)
        sums[:, 0, 0] = xin.sum(dim=(1, 2))
        sums[:, 0, 1] = (xin * xin).sum(dim=(1, 2))
        kw.update(in_sums=sums, in_gamma=gamma, in_beta=beta)
        mean = xin.mean(dim=(1, 2), keepdim=True)
        var = (xin * xin).mean(dim=(1, 2), keepdim=True) - mean * mean
        xin = gamma.double().view(1, -1, 1) * (xin - mean) / torch.sqrt(var + 1e-8) + beta.double().view(1, -1, 1)
    if pro in (2, 3):
        kw.update(in_prelu=torch.tensor([0.17], device=DEV))
        xin = torch.where(xin >= 0, xin, 0.17 * xin)
    res = None
    if pro == 2:
        res = torch.randn(Bt, Cout, L, generator=g, device=DEV)
        kw.update(residual=res)
    cols = torch.randperm(L, generator=torch.Generator().manual_seed(L + pro))[:192].sort().values.to(DEV)
    want = torch.einsum("mk,bkl->bml", w[:, :, 0].double(), xin[:, :, cols]) + bias.double().view(1, -1, 1)
    if res is not None:
        want = want + res.double()[:, :, cols]
    packed3 = ops.pack3_pw_weight(w)
    assert packed3 is not None
    osums = ops.new_sums(Bt, DEV) if pro == 0 else None
    with ops.kernel_trace(DEV) as tr:
        got = ops.pw_conv3(x, w, bias, packed3, out_sums=osums, **kw)
    assert tr.names == {"pw_conv_x3w%d<%d>" % (3 if parts == "bf16x3" else 4, pro)}, tr.names
    ops.set_debug_flags(0)
    try:
        ops.set_kernel_mode(2)
        exact = ops.pw_conv(x, w, bias, **kw)
    finally:
        ops.set_kernel_mode(0)
    two = ops.pw_conv(x, w, bias, packed=ops.pack_pw_weight(w), **kw)
    e3 = float((got[:, :, cols].double() - want).abs().max())
    ex = float((exact[:, :, cols].double() - want).abs().max())
    e2 = float((two[:, :, cols].double() - want).abs().max())
    print(f"three-part {e3:.2e}  exact fp32 MFMA {ex:.2e}  two-part {e2:.2e}  (|y| max {float(want.abs().max()):.1f})")
    assert e3 <= 2.0 * ex + 1e-7 and e3 <= 0.6 * e2      # (the floor both share is the fp32 accumulation over K)
    assert float((got - exact).abs().max()) <= 4.0 * ex + 1e-6            # whole tensor against the exact kernel
    if osums is not None:
        tot = osums.sum(dim=1).cpu()
        ref = torch.stack([got.double().sum(dim=(1, 2)), (got.double() ** 2).sum(dim=(1, 2))], dim=1).cpu()
        assert torch.allclose(tot, ref, rtol=1e-5, atol=1e-6 * got[0].numel())


def _fp16_split_emulation(w, x, cols):
    """The two-part arithmetic itself, in numpy on the kernel's own operands: hi = fp16(v), lo = fp16(v - hi) (round to nearest
    even, subnormals kept), the weights times 2^4 first, the three products hi hi + lo hi + hi lo accumulated in fp32, times 2^-4.
    w [Cout, Cin], x [Bt, Cin, L] float32 numpy; returns [Bt, Cout, len(cols)] float32."""
    def split(v):
        hi = v.astype(np.float16)
        return hi.astype(np.float32), (v - hi.astype(np.float32)).astype(np.float16).astype(np.float32)
    wh, wl = split(w * np.float32(16.0))
    xh, xl = split(np.ascontiguousarray(x[:, :, cols]))
    y = np.einsum("mk,bkl->bml", wh, xh) + np.einsum("mk,bkl->bml", wl, xh) + np.einsum("mk,bkl->bml", wh, xl)
    return (y * np.float32(1.0 / 16.0)).astype(np.float32)


@pytest.mark.parametrize("scale", [1e-2, 1.0, 30.0, 1e3, 1e-3, 1e-4, 1e-5, 1e-6])
def test_pw_conv_fp16_split_accuracy_over_magnitudes(scale):
    """The training forward's default GEMM (two fp16 parts per operand) against fp64 over five decades of operand magnitude:
    the error relative to the output's scale stays in the exact-fp32 class (a per-example GlobLN downstream makes relative error
    the quantity that matters).
    Below 1e-2 the lo parts, then the hi parts, fall into fp16's subnormal range and the form loses bits by construction (the
    range contract in csrc/srf_pwconv.hip): there the kernel is held to 2 x what the two-part arithmetic itself gives on the
    same operands (a numpy emulation of the split, not the kernel's output), and the three-bf16-part form (DebugFlag.TRAIN_BF16X3),
    which has fp32's exponent range, to the 2e-6 of the upper decades -- at every scale."""
    from tests import edge_signals as es
    from sudo_rm_rf_amd import ops
    ops.set_kernel_mode(0)
    Bt, Cin, Cout, L = 16, 256, 256, 3200          # 400 tiles: served by the 256 x 128 kernel (asserted below)
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn(Bt, Cin, L, generator=g, device=DEV) * scale
    w = torch.randn(Cout, Cin, 1, generator=g, device=DEV) * Cin ** -0.5
    bias = torch.zeros(Cout, device=DEV)
    want = torch.einsum("mk,bkl->bml", w[:, :, 0].double(), x.double())
    packed = ops.pack3_pw_weight(w)
    with ops.kernel_trace(DEV) as tr:
        got = ops.pw_conv3(x, w, bias, packed)
    assert tr.names == {"pw_conv_x3w4<0>"}, tr.names
    rel = float((got.double() - want).abs().max()) / float(want.abs().max())
    with ops.debug_flags(DebugFlag.TRAIN_BF16X3):
        packed3 = ops.pack3_pw_weight(w)
        with ops.kernel_trace(DEV) as tr3:
            got3 = ops.pw_conv3(x, w, bias, packed3)
    assert tr3.names == {"pw_conv_x3w3<0>"}, tr3.names
    rel3 = float((got3.double() - want).abs().max()) / float(want.abs().max())
    line = "operand scale %g: two fp16 parts %.3e, three bf16 parts %.3e (relative to max|y| = %.3e)" % (
        scale, rel, rel3, float(want.abs().max()))
    if scale >= 1e-2:
        print(line)
        assert rel <= 2e-6, (scale, rel)
    else:
        cols = np.arange(0, L, 17)
        emu = _fp16_split_emulation(w[:, :, 0].cpu().numpy(), x.cpu().numpy(), cols)
        wc = want[:, :, cols].cpu().numpy()
        emu_rel = float(np.abs(emu.astype(np.float64) - wc).max()) / float(np.abs(wc).max())
        rel_c = float((got[:, :, cols].double() - want[:, :, cols]).abs().max()) / float(np.abs(wc).max())
        line += "; on every 17th column: kernel %.3e, the split's own arithmetic %.3e, bar %.3e" % (rel_c, emu_rel, 2 * emu_rel)
        print(line)
        es.write_profile_lines("fp16_split_%g" % scale, [line])
        assert torch.isfinite(got).all() and rel_c <= 2.0 * emu_rel, line
    assert rel3 <= 2e-6, (scale, rel3)


def test_pw_conv_fp16_split_is_loud_beyond_its_range():
    """Range contract of the two-fp16-part GEMM (round 5): operands beyond fp16's range and NaN / inf operands make
    the affected outputs NON-FINITE -- as the fp32 reference's own overflow / NaN would -- instead of being clamped to a
    plausible wrong number (rounds 3-4); every other column stays exact; debug flag 16384 (three bf16 parts: fp32's exponent
    range) computes the large finite case exactly."""
    from sudo_rm_rf_amd import ops
    ops.set_kernel_mode(0)
    Bt, Cin, Cout, L = 16, 256, 256, 3200
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn(Bt, Cin, L, generator=g, device=DEV)
    x[0, 5, 17] = 3.0e5                      # beyond fp16
    x[1, 9, 100] = float("nan")
    x[2, 0, 7] = float("inf")
    w = torch.randn(Cout, Cin, 1, generator=g, device=DEV) * Cin ** -0.5
    bias = torch.zeros(Cout, device=DEV)
    got = ops.pw_conv3(x, w, bias, ops.pack3_pw_weight(w))
    for b, l in ((0, 17), (1, 100), (2, 7)):
        assert not torch.isfinite(got[b, :, l]).any(), (b, l)          # the whole output column of a poisoned operand column
    mask = torch.ones(Bt, L, dtype=torch.bool, device=DEV)
    mask[0, 17] = mask[1, 100] = mask[2, 7] = False
    xc = torch.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0).double()
    want = torch.einsum("mk,bkl->bml", w[:, :, 0].double(), xc)
    sel = mask[:, None, :].expand_as(got)
    assert torch.isfinite(got[sel]).all()
    assert float((got.double() - want)[sel].abs().max()) <= 1e-5 * float(want[sel].abs().max())
    x2 = torch.randn(Bt, Cin, L, generator=g, device=DEV)
    x2[0, 5, 17] = 3.0e5
    with ops.debug_flags(DebugFlag.TRAIN_BF16X3):
        exact = ops.pw_conv3(x2, w, bias, ops.pack3_pw_weight(w))
    want2 = torch.einsum("mk,bkl->bml", w[:, :, 0].double(), x2.double())
    assert float((exact.double() - want2).abs().max()) <= 1e-5 * float(want2.abs().max())


@pytest.mark.parametrize("Bt,Cin1,Cout2,L", [(32, 512, 512, 3200), (12, 512, 512, 3200), (24, 256, 384, 1604)])
@pytest.mark.parametrize("pro", [1, 2])
def test_pw_conv_pair_fp16_parts_is_bitwise_the_two_training_launches(Bt, Cin1, Cout2, L, pro):
    """srf_pw_conv_pair_packed3 (round 5: the training forward's fused pair, operands on two fp16 parts) against the two
    srf_pw_conv_packed3 launches it replaces: both output tensors BIT FOR BIT, the statistics to rounding, and against fp64 at
    the exact-fp32 class."""
    from sudo_rm_rf_amd import ops
    ops.set_kernel_mode(0)
    Cmid = 256
    if not ops.pw_conv_pair3_supported(Bt, Cin1, Cmid, Cout2, L):
        pytest.skip("shape not served on this device")
    x = dev32(rnd(Bt, Cin1, L, seed=150, scale=1.3, shift=0.2))
    w1, b1 = dev32(rnd(Cmid, Cin1, 1, seed=151, scale=Cin1 ** -0.5)), dev32(rnd(Cmid, seed=152, scale=0.2))
    w2, b2 = dev32(rnd(Cout2, Cmid, 1, seed=153, scale=Cmid ** -0.5)), dev32(rnd(Cout2, seed=154, scale=0.2))
    res = dev32(rnd(Bt, Cmid, L, seed=155)) if pro == 2 else None
    gamma, beta = rnd(Cin1, seed=156, scale=0.3, shift=1.0), rnd(Cin1, seed=157, scale=0.3)
    xin = x.double().cpu()
    kw = dict(in_sums=sums64(xin).to(DEV), in_gamma=dev32(gamma), in_beta=dev32(beta))
    xin = gln64(xin, gamma, beta)
    slope = None
    if pro == 2:
        slope = dev32(torch.tensor([0.17], dtype=torch.float64))
        kw.update(in_prelu=slope)
        xin = torch.where(xin >= 0, xin, 0.17 * xin)
    want1 = F.conv1d(xin, w1.double().cpu(), b1.double().cpu())
    if res is not None:
        want1 = want1 + res.double().cpu()
    p1, p2 = ops.pack3_pw_weight(w1), ops.pack3_pw_weight(w2)
    with ops.kernel_trace(DEV) as tr:
        y_ref = ops.pw_conv3(x, w1, b1, p1, residual=res, **kw)
        sums_ref = ops.new_sums(Bt, DEV)
        y2_ref = ops.pw_conv3(y_ref, w2, b2, p2, out_sums=sums_ref)
    assert tr.names == {"pw_conv_x3w4<%d>" % pro, "pw_conv_x3w4<0>"}, tr.names
    sums = ops.new_sums(Bt, DEV)
    with ops.kernel_trace(DEV) as tr:
        y, y2 = ops.pw_conv_pair3(x, p1, b1, kw["in_sums"], kw["in_gamma"], kw["in_beta"], slope, res, p2, b2, Cmid, Cout2, out_sums2=sums)
    assert tr.names == {"pw_pair_x3f4<%d>" % pro}, tr.names
    assert torch.equal(y, y_ref), "y: %d values differ" % int((y != y_ref).sum())
    assert torch.equal(y2, y2_ref), "y2: %d values differ" % int((y2 != y2_ref).sum())
    want2 = F.conv1d(y_ref.double().cpu(), w2.double().cpu(), b2.double().cpu())
    check(y, want1, 2e-5, "fp16 pair: y")
    check(y2, want2, 2e-5, "fp16 pair: y2")
    check_sums(sums, y2.double().cpu(), "fp16 pair: statistics of y2")


def test_pw_conv_packed3_refuses_an_image_of_the_other_format():
    """The packed3 image's format (two fp16 parts | three bf16 parts) is fixed when it is packed; a launch under the other
    setting of debug flag 16384 must fail with an error instead of reinterpreting the bits."""
    from sudo_rm_rf_amd import ops
    ops.set_kernel_mode(0)
    Bt, Cin, Cout, L = 16, 256, 256, 3200
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(Bt, Cin, L, generator=g, device=DEV)
    w = torch.randn(Cout, Cin, 1, generator=g, device=DEV) * Cin ** -0.5
    bias = torch.zeros(Cout, device=DEV)
    packed = ops.pack3_pw_weight(w)                       # fp16 parts
    ref = ops.pw_conv3(x, w, bias, packed)
    with ops.debug_flags(DebugFlag.TRAIN_BF16X3):
        with pytest.raises(RuntimeError, match="packed as two fp16 parts"):
            ops.pw_conv3(x, w, bias, packed)
        packed3 = ops.pack3_pw_weight(w)                  # re-packed under the flag: served
        again = ops.pw_conv3(x, w, bias, packed3)
    assert float((again - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    with pytest.raises(RuntimeError, match="packed as three bf16 parts"):
        ops.pw_conv3(x, w, bias, packed3)


# (Bt, Cin, Cout, L, prologue, epilogue): the GEMMs of BASELINE cfg 4 / cfg 5 AT BENCH BATCH that no golden reaches
# (VERDICT r2 weak 1): bottleneck K = 2048 / 4096 (64 / 128 k-tiles), proj_1x1 / res_conv at 512 -> 512 (two M tiles,
# statistics epilogue / residual epilogue), cfg 5's mask GEMM (Cout = S N = 8192: 32 M tiles, ReLU x encoder epilogue)
X3W_MODEL_SHAPES = [(16, 2048, 512, 3200, 1, "sums"), (8, 4096, 512, 12800, 1, "sums"), (16, 512, 512, 3200, 0, "sums"),
                    (16, 512, 512, 3200, 2, "residual"), (4, 512, 8192, 3200, 3, "mask")]


@pytest.mark.parametrize("Bt,Cin,Cout,L,pro,epi", X3W_MODEL_SHAPES,
                         ids=["cfg4-bottleneck", "cfg5-bottleneck", "cfg4-proj", "cfg4-res_conv", "cfg5-mask"])
def test_pw_conv_x3w_at_cfg4_cfg5_shapes(Bt, Cin, Cout, L, pro, epi):
    """The 256 x 128 split-bf16 GEMM at the shapes bench.py times for BASELINE cfg 4 / 5: (a) the in-library profiler proves
    that kernel family served the launch, (b) 160 sampled time columns of every example match an fp64 reference of the same
    op (torch fp64 on the GPU: the full fp64 product is 0.4 TFLOP for the largest shape), (c) the FULL output tensor is
    bitwise equal to the 128 x 128 kernels (same splits, same summation order), which the small-shape tests pin to fp64
    element by element, (d) the statistics epilogue's sums match the fp64 sums of the output it wrote."""
    from sudo_rm_rf_amd import ops
    ops.set_kernel_mode(0)
    g = torch.Generator(device=DEV).manual_seed(1000 + Cin + Cout + L + pro)
    x = torch.randn(Bt, Cin, L, generator=g, device=DEV) * 1.3 + 0.2
    x *= 1.0 + 0.5 * torch.arange(Bt, device=DEV, dtype=torch.float32).view(Bt, 1, 1) / Bt    # per-example statistics differ
    w = torch.randn(Cout, Cin, 1, generator=g, device=DEV) * Cin ** -0.5
    bias = torch.randn(Cout, generator=g, device=DEV) * 0.2
    kw = {}
    cols = torch.randperm(L, generator=torch.Generator().manual_seed(L + pro))[:160].sort().values.to(DEV)
    cols[0], cols[-1] = 0, L - 1                                   # (first / last column of the first / last tile)
    xs = x[:, :, cols].double()
    if pro in (1, 2):
        gamma = torch.rand(Cin, generator=g, device=DEV) * 0.6 + 0.7
        beta = torch.randn(Cin, generator=g, device=DEV) * 0.3
        kw.update(in_sums=ops.gln_stats(x, Bt), in_gamma=gamma, in_beta=beta)
        xd = x.double()
        mu = xd.mean(dim=(1, 2), keepdim=True)
        var = (xd * xd).mean(dim=(1, 2), keepdim=True) - mu * mu
        del xd
        xs = gamma.double().view(1, -1, 1) * (xs - mu) / (var + 1e-8).sqrt() + beta.double().view(1, -1, 1)
    if pro in (2, 3):
        kw.update(in_prelu=torch.tensor([0.17], device=DEV))
        xs = torch.where(xs >= 0, xs, 0.17 * xs)
    want = torch.einsum("oc,bcl->bol", w[:, :, 0].double(), xs) + bias.double().view(1, -1, 1)
    sums = None
    if epi == "residual":
        res = torch.randn(Bt, Cout, L, generator=g, device=DEV)
        kw.update(residual=res)
        want = want + res[:, :, cols].double()
    elif epi == "mask":
        enc = torch.randn(Bt, Cout // 2, L, generator=g, device=DEV)       # S = 2 sources share the encoder output
        kw.update(mask_mul=enc)
        want = torch.relu(want) * enc[:, :, cols].double().repeat(1, 2, 1)
    else:
        sums = ops.new_sums(Bt, DEV)
        kw.update(out_sums=sums)
    packed = ops.pack_pw_weight(w)
    assert packed is not None
    with ops.kernel_trace(DEV) as tr:
        got = ops.pw_conv(x, w, bias, packed=packed, **kw)
    assert tr.names == {"pw_conv_x3w<%d>" % pro}, tr.names
    err = (got[:, :, cols].double() - want).abs().max().item()
    scale = want.abs().max().item()
    print("x3w %s pro %d: max abs err %.3e on sampled columns (|want| max %.2f)" % ((Bt, Cin, Cout, L), pro, err, scale))
    assert err <= 1e-4 * max(1.0, scale / 8), err        # split-bf16 products carry ~2^-17 relative error (un-normalised operands)
    if sums is not None:
        gd = got.double().reshape(Bt, -1)
        tot = sums.sum(1)
        assert ((tot[:, 0] - gd.sum(1)).abs() <= 4e-6 * gd.abs().sum(1) + 1e-9).all()
        assert ((tot[:, 1] - (gd * gd).sum(1)).abs() <= 4e-6 * (gd * gd).sum(1) + 1e-9).all()
        del gd
        kw["out_sums"] = ops.new_sums(Bt, DEV)
    if epi != "mask":
        # (round 4) the PAIRED-BLOCK form of the kernel -- what srf_forward runs for every form but the mask epilogue; stand-alone
        # calls get it with debug flag 8192 -- is bit-identical and its statistics agree to rounding
        with ops.debug_flags(DebugFlag.GEMM_256_SWAP_FORMS), ops.kernel_trace(DEV) as tr1:
            one = ops.pw_conv(x, w, bias, packed=packed, **kw)
        assert tr1.names == {"pw_conv_x3p<%d>" % pro}, tr1.names
        assert torch.equal(got, one)
        if sums is not None:
            assert torch.allclose(kw["out_sums"].sum(1), sums.sum(1), rtol=1e-6, atol=1e-6 * got[0].numel())
            kw["out_sums"] = ops.new_sums(Bt, DEV)
        del one
    with ops.debug_flags(DebugFlag.NO_GEMM_256), ops.kernel_trace(DEV) as tr2:
        ref = ops.pw_conv(x, w, bias, packed=packed, **kw)
    assert not any(n.startswith(("pw_conv_x3w", "pw_conv_x3p")) for n in tr2.names), tr2.names
    assert torch.equal(got, ref)


def test_pw_conv_beyond_2gb_is_chunked_over_examples():
    """An activation tensor beyond the 256 x 128 kernel's 32-bit buffer reach (cfg 5's bottleneck: 3.4 GB) goes out as
    several launches over runs of whole examples: same outputs and same per-example statistics as the 64-bit pointer
    kernels, including the input-norm prologue whose statistic slots move with the run."""
    from sudo_rm_rf_amd import ops
    ops.set_kernel_mode(0)
    Bt, Cin, Cout, L = 3, 512, 256, 358400                      # 2.2 GB of activations, 0.73 GB per example
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(Bt, Cin, L, generator=g, device=DEV) * 1.2 + 0.1
    x[1] *= 3.0          # per-example statistics must not be mixed up (the prologue normalises with them: outputs would differ)
    w = torch.randn(Cout, Cin, 1, generator=g, device=DEV) * Cin ** -0.5
    bias = torch.randn(Cout, generator=g, device=DEV) * 0.2
    res = torch.randn(Bt, Cout, L, generator=g, device=DEV)
    kw = dict(in_sums=ops.gln_stats(x, Bt), in_gamma=torch.rand(Cin, generator=g, device=DEV) + 0.5,
              in_beta=torch.randn(Cin, generator=g, device=DEV) * 0.3, in_prelu=torch.tensor([0.2], device=DEV), residual=res)
    packed = ops.pack_pw_weight(w)
    s_a, s_b = ops.new_sums(Bt, DEV), ops.new_sums(Bt, DEV)
    got = ops.pw_conv(x, w, bias, packed=packed, out_sums=s_a, **kw)
    with ops.debug_flags(DebugFlag.NO_GEMM_256):                 # 64-bit pointer form
        want = ops.pw_conv(x, w, bias, packed=packed, out_sums=s_b, **kw)
    assert torch.equal(got, want)
    ta, tb = s_a.sum(1), s_b.sum(1)                              # [example][{sum, sumsq}]
    assert ((ta - tb).abs() <= 1e-7 * tb.abs().clamp_min(1.0)).all()      # (fp32 partial sums in a different order)


def test_pw_conv_mask_epilogue(mode):
    from sudo_rm_rf_amd import ops
    Bt, Cin, N, S, L = 2, 64, 48, 2, 260
    x, w, bias = rnd(Bt, Cin, L, seed=20), rnd(S * N, Cin, 1, seed=21, scale=0.2), rnd(S * N, seed=22)
    enc = rnd(Bt, N, L, seed=23)
    slope = torch.tensor([0.3], dtype=torch.float64)
    m = F.conv1d(torch.where(x >= 0, x, slope * x), w, bias)
    want = (torch.relu(m.view(Bt, S, N, L)) * enc.unsqueeze(1)).view(Bt, S * N, L)
    got = ops.pw_conv(dev32(x), dev32(w), dev32(bias), in_prelu=dev32(slope), mask_mul=dev32(enc))
    # un-normalised N(0,1) operands times |enc| up to 4: split-bf16 products carry ~2^-17 relative error
    check(got, want, 2e-4 if mode == 0 else 2e-5, "mask epilogue")


def test_pw_conv_transpose_detecting(mode):
    """A = I-like weights with an ASYMMETRIC operand catch row/col swaps in the MFMA C layout."""
    from sudo_rm_rf_amd import ops
    Bt, C, L = 1, 128, 256
    x = (torch.arange(C, dtype=torch.float64)[:, None] * 1000 + torch.arange(L, dtype=torch.float64)[None, :])
    x = (x / 1e5).unsqueeze(0)          # <= 1.28: a row/col swap moves entries by >= 1e-2
    w = torch.zeros(C, C, 1, dtype=torch.float64)
    w[torch.arange(C), (torch.arange(C) * 7 + 3) % C, 0] = 1.0     # permutation matrix
    got = ops.pw_conv(dev32(x), dev32(w), dev32(torch.zeros(C, dtype=torch.float64)))
    check(got, F.conv1d(x, w), 1e-4, "permutation GEMM")


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Bt,C,Lin,stride", [(2, 64, 3200, 1), (2, 64, 3200, 2), (3, 20, 200, 2),
                                             (2, 7, 404, 2), (2, 7, 202, 1), (1, 5, 50, 2),
                                             (2, 32, 256, 1), (2, 32, 512, 2), (1, 3, 4, 1), (1, 3, 8, 2),
                                             (1, 3, 6, 2)])
@pytest.mark.parametrize("pro", [0, 1, 2])
def test_dwconv5(mode, Bt, C, Lin, stride, pro):
    from sudo_rm_rf_amd import ops
    x = rnd(Bt, C, Lin, seed=30, scale=1.3, shift=-0.4)
    w, bias = rnd(C, 1, 5, seed=31, scale=0.5), rnd(C, seed=32, scale=0.2)
    gamma, beta = rnd(C, seed=33, scale=0.3, shift=1.0), rnd(C, seed=34, scale=0.3)
    slope = torch.tensor([0.21], dtype=torch.float64)
    xin, kw = x, {}
    if pro >= 1:
        xin = gln64(x, gamma, beta)
        kw.update(in_sums=sums64(x).to(DEV), in_gamma=dev32(gamma), in_beta=dev32(beta))
    if pro == 2:
        xin = torch.where(xin >= 0, xin, slope * xin)
        kw.update(in_prelu=dev32(slope))
    want = F.conv1d(xin, w, bias, stride=stride, padding=2, groups=C)
    osums = ops.new_sums(Bt, DEV)
    got = ops.dwconv5(dev32(x), dev32(w), dev32(bias), stride, out_sums=osums, **kw)
    check(got, want, 2e-5, "dwconv5")
    check_sums(osums, want, "dwconv5 sums")


@pytest.mark.parametrize("Bt,C,L,D", [(2, 64, 3200, 5), (2, 16, 6400, 6), (2, 5, 808, 3), (1, 3, 36, 3),
                                      (2, 4, 64, 1), (1, 3, 6, 2), (1, 2, 256, 8)])
def test_merge(mode, Bt, C, L, D):
    from sudo_rm_rf_amd import ops
    levels = [rnd(Bt, C, L >> k, seed=40 + k, scale=1.0 + 0.2 * k, shift=0.1 * k) for k in range(D)]
    gam = [rnd(C, seed=50 + k, scale=0.3, shift=1.0) for k in range(D)]
    bet = [rnd(C, seed=60 + k, scale=0.3) for k in range(D)]
    normed = [gln64(levels[k], gam[k], bet[k]) for k in range(D)]
    u = normed[-1]
    for k in range(D - 2, -1, -1):
        u = normed[k] + u.repeat_interleave(2, dim=-1)
    osums = ops.new_sums(Bt, DEV)
    got = ops.merge([dev32(t) for t in levels], [sums64(t).to(DEV) for t in levels],
                    [dev32(t) for t in gam], [dev32(t) for t in bet], out_sums=osums)
    check(got, u, 3e-5, "merge")
    check_sums(osums, u, "merge sums")


@pytest.mark.parametrize("flags", [0, DebugFlag.PYR_NO_REG, DebugFlag.PYR_NO_REG | DebugFlag.PYR_NO_LDS_TILES],
                         ids=["registers", "lds-tiles", "lds-rows"])
@pytest.mark.parametrize("Bt,C,L,D", [(2, 64, 3200, 5), (2, 16, 6400, 6), (1, 8, 128, 4), (3, 20, 256, 2),
                                      (2, 4, 64, 1), (1, 5, 12800, 6), (2, 3, 64, 3), (2, 6, 3232, 5),
                                      (1, 3, 3264, 6)])
def test_fused_pyramid(Bt, C, L, D, flags):
    """srf_pyramid (two passes, statistics through the linearity of conv o GlobLN) == the reference's
    chain DilatedConvNorm x D + upsample/add (improved_sudormrf.py:206-216)."""
    from sudo_rm_rf_amd import ops
    y1 = rnd(Bt, C, L, seed=100, scale=1.4, shift=0.2)
    g_in, b_in = rnd(C, seed=101, scale=0.3, shift=1.0), rnd(C, seed=102, scale=0.3)
    slope = torch.tensor([0.23], dtype=torch.float64)
    W = [rnd(C, 1, 5, seed=110 + k, scale=0.5) for k in range(D)]
    Bi = [rnd(C, seed=120 + k, scale=0.2) for k in range(D)]
    Ga = [rnd(C, seed=130 + k, scale=0.3, shift=1.0) for k in range(D)]
    Be = [rnd(C, seed=140 + k, scale=0.3) for k in range(D)]
    cur = gln64(y1, g_in, b_in)
    cur = torch.where(cur >= 0, cur, slope * cur)
    outs = []
    for k in range(D):
        d = F.conv1d(cur, W[k], Bi[k], stride=1 if k == 0 else 2, padding=2, groups=C)
        cur = gln64(d, Ga[k], Be[k])
        outs.append(cur)
    u = outs[-1]
    for k in range(D - 2, -1, -1):
        u = outs[k] + u.repeat_interleave(2, dim=-1)
    osums = ops.new_sums(Bt, DEV)
    from sudo_rm_rf_amd import _lib
    with ops.debug_flags(flags):
        if not _lib.load().srf_pyramid_supported(C, L, D):
            pytest.skip("shape not supported by this kernel family")
        got = _run_pyramid(ops, y1, g_in, b_in, slope, W, Bi, Ga, Be, osums)
    check(got, u, 5e-5, "fused pyramid")
    check_sums(osums, u, "fused pyramid sums")


def _run_pyramid(ops, y1, g_in, b_in, slope, W, Bi, Ga, Be, osums):
    return ops.pyramid(dev32(y1), sums64(y1).to(DEV), dev32(g_in), dev32(b_in), dev32(slope),
                      [dev32(t) for t in W], [dev32(t) for t in Bi], [dev32(t) for t in Ga],
                      [dev32(t) for t in Be], out_sums=osums)


@pytest.mark.parametrize("Bt,Ci,Co,K,L,T", [(2, 64, 2, 21, 100, 1000), (1, 96, 2, 21, 64, 633),
                                            (2, 32, 4, 11, 40, 200), (1, 1024, 2, 21, 320, 3200)])
def test_decoder(mode, Bt, Ci, Co, K, L, T):
    from sudo_rm_rf_amd import ops
    h = K // 2
    v, w = rnd(Bt, Ci, L, seed=70), rnd(Ci, Co, K, seed=71, scale=Ci ** -0.5)
    want = F.conv_transpose1d(v, w, None, stride=h, padding=h, output_padding=h - 1)[..., :T]
    got = ops.decoder(dev32(v), dev32(w), T)
    check(got, want, 3e-5, "decoder")


@pytest.mark.parametrize("flags", [0, DebugFlag.TAC_LANES_4TILES, DebugFlag.TAC_GENERIC], ids=["lanes", "lanes-4tiles", "columns"])
@pytest.mark.parametrize("Bt,G,n,L", [(2, 16, 16, 300), (1, 4, 8, 77), (2, 8, 4, 130), (1, 2, 32, 64),
                                      (3, 16, 16, 1601), (2, 4, 4, 100), (2, 2, 2, 70), (1, 8, 16, 50),
                                      (2, 16, 8, 64), (1, 16, 2, 33), (1, 3, 4, 40)])
def test_tac(Bt, G, n, L, flags):
    from sudo_rm_rf_amd import ops
    with ops.debug_flags(flags):
        _tac_case(Bt, G, n, L)


def test_tac_mfma_forms_serve_the_cfg3_shape_and_agree_with_the_valu_kernels():
    """n = 16, G = 16 (BASELINE's GroupComm shape) runs on the matrix pipe -- the in-library profiler proves which kernel served
    the call, forward and backward -- and agrees with the VALU kernels (debug flag 1 << 22) far inside test_tac's bar: two
    independent implementations of groupcomm_sudormrf_v2.py:356-377."""
    from sudo_rm_rf_amd import ops
    ops.set_kernel_mode(0)
    Bt, G, n, L = 3, 16, 16, 1000
    H = 3 * n
    x = dev32(rnd(Bt, G, n, L, seed=180, scale=2.0))
    go = dev32(rnd(Bt, G, n, L, seed=189, scale=1e-4))           # (gradient-sized: far below fp16's normal range)
    P = [dev32(t) for t in (rnd(H, n, seed=181, scale=n ** -0.5), rnd(H, seed=182, scale=0.2),
                            torch.tensor([0.2], dtype=torch.float64), rnd(H, H, seed=183, scale=H ** -0.5),
                            rnd(H, seed=184, scale=0.2), torch.tensor([0.3], dtype=torch.float64),
                            rnd(n, 2 * H, seed=185, scale=(2 * H) ** -0.5), rnd(n, seed=186, scale=0.2),
                            torch.tensor([0.15], dtype=torch.float64))]
    with ops.kernel_trace(DEV) as tr:
        q = ops.tac(x, P)
        gx, grads = ops.tac_bwd(x, go, P)
    assert {"tac_mfma", "tac_bwd_mfma"} <= tr.names, tr.names
    with ops.debug_flags(DebugFlag.TAC_VALU), ops.kernel_trace(DEV) as tr2:
        q2 = ops.tac(x, P)
        gx2, grads2 = ops.tac_bwd(x, go, P)
    assert {"tac", "tac_bwd"} <= tr2.names and not (tr2.names & {"tac_mfma", "tac_bwd_mfma"}), tr2.names
    assert float((q - q2).abs().max()) <= 5e-6 * max(1.0, float(q2.abs().max()))
    rel = lambda a, b: float((a - b).norm() / b.norm())
    assert rel(gx, gx2) <= 3e-5, rel(gx, gx2)
    for i, (g1, g2) in enumerate(zip(grads, grads2)):
        assert rel(g1, g2) <= 5e-5, (i, rel(g1, g2))


def _tac_case(Bt, G, n, L):
    from sudo_rm_rf_amd import ops
    H = 3 * n
    x = rnd(Bt, G, n, L, seed=80)
    P = [rnd(H, n, seed=81, scale=n ** -0.5), rnd(H, seed=82, scale=0.2), torch.tensor([0.2], dtype=torch.float64),
         rnd(H, H, seed=83, scale=H ** -0.5), rnd(H, seed=84, scale=0.2), torch.tensor([0.3], dtype=torch.float64),
         rnd(n, 2 * H, seed=85, scale=(2 * H) ** -0.5), rnd(n, seed=86, scale=0.2),
         torch.tensor([0.15], dtype=torch.float64)]
    pr = lambda t, a: torch.where(t >= 0, t, a * t)
    rows = x.permute(0, 3, 1, 2).reshape(-1, n)
    z = pr(rows @ P[0].T + P[1], P[2]).view(Bt, L, G, H)
    q = pr(z.mean(2).view(Bt * L, H) @ P[3].T + P[4], P[5])
    cat = torch.cat([z.view(Bt * L, G, H), q.unsqueeze(1).expand(Bt * L, G, H)], 2).reshape(-1, 2 * H)
    o = pr(cat @ P[6].T + P[7], P[8]).view(Bt, L, G, n).permute(0, 2, 3, 1).contiguous()
    osums = ops.new_sums(Bt * G, DEV)
    got = ops.tac(dev32(x), [dev32(p) for p in P], out_sums=osums)
    check(got, o, 2e-5, "tac")
    check_sums(osums, o.view(Bt * G, n, L), "tac sums")
    # TAC_norm + residual
    gam, bet = rnd(n, seed=87, shift=1.0, scale=0.2), rnd(n, seed=88, scale=0.2)
    want = x + gln64(o.view(Bt * G, n, L), gam, bet).view(x.shape)
    y = ops.gln_apply(got.view(Bt * G, n, L), osums, dev32(gam), dev32(bet),
                      residual=dev32(x).view(Bt * G, n, L))
    check(y.view(x.shape), want, 3e-5, "tac norm + residual")


def test_mixture_consistency():
    from sudo_rm_rf_amd import ops
    pr, mix = rnd(3, 4, 1001, seed=90), rnd(3, 1, 1001, seed=91)
    want = pr + (mix - pr.sum(1, keepdim=True)) / 4
    check(ops.mixture_consistency(dev32(pr), dev32(mix)), want, 1e-6, "mixture consistency")


def test_mixture_consistency_magsq():
    """the 'magsq' weights (mixture_consistency.py:26-28) against the numpy oracle, through the module mirror."""
    import sudo_rm_rf.dnn.experiments.utils.mixture_consistency as mixture_consistency
    from oracle import np_oracle
    for (Bt, S, T, seed) in [(3, 4, 1001, 92), (2, 2, 32000, 93), (1, 1, 7, 94)]:
        pr = rnd(Bt, S, T, seed=seed) * torch.arange(1, S + 1, dtype=torch.float64).view(1, S, 1)   # unequal energies
        mix = rnd(Bt, 1, T, seed=seed + 10)
        want = torch.from_numpy(np_oracle.mixture_consistency(pr.numpy(), mix.numpy(), "magsq"))
        got = mixture_consistency.apply(dev32(pr), dev32(mix), mix_weights_type='magsq')
        check(got, want, 2e-6 * float(want.abs().max()), "mixture consistency magsq")
    with pytest.raises(ValueError):
        mixture_consistency.apply(dev32(pr), dev32(mix), mix_weights_type='nope')
    with pytest.raises(NotImplementedError):
        mixture_consistency.apply(dev32(pr).requires_grad_(), dev32(mix), mix_weights_type='magsq')


@pytest.mark.parametrize("Bt,S,T,mc", [(3, 2, 1001, False), (2, 2, 32000, True), (1, 3, 77, True), (4, 1, 5, False)])
def test_wav_normalize_denormalize(Bt, S, T, mc):
    """README.md:100-114: (x-mean)/(std+1e-9) with torch's unbiased std, est*std+mean, mixture consistency."""
    from sudo_rm_rf_amd import ops
    x = rnd(Bt, 1, T, seed=95, scale=3.0, shift=0.7)
    std, mean = x.std(-1, keepdim=True), x.mean(-1, keepdim=True)
    want = (x - mean) / (std + 1e-9)
    got, stats = ops.wav_normalize(dev32(x))
    check(got, want, 2e-6, "wav_normalize")
    check(stats[:, 0], mean.view(-1), 1e-6, "mean")
    check(stats[:, 1], std.view(-1), 1e-6, "std")
    est = rnd(Bt, S, T, seed=96)
    ref = est * std + mean
    if mc:
        ref = ref + (want - ref.sum(1, keepdim=True)) / S      # mixture_consistency.py:14-36, uniform
    out = ops.wav_denormalize(dev32(est), stats, got if mc else None)
    check(out, ref, 5e-6, "wav_denormalize")


def test_stats_robust_to_large_mean():
    """E[x^2]-mu^2 in fp64 must survive mean >> std (fp32 accumulation would not)."""
    from sudo_rm_rf_amd import ops
    x = rnd(2, 16, 4096, seed=95, scale=0.05, shift=30.0)
    g, b = torch.ones(16, dtype=torch.float64), torch.zeros(16, dtype=torch.float64)
    x32 = x.to(torch.float32).to(torch.float64)           # what the kernel actually sees
    got = ops.glob_ln(dev32(x), dev32(g), dev32(b))
    check(got, gln64(x32, g, b), 2e-3, "large-mean GlobLN")   # (x-mu) itself loses bits in fp32


def test_tac_next_to_mfma_gemm():
    """gfx950 erratum regression (tools/probes/pk_opsel_probe.hip): a packed-fp32 instruction with
    op_sel = 1 on src1 returns a wrong low result in lanes 48..63 while ANOTHER wavefront's bf16 MFMA runs on the same
    SIMD.  The two-time-steps-per-lane TAC kernel contained that form (packed bias adds) and produced wrong columns in
    every run next to the split-bf16 GEMM of a second stream; serially it was always right.  TAC runs 16 times on one
    stream while a second stream loops over GEMM launches: every output equals the serial one bit for bit."""
    from sudo_rm_rf_amd import ops
    ops.set_kernel_mode(0)
    Bt, G, n, L = 20, 16, 16, 3200
    H = 3 * n
    x = dev32(rnd(Bt, G, n, L, seed=90))
    P = [dev32(t) for t in (rnd(H, n, seed=91, scale=n ** -0.5), rnd(H, seed=92, scale=0.2),
                            torch.tensor([0.2], dtype=torch.float64), rnd(H, H, seed=93, scale=H ** -0.5),
                            rnd(H, seed=94, scale=0.2), torch.tensor([0.3], dtype=torch.float64),
                            rnd(n, 2 * H, seed=95, scale=(2 * H) ** -0.5), rnd(n, seed=96, scale=0.2),
                            torch.tensor([0.15], dtype=torch.float64))]
    xg, wg, bg = dev32(rnd(32, 256, L, seed=97)), dev32(rnd(512, 256, 1, seed=98, scale=1 / 16)), dev32(rnd(512, seed=99))
    ref = ops.tac(x, P)
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    with torch.cuda.stream(sb):
        for _ in range(48):
            ops.pw_conv(xg, wg, bg)
    with torch.cuda.stream(sa):
        for _ in range(16):
            outs.append(ops.tac(x, P))
    torch.cuda.synchronize()
    bad = [i for i, o in enumerate(outs) if not torch.equal(o, ref)]
    assert not bad, "TAC outputs differ from the serial run next to the MFMA GEMM: runs %s" % bad
