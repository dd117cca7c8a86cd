"""Every kernel entry point off the 16-byte grid, with guard bands (tests/placement.py).

For every entry of placement.PLACEMENT: two shapes of that op's existing parametrisation (one where nothing is a multiple of
a tile, one that reaches its fast kernel -- asserted with ops.kernel_trace), the fullest prologue / epilogue variant and the
plain one, the fp64 reference and the tolerance of the op's existing test, and for each of them
  (a) every operand, output and scratch buffer on the grid, poisoned and guarded;
  (b) one operand at a time one float in, then all of them by different amounts: correct (FALLBACK rows, and the trace shows
      the kernel family the table names) or refused on the host with the operand's name and nothing written (REFUSES rows);
  (c) position-dependent inputs for the ops that gather.
Nothing here expects a fault: the expectation is always "correct" or "refused before any launch".
The whole-model, training, streaming and optimiser cases (poisoned workspaces, inputs as views) follow below."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import placement as pl

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ARENA_BYTES = 640 << 20
_NOT_FULLY_WRITTEN = {"scratch", "work", "packed"}       # buffers an op may leave partly unused


@pytest.fixture(scope="module")
def arena():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    from sudo_rm_rf_amd import _lib, ops
    _lib.load()
    ops.set_kernel_mode(0)
    ops.set_debug_flags(0)
    a = pl.Arena(DEV, ARENA_BYTES)
    yield a
    ops.set_kernel_mode(0)


# ---- data and references (restated from test_gpu_ops.py / test_gpu_backward.py / test_gpu_causal.py) ------------------
@functools.lru_cache(maxsize=24)
def rnd(*shape, seed=0, scale=1.0, shift=0.0):
    """(cached: the runs of one case differ in placement only, and nothing writes into these tensors)"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale + shift


def ramp(*shape):
    """row * 1000 + column scaled to O(1) (test_pw_conv_transpose_detecting): an off-by-one in a shifted base moves every
    value by a thousandth of the scale, a wrong row by the whole scale -- nothing can hide in it."""
    rows = int(np.prod(shape[:-1]))
    t = torch.arange(rows, dtype=torch.float64)[:, None] * 1000 + torch.arange(shape[-1], dtype=torch.float64)[None, :]
    return (t / (1000.0 * rows)).reshape(shape)


def f32(t):
    """what the kernel sees: the fp32 rounding of a host tensor, back in fp64"""
    return t.to(torch.float32).to(torch.float64)


def gln64(x, gamma, beta):
    dims = list(range(1, x.dim()))
    mu = x.mean(dim=dims, keepdim=True)
    var = ((x - mu) ** 2).mean(dim=dims, keepdim=True)
    shape = [1, -1] + [1] * (x.dim() - 2)
    return gamma.view(shape) * (x - mu) / (var + 1e-8).sqrt() + beta.view(shape)


def sums64(x):
    xf = x.reshape(x.shape[0], -1)
    out = torch.zeros(x.shape[0], 64, 2, dtype=torch.float64)
    out[:, 0, 0] = xf.sum(1)
    out[:, 0, 1] = (xf * xf).sum(1)
    return out


def prelu64(t, a):
    return torch.where(t >= 0, t, a * t)


class Abs:
    def __init__(self, tol):
        self.tol = tol

    def __call__(self, got, want, what):
        assert got.shape == want.shape, (what, got.shape, want.shape)
        err = (got - want).abs().max().item()
        assert err <= self.tol, "%s: max abs err %.3e > %.1e" % (what, err, self.tol)


class Rel:
    """max |got - want| / max |want| (test_gpu_backward.rel_err)"""

    def __init__(self, tol):
        self.tol = tol

    def __call__(self, got, want, what):
        assert got.shape == want.shape, (what, got.shape, want.shape)
        err = ((got - want).abs().max() / want.abs().max().clamp_min(1e-30)).item()
        assert err <= self.tol, "%s: rel err %.3e > %.1e" % (what, err, self.tol)


class Sums:
    """test_gpu_ops.check_sums: bucketed fp64 sums against the fp64 tensor they describe"""

    def __call__(self, got, x64, what):
        xf = x64.reshape(x64.shape[0], -1)
        got = got.sum(1)
        assert ((got[:, 0] - xf.sum(1)).abs() <= 4e-6 * xf.abs().sum(1) + 1e-9).all(), "%s: sum" % what
        assert ((got[:, 1] - (xf * xf).sum(1)).abs() <= 4e-6 * (xf * xf).sum(1) + 1e-9).all(), "%s: sumsq" % what


class Placer:
    """Places a case's operands in the arena at the shifts of one run and collects what must be checked afterwards."""

    def __init__(self, arena, shifts, use_ramp=False):
        self.arena, self.shifts, self.use_ramp = arena, shifts, use_ramp
        self.checks, self.placed, self.absent, self.trace, self.made, self.accum = [], set(), set(), None, pl._Made(), []

    def _shift(self, name, i=0):
        s = self.shifts.get(name, 0)
        return 0 if not s else (s - 1 + i) % 3 + 1

    def t(self, name, host, dtype=torch.float32, i=0):
        if host is None:
            return None
        self.placed.add(name)
        s = self._shift(name, i)
        if dtype == torch.float64 and s:
            s = 2
        return self.arena.put(host, dtype, s, name=name)

    def tl(self, name, hosts, dtype=torch.float32):
        return [self.t(name, h, dtype, i) for i, h in enumerate(hosts)]

    def z(self, name, shape, dtype=torch.float32):
        """a zeroed accumulator handed in by the caller (out_sums, dw=, gx= ...)"""
        self.placed.add(name)
        s = self._shift(name)
        if dtype == torch.float64 and s:
            s = 2
        v = self.arena.place(shape, dtype, s, name=name, zero=True)
        self.accum.append(v)
        return v

    def data(self, *shape, **kw):
        return ramp(*shape) if self.use_ramp else rnd(*shape, **kw)

    def run(self, names, fn):
        """fn() under the allocation proxy and the kernel trace; names = the wrapper's allocations in order"""
        from sudo_rm_rf_amd import ops
        self.placed.update(names)
        with self.arena.allocating(ops, names=names, shifts={n: self._shift(n) for n in set(names)}) as made:
            self.made = made
            with ops.kernel_trace(DEV) as tr:
                out = fn()
        self.trace = tr.names
        return out

    def want(self, what, got, ref64, crit):
        self.checks.append((what, got, ref64, crit))


# ---- the cases: fn(P, shape, variant) places, calls and registers references ----------------------------------------
def _prologue(P, x, Cin, pro, seeds=(13, 14), slope=0.17, prefix="in_"):
    """(f(x) in fp64, wrapper keywords) for prologue pro: 0 none, 1 GlobLN, 2 GlobLN + PReLU, 3 PReLU"""
    kw, xin = {}, f32(x)
    if pro in (1, 2):
        gamma, beta = rnd(Cin, seed=seeds[0], scale=0.3, shift=1.0), rnd(Cin, seed=seeds[1], scale=0.3)
        kw[prefix + "sums"] = P.t(prefix + "sums", sums64(xin), torch.float64)
        kw[prefix + "gamma"], kw[prefix + "beta"] = P.t(prefix + "gamma", gamma), P.t(prefix + "beta", beta)
        xin = gln64(xin, f32(gamma), f32(beta))
    if pro in (2, 3):
        a = torch.tensor([slope], dtype=torch.float64)
        kw[prefix + "prelu"] = P.t(prefix + "prelu", a)
        xin = prelu64(xin, f32(a))
    return xin, kw


def case_encoder(P, shape, variant):
    from sudo_rm_rf_amd import ops
    A, K, T, N, Bt = shape
    h, D = K // 2, 3
    nls = h * 2 ** D
    Tp = nls if T < nls else (T // nls + (1 if T % nls else 0)) * nls
    L = (Tp + 2 * h - K) // h + 1
    x, w = P.data(Bt, A, T, seed=1), rnd(N, A, K, seed=2, scale=0.3)
    xp = torch.zeros(Bt, A, Tp, dtype=torch.float64)
    xp[..., :T] = f32(x)
    want = F.conv1d(xp, f32(w), None, stride=h, padding=h)
    xd, wd = P.t("wav", x), P.t("weight", w)
    sums = P.z("sums", (Bt, 64, 2), torch.float64) if variant == "full" else None
    got = P.run(("out",), lambda: ops.encoder(xd, wd, L, sums))
    P.want("encoder", got, want, Abs(2e-5))
    if sums is not None:
        P.want("encoder sums", sums, want, Sums())


def case_gln_stats(P, shape, variant):
    from sudo_rm_rf_amd import ops
    x = rnd(*shape, seed=3, scale=2.0, shift=0.7)
    xd = P.t("x", x)
    got = P.run(("sums",), lambda: ops.gln_stats(xd, shape[0]))
    P.want("gln_stats", got, f32(x), Sums())


def case_gln_apply(P, shape, variant):
    from sudo_rm_rf_amd import ops
    x, g, b = rnd(*shape, seed=3, scale=2.0, shift=0.7), rnd(shape[1], seed=4), rnd(shape[1], seed=5)
    want = gln64(f32(x), f32(g), f32(b))
    kw = {}
    if variant == "full":       # the two forms the model has: + PReLU, or residual + GlobLN; the fullest of each in turn
        a, res = torch.tensor([0.2], dtype=torch.float64), rnd(*shape, seed=6)
        want_a = prelu64(want, f32(a))
        xd, sd, gd, bd = P.t("x", x), P.t("sums", sums64(f32(x)), torch.float64), P.t("gamma", g), P.t("beta", b)
        ad, rd = P.t("prelu", a), P.t("residual", res)
        got_a, got_r = P.run(("y", "y"), lambda: (ops.gln_apply(xd, sd, gd, bd, prelu=ad), ops.gln_apply(xd, sd, gd, bd, residual=rd)))
        P.want("gln_apply + prelu", got_a, want_a, Abs(2e-5))
        P.want("gln_apply + residual", got_r, f32(res) + want, Abs(3e-5))
        return
    xd, sd, gd, bd = P.t("x", x), P.t("sums", sums64(f32(x)), torch.float64), P.t("gamma", g), P.t("beta", b)
    got = P.run(("y",), lambda: ops.gln_apply(xd, sd, gd, bd, **kw))
    P.want("gln_apply", got, want, Abs(2e-5))


def case_glob_ln(P, shape, variant):
    from sudo_rm_rf_amd import ops
    x, g, b = rnd(*shape, seed=3, scale=2.0, shift=0.7), rnd(shape[1], seed=4), rnd(shape[1], seed=5)
    xd, gd, bd = P.t("x", x), P.t("gamma", g), P.t("beta", b)
    got = P.run(("sums", "y"), lambda: ops.glob_ln(xd, gd, bd))
    P.want("glob_ln", got, gln64(f32(x), f32(g), f32(b)), Abs(2e-5))


def _pw_data(P, Bt, Cin, Cout, L, seeds):
    x = P.data(Bt, Cin, L, seed=seeds, scale=1.5, shift=0.3)
    w = rnd(Cout, Cin, 1, seed=seeds + 1, scale=Cin ** -0.5)
    bias = rnd(Cout, seed=seeds + 2, scale=0.2)
    return x, w, bias


def _pw_ref(xin, w, bias):
    """fp64 1x1 conv on the GPU (the large shapes are 10 GFLOP) -> host"""
    return (torch.einsum("mk,bkl->bml", f32(w)[:, :, 0].to(DEV), xin.to(DEV)) + f32(bias).to(DEV).view(1, -1, 1)).cpu()


def _pw_tol(P, packed):
    """test_pw_conv's bar (5e-5, both kernel modes) -- for the packed model-sized launches test_pw_conv_persistent_variants'
    (1e-4), unless the exact-fp32 scalar kernel served the call: then the tighter of the two applies"""
    return 1e-4 if packed is not None and "pw_conv_generic" not in P.trace else 5e-5


def _pw3_tol(P, big):
    """2e-5 where the two-fp16-part kernel ran (test_pw_conv_pair_fp16_parts...), test_pw_conv's 5e-5 on the exact-fp32 scalar
    kernel and at small shapes, test_pw_conv_persistent_variants' 1e-4 where the launch fell to the two-bf16-part kernels"""
    if any(n.startswith("pw_conv_x3w4") for n in P.trace):
        return 2e-5
    return 5e-5 if (not big or "pw_conv_generic" in P.trace) else 1e-4


def case_pw_conv(P, shape, variant):
    from sudo_rm_rf_amd import ops
    Bt, Cin, Cout, L = shape
    if variant == "mask":                                  # test_pw_conv_mask_epilogue
        N, S = Cout // 2, 2
        x, w, bias = rnd(Bt, Cin, L, seed=20), rnd(Cout, Cin, 1, seed=21, scale=0.2), rnd(Cout, seed=22)
        enc, slope = rnd(Bt, N, L, seed=23), torch.tensor([0.3], dtype=torch.float64)
        m = _pw_ref(prelu64(f32(x), f32(slope)), w, bias)
        want = (torch.relu(m.view(Bt, S, N, L)) * f32(enc).unsqueeze(1)).view(Bt, Cout, L)
        xd, wd, bd, ad, ed = P.t("x", x), P.t("weight", w), P.t("bias", bias), P.t("in_prelu", slope), P.t("mask_mul", enc)
        got = P.run(("y",), lambda: ops.pw_conv(xd, wd, bd, in_prelu=ad, mask_mul=ed))
        # 2e-4 on the split-bf16 kernels, 2e-5 on the exact-fp32 ones (the scalar kernel is one of them)
        P.want("pw_conv mask epilogue", got, want, Abs(2e-5 if P.trace == {"pw_conv_generic"} else 2e-4))
        return
    x, w, bias = _pw_data(P, Bt, Cin, Cout, L, 10)
    xd, wd, bd = P.t("x", x), P.t("weight", w), P.t("bias", bias)
    packed = None
    if variant.startswith("packed"):
        img = ops.pack_pw_weight(w.to(torch.float32).to(DEV))
        assert img is not None
        packed = P.t("packed", img, torch.uint8)
    if variant in ("plain", "packed-plain"):
        got = P.run(("y",), lambda: ops.pw_conv(xd, wd, bd, packed=packed))
        P.want("pw_conv", got, _pw_ref(f32(x), w, bias), Abs(_pw_tol(P, packed)))
        return
    xin, kw = _prologue(P, x, Cin, 2)
    res = rnd(Bt, Cout, L, seed=15)
    want = _pw_ref(xin, w, bias) + f32(res)
    rd, osums = P.t("residual", res), P.z("out_sums", (Bt, 64, 2), torch.float64)
    got = P.run(("y",), lambda: ops.pw_conv(xd, wd, bd, residual=rd, out_sums=osums, packed=packed, **kw))
    P.want("pw_conv pro=2 + residual", got, want, Abs(_pw_tol(P, packed)))
    P.want("pw_conv sums", osums, want, Sums())


def case_pack(P, shape, variant, three=False):
    from sudo_rm_rf_amd import ops
    Cout, Cin = shape
    wd = P.t("weight", rnd(Cout, Cin, 1, seed=41, scale=Cin ** -0.5))
    img = P.run(("packed",), lambda: (ops.pack3_pw_weight if three else ops.pack_pw_weight)(wd))
    assert img is not None and P.arena.owns(img)
    # the image is proved by use: a conv through it against fp64
    Bt, L = 16, 3200          # 400 tiles of 256 x 128: the kernel that reads the image serves the launch
    x, bias = rnd(Bt, Cin, L, seed=40, scale=1.3, shift=0.2), rnd(Cout, seed=42, scale=0.2)
    xd, bd = x.to(torch.float32).to(DEV), bias.to(torch.float32).to(DEV)
    got = ops.pw_conv3(xd, wd, bd, img) if three else ops.pw_conv(xd, wd, bd, packed=img)
    want = _pw_ref(f32(x), f32(wd.cpu().double()), bias)
    P.want("conv through the packed image", got, want, Abs(2e-5 if three else 1e-4))


def case_pw_conv3(P, shape, variant):
    from sudo_rm_rf_amd import ops
    Bt, Cin, Cout, L = shape
    x = rnd(Bt, Cin, L, seed=150, scale=1.3, shift=0.2)
    w, bias = rnd(Cout, Cin, 1, seed=151, scale=Cin ** -0.5), rnd(Cout, seed=152, scale=0.2)
    xd, wd, bd = P.t("x", x), P.t("weight", w), P.t("bias", bias)
    img = ops.pack3_pw_weight(w.to(torch.float32).to(DEV))
    packed3 = None
    if img is not None:
        # a copy of the image: the library's format record is per address, an unrecorded address is taken as it comes
        packed3 = P.t("packed3", img, torch.uint8)
    else:
        P.absent.add("packed3")               # (a shape the three-part kernel does not take: the call IS srf_pw_conv)
    big = Cin >= 256
    if variant == "plain":
        osums = P.z("out_sums", (Bt, 64, 2), torch.float64)
        got = P.run(("y",), lambda: ops.pw_conv3(xd, wd, bd, packed3, out_sums=osums))
        want = _pw_ref(f32(x), w, bias)
        P.want("pw_conv3", got, want, Abs(_pw3_tol(P, big)))
        P.want("pw_conv3 sums", osums, want, Sums())
        return
    xin, kw = _prologue(P, x, Cin, 2, seeds=(156, 157))
    res = rnd(Bt, Cout, L, seed=155)
    rd = P.t("residual", res)
    got = P.run(("y",), lambda: ops.pw_conv3(xd, wd, bd, packed3, residual=rd, **kw))
    P.want("pw_conv3 pro=2 + residual", got, _pw_ref(xin, w, bias) + f32(res), Abs(_pw3_tol(P, big)))


def case_pw_pair(P, shape, variant, three=False):
    from sudo_rm_rf_amd import ops
    Bt, Cin1, Cout2, L = shape
    Cmid = 256
    supported = ops.pw_conv_pair3_supported if three else ops.pw_conv_pair_supported
    assert supported(Bt, Cin1, Cmid, Cout2, L), "the shapes were chosen as served ones"
    x = rnd(Bt, Cin1, L, seed=50, scale=1.3, shift=0.2)
    w1, b1 = rnd(Cmid, Cin1, 1, seed=51, scale=Cin1 ** -0.5), rnd(Cmid, seed=52, scale=0.2)
    w2, b2 = rnd(Cout2, Cmid, 1, seed=53, scale=Cmid ** -0.5), rnd(Cout2, seed=54, scale=0.2)
    # full: GlobLN + PReLU prologue, residual, statistics; plain: the barest form the entry point has
    pro = 2 if variant == "full" else (1 if three else 0)
    res = rnd(Bt, Cmid, L, seed=55) if pro != 1 else None
    pack = ops.pack3_pw_weight if three else ops.pack_pw_weight
    i1, i2 = pack(w1.to(torch.float32).to(DEV)), pack(w2.to(torch.float32).to(DEV))
    shifted_image = any(P.shifts.get(n) for n in ("packed1", "packed2", "packed3_1", "packed3_2"))
    n1, n2 = ("packed3_1", "packed3_2") if three else ("packed1", "packed2")
    if three and not shifted_image:
        p1, p2 = i1, i2          # (the fp16 pair wants the very buffers srf_pack3_pw_weights wrote: recorded per address)
        P.placed.update((n1, n2))
    else:
        p1, p2 = P.t(n1, i1, torch.uint8), P.t(n2, i2, torch.uint8)
    xd, b1d, b2d, rd = P.t("x", x), P.t("bias1", b1), P.t("bias2", b2), P.t("residual", res)
    xin, kw = _prologue(P, x, Cin1, pro, seeds=(56, 57))
    osums = P.z("out_sums2", (Bt, 64, 2), torch.float64) if variant == "full" else None
    fn = ops.pw_conv_pair3 if three else ops.pw_conv_pair
    y, y2 = P.run(("y", "y2"), lambda: fn(xd, p1, b1d, kw.get("in_sums"), kw.get("in_gamma"), kw.get("in_beta"), kw.get("in_prelu"),
                                          rd, p2, b2d, Cmid, Cout2, out_sums2=osums))
    want1 = _pw_ref(xin, w1, b1)
    if res is not None:
        want1 = want1 + f32(res)
    tol = 2e-5 if three else 1e-4
    P.want("pair: y", y, want1, Abs(tol))
    P.want("pair: y2", y2, _pw_ref(y.double().cpu(), w2, b2), Abs(tol))
    if osums is not None:
        P.want("pair: statistics of y2", osums, y2.double().cpu(), Sums())


def case_dwconv5(P, shape, variant):
    from sudo_rm_rf_amd import ops
    Bt, C, Lin, stride = shape
    x = P.data(Bt, C, Lin, seed=30, scale=1.3, shift=-0.4)
    w, bias = rnd(C, 1, 5, seed=31, scale=0.5), rnd(C, seed=32, scale=0.2)
    xd, wd, bd = P.t("x", x), P.t("weight", w), P.t("bias", bias)
    xin, kw = _prologue(P, x, C, 2 if variant == "full" else 0, seeds=(33, 34), slope=0.21)
    want = F.conv1d(xin, f32(w), f32(bias), stride=stride, padding=2, groups=C)
    osums = P.z("out_sums", (Bt, 64, 2), torch.float64) if variant == "full" else None
    got = P.run(("y",), lambda: ops.dwconv5(xd, wd, bd, stride, out_sums=osums, **kw))
    P.want("dwconv5", got, want, Abs(2e-5))
    if osums is not None:
        P.want("dwconv5 sums", osums, want, Sums())


def case_conv1d(P, shape, variant):
    from sudo_rm_rf_amd import ops
    Bt, Cin, Cout, Lin, K, stride, pad, dil, groups = shape
    x = rnd(Bt, Cin, Lin, seed=200)
    w, bias = rnd(Cout, Cin // groups, K, seed=201, scale=(Cin // groups * K) ** -0.5), rnd(Cout, seed=202, scale=0.2)
    want = F.conv1d(f32(x), f32(w), f32(bias), stride=stride, padding=pad, dilation=dil, groups=groups)
    xd, wd, bd = P.t("x", x), P.t("weight", w), P.t("bias", bias)
    osums = P.z("out_sums", (Bt, 64, 2), torch.float64) if variant == "full" else None
    got = P.run(("y",), lambda: ops.conv1d(xd, wd, bd, stride, pad, dil, groups, out_sums=osums))
    P.want("conv1d", got, want, Abs(2e-5))
    if osums is not None:
        P.want("conv1d sums", osums, want, Sums())


def case_merge(P, shape, variant):
    from sudo_rm_rf_amd import ops
    Bt, C, L, D = shape
    levels = [P.data(Bt, C, L >> k, seed=40 + k, scale=1.0 + 0.2 * k, shift=0.1 * k) * (1 if not P.use_ramp else 1 + k) for k in range(D)]
    gam = [rnd(C, seed=50 + k, scale=0.3, shift=1.0) for k in range(D)]
    bet = [rnd(C, seed=60 + k, scale=0.3) for k in range(D)]
    normed = [gln64(f32(levels[k]), f32(gam[k]), f32(bet[k])) for k in range(D)]
    u = normed[-1]
    for k in range(D - 2, -1, -1):
        u = normed[k] + u.repeat_interleave(2, dim=-1)
    lv, sm = P.tl("levels", levels), P.tl("sums", [sums64(f32(t)) for t in levels], torch.float64)
    gd, bd = P.tl("gammas", gam), P.tl("betas", bet)
    osums = P.z("out_sums", (Bt, 64, 2), torch.float64) if variant == "full" else None
    got = P.run(("y",), lambda: ops.merge(lv, sm, gd, bd, out_sums=osums))
    P.want("merge", got, u, Abs(3e-5))
    if osums is not None:
        P.want("merge sums", osums, u, Sums())


def case_pyramid(P, shape, variant):
    from sudo_rm_rf_amd import ops
    Bt, C, L, D = shape
    y1 = rnd(Bt, C, L, seed=100, scale=1.4, shift=0.2)
    g_in, b_in = rnd(C, seed=101, scale=0.3, shift=1.0), rnd(C, seed=102, scale=0.3)
    slope = torch.tensor([0.23], dtype=torch.float64)
    W = [rnd(C, 1, 5, seed=110 + k, scale=0.5) for k in range(D)]
    Bi = [rnd(C, seed=120 + k, scale=0.2) for k in range(D)]
    Ga = [rnd(C, seed=130 + k, scale=0.3, shift=1.0) for k in range(D)]
    Be = [rnd(C, seed=140 + k, scale=0.3) for k in range(D)]
    cur = prelu64(gln64(f32(y1), f32(g_in), f32(b_in)), f32(slope))
    outs = []
    for k in range(D):
        d = F.conv1d(cur, f32(W[k]), f32(Bi[k]), stride=1 if k == 0 else 2, padding=2, groups=C)
        cur = gln64(d, f32(Ga[k]), f32(Be[k]))
        outs.append(cur)
    u = outs[-1]
    for k in range(D - 2, -1, -1):
        u = outs[k] + u.repeat_interleave(2, dim=-1)
    yd, sd = P.t("y1", y1), P.t("in_sums", sums64(f32(y1)), torch.float64)
    gd, bd, ad = P.t("in_gamma", g_in), P.t("in_beta", b_in), P.t("in_prelu", slope)
    Wd, Bd, Gd, Ed = P.tl("weights", W), P.tl("biases", Bi), P.tl("gammas", Ga), P.tl("betas", Be)
    osums = P.z("out_sums", (Bt, 64, 2), torch.float64) if variant == "full" else None
    got = P.run(("merged", "scratch"), lambda: ops.pyramid(yd, sd, gd, bd, ad, Wd, Bd, Gd, Ed, out_sums=osums))
    P.want("fused pyramid", got, u, Abs(5e-5))
    if osums is not None:
        P.want("fused pyramid sums", osums, u, Sums())


def case_decoder(P, shape, variant):
    from sudo_rm_rf_amd import ops
    Bt, Ci, Co, K, L, T = shape
    h = K // 2
    v, w = P.data(Bt, Ci, L, seed=70), rnd(Ci, Co, K, seed=71, scale=Ci ** -0.5)
    want = F.conv_transpose1d(f32(v), f32(w), None, stride=h, padding=h, output_padding=h - 1)[..., :T]
    vd, wd = P.t("v", v), P.t("weight", w)
    got = P.run(("scratch", "out"), lambda: ops.decoder(vd, wd, T))
    P.want("decoder", got, want, Abs(3e-5))


def _tac_params(n, seed0):
    H = 3 * n
    return [rnd(H, n, seed=seed0 + 1, scale=n ** -0.5), rnd(H, seed=seed0 + 2, scale=0.2), torch.tensor([0.2], dtype=torch.float64),
            rnd(H, H, seed=seed0 + 3, scale=H ** -0.5), rnd(H, seed=seed0 + 4, scale=0.2), torch.tensor([0.3], dtype=torch.float64),
            rnd(n, 2 * H, seed=seed0 + 5, scale=(2 * H) ** -0.5), rnd(n, seed=seed0 + 6, scale=0.2),
            torch.tensor([0.15], dtype=torch.float64)]


def _tac64(x, P_, Bt, G, n, L):
    H = 3 * n
    rows = x.permute(0, 3, 1, 2).reshape(-1, n)
    z = prelu64(rows @ P_[0].T + P_[1], P_[2]).view(Bt, L, G, H)
    q = prelu64(z.mean(2).view(Bt * L, H) @ P_[3].T + P_[4], P_[5])
    cat = torch.cat([z.view(Bt * L, G, H), q.unsqueeze(1).expand(Bt * L, G, H)], 2).reshape(-1, 2 * H)
    return prelu64(cat @ P_[6].T + P_[7], P_[8]).view(Bt, L, G, n).permute(0, 2, 3, 1).contiguous()


def case_tac(P, shape, variant):
    from sudo_rm_rf_amd import ops
    Bt, G, n, L = shape
    x, pr = rnd(Bt, G, n, L, seed=80), _tac_params(n, 80)
    o = _tac64(f32(x), [f32(p) for p in pr], Bt, G, n, L)
    xd, pd = P.t("x4", x), P.tl("params", pr)
    osums = P.z("out_sums", (Bt * G, 64, 2), torch.float64) if variant == "full" else None
    got = P.run(("q",), lambda: ops.tac(xd, pd, out_sums=osums))
    P.want("tac", got, o, Abs(2e-5))
    if osums is not None:
        P.want("tac sums", osums, o.view(Bt * G, n, L), Sums())


def case_tac_bwd(P, shape, variant):
    from sudo_rm_rf_amd import ops
    Bt, G, n, L = shape
    x = f32(rnd(Bt, G, n, L, seed=90)).requires_grad_(True)
    pr = [f32(p).requires_grad_(True) for p in _tac_params(n, 90)]
    go = rnd(Bt, G, n, L, seed=97)
    _tac64(x, pr, Bt, G, n, L).backward(f32(go))
    xd, gd, pd = P.t("x", x.detach()), P.t("go", go), P.tl("params", [p.detach() for p in pr])
    gx, grads = P.run(("grads",) * 9 + ("gx", "scratch"), lambda: ops.tac_bwd(xd, gd, pd))
    P.want("tac_bwd gx", gx, x.grad, Rel(3e-5))
    for i, (g, p) in enumerate(zip(grads, pr)):
        P.want("tac_bwd grad %d" % i, g, p.grad, Rel(5e-5))


def case_mixture_consistency(P, shape, variant):
    from sudo_rm_rf_amd import ops
    from oracle import np_oracle
    Bt, S, T = shape
    if variant == "full":                                   # the magsq weights (test_mixture_consistency_magsq)
        pr = rnd(Bt, S, T, seed=92) * torch.arange(1, S + 1, dtype=torch.float64).view(1, S, 1)
        mix = rnd(Bt, 1, T, seed=102)
        want = torch.from_numpy(np_oracle.mixture_consistency(f32(pr).numpy(), f32(mix).numpy(), "magsq"))
        pd, md = P.t("pr_batch", pr), P.t("input_mixture", mix)
        got = P.run(("out", "work"), lambda: ops.mixture_consistency(pd, md, "magsq"))
        P.want("mixture consistency magsq", got, want, Abs(2e-6 * float(want.abs().max())))
        return
    pr, mix = rnd(Bt, S, T, seed=90), rnd(Bt, 1, T, seed=91)
    pd, md = P.t("pr_batch", pr), P.t("input_mixture", mix)
    got = P.run(("out",), lambda: ops.mixture_consistency(pd, md))
    P.want("mixture consistency", got, f32(pr) + (f32(mix) - f32(pr).sum(1, keepdim=True)) / S, Abs(1e-6))


def case_pw_wgrad(P, shape, variant):
    from sudo_rm_rf_amd import ops
    Bt, Cin, Cout, L = shape
    x, g = rnd(Bt, Cin, L, seed=1, scale=1.3, shift=0.2), rnd(Bt, Cout, L, seed=2, scale=0.7)
    gd, xd = P.t("g", g), P.t("x", x)
    fx, kw = _prologue(P, x, Cin, 2 if variant == "full" else 0, seeds=(3, 4))
    want_w = torch.einsum("bml,bnl->mn", f32(g).to(DEV), fx.to(DEV)).cpu()
    want_b = f32(g).sum(dim=(0, 2))
    if variant == "full":                                   # ... accumulating into zeroed dw / dbias
        dw, db = P.z("dw", (Cout, Cin)), P.z("dbias", (Cout,))
        P.run(("scratch",), lambda: ops.pw_wgrad(gd, xd, dw=dw, dbias=db, **kw))
    else:
        dw, db = P.run(("dw", "dbias", "scratch"), lambda: ops.pw_wgrad(gd, xd, **kw))
    P.want("pw_wgrad dw", dw, want_w, Rel(2e-5))
    P.want("pw_wgrad dbias", db, want_b, Rel(2e-5))


def case_gln_bwd(P, shape, variant):
    from sudo_rm_rf_amd import ops
    Bt, C, L = shape
    act = variant == "full"
    x = f32(rnd(Bt, C, L, seed=10, scale=1.7, shift=-0.4)).requires_grad_(True)
    gamma = f32(rnd(C, seed=11, scale=0.3, shift=1.0)).requires_grad_(True)
    beta = f32(rnd(C, seed=12, scale=0.3)).requires_grad_(True)
    slope = torch.tensor([0.23], dtype=torch.float32).double().requires_grad_(True)
    gout, gout2 = rnd(Bt, C, L, seed=13), rnd(Bt, C, L, seed=14, scale=0.5)
    y = gln64(x, gamma, beta)
    if act:
        y = prelu64(y, slope)
    y.backward(f32(gout) + (f32(gout2) if act else 0))
    god, xd = P.t("gout", gout), P.t("x", x.detach())
    sd, gd, bd = P.t("sums", sums64(x.detach()), torch.float64), P.t("gamma", gamma.detach()), P.t("beta", beta.detach())
    if act:          # PReLU, the second gradient, every accumulator handed in zeroed
        ad, g2d = P.t("prelu", slope.detach()), P.t("gout2", gout2)
        gx, dg, db, ds = P.z("gx", (Bt, C, L)), P.z("dgamma", (C,)), P.z("dbeta", (C,)), P.z("dslope", (1,))
        P.run(("scratch",), lambda: ops.gln_bwd(god, xd, sd, gd, bd, prelu=ad, gout2=g2d, gx=gx, dgamma=dg, dbeta=db, dslope=ds))
        P.want("gln_bwd dslope", ds, slope.grad, Rel(3e-5))
    else:
        gx, dg, db, _ = P.run(("gx", "dgamma", "dbeta", "scratch"), lambda: ops.gln_bwd(god, xd, sd, gd, bd))
    P.want("gln_bwd gx", gx, x.grad, Rel(3e-5))
    P.want("gln_bwd dgamma", dg, gamma.grad, Rel(3e-5))
    P.want("gln_bwd dbeta", db, beta.grad, Rel(3e-5))


def case_merge_bwd(P, shape, variant):
    from sudo_rm_rf_amd import ops
    Bt, C, L, D = shape
    levels = [torch.zeros(Bt, C, L >> k, dtype=torch.float64, requires_grad=True) for k in range(D)]
    out = levels[-1]
    for k in range(D - 2, -1, -1):
        out = levels[k] + F.interpolate(out, scale_factor=2, mode="nearest")
    gm = P.data(Bt, C, L, seed=30)
    out.backward(f32(gm))
    gd = P.t("g_merged", gm)
    got = P.run(("levels",) * (D - 1), lambda: ops.merge_bwd(gd, D))
    for k in range(D):
        P.want("merge_bwd level %d" % k, got[k], levels[k].grad, Rel(1e-6))


def case_dwconv5_bwd(P, shape, variant):
    from sudo_rm_rf_amd import ops
    Bt, C, Lin, stride = shape
    x = rnd(Bt, C, Lin, seed=40, scale=1.4, shift=0.3)
    w = f32(rnd(C, 1, 5, seed=41, scale=0.4)).requires_grad_(True)
    b = f32(rnd(C, seed=42, scale=0.2)).requires_grad_(True)
    xd, wd = P.t("xin", x), P.t("weight", w.detach())
    u, kw = _prologue(P, x, C, 2 if variant == "full" else 0, seeds=(43, 44), slope=0.21)
    u = u.detach().requires_grad_(True)
    d = F.conv1d(u, w, b, stride=stride, padding=2, groups=C)
    gd = rnd(*d.shape, seed=45)
    d.backward(f32(gd))
    gdd = P.t("gd", gd)
    if variant == "full":
        dw, db = P.z("dw", (C, 1, 5)), P.z("dbias", (C,))
        gin, _, _ = P.run(("gin", "scratch"), lambda: ops.dwconv5_bwd(gdd, xd, wd, stride, dw=dw, dbias=db, **kw))
    else:
        gin, dw, db = P.run(("gin", "dw", "dbias", "scratch"), lambda: ops.dwconv5_bwd(gdd, xd, wd, stride, **kw))
    P.want("dwconv5_bwd gin", gin, u.grad, Rel(2e-6))
    P.want("dwconv5_bwd dw", dw, w.grad, Rel(2e-5))
    P.want("dwconv5_bwd dbias", db, b.grad, Rel(2e-5))


def case_mask_apply(P, shape, variant):
    from sudo_rm_rf_amd import ops
    Bt, S, N, L = shape
    m, e = rnd(Bt, S * N, L, seed=50), rnd(Bt, N, L, seed=51)
    md, ed = P.t("m", m), P.t("enc", e)
    got = P.run(("v",), lambda: ops.mask_apply(md, ed))
    P.want("mask_apply", got, (torch.relu(f32(m)).view(Bt, S, N, L) * f32(e).unsqueeze(1)).reshape(Bt, S * N, L), Rel(1e-6))


def case_mask_bwd(P, shape, variant):
    from sudo_rm_rf_amd import ops
    Bt, S, N, L = shape
    m, e = f32(rnd(Bt, S * N, L, seed=50)).requires_grad_(True), f32(rnd(Bt, N, L, seed=51)).requires_grad_(True)
    gv = rnd(Bt, S * N, L, seed=52)
    (torch.relu(m).view(Bt, S, N, L) * e.unsqueeze(1)).reshape(Bt, S * N, L).backward(f32(gv))
    gvd, md, ed = P.t("gv", gv), P.t("m", m.detach()), P.t("enc", e.detach())
    if variant == "full":
        genc = P.z("genc", (Bt, N, L))
        gm, _ = P.run(("gm",), lambda: ops.mask_bwd(gvd, md, ed, genc=genc))
    else:
        gm, genc = P.run(("genc", "gm"), lambda: ops.mask_bwd(gvd, md, ed))
    P.want("mask_bwd gm", gm, m.grad, Rel(1e-6))
    P.want("mask_bwd genc", genc, e.grad, Rel(2e-6))


def case_prelu_bwd(P, shape, variant):
    from sudo_rm_rf_amd import ops
    x = f32(rnd(*shape, seed=60)).requires_grad_(True)
    a = torch.tensor([0.31], dtype=torch.float32).double().requires_grad_(True)
    g = rnd(*shape, seed=61)
    F.prelu(x, a).backward(f32(g))
    gd, xd, ad = P.t("gout", g), P.t("x", x.detach()), P.t("slope", a.detach())
    if variant == "full":
        ds = P.z("dslope", (1,))
        gx, _ = P.run(("gx",), lambda: ops.prelu_bwd(gd, xd, ad, dslope=ds))
    else:
        gx, ds = P.run(("gx", "dslope"), lambda: ops.prelu_bwd(gd, xd, ad))
    P.want("prelu_bwd gx", gx, x.grad, Rel(1e-6))
    P.want("prelu_bwd dslope", ds, a.grad, Rel(1e-5))


def case_frames_gather(P, shape, variant):
    from sudo_rm_rf_amd import ops
    Bt, R, T, K, L, rows_out = shape
    h = K // 2
    src = P.data(Bt, R, T, seed=70)
    want = torch.zeros(Bt, rows_out or R * K, L, dtype=torch.float64)
    s = F.pad(f32(src), (h, h * L + K))
    for k in range(K):
        want[:, k:R * K:K, :] = s[:, :, k:k + h * L:h][:, :, :L]
    sd = P.t("src", src)
    got = P.run(("out",), lambda: ops.frames_gather(sd, K, h, h, L, rows_out=rows_out))
    P.want("frames_gather", got, want, Abs(0.0))


def case_wav_normalize(P, shape, variant):
    from sudo_rm_rf_amd import ops
    Bt, S, T = shape
    x = f32(rnd(Bt, 1, T, seed=95, scale=3.0, shift=0.7))
    std, mean = x.std(-1, keepdim=True), x.mean(-1, keepdim=True)
    xd = P.t("wav", x)
    got, stats = P.run(("out", "stats"), lambda: ops.wav_normalize(xd))
    P.want("wav_normalize", got, (x - mean) / (std + 1e-9), Abs(2e-6))
    P.want("mean", stats[:, 0], mean.view(-1), Abs(1e-6))
    P.want("std", stats[:, 1], std.view(-1), Abs(1e-6))


def case_wav_denormalize(P, shape, variant):
    from sudo_rm_rf_amd import ops
    Bt, S, T = shape
    x = f32(rnd(Bt, 1, T, seed=95, scale=3.0, shift=0.7))
    std, mean = x.std(-1, keepdim=True), x.mean(-1, keepdim=True)
    norm = f32((x - mean) / (std + 1e-9))
    stats = f32(torch.cat([mean, std], dim=-1).view(Bt, 2))
    est = rnd(Bt, S, T, seed=96)
    ref = f32(est) * stats[:, 1].view(Bt, 1, 1) + stats[:, 0].view(Bt, 1, 1)
    mc = variant == "full"
    if mc:
        ref = ref + (norm - ref.sum(1, keepdim=True)) / S
    ed, sd, md = P.t("est", est), P.t("stats", stats), P.t("mix_norm", norm if mc else None)
    got = P.run(("out",), lambda: ops.wav_denormalize(ed, sd, md))
    P.want("wav_denormalize", got, ref, Abs(5e-6))


def _causal_level(src, w, b, a_out, stride, C):
    return F.prelu(F.conv1d(F.pad(src, (10, 0)), w[..., :11], b, stride=stride, groups=C), a_out)


def _causal_params(C, D, seed):
    g = torch.Generator().manual_seed(seed)
    ws = [(torch.randn(C, 1, 21, generator=g) * 0.3).double() for _ in range(D)]
    bs = [(torch.randn(C, generator=g) * 0.1).double() for _ in range(D)]
    acts = [(torch.rand(1, generator=g) * 0.4).double() for _ in range(D)]
    ap = (torch.rand(1, generator=g) * 0.4).double()
    return ws, bs, acts, ap


def _causal_pyramid64(y1, ap, ws, bs, acts):
    lv, src = [], F.prelu(y1, ap)
    for k in range(len(ws)):
        src = _causal_level(src, ws[k], bs[k], acts[k], 1 if k == 0 else 2, y1.shape[1])
        lv.append(src)
    out = lv[-1]
    for k in range(len(lv) - 2, -1, -1):
        out = lv[k] + torch.repeat_interleave(out, 2, dim=-1)
    return out


def case_causal_encoder(P, shape, variant):
    from sudo_rm_rf_amd import ops
    Bt, A, T, N, K, L = shape
    h = K // 2
    x, w = P.data(Bt, A, T, seed=300), rnd(N, A, 2 * K - 1, seed=301, scale=0.3)
    xp = F.pad(f32(x), (2 * h, h * L + K))
    want = F.conv1d(xp, f32(w)[..., :K], None, stride=h)[..., :L]
    xd, wd = P.t("wav", x), P.t("weight", w)
    got = P.run(("out",), lambda: ops.causal_encoder(xd, wd, L))
    P.want("causal_encoder", got, want, Abs(1e-5))


def case_causal_dwconv(P, shape, variant):
    from sudo_rm_rf_amd import ops
    Bt, C, Lin, stride = shape
    ws, bs, acts, ap = _causal_params(C, 1, Bt * 1000 + C + Lin)
    x = P.data(Bt, C, Lin, seed=310)
    full = variant == "full"
    src = F.prelu(f32(x), ap) if full else f32(x)
    want = F.conv1d(F.pad(src, (10, 0)), ws[0][..., :11], bs[0], stride=stride, groups=C)
    if full:
        want = F.prelu(want, acts[0])
    xd, wd, bd = P.t("x", x), P.t("weight", ws[0]), P.t("bias", bs[0])
    ad, od = P.t("in_prelu", ap if full else None), P.t("out_prelu", acts[0] if full else None)
    got = P.run(("y",), lambda: ops.causal_dwconv(xd, wd, bd, stride, in_prelu=ad, out_prelu=od))
    P.want("causal_dwconv", got, want, Abs(1e-5))


def case_causal_merge(P, shape, variant):
    from sudo_rm_rf_amd import ops
    Bt, C, L, D = shape
    levels = [rnd(Bt, C, L >> k, seed=320 + k) for k in range(D)]
    out = f32(levels[-1])
    for k in range(D - 2, -1, -1):
        out = f32(levels[k]) + torch.repeat_interleave(out, 2, dim=-1)
    lv = P.tl("levels", levels)
    got = P.run(("y",), lambda: ops.causal_merge(lv))
    P.want("causal_merge", got, out, Abs(1e-5))


def case_causal_pyramid(P, shape, variant):
    from sudo_rm_rf_amd import ops
    Bt, C, L, D = shape
    ws, bs, acts, ap = _causal_params(C, D, Bt * 1000 + C + L + D)
    y1 = rnd(Bt, C, L, seed=330)
    want = _causal_pyramid64(f32(y1), ap, ws, bs, acts)
    assert ops.causal_pyramid_supported(C, L, D)
    yd, ad = P.t("y1", y1), P.t("in_prelu", ap)
    wd, bd, pd = P.tl("weights", ws), P.tl("biases", bs), P.tl("prelus", acts)
    got = P.run(("merged",), lambda: ops.causal_pyramid(yd, ad, wd, bd, pd))
    P.want("causal_pyramid", got, want, Abs(1e-5))


def case_causal_stream_pyramid(P, shape, variant):
    """two chunks against the whole-sequence pyramid; the state tensors are updated in place"""
    from sudo_rm_rf_amd import ops
    Bt, C, L, D = shape
    ws, bs, acts, ap = _causal_params(C, D, Bt * 1000 + C + L + D)
    y1 = rnd(Bt, C, L, seed=340)
    want = _causal_pyramid64(f32(y1), ap, ws, bs, acts)
    cut = (L // 2) // (1 << (D - 1)) * (1 << (D - 1))
    a, b = P.t("y1", y1[..., :cut].contiguous()), P.t("y1", y1[..., cut:].contiguous())
    state = P.tl("state", [torch.zeros(Bt, C, 10, dtype=torch.float64) for _ in range(D)])
    ad, wd, bd, pd = P.t("in_prelu", ap), P.tl("weights", ws), P.tl("biases", bs), P.tl("prelus", acts)
    m1, m2 = P.run(("merged", "merged"), lambda: (ops.causal_stream_pyramid(a, state, ad, wd, bd, pd),
                                                  ops.causal_stream_pyramid(b, state, ad, wd, bd, pd)))
    P.want("stream pyramid, first chunk", m1, want[..., :cut], Abs(1e-5))
    P.want("stream pyramid, second chunk", m2, want[..., cut:], Abs(1e-5))


def case_causal_scale(P, shape, variant):
    from sudo_rm_rf_amd import ops
    src, ds = rnd(*shape, seed=350), torch.tensor([0.37], dtype=torch.float64)
    sd, dd = P.t("src", src), P.t("dscale", ds if variant == "full" else None)
    got = P.run(("dst",), lambda: ops.causal_scale(sd, dd, 1.25))
    want = f32(src) * 1.25 * (f32(ds) if variant == "full" else 1.0)
    P.want("causal_scale", got, want, Rel(1e-6))


def case_prelu(P, shape, variant):
    from sudo_rm_rf_amd import ops
    x, a = rnd(*shape, seed=360), torch.tensor([0.31], dtype=torch.float64)
    xd, ad = P.t("x", x), P.t("slope", a)
    got = P.run(("y",), lambda: ops.prelu(xd, ad))
    P.want("prelu", got, prelu64(f32(x), f32(a)), Rel(1e-6))


# key -> (PLACEMENT entry, case, [ragged shape, fast shape], {variant: operands shifted one at a time}, fast kernel family)
_PRO4 = ["in_sums", "in_gamma", "in_beta", "in_prelu"]
CASES = {
    "encoder": ("encoder", case_encoder, [(1, 21, 1237, 33, 3), (1, 21, 32000, 96, 2)],
                {"full": ["wav", "weight", "sums", "out"], "plain": []}, "encoder"),
    "gln_stats": ("gln_stats", case_gln_stats, [(3, 40, 333), (2, 64, 3200)], {"plain": ["x", "sums"]}, "gln_stats"),
    "gln_apply": ("gln_apply", case_gln_apply, [(3, 40, 333), (2, 64, 3200)],
                  {"full": ["x", "sums", "gamma", "beta", "prelu", "residual", "y"], "plain": []}, "gln_apply"),
    "glob_ln": ("glob_ln", case_glob_ln, [(3, 40, 333), (2, 64, 3200)], {"plain": ["x", "gamma", "beta", "y"]}, "gln_apply"),
    "pack_pw_weight": ("pack_pw_weight", case_pack, [(256, 256), (512, 256)], {"plain": ["weight", "packed"]}, "pack_pw_weights"),
    "pack3_pw_weight": ("pack3_pw_weight", lambda P, s, v: case_pack(P, s, v, True), [(256, 256), (512, 256)],
                        {"plain": ["weight", "packed"]}, "pack_pw_weights"),
    "pw_conv": ("pw_conv", case_pw_conv, [(3, 48, 160, 132), (2, 256, 512, 3200)],
                {"full": ["x", "weight", "bias", "residual", "out_sums", "y"] + _PRO4, "plain": []}, "pw_conv_bf16x3"),
    "pw_conv@mask": ("pw_conv", case_pw_conv, [(2, 64, 96, 260), (2, 256, 512, 3200)],
                     {"mask": ["x", "weight", "mask_mul", "y"]}, "pw_conv_bf16x3"),
    "pw_conv@packed": ("pw_conv", case_pw_conv, [(8, 256, 512, 3200)],
                       {"packed-full": ["x", "packed", "residual", "y"], "packed-plain": []}, "pw_conv_x3w"),
    "pw_conv3": ("pw_conv3", case_pw_conv3, [(3, 48, 160, 132), (16, 256, 256, 3200)],
                 {"full": ["x", "weight", "packed3", "bias", "residual", "y"] + _PRO4, "plain": ["out_sums"]}, "pw_conv_x3w4"),
    "pw_conv_pair": ("pw_conv_pair", case_pw_pair, [(24, 256, 384, 1604), (12, 512, 512, 3200)],
                     {"full": ["x", "packed1", "bias1", "residual", "packed2", "bias2", "out_sums2", "y", "y2"] + _PRO4,
                      "plain": []}, "pw_pair_x3f"),
    "pw_conv_pair3": ("pw_conv_pair3", lambda P, s, v: case_pw_pair(P, s, v, True), [(24, 256, 384, 1604), (12, 512, 512, 3200)],
                      {"full": ["x", "packed3_1", "bias1", "residual", "packed3_2", "bias2", "out_sums2", "y", "y2"] + _PRO4,
                       "plain": []}, "pw_pair_x3f4"),
    "dwconv5": ("dwconv5", case_dwconv5, [(2, 7, 202, 1), (2, 64, 3200, 2)],
                {"full": ["x", "weight", "bias", "out_sums", "y"] + _PRO4, "plain": []}, "dwconv5_s2_fast"),
    "dwconv5@s1": ("dwconv5", case_dwconv5, [(3, 20, 200, 2), (2, 64, 3200, 1)], {"full": ["x", "y"], "plain": []}, "dwconv5_s1_fast"),
    "conv1d": ("conv1d", case_conv1d, [(2, 6, 9, 77, 3, 2, 1, 2, 3), (2, 64, 64, 3200, 5, 1, 2, 1, 64)],
               {"full": ["x", "weight", "bias", "out_sums", "y"], "plain": []}, "conv1d"),
    "merge": ("merge", case_merge, [(2, 5, 808, 3), (2, 64, 3200, 5)],
              {"full": ["levels", "sums", "gammas", "betas", "out_sums", "y"], "plain": []}, "merge_fast"),
    "pyramid": ("pyramid", case_pyramid, [(2, 6, 3232, 5), (2, 64, 3200, 5)],
                {"full": ["y1", "weights", "biases", "gammas", "betas", "out_sums", "merged", "scratch"] + _PRO4, "plain": []},
                "pyramid"),
    "decoder": ("decoder", case_decoder, [(1, 96, 2, 21, 64, 633), (1, 1024, 2, 21, 320, 3200)],
                {"plain": ["v", "weight", "scratch", "out"]}, "pw_conv_bf16x3"),
    "tac": ("tac", case_tac, [(1, 3, 4, 40), (2, 16, 16, 300)], {"full": ["x4", "params", "out_sums", "q"], "plain": []}, "tac_mfma"),
    "mixture_consistency": ("mixture_consistency", case_mixture_consistency, [(3, 4, 1001), (2, 2, 32000)],
                            {"full": ["pr_batch", "input_mixture", "out", "work"], "plain": []}, "mixture_consistency"),
    "pw_wgrad": ("pw_wgrad", case_pw_wgrad, [(5, 48, 160, 132), (3, 256, 512, 3200)],
                 {"full": ["g", "x", "dw", "dbias", "scratch"] + _PRO4, "plain": ["dw", "dbias"]}, "pw_wgrad"),
    "gln_bwd": ("gln_bwd", case_gln_bwd, [(2, 20, 203), (3, 64, 3200)],
                {"full": ["gout", "x", "sums", "gamma", "beta", "prelu", "gout2", "gx", "dgamma", "dbeta", "dslope", "scratch"],
                 "plain": ["gx"]}, "gln_bwd_reduce"),
    "merge_bwd": ("merge_bwd", case_merge_bwd, [(3, 5, 64, 3), (2, 16, 3200, 5)], {"plain": ["g_merged", "levels"]}, "merge_bwd"),
    # depths beyond the one-pass kernel's instantiations (3..6) take the chain of pair sums, on the grid too
    "merge_bwd@deep": ("merge_bwd", case_merge_bwd, [(2, 2, 128, 7), (1, 3, 256, 8)], {"plain": ["g_merged"]}, "merge_bwd"),
    "dwconv5_bwd": ("dwconv5_bwd", case_dwconv5_bwd, [(3, 20, 200, 2), (2, 64, 3200, 1)],
                    {"full": ["gd", "xin", "weight", "dw", "dbias", "gin", "scratch"] + _PRO4, "plain": ["gin"]}, "dwconv5_bwd"),
    "mask_apply": ("mask_apply", case_mask_apply, [(1, 3, 5, 17), (2, 2, 24, 300)], {"plain": ["m", "enc", "v"]}, "mask_apply"),
    "mask_bwd": ("mask_bwd", case_mask_bwd, [(1, 3, 5, 17), (2, 2, 24, 300)],
                 {"full": ["gv", "m", "enc", "genc", "gm"], "plain": ["genc"]}, "mask_bwd"),
    "prelu_bwd": ("prelu_bwd", case_prelu_bwd, [(3, 40, 1001), (3, 40, 1000)],
                  {"full": ["gout", "x", "slope", "dslope", "gx"], "plain": ["dslope"]}, "prelu_bwd"),
    "frames_gather": ("frames_gather", case_frames_gather, [(1, 2, 330, 11, 68, None), (2, 2, 2100, 21, 100, 64)],
                      {"plain": ["src", "out"]}, "frames_gather"),
    "tac_bwd": ("tac_bwd", case_tac_bwd, [(1, 4, 8, 76), (2, 16, 16, 300)],
                {"plain": ["x", "go", "params", "grads", "gx", "scratch"]}, "tac_bwd_mfma"),
    "wav_normalize": ("wav_normalize", case_wav_normalize, [(1, 3, 77), (2, 2, 32000)], {"plain": ["wav", "out", "stats"]},
                      "wav_normalize"),
    "wav_denormalize": ("wav_denormalize", case_wav_denormalize, [(1, 3, 77), (2, 2, 32000)],
                        {"full": ["est", "stats", "mix_norm", "out"], "plain": []}, "wav_denormalize"),
    "causal_encoder": ("causal_encoder", case_causal_encoder, [(2, 2, 333, 16, 11, 70), (2, 1, 16000, 64, 21, 1600)],
                       {"plain": ["wav", "weight", "out"]}, "causal_encoder"),
    "causal_dwconv": ("causal_dwconv", case_causal_dwconv, [(2, 33, 101, 2), (2, 64, 2048, 2)],
                      {"full": ["x", "weight", "bias", "in_prelu", "out_prelu", "y"], "plain": []}, "causal_dwconv"),
    "causal_merge": ("causal_merge", case_causal_merge, [(1, 16, 176, 5), (3, 64, 2048, 4)], {"plain": ["levels", "y"]},
                     "causal_merge"),
    "causal_pyramid": ("causal_pyramid", case_causal_pyramid, [(2, 33, 3202, 2), (3, 64, 2048, 4)],
                       {"plain": ["y1", "in_prelu", "weights", "biases", "prelus", "merged"]}, "causal_pyramid"),
    "causal_stream_pyramid": ("causal_stream_pyramid", case_causal_stream_pyramid, [(1, 16, 176, 5), (3, 64, 2048, 4)],
                              {"plain": ["y1", "state", "in_prelu", "weights", "biases", "prelus", "merged"]}, "stream_pyramid"),
    "causal_scale": ("causal_scale", case_causal_scale, [(3, 5, 77), (2, 64, 3200)], {"full": ["src", "dscale", "dst"], "plain": []},
                     "causal_scale"),
    "prelu": ("prelu", case_prelu, [(3, 5, 77), (2, 64, 3200)], {"plain": ["x", "slope", "y"]}, "prelu_apply"),
}


def _params():
    out = []
    for key, (entry, _fn, shapes, variants, _fast) in CASES.items():
        ops_ = pl.PLACEMENT[entry]["operands"]
        for si in range(len(shapes)):
            for variant, singles in variants.items():
                runs = ["aligned"]
                for o in singles:
                    # a refusal is host code: one shape is enough for it (the first)
                    if ops_[o][0] == pl.FALLBACK or si == 0:
                        runs.append(o)
                runs.append("all")
                if singles and any(ops_[o][0] == pl.REFUSES for o in singles):
                    runs.append("all+refused")
                out += [pytest.param(key, si, variant, r, id="%s-%s-%s-%s" % (key, "ragged" if si == 0 and len(shapes) > 1 else "fast", variant, r))
                        for r in runs]
    return out


def _shifts(entry, run):
    """operand -> floats behind the 256-byte boundary for one run"""
    table = pl.PLACEMENT[entry]["operands"]
    if run == "aligned":
        return {}
    if run in ("all", "all+refused"):
        names = [o for o, (kind, _) in table.items() if kind == pl.FALLBACK or (kind == pl.REFUSES and run == "all+refused")]
        return {o: i % 3 + 1 for i, o in enumerate(names)}
    return {run: 1}


def _run_case(arena, key, si, variant, run, use_ramp=False):
    from sudo_rm_rf_amd import _lib
    entry, fn, shapes, variants, fast = CASES[key]
    table = pl.PLACEMENT[entry]["operands"]
    shifts = _shifts(entry, run)
    arena.reset()
    P = Placer(arena, shifts, use_ramp)
    refused = None
    try:
        fn(P, shapes[si], variant)
    except _lib.SrfError as e:
        refused = str(e)
    torch.cuda.synchronize()
    used = {o for o in shifts if o in P.placed}
    expect_refusal = [table[o][1] for o in used if table[o][0] == pl.REFUSES]
    if run not in ("aligned", "all", "all+refused") and run not in P.absent:
        assert run in P.placed, "operand %r is not part of this case: the parametrisation is out of date" % run
    if expect_refusal:
        assert refused is not None, "a misaligned %s must be refused on the host, the call went through" % sorted(used)
        assert "16-byte aligned" in refused and any(n in refused for n in expect_refusal), refused
        for name, view in P.made:                    # a refusal happens before any launch: nothing was written
            if name not in P.made.zeroed:
                arena.assert_untouched(view, name)
        for v in P.accum:
            assert float(v.double().abs().sum()) == 0.0, "an accumulator changed although the call was refused"
        arena.check()
        return P
    assert refused is None, "unexpected refusal: %s" % refused
    for name, view in P.made:
        if view.is_floating_point():
            if name not in _NOT_FULLY_WRITTEN:
                if name not in P.made.zeroed:
                    arena.assert_written(view, name)
                arena.assert_clean(view, name)
    for v in P.accum:
        arena.assert_clean(v)
    arena.check()
    for what, got, want, crit in P.checks:
        g = got.detach().double().cpu()
        assert not torch.isnan(g).any(), "%s: NaN in the result" % what
        crit(g, want.detach(), what)
    # the dispatch: the fast family on the grid (second shape), the family the table names off it
    if run == "aligned" and fast and si == len(shapes) - 1:
        assert any(n.startswith(fast) for n in P.trace), (fast, P.trace)
    if run in table and run not in P.absent and table[run][0] == pl.FALLBACK and table[run][1] != pl.SAME:
        families = table[run][1] if isinstance(table[run][1], tuple) else (table[run][1],)
        assert any(n.startswith(f) for n in P.trace for f in families), (run, families, P.trace)
        # ... and the grid-only family is gone, where the two have different names (gln_bwd's scalar kernels share theirs)
        if fast and entry != "gln_bwd" and not any(f.startswith(fast) or fast.startswith(f) for f in families):
            assert not any(n.startswith(fast) for n in P.trace), (run, P.trace)
    return P


@pytest.mark.parametrize("key,si,variant,run", _params())
def test_operand_placement(arena, key, si, variant, run):
    _run_case(arena, key, si, variant, run)


# (c) the ops that gather, on position-dependent data: key, shape index, variant
GATHERING = [("frames_gather", 1, "plain"), ("encoder", 0, "full"), ("decoder", 0, "plain"), ("merge", 0, "full"),
             ("merge_bwd", 1, "plain"), ("causal_dwconv", 0, "full"), ("dwconv5", 1, "full"), ("causal_encoder", 0, "plain")]


@pytest.mark.parametrize("run", ["aligned", "all"])
@pytest.mark.parametrize("key,si,variant", GATHERING, ids=[g[0] for g in GATHERING])
def test_gathering_ops_on_position_dependent_inputs(arena, key, si, variant, run):
    _run_case(arena, key, si, variant, run, use_ramp=True)


# =====================================================================================================================
# Whole-model, training, streaming and optimiser paths: poisoned workspaces, inputs as views (committed fixtures only)
# =====================================================================================================================
def _poison(t):
    t.view(-1).view(torch.uint8).fill_(pl.SENTINEL_BYTE)


def _view_at(host, shift_floats):
    """a device tensor equal to `host` that starts shift_floats floats into its allocation: a contiguous view, as
    buf[a:a + n].view(shape) of a longer signal is"""
    flat = torch.from_numpy(np.ascontiguousarray(host)).reshape(-1)
    buf = torch.full((flat.numel() + 8,), float("nan"), dtype=torch.float32, device=DEV)
    buf[shift_floats:shift_floats + flat.numel()] = flat.to(DEV)
    v = buf[shift_floats:shift_floats + flat.numel()].view(tuple(host.shape))
    assert v.is_contiguous() and v.data_ptr() % 16 == (4 * shift_floats) % 16
    return v


def _improved_or_groupcomm(manifest, name):
    from conftest import load_case
    import sudo_rm_rf.dnn.models.groupcomm_sudormrf_v2 as sudormrf_gc_v2
    import sudo_rm_rf.dnn.models.improved_sudormrf as improved_sudormrf
    cfg, sd, wav, gold = load_case(manifest, name)
    cls = improved_sudormrf.SuDORMRF if cfg.variant == "improved" else sudormrf_gc_v2.GroupCommSudoRmRf
    m = cls(**cfg.ctor_kwargs())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(DEV).eval(), wav, gold["out"]


def _causal(name):
    from sudo_rm_rf_amd.dnn.models.causal_improved_sudormrf_v3 import CausalSuDORMRF
    from tests import causal_fixtures as cf
    cfg, seed = cf.CASES[name][0], cf.CASES[name][3]
    torch.manual_seed(0)
    m = CausalSuDORMRF(**cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in cf.make_state_dict(cfg, seed).items()})
    return m.to(DEV).eval(), cf.make_input(name), cf.load_golden(name)["out"]


def _whole_model(manifest, name):
    return _causal(name) if name.startswith("causal") else _improved_or_groupcomm(manifest, name)


MODELS = ["tiny_improved", "tiny_groupcomm", "cfg1_improved_u8_pad", "causal_tiny", "causal_default"]


@pytest.mark.parametrize("name", MODELS)
def test_forward_does_not_depend_on_what_the_workspace_held(arena, manifest, name):
    """(d) forward, plan.workspace.fill_(0xFF), forward again: within test_run_to_run_determinism's 1e-6 of the first and
    within the golden bar (1e-4); then the explicit two-stream splits of test_two_stream_split_is_bit_identical, every plan's
    workspace poisoned before each."""
    model, wav, gold = _whole_model(manifest, name)
    x = torch.from_numpy(wav).to(DEV)
    eng = model._engine()
    eng.multi_stream = False
    with torch.no_grad():
        first = model(x).clone()
        for plan in list(eng._plans.values()):
            _poison(plan.workspace)
        second = model(x).clone()
        torch.cuda.synchronize()
        assert not torch.isnan(second).any()
        assert (first - second).abs().max().item() <= 1e-6
        assert np.abs(second.cpu().numpy() - gold).max() <= 1e-4
        batch = x.shape[0]
        params = [p.detach() for p in model.state_dict(keep_vars=True).values()]
        table = eng._param_table(params, x.device)
        eng.multi_stream = True
        for parts in [(batch,), (batch - batch // 2, batch // 2), (batch - batch // 3, batch // 3)]:
            parts = tuple(p for p in parts if p)
            out = torch.empty_like(first)
            _poison(out)
            eng._forward_split(parts, x, out, table)              # (creates the sub-batch plans on first use)
            torch.cuda.synchronize()
            for plan in list(eng._plans.values()):
                _poison(plan.workspace)
            _poison(out)
            eng._forward_split(parts, x, out, table)
            torch.cuda.synchronize()
            assert not torch.isnan(out).any(), parts
            assert (out - first).abs().max().item() <= 1e-6, parts
            assert np.abs(out.cpu().numpy() - gold).max() <= 1e-4, parts


@pytest.mark.parametrize("name", ["train_tiny_improved", "train_tiny_groupcomm"])
def test_training_step_with_poisoned_scratch(arena, name):
    """(e) include/sudormrf_hip.h: `saved` and `scratch` need no initialisation and `scratch` carries nothing from
    srf_forward_train to srf_backward (`saved` does): saved / scratch / the plan workspace hold 0xFF before the forward, scratch
    (and the workspace, which neither call takes) again between the two.  Bars: test_training_step_matches_reference_golden."""
    import sudo_rm_rf.dnn.experiments.utils.mixture_consistency as mixture_consistency
    import sudo_rm_rf.dnn.losses.sisdr as sisdr_lib
    from sudo_rm_rf_amd import engine as engine_mod
    from test_gpu_train import build
    from test_oracle_golden import check_grads_against_golden, train_case
    cfg, sd, mix, tgt, z = train_case(name)
    model = build(cfg, sd).train()
    eng = model._engine()
    plan = eng.plan_for(mix.shape[0], mix.shape[-1], torch.device(DEV))
    _poison(plan.train_scratch())
    _poison(plan.workspace)
    loss_fn = sisdr_lib.PITLossWrapper(sisdr_lib.PairwiseNegSDR("sisdr"), pit_from='pw_mtx')
    with pl.poisoned_allocations(engine_mod):                    # `saved` and the output are allocated by the forward
        rec = model(mix.to(DEV))
    assert eng.last_plan is plan
    _poison(plan.train_scratch())
    _poison(plan.workspace)
    if cfg.variant == "groupcomm":
        rec = mixture_consistency.apply(rec, mix.to(DEV))
    l = torch.clamp(loss_fn(rec, tgt.to(DEV)), min=-30., max=+30.)
    l.backward()
    assert abs(l.item() - float(z["loss"])) <= 1e-3
    check_grads_against_golden([(k, p.grad.cpu().numpy()) for k, p in model.state_dict(keep_vars=True).items()],
                               z, 2e-4, fp32_yardstick=0.0, flip_budget=0.0)


def _stream_views(s, x, sizes, poison_workspace):
    from tests.causal_stream_ref import schedule_chunks
    outs = []
    for a, b in schedule_chunks(x.shape[-1], sizes):
        if poison_workspace:
            _poison(s._workspace)
        chunk = x[..., a:b]
        assert chunk.is_contiguous()                             # batch 1, one channel: a slice is a view, never a copy
        outs.append(s.push(chunk))
    if poison_workspace:
        _poison(s._workspace)
    outs.append(s.finish())
    torch.cuda.synchronize()
    return torch.cat(outs, dim=-1).cpu().numpy()


@pytest.mark.parametrize("sched", ["g", "ragged"])
def test_streaming_from_views_and_with_a_poisoned_workspace_is_bit_identical(arena, sched):
    """(f) causal_tiny at batch 1: the signal lies 1, 2 and 3 floats into its allocation and is pushed as views; then the
    session's workspace is poisoned before every push.  Same samples, same bits.  _state and _weights
    carry state by contract and are left alone."""
    from test_gpu_causal_stream import RAGGED
    model, wav, _ = _causal("causal_tiny")
    wav = wav[:1]
    assert wav.shape[1] == 1
    with torch.no_grad():
        s = model.stream(batch=1)
        sizes = (s.granule,) if sched == "g" else RAGGED
        want = _stream_views(s, _view_at(wav, 0), sizes, False)
        assert not np.isnan(want).any()
        for shift in (1, 2, 3):
            s.reset()
            got = _stream_views(s, _view_at(wav, shift), sizes, False)
            assert np.array_equal(got, want), shift
        s.reset()
        got = _stream_views(s, _view_at(wav, 1), sizes, True)
        assert np.array_equal(got, want)


@pytest.mark.parametrize("name", ["tiny_improved", "tiny_groupcomm", "causal_tiny"])
def test_model_input_as_a_view_is_bit_identical(arena, manifest, name):
    """(g) model(wav) with wav = buf[1:1 + T].view(1, 1, T), and a batch-2 input two floats in, against the run on an aligned
    copy of the same samples."""
    model, wav, _ = _whole_model(manifest, name)
    model._engine().multi_stream = False
    with torch.no_grad():
        for host, shift in ((wav[:1], 1), (wav[:2], 2)):
            if host.shape[0] < (1 if shift == 1 else 2):
                host = np.concatenate([wav, wav[:, :, ::-1]], axis=0)[:2]
            want = model(_view_at(host, 0)).clone()
            got = model(_view_at(host, shift)).clone()
            torch.cuda.synchronize()
            assert not torch.isnan(want).any()
            assert torch.equal(got, want), (name, shift)


def test_fused_clip_adam_on_views_of_flat_buffers(arena):
    """(h) parameters and gradients are views into one flat buffer each (sizes 1, 3, 7, 129, 4096: most start off the
    16-byte grid), guards around both; three steps against clip_grad_norm_ + torch.optim.Adam at
    test_fused_clip_adam_matches_torch's tolerance."""
    from sudo_rm_rf_amd import optim
    sizes = [1, 3, 7, 129, 4096]
    total = sum(sizes)
    arena.reset()
    g = torch.Generator().manual_seed(7)
    flat_p = arena.put(torch.randn(total, generator=g, dtype=torch.float64), shift_floats=1, name="flat parameters")
    flat_g = arena.place((total,), shift_floats=3, name="flat gradients", zero=True)
    offs = np.cumsum([0] + sizes)
    pb = [flat_p[a:b].requires_grad_(True) for a, b in zip(offs[:-1], offs[1:])]
    assert sum(p.data_ptr() % 16 != 0 for p in pb) >= 3 and sum(flat_g[a:].data_ptr() % 16 != 0 for a in offs[:-1]) >= 3
    pa = [p.detach().clone().requires_grad_(True) for p in pb]
    ref = torch.optim.Adam(pa, lr=1e-3)
    fused = optim.FusedClipAdam(pb, lr=1e-3, clip_grad_norm=0.05)
    for it in range(3):
        flat_g.copy_(torch.randn(total, generator=g) * (0.1 + it))
        for p, q, a, b in zip(pa, pb, offs[:-1], offs[1:]):
            p.grad = flat_g[a:b].clone()
            q.grad = flat_g[a:b]
        want_norm = torch.nn.utils.clip_grad_norm_(pa, 0.05)
        ref.step()
        fused.step()
        assert abs(fused.last_grad_norm.item() - want_norm.item()) <= 1e-5 * want_norm.item()
        for p, q in zip(pa, pb):
            assert (p - q).abs().max().item() <= 2e-6, it
        arena.check()
    sa, sb = ref.state_dict()["state"], fused.state_dict()["state"]
    for k in sa:
        for name in ("exp_avg", "exp_avg_sq"):
            a, b = sa[k][name], sb[k][name]
            assert ((a - b).abs() <= 1e-7 + 1e-4 * a.abs()).all(), name


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_fuss_loss_metric_and_augmentation_in_the_arena(arena, shift):
    """The loss / metric / augmentation rows of PLACEMENT: test_zeroref_snr_rows_off_the_16_byte_grid's case (T % 4 == 0: on the
    grid the 16-byte-load kernels, off it the scalar ones) with every input, output, gradient and work buffer in the arena --
    same fp64 restatement, same bars; nothing outside a payload is written, nothing comes back unwritten."""
    import sudo_rm_rf.dnn.losses.sisdr as sisdr_lib
    import sudo_rm_rf.dnn.losses.snr as snr_lib
    from sudo_rm_rf_amd import augment
    from sudo_rm_rf_amd.dnn.losses import sisdr as sisdr_amd, snr as snr_amd
    from tests import fuss_fixtures as ff
    from test_gpu_fuss import _random_case
    B, S, T = 3, 4, 2048
    est_np, tgt_np = _random_case(B, S, T, 99)
    v64, i64, _, g64 = ff.zeroref_loss_and_grad(est_np, tgt_np)
    arena.reset()
    est = arena.put(torch.from_numpy(est_np), shift_floats=shift, name="est").requires_grad_()
    tgt = arena.put(torch.from_numpy(tgt_np), shift_floats=(shift * 2) % 4 if shift else 0, name="tgt")
    tgt2 = arena.put(torch.from_numpy(np.ascontiguousarray(tgt_np[:, :2])), shift_floats=shift, name="tgt (2 sources)")
    # (the wrappers' own buffers one double in: the work buffers hold doubles and are refused at 4 mod 8, as the header says)
    with arena.allocating(snr_amd, sisdr_amd, augment, shifts={"alloc%d" % i: 2 if shift else 0 for i in range(32)}) as made:
        ind = snr_lib.PermInvariantSNRwithZeroRefs(n_sources=S, backward_loss=False, return_individual_results=True)
        vals = ind(est, tgt)
        vals.sum().backward()
        fn = sisdr_lib.StabilizedPermInvSISDRMetric(zero_mean=True, n_estimated_sources=4, n_actual_sources=2, backward_loss=False,
                                                    improvement=True, return_individual_results=True)
        with torch.no_grad():
            got = fn(est.detach(), tgt2)
        src_b, src_s, gain = augment.fuss_draws(B, S)
        src, mix, _, _ = augment.fuss_augment_with_draws(tgt, src_b, src_s, gain)
    torch.cuda.synchronize()
    assert len(made) >= 8 and all(arena.owns(v) for _, v in made)
    arena.check()
    assert (np.abs(vals.detach().cpu().numpy() - v64) <= 2e-5 * np.maximum(1.0, np.abs(v64))).all()
    for name, view in made:              # (among them the gradient buffer the backward fills; autograd may hand on a copy)
        if view.dtype == torch.float32:
            arena.assert_written(view, name)
            arena.assert_clean(view, name)
    assert np.abs(est.grad.cpu().numpy() - g64).max() <= 2e-5 * np.abs(g64).max()
    want, _, _ = ff.stabilized_sisdr(torch.tensor(est_np), torch.tensor(tgt_np[:, :2]), improvement=True)
    ok = np.abs(want.numpy()) < 30
    assert (np.abs(got.cpu().numpy() - want.numpy())[ok] <= 2e-4 + 2e-5 * np.abs(want.numpy()[ok])).all()
    w_src, w_mix, _, _ = ff.augment(tgt_np, src_b.numpy(), src_s.numpy(), gain.numpy())
    assert arena.owns(src) and arena.owns(mix) and arena.unwritten(src) == 0 and arena.unwritten(mix) == 0
    assert np.array_equal(src.cpu().numpy(), w_src.numpy()) and np.abs(mix.cpu().numpy() - w_mix.numpy()).max() <= 2e-5
