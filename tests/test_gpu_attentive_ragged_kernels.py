"""The seven ragged kernels of the attentive block against fp64 torch restatements on each example's own
slice: values (1e-4 max-abs, the project's bar for forward outputs), exact zeros past the end, NaN past every length changing
nothing, equal bits on a second run, a row's bits unchanged when the other rows change in content and length, lengths all equal
to the stride agreeing with the uniform twin -- and every entry off the 16-byte grid between guard bands.
Worst errors measured on an MI355X: profiles/attentive_block_ragged.txt."""
import pytest
import torch
import torch.nn.functional as F

from tests import attentive_ref as ar
from tests.placement import Arena

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR = 1e-4


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _rand(g, *shape, scale=1.0, shift=0.0):
    return torch.randn(*shape, generator=g, dtype=torch.float32) * scale + shift


def _own_sums(x, lengths):
    """own-column {sum, sumsq} of x [Bt, C, L] (host fp32 tensor) as a device statistics tensor: everything in bucket 0"""
    s = torch.zeros(x.shape[0], 64, 2, dtype=torch.float64)
    for b, n in enumerate(lengths):
        own = x[b, :, :n].double()
        s[b, 0, 0], s[b, 0, 1] = own.sum(), (own * own).sum()
    return s.to(DEV)


def _nan_tail(x, lengths):
    x = x.clone()
    for b, n in enumerate(lengths):
        x[b, :, n:] = float("nan")
    return x


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _check_rows(what, got, want, lengths):
    """got [Bt, C, L] device; want: per example an fp64 [C, n_b] tensor.  -> worst error; zeros past the end are exact"""
    got = got.cpu()
    worst = 0.0
    for b, n in enumerate(lengths):
        assert want[b].shape[-1] == n
        err = (got[b, :, :n].double() - want[b]).abs().max().item()
        worst = max(worst, err)
        assert err <= BAR, "%s: example %d: max-abs error %.3g" % (what, b, err)
        tail = got[b, :, n:]
        assert tail.numel() == 0 or (_bits(tail) == 0).all(), "%s: example %d is not exact +0 past its end" % (what, b)
    print("  %s: worst max-abs error %.3g" % (what, worst))
    return worst


def _check_sums(what, sums, stored, lengths):
    """sums [Bt, 64, 2] against the fp64 sums of the STORED rows.  The float4 kernels add the four outputs of a lane (and their
    squares) in fp32 before the fp64 accumulation, as their uniform twins do: at most four fp32 roundings per group, each at most
    2^-24 of the group's sum of magnitudes -- so the total may be off by 2^-22 * sum |v| (resp. sum v^2); the rest is fp64."""
    tot = sums.sum(1).cpu()
    for b, n in enumerate(lengths):
        own = stored[b, :, :n].double().cpu()
        for i, (w, mag) in enumerate(((own.sum().item(), own.abs().sum().item()), ((own * own).sum().item(),) * 2)):
            assert abs(tot[b, i].item() - w) <= 2.0 ** -22 * mag + 1e-9, (what, b, i, tot[b, i].item(), w)


def _properties(what, run, inputs, lengths, others):
    """run(inputs, lengths) -> output [Bt, C, L'] (own columns of example b: out_len(b)).  NaN past every length, a second
    run, and the other rows changed in content and length (others = (inputs', lengths') with example 1 kept)."""
    y = run(inputs, lengths)
    y2 = run(inputs, lengths)
    assert torch.equal(_bits(y), _bits(y2)), "%s: two runs differ" % what
    y3 = run([(_nan_tail(t, ln), ln) for t, ln in inputs], lengths)
    assert torch.equal(_bits(y), _bits(y3)), "%s: NaN past the lengths changed the output" % what
    o_inputs, o_lengths = others
    y4 = run(o_inputs, o_lengths)
    assert torch.equal(_bits(y[1]), _bits(y4[1])), "%s: example 1 changed with the other rows" % what
    return y


# ---- srf_dwconv5_ragged ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride,L,lengths,kernel", [
    (1, 24, [24, 10, 2], "dwconv5_generic_ragged"), (2, 24, [24, 10, 2], "dwconv5_generic_ragged"),
    (1, 24, [24, 8, 16], "dwconv5_s1_fast_ragged"), (2, 24, [24, 8, 16], "dwconv5_s2_fast_ragged"),
    (1, 520, [520, 258, 2], "dwconv5_generic_ragged"), (1, 520, [520, 264, 8], "dwconv5_s1_fast_ragged"),
    (2, 528, [528, 264, 8], "dwconv5_s2_fast_ragged")])
def test_dwconv5_ragged(stride, L, lengths, kernel):
    from sudo_rm_rf_amd import ops, ragged
    g = _g(100 * stride + L + lengths[1])
    Bt, Cc = 3, 5
    w, bias = _rand(g, Cc, 1, 5, scale=0.5), _rand(g, Cc, scale=0.2)
    gamma, beta, slope = _rand(g, Cc, scale=0.2, shift=1.0), _rand(g, Cc, scale=0.2), torch.tensor([0.25])
    dv = lambda t: t.to(DEV)

    def make(seed, lens):
        return [(_rand(_g(seed), Bt, Cc, L, scale=2.0, shift=0.5), lens)]

    def run(inputs, lens):
        x = inputs[0][0]
        osums = ops.new_sums(Bt, DEV)
        with ops.kernel_trace(DEV) as tr:
            y = ragged.dwconv5(dv(x), dv(w), dv(bias), stride, lens, _own_sums(x, lens), dv(gamma), dv(beta), dv(slope), out_sums=osums)
        run.names, run.sums = [n for n, _ in tr.launches], osums
        return y

    inputs = make(1, lengths)
    keep = inputs[0][0][1].clone()
    other_len = [lengths[2], lengths[1], lengths[0] - (2 if kernel.endswith("generic_ragged") else 0)]
    others = make(2, other_len)
    others[0][0][1] = keep
    y = _properties("dwconv5_ragged s%d" % stride, run, inputs, lengths, (others, other_len))
    y = run(inputs, lengths)
    assert run.names == [kernel], run.names
    x = inputs[0][0].double()
    out_len = [n // stride for n in lengths]
    want = []
    for b, n in enumerate(lengths):
        a = ar.prelu(ar.gln(x[b:b + 1, :, :n], gamma.double(), beta.double()), slope.double())
        want.append(F.conv1d(a, w.double(), bias.double(), stride=stride, padding=2, groups=Cc)[0])
    _check_rows("dwconv5_ragged s%d %s %s" % (stride, lengths, kernel), y, want, out_len)
    _check_sums("dwconv5_ragged", run.sums, y, out_len)
    # lengths all equal to the stride: the uniform twin
    full = [L] * Bt
    yu = ops.dwconv5(dv(inputs[0][0]), dv(w), dv(bias), stride, _own_sums(inputs[0][0], full), dv(gamma), dv(beta), dv(slope))
    assert (run(inputs, full) - yu).abs().max().item() <= BAR


# ---- srf_merge_ragged -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,L,lengths,kernel", [(2, 10, [6, 2, 10], "merge_generic_ragged"), (3, 20, [12, 4, 20], "merge_fast_ragged"),
                                                (3, 24, [8, 16, 24], "merge_fast_ragged"),
                                                (2, 1032, [1032, 1026, 2], "merge_generic_ragged")])
def test_merge_ragged(D, L, lengths, kernel):
    from sudo_rm_rf_amd import ops, ragged
    g = _g(10 * D + L)
    Bt, Cc = 3, 3
    gammas = [_rand(g, Cc, scale=0.2, shift=1.0) for _ in range(D)]
    betas = [_rand(g, Cc, scale=0.2) for _ in range(D)]
    dv = lambda t: t.to(DEV)

    def make(seed, lens):
        gg = _g(seed)
        return [(_rand(gg, Bt, Cc, L >> k, scale=1.5, shift=0.3), [n >> k for n in lens]) for k in range(D)]

    def run(inputs, lens):
        osums = ops.new_sums(Bt, DEV)
        with ops.kernel_trace(DEV) as tr:
            y = ragged.merge([dv(t) for t, _ in inputs], [_own_sums(t, [n >> k for n in lens]) for k, (t, _) in enumerate(inputs)], [dv(t) for t in gammas],
                             [dv(t) for t in betas], lens, out_sums=osums)
        run.names, run.sums = [n for n, _ in tr.launches], osums
        return y

    inputs = make(1, lengths)
    other_len = [lengths[2], lengths[1], lengths[0]]
    others = make(2, other_len)
    for k in range(D):
        others[k][0][1] = inputs[k][0][1]
    _properties("merge_ragged D%d" % D, run, inputs, lengths, (others, other_len))
    y = run(inputs, lengths)
    assert run.names == [kernel], run.names
    want = []
    for b, n in enumerate(lengths):
        t = 0
        for k in range(D):
            lv = ar.gln(inputs[k][0][b:b + 1, :, :n >> k].double(), gammas[k].double(), betas[k].double())
            t = t + lv.repeat_interleave(1 << k, dim=-1)
        want.append(t[0])
    _check_rows("merge_ragged D%d %s %s" % (D, lengths, kernel), y, want, lengths)
    _check_sums("merge_ragged", run.sums, y, lengths)
    full = [L] * Bt
    yu = ops.merge([dv(t) for t, _ in inputs], [_own_sums(t, [L >> k] * Bt) for k, (t, _) in enumerate(inputs)],
                   [dv(t) for t in gammas], [dv(t) for t in betas])
    assert (run(inputs, full) - yu).abs().max().item() <= BAR


# ---- srf_posenc_apply_ragged ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lazy", [False, True])
def test_posenc_apply_ragged(lazy):
    from sudo_rm_rf_amd import attention, ops
    g = _g(7 + lazy)
    Bt, Cc, L, lengths = 3, 37, 40, [35, 13, 1]
    pe = _rand(g, 50, Cc, scale=0.7)
    pe[max(lengths):] = float("nan")                       # rows past the longest length are never read
    gamma, beta = _rand(g, Cc, scale=0.2, shift=1.0), _rand(g, Cc, scale=0.2)
    dv = lambda t: t.to(DEV)

    def run(inputs, lens):
        a = inputs[0][0]
        norm = (_own_sums(a, lens), dv(gamma), dv(beta)) if lazy else ()
        with ops.kernel_trace(DEV) as tr:
            x = attention.posenc_apply(dv(a), dv(pe), *norm, lengths=lens)
        run.names = [n for n, _ in tr.launches]
        return x

    inputs = [(_rand(g, Bt, Cc, L, scale=2.0, shift=0.4), lengths)]
    other_len = [1, 13, 35]
    others = [(_rand(_g(99), Bt, Cc, L), other_len)]
    others[0][0][1] = inputs[0][0][1]
    x = _properties("posenc_apply_ragged", run, inputs, lengths, (others, other_len))
    assert run.names == ["posenc_apply_ragged"]
    want = []
    for b, n in enumerate(lengths):
        a = inputs[0][0][b:b + 1, :, :n].double()
        a = ar.gln(a, gamma.double(), beta.double()) if lazy else a
        want.append((a + pe[:n].double().t()[None])[0])
    _check_rows("posenc_apply_ragged lazy=%d" % lazy, x, want, lengths)
    full = [30] * Bt                                       # (a stride whose every pe row is finite)
    a30 = inputs[0][0][:, :, :30].contiguous()
    norm = (_own_sums(a30, full), dv(gamma), dv(beta)) if lazy else ()
    xu = attention.posenc_apply(dv(a30), dv(pe), *norm)
    assert (attention.posenc_apply(dv(a30), dv(pe), *norm, lengths=full) - xu).abs().max().item() <= BAR


# ---- srf_gln_apply2_add_ragged, srf_gln_apply_ragged ----------------------------------------------------------------------------
@pytest.mark.parametrize("Cc,L,lengths", [(5, 26, [26, 13, 1]), (2, 1030, [1030, 1025, 3])])
def test_gln_apply2_add_and_gln_apply_ragged(Cc, L, lengths):
    from sudo_rm_rf_amd import attention, ops, ragged
    g = _g(Cc + L)
    Bt = 3
    gf, bf, gy, by = (_rand(g, Cc, scale=0.2, shift=s) for s in (1.0, 0.0, 1.0, 0.0))
    slope = torch.tensor([0.25])
    dv = lambda t: t.to(DEV)

    def make(seed, lens):
        gg = _g(seed)
        return [(_rand(gg, Bt, Cc, L, scale=2.0, shift=0.5), lens), (_rand(gg, Bt, Cc, L, scale=0.7, shift=-0.2), lens)]

    def run2(inputs, lens):
        (f, _), (y, _) = inputs
        osums = ops.new_sums(Bt, DEV)
        with ops.kernel_trace(DEV) as tr:
            z = attention.gln_apply2_add(dv(f), _own_sums(f, lens), dv(gf), dv(bf), dv(slope), dv(y), _own_sums(y, lens), dv(gy), dv(by),
                                         out_sums=osums, lengths=lens)
        run2.names, run2.sums = [n for n, _ in tr.launches], osums
        return z

    def run1(inputs, lens):
        f = inputs[0][0]
        with ops.kernel_trace(DEV) as tr:
            z = ragged.gln_apply(dv(f), _own_sums(f, lens), dv(gf), dv(bf), lens, prelu=dv(slope))
        run1.names = [n for n, _ in tr.launches]
        return z

    inputs = make(1, lengths)
    other_len = [lengths[2], lengths[1], lengths[0]]
    others = make(2, other_len)
    for i in range(2):
        others[i][0][1] = inputs[i][0][1]
    z2 = _properties("gln_apply2_add_ragged", run2, inputs, lengths, (others, other_len))
    z1 = _properties("gln_apply_ragged", run1, inputs, lengths, (others, other_len))
    assert run2.names == ["gln_apply2_add_ragged"] and run1.names == ["gln_apply_ragged"]
    want2, want1 = [], []
    for b, n in enumerate(lengths):
        f, y = (t[b:b + 1, :, :n].double() for t, _ in inputs)
        nf = ar.prelu(ar.gln(f, gf.double(), bf.double()), slope.double())
        want1.append(nf[0])
        want2.append((nf + ar.gln(y, gy.double(), by.double()))[0])
    _check_rows("gln_apply2_add_ragged %s" % lengths, z2, want2, lengths)
    _check_rows("gln_apply_ragged %s" % lengths, z1, want1, lengths)
    run2(inputs, lengths)
    _check_sums("gln_apply2_add_ragged", run2.sums, z2, lengths)
    full = [L] * Bt
    (f, _), (y, _) = inputs
    zu = attention.gln_apply2_add(dv(f), _own_sums(f, full), dv(gf), dv(bf), dv(slope), dv(y), _own_sums(y, full), dv(gy), dv(by))
    assert (run2(inputs, full) - zu).abs().max().item() <= BAR
    yu = ops.gln_apply(dv(f), _own_sums(f, full), dv(gf), dv(bf), dv(slope))
    assert (run1(inputs, full) - yu).abs().max().item() <= BAR


# ---- srf_gln_stats_ragged, srf_sums_scale_ragged --------------------------------------------------------------------------------
def test_gln_stats_ragged_and_sums_scale_ragged():
    from sudo_rm_rf_amd import ops, ragged
    g = _g(26)
    Bt, Cc, L, lengths = 3, 70, 26, [26, 13, 1]
    x = _rand(g, Bt, Cc, L, scale=2.0, shift=0.7)
    with ops.kernel_trace(DEV) as tr:
        s = ragged.gln_stats(x.to(DEV), lengths)
        sc = ragged.sums_scale(s, L, lengths)
    assert [n for n, _ in tr.launches] == ["gln_stats_ragged", "sums_scale_ragged"]
    assert torch.equal(s, ragged.gln_stats(x.to(DEV), lengths))                     # a fixed order: the same bits
    assert torch.equal(s, ragged.gln_stats(_nan_tail(x, lengths).to(DEV), lengths))
    other = _rand(_g(5), Bt, Cc, L)
    other[1] = x[1]
    assert torch.equal(s[1], ragged.gln_stats(other.to(DEV), [1, 13, 26])[1])        # ... whatever the other groups hold
    sh = s.cpu()
    for b, n in enumerate(lengths):
        own = x[b, :, :n].double()
        for k in range(64):                                                         # bucket k: the rows k mod 64
            rows = own[k::64]
            for i, w in enumerate((rows.sum().item(), (rows * rows).sum().item())):
                assert abs(sh[b, k, i].item() - w) <= 1e-12 * max(1.0, abs(w)), (b, k, i)
        assert torch.equal(sc[b].cpu(), sh[b] * (float(L) / float(n)))              # one IEEE multiply by one IEEE quotient
    # the uniform twin at full lengths: the same totals
    su = ops.gln_stats(x.to(DEV), Bt).sum(1).cpu()
    sf = ragged.gln_stats(x.to(DEV), [L] * Bt).sum(1).cpu()
    assert ((su - sf).abs() <= 1e-9 * su.abs().clamp(min=1.0)).all()


# ---- every new entry off the 16-byte grid, between guard bands ------------------------------------------------------------------
def test_every_new_entry_off_the_16_byte_grid_between_guard_bands():
    from sudo_rm_rf_amd import attention, ops, ragged
    g = _g(77)
    Bt, Cc, L, lengths = 3, 6, 24, [24, 12, 4]
    arena = Arena(DEV, 1 << 20)
    gamma, beta, slope = _rand(g, Cc, scale=0.2, shift=1.0), _rand(g, Cc, scale=0.2), torch.tensor([0.25])
    x, y2 = _rand(g, Bt, Cc, L, scale=2.0), _rand(g, Bt, Cc, L)
    lv1 = _rand(g, Bt, Cc, L // 2)
    w, bias = _rand(g, Cc, 1, 5, scale=0.5), _rand(g, Cc, scale=0.2)
    pe = _rand(g, 30, Cc)

    def case(what, fn):
        """fn(put) -> output; put(tensor) places an input one float off the grid; the wrapper's allocations are three floats off"""
        arena.reset()
        put = lambda t, shift=1: arena.put(t, t.dtype, shift)
        with arena.allocating(ragged, attention, shifts={"alloc%d" % i: 3 for i in range(4)}) as made:
            with ops.kernel_trace(DEV) as tr:
                out = fn(put)
        torch.cuda.synchronize()
        assert all(n.endswith("_ragged") for n, _ in tr.launches) and len(tr.launches) == 1, (what, tr.launches)
        arena.check()
        assert arena.owns(out) and out.data_ptr() % 16 != 0, what
        arena.assert_written(out, what)
        arena.assert_clean(out, what)
        return out.clone()

    sums = lambda t, ln: put_sums(_own_sums(t, ln))
    put_sums = lambda s: arena.put(s, torch.float64, 0)          # (statistics are read as pairs of doubles: 16-byte aligned)
    for stride in (1, 2):
        got = case("dwconv5 s%d" % stride, lambda put: ragged.dwconv5(put(x), put(w), put(bias), stride, lengths, sums(x, lengths),
                                                                      put(gamma), put(beta), put(slope)))
        want = ragged.dwconv5(x.to(DEV), w.to(DEV), bias.to(DEV), stride, lengths, _own_sums(x, lengths), gamma.to(DEV), beta.to(DEV),
                              slope.to(DEV))
        assert (got - want).abs().max().item() <= BAR          # (the aligned call may take the float4 kernel)
    half = [n // 2 for n in lengths]
    got = case("merge", lambda put: ragged.merge([put(x), put(lv1)], [sums(x, lengths), sums(lv1, half)], [put(gamma), put(gamma)],
                                                 [put(beta), put(beta)], lengths))
    want = ragged.merge([x.to(DEV), lv1.to(DEV)], [_own_sums(x, lengths), _own_sums(lv1, half)], [gamma.to(DEV)] * 2, [beta.to(DEV)] * 2,
                        lengths)
    assert (got - want).abs().max().item() <= BAR              # (the aligned call takes the float4 kernel)
    got = case("posenc", lambda put: attention.posenc_apply(put(x), put(pe), sums(x, lengths), put(gamma), put(beta), lengths=lengths))
    assert torch.equal(_bits(got), _bits(attention.posenc_apply(x.to(DEV), pe.to(DEV), _own_sums(x, lengths), gamma.to(DEV), beta.to(DEV),
                                                                lengths=lengths)))
    got = case("apply2_add", lambda put: attention.gln_apply2_add(put(x), sums(x, lengths), put(gamma), put(beta), put(slope), put(y2),
                                                                  sums(y2, lengths), put(gamma), put(beta), lengths=lengths))
    assert torch.equal(_bits(got), _bits(attention.gln_apply2_add(x.to(DEV), _own_sums(x, lengths), gamma.to(DEV), beta.to(DEV),
                                                                  slope.to(DEV), y2.to(DEV), _own_sums(y2, lengths), gamma.to(DEV),
                                                                  beta.to(DEV), lengths=lengths)))
    got = case("gln_apply", lambda put: ragged.gln_apply(put(x), sums(x, lengths), put(gamma), put(beta), lengths))
    assert torch.equal(_bits(got), _bits(ragged.gln_apply(x.to(DEV), _own_sums(x, lengths), gamma.to(DEV), beta.to(DEV), lengths)))
    got = case("gln_stats", lambda put: ragged.gln_stats(put(x), lengths))
    want = ragged.gln_stats(x.to(DEV), lengths)
    assert torch.equal(got, want)
    got = case("sums_scale", lambda put: ragged.sums_scale(arena.put(want, torch.float64, 2), L, lengths))
    assert torch.equal(got, ragged.sums_scale(want, L, lengths))
