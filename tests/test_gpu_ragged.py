"""Ragged forms on the GPU, one test per form: every example of the batch must come out as its own batch-1 call computes it.

References are fp64 restatements written here, evaluated per example on the example's own length.  The bar of each form is
the one tests/test_gpu_ops.py holds its uniform twin to -- the arithmetic is the same.  Every output (and the scratch) is
allocated pre-filled with 0xFF bytes (tests/placement.py), so "exactly zero past the end" proves the kernel wrote it.

Then the whole model (second half of the file): cfg 2 weights, batch 32, rows of unequal length in ONE call
(SuDORMRF.forward_ragged / srf_forward_ragged), every row against oracle.torch_oracle.forward of that row ALONE at its own
length -- the reference shares no code with the library -- and pipeline.separate_list against pipeline.separate per utterance."""
import pytest
import torch
import torch.nn.functional as F

import numpy as np

from conftest import load_case
from oracle import torch_oracle, weights
from oracle.schema import ModelConfig
from test_gpu_batch_distinct import per_example_error, report
from test_gpu_model import TOL, build
from tests.placement import poisoned_allocations
from tests.test_gpu_ops import DEV, check, check_sums, dev32, gln64, rnd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    from sudo_rm_rf_amd import _lib, ops
    _lib.load()
    ops.set_kernel_mode(0)


def _sums64_valid(x, frames):
    """exact fp64 {sum, sumsq} of x[g, :, :frames[g]] in the bucketed layout [groups, 64, 2] (bucket 0)."""
    out = torch.zeros(x.shape[0], 64, 2, dtype=torch.float64)
    for g, n in enumerate(frames):
        v = x[g, :, :n]
        out[g, 0, 0], out[g, 0, 1] = v.sum(), (v * v).sum()
    return out


def _check_rows(got, want_rows, frames, atol, what):
    """valid columns against the per-example reference, everything from the example's end to the row stride exactly 0"""
    got = got.detach().cpu()
    assert torch.isfinite(got).all(), what
    for g, n in enumerate(frames):
        check(got[g, :, :n], want_rows[g], atol, "%s example %d (%d frames)" % (what, g, n))
        assert (got[g, :, n:] == 0).all(), "%s example %d: not exactly zero past frame %d" % (what, g, n)


def _check_sums_rows(sums, want_rows, what):
    for g, w in enumerate(want_rows):
        check_sums(sums[g:g + 1], w.unsqueeze(0), "%s example %d" % (what, g))


# ---- encoder: K = 21, h = 10, D = 4 -> 160-sample / 16-frame steps; row stride L = 400 (3 full 128-frame blocks + 16) ----------
ENC_T, ENC_L, ENC_N = 4000, 400, 40
# (samples, frames): full | on a 128-frame block edge, the length ending ON the hop grid (frame 256 would see the last 10
# samples) | one 16-frame step past the edge | one step short of full | the shortest (one step) | a lone sample
ENC_CASES = [(4000, 400), (2560, 256), (2713, 272), (3833, 384), (160, 16), (1, 16)]


def test_encoder_ragged():
    from sudo_rm_rf_amd import ops, ragged
    Bt = len(ENC_CASES)
    lens, frames = [c[0] for c in ENC_CASES], [c[1] for c in ENC_CASES]
    assert frames == [ragged.padded_frames(n, 21, 4) for n in lens]
    x, w = rnd(Bt, 1, ENC_T, seed=1), rnd(ENC_N, 1, 21, seed=2, scale=0.3)
    want = []
    for b in range(Bt):
        xp = torch.zeros(1, 1, frames[b] * 10, dtype=torch.float64)
        xp[..., :lens[b]] = x[b, :, :lens[b]]
        want.append(F.conv1d(xp, w, None, stride=10, padding=10)[0])
        assert want[-1].shape == (ENC_N, frames[b])
    sums = ops.new_sums(Bt, DEV)
    with poisoned_allocations(ragged), ops.kernel_trace(DEV) as tr:
        got = ragged.encoder(dev32(x), dev32(w), ENC_L, lens, frames, sums)
    assert [n for n, _ in tr.launches] == ["encoder_ragged"]
    _check_rows(got, want, frames, 2e-5, "encoder_ragged")
    _check_sums_rows(sums, want, "encoder_ragged sums")
    # the input past every example's end is never interpreted
    xn = x.clone()
    for b in range(Bt):
        xn[b, :, lens[b]:] = float("nan")
    sums2 = ops.new_sums(Bt, DEV)
    with poisoned_allocations(ragged):
        got2 = ragged.encoder(dev32(xn), dev32(w), ENC_L, lens, frames, sums2)
    assert torch.equal(got2, got), "encoder_ragged: the result depends on samples past an example's end"
    _check_sums_rows(sums2, want, "encoder_ragged sums (NaN tail)")


def test_encoder_ragged_equal_lengths_is_the_uniform_encoder():
    from sudo_rm_rf_amd import ops, ragged
    x, w = dev32(rnd(3, 1, ENC_T, seed=3)), dev32(rnd(ENC_N, 1, 21, seed=4, scale=0.3))
    assert torch.equal(ragged.encoder(x, w, ENC_L, [ENC_T] * 3, [ENC_L] * 3), ops.encoder(x, w, ENC_L))


# ---- pyramid ------------------------------------------------------------------------------------------------------------
# (C, D, row stride L, frames per example).  A wavefront of the register kernels owns up to 60 chunks of 16 (32) frames:
#   D = 4: L = 1200 = 75 chunks -> 2 tiles of 38, boundary at frame 608.  full | one 16-frame step short | on a 128-frame edge |
#          one step past it | the shortest the predicate takes | on the kernels' own tile boundary | one step past that
#   D = 6: chunks of 32, steps of 64; L = 2240 = 70 chunks -> 2 tiles of 35, boundary at frame 1120
PYR_CASES = [(20, 4, 1200, [1200, 1184, 256, 272, 64, 608, 624]),
             (6, 6, 2240, [2240, 2176, 1152, 1216, 256, 1120, 1184]),
             (5, 1, 96, [96, 64, 80])]


def _pyramid_ref(y1, g_in, b_in, slope, W, Bi, Ga, Be):
    """improved_sudormrf.py:206-216 in fp64 on ONE example [1, C, n]; returns merged [C, n]"""
    C_ = y1.shape[1]
    cur = gln64(y1, g_in, b_in)
    cur = torch.where(cur >= 0, cur, slope * cur)
    outs = []
    for k in range(len(W)):
        d = F.conv1d(cur, W[k], Bi[k], stride=1 if k == 0 else 2, padding=2, groups=C_)
        cur = gln64(d, Ga[k], Be[k])
        outs.append(cur)
    u = outs[-1]
    for k in range(len(W) - 2, -1, -1):
        u = outs[k] + u.repeat_interleave(2, dim=-1)
    return u[0]


@pytest.mark.parametrize("C_,D,L,frames", PYR_CASES, ids=["D4", "D6", "D1"])
def test_pyramid_ragged(C_, D, L, frames):
    from sudo_rm_rf_amd import ops, ragged
    groups = len(frames)
    assert all(ragged.frames_ok(n, L, D) for n in frames)
    y1 = rnd(groups, C_, L, seed=100, scale=1.4, shift=0.2)           # (past an example's end: garbage of the same kind)
    g_in, b_in = rnd(C_, seed=101, scale=0.3, shift=1.0), rnd(C_, seed=102, scale=0.3)
    slope = torch.tensor([0.23], dtype=torch.float64)
    W = [rnd(C_, 1, 5, seed=110 + k, scale=0.5) for k in range(D)]
    Bi = [rnd(C_, seed=120 + k, scale=0.2) for k in range(D)]
    Ga = [rnd(C_, seed=130 + k, scale=0.3, shift=1.0) for k in range(D)]
    Be = [rnd(C_, seed=140 + k, scale=0.3) for k in range(D)]
    want = [_pyramid_ref(y1[g:g + 1, :, :n], g_in, b_in, slope, W, Bi, Ga, Be) for g, n in enumerate(frames)]
    in_sums = _sums64_valid(y1, frames).to(DEV)
    dl = lambda ts: [dev32(t) for t in ts]

    def run(y):
        osums = ops.new_sums(groups, DEV)
        with poisoned_allocations(ragged), ops.kernel_trace(DEV) as tr:
            got = ragged.pyramid(dev32(y), in_sums, dev32(g_in), dev32(b_in), dev32(slope), dl(W), dl(Bi), dl(Ga), dl(Be),
                                 frames, out_sums=osums)
        assert [n for n, _ in tr.launches] == ["pyramid_moments_ragged", "pyramid_finalize_ragged", "pyramid_merge_ragged"]
        return got, osums

    got, osums = run(y1)
    _check_rows(got, want, frames, 5e-5, "pyramid_ragged")
    _check_sums_rows(osums, want, "pyramid_ragged sums")
    # y1 past every example's end is never interpreted
    yn = y1.clone()
    for g, n in enumerate(frames):
        yn[g, :, n:] = float("nan")
    got2, osums2 = run(yn)
    assert torch.equal(got2, got), "pyramid_ragged: the result depends on y1 past an example's end"
    _check_sums_rows(osums2, want, "pyramid_ragged sums (NaN tail)")


def test_pyramid_ragged_equal_lengths_is_the_uniform_pyramid():
    from sudo_rm_rf_amd import ops, ragged
    C_, D, L, groups = 20, 4, 1200, 3
    y1 = rnd(groups, C_, L, seed=100, scale=1.4, shift=0.2)
    in_sums = _sums64_valid(y1, [L] * groups).to(DEV)
    par = [dev32(rnd(C_, seed=101, scale=0.3, shift=1.0)), dev32(rnd(C_, seed=102, scale=0.3)), dev32(torch.tensor([0.23]))]
    lv = [[dev32(rnd(C_, 1, 5, seed=110 + k, scale=0.5)) for k in range(D)], [dev32(rnd(C_, seed=120 + k, scale=0.2)) for k in range(D)],
          [dev32(rnd(C_, seed=130 + k, scale=0.3, shift=1.0)) for k in range(D)], [dev32(rnd(C_, seed=140 + k, scale=0.3)) for k in range(D)]]
    a = ragged.pyramid(dev32(y1), in_sums, *par, *lv, [L] * groups)
    b = ops.pyramid(dev32(y1), in_sums, *par, *lv)
    assert torch.equal(a, b)


# ---- 1x1 convolutions: row stride 400 = 3 tiles of 128 columns + 16; steps of 16 frames (D = 4) ----------------------------------
# full | on a tile edge | one step past it | one step short of full | the shortest (one step)
PW_L, PW_FRAMES = 400, [400, 256, 272, 384, 16]


def _nan_tail(x, frames):
    xn = x.clone()
    for b, n in enumerate(frames):
        xn[b, :, n:] = float("nan")
    return xn


def _pro_ref(x, frames, pro, gamma, beta, slope):
    """the prologue in fp64, per example over its own columns: list of [1, Cin, frames[b]]"""
    rows = []
    for b, n in enumerate(frames):
        v = x[b:b + 1, :, :n].double()
        if pro in (1, 2):
            v = gln64(v, gamma, beta)
        if pro == 2:
            v = torch.where(v >= 0, v, slope * v)
        rows.append(v)
    return rows


@pytest.mark.parametrize("pro", [0, 1, 2], ids=["plain", "gln", "gln-prelu-residual"])
def test_pw_conv_packed_ragged(pro):
    """bar: 1e-4, what test_pw_conv_persistent_variants holds the uniform 256 x 128 kernel to (split-bf16 products)"""
    from sudo_rm_rf_amd import ops, ragged
    frames, L, Bt, Cin, Cout = PW_FRAMES, PW_L, len(PW_FRAMES), 256, 512
    x = rnd(Bt, Cin, L, seed=40, scale=1.3, shift=0.2).float()
    w, bias = rnd(Cout, Cin, 1, seed=41, scale=Cin ** -0.5).float(), rnd(Cout, seed=42, scale=0.2).float()
    gamma, beta = rnd(Cin, seed=44, scale=0.3, shift=1.0), rnd(Cin, seed=45, scale=0.3)
    res = rnd(Bt, Cout, L, seed=43).float() if pro == 2 else None
    xin = _pro_ref(x, frames, pro, gamma, beta, 0.17)
    want = [F.conv1d(xin[b], w.double(), bias.double())[0] + (res[b, :, :n].double() if pro == 2 else 0.0)
            for b, n in enumerate(frames)]
    kw = {}
    if pro:
        kw.update(in_sums=_sums64_valid(x.double(), frames).to(DEV), in_gamma=dev32(gamma), in_beta=dev32(beta))
    if pro == 2:
        kw.update(in_prelu=dev32(torch.tensor([0.17])), residual=res.to(DEV))
    packed = ops.pack_pw_weight(w.to(DEV))
    assert packed is not None

    def run(xx):
        osums = ops.new_sums(Bt, DEV) if pro != 2 else None
        with poisoned_allocations(ragged), ops.kernel_trace(DEV) as tr:
            y = ragged.pw_conv(xx.to(DEV), packed, bias.to(DEV), Cout, frames, out_sums=osums, **kw)
        assert [n for n, _ in tr.launches] == ["pw_conv_x3w_ragged<%d>" % pro]
        return y, osums

    y, osums = run(x)
    for b, n in enumerate(frames):
        check(y[b, :, :n], want[b], 1e-4, "pw_conv_packed_ragged pro=%d example %d" % (pro, b))
    if pro != 2:
        _check_rows(y, want, frames, 1e-4, "pw_conv_packed_ragged pro=%d" % pro)        # exact zeros past the end
        _check_sums_rows(osums, [y[b, :, :n].double().cpu() for b, n in enumerate(frames)], "pw_conv_packed_ragged sums")
    y2, osums2 = run(_nan_tail(x, frames))
    for b, n in enumerate(frames):
        assert torch.equal(y2[b, :, :n], y[b, :, :n]), "example %d depends on x past its end" % b
    if pro != 2:
        assert torch.equal(y2, y), "y depends on x past an example's end"
        _check_sums_rows(osums2, [y[b, :, :n].double().cpu() for b, n in enumerate(frames)], "sums (NaN tail)")


@pytest.mark.parametrize("pro,Cin1,Cout2", [(1, 128, 256), (2, 256, 256), (2, 512, 512)],
                         ids=["bottleneck-128-256", "res-256-256", "res-512-512"])
def test_pw_conv_pair_ragged(pro, Cin1, Cout2):
    """bars: those of test_pw_conv_pair_is_bitwise_the_two_launches -- y and y2 within 1e-4 of fp64 (y2 from the kernel's own y),
    statistics = the fp64 sums of the stored y2 -- per example over its own columns; y2 exactly zero past them.  The pair's
    ragged form runs whatever the uniform form's "tiles >= CUs" gate says, so a batch of five reaches it."""
    from sudo_rm_rf_amd import ops, ragged
    frames, L, Bt, Cmid = PW_FRAMES, PW_L, len(PW_FRAMES), 256
    assert ragged.pw_conv_pair_supported(Cin1, Cmid, Cout2, L)
    x = rnd(Bt, Cin1, L, seed=50, scale=1.3, shift=0.2).float()
    w1, b1 = rnd(Cmid, Cin1, 1, seed=51, scale=Cin1 ** -0.5).float(), rnd(Cmid, seed=52, scale=0.2).float()
    w2, b2 = rnd(Cout2, Cmid, 1, seed=53, scale=Cmid ** -0.5).float(), rnd(Cout2, seed=54, scale=0.2).float()
    res = rnd(Bt, Cmid, L, seed=55).float() if pro == 2 else None
    gamma, beta = rnd(Cin1, seed=56, scale=0.3, shift=1.0), rnd(Cin1, seed=57, scale=0.3)
    xin = _pro_ref(x, frames, pro, gamma, beta, 0.17)
    want1 = [F.conv1d(xin[b], w1.double(), b1.double())[0] + (res[b, :, :n].double() if pro == 2 else 0.0)
             for b, n in enumerate(frames)]
    p1, p2 = ops.pack_pw_weight(w1.to(DEV)), ops.pack_pw_weight(w2.to(DEV))
    assert p1 is not None and p2 is not None
    in_sums = _sums64_valid(x.double(), frames).to(DEV)
    slope = dev32(torch.tensor([0.17])) if pro == 2 else None

    def run(xx):
        sums = ops.new_sums(Bt, DEV)
        with poisoned_allocations(ragged), ops.kernel_trace(DEV) as tr:
            y, y2 = ragged.pw_conv_pair(xx.to(DEV), p1, b1.to(DEV), in_sums, dev32(gamma), dev32(beta), slope,
                                        res.to(DEV) if res is not None else None, p2, b2.to(DEV), Cmid, Cout2, frames,
                                        out_sums2=sums)
        assert [n for n, _ in tr.launches] == ["pw_pair_x3f_ragged<%d>" % pro]
        return y, y2, sums

    y, y2, sums = run(x)
    want2 = []
    for b, n in enumerate(frames):
        check(y[b, :, :n], want1[b], 1e-4, "pair conv 1, example %d" % b)
        want2.append(F.conv1d(y[b:b + 1, :, :n].double().cpu(), w2.double(), b2.double())[0])
    _check_rows(y2, want2, frames, 1e-4, "pair conv 2")
    _check_sums_rows(sums, [y2[b, :, :n].double().cpu() for b, n in enumerate(frames)], "pair statistics")
    ya, y2a, sums_a = run(_nan_tail(x, frames))
    for b, n in enumerate(frames):
        assert torch.equal(ya[b, :, :n], y[b, :, :n]), "y of example %d depends on x past its end" % b
    assert torch.equal(y2a, y2), "y2 depends on x past an example's end"
    _check_sums_rows(sums_a, [y2[b, :, :n].double().cpu() for b, n in enumerate(frames)], "pair statistics (NaN tail)")


def test_pw_conv_pair_ragged_equal_lengths_is_the_uniform_pair():
    from sudo_rm_rf_amd import ops, ragged
    Bt, Cin1, Cmid, Cout2, L = 64, 128, 256, 256, 512            # (the uniform pair wants at least as many tiles as CUs)
    if not ops.pw_conv_pair_supported(Bt, Cin1, Cmid, Cout2, L):
        pytest.fail("the uniform pair does not take the comparison shape on this device")
    x = dev32(rnd(Bt, Cin1, L, seed=50, scale=1.3, shift=0.2))
    w1, b1 = dev32(rnd(Cmid, Cin1, 1, seed=51, scale=Cin1 ** -0.5)), dev32(rnd(Cmid, seed=52, scale=0.2))
    w2, b2 = dev32(rnd(Cout2, Cmid, 1, seed=53, scale=Cmid ** -0.5)), dev32(rnd(Cout2, seed=54, scale=0.2))
    gamma, beta = dev32(rnd(Cin1, seed=56, scale=0.3, shift=1.0)), dev32(rnd(Cin1, seed=57, scale=0.3))
    in_sums = _sums64_valid(x.double().cpu(), [L] * Bt).to(DEV)
    p1, p2 = ops.pack_pw_weight(w1), ops.pack_pw_weight(w2)
    a = ragged.pw_conv_pair(x, p1, b1, in_sums, gamma, beta, None, None, p2, b2, Cmid, Cout2, [L] * Bt)
    b = ops.pw_conv_pair(x, p1, b1, in_sums, gamma, beta, None, None, p2, b2, Cmid, Cout2)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ======================================================================================================================
# whole model
# ======================================================================================================================
CASE, BATCH, T = "cfg2_improved_u16", 32, 10400      # the shortest length that keeps the bench kernel set (test_gpu_batch_distinct)
ORDER_TOL = 2e-6                                     # results that differ only in fp64 atomic order (test_split_forward_stress)




def ragged_lengths(cfg):
    """Row lengths in samples.  n_req = (K // 2) * 2^D = 320 for this config (D = 5): 10240 and 1280 are multiples of it AND of
    the 128-frame tile (1024 / 128 frames), so they stay what they are for n_req = 160: the tile edge and one sample past it.
    The shortest length the fused pyramid takes as an example of its own is 128 frames (8 positions on level D - 1), i.e. any
    length that pads to 1280: 961."""
    n_req = (cfg.enc_kernel_size // 2) << cfg.upsampling_depth
    shortest = 128 * (cfg.enc_kernel_size // 2) - n_req + 1
    fixed = {0: T, 31: T, 3: 10240, 4: 10241, 9: 1280, 10: 1281, 17: shortest, 22: 5119, 27: 7777}
    rng = np.random.default_rng(20260)
    lens = [fixed.get(i, int(rng.integers(shortest, T + 1))) for i in range(BATCH)]
    d = np.diff(lens)
    assert (d > 0).any() and (d < 0).any(), "the lengths must not be monotone in the row index"
    return lens


@pytest.fixture(scope="module")
def setup(manifest):
    cfg, sd, _, _ = load_case(manifest, CASE)
    lens = ragged_lengths(cfg)
    x = torch.from_numpy(weights.make_mixture(BATCH, T, 9120).astype(np.float32))
    x = (x - x.mean(-1, keepdim=True)) / (x.std(-1, keepdim=True) + 1e-9)
    sdt = torch_oracle.to_torch(sd)
    with torch.no_grad():            # the reference, ONCE, row by row at the row's own length
        want = [torch_oracle.forward(cfg, sdt, x[i:i + 1, :, :n].contiguous())[0] for i, n in enumerate(lens)]
    model = build(cfg, sd)
    model._engine().multi_stream = False
    return cfg, model, x, lens, want


def _row_errors(out, rows, lens):
    out = out.detach().cpu()
    return np.array([float((out[i, :, :lens[i]] - rows[i]).abs().max()) for i in range(len(lens))])


def test_ragged_forward_matches_the_oracle_row_by_row(setup):
    from sudo_rm_rf_amd import ops
    cfg, model, x, lens, want = setup
    eng = model._engine()
    assert eng.ragged_plan_supported(BATCH, T, torch.device(DEV)), "zero examples may take the fallback"
    with torch.no_grad(), ops.kernel_trace(DEV) as tr:
        out = model.forward_ragged(x.to(DEV), lens)
    U = cfg.num_blocks
    count = {n: sum(1 for k, _ in tr.launches if k == n) for n in tr.names}
    print("ragged forward dispatched", sorted(count.items()))
    assert count == {"zero_fill": 1, "pack_pw_weights": 1, "encoder_ragged": 1, "pw_pair_x3f_ragged<1>": 1,
                     "pw_pair_x3f_ragged<2>": U - 1, "pyramid_moments_ragged": U, "pyramid_finalize_ragged": U,
                     "pyramid_merge_ragged": U, "pw_conv_x3w_ragged<2>": 1, "pack_decoder": 1, "pw_mask_decode": 1,
                     "overlap_add_ragged": 1}
    assert out.shape == (BATCH, cfg.num_sources, T) and torch.isfinite(out).all()
    report("forward_ragged vs oracle at each row's own length", _row_errors(out, want, lens), TOL)
    for i, n in enumerate(lens):
        assert (out[i, :, n:] == 0).all(), "row %d is not exactly zero past its length %d" % (i, n)


# rows that take degenerate content (tests/edge_signals.py): none of ragged_lengths' fixed rows, lengths of their own
DEGENERATE_ROWS = {6: "silence", 13: "dc", 21: "near_silent"}


def degenerate_batch(x, lens, nan_past_end=False):
    """x with the valid part of three rows replaced: a silent utterance, one that is DC, a near-silent one (1e-8, unnormalised).
    What lies past those rows' ends stays what it was (or NaN): it must not be read."""
    from tests import edge_signals as es
    sig = es.signals(1, 1, x.shape[-1])
    x2 = x.clone()
    for r, name in DEGENERATE_ROWS.items():
        x2[r, 0, :lens[r]] = torch.from_numpy(sig[name][0, 0, :lens[r]])
        if nan_past_end:
            x2[r, 0, lens[r]:] = float("nan")
    return x2


def check_degenerate_rows_forward(manifest, case, setup):
    """forward_ragged on a batch that contains a silent, a DC and a near-silent utterance among ordinary ones: each of the three
    against the fp64 oracle of that row ALONE at its own length under edge_signals.inference_bar (relative to the row's own output
    scale: 1e-9 for the near-silent one; the silent row's reference is identically zero), every other row against the reference
    it had before within TOL -- a statistic leaking into or out of the silent row shows in one or the other -- and every row
    exactly zero past its end."""
    from tests import edge_signals as es
    cfg, model, x, lens, want = setup
    _, sd, _, _ = load_case(manifest, case)
    sd64 = {k: v.double() for k, v in torch_oracle.to_torch(sd).items()}
    x2 = degenerate_batch(x, lens, nan_past_end=True)
    assert model._engine().ragged_plan_supported(BATCH, T, torch.device(DEV)), "the batch must take the ragged kernels"
    with torch.no_grad():
        out = model.forward_ragged(x2.to(DEV), lens).cpu()
    assert torch.isfinite(out).all()
    for r, name in DEGENERATE_ROWS.items():
        n = lens[r]
        with torch.no_grad():
            ref = torch_oracle.forward(cfg, sd64, x2[r:r + 1, :, :n].double())[0]
        wmax = float(ref.abs().max())
        zero = name == "silence"
        assert (wmax == 0.0) == zero, (name, wmax)
        bar = es.inference_bar(wmax, zero)
        err = float((out[r, :, :n].double() - ref).abs().max())
        print("forward_ragged row %d (%s, %d samples): err %.3e bar %.3e (max|want| %.3e)" % (r, name, n, err, bar, wmax))
        assert err <= bar, (name, err, bar)
    others = [i for i in range(BATCH) if i not in DEGENERATE_ROWS]
    errs = _row_errors(out, want, lens)
    report("forward_ragged, the ordinary rows beside the degenerate ones", errs[others], TOL, labels=others)
    for i, n in enumerate(lens):
        assert (out[i, :, n:] == 0).all(), "row %d is not exactly zero past its length %d" % (i, n)


def test_ragged_forward_with_silent_dc_and_near_silent_rows(manifest, setup):
    check_degenerate_rows_forward(manifest, CASE, setup)


@pytest.mark.parametrize("keep", [0, 1], ids=["even-rows", "odd-rows"])
def test_ragged_rows_are_isolated(setup, keep):
    """Same call again with everything a row must not depend on changed: the input past every length NaN, the workspace and
    the output buffer filled with 0xFF bytes beforehand, and the CONTENT of every other row replaced.  The kept rows must be
    finite and within 2e-6 of their first result (only the fp64 atomic order differs); every row exactly zero past its length."""
    from sudo_rm_rf_amd import engine as engine_mod
    cfg, model, x, lens, _ = setup
    with torch.no_grad():
        first = model.forward_ragged(x.to(DEV), lens).cpu()
    other = torch.from_numpy(weights.make_mixture(BATCH, T, 9121 + keep).astype(np.float32)) * 3.0 + 0.25
    x2 = x.clone()
    for i, n in enumerate(lens):
        if i % 2 != keep:
            x2[i] = other[i]
        x2[i, :, n:] = float("nan")
    eng = model._engine()
    eng.last_plan.workspace.fill_(0xFF)
    with torch.no_grad(), poisoned_allocations(engine_mod):
        out = model.forward_ragged(x2.to(DEV), lens).cpu()
    kept = [i for i in range(BATCH) if i % 2 == keep]
    for i in kept:
        assert torch.isfinite(out[i]).all(), "row %d is not finite" % i
    err = np.array([float((out[i, :, :lens[i]] - first[i, :, :lens[i]]).abs().max()) for i in kept])
    report("kept rows vs their first result", err, ORDER_TOL, labels=kept)
    for i, n in enumerate(lens):
        assert (out[i, :, n:] == 0).all(), "row %d is not exactly zero past its length %d" % (i, n)


def test_ragged_forward_with_equal_lengths_is_the_uniform_forward(setup):
    cfg, model, x, _, _ = setup
    rows = x[:BATCH].to(DEV)
    with torch.no_grad():
        a = model.forward_ragged(rows, [T] * BATCH)
        b = model(rows)
    report("forward_ragged(all lengths = T) vs model(x)", per_example_error(a, b.cpu()), ORDER_TOL)


def test_ragged_forward_is_inference_only(setup):
    cfg, model, x, lens, _ = setup
    with pytest.raises(NotImplementedError):
        model.forward_ragged(x.to(DEV), lens)            # (grad mode on, parameters require grad)


def test_separate_list_matches_separate_per_utterance(setup):
    """40 utterances of mixed length, level and offset: each result against pipeline.separate of that tensor alone, within
    TOL * max(1, std_i) (the rescale multiplies the model's error by the utterance's std); the whole list costs two plans."""
    from sudo_rm_rf_amd import pipeline
    cfg, model, _, _, _ = setup
    rng = np.random.default_rng(77)
    n = 40
    lens = [int(v) for v in rng.integers(3000, T + 1, n)]
    gain = np.geomspace(0.05, 20.0, n)[rng.permutation(n)]
    mixes = [torch.from_numpy((gain[i] * weights.make_mixture(1, lens[i], 9200 + i)[0, 0] + rng.uniform(-0.5, 0.5)).astype(np.float32)).to(DEV)
             for i in range(n)]
    assert all(pipeline.ragged_route(model, m.numel()) == "ragged" for m in mixes)
    eng = model._engine()
    before = set(eng._plans)
    got = pipeline.separate_list(model, [m if i % 2 else m.unsqueeze(0) for i, m in enumerate(mixes)], max_batch=20)
    made = set(eng._plans) - before
    print("separate_list: %d utterances, %d plans created: %s" % (n, len(made), sorted((k[1], k[2]) for k in made)))
    assert len(made) <= 2 < n
    err, bar = [], []
    for i, m in enumerate(mixes):
        want = pipeline.separate(model, m.unsqueeze(0))[0]
        assert got[i].shape == want.shape == (cfg.num_sources, lens[i])
        err.append(float((got[i] - want).abs().max()))
        bar.append(TOL * max(1.0, float(m.std())))
    report("separate_list vs separate per utterance", np.array(err), np.array(bar))


def test_separate_list_with_mixture_consistency_on_the_ragged_path(setup):
    """mixture_consistency=True on the Improved model: the ragged path's own consistency step (README.md:106-114: on the
    rescaled estimates, against the normalised mixture) against separate() per utterance, same bar as above."""
    from sudo_rm_rf_amd import ops, pipeline
    cfg, model, _, _, _ = setup
    lens = [6000 + 37 * i for i in range(20)]
    mixes = [torch.from_numpy((0.5 + 0.3 * i) * weights.make_mixture(1, n, 9500 + i)[0, 0].astype(np.float32) + 0.2).to(DEV)
             for i, n in enumerate(lens)]
    with ops.kernel_trace(DEV) as tr:
        got = pipeline.separate_list(model, mixes, mixture_consistency=True, max_batch=20)
    assert "overlap_add_ragged" in tr.names
    err, bar = [], []
    for g, m in zip(got, mixes):
        want = pipeline.separate(model, m.unsqueeze(0), mixture_consistency=True)[0]
        err.append(float((g - want).abs().max()))
        bar.append(TOL * max(1.0, float(m.std())))
    report("separate_list(mixture_consistency=True) vs separate per utterance", np.array(err), np.array(bar))


def test_separate_list_falls_back_to_the_per_utterance_path(setup):
    """A GroupComm model (no ragged kernels) and an Improved list with a too-short utterance and a batch too small for the
    ragged plan: the same call still returns the per-utterance answers."""
    from sudo_rm_rf_amd import ops, pipeline
    cfg, model, _, _, _ = setup
    gcfg = ModelConfig("groupcomm", 64, 128, 2, 3, 21, 64, 2, 1, 4)
    gmodel = build(gcfg, weights.make_state_dict(gcfg, seed=3))
    for mdl, lens in ((gmodel, [2500, 1800, 3100]), (model, [200, 4000, 5000, 7000])):
        mixes = [torch.from_numpy(weights.make_mixture(1, n, 9300 + n)[0, 0].astype(np.float32) * 2.0 + 0.1).to(DEV) for n in lens]
        assert pipeline.ragged_route(mdl, lens[0]) == "single"
        with ops.kernel_trace(DEV) as tr:
            got = pipeline.separate_list(mdl, mixes)
        assert not any(n.endswith("_ragged") or "_ragged<" in n for n in tr.names), tr.names
        for g, m in zip(got, mixes):
            want = pipeline.separate(mdl, m.unsqueeze(0))[0]
            assert g.shape == want.shape and float((g - want).abs().max()) <= TOL * max(1.0, float(m.std()))
