"""Depths 7 and 8 at kernel level.  The library takes upsampling_depth 1..8, and every kernel that takes D changes shape up
there: srf_pyramid leaves the register-resident kernels for the LDS ones (srf_pyramid_reg_supported stops at 6), whose halo
table h[k] = 2 h[k+1] + 4 reaches 508 frames beside a 512-frame tile at D = 8; srf_causal_pyramid<8> loads 1280 frames left of
a 1024-frame tile, so a tile's halo spans two earlier tiles; srf_stream_pyramid<D> is one instantiation per depth.

Every expected value is an fp64 restatement on the CPU (the chain of tests/test_gpu_ops.py test_fused_pyramid, _cpu_pyramid of
tests/test_gpu_causal.py); the bars are those tests' bars.  Each test prints its worst error next to the bar
(profiles/deep_depths.txt keeps one run)."""
import pytest
import torch
import torch.nn.functional as F

from sudo_rm_rf_amd.ops import DebugFlag
from tests.test_gpu_causal import _cpu_pyramid
from tests.test_gpu_ops import DEV, check_sums, dev32, gln64, rnd, sums64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    from sudo_rm_rf_amd import _lib
    _lib.load()


# ---- srf_pyramid, the two LDS forms ---------------------------------------------------------------------------------------------
# (Bt, C, L, D, form under no flags).  pyr_pick_tile: a tile is q * 4 * 2^(D-1) frames, q | L / (4 * 2^(D-1)), 384..1024, nearest
# 640, and not the whole row.  D = 7 (unit 256): L = 512 has the candidate 512 = L only -> block per row; L = 1024 -> 512 (two
# tiles).  D = 8 (unit 512): 1024, 1536, 2048 -> 512-frame tiles (two, three, four), halo h[0] = 508; 3136 floats of LDS per
# wavefront, 49 KiB per block.
PYR_SHAPES = [(2, 5, 512, 7, "rows"), (1, 3, 1024, 7, "tiles"), (2, 4, 1024, 8, "tiles"), (1, 3, 1536, 8, "tiles"),
              (1, 2, 2048, 8, "tiles")]
PYR_BAR = 5e-5          # test_fused_pyramid's
# the in-library trace names both forms' passes alike; only the tiled form pre-finalises the input norm's statistics in a launch
# of its own, which is how the trace tells them apart (with an input norm)
PYR_TRACE = {"tiles": ["stats_finalize", "pyramid_moments", "pyramid_finalize", "pyramid_merge"],
             "rows": ["pyramid_moments", "pyramid_finalize", "pyramid_merge"]}
_PYR_CACHE = {}


def _pyr_case(Bt, C, L, D, in_norm):
    """operands and the fp64 chain DilatedConvNorm x D + upsample-and-add (computed once per shape, never written to)"""
    key = (Bt, C, L, D, in_norm)
    if key not in _PYR_CACHE:
        y1 = rnd(Bt, C, L, seed=100 + D, scale=1.4, shift=0.2)
        g_in, b_in = rnd(C, seed=101, scale=0.3, shift=1.0), rnd(C, seed=102, scale=0.3)
        slope = torch.tensor([0.23], dtype=torch.float64)
        W = [rnd(C, 1, 5, seed=110 + k, scale=0.5) for k in range(D)]
        Bi = [rnd(C, seed=120 + k, scale=0.2) for k in range(D)]
        Ga = [rnd(C, seed=130 + k, scale=0.3, shift=1.0) for k in range(D)]
        Be = [rnd(C, seed=140 + k, scale=0.3) for k in range(D)]
        if in_norm:
            cur = gln64(y1, g_in, b_in)
            cur = torch.where(cur >= 0, cur, slope * cur)
        else:
            y1 = y1.float().double()           # no norm: the kernel's input is the chain's input, bit for bit
            cur = y1
        outs = []
        for k in range(D):
            cur = gln64(F.conv1d(cur, W[k], Bi[k], stride=1 if k == 0 else 2, padding=2, groups=C), Ga[k], Be[k])
            outs.append(cur)
        u = outs[-1]
        for k in range(D - 2, -1, -1):
            u = outs[k] + u.repeat_interleave(2, dim=-1)
        _PYR_CACHE[key] = (y1, g_in, b_in, slope, W, Bi, Ga, Be, u)
    return _PYR_CACHE[key]


def _run_deep_pyramid(Bt, C, L, D, flags, in_norm):
    from sudo_rm_rf_amd import _lib, ops
    y1, g_in, b_in, slope, W, Bi, Ga, Be, want = _pyr_case(Bt, C, L, D, in_norm)
    osums = ops.new_sums(Bt, DEV)
    dl = lambda ts: [dev32(t) for t in ts]
    norm = (sums64(y1).to(DEV), dev32(g_in), dev32(b_in), dev32(slope)) if in_norm else (None, None, None, None)
    with ops.debug_flags(flags):
        assert _lib.load().srf_pyramid_supported(C, L, D) == 1, (C, L, D, int(flags))
        with ops.kernel_trace(DEV) as tr:
            got = ops.pyramid(dev32(y1), *norm, dl(W), dl(Bi), dl(Ga), dl(Be), out_sums=osums)
    torch.cuda.synchronize()
    assert torch.isfinite(got).all()
    err = (got.double().cpu() - want).abs().max().item()
    return err, osums, want, [n for n, _ in tr.launches]


@pytest.mark.parametrize("flags", [0, DebugFlag.PYR_NO_LDS_TILES], ids=["default", "no-lds-tiles"])
@pytest.mark.parametrize("Bt,C,L,D,form", PYR_SHAPES)
def test_fused_pyramid_at_depth_7_and_8(Bt, C, L, D, form, flags):
    """srf_pyramid where only the LDS kernels serve (D > 6), on the wave-per-tile form and, under PYR_NO_LDS_TILES, on the
    block-per-row form; never skipped: the shape must be supported."""
    want_form = "rows" if flags else form
    err, osums, want, names = _run_deep_pyramid(Bt, C, L, D, flags, True)
    print("deep pyramid (%d,%d,%d) D=%d lds-%s: max abs err %.3e (bar %.1e)" % (Bt, C, L, D, want_form, err, PYR_BAR))
    assert names == PYR_TRACE[want_form], names
    assert err <= PYR_BAR, err
    check_sums(osums, want, "deep pyramid sums")


@pytest.mark.parametrize("flags", [0, DebugFlag.PYR_NO_LDS_TILES], ids=["default", "no-lds-tiles"])
def test_fused_pyramid_at_depth_8_without_an_input_norm(flags):
    """The form the original model's walk uses (in_norm = NULL) on three tiles of D = 8.  Without an input norm neither form
    launches stats_finalize, so the trace shows the three passes only; which form they are is fixed by the flag and by the same
    shape's trace in test_fused_pyramid_at_depth_7_and_8."""
    err, osums, want, names = _run_deep_pyramid(1, 3, 1536, 8, flags, False)
    print("deep pyramid (1,3,1536) D=8 no input norm, flags %d: max abs err %.3e (bar %.1e)" % (int(flags), err, PYR_BAR))
    assert names == PYR_TRACE["rows"], names
    assert err <= PYR_BAR, err
    check_sums(osums, want, "deep pyramid sums (no input norm)")


@pytest.mark.parametrize("C,L,D", [(4, 1280, 8), (4, 896, 8), (1, 1280, 8), (1, 896, 8)])
def test_fused_pyramid_refuses_what_the_lds_kernels_cannot_take(C, L, D):
    """1280 = 2.5 units of 4 * 2^7 frames (the LDS kernels work on float4 groups of the deepest level); 896 >> 7 = 7 frames on
    the deepest level, fewer than the finalize step's edge algebra needs."""
    from sudo_rm_rf_amd import _lib, ops
    lib = _lib.load()
    assert lib.srf_pyramid_supported(C, L, D) == 0
    with ops.debug_flags(DebugFlag.PYR_NO_LDS_TILES):
        assert lib.srf_pyramid_supported(C, L, D) == 0
    y1 = torch.zeros(1, C, L, device=DEV)
    p = [torch.zeros(C, 1, 5, device=DEV)] * D
    v = [torch.zeros(C, device=DEV)] * D
    with pytest.raises(_lib.SrfError, match="unsupported shape"):
        ops.pyramid(y1, None, None, None, None, p, v, v, v)


# ---- the causal pyramid: fused, per level, streamed -------------------------------------------------------------------------------
# (Bt, C, L, D): one frame on the deepest level | the second tile's 1280-frame halo clipped at the signal start across a whole
# tile | the third tile's halo reaches into tile 0, last tile partial | D = 7 | D = 6
CAUSAL_SHAPES = [(2, 5, 128, 8), (1, 5, 1152, 8), (1, 3, 2432, 8), (2, 7, 1088, 7), (1, 9, 2080, 6)]
CAUSAL_BAR = 1e-5       # test_fused_vs_per_level_vs_cpu's
# two chunk schedules per shape (frames, multiples of 2^(D-1)).  L = 128 at D = 8 is one granule: one schedule exists.  The
# largest chunks (1280 at D = 8: 62 560 bytes of LDS) sit just under what srf_causal_stream_pyramid takes.
STREAM_SCHEDULES = {(2, 5, 128, 8): ([128],),
                    (1, 5, 1152, 8): ([128] * 9, [384, 128, 640]),
                    (1, 3, 2432, 8): ([128] * 19, [384, 128, 640, 1280]),
                    (2, 7, 1088, 7): ([64] * 17, [192, 64, 832]),
                    (1, 9, 2080, 6): ([32] * 65, [96, 32, 928, 1024])}
_CAUSAL_CACHE = {}


def _causal_case(Bt, Cc, L, D):
    key = (Bt, Cc, L, D)
    if key not in _CAUSAL_CACHE:
        g = torch.Generator().manual_seed(Bt * 1000 + Cc + L + D)
        y1 = torch.randn(Bt, Cc, L, generator=g)
        ws = [torch.randn(Cc, 1, 21, generator=g) * 0.3 for _ in range(D)]
        bs = [torch.randn(Cc, generator=g) * 0.1 for _ in range(D)]
        acts = [torch.rand(1, generator=g) * 0.4 for _ in range(D)]
        ap = torch.rand(1, generator=g) * 0.4
        want = _cpu_pyramid(y1.double(), ap.double(), [w.double() for w in ws], [b.double() for b in bs], [a.double() for a in acts])
        _CAUSAL_CACHE[key] = (y1, ap, ws, bs, acts, want)
    return _CAUSAL_CACHE[key]


def _causal_on_device(Bt, Cc, L, D):
    y1, ap, ws, bs, acts, want = _causal_case(Bt, Cc, L, D)
    d = lambda t: t.to(DEV)
    return d(y1), d(ap), [d(w) for w in ws], [d(b) for b in bs], [d(a) for a in acts], want


def _per_level(ops, y1, ap, ws, bs, acts):
    """[PReLU_p(y1), a_0, ..., a_{D-1}] from one srf_causal_dwconv per level: the inputs of the levels, then the last output"""
    lv, src = [ops.prelu(y1, ap)], y1
    for k in range(len(ws)):
        src = ops.causal_dwconv(src, ws[k], bs[k], 1 if k == 0 else 2, in_prelu=ap if k == 0 else None, out_prelu=acts[k])
        lv.append(src)
    return lv


@pytest.mark.parametrize("Bt,Cc,L,D", CAUSAL_SHAPES)
def test_causal_pyramid_at_depth_6_to_8(Bt, Cc, L, D):
    """srf_causal_pyramid_kernel<6 | 7 | 8>: bitwise the per-level kernels, and the fp64 chain within the forward bar."""
    from sudo_rm_rf_amd import ops
    y1, ap, ws, bs, acts, want = _causal_on_device(Bt, Cc, L, D)
    assert ops.causal_pyramid_supported(Cc, L, D)
    with ops.kernel_trace(DEV) as tr:
        fused = ops.causal_pyramid(y1, ap, ws, bs, acts)
    assert [n for n, _ in tr.launches] == ["causal_pyramid"]
    per_level = ops.causal_merge(_per_level(ops, y1, ap, ws, bs, acts)[1:])
    torch.cuda.synchronize()
    err = float((fused.cpu().double() - want).abs().max())
    print("deep causal pyramid (%d,%d,%d) D=%d: max abs err %.3e (bar %.1e), max|ref| %.2f" % (Bt, Cc, L, D, err, CAUSAL_BAR,
                                                                                             want.abs().max()))
    assert torch.equal(fused, per_level)
    assert err <= CAUSAL_BAR


@pytest.mark.parametrize("Bt,Cc,L,D", CAUSAL_SHAPES)
def test_causal_stream_pyramid_at_depth_6_to_8(Bt, Cc, L, D):
    """srf_stream_pyramid_kernel<6 | 7 | 8>: the chunk schedules agree bit for bit, in what they return and in the state they
    leave; the concatenation is within the forward bar of the fp64 whole-signal chain; and the state is the last 10 inputs of
    every level as the per-level kernels produce them on the whole signal (zeros where a level is shorter than 10 frames)."""
    from sudo_rm_rf_amd import ops
    y1, ap, ws, bs, acts, want = _causal_on_device(Bt, Cc, L, D)
    inputs = _per_level(ops, y1, ap, ws, bs, acts)
    runs = []
    for sizes in STREAM_SCHEDULES[(Bt, Cc, L, D)]:
        assert sum(sizes) == L and all(n % (1 << (D - 1)) == 0 for n in sizes)
        state = [torch.zeros(Bt, Cc, 10, device=DEV) for _ in range(D)]
        cuts, a = [], 0
        for n in sizes:
            cuts.append((a, a + n))
            a += n
        with ops.kernel_trace(DEV) as tr:
            parts = [ops.causal_stream_pyramid(y1[..., a:b].contiguous(), state, ap, ws, bs, acts) for a, b in cuts]
        torch.cuda.synchronize()
        assert [n for n, _ in tr.launches] == ["stream_pyramid"] * len(sizes)
        runs.append((torch.cat(parts, dim=-1), state))
    out0, state0 = runs[0]
    err = float((out0.cpu().double() - want).abs().max())
    print("deep stream pyramid (%d,%d,%d) D=%d: max abs err %.3e (bar %.1e)" % (Bt, Cc, L, D, err, CAUSAL_BAR))
    for out, state in runs[1:]:
        assert torch.equal(out, out0)
        assert all(torch.equal(a, b) for a, b in zip(state, state0))
    assert err <= CAUSAL_BAR
    for k in range(D):
        assert torch.equal(state0[k], F.pad(inputs[k], (10, 0))[..., -10:].contiguous()), k
