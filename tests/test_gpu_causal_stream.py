"""Streaming inference of the causal SuDoRM-RF (v3) on the MI355X: reference parity of every fixture under three chunk
schedules, schedule invariance (bit-exact), the streaming pyramid against the whole-sequence kernels (bit-exact), row
independence, prepared-once weights and the dispatch seen by the in-library profiler."""
import numpy as np
import pytest
import torch

from tests import causal_fixtures as cf
from tests.causal_stream_ref import schedule_chunks

pytestmark = pytest.mark.gpu
TOL = 1e-4
RAGGED = (7, 133, 1, 64, 250, 3, 415, 2000)   # samples; not multiples of any granule, one longer than 16 granules
SCHEDULES = ("g", "4g", "ragged")              # fixed: no fixture or schedule is filtered at run time


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _model(cfg, seed, dev):
    from sudo_rm_rf_amd.dnn.models.causal_improved_sudormrf_v3 import CausalSuDORMRF
    torch.manual_seed(0)
    m = CausalSuDORMRF(**cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in cf.make_state_dict(cfg, seed).items()})
    return m.to(dev).eval()


def _sizes(sched, g):
    return {"g": (g,), "4g": (4 * g,), "ragged": RAGGED}[sched]


def _stream_all(s, x, sizes):
    """Push x [batch, A, T] through session s cut by `sizes`, finish, return the concatenation on the host."""
    outs = [s.push(x[..., a:b]) for a, b in schedule_chunks(x.shape[-1], sizes)]
    outs.append(s.finish())
    torch.cuda.synchronize()
    return torch.cat(outs, dim=-1).cpu().numpy()


@pytest.mark.parametrize("name", list(cf.CASES))
def test_reference_parity(dev, name):
    """Observed max|stream - stored reference| on an MI355X (bar 1e-4; the full forward's are <= 2e-6):
    causal_tiny 8.9e-8, causal_tiny_a2_k11 3.1e-7, causal_tiny_short 6.7e-8, causal_default 2.8e-7, causal_main 6.1e-7;
    the three schedules give the same figure (they are bit-identical).  These equal the distance of the fp64 recurrence
    from the stored outputs, i.e. the reference's own fp32 rounding."""
    cfg, batch, T, wseed, _, _ = cf.CASES[name]
    m = _model(cfg, wseed, dev)
    x = torch.from_numpy(cf.make_input(name)).to(dev)
    want = cf.load_golden(name)["out"]
    with torch.no_grad():
        s = m.stream(batch=batch)
        for sched in SCHEDULES:
            got = _stream_all(s, x, _sizes(sched, s.granule))
            assert got.shape == want.shape
            err = float(np.abs(got - want).max())
            print("%s / %s: max|stream - reference| = %.3e" % (name, sched, err))
            assert err <= TOL, (name, sched, err)


@pytest.mark.parametrize("name", ["causal_tiny", "causal_default"])
def test_schedule_invariance_is_bit_exact(dev, name):
    cfg, batch, T, wseed, _, _ = cf.CASES[name]
    m = _model(cfg, wseed, dev)
    x = torch.from_numpy(cf.make_input(name)).to(dev)
    with torch.no_grad():
        s = m.stream(batch=batch)
        outs = []
        for sched in SCHEDULES:
            s.reset()
            outs.append(_stream_all(s, x, _sizes(sched, s.granule)))
        full = m(x).cpu().numpy()
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    assert float(np.abs(outs[0] - full).max()) <= TOL      # and the whole-signal forward of the same module agrees


@pytest.mark.parametrize("Bt,Cc,L,D", [(1, 40, 96, 1), (2, 72, 1000, 2), (1, 100, 1040, 5), (3, 64, 2048, 4),
                                       (2, 33, 3200, 3), (1, 512, 1024, 4), (1, 16, 176, 5)])
def test_stream_pyramid_is_bit_identical_to_the_whole_sequence(dev, Bt, Cc, L, D):
    from sudo_rm_rf_amd import ops
    g = torch.Generator().manual_seed(Bt * 1000 + Cc + L + D)
    y1 = torch.randn(Bt, Cc, L, generator=g)
    ws = [torch.randn(Cc, 1, 21, generator=g) * 0.3 for _ in range(D)]
    bs = [torch.randn(Cc, generator=g) * 0.1 for _ in range(D)]
    acts = [torch.rand(1, generator=g) * 0.4 for _ in range(D)]
    ap = torch.rand(1, generator=g) * 0.4
    d = lambda t: t.to(dev)
    y1, ap, ws, bs, acts = d(y1), d(ap), [d(w) for w in ws], [d(b) for b in bs], [d(a) for a in acts]
    whole = ops.causal_pyramid(y1, ap, ws, bs, acts)
    inputs, src = [ops.prelu(y1, ap)], y1
    for k in range(D):
        src = ops.causal_dwconv(src, ws[k], bs[k], 1 if k == 0 else 2, in_prelu=ap if k == 0 else None, out_prelu=acts[k])
        inputs.append(src)
    unit = 1 << (D - 1)          # frames of one granule
    for sizes in ((unit,), (unit, unit, 3 * unit, 8 * unit, 2 * unit, 20 * unit)):
        state = [torch.zeros(Bt, Cc, 10, device=dev) for _ in range(D)]
        parts = [ops.causal_stream_pyramid(y1[..., a:b].contiguous(), state, ap, ws, bs, acts)
                 for a, b in schedule_chunks(L, sizes)]
        torch.cuda.synchronize()
        assert torch.equal(torch.cat(parts, dim=-1), whole), sizes
        for k in range(D):
            assert torch.equal(state[k], inputs[k][..., -10:]), (sizes, k)


def test_rows_are_independent(dev):
    cfg = cf.TINY
    m = _model(cfg, 101, dev)
    rng = np.random.default_rng(11)
    with torch.no_grad():
        s = m.stream(batch=4)
        g, h = s.granule, s.delay
        x = torch.from_numpy(rng.standard_normal((4, 1, 20 * g)).astype(np.float32)).to(dev)
        cuts = schedule_chunks(20 * g, (2 * g,))
        plain = [s.push(x[..., a:b]) for a, b in cuts]
        s.reset()
        mixed = []
        for i, (a, b) in enumerate(cuts):
            if i == 5:
                s.reset(rows=[2])
            mixed.append(s.push(x[..., a:b]))
        fresh_s = m.stream(batch=4)
        fresh = [fresh_s.push(x[..., a:b]) for a, b in cuts[5:]]
        torch.cuda.synchronize()
    plain, mixed, fresh = (torch.cat(t, dim=-1).cpu().numpy() for t in (plain, mixed, fresh))
    assert np.array_equal(plain[[0, 1, 3]], mixed[[0, 1, 3]])
    cut = 10 * g - h                                   # output index of the first sample returned after the row reset
    assert np.array_equal(plain[2, :, :cut], mixed[2, :, :cut])
    assert np.array_equal(mixed[2, :, cut + h:], fresh[2])      # the h samples in between lie before the new start
    assert not np.array_equal(mixed[2, :, cut + h:], plain[2, :, cut + h:])


def test_two_sessions_interleave(dev):
    m = _model(cf.TINY, 101, dev)
    rng = np.random.default_rng(12)
    with torch.no_grad():
        sa, sb = m.stream(batch=2), m.stream(batch=2)
        g = sa.granule
        xa, xb = (torch.from_numpy(rng.standard_normal((2, 1, 12 * g + 17)).astype(np.float32)).to(dev) for _ in range(2))
        cuts = schedule_chunks(xa.shape[-1], (g, 3 * g, 57))
        oa, ob = [], []
        for a, b in cuts:
            oa.append(sa.push(xa[..., a:b]))
            ob.append(sb.push(xb[..., a:b]))
        oa.append(sa.finish())
        ob.append(sb.finish())
        inter = [torch.cat(o, dim=-1).cpu().numpy() for o in (oa, ob)]
        seq = [_stream_all(s, x, (g, 3 * g, 57)) for s, x in ((sa, xa), (sb, xb))]
    assert np.array_equal(inter[0], seq[0]) and np.array_equal(inter[1], seq[1])
    assert not np.array_equal(seq[0], seq[1])


def test_weights_are_prepared_once_and_refreshed_on_request(dev):
    m, m_old = _model(cf.TINY, 101, dev), _model(cf.TINY, 101, dev)
    rng = np.random.default_rng(13)
    with torch.no_grad():
        s, s_old = m.stream(), m_old.stream()
        g = s.granule
        x = torch.from_numpy(rng.standard_normal((1, 1, 9 * g)).astype(np.float32)).to(dev)
        a0, b0 = s.push(x[..., :3 * g]), s_old.push(x[..., :3 * g])
        m.sm[1].skipinit_gain.fill_(0.85)                       # in place: the session keeps its snapshot
        a1, b1 = s.push(x[..., 3 * g:6 * g]), s_old.push(x[..., 3 * g:6 * g])
        assert torch.equal(a0, b0) and torch.equal(a1, b1)
        s.refresh_weights()
        s.reset()
        m_new = _model(cf.TINY, 101, dev)
        m_new.sm[1].skipinit_gain.fill_(0.85)
        s_new = m_new.stream()
        a2, c2 = s.push(x), s_new.push(x)
        s_old.reset()
        b2 = s_old.push(x)
        torch.cuda.synchronize()
    assert torch.equal(a2, c2)
    assert not torch.equal(a2, b2)


def test_dispatch_is_the_same_at_one_granule_and_at_max_chunk(dev):
    from sudo_rm_rf_amd import ops
    cfg = cf.DEFAULTS
    m = _model(cfg, 104, dev)
    with torch.no_grad():
        s = m.stream(batch=2)
        seen = []
        for n in (s.granule, s.max_chunk):
            x = torch.randn(2, 1, n, device=dev)
            s.push(x)
            s.reset()
            torch.cuda.synchronize()
            with ops.kernel_trace(dev) as tr:
                s.push(x)
            names = [k for k, _ in tr.launches]
            assert len(names) == s.num_launches == 3 * cfg["num_blocks"] + 5, names
            seen.append(names)
    assert seen[0] == seen[1]
    cnt = {k: seen[0].count(k) for k in set(seen[0])}
    U = cfg["num_blocks"]
    assert cnt == {"stream_encoder": 1, "stream_pw": 2 * U + 3, "stream_pyramid": U, "stream_ola": 1}, cnt
