"""Independent streams of one streaming session on the MI355X (CausalSuDORMRF.stream_pool / srf_stream_push_rows): every
stream of a pool gets bit for bit what a batch-1 session of its own returns, whatever the others do in the same push;
reference parity; idle streams, slot reuse, row groups beyond 128, migration between pools, and operand placement."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import causal_fixtures as cf
from tests.causal_stream_ref import schedule_chunks

pytestmark = pytest.mark.gpu
TOL = 1e-4


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


def _signal(rng, A, T, dev):
    return torch.from_numpy(rng.standard_normal((A, T)).astype(np.float32)).to(dev)


def _private(m, x, sizes):
    """x [A, T] through a batch-1 session of its own, cut into `sizes` (a list of sample counts summing to T) -> [S*A, T]."""
    s = m.stream(batch=1)
    outs, t = [], 0
    for n in sizes:
        outs.append(s.push(x[None, :, t:t + n]))
        t += n
    assert t == x.shape[-1]
    outs.append(s.finish())
    return torch.cat(outs, dim=-1)[0]


def _run_plan(pool, xs, plans):
    """plans[i] = ({tick: samples}, close tick): stream i opens at its first tick, delivers xs[i] in those pieces (it is
    absent from every other push) and closes at its close tick.  Returns each stream's concatenated output and its slot."""
    last = max(c for _, c in plans)
    sids, outs, taken, slots = {}, [[] for _ in plans], [0] * len(plans), {}
    for tick in range(last + 1):
        chunks = {}
        for i, (sched, close) in enumerate(plans):
            if tick == min(sched):
                sids[i] = pool.open()
                slots[i] = pool.slot_of(sids[i])
            if tick in sched:
                chunks[sids[i]] = xs[i][:, taken[i]:taken[i] + sched[tick]]
                taken[i] += sched[tick]
        if chunks:
            res = pool.push(chunks)
            assert set(res) == set(chunks)
            for i, sid in sids.items():
                if sid in res:
                    outs[i].append(res[sid])
        for i, (sched, close) in enumerate(plans):
            if tick == close:
                outs[i].append(pool.close(sids[i]))
                del sids[i]
    assert not pool.active and all(t == x.shape[-1] for t, x in zip(taken, xs))
    return [torch.cat(o, dim=-1) for o in outs], slots


def _five_plans(g, max_chunk):
    """Five streams opened at ticks 0, 1, 0, 2, 1: the one-granule, three-granule, ragged, max_chunk and zero-length-tick
    schedules, then ONE push at tick 5 in which all five deliver a different number of whole granules (1, 2, 3, 4, 5 with
    the remainders they carry), so that the 4-row wavefronts of the pyramid hold rows of different lengths and the last
    one holds a single row; they close at different ticks."""
    return [({0: g, 5: g + 3}, 6),
            ({1: 3 * g, 5: 2 * g + 7}, 7),
            ({0: 7, 1: 133, 2: 1, 3: 64, 4: 250, 5: 3 * g - (455 % g) + g // 2}, 6),
            ({2: max_chunk, 5: 4 * g}, 8),
            ({1: 2 * g, 2: 0, 3: g, 5: 5 * g + g - 1}, 6)]


@pytest.mark.parametrize("cfg,seed", [(cf.TINY, 101), (cf.TINY_A2, 102)], ids=["tiny", "tiny_a2"])
def test_every_stream_gets_the_bits_of_a_private_session(dev, cfg, seed):
    m = _model(cfg, seed, dev)
    rng = np.random.default_rng(21)
    with torch.no_grad():
        pool = m.stream_pool(5)
        g = pool.granule
        plans = _five_plans(g, pool.max_chunk)
        xs = [_signal(rng, cfg["in_audio_channels"], sum(p.values()), dev) for p, _ in plans]
        got, slots = _run_plan(pool, xs, plans)
        want = [_private(m, x, [p[t] for t in sorted(p)]) for x, (p, _) in zip(xs, plans)]
        torch.cuda.synchronize()
    assert sorted(slots.values()) == [0, 1, 2, 3, 4]
    SA = cfg["num_sources"] * cfg["in_audio_channels"]
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape == (SA, xs[i].shape[-1]), (i, a.shape, b.shape)
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()), "stream %d differs from its private session" % i
    assert not np.array_equal(got[0].cpu().numpy()[:, :g], got[1].cpu().numpy()[:, :g])


@pytest.mark.parametrize("name", ["causal_tiny", "causal_tiny_a2_k11"])
def test_reference_parity(dev, name):
    """Bar 1e-4 (the streaming suite's); each batch row of the fixture is a pool stream of its own, opened one tick after the
    row before it and cut by a schedule of its own.  Observed max|pool - stored reference| on an MI355X: causal_tiny 8.9e-8,
    causal_tiny_a2_k11 3.1e-7 -- the lock-step path's figures, as the pool is bit-identical to it."""
    cfg, batch, T, wseed, _, _ = cf.CASES[name]
    m = _model(cfg, wseed, dev)
    x = torch.from_numpy(cf.make_input(name)).to(dev)
    want = cf.load_golden(name)["out"]
    with torch.no_grad():
        pool = m.stream_pool(batch)
        g = pool.granule
        sizes = [(g,), (7, 133, 1, 64, 250, 3, 415), (4 * g,)]
        plans = []
        for b in range(batch):
            cuts = schedule_chunks(T, sizes[b % 3])
            plans.append(({b + t: hi - lo for t, (lo, hi) in enumerate(cuts)}, b + len(cuts)))
        got, _ = _run_plan(pool, [x[b] for b in range(batch)], plans)
        torch.cuda.synchronize()
    got = torch.stack(got).cpu().numpy()
    assert got.shape == want.shape
    err = float(np.abs(got - want).max())
    print("%s: max|pool - reference| = %.3e" % (name, err))
    assert err <= TOL, (name, err)


def _equal_states(a, b):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) if isinstance(a[k], torch.Tensor) else a[k] == b[k] for k in a)


def test_idle_streams_are_untouched(dev):
    m = _model(cf.TINY, 101, dev)
    rng = np.random.default_rng(22)
    with torch.no_grad():
        pool = m.stream_pool(3)
        g = pool.granule
        x = _signal(rng, 1, 6 * g + 13, dev)
        noise = _signal(rng, 1, 40 * g, dev)
        other1, idle, other2 = pool.open(), pool.open(), pool.open()      # the idle stream sits between two busy slots
        first = pool.push({idle: x[:, :2 * g + 5], other1: noise[:, :g]})[idle]
        before = pool.export_state(idle)
        for t in range(10):
            busy = {other1: noise[:, t * g:(t + 2) * g], other2: noise[:, t * 3:t * 3 + g + t]}
            assert set(pool.push(busy)) == {other1, other2}
        after = pool.export_state(idle)
        rest = pool.push({idle: x[:, 2 * g + 5:]})[idle]
        waited = torch.cat([first, rest, pool.close(idle)], dim=-1)
        want = _private(m, x, [2 * g + 5, 4 * g + 8])
        torch.cuda.synchronize()
    assert _equal_states(before, after)
    assert float(before["dw"].abs().max()) > 0 and float(before["hist"].abs().max()) > 0 and before["rem"].shape == (1, 5)
    assert torch.equal(waited, want)
    assert pool.active == [other1, other2]


def test_a_closed_slot_is_reused_and_starts_fresh(dev):
    m = _model(cf.TINY, 101, dev)
    rng = np.random.default_rng(23)
    with torch.no_grad():
        pool = m.stream_pool(2)
        g = pool.granule
        xa, xb, xc = (_signal(rng, 1, 5 * g + 9, dev) for _ in range(3))
        a, b = pool.open(), pool.open()
        with pytest.raises(RuntimeError, match="all 2 streams are open"):
            pool.open()
        ob = [pool.push({a: xa[:, :3 * g], b: xb[:, :3 * g]})[b]]
        slot_a = pool.slot_of(a)
        pool.close(a)                                   # leaves slot 0 with a used state
        c = pool.open()
        assert pool.slot_of(c) == slot_a == 0 and c not in (a, b)
        res = pool.push({c: xc[:, :2 * g + 1], b: xb[:, 3 * g:]})
        ob.append(res[b])
        oc = [res[c], pool.push({c: xc[:, 2 * g + 1:]})[c], pool.close(c)]
        ob.append(pool.close(b))
        want_c = _private(m, xc, [2 * g + 1, 3 * g + 8])
        want_b = _private(m, xb, [3 * g, 2 * g + 9])
        torch.cuda.synchronize()
    assert torch.equal(torch.cat(oc, dim=-1), want_c)
    assert torch.equal(torch.cat(ob, dim=-1), want_b)
    with pytest.raises(RuntimeError, match="not open"):
        pool.push({a: xa[:, :g]})


def test_row_groups_beyond_128_rows(dev):
    """130 streams x one granule: two groups of rows for the encoder, the pyramids and the overlap-add (128 + 2), one GEMM
    launch over all 520 columns; two pushes, so that the second one runs on the state the first one left."""
    from sudo_rm_rf_amd import ops
    cfg = cf.TINY
    U = cfg["num_blocks"]
    m = _model(cfg, 101, dev)
    rng = np.random.default_rng(24)
    with torch.no_grad():
        pool = m.stream_pool(130)
        g = pool.granule
        x = torch.from_numpy(rng.standard_normal((130, 1, 2 * g)).astype(np.float32)).to(dev)
        sids = [pool.open() for _ in range(130)]
        assert [pool.slot_of(s) for s in sids] == list(range(130))
        r0 = pool.push({s: x[i, :, :g] for i, s in enumerate(sids)})
        torch.cuda.synchronize()
        with ops.kernel_trace(dev) as tr:
            r1 = pool.push({s: x[i, :, g:] for i, s in enumerate(sids)})
        names = [k for k, _ in tr.launches]
        assert len(names) == pool.num_launches(130) == 2 * U + 3 + 2 * (U + 2), names
        cnt = {k: names.count(k) for k in set(names)}
        assert cnt == {"stream_encoder": 2, "stream_pw": 2 * U + 3, "stream_pyramid": 2 * U, "stream_ola": 2}, cnt
        for i in (0, 127, 128, 129):
            got = torch.cat([r0[sids[i]], r1[sids[i]]], dim=-1)
            s = m.stream(batch=1)
            want = torch.cat([s.push(x[i:i + 1, :, :g]), s.push(x[i:i + 1, :, g:])], dim=-1)[0]
            assert got.shape == want.shape == (2, 2 * g - pool.delay)
            assert torch.equal(got, want), "row %d" % i
        lock = m.stream(batch=5)
        with ops.kernel_trace(dev) as tr5:
            pool.push({sids[i]: x[i, :, :g] for i in (3, 127, 128, 64, 0)})
        assert len(tr5.launches) == pool.num_launches(5) == lock.num_launches == 3 * U + 5
        cnt5 = {k: [n for n, _ in tr5.launches].count(k) for k in tr5.names}
        assert cnt5 == {"stream_encoder": 1, "stream_pw": 2 * U + 3, "stream_pyramid": U, "stream_ola": 1}, cnt5


def test_long_inputs_go_out_in_rounds(dev):
    """max_chunk = 2 granules: a 7-granule input takes four passes while the short stream beside it is in the first only."""
    m = _model(cf.TINY_A2, 102, dev)
    rng = np.random.default_rng(25)
    with torch.no_grad():
        g = m.stream(batch=1).granule
        pool = m.stream_pool(2, max_chunk=2 * g)
        assert pool.max_chunk == 2 * g and pool.capacity == 2
        xl, xs = _signal(rng, 2, 7 * g + 3, dev), _signal(rng, 2, g, dev)
        a, b = pool.open(), pool.open()
        res = pool.push({a: xl, b: xs})
        got_l = torch.cat([res[a], pool.close(a)], dim=-1)
        got_s = torch.cat([res[b], pool.close(b)], dim=-1)
        torch.cuda.synchronize()
        assert res[a].shape[-1] == 7 * g - pool.delay and res[b].shape[-1] == g - pool.delay
        assert torch.equal(got_l, _private(m, xl, [7 * g + 3])) and torch.equal(got_s, _private(m, xs, [g]))


def test_a_stream_moves_to_another_pool(dev):
    from sudo_rm_rf_amd._lib import SrfError
    m = _model(cf.TINY, 101, dev)
    rng = np.random.default_rng(26)
    with torch.no_grad():
        src, dst = m.stream_pool(3), m.stream_pool(4)
        g = src.granule
        x, noise = _signal(rng, 1, 9 * g + 17, dev), _signal(rng, 1, 4 * g, dev)
        src.open()
        s = src.open()                                                   # slot 1 of the source pool
        cut = 4 * g + 11
        outs = [src.push({s: x[:, :g + 30]})[s], src.push({s: x[:, g + 30:cut]})[s]]
        state = src.export_state(s)
        d0, d1, d2 = dst.open(), dst.open(), dst.open()
        t = dst.open()                                                   # slot 3 of the destination pool
        dst.push({d2: noise, t: noise[:, :g + 1]})                      # the slot has a history of its own before the import
        dst.import_state(t, state)
        assert src.slot_of(s) == 1 and dst.slot_of(t) == 3
        assert _equal_states(dst.export_state(t), state)
        outs.append(dst.push({t: x[:, cut:cut + 2 * g], d0: noise[:, :3 * g]})[t])
        outs.append(dst.push({t: x[:, cut + 2 * g:]})[t])
        outs.append(dst.close(t))
        want = _private(m, x, [g + 30, cut - g - 30, 2 * g, x.shape[-1] - cut - 2 * g])
        torch.cuda.synchronize()
        assert torch.equal(torch.cat(outs, dim=-1), want)
        other = _model(cf.TINY_A2, 102, dev).stream_pool(2)
        o = other.open()
        with pytest.raises(SrfError, match="geometry"):
            other.import_state(o, state)


def test_push_refuses_cpu_tensors_autograd_and_wrong_shapes(dev):
    from sudo_rm_rf_amd._lib import SrfError
    m = _model(cf.TINY, 101, dev)
    with torch.no_grad():
        pool = m.stream_pool(2)
        s = pool.open()
        with pytest.raises(SrfError, match="MI355X"):
            pool.push({s: torch.zeros(1, 40)})
        with pytest.raises(RuntimeError, match=r"shape \[1, n\]"):
            pool.push({s: torch.zeros(1, 1, 40, device=dev)})
    with torch.enable_grad(), pytest.raises(NotImplementedError, match="forward-only"):
        pool.push({s: torch.zeros(1, 40, device=dev, requires_grad=True)})
    with torch.no_grad():
        assert pool.push({s: torch.zeros(1, 0, device=dev)})[s].shape == (2, 0)
        assert pool.close(s).shape == (2, 0) and pool.active == []


def test_push_rows_touches_nothing_outside_its_operands(dev):
    """One srf_stream_push_rows through ctypes with wav, out and the state inside a guarded arena: wav and out start 4 and 12
    bytes behind a 256-byte boundary (any address is their contract), the state on one (its contract).  A ragged five-row
    push with the slots out of order writes every word of out, reads no poison and leaves every guard word alone; a refused
    call writes nothing."""
    from sudo_rm_rf_amd import _lib
    from tests.placement import Arena
    cfg = cf.TINY_A2
    A, SA = cfg["in_audio_channels"], cfg["num_sources"] * cfg["in_audio_channels"]
    m = _model(cfg, 102, dev)
    rng = np.random.default_rng(27)
    lib = _lib.load()
    with torch.no_grad():
        pool = m.stream_pool(5)                      # the session, its prepared weights and its workspace
        g, h = pool.granule, pool.delay
        rows = [(4, g), (0, 3 * g), (2, 2 * g), (1, pool.max_chunk), (3, g)]
        total = sum(n for _, n in rows)
        xs = [_signal(rng, A, n, dev) for _, n in rows]
        arena = Arena(dev, 2 << 20)

        def place():
            arena.reset()
            state = arena.place((pool.state_bytes // 4,), shift_floats=0, name="state", zero=True)
            wav = arena.put(torch.cat([x.reshape(-1) for x in xs]), shift_floats=1, name="wav")
            out = arena.place((SA * total,), shift_floats=3, name="out")
            assert wav.data_ptr() % 16 == 4 and out.data_ptr() % 16 == 12 and state.data_ptr() % 256 == 0
            return state, wav, out

        def call(rows, state, wav, out):
            arr = (_lib.srf_stream_row * len(rows))(*rows)
            return lib.srf_stream_push_rows(pool._s.handle, _lib.ptr(pool._weights), _lib.ptr(state), arr, len(rows),
                                            _lib.ptr(wav), _lib.ptr(out), _lib.ptr(pool._workspace), pool._s.workspace_bytes,
                                            _lib.current_stream(dev))

        state, wav, out = place()
        assert call(rows, state, wav, out) == 0, lib.srf_last_error().decode()
        torch.cuda.synchronize()
        arena.check()
        arena.assert_written(out)
        arena.assert_clean(out)
        arena.assert_clean(state)
        o = 0
        for (slot, n), x in zip(rows, xs):
            want = m.stream(batch=1).push(x[None])[0]
            assert torch.equal(out[o:o + SA * n].view(SA, n)[:, h:], want), slot
            o += SA * n
        tail = arena.place((5, SA, h), shift_floats=1, name="out_tail")
        slots = (C.c_int * 5)(*[s for s, _ in rows])
        assert lib.srf_stream_flush_rows(pool._s.handle, _lib.ptr(state), slots, 5, _lib.ptr(tail), _lib.current_stream(dev)) == 0
        torch.cuda.synchronize()
        arena.check()
        arena.assert_written(tail)
        arena.assert_clean(tail)

        state, wav, out = place()
        assert call(rows[:2] + [(4, 2 * g)], state, wav, out) == -1 and "twice" in lib.srf_last_error().decode()
        assert call(rows[:2] + [(5, g)], state, wav, out) == -1 and "slot 5" in lib.srf_last_error().decode()
        assert call(rows[:2] + [(3, g + 1)], state, wav, out) == -1 and "granule" in lib.srf_last_error().decode()
        torch.cuda.synchronize()
        arena.assert_untouched(out)
        assert int(state.count_nonzero()) == 0
        arena.check()
