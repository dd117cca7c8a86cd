"""Streaming inference of the causal SuDoRM-RF (v3), host side (no GPU): the streaming recurrence restated in fp64
(tests/causal_stream_ref.py) against the stored reference outputs, session geometry, and the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import causal_fixtures as cf
from tests.causal_stream_ref import StreamRef, schedule_chunks

RAGGED = (7, 133, 1, 64, 250, 3, 415)   # sample counts that are not multiples of any fixture's granule


def _schedules(g):
    return {"g": (g,), "5g": (5 * g,), "ragged": RAGGED}


@pytest.mark.parametrize("sched", ["g", "5g", "ragged"])
@pytest.mark.parametrize("name", ["causal_tiny", "causal_tiny_a2_k11", "causal_tiny_short"])
def test_fp64_recurrence_reproduces_the_stored_reference(name, sched):
    """Bar 1e-5: the recurrence in fp64 is within 3.2e-7 of these stored outputs (the reference's own fp32 rounding); a
    one-sample shift or a missing state entry shows at 1e-2 and above on outputs of size 0.1-0.2."""
    cfg, batch, T, wseed, _, _ = cf.CASES[name]
    ref = StreamRef(cfg, cf.make_state_dict(cfg, wseed), batch)
    x = torch.from_numpy(cf.make_input(name))
    outs = [ref.push(x[..., a:b]) for a, b in schedule_chunks(T, _schedules(ref.granule)[sched])]
    assert all(o.shape[:2] == (batch, ref.SA) for o in outs)
    outs.append(ref.finish())
    got = torch.cat(outs, dim=-1).numpy()
    want = cf.load_golden(name)["out"]
    assert got.shape == want.shape
    err = float(np.abs(got - want).max())
    print("%s / %s: max|streamed fp64 - stored reference| = %.3e" % (name, sched, err))
    assert err <= 1e-5
    assert ref.pos == 0 and ref.rem.shape[-1] == 0      # finish() resets


def _tuple(cfg, variant="causal"):
    return (variant,) + tuple(cfg[f] for f in cf.FIELDS) + (1,)


def _align64(n):
    return -(-n // 64) * 64


@pytest.mark.parametrize("name", sorted(cf.CASES))
def test_session_geometry(name):
    from sudo_rm_rf_amd.streaming import _Session
    cfg, batch = cf.CASES[name][0], cf.CASES[name][1]
    A, B, Cc, U, D, K, N, S = (cfg[f] for f in cf.FIELDS)
    h = K // 2
    s = _Session(_tuple(cfg), batch)
    assert s.granule == h * 2 ** (D - 1) and s.delay == h
    assert {"causal_tiny": 40, "causal_tiny_a2_k11": 10, "causal_tiny_short": 40, "causal_default": 80,
            "causal_main": 160, "causal_tiny_d8": 1280}[name] == s.granule
    # three sections, each padded to 64 floats (include/sudormrf_hip.h)
    assert s.state_bytes == 4 * (_align64(batch * A * 2 * h) + _align64(U * D * batch * Cc * 10) + _align64(batch * S * A * (h + 1)))
    assert s.state_bytes >= 4 * (A * 2 * h + U * D * Cc * 10 + S * A * (h + 1)) * batch
    assert s.num_launches == 3 * U + 5
    # 16 granules by default; at depth 8 those are 2048 frames, more than the streaming pyramid's LDS holds (srf_stream_create
    # refuses them), and the default is the 10 granules = 1280 frames = 62 560 bytes that fit
    assert s.max_chunk == (10 if D == 8 else 16) * s.granule
    n_floats = sum(int(np.prod(shape)) if shape else 1 for _, shape in cf.schema(cfg))
    assert 4 * n_floats <= s.weights_bytes <= 4 * (n_floats + 64 * len(cf.schema(cfg)))
    assert s.workspace_bytes >= 4 * batch * (s.max_chunk // h) * (N + 2 * B + 2 * Cc + S * A * N + S * A * K)


def _err(lib):
    return lib.srf_last_error().decode()


def test_create_refusals():
    from sudo_rm_rf_amd import _lib
    from sudo_rm_rf_amd.engine import _config_struct
    lib = _lib.load()
    h = C.c_void_p()

    def create(cfg_tuple, batch, max_chunk):
        cfg = _config_struct(*cfg_tuple)
        return lib.srf_stream_create(C.byref(cfg), batch, max_chunk, C.byref(h))

    assert create(_tuple(cf.TINY, "improved"), 1, 40) == -1 and "variant 0" in _err(lib)
    assert create(_tuple(cf.TINY, "groupcomm"), 1, 40) == -1 and "variant 1" in _err(lib)
    assert create(_tuple(cf.TINY), 0, 40) == -1 and "batch 0" in _err(lib)
    assert create(_tuple(cf.TINY), 1, 50) == -1 and "50" in _err(lib) and "granule 40" in _err(lib)
    assert create(_tuple(cf.TINY), 1, 0) == -1 and "max_chunk_samples 0" in _err(lib)
    assert create(_tuple(dict(cf.TINY, enc_kernel_size=20)), 1, 40) == -1 and "odd" in _err(lib)
    assert create(_tuple(cf.TINY), 1, 40 * 4000) == -1 and "LDS" in _err(lib)
    assert create(_tuple(cf.TINY), 1, 40) == 0
    lib.srf_stream_destroy(h)
    from sudo_rm_rf_amd.streaming import _Session
    with pytest.raises(_lib.SrfError, match="causal"):
        _Session(_tuple(cf.TINY, "improved"), 1)


@pytest.mark.parametrize("D", range(1, 9))
def test_default_max_chunk_is_the_largest_the_library_takes_up_to_16_granules(D):
    """srf_stream_create takes the default of every depth; where the default is below 16 granules (depth 8: 10), one granule more
    is refused for the pyramid's LDS."""
    from sudo_rm_rf_amd import _lib
    from sudo_rm_rf_amd.engine import _config_struct
    from sudo_rm_rf_amd.streaming import _Session, default_max_chunk
    cfg = dict(cf.TINY_D8, upsampling_depth=D)
    g = 10 << (D - 1)
    n = default_max_chunk(21, D)
    assert n % g == 0 and n // g == (10 if D == 8 else 16)
    s = _Session(_tuple(cfg), 2)
    assert (s.granule, s.max_chunk) == (g, n)
    if n < 16 * g:
        lib, h = _lib.load(), C.c_void_p()
        c = _config_struct(*_tuple(cfg))
        assert lib.srf_stream_create(C.byref(c), 2, n + g, C.byref(h)) == -1 and "LDS" in _err(lib)


def test_push_reset_and_prepare_refusals_come_before_any_launch():
    """Fake (aligned, never dereferenced) device pointers on a machine without a GPU: every refusal must return before the
    first launch, or this test would crash instead of reading an error message."""
    from sudo_rm_rf_amd import _lib
    from sudo_rm_rf_amd.streaming import _Session
    lib = _lib.load()
    s = _Session(_tuple(cf.TINY), 2, 80)          # granule 40, max chunk 80
    p = lambda k: C.c_void_p(4096 * k)
    ws = s.workspace_bytes

    def push(n, weights=p(1), state=p(2), wav=p(3), out=p(4), work=p(5), nbytes=ws):
        return lib.srf_stream_push(s.handle, weights, state, wav, n, out, work, nbytes, None)

    assert push(0) == -1 and "n = 0" in _err(lib)
    assert push(-40) == -1 and "n = -40" in _err(lib)
    assert push(41) == -1 and "n = 41" in _err(lib) and "granule 40" in _err(lib)
    assert push(120) == -1 and "n = 120" in _err(lib) and "80" in _err(lib)
    assert push(40, nbytes=ws - 1) == -1 and str(ws - 1) in _err(lib) and str(ws) in _err(lib)
    assert push(40, state=C.c_void_p(4096 * 2 + 4)) == -1 and "aligned" in _err(lib) and "0x2004" in _err(lib)
    assert push(40, work=C.c_void_p(4096 * 5 + 128)) == -1 and "0x5080" in _err(lib)
    assert push(40, weights=C.c_void_p(4096 + 16)) == -1 and "0x1010" in _err(lib)
    assert push(40, wav=None) == -1 and "null" in _err(lib)
    for row in (2, 7, -2):
        assert lib.srf_stream_reset(s.handle, p(2), row, None) == -1 and "row %d" % row in _err(lib)
    assert lib.srf_stream_reset(s.handle, C.c_void_p(4096 * 2 + 64), 0, None) == -1 and "0x2040" in _err(lib)
    assert lib.srf_stream_flush(s.handle, C.c_void_p(4096 * 2 + 64), p(3), None) == -1 and "0x2040" in _err(lib)
    arr = (C.c_void_p * 3)(1, 2, 3)
    assert lib.srf_stream_prepare(s.handle, arr, 3, p(1), None) == -1 and "got 3" in _err(lib)
    bad = (C.c_float * 2)(1.0, 0.0)
    assert lib.srf_stream_set_block_scales(s.handle, bad, bad, 2) == -1 and "beta[1]" in _err(lib)
    assert lib.srf_stream_set_block_scales(s.handle, bad, bad, 3) == -1 and "got 3" in _err(lib)
    y1 = p(1)
    arrs = (C.c_void_p * 3)(4096, 8192, 12288)
    rc = lib.srf_causal_stream_pyramid(y1, p(2), arrs, p(3), arrs, arrs, arrs, 1, 8, 6, 3, None)
    assert rc == -1 and "6 frames" in _err(lib)


def test_stream_refuses_autograd_and_cpu():
    from sudo_rm_rf_amd._lib import SrfError
    from sudo_rm_rf_amd.dnn.models.causal_improved_sudormrf_v3 import CausalSuDORMRF
    m = CausalSuDORMRF(**cf.TINY)
    with torch.enable_grad(), pytest.raises(NotImplementedError, match="forward-only"):
        m.stream()
    with torch.no_grad(), pytest.raises(SrfError, match="MI355X"):
        m.stream()
    assert "_srf" not in "".join(m.state_dict().keys()) and not any("stream" in k for k in m.__dict__)


def test_push_byte_model():
    """roofline.causal_stream_push_bytes: weights once (live taps only) + activations and state that scale with the streams."""
    from sudo_rm_rf_amd import roofline
    c = cf.DEFAULTS
    args = [c[f] for f in cf.FIELDS]
    f = lambda bt, n: roofline.causal_stream_push_bytes(bt, *args, n)
    h, U, D, Cc = 10, c["num_blocks"], c["upsampling_depth"], c["in_channels"]
    per_stream = f(2, 80) - f(1, 80)
    weights = f(1, 80) - per_stream
    n_params = sum(int(np.prod(s)) if s else 1 for _, s in cf.schema(c))
    assert 0.85 * 4 * n_params < weights < 4 * n_params          # masked taps and scalars are not counted
    assert per_stream > 4 * 2 * U * D * Cc * 10                  # the state is read and written
    assert f(1, 160) - f(1, 80) == pytest.approx(f(1, 320) - f(1, 240))   # activations are linear in n
    assert weights / f(1, 80) > 0.7                              # one stream, one granule: mostly weights
