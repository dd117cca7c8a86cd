"""Independent streams of one streaming session (srf_stream_push_rows / srf_stream_flush_rows), host side (no GPU): every
refusal comes back before anything is launched, the launch count follows its formula, and the Python surface exists."""
import ctypes as C

import pytest
import torch

from tests import causal_fixtures as cf


def _tuple(cfg):
    return ("causal",) + tuple(cfg[f] for f in cf.FIELDS) + (1,)


def _err(lib):
    return lib.srf_last_error().decode()


def _rows(*pairs):
    from sudo_rm_rf_amd import _lib
    return (_lib.srf_stream_row * max(len(pairs), 1))(*pairs)


def test_push_rows_and_flush_rows_refusals_come_before_any_launch():
    """Fake (aligned, never dereferenced) device pointers on a machine without a GPU: a refusal that came after the first
    launch would crash this test instead of returning a message."""
    from sudo_rm_rf_amd import _lib
    from sudo_rm_rf_amd.streaming import _Session
    lib = _lib.load()
    s = _Session(_tuple(cf.TINY), 3, 80)          # 3 slots, granule 40, max chunk 80
    p = lambda k: C.c_void_p(4096 * k)
    ws = s.workspace_bytes

    def push(rows, m=None, weights=p(1), state=p(2), wav=p(3), out=p(4), work=p(5), nbytes=ws):
        arr = _rows(*rows) if rows is not None else None
        return lib.srf_stream_push_rows(s.handle, weights, state, arr, len(rows) if m is None else m, wav, out, work, nbytes, None)

    ok = [(0, 40), (2, 80)]
    assert push(ok, m=0) == -1 and "m = 0" in _err(lib)
    assert push(ok, m=-1) == -1 and "m = -1" in _err(lib)
    assert push([(0, 40)] * 4) == -1 and "m = 4" in _err(lib) and "1..3" in _err(lib)
    assert push([(0, 40), (3, 40)]) == -1 and "slot 3" in _err(lib) and "row 1" in _err(lib)
    assert push([(-1, 40)]) == -1 and "slot -1" in _err(lib)
    assert push([(1, 40), (0, 40), (1, 80)]) == -1 and "slot 1" in _err(lib) and "twice" in _err(lib) and "row 2" in _err(lib)
    assert push([(0, 40), (1, 0)]) == -1 and "n = 0" in _err(lib) and "row 1" in _err(lib)
    assert push([(0, -40)]) == -1 and "n = -40" in _err(lib)
    assert push([(0, 40), (1, 41)]) == -1 and "n = 41" in _err(lib) and "granule 40" in _err(lib)
    assert push([(2, 120)]) == -1 and "n = 120" in _err(lib) and "80" in _err(lib)
    assert push(ok, nbytes=ws - 1) == -1 and str(ws - 1) in _err(lib) and str(ws) in _err(lib)
    assert push(ok, state=C.c_void_p(4096 * 2 + 4)) == -1 and "aligned" in _err(lib) and "0x2004" in _err(lib)
    assert push(ok, work=C.c_void_p(4096 * 5 + 128)) == -1 and "0x5080" in _err(lib)
    assert push(ok, weights=C.c_void_p(4096 + 16)) == -1 and "0x1010" in _err(lib)
    for null in ("weights", "state", "wav", "out", "work"):
        assert push(ok, **{null: None}) == -1 and "null" in _err(lib), null
    assert push(None, m=1) == -1 and "null" in _err(lib)
    assert lib.srf_stream_push_rows(None, p(1), p(2), _rows(*ok), 2, p(3), p(4), p(5), ws, None) == -1 and "null" in _err(lib)

    def flush(slots, m=None, state=p(2), out=p(3)):
        arr = (C.c_int * max(len(slots), 1))(*slots) if slots is not None else None
        return lib.srf_stream_flush_rows(s.handle, state, arr, len(slots) if m is None else m, out, None)

    assert flush([0], m=0) == -1 and "m = 0" in _err(lib)
    assert flush([0, 1, 2, 0]) == -1 and "m = 4" in _err(lib)
    assert flush([0, 3]) == -1 and "slot 3" in _err(lib)
    assert flush([-1]) == -1 and "slot -1" in _err(lib)
    assert flush([0], state=C.c_void_p(4096 * 2 + 64)) == -1 and "0x2040" in _err(lib)
    assert flush([0], out=None) == -1 and "null" in _err(lib)
    assert flush(None, m=1) == -1 and "null" in _err(lib)


@pytest.mark.parametrize("cfg", [cf.TINY, cf.DEFAULTS], ids=["tiny", "defaults"])
def test_push_rows_launch_count(cfg):
    from sudo_rm_rf_amd import _lib
    from sudo_rm_rf_amd.streaming import _Session
    lib = _lib.load()
    U = cfg["num_blocks"]
    s = _Session(_tuple(cfg), 130, None)
    for m, groups in ((1, 1), (128, 1), (129, 2), (130, 2)):
        assert lib.srf_stream_push_rows_num_launches(s.handle, m) == 2 * U + 3 + groups * (U + 2), m
    assert lib.srf_stream_push_rows_num_launches(s.handle, 5) == s.num_launches == 3 * U + 5      # the lock-step push's count
    assert lib.srf_stream_push_rows_num_launches(s.handle, 0) == 0
    assert lib.srf_stream_push_rows_num_launches(None, 1) == 0


def test_row_struct_matches_the_header():
    from sudo_rm_rf_amd import _lib
    assert C.sizeof(_lib.srf_stream_row) == 8 and [f[0] for f in _lib.srf_stream_row._fields_] == ["slot", "n"]
    assert _lib.ABI_VERSION == 19 and _lib.load().srf_abi_version() == 19


def test_stream_pool_refuses_autograd_and_cpu_and_adds_nothing_to_ops():
    from sudo_rm_rf_amd import ops
    from sudo_rm_rf_amd._lib import SrfError
    from sudo_rm_rf_amd.dnn.models.causal_improved_sudormrf_v3 import CausalSuDORMRF
    m = CausalSuDORMRF(**cf.TINY)
    with torch.enable_grad(), pytest.raises(NotImplementedError, match="forward-only"):
        m.stream_pool(4)
    with torch.no_grad(), pytest.raises(SrfError, match="MI355X"):
        m.stream_pool(4)
    assert not any("pool" in k for k in m.__dict__)
    assert not any("pool" in n or "push_rows" in n for n in vars(ops))
