"""srf_separate_ragged and its two helpers, host side (no GPU): the symbols are declared and bound under the unchanged ABI
number, and every refusal comes back before anything is launched -- the pointers below are fake, so a refusal that came after
the first launch would crash the test."""
import ctypes as C
import os
import re

import pytest

FAKE = lambda k: C.c_void_p(4096 * k)      # aligned, never dereferenced
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("srf_wav_stats_ragged", "srf_wav_gather_ragged", "srf_separate_ragged")


def _err(lib):
    return lib.srf_last_error().decode()


def _ints(*v):
    return (C.c_int * max(len(v), 1))(*v)


def _plan(lib, variant, batch, T):
    from sudo_rm_rf_amd import _lib
    cfg = _lib.srf_config(variant, 1, 256, 512, 2, 4, 21, 512, 2, 1)
    plan = C.c_void_p()
    assert lib.srf_plan_create(C.byref(cfg), batch, T, C.byref(plan)) == 0, _err(lib)
    return plan


def test_symbols_are_exported_declared_and_the_abi_is_19():
    from sudo_rm_rf_amd import _lib, ragged
    lib = _lib.load()
    assert lib.srf_abi_version() == 19 == _lib.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "sudormrf_hip.h")).read()
    assert "#define SRF_ABI_VERSION 19" in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW + ("srf_encoder_ragged_stats",):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\bint %s\s*\(" % name, hdr), "%s is not declared in the public header" % name
    assert callable(ragged.wav_stats) and callable(ragged.wav_gather)


def test_separate_ragged_refusals_come_before_any_launch():
    """length 0, length T + 1, a too-short example, a null stats pointer, a causal plan."""
    from sudo_rm_rf_amd import _lib
    lib = _lib.load()
    T, batch = 10400, 32
    plan = _plan(lib, _lib.VARIANT_IMPROVED, batch, T)
    n = lib.srf_plan_num_params(plan)
    params = (C.c_void_p * n)(*[4096 * (100 + i) for i in range(n)])
    ws = lib.srf_plan_workspace_bytes(plan)

    def run(p, lengths, stats=FAKE(4), wav=FAKE(1), nparams=n, nbytes=None, mc=1):
        return lib.srf_separate_ragged(p, params, nparams, wav, _ints(*lengths), FAKE(2), stats, mc, FAKE(3),
                                       ws if nbytes is None else nbytes, None)

    try:
        assert lib.srf_plan_ragged_supported(plan) == 1
        ok = [T] * batch
        assert run(plan, ok[:5] + [0] + ok[6:]) == -1 and "srf_separate_ragged" in _err(lib)
        assert "example 5" in _err(lib) and "length 0" in _err(lib)
        assert run(plan, ok[:31] + [T + 1]) == -1 and "example 31" in _err(lib) and "1..10400" in _err(lib)
        assert run(plan, [T, 200] + ok[2:]) == -1 and "example 1" in _err(lib) and "too short" in _err(lib)
        assert run(plan, ok, stats=None) == -1 and "null pointer" in _err(lib)
        assert run(plan, ok, wav=None) == -1 and "null pointer" in _err(lib)
        assert run(plan, ok, nparams=n - 1) == -1 and "parameter tensors" in _err(lib)
        assert run(plan, ok, nbytes=ws - 256) == -3 and "workspace too small" in _err(lib)
    finally:
        lib.srf_plan_destroy(plan)
    causal = _plan(lib, _lib.VARIANT_CAUSAL, 4, T)
    try:
        m = lib.srf_plan_num_params(causal)
        rc = lib.srf_separate_ragged(causal, (C.c_void_p * m)(*[4096] * m), m, FAKE(1), _ints(T, T, T, T), FAKE(2), FAKE(4), 0,
                                     FAKE(3), lib.srf_plan_workspace_bytes(causal), None)
        assert rc == -1 and "srf_separate_ragged" in _err(lib) and "not supported" in _err(lib) and "causal" in _err(lib)
    finally:
        lib.srf_plan_destroy(causal)


def test_wav_stats_ragged_refusals_come_before_any_launch():
    from sudo_rm_rf_amd import _lib
    lib = _lib.load()
    run = lambda lengths, rows=None, T=77, wav=FAKE(1), stats=FAKE(2): lib.srf_wav_stats_ragged(
        wav, _ints(*lengths) if lengths is not None else None, stats, len(lengths) if rows is None else rows, T, None)
    assert run([77, 0]) == -1 and "srf_wav_stats_ragged" in _err(lib) and "example 1" in _err(lib)
    assert run([78]) == -1 and "example 0" in _err(lib) and "1..77" in _err(lib)
    assert run([5] * 129) == -1 and "129" in _err(lib) and "128" in _err(lib)
    assert run(None, rows=1) == -1 and "null" in _err(lib)
    assert run([5], wav=None) == -1 and "null" in _err(lib)
    assert run([5], stats=None) == -1 and "null" in _err(lib)


def test_wav_gather_ragged_refusals_come_before_any_launch():
    """a null entry in the pointer table (the message names the example), a batch of 129, lengths outside 1..T"""
    from sudo_rm_rf_amd import _lib
    lib = _lib.load()

    def run(ptrs, lengths, T=80, wav=FAKE(9)):
        tab = (C.c_void_p * max(len(ptrs), 1))(*ptrs)
        return lib.srf_wav_gather_ragged(tab, _ints(*lengths), wav, len(ptrs), T, None)

    assert run([4096, 0, 8192], [5, 77, 1]) == -1 and "srf_wav_gather_ragged" in _err(lib)
    assert "example 1" in _err(lib) and "null" in _err(lib)
    assert run([4096] * 129, [5] * 129) == -1 and "129" in _err(lib) and "128" in _err(lib)
    assert run([4096, 8192], [5, 81]) == -1 and "example 1" in _err(lib) and "1..80" in _err(lib)
    assert run([4096, 8192], [0, 5]) == -1 and "example 0" in _err(lib)
    assert run([4096], [5], wav=None) == -1 and "null" in _err(lib)
    assert lib.srf_wav_gather_ragged(None, _ints(5), FAKE(9), 1, 80, None) == -1 and "null" in _err(lib)


def test_python_wav_gather_refuses_what_it_cannot_take():
    import torch
    from sudo_rm_rf_amd import _lib, ragged
    with pytest.raises(_lib.SrfError, match="CUDA"):
        ragged.wav_gather([torch.zeros(5), torch.zeros(7)], 8)               # CPU tensors
    with pytest.raises(_lib.SrfError, match="1-D"):
        ragged.wav_gather([torch.zeros(1, 5)], 8)                            # a 2-D tensor
    with pytest.raises(_lib.SrfError, match="float32"):
        ragged.wav_gather([torch.zeros(5, dtype=torch.float64)], 8)
    with pytest.raises(_lib.SrfError, match="empty"):
        ragged.wav_gather([], 8)
    with pytest.raises(_lib.SrfError):
        ragged.wav_stats(torch.zeros(2, 1, 8), [8, 4])                       # CPU tensor
