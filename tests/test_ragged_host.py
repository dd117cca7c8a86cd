"""Ragged forms, host side (no GPU): the symbols are bound under the unchanged ABI number, the per-example length predicate
follows its rule, and every refusal comes back before anything is launched."""
import ctypes as C

import pytest

FAKE = lambda k: C.c_void_p(4096 * k)      # aligned, never dereferenced


def _err(lib):
    return lib.srf_last_error().decode()


def _ints(*v):
    return (C.c_int * max(len(v), 1))(*v)


def test_symbols_bound_and_abi_unchanged():
    from sudo_rm_rf_amd import _lib, ragged
    lib = _lib.load()
    assert lib.srf_abi_version() == 19 == _lib.ABI_VERSION
    for name in ("srf_encoder_ragged", "srf_pyramid_ragged", "srf_pyramid_ragged_frames_ok"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert ragged.MAX_BATCH == 128
    assert callable(ragged.encoder) and callable(ragged.pyramid)


@pytest.mark.parametrize("length,K,D,frames", [(1, 21, 4, 16), (160, 21, 4, 16), (161, 21, 4, 32), (10400, 21, 4, 1040),
                                               (10241, 21, 4, 1040), (10240, 21, 4, 1024), (32000, 21, 5, 3200),
                                               (7777, 41, 6, 448)])
def test_padded_frames_is_the_reference_padding_rule(length, K, D, frames):
    """ragged.padded_frames == srf_plan_frames of a batch-1 plan (improved_sudormrf.py:244,303-314)."""
    from sudo_rm_rf_amd import _lib, ragged
    assert ragged.padded_frames(length, K, D) == frames
    cfg = _lib.srf_config(0, 1, 64, 128, 2, D, K, 64, 2, 1)
    plan = C.c_void_p()
    lib = _lib.load()
    assert lib.srf_plan_create(C.byref(cfg), 1, length, C.byref(plan)) == 0, _err(lib)
    try:
        assert lib.srf_plan_frames(plan) == frames
    finally:
        lib.srf_plan_destroy(plan)


def test_frames_predicate():
    """An example's own length must be what the register-resident kernels and the finalize step's edge algebra take as a
    row length: on the 2^(D-1) grid and the chunk grid (16; 32 for D = 6), >= 4 chunks, >= 8 positions on the deepest level."""
    from sudo_rm_rf_amd import ragged
    ok = ragged.frames_ok
    assert ok(64, 1040, 4) and ok(1040, 1040, 4) and ok(1024, 1040, 4)
    assert not ok(48, 1040, 4)            # 48 >> 3 = 6 positions on the deepest level
    assert not ok(1056, 1040, 4)          # longer than the row stride
    assert not ok(72, 1040, 4)            # off the 16-frame chunk grid
    assert not ok(0, 1040, 4) and not ok(-16, 1040, 4)
    assert ok(128, 3200, 5) and not ok(112, 3200, 5)      # D = 5: 8 positions on level 4 need 128 frames
    assert ok(256, 6400, 6) and not ok(224, 6400, 6) and not ok(272, 6400, 6)
    assert not ok(64, 1040, 0) and not ok(4096, 8192, 9)


def test_pyramid_ragged_refusals_come_before_any_launch():
    """Fake device pointers on a machine without a GPU: a refusal that came after the first launch would crash this test."""
    from sudo_rm_rf_amd import _lib
    lib = _lib.load()
    D, Cc, L = 4, 32, 1040
    arr = (C.c_void_p * D)(*[4096 * (10 + k) for k in range(D)])
    nrm = _lib.srf_norm()

    def run(frames, groups=None, L_=L, y1=FAKE(1), merged=FAKE(2), scratch=FAKE(3)):
        t = _ints(*frames) if frames is not None else None
        return lib.srf_pyramid_ragged(y1, merged, C.byref(nrm), arr, arr, arr, arr, len(frames) if groups is None else groups,
                                      Cc, L_, D, scratch, None, t, None)

    assert run([1040, 0]) == -1 and "example 1" in _err(lib) and "0 frames" in _err(lib)
    assert run([1056]) == -1 and "example 0" in _err(lib) and "1056" in _err(lib) and "1..1040" in _err(lib)
    assert run([1040, 1040, 48]) == -1 and "example 2" in _err(lib) and "48 frames" in _err(lib) and "too short" in _err(lib)
    assert run([1040, 72]) == -1 and "example 1" in _err(lib) and "chunk grid" in _err(lib)
    assert run([-16]) == -1 and "example 0" in _err(lib)
    assert run(None, groups=2) == -1 and "null" in _err(lib)
    assert run([64] * 129) == -1 and "129" in _err(lib) and "128" in _err(lib)
    assert run([], groups=0) == -1 and "1..128" in _err(lib)
    assert run([520], L_=1044) == -1 and "L=1044" in _err(lib)          # a row stride the register kernels do not take
    assert run([1040], merged=FAKE(1)) == -1 and "alias" in _err(lib)
    assert run([1040], y1=None) == -1 and "null" in _err(lib)
    assert run([1040], scratch=C.c_void_p(4096 * 3 + 8)) == -1 and "scratch" in _err(lib) and "aligned" in _err(lib)


def test_encoder_ragged_refusals_come_before_any_launch():
    from sudo_rm_rf_amd import _lib
    lib = _lib.load()
    T, L, N = 10400, 1040, 64

    def run(lengths, frames, Bt=None, A=1, K=21, wav=FAKE(1)):
        return lib.srf_encoder_ragged(wav, FAKE(2), FAKE(3), None, len(lengths) if Bt is None else Bt, A, T, N, K, L,
                                      _ints(*lengths) if lengths is not None else None,
                                      _ints(*frames) if frames is not None else None, None)

    assert run([10400, 0], [1040, 16]) == -1 and "example 1" in _err(lib) and "lengths" in _err(lib)
    assert run([10401], [1040]) == -1 and "example 0" in _err(lib) and "1..10400" in _err(lib)
    assert run([10400], [1041]) == -1 and "frames" in _err(lib) and "1..1040" in _err(lib)
    assert run([5000], [496]) == -1 and "example 0" in _err(lib) and "5000 samples exceed" in _err(lib)
    assert run(None, [16], Bt=1) == -1 and "null" in _err(lib)
    assert run([160], None, Bt=1) == -1 and "null" in _err(lib)
    assert run([160] * 129, [16] * 129) == -1 and "1..128" in _err(lib)
    assert run([160], [16], A=2) == -1 and "A=2" in _err(lib)
    assert run([160], [16], K=11) == -1 and "K=11" in _err(lib)
    assert run([160], [16], wav=None) == -1 and "null" in _err(lib)


def test_python_wrappers_refuse_device_tables_and_wrong_counts():
    import torch
    from sudo_rm_rf_amd import _lib, ragged
    with pytest.raises(_lib.SrfError, match="CUDA"):
        ragged.encoder(torch.zeros(2, 1, 320), torch.zeros(8, 1, 21), 32, [320, 160], [32, 16])
    t, n = ragged._table(torch.tensor([3, 5], dtype=torch.int64), "frames")
    assert n == 2 and list(t) == [3, 5]


# ---- whole-model entry points ---------------------------------------------------------------------------------------------
def _plan(lib, variant, batch, T, out_ch=256, in_ch=512, blocks=2, depth=4, basis=512, A=1, group=1):
    from sudo_rm_rf_amd import _lib
    cfg = _lib.srf_config(variant, A, out_ch, in_ch, blocks, depth, 21, basis, 2, group)
    plan = C.c_void_p()
    assert lib.srf_plan_create(C.byref(cfg), batch, T, C.byref(plan)) == 0, _err(lib)
    return plan


def test_forward_ragged_refusals_come_before_any_launch():
    """length 0, length T + 1, a too-short example, a GroupComm plan, a causal plan -- with fake device pointers."""
    from sudo_rm_rf_amd import _lib
    lib = _lib.load()
    assert {"srf_forward_ragged", "srf_plan_ragged_supported", "srf_plan_ragged_workspace_bytes", "srf_pw_conv_packed_ragged",
            "srf_pw_conv_pair_ragged"} <= set(_lib.EXPORTED_SYMBOLS)
    T, batch = 10400, 32
    plan = _plan(lib, 0, batch, T)
    n = lib.srf_plan_num_params(plan)
    params = (C.c_void_p * n)(*[4096 * (100 + i) for i in range(n)])
    ws = lib.srf_plan_workspace_bytes(plan)

    def run(p, lengths, nparams=n, nbytes=None):
        return lib.srf_forward_ragged(p, params, nparams, FAKE(1), _ints(*lengths), FAKE(2), FAKE(3),
                                      ws if nbytes is None else nbytes, None)

    try:
        assert lib.srf_plan_ragged_supported(plan) == 1, "Improved, 256 channels, batch 32 x 10400 samples"
        assert lib.srf_plan_ragged_workspace_bytes(plan) == ws == lib.srf_plan_workspace_bytes(plan)
        ok = [T] * batch
        assert run(plan, ok[:5] + [0] + ok[6:]) == -1 and "example 5" in _err(lib) and "length 0" in _err(lib)
        assert run(plan, ok[:31] + [T + 1]) == -1 and "example 31" in _err(lib) and "1..10400" in _err(lib)
        assert run(plan, [T, 200] + ok[2:]) == -1 and "example 1" in _err(lib) and "too short" in _err(lib)   # 320 samples = 32 frames
        assert run(plan, ok, nparams=n - 1) == -1 and "parameter tensors" in _err(lib)
        assert run(plan, ok, nbytes=ws - 256) == -3 and "workspace too small" in _err(lib)
    finally:
        lib.srf_plan_destroy(plan)
    for variant, kw, word in ((1, dict(out_ch=64, in_ch=128, basis=64, A=2, group=4), "Improved"), (2, dict(), "Improved")):
        p = _plan(lib, variant, 4, T, **kw)
        try:
            assert lib.srf_plan_ragged_supported(p) == 0 and lib.srf_plan_ragged_workspace_bytes(p) == 0
            m = lib.srf_plan_num_params(p)
            assert lib.srf_forward_ragged(p, (C.c_void_p * m)(*[4096] * m), m, FAKE(1), _ints(T, T, T, T), FAKE(2), FAKE(3),
                                          lib.srf_plan_workspace_bytes(p), None) == -1
            assert "not supported" in _err(lib) and word in _err(lib)
        finally:
            lib.srf_plan_destroy(p)
    # small shapes: too few tiles for the fused tail -> not supported (separate_list runs those one by one)
    p = _plan(lib, 0, 2, 1600)
    try:
        assert lib.srf_plan_ragged_supported(p) == 0
    finally:
        lib.srf_plan_destroy(p)


@pytest.mark.parametrize("n,max_batch", [(0, 32), (1, 32), (40, 20), (40, 32), (97, 8), (5, 1)])
def test_ragged_batches(n, max_batch):
    import numpy as np
    from sudo_rm_rf_amd import pipeline
    rng = np.random.default_rng(n)
    lengths = [int(v) for v in rng.integers(1, 64000, n)]
    if n >= 5:
        lengths[3] = lengths[1]          # a tie
    batches = pipeline.ragged_batches(lengths, max_batch)
    seen = [i for idx, _ in batches for i in idx]
    assert sorted(seen) == list(range(n)), "every index exactly once"
    assert len(batches) == -(-n // max_batch)
    for idx, T in batches:
        assert 1 <= len(idx) <= max_batch
        assert T >= max(lengths[i] for i in idx) and T % pipeline.BUCKET == 0 and T - max(lengths[i] for i in idx) < pipeline.BUCKET
    assert len({(len(idx), T) for idx, T in batches}) <= len(batches)
    # sorted by length across batches; restoring the caller's order is a scatter by these indices
    flat = [lengths[i] for i in seen]
    assert flat == sorted(flat)
    restored = [None] * n
    for idx, _ in batches:
        for i in idx:
            restored[i] = lengths[i]
    assert restored == lengths


def test_fallback_routing_is_decided_from_the_config_alone():
    import sudo_rm_rf.dnn.models.causal_improved_sudormrf_v3 as causal
    import sudo_rm_rf.dnn.models.groupcomm_sudormrf_v2 as gc
    import sudo_rm_rf.dnn.models.improved_sudormrf as imp
    from sudo_rm_rf_amd import pipeline
    m = imp.SuDORMRF(out_channels=256, in_channels=512, num_blocks=2, upsampling_depth=5, enc_kernel_size=21, enc_num_basis=512,
                     num_sources=2)
    assert pipeline.ragged_route(m) == "ragged" and pipeline.ragged_route(m, 10400) == "ragged"
    assert pipeline.ragged_route(m, 961) == "ragged" and pipeline.ragged_route(m, 960) == "single"      # 128 / 96 frames
    small = imp.SuDORMRF(out_channels=64, in_channels=128, num_blocks=2, upsampling_depth=4, enc_kernel_size=21, enc_num_basis=128,
                         num_sources=2)
    assert pipeline.ragged_route(small, 10400) == "single"                 # (the fused conv pair needs 256 bottleneck channels)
    g = gc.GroupCommSudoRmRf(in_audio_channels=1, out_channels=64, in_channels=128, num_blocks=2, upsampling_depth=3,
                             enc_kernel_size=21, enc_num_basis=64, num_sources=2, group_size=4)
    assert pipeline.ragged_route(g, 10400) == "single"
    c = causal.CausalSuDORMRF(in_audio_channels=1, out_channels=64, in_channels=128, num_blocks=2, upsampling_depth=3,
                              enc_kernel_size=21, enc_num_basis=64, num_sources=2)
    assert pipeline.ragged_route(c, 10400) == "single"
