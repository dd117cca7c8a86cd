"""Ragged batch for the GroupComm model, host side (no GPU): which plans srf_forward_ragged takes, that every refusal comes
back before anything is launched (fake device pointers), and where pipeline.separate_list sends a GroupComm model."""
import ctypes as C

FAKE = lambda k: C.c_void_p(4096 * k)      # aligned, never dereferenced
T, BATCH = 10400, 32


def _err(lib):
    return lib.srf_last_error().decode()


def _ints(*v):
    return (C.c_int * max(len(v), 1))(*v)


def _plan(lib, batch=BATCH, T_=T, A=1, out_ch=256, in_ch=512, group=16, blocks=2, depth=5, basis=512):
    from sudo_rm_rf_amd import _lib
    cfg = _lib.srf_config(1, A, out_ch, in_ch, blocks, depth, 21, basis, 2, group)
    plan = C.c_void_p()
    assert lib.srf_plan_create(C.byref(cfg), batch, T_, C.byref(plan)) == 0, _err(lib)
    return plan


def test_symbols_bound_and_abi_unchanged():
    from sudo_rm_rf_amd import _lib, ragged
    lib = _lib.load()
    assert lib.srf_abi_version() == 19 == _lib.ABI_VERSION
    for name in ("srf_tac_ragged", "srf_pw_conv_small_ragged", "srf_pw_conv_small_ragged_supported", "srf_pyramid_ragged_rows"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert callable(ragged.tac) and callable(ragged.pw_conv_small)
    assert ragged.pw_conv_small_supported(16, 32, 400) and ragged.pw_conv_small_supported(32, 16, 400)
    assert not ragged.pw_conv_small_supported(8, 16, 400) and not ragged.pw_conv_small_supported(16, 32, 402)


def test_groupcomm_plan_is_supported():
    """variant GroupComm, A = 1, 256 / 512 channels, D = 5, N = 512, G = 16, batch 32 x 10400 samples"""
    from sudo_rm_rf_amd import _lib
    lib = _lib.load()
    plan = _plan(lib)
    try:
        assert lib.srf_plan_ragged_supported(plan) == 1
        assert lib.srf_plan_ragged_workspace_bytes(plan) == lib.srf_plan_workspace_bytes(plan) > 0
    finally:
        lib.srf_plan_destroy(plan)


def test_other_groupcomm_plans_stay_refused():
    from sudo_rm_rf_amd import _lib
    lib = _lib.load()
    for kw in (dict(A=2), dict(group=8), dict(out_ch=128), dict(batch=2, T_=1600)):
        p = _plan(lib, **kw)
        try:
            assert lib.srf_plan_ragged_supported(p) == 0, kw
            assert lib.srf_plan_ragged_workspace_bytes(p) == 0, kw
            batch = kw.get("batch", BATCH)
            m = lib.srf_plan_num_params(p)
            rc = lib.srf_forward_ragged(p, (C.c_void_p * m)(*[4096] * m), m, FAKE(1), _ints(*[kw.get("T_", T)] * batch), FAKE(2),
                                        FAKE(3), lib.srf_plan_workspace_bytes(p), None)
            assert rc == -1 and "not supported" in _err(lib) and "Improved" in _err(lib), (kw, _err(lib))
        finally:
            lib.srf_plan_destroy(p)


def test_forward_ragged_refusals_come_before_any_launch():
    """length 0, length T + 1 and a 200-sample row on the supported plan -- with fake device pointers: a refusal that came
    after the first launch would crash this test."""
    from sudo_rm_rf_amd import _lib
    lib = _lib.load()
    plan = _plan(lib)
    n = lib.srf_plan_num_params(plan)
    params = (C.c_void_p * n)(*[4096 * (100 + i) for i in range(n)])
    ws = lib.srf_plan_workspace_bytes(plan)

    def run(lengths, nparams=n, nbytes=ws):
        return lib.srf_forward_ragged(plan, params, nparams, FAKE(1), _ints(*lengths), FAKE(2), FAKE(3), nbytes, None)

    try:
        ok = [T] * BATCH
        assert run(ok[:5] + [0] + ok[6:]) == -1 and "example 5" in _err(lib) and "length 0" in _err(lib)
        assert run(ok[:31] + [T + 1]) == -1 and "example 31" in _err(lib) and "1..10400" in _err(lib)
        assert run([T, 200] + ok[2:]) == -1 and "example 1" in _err(lib) and "too short" in _err(lib)     # 320 samples = 32 frames
        assert run(ok, nparams=n - 1) == -1 and "parameter tensors" in _err(lib)
        assert run(ok, nbytes=ws - 256) == -3 and "workspace too small" in _err(lib)
    finally:
        lib.srf_plan_destroy(plan)


def test_kernel_entry_refusals_come_before_any_launch():
    from sudo_rm_rf_amd import _lib
    lib = _lib.load()
    L = 400
    par = (C.c_void_p * 9)(*[4096 * (20 + i) for i in range(9)])
    tac = lambda frames, G=16, n=16, Bt=None: lib.srf_tac_ragged(FAKE(1), FAKE(2), par, len(frames) if Bt is None else Bt, G, n,
                                                                 3 * n, L, None, _ints(*frames), None)
    assert tac([400, 0]) == -1 and "example 1" in _err(lib)
    assert tac([401]) == -1 and "example 0" in _err(lib) and "1..400" in _err(lib)
    assert tac([400], G=8) == -1 and "MFMA" in _err(lib) and "G=8" in _err(lib)
    assert tac([400], n=8) == -1 and "n=8" in _err(lib)
    assert tac([16] * 129) == -1 and "1..128" in _err(lib)
    nrm, pre = _lib.srf_norm(), _lib.srf_norm()
    for s in (nrm, pre):
        s.sums, s.gamma, s.beta = 4096 * 40, 4096 * 41, 4096 * 42
    nrm.prelu = 4096 * 43

    def small(frames, rows, rpe, Cin=16, Cout=32, form="pre"):
        if form == "pre":
            return lib.srf_pw_conv_small_ragged(FAKE(1), FAKE(2), FAKE(3), FAKE(4), rows, Cin, Cout, L, None, None, FAKE(5), FAKE(6),
                                                C.byref(pre), FAKE(7), _ints(*frames), rpe, None)
        return lib.srf_pw_conv_small_ragged(FAKE(1), FAKE(2), FAKE(3), FAKE(4), rows, Cin, Cout, L, C.byref(nrm), FAKE(5), None, None,
                                            None, None, _ints(*frames), rpe, None)

    assert small([400, 500], 32, 16) == -1 and "example 1" in _err(lib) and "500" in _err(lib)
    assert small([400, 398], 32, 16) == -1 and "example 1" in _err(lib) and "multiple of 4" in _err(lib)
    assert small([400, 400], 33, 16) == -1 and "whole number" in _err(lib)
    assert small([400], 16, 16, Cin=8, Cout=16) == -1 and "8 -> 16" in _err(lib)
    assert small([400, 0], 32, 16, Cin=32, Cout=16, form="res") == -1 and "example 1" in _err(lib)


def _gc(**kw):
    import sudo_rm_rf.dnn.models.groupcomm_sudormrf_v2 as gc
    args = dict(in_audio_channels=1, out_channels=256, in_channels=512, num_blocks=2, upsampling_depth=5, enc_kernel_size=21,
                enc_num_basis=512, num_sources=2, group_size=16)
    args.update(kw)
    return gc.GroupCommSudoRmRf(**args)


def test_route_is_decided_from_the_config_alone():
    from sudo_rm_rf_amd import pipeline
    m = _gc()
    assert pipeline.ragged_route(m) == "ragged"
    assert pipeline.ragged_route(m, 10400) == "ragged" and pipeline.ragged_route(m, 961) == "ragged"      # 128 frames
    assert pipeline.ragged_route(m, 960) == "single"                                                     # 96 frames
    assert pipeline.ragged_route(_gc(in_audio_channels=2), 10400) == "single"
    assert pipeline.ragged_route(_gc(group_size=8), 10400) == "single"
    assert pipeline.ragged_route(_gc(out_channels=128), 10400) == "single"
