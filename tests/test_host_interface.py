"""Host-side mirror of the reference interface: schema, attributes, pickles, error behaviour (CPU)."""
import io
import json
import os
import pickle
import re

import numpy as np
import pytest
import torch

from oracle.schema import CONFIGS, ModelConfig, state_dict_schema

# what the reference's own classes made (tools/make_golden_host.py): state_dict digests and attributes per SMALL
# configuration, and a whole-module pickle
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _host_manifest():
    with open(os.path.join(GOLDEN, "HOST_MANIFEST.json")) as f:
        return json.load(f)


def _ours(cfg):
    import sudo_rm_rf_amd.dnn.models.improved_sudormrf as imp
    import sudo_rm_rf_amd.dnn.models.groupcomm_sudormrf_v2 as gc
    return (imp.SuDORMRF if cfg.variant == "improved" else gc.GroupCommSudoRmRf)(**cfg.ctor_kwargs())


SMALL = [ModelConfig("improved", 16, 32, 2, 3, 21, 24, 2),
         ModelConfig("improved", 128, 512, 2, 4, 21, 512, 2),
         ModelConfig("groupcomm", 32, 64, 2, 3, 21, 24, 2, 1, 4),
         ModelConfig("groupcomm", 32, 64, 1, 2, 11, 16, 2, 2, 8)]


@pytest.mark.parametrize("cfg", SMALL + [CONFIGS["cfg2_improved_u16"], CONFIGS["cfg3_groupcomm_u8"]],
                         ids=lambda c: f"{c.variant}-U{c.num_blocks}-N{c.enc_num_basis}")
def test_state_dict_schema(cfg):
    m = _ours(cfg)
    sd = m.state_dict()
    schema = state_dict_schema(cfg)
    assert list(sd.keys()) == [k for k, _ in schema]
    for k, shp in schema:
        assert tuple(sd[k].shape) == shp, k
    # parameters() order == state_dict() order (the engine relies on it) and there are no buffers
    assert [id(p) for p in m.parameters()] == [id(v) for v in m.state_dict(keep_vars=True).values()]
    assert len(list(m.buffers())) == 0


def test_public_attributes_and_defaults():
    import sudo_rm_rf_amd.dnn.models.improved_sudormrf as imp
    import sudo_rm_rf_amd.dnn.models.groupcomm_sudormrf_v2 as gc
    m = imp.SuDORMRF()
    assert (m.out_channels, m.in_channels, m.num_blocks, m.upsampling_depth, m.enc_kernel_size,
            m.enc_num_basis, m.num_sources) == (128, 512, 16, 4, 21, 512, 2)
    assert m.n_least_samples_req == 10 * 16
    for name in ("encoder", "ln", "bottleneck", "sm", "mask_net", "decoder", "mask_nl_class"):
        assert hasattr(m, name)
    g = gc.GroupCommSudoRmRf(num_blocks=1)
    assert (g.in_audio_channels, g.out_channels, g.in_channels, g.upsampling_depth, g.enc_kernel_size,
            g.enc_num_basis, g.num_sources) == (1, 256, 512, 5, 21, 512, 2)
    assert g.sm[0].num_group == 16
    with pytest.raises(AssertionError):
        gc.GroupCommSudoRmRf(num_blocks=1, enc_kernel_size=20)   # odd-K assert, groupcomm_sudormrf_v2.py:255-258


def test_reference_import_paths_resolve():
    import sudo_rm_rf.dnn.experiments.utils.mixture_consistency as mixture_consistency
    import sudo_rm_rf.dnn.models.improved_sudormrf as improved_sudormrf
    import sudo_rm_rf.dnn.models.groupcomm_sudormrf_v2 as sudormrf_gc_v2
    assert callable(mixture_consistency.apply)
    for name in ("SuDORMRF", "UConvBlock", "ConvNormAct", "DilatedConvNorm", "NormAct", "GlobLN"):
        assert hasattr(improved_sudormrf, name)
    for name in ("GroupCommSudoRmRf", "GC_UConvBlock", "TAC", "UConvBlock", "GlobLN"):
        assert hasattr(sudormrf_gc_v2, name)


def test_cpu_input_fails_loudly():
    from sudo_rm_rf_amd._lib import SrfError
    m = _ours(SMALL[0])
    with pytest.raises(SrfError, match="no CPU"):
        m(torch.zeros(1, 1, 400))
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 400))          # 2-D input is an error in the reference as well
    import sudo_rm_rf_amd.dnn.experiments.utils.mixture_consistency as mc
    with pytest.raises(ValueError, match="Invalid mixture consistency weight type"):
        mc.apply(torch.zeros(1, 2, 8), torch.zeros(1, 1, 8), "bogus")
    with pytest.raises(RuntimeError):
        mc.apply(torch.zeros(1, 2, 8), torch.zeros(1, 1, 8))


def test_pickle_roundtrip_own_class():
    m = _ours(SMALL[2])
    m._engine()                                  # engine must not be pickled
    buf = io.BytesIO()
    torch.save(m, buf)
    buf.seek(0)
    m2 = torch.load(buf, weights_only=False)
    assert "_srf_engine" not in m2.__dict__
    for (k1, v1), (k2, v2) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert k1 == k2 and torch.equal(v1, v2)


@pytest.mark.parametrize("cfg", SMALL, ids=lambda c: f"{c.variant}-U{c.num_blocks}")
def test_same_seed_same_weights_as_reference(cfg):
    """Under one torch seed our constructor makes the reference's weights: same keys in the same order, and every tensor
    bit for bit (sha256 of its bytes against the reference's state_dict), so a state_dict loads either way; and the
    public attributes the README recipe reads back (README.md:81-88) agree."""
    import hashlib
    want = [c for c in _host_manifest()["cases"].values() if ModelConfig(**c["config"]) == cfg]
    assert len(want) == 1, cfg
    want = want[0]
    assert want["seed"] == 1234
    torch.manual_seed(1234)
    o = _ours(cfg)
    osd = o.state_dict()
    assert list(osd.keys()) == [k for k, _, _, _ in want["state_dict"]]
    for k, shape, dtype, digest in want["state_dict"]:
        v = osd[k]
        assert list(v.shape) == shape and str(v.dtype) == "torch." + dtype, k
        assert hashlib.sha256(v.contiguous().numpy().tobytes()).hexdigest() == digest, k
    o.load_state_dict({k: v.clone() for k, v in osd.items()})
    for a, v in want["attributes"].items():
        assert getattr(o, a) == v, a


def test_reference_whole_module_pickle_unpickles_into_our_classes():
    """Published checkpoints are whole-module pickles (README.md:75): a pickle made by the REFERENCE
    classes (tests/golden/ref_groupcomm_module.pt, tools/make_golden_host.py) must resolve to OUR classes when this
    repo is first on sys.path."""
    meta = _host_manifest()["pickle"]
    cfg = ModelConfig(**meta["config"])
    import sudo_rm_rf_amd.dnn.models.groupcomm_sudormrf_v2 as ours
    m = torch.load(os.path.join(GOLDEN, meta["file"]), weights_only=False)
    assert type(m) is ours.GroupCommSudoRmRf
    assert type(m.sm[0].TAC) is ours.TAC
    assert m.num_sources == cfg.num_sources and m._config_tuple()[-1] == cfg.group_size
    assert [k for k, _ in state_dict_schema(cfg)] == list(m.state_dict().keys())


def test_library_exports_every_declared_symbol():
    """The C-ABI library loads on CPU and exports exactly what include/sudormrf_hip.h declares."""
    from sudo_rm_rf_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "sudormrf_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(srf_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.EXPORTED_SYMBOLS)
    if not os.path.exists(_lib.LIB_PATH):
        from sudo_rm_rf_amd.build import build
        build(verbose=False)
    lib = _lib.load()
    assert lib.srf_abi_version() == _lib.ABI_VERSION
    for name in declared:
        assert hasattr(lib, name), name


def test_plan_geometry_matches_reference_padding_rule():
    """Host-only plan arithmetic (no GPU): L and T' follow improved_sudormrf.py:244,303-310."""
    import ctypes as C
    from sudo_rm_rf_amd import _lib
    from sudo_rm_rf_amd.engine import _config_struct
    lib = _lib.load()
    for cfg in SMALL + [CONFIGS["cfg2_improved_u16"], CONFIGS["cfg5_improved_u36_n4096"]]:
        for T in (1, 50, 517, 1001, 32000, 32079, 128000):
            tup = (cfg.variant, cfg.in_audio_channels, cfg.out_channels, cfg.in_channels, cfg.num_blocks,
                   cfg.upsampling_depth, cfg.enc_kernel_size, cfg.enc_num_basis, cfg.num_sources,
                   cfg.group_size)
            st = _config_struct(*tup)
            h = C.c_void_p()
            _lib.check(lib.srf_plan_create(C.byref(st), 2, T, C.byref(h)))
            assert lib.srf_plan_padded_length(h) == cfg.padded_length(T)
            assert lib.srf_plan_frames(h) == cfg.frames(T)
            assert lib.srf_plan_num_params(h) == len(state_dict_schema(cfg))
            assert lib.srf_plan_workspace_bytes(h) > 0
            lib.srf_plan_destroy(h)
    # argument validation: even kernel size, bad depth
    bad = _config_struct("improved", 1, 16, 32, 1, 3, 20, 16, 2, 1)
    h = C.c_void_p()
    assert lib.srf_plan_create(C.byref(bad), 1, 100, C.byref(h)) == -1
    assert b"odd" in lib.srf_last_error()


@pytest.mark.skipif(torch.cuda.is_available(), reason="host-memory pointers must never reach a HIP call on a GPU box; "
                    "test_backward_follows_its_forward_when_flags_change_in_between[mode_0_to_1] covers it with real buffers")
def test_backward_that_cannot_follow_its_forward_is_refused_before_any_device_call():
    """srf_backward decides every block's pyramid path -- and refuses a backward that cannot follow its forward -- before its first
    HIP call.  No forward filled these buffers (plain host memory), so d_0 counts as missing; under kernel mode 1 the fused head
    that would re-compute it cannot run: SRF_EINVAL with the message that says so, not a HIP error from a memset."""
    import ctypes as C
    from sudo_rm_rf_amd import _lib
    from sudo_rm_rf_amd.engine import _config_struct
    lib = _lib.load()
    cfg = ModelConfig("improved", 16, 32, 2, 3, 21, 24, 2)
    st = _config_struct(cfg.variant, cfg.in_audio_channels, cfg.out_channels, cfg.in_channels, cfg.num_blocks,
                        cfg.upsampling_depth, cfg.enc_kernel_size, cfg.enc_num_basis, cfg.num_sources, cfg.group_size)
    Bt, T = 2, 517
    h = C.c_void_p()
    _lib.check(lib.srf_plan_create(C.byref(st), Bt, T, C.byref(h)))
    prev = lib.srf_get_kernel_mode()
    try:
        n = lib.srf_plan_num_params(h)
        saved_bytes, scratch_bytes = lib.srf_train_saved_bytes(h), lib.srf_train_scratch_bytes(h)
        assert saved_bytes > 0 and scratch_bytes > 0
        host = np.zeros((saved_bytes + scratch_bytes) // 4 + 256, np.float32)
        base = (host.ctypes.data + 255) // 256 * 256
        ptrs = (C.c_void_p * n)(*([base] * n))
        lib.srf_set_kernel_mode(1)
        rc = lib.srf_backward(h, ptrs, ptrs, n, base, base, base, saved_bytes, base + saved_bytes // 256 * 256 + 256, scratch_bytes, None)
        msg = lib.srf_last_error().decode()
        assert rc == -1, (rc, msg)      # SRF_EINVAL
        assert "d_0" in msg and "kernel mode 1" in msg, msg
    finally:
        lib.srf_set_kernel_mode(prev)
        lib.srf_plan_destroy(h)


def test_training_entry_points_share_their_refusals():
    """srf_forward_train, srf_backward and srf_backward_wav go through the entry check of the causal and the original step
    (tests/test_causal_train_host.py, tests/test_original_train_host.py pin those): same wordings, and the two backwards refuse
    a `saved` / `scratch` off the 256-byte grid as the forward always did.  Fake pointers: every call is refused before it
    reads one."""
    import ctypes as C
    from sudo_rm_rf_amd import _lib
    from sudo_rm_rf_amd.engine import Plan
    lib = _lib.load()
    cfg = ModelConfig("improved", 16, 32, 2, 3, 21, 24, 2)
    plan = Plan((cfg.variant, cfg.in_audio_channels, cfg.out_channels, cfg.in_channels, cfg.num_blocks, cfg.upsampling_depth,
                 cfg.enc_kernel_size, cfg.enc_num_basis, cfg.num_sources, cfg.group_size), 2, 517, torch.device("cpu"))
    h, n = plan.handle, plan.num_params
    saved, scratch = plan.train_sizes()
    assert saved > 0 and scratch > 0
    fake, off = C.c_void_p(256), C.c_void_p(260)
    tab = (C.c_void_p * n)(*[256] * n)
    hole = (C.c_void_p * n)(*([256] * (n - 1) + [None]))
    fwd, bwd, wav = lib.srf_forward_train, lib.srf_backward, lib.srf_backward_wav
    cases = [
        (fwd, (None, tab, n, fake, fake, fake, saved, fake, scratch, None), b"srf_forward_train: null plan"),
        (fwd, (h, tab, n, None, fake, fake, saved, fake, scratch, None), b"srf_forward_train: null pointer"),
        (bwd, (h, tab, None, n, fake, fake, fake, saved, fake, scratch, None), b"srf_backward: null pointer"),
        (wav, (h, tab, tab, n, fake, fake, fake, saved, fake, scratch, None, None), b"srf_backward_wav: null grad_wav"),
        (fwd, (h, tab, n + 1, fake, fake, fake, saved, fake, scratch, None), b"parameter tensors"),
        (fwd, (h, hole, n, fake, fake, fake, saved, fake, scratch, None), b"parameter %d is null" % (n - 1)),
        (bwd, (h, tab, hole, n, fake, fake, fake, saved, fake, scratch, None), b"gradient %d is null" % (n - 1)),
        (fwd, (h, tab, n, fake, fake, fake, saved - 1, fake, scratch, None), b"saved buffer too small"),
        (wav, (h, tab, tab, n, fake, fake, fake, saved, fake, scratch - 1, fake, None), b"srf_backward_wav: scratch buffer too small"),
        (fwd, (h, tab, n, fake, fake, off, saved, fake, scratch, None), b"256-byte aligned"),
        (bwd, (h, tab, tab, n, fake, fake, off, saved, fake, scratch, None), b"256-byte aligned"),
        (wav, (h, tab, tab, n, fake, fake, fake, saved, off, scratch, fake, None), b"256-byte aligned"),
    ]
    for fn, args, text in cases:
        assert fn(*args) == -1 and text in lib.srf_last_error(), (text, lib.srf_last_error())


# ---------------------------------------------------------------------------------------------
# checkpoint tooling: DataParallel prefixes, whole-module pickles, wrapped dicts
# ---------------------------------------------------------------------------------------------
def _tiny_models():
    from sudo_rm_rf_amd.dnn.models import groupcomm_sudormrf_v2, improved_sudormrf
    torch.manual_seed(3)
    a = improved_sudormrf.SuDORMRF(out_channels=16, in_channels=32, num_blocks=2, upsampling_depth=3,
                                   enc_kernel_size=11, enc_num_basis=24, num_sources=2)
    b = groupcomm_sudormrf_v2.GroupCommSudoRmRf(in_audio_channels=1, out_channels=16, in_channels=32,
                                                num_blocks=2, upsampling_depth=3, enc_kernel_size=11,
                                                enc_num_basis=24, num_sources=2, group_size=4)
    return a, b


def test_checkpoint_module_prefix_roundtrip():
    from sudo_rm_rf_amd import checkpoint
    for m in _tiny_models():
        sd = m.state_dict()
        pref = checkpoint.add_module_prefix(sd)
        assert all(k.startswith("module.") for k in pref) and len(pref) == len(sd)
        assert list(checkpoint.strip_module_prefix(pref).keys()) == list(sd.keys())
        assert list(checkpoint.add_module_prefix(pref).keys()) == list(pref.keys())     # idempotent
        fresh = type(m)(**checkpoint.config_from_module(m))
        checkpoint.load_checkpoint({"state_dict": pref, "epoch": 3}, fresh)
        for (k, v), (k2, v2) in zip(sd.items(), fresh.state_dict().items()):
            assert k == k2 and torch.equal(v, v2)


def test_checkpoint_whole_module_pickle_and_dataparallel(tmp_path):
    from sudo_rm_rf_amd import checkpoint
    for i, m in enumerate(_tiny_models()):
        # the published pre-trained files are whole-module pickles (README.md:75-98)
        p = tmp_path / ("whole%d.pt" % i)
        torch.save(m, p)
        got = checkpoint.load_checkpoint(str(p))
        assert type(got) is type(m)
        assert checkpoint.config_from_module(got) == checkpoint.config_from_module(m)
        for v, v2 in zip(m.state_dict().values(), got.state_dict().values()):
            assert torch.equal(v, v2)
        # older runners saved the DataParallel wrapper's state_dict
        p2 = tmp_path / ("dp%d.pt" % i)
        torch.save(torch.nn.DataParallel(m).state_dict(), p2)
        fresh = torch.nn.DataParallel(type(m)(**checkpoint.config_from_module(m)))
        checkpoint.load_checkpoint(str(p2), fresh)
        for v, v2 in zip(m.state_dict().values(), fresh.module.state_dict().values()):
            assert torch.equal(v, v2)
    with pytest.raises(TypeError):
        checkpoint.load_checkpoint(m.state_dict())      # bare state_dict without a model to load into


def test_weights_of_a_data_parallel_style_replica_follow_state_dict_order():
    """torch.nn.DataParallel replicas report an empty state_dict and no parameters; the engine collects their weights
    from `_former_parameters` of every sub-module in state_dict (pre-)order.  Emulated on the CPU exactly the way
    torch/nn/parallel/replicate.py builds a replica (the GPU test runs real replicas)."""
    from collections import OrderedDict
    import torch
    import sudo_rm_rf.dnn.models.groupcomm_sudormrf_v2 as gc
    import sudo_rm_rf.dnn.models.improved_sudormrf as imp
    from sudo_rm_rf_amd.engine import _weights
    for model in (imp.SuDORMRF(out_channels=16, in_channels=32, num_blocks=2, upsampling_depth=3, enc_kernel_size=21,
                               enc_num_basis=24, num_sources=2),
                  gc.GroupCommSudoRmRf(in_audio_channels=1, out_channels=32, in_channels=64, num_blocks=2,
                                       upsampling_depth=3, enc_kernel_size=21, enc_num_basis=24, num_sources=2,
                                       group_size=4)):
        modules = list(model.modules())
        index = {m: i for i, m in enumerate(modules)}
        replicas = []
        for m in modules:
            r = m._replicate_for_data_parallel()
            r._former_parameters = OrderedDict()
            replicas.append(r)
        for i, m in enumerate(modules):
            for key, child in m._modules.items():
                setattr(replicas[i], key, None if child is None else replicas[index[child]])
            for key, p in m._parameters.items():
                if p is None:
                    replicas[i]._parameters[key] = None
                else:
                    copy = p.detach().clone().requires_grad_()       # stands in for the Broadcast output
                    setattr(replicas[i], key, copy)
                    replicas[i]._former_parameters[key] = copy
        rep = replicas[0]
        assert len(rep.state_dict()) == 0 and not list(rep.parameters())
        got, want = _weights(rep), list(model.state_dict(keep_vars=True).values())
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert a.shape == b.shape and torch.equal(a.detach(), b.detach())
        assert [id(t) for t in _weights(model)] == [id(t) for t in want]
