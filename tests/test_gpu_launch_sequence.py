"""The ORDERED list of kernel launches of one forward (and of one training step), pinned launch by launch.

The uniform forward, the ragged forward and the training forward share their parameter views, their step helpers and the
per-level pyramid walk; a change to any of them must leave every configuration's launch sequence what it was.  The expected
lists below were recorded with ops.kernel_trace (single stream) on the commit BEFORE the walks were folded together and are
literals: (names of a run of launches, how often the run repeats) pairs, expanded by _expand.  The ragged forwards are
pinned by name and count in test_gpu_ragged.py / test_gpu_ragged_groupcomm.py.

Shapes: the two smallest golden cases at their own batch and T (per-level pyramid, separate convs, unfused tail -- what the
big shape never runs), cfg 2 and cfg 3 at batch 32, T = 10400 (the smallest shapes that keep the pairs, the fused pyramid and
the fused tail: test_gpu_ragged.py, test_gpu_ragged_groupcomm.py), cfg 2 again under the two debug flags that take the pairs
and the fused pyramid away, and the training step at the shape of the golden case train_cfg2_shape.

Training steps (forward + backward; "train ..." below): srf_backward chooses every block's pyramid path -- chunked / row
kernels, apply-on-load, the fused head -- from L, D, the kernel mode, the debug flags and its forward's record.  TRAIN_SHAPES are
the smallest shapes that reach each of those paths, recorded on the commit BEFORE the path became a table.

Causal (v3) and attentive (v2) walks ("causal ...", "attentive ..." below): the forward, one opted-in training step and one
streamed granule of the causal model, the attentive forward at the shapes of its two fixtures, and the causal shape that runs
res_conv + proj_1x1 as one launch (tests/test_gpu_causal.py, PAIR_CASE).  Recorded on commit 13ee426, the commit BEFORE these walks
took their parameters through the named views of srf_plan.h and shared their weight fold, pack helpers and tail.

The original model's training step ("original train ..." below): one opted-in step at three fixture shapes -- orig_tiny (also
under kernel mode 1), orig_same (no reshape_before_masks) and orig_d1 (34 frames: the padded weight-gradient path) -- recorded on
commit 4711e9b, the commit BEFORE the three training steps took their pack queue, call guards and entry check from one place.

The original model's inference, separate and ragged walks ("original ..." below, without "train"): four fixture shapes at their own
batch and T (orig_tiny, orig_same, orig_d1, orig_s3_k9: the pyramid level by level), orig_default_u2 (the one uniform shape of
these that runs the fused pyramid), orig_tiny again under PYR_PER_LEVEL, under kernel mode 1 and through
pipeline.separate with mixture consistency, and rg_c -- the smallest configuration the ragged gate takes -- through forward_ragged
and separate_ragged.  Recorded on commit 30e11c2, the commit BEFORE the inference walk and the training forward became one walk.

The branches of the Improved / GroupComm walk that the lists above leave out ("IMPROVED_WALK_TRACES" below): a training step whose
forward runs the fp16 pairs (improved_pairs: out_channels = in_channels = 256 and 8 x 32 tiles of 128 frames, one per CU), improved_d5's step under
PYR_PER_LEVEL, TRAIN_FWD_SPLIT_BF16 and TRAIN_FWD_EXACT_MFMA, the GroupComm forward and step under kernel mode 1 (no pre-add: u = x +
GlobLN(q) as a kernel of its own), and the ragged forwards of cfg 2 and cfg 3 and separate_ragged of cfg 2 in order (the shapes of
test_gpu_ragged.py, test_gpu_ragged_groupcomm.py, test_gpu_separate_ragged.py).  Recorded on commit 2377517, the commit BEFORE the
inference walk and the training forward of these two models became one walk."""
import numpy as np
import pytest
import torch

from conftest import load_case
from tests import attentive_fixtures as af
from tests import causal_fixtures as cf
from tests import original_fixtures as of
from tests import original_ragged_fixtures as rf
from oracle import weights
from oracle.schema import ModelConfig
from test_gpu_model import build
from tests.test_gpu_ops import DEV

pytestmark = pytest.mark.gpu

BATCH, T = 32, 10400


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    from sudo_rm_rf_amd import _lib, ops
    _lib.load()
    ops.set_kernel_mode(0)


def _expand(runs):
    out = []
    for names, times in runs:
        out += list(names) * times
    return out


def _forward_trace(model, x, flags=0):
    """launch names, in order, of ONE single-stream inference forward of a model whose plan for x's shape already exists
    (a plan decides its fused pyramid under the flags of its creation: always the default ones here)"""
    from sudo_rm_rf_amd import ops
    eng = model._engine()
    eng.multi_stream = False
    eng.plan_for(x.shape[0], x.shape[2], torch.device(DEV))
    with torch.no_grad(), ops.debug_flags(flags), ops.kernel_trace(DEV) as tr:
        model(x)
    assert ops._debug_flags == 0, "the debug flags were not put back"
    return [n for n, _ in tr.launches]


def _golden_model(manifest, case, batch=None, T_=None, seed=9120):
    cfg, sd, wav, _ = load_case(manifest, case)
    x = torch.from_numpy(wav if batch is None else weights.make_mixture(batch, T_, seed).astype(np.float32))
    return build(cfg, sd), x.to(DEV)


@pytest.fixture(scope="module")
def cfg2(manifest):
    return _golden_model(manifest, "cfg2_improved_u16", BATCH, T)


def trace_tiny_improved(manifest):
    return _forward_trace(*_golden_model(manifest, "tiny_improved"))


def trace_tiny_groupcomm(manifest):
    return _forward_trace(*_golden_model(manifest, "tiny_groupcomm"))


def trace_cfg3(manifest):
    return _forward_trace(*_golden_model(manifest, "cfg3_groupcomm_u8", BATCH, T))


def trace_train(manifest):
    """forward + backward of the training step (model.train(), gradients on) at the shape of train_cfg2_shape"""
    from sudo_rm_rf_amd import ops
    from test_oracle_golden import train_case
    cfg, sd, mix, _, _ = train_case("train_cfg2_shape")
    model = build(cfg, sd).train()
    with ops.kernel_trace(DEV) as tr:
        rec = model(mix.to(DEV))
        (rec * rec).mean().backward()
    return [n for n, _ in tr.launches]


TRAIN_SHAPES = {      # name: (configuration, batch, T)
    "improved_d5": (ModelConfig("improved", 64, 128, 3, 5, 21, 128, 2), 3, 8000),
    "improved_d2": (ModelConfig("improved", 16, 24, 2, 2, 21, 32, 2), 3, 2530),     # level 1 is the deepest: the head starts from a gradient that is not pre-reduced
    "improved_d2_l36": (ModelConfig("improved", 8, 16, 1, 2, 11, 8, 3), 3, 180),    # L = 36: nine float4 per row, L % 8 == 4
    "improved_d1": (ModelConfig("improved", 16, 24, 2, 1, 21, 32, 2), 2, 1000),     # no head, no pyramid loop beyond level 0
    "groupcomm_d4": (ModelConfig("groupcomm", 64, 128, 2, 4, 21, 64, 2, 1, 4), 2, 4000),   # TAC; the non-deferred srf_gln_bwd
    "improved_pairs": (ModelConfig("improved", 256, 256, 2, 2, 21, 128, 2), 8, 40000),     # 4000 frames: the forward's fp16 pairs
}
TRAIN_STEPS = [("improved_d5", "0"), ("improved_d5", "BWD_NO_FUSED_HEAD"), ("improved_d5", "BWD_DW_CHUNKED"),
               ("improved_d5", "BWD_GLN_SCALAR"), ("improved_d5", "kernel_mode_1"), ("improved_d2", "0"), ("improved_d2_l36", "0"),
               ("improved_d1", "0"), ("groupcomm_d4", "0")]


def train_step_trace(shape, setting):
    """launch names, in order, of one training step (forward + backward) of TRAIN_SHAPES[shape] under a debug flag, or under
    kernel mode 1 (forward and backward both): _setting"""
    from sudo_rm_rf_amd import ops
    cfg, batch, T_ = TRAIN_SHAPES[shape]
    if shape == "improved_d2_l36":
        assert cfg.frames(T_) == 36
    model = build(cfg, weights.make_state_dict(cfg, seed=31)).train()
    x = torch.from_numpy(weights.make_mixture(batch, T_, 9120).astype(np.float32)).to(DEV)
    flags, mode = _setting(setting)
    try:
        ops.set_kernel_mode(mode)
        with ops.debug_flags(flags), ops.kernel_trace(DEV) as tr:
            rec = model(x)
            (rec * rec).mean().backward()
    finally:
        ops.set_kernel_mode(0)
    return [n for n, _ in tr.launches]


def _setting(setting):
    """(debug flags, kernel mode) of a setting: "0", a DebugFlag name, or kernel mode 1"""
    from sudo_rm_rf_amd import ops
    if setting == "kernel_mode_1":
        return 0, 1
    return (0 if setting == "0" else int(getattr(ops.DebugFlag, setting))), 0


def causal_model(cfg, seed, scales=None):
    from sudo_rm_rf_amd.dnn.models.causal_improved_sudormrf_v3 import CausalSuDORMRF
    m = CausalSuDORMRF(**cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in cf.make_state_dict(cfg, seed).items()})
    for blk, (alpha, beta) in zip(m.sm, scales or ()):
        blk.alpha, blk.beta = alpha, beta
    return m.to(DEV).eval()


def causal_forward_trace(m, x, setting="0"):
    from sudo_rm_rf_amd import ops
    flags, mode = _setting(setting)
    try:
        ops.set_kernel_mode(mode)
        return _forward_trace(m, x, flags)
    finally:
        ops.set_kernel_mode(0)


def causal_case_trace(name, setting="0"):
    cfg, _, _, wseed, _, _ = cf.CASES[name]
    return causal_forward_trace(causal_model(cfg, wseed), torch.from_numpy(cf.make_input(name)).to(DEV), setting)


def causal_train_step_trace(setting):
    """one opted-in training step (forward + backward of (out * out).mean()) of cf.TINY at batch 2, T = 1001"""
    from sudo_rm_rf_amd import ops
    m = causal_model(cf.TINY, cf.CASES["causal_tiny"][3]).train().enable_hip_training()
    x = torch.from_numpy(cf.make_input("causal_tiny")).to(DEV)
    assert tuple(x.shape) == (2, 1, 1001)
    flags, mode = _setting(setting)
    try:
        ops.set_kernel_mode(mode)
        with ops.debug_flags(flags), ops.kernel_trace(DEV) as tr:
            out = m(x)
            (out * out).mean().backward()
    finally:
        ops.set_kernel_mode(0)
    return [n for n, _ in tr.launches]


def original_train_step_trace(name, setting="0"):
    """one opted-in training step (forward + backward of (out * out).mean()) of the original model at the shape of an
    of.CASES fixture"""
    from sudo_rm_rf_amd import ops
    from sudo_rm_rf_amd.dnn.models.sudormrf import SuDORMRF
    cfg, batch, T_, wseed, _ = of.CASES[name]
    m = SuDORMRF(**cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in of.make_state_dict(cfg, wseed).items()})
    m = m.to(DEV).train().enable_hip_training()
    x = torch.from_numpy(of.make_input(name)).to(DEV)
    assert tuple(x.shape) == (batch, 1, T_)
    flags, mode = _setting(setting)
    try:
        ops.set_kernel_mode(mode)
        with ops.debug_flags(flags), ops.kernel_trace(DEV) as tr:
            out = m(x)
            (out * out).mean().backward()
    finally:
        ops.set_kernel_mode(0)
    return [n for n, _ in tr.launches]


def original_model(cfg, wseed):
    from sudo_rm_rf_amd.dnn.models.sudormrf import SuDORMRF
    m = SuDORMRF(**cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in of.make_state_dict(cfg, wseed).items()})
    return m.to(DEV).eval()


def original_forward_trace(name, setting="0"):
    """one inference forward of the original model at the batch and T of an of.CASES fixture"""
    cfg, batch, T_, wseed, _ = of.CASES[name]
    x = torch.from_numpy(of.make_input(name)).to(DEV)
    assert tuple(x.shape) == (batch, 1, T_)
    return causal_forward_trace(original_model(cfg, wseed), x, setting)


def original_separate_trace(name):
    """pipeline.separate (srf_separate) with mixture consistency on: the statistics launch, then the forward's walk"""
    from sudo_rm_rf_amd import ops, pipeline
    cfg, batch, T_, wseed, _ = of.CASES[name]
    m = original_model(cfg, wseed)
    m._engine().multi_stream = False
    with ops.kernel_trace(DEV) as tr:
        pipeline.separate(m, torch.from_numpy(of.make_input(name)).to(DEV), mixture_consistency=True)
    return [n for n, _ in tr.launches]


def original_ragged_trace(name, entry):
    """forward_ragged / separate_ragged of an opted-in model over the padded batch of an rf.CASES fixture"""
    from sudo_rm_rf_amd import ops
    cfg, T_, lengths, wseed, _ = rf.CASES[name]
    m = original_model(cfg, wseed).enable_ragged()
    m._engine().multi_stream = False
    x = torch.from_numpy(rf.make_wav(name)).to(DEV)
    assert tuple(x.shape) == (len(lengths), 1, T_)
    with torch.no_grad(), ops.kernel_trace(DEV) as tr:
        getattr(m, entry)(x, list(lengths))
    return [n for n, _ in tr.launches]


def causal_stream_push_trace():
    """one srf_stream_push of one granule per stream, on a session of causal_tiny's model and batch"""
    from sudo_rm_rf_amd import ops
    cfg, batch, _, wseed, _, _ = cf.CASES["causal_tiny"]
    m = causal_model(cfg, wseed)
    with torch.no_grad():
        s = m.stream(batch=batch)
        x = torch.from_numpy(cf.make_input("causal_tiny")[..., :s.granule]).to(DEV).contiguous()
        with ops.kernel_trace(DEV) as tr:
            s.push(x)
    return [n for n, _ in tr.launches]


def causal_pair_trace(flags):
    """the shape of tests/test_gpu_causal.py that runs res_conv + the next block's proj_1x1 as one launch"""
    from oracle.weights import make_mixture
    from tests import test_gpu_causal as tgc
    x = torch.from_numpy(make_mixture(tgc.PAIR_BATCH, tgc.PAIR_T, tgc.PAIR_SEED)).to(DEV)
    return tgc.pair_trace(tgc.pair_model(torch.device(DEV)), x, flags)[1]


def attentive_trace(cfg, wseed, wav):
    from sudo_rm_rf_amd import ops
    from sudo_rm_rf_amd.dnn.models.attentive_sudormrf_v2 import SuDORMRF
    m = SuDORMRF(**cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in af.make_state_dict(cfg, wseed).items()})
    m = m.to(DEV).eval()
    with torch.no_grad(), ops.kernel_trace(DEV) as tr:
        m(torch.from_numpy(wav).to(DEV))
    return [n for n, _ in tr.launches]


CAUSAL_TRACES = {
    "causal_tiny 0": lambda: causal_case_trace("causal_tiny"),
    "causal_tiny PYR_PER_LEVEL": lambda: causal_case_trace("causal_tiny", "PYR_PER_LEVEL"),
    "causal_tiny kernel_mode_1": lambda: causal_case_trace("causal_tiny", "kernel_mode_1"),
    "causal_tiny_a2_k11 0": lambda: causal_case_trace("causal_tiny_a2_k11"),
    "causal train 0": lambda: causal_train_step_trace("0"),
    "causal train PYR_PER_LEVEL": lambda: causal_train_step_trace("PYR_PER_LEVEL"),
    "causal train kernel_mode_1": lambda: causal_train_step_trace("kernel_mode_1"),
    "causal stream push": causal_stream_push_trace,
    "attentive tiny": lambda: attentive_trace(af.TINY, af.CASES["attn_tiny"][3], af.make_input("attn_tiny")),
    "causal pair 0": lambda: causal_pair_trace(0),
    "causal pair NO_PAIRS": lambda: causal_pair_trace(1),
    "attentive wide batch 8": lambda: attentive_trace(af.WIDE, af.WIDE_WSEED, af.make_distinct(8, af.WIDE_T, af.WIDE_INPUT_SEED)),
    "original train orig_tiny 0": lambda: original_train_step_trace("orig_tiny"),
    "original train orig_tiny kernel_mode_1": lambda: original_train_step_trace("orig_tiny", "kernel_mode_1"),
    "original train orig_same 0": lambda: original_train_step_trace("orig_same"),          # B == N: no reshape_before_masks
    "original train orig_d1 0": lambda: original_train_step_trace("orig_d1"),              # 34 frames: the padded weight-gradient path
}

ORIGINAL_TRACES = {
    "original orig_tiny 0": lambda: original_forward_trace("orig_tiny"),
    "original orig_same 0": lambda: original_forward_trace("orig_same"),                   # B == N: no reshape_before_masks
    "original orig_d1 0": lambda: original_forward_trace("orig_d1"),
    "original orig_s3_k9 0": lambda: original_forward_trace("orig_s3_k9"),                 # K = 9: the any-K encoder; three sources
    "original orig_default_u2 0": lambda: original_forward_trace("orig_default_u2"),       # the fused pyramid, uniform
    "original orig_tiny PYR_PER_LEVEL": lambda: original_forward_trace("orig_tiny", "PYR_PER_LEVEL"),
    "original orig_tiny kernel_mode_1": lambda: original_forward_trace("orig_tiny", "kernel_mode_1"),
    "original separate orig_tiny mixture_consistency": lambda: original_separate_trace("orig_tiny"),
    "original forward_ragged rg_c": lambda: original_ragged_trace("rg_c", "forward_ragged"),
    "original separate_ragged rg_c": lambda: original_ragged_trace("rg_c", "separate_ragged"),
}


def ragged_trace(manifest, case, entry, **kw):
    """forward_ragged / separate_ragged of a golden case's model over BATCH rows of test_gpu_ragged.ragged_lengths"""
    from sudo_rm_rf_amd import ops
    from test_gpu_ragged import ragged_lengths
    cfg, sd, _, _ = load_case(manifest, case)
    model = build(cfg, sd)
    model._engine().multi_stream = False
    x = torch.from_numpy(weights.make_mixture(BATCH, T, 9120).astype(np.float32)).to(DEV)
    with torch.no_grad(), ops.kernel_trace(DEV) as tr:
        getattr(model, entry)(x, ragged_lengths(cfg), **kw)
    return [n for n, _ in tr.launches]


IMPROVED_WALK_TRACES = {
    "train improved_pairs 0": lambda m: train_step_trace("improved_pairs", "0"),
    "train improved_d5 PYR_PER_LEVEL": lambda m: train_step_trace("improved_d5", "PYR_PER_LEVEL"),
    "train improved_d5 TRAIN_FWD_SPLIT_BF16": lambda m: train_step_trace("improved_d5", "TRAIN_FWD_SPLIT_BF16"),
    "train improved_d5 TRAIN_FWD_EXACT_MFMA": lambda m: train_step_trace("improved_d5", "TRAIN_FWD_EXACT_MFMA"),
    "tiny_groupcomm kernel_mode_1": lambda m: causal_forward_trace(*_golden_model(m, "tiny_groupcomm"), "kernel_mode_1"),
    "train groupcomm_d4 kernel_mode_1": lambda m: train_step_trace("groupcomm_d4", "kernel_mode_1"),
    "forward_ragged cfg2": lambda m: ragged_trace(m, "cfg2_improved_u16", "forward_ragged"),
    "forward_ragged cfg3": lambda m: ragged_trace(m, "cfg3_groupcomm_u8", "forward_ragged"),
    "separate_ragged cfg2 mixture_consistency": lambda m: ragged_trace(m, "cfg2_improved_u16", "separate_ragged", mixture_consistency=True),
}


EXPECTED = {
    "tiny_improved": [      # 20 launches
        (("zero_fill", "encoder", "pw_conv_generic"), 1),
        (("pw_conv_small", "dwconv5_s1_fast", "dwconv5_s2_fast", "dwconv5_generic", "merge_fast", "pw_conv_small"), 2),
        (("pw_conv_generic", "transpose", "zero_fill", "pw_conv_mfma", "overlap_add"), 1),
    ],
    "tiny_groupcomm": [      # 22 launches
        (("zero_fill", "encoder", "pw_conv_generic"), 1),
        (("tac", "pw_conv_small", "dwconv5_s1_fast", "dwconv5_s2_fast", "dwconv5_generic", "merge_fast", "pw_conv_small"), 2),
        (("pw_conv_mfma", "transpose", "zero_fill", "pw_conv_mfma", "overlap_add"), 1),
    ],
    "cfg3": [      # 55 launches
        (("zero_fill", "pack_pw_weights", "encoder", "pw_conv_x3p<1>"), 1),
        (("tac_mfma", "pw_conv_small", "pyramid_moments", "pyramid_finalize", "pyramid_merge", "pw_conv_small"), 8),
        (("pack_decoder", "pw_mask_decode", "overlap_add"), 1),
    ],
    "train": [      # 387 launches
        (("pack_pw_weights_f16", "encoder"), 1),
        (("pw_conv_mfma", "pw_conv_mfma", "pyramid_moments", "pyramid_finalize", "pyramid_merge_save"), 16),
        (("pw_conv_mfma",), 2),
        (("mask_apply", "transpose", "zero_fill", "pw_conv_bf16x3_w4", "overlap_add", "pack_pw_weights", "frames_gather",
          "pw_wgrad", "pw_wgrad_reduce", "pw_conv_bf16x3_w4", "mask_bwd", "pw_wgrad", "pw_wgrad_reduce", "transpose",
          "pw_conv_bf16x3_w4", "prelu_bwd"), 1),
        (("pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_bf16x3_w4", "gln_bwd_reduce", "gln_bwd_apply",
          "gln_bwd_reduce", "dwconv5_bwd", "dwconv5_bwd", "dwconv5_bwd", "bwd_l1h", "bwd_l0p_reduce", "bwd_l0p_apply",
          "pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_bf16x3_w4"), 16),
        (("pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_bf16x3_w4", "gln_bwd_reduce", "gln_bwd_params",
          "gln_bwd_apply"), 1),
        (("gln_bwd_params",), 3),
        (("dwconv5_bwd_params",), 2),
        (("frames_gather", "pw_wgrad", "pw_wgrad_reduce"), 1),
    ],
    "cfg2 0": [      # 71 launches
        (("zero_fill", "pack_pw_weights", "encoder", "pw_pair_x3f<1>"), 1),
        (("pyramid_moments", "pyramid_finalize", "pyramid_merge", "pw_pair_x3f<2>"), 15),
        (("pyramid_moments", "pyramid_finalize", "pyramid_merge", "pw_conv_x3p<2>", "pack_decoder", "pw_mask_decode",
          "overlap_add"), 1),
    ],
    "cfg2 NO_PAIRS": [      # 87 launches
        (("zero_fill", "pack_pw_weights", "encoder", "pw_conv_x3p<1>"), 1),
        (("pw_conv_x3p<0>", "pyramid_moments", "pyramid_finalize", "pyramid_merge", "pw_conv_x3p<2>"), 16),
        (("pack_decoder", "pw_mask_decode", "overlap_add"), 1),
    ],
    "cfg2 PYR_PER_LEVEL": [      # 135 launches
        (("zero_fill", "pack_pw_weights", "encoder", "pw_conv_x3p<1>"), 1),
        (("pw_conv_x3p<0>", "dwconv5_s1_fast", "dwconv5_s2_fast", "dwconv5_s2_fast", "dwconv5_s2_fast",
          "dwconv5_generic", "merge_fast", "pw_conv_x3p<2>"), 16),
        (("pack_decoder", "pw_mask_decode", "overlap_add"), 1),
    ],
    "cfg2 NO_PAIRS|PYR_PER_LEVEL": [      # 135 launches
        (("zero_fill", "pack_pw_weights", "encoder", "pw_conv_x3p<1>"), 1),
        (("pw_conv_x3p<0>", "dwconv5_s1_fast", "dwconv5_s2_fast", "dwconv5_s2_fast", "dwconv5_s2_fast",
          "dwconv5_generic", "merge_fast", "pw_conv_x3p<2>"), 16),
        (("pack_decoder", "pw_mask_decode", "overlap_add"), 1),
    ],
    "train improved_d5 0": [      # 96 launches
        (("encoder",), 1),
        (("pw_conv_mfma", "pw_conv_mfma", "pyramid_moments", "pyramid_finalize", "pyramid_merge_save"), 3),
        (("pw_conv_mfma",), 2),
        (("mask_apply", "transpose", "zero_fill", "pw_conv_bf16x3_w4", "overlap_add", "frames_gather", "pw_wgrad",
          "pw_wgrad_reduce", "pw_conv_bf16x3_w4", "mask_bwd", "pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_bf16x3_w4",
          "prelu_bwd"), 1),
        (("pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_bf16x3_w4", "gln_bwd_reduce", "gln_bwd_apply",
          "gln_bwd_reduce", "dwconv5_bwd", "dwconv5_bwd", "dwconv5_bwd", "bwd_l1h", "bwd_l0p_reduce", "bwd_l0p_apply",
          "pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_bf16x3_w4"), 3),
        (("pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_bf16x3_w4", "gln_bwd_reduce", "gln_bwd_params",
          "gln_bwd_apply", "gln_bwd_params", "dwconv5_bwd_params", "frames_gather", "pw_wgrad", "pw_wgrad_reduce"), 1),
    ],
    "train improved_d5 BWD_NO_FUSED_HEAD": [      # 96 launches
        (("encoder",), 1),
        (("pw_conv_mfma", "pw_conv_mfma", "pyramid_moments", "pyramid_finalize", "pyramid_merge_save"), 3),
        (("pw_conv_mfma",), 2),
        (("mask_apply", "transpose", "zero_fill", "pw_conv_bf16x3_w4", "overlap_add", "frames_gather", "pw_wgrad",
          "pw_wgrad_reduce", "pw_conv_bf16x3_w4", "mask_bwd", "pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_bf16x3_w4",
          "prelu_bwd"), 1),
        (("pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_bf16x3_w4", "gln_bwd_reduce", "gln_bwd_apply",
          "gln_bwd_reduce", "dwconv5_bwd", "dwconv5_bwd", "dwconv5_bwd", "dwconv5_bwd", "dwconv5_bwd", "gln_bwd_apply",
          "pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_bf16x3_w4"), 3),
        (("pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_bf16x3_w4", "gln_bwd_reduce", "gln_bwd_params",
          "gln_bwd_apply", "gln_bwd_params", "dwconv5_bwd_params", "frames_gather", "pw_wgrad", "pw_wgrad_reduce"), 1),
    ],
    "train improved_d5 BWD_DW_CHUNKED": [      # 126 launches
        (("encoder",), 1),
        (("pw_conv_mfma", "pw_conv_mfma", "pyramid_moments", "pyramid_finalize", "pyramid_merge_save"), 3),
        (("pw_conv_mfma",), 2),
        (("mask_apply", "transpose", "zero_fill", "pw_conv_bf16x3_w4", "overlap_add", "frames_gather", "pw_wgrad",
          "pw_wgrad_reduce", "pw_conv_bf16x3_w4", "mask_bwd", "pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_bf16x3_w4",
          "prelu_bwd"), 1),
        (("pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_bf16x3_w4", "gln_bwd_reduce", "gln_bwd_apply",
          "gln_bwd_reduce", "gln_bwd_apply", "dwconv5_bwd", "gln_bwd_reduce", "gln_bwd_apply", "dwconv5_bwd",
          "gln_bwd_reduce", "gln_bwd_apply", "dwconv5_bwd", "gln_bwd_reduce", "gln_bwd_apply", "dwconv5_bwd",
          "gln_bwd_reduce", "gln_bwd_apply", "dwconv5_bwd", "gln_bwd_reduce", "gln_bwd_apply", "pw_wgrad", "pw_wgrad_reduce",
          "transpose", "pw_conv_bf16x3_w4"), 3),
        (("pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_bf16x3_w4", "gln_bwd_reduce", "gln_bwd_params",
          "gln_bwd_apply", "gln_bwd_params", "dwconv5_bwd_params", "frames_gather", "pw_wgrad", "pw_wgrad_reduce"), 1),
    ],
    "train improved_d5 BWD_GLN_SCALAR": [      # 129 launches
        (("encoder",), 1),
        (("pw_conv_mfma", "pw_conv_mfma", "pyramid_moments", "pyramid_finalize", "pyramid_merge_save"), 3),
        (("pw_conv_mfma",), 2),
        (("mask_apply", "transpose", "zero_fill", "pw_conv_bf16x3_w4", "overlap_add", "frames_gather", "pw_wgrad",
          "pw_wgrad_reduce", "pw_conv_bf16x3_w4", "mask_bwd", "pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_bf16x3_w4",
          "prelu_bwd"), 1),
        (("pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_bf16x3_w4", "gln_bwd_reduce", "gln_bwd_apply", "merge_bwd",
          "gln_bwd_reduce", "gln_bwd_apply", "dwconv5_bwd", "gln_bwd_reduce", "gln_bwd_apply", "dwconv5_bwd",
          "gln_bwd_reduce", "gln_bwd_apply", "dwconv5_bwd", "gln_bwd_reduce", "gln_bwd_apply", "dwconv5_bwd",
          "gln_bwd_reduce", "gln_bwd_apply", "dwconv5_bwd", "gln_bwd_reduce", "gln_bwd_apply", "pw_wgrad", "pw_wgrad_reduce",
          "transpose", "pw_conv_bf16x3_w4"), 3),
        (("pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_bf16x3_w4", "gln_bwd_reduce", "gln_bwd_params",
          "gln_bwd_apply", "gln_bwd_params", "dwconv5_bwd_params", "frames_gather", "pw_wgrad", "pw_wgrad_reduce"), 1),
    ],
    "train improved_d5 kernel_mode_1": [      # 138 launches
        (("encoder",), 1),
        (("pw_conv_generic", "pw_conv_generic", "dwconv5_generic", "dwconv5_generic", "dwconv5_generic", "dwconv5_generic",
          "dwconv5_generic", "merge_generic"), 3),
        (("pw_conv_generic",), 2),
        (("mask_apply", "transpose", "zero_fill", "pw_conv_generic", "overlap_add", "frames_gather", "pw_wgrad",
          "pw_wgrad_reduce", "pw_conv_generic", "mask_bwd", "pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_generic",
          "prelu_bwd"), 1),
        (("pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_generic", "gln_bwd_reduce", "gln_bwd_apply", "merge_bwd",
          "gln_bwd_reduce", "gln_bwd_apply", "dwconv5_bwd", "gln_bwd_reduce", "gln_bwd_apply", "dwconv5_bwd",
          "gln_bwd_reduce", "gln_bwd_apply", "dwconv5_bwd", "gln_bwd_reduce", "gln_bwd_apply", "dwconv5_bwd",
          "gln_bwd_reduce", "gln_bwd_apply", "dwconv5_bwd", "gln_bwd_reduce", "gln_bwd_apply", "pw_wgrad", "pw_wgrad_reduce",
          "transpose", "pw_conv_generic"), 3),
        (("pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_generic", "gln_bwd_reduce", "gln_bwd_params", "gln_bwd_apply",
          "gln_bwd_params", "dwconv5_bwd_params", "frames_gather", "pw_wgrad", "pw_wgrad_reduce"), 1),
    ],
    "train improved_d2 0": [      # 68 launches
        (("encoder", "pw_conv_small"), 1),
        (("pw_conv_generic", "pyramid_moments", "pyramid_finalize", "pyramid_merge_save", "pw_conv_generic"), 2),
        (("pw_conv_small", "mask_apply", "transpose", "zero_fill", "pw_conv_bf16x3_w4", "overlap_add", "frames_gather",
          "pw_wgrad_small", "pw_wgrad_reduce", "pw_conv_bf16x3_w4", "mask_bwd", "pw_wgrad_small", "pw_wgrad_reduce",
          "transpose", "pw_conv_generic", "prelu_bwd"), 1),
        (("pw_wgrad_small", "pw_wgrad_reduce", "transpose", "pw_conv_generic", "gln_bwd_reduce", "gln_bwd_apply",
          "gln_bwd_reduce", "bwd_l1h", "bwd_l0p_reduce", "bwd_l0p_apply", "pw_wgrad_small", "pw_wgrad_reduce", "transpose",
          "pw_conv_generic"), 2),
        (("pw_wgrad_small", "pw_wgrad_reduce", "transpose", "pw_conv_small", "gln_bwd_reduce", "gln_bwd_params",
          "gln_bwd_apply", "gln_bwd_params", "dwconv5_bwd_params", "frames_gather", "pw_wgrad", "pw_wgrad_reduce"), 1),
    ],
    "train improved_d2_l36 0": [      # 49 launches
        (("encoder",), 1),
        (("pw_conv_small",), 2),
        (("dwconv5_s1_fast", "dwconv5_generic", "merge_fast", "pw_conv_small", "pw_conv_generic", "mask_apply", "transpose",
          "zero_fill", "pw_conv_generic", "overlap_add", "frames_gather", "pw_wgrad_small", "pw_wgrad_reduce",
          "pw_conv_generic", "mask_bwd", "pw_wgrad_small", "pw_wgrad_reduce", "transpose", "pw_conv_generic", "prelu_bwd",
          "pw_wgrad_small", "pw_wgrad_reduce", "transpose", "pw_conv_small", "gln_bwd_reduce", "gln_bwd_apply",
          "gln_bwd_reduce", "bwd_l1h", "bwd_l0p_reduce", "bwd_l0p_apply"), 1),
        (("pw_wgrad_small", "pw_wgrad_reduce", "transpose", "pw_conv_small"), 2),
        (("gln_bwd_reduce", "gln_bwd_params", "gln_bwd_apply", "gln_bwd_params", "dwconv5_bwd_params", "frames_gather",
          "pw_wgrad", "pw_wgrad_reduce"), 1),
    ],
    "train improved_d1 0": [      # 64 launches
        (("encoder", "pw_conv_small"), 1),
        (("pw_conv_generic", "dwconv5_s1_fast", "merge_fast", "pw_conv_generic"), 2),
        (("pw_conv_small", "mask_apply", "transpose", "zero_fill", "pw_conv_bf16x3_w4", "overlap_add", "frames_gather",
          "pw_wgrad_small", "pw_wgrad_reduce", "pw_conv_bf16x3_w4", "mask_bwd", "pw_wgrad_small", "pw_wgrad_reduce",
          "transpose", "pw_conv_generic", "prelu_bwd"), 1),
        (("pw_wgrad_small", "pw_wgrad_reduce", "transpose", "pw_conv_generic", "gln_bwd_reduce", "gln_bwd_apply",
          "gln_bwd_reduce", "dwconv5_bwd", "gln_bwd_apply", "pw_wgrad_small", "pw_wgrad_reduce", "transpose",
          "pw_conv_generic"), 2),
        (("pw_wgrad_small", "pw_wgrad_reduce", "transpose", "pw_conv_small", "gln_bwd_reduce", "gln_bwd_params",
          "gln_bwd_apply", "gln_bwd_params", "dwconv5_bwd_params", "frames_gather", "pw_wgrad", "pw_wgrad_reduce"), 1),
    ],
    "train groupcomm_d4 0": [      # 102 launches
        (("encoder", "pw_conv_mfma"), 1),
        (("tac", "pw_conv_small", "pyramid_moments", "pyramid_finalize", "pyramid_merge_save", "pw_conv_small"), 2),
        (("pw_conv_mfma", "mask_apply", "transpose", "zero_fill", "pw_conv_bf16x3_w4", "overlap_add", "frames_gather",
          "pw_wgrad", "pw_wgrad_reduce", "pw_conv_bf16x3_w4", "mask_bwd", "pw_wgrad", "pw_wgrad_reduce", "transpose",
          "pw_conv_bf16x3_w4", "prelu_bwd"), 1),
        (("pw_wgrad_small", "pw_wgrad_reduce", "transpose", "pw_conv_small", "gln_bwd_reduce", "gln_bwd_apply",
          "gln_bwd_reduce", "dwconv5_bwd", "dwconv5_bwd", "bwd_l1h", "bwd_l0p_reduce", "bwd_l0p_apply", "pw_wgrad_small",
          "pw_wgrad_reduce", "transpose", "pw_conv_small", "gln_bwd_reduce", "gln_bwd_params", "gln_bwd_apply", "tac_bwd",
          "pw_wgrad_small", "pw_wgrad_reduce", "pw_wgrad_small", "pw_wgrad_reduce", "pw_wgrad_small", "pw_wgrad_reduce",
          "pw_wgrad_small", "pw_wgrad_reduce", "tac_bwd_slopes", "accumulate"), 2),
        (("pw_wgrad_small", "pw_wgrad_reduce", "transpose", "pw_conv_bf16x3_w4", "gln_bwd_reduce", "gln_bwd_params",
          "gln_bwd_apply", "gln_bwd_params", "dwconv5_bwd_params", "frames_gather", "pw_wgrad", "pw_wgrad_reduce"), 1),
    ],
}


EXPECTED.update({      # recorded on commit 13ee426
    "causal_tiny 0": [      # 14 launches
        (("causal_scale", "causal_encoder", "pw_conv_bf16x3_w4"), 1),
        (("pw_conv_small", "causal_pyramid", "pw_conv_bf16x3_w4"), 2),
        (("pw_conv_mfma", "transpose", "zero_fill", "pw_conv_bf16x3_w4", "overlap_add"), 1),
    ],
    "causal_tiny PYR_PER_LEVEL": [      # 20 launches
        (("causal_scale", "causal_encoder", "pw_conv_bf16x3_w4"), 1),
        (("pw_conv_small", "causal_dwconv", "causal_dwconv", "causal_dwconv", "causal_merge", "pw_conv_bf16x3_w4"), 2),
        (("pw_conv_mfma", "transpose", "zero_fill", "pw_conv_bf16x3_w4", "overlap_add"), 1),
    ],
    "causal_tiny kernel_mode_1": [      # 20 launches
        (("causal_scale", "causal_encoder", "pw_conv_generic"), 1),
        (("pw_conv_generic", "causal_dwconv", "causal_dwconv", "causal_dwconv", "causal_merge", "pw_conv_generic"), 2),
        (("pw_conv_generic", "transpose", "zero_fill", "pw_conv_generic", "overlap_add"), 1),
    ],
    "causal_tiny_a2_k11 0": [      # 14 launches
        (("causal_scale", "causal_encoder", "pw_conv_bf16x3_w4"), 1),
        (("pw_conv_small", "causal_pyramid", "pw_conv_bf16x3_w4"), 2),
        (("pw_conv_mfma", "transpose", "zero_fill", "pw_conv_bf16x3_w4", "overlap_add"), 1),
    ],
    "causal train 0": [      # 66 launches
        (("causal_scale", "causal_encoder", "pw_conv_mfma"), 1),
        (("pw_conv_small", "causal_dwconv", "causal_dwconv", "causal_dwconv", "causal_merge_act", "pw_conv_mfma"), 2),
        (("pw_conv_mfma", "prelu_apply", "transpose", "zero_fill", "pw_conv_bf16x3_w4", "overlap_add", "causal_scale",
          "frames_gather", "prelu_apply", "pw_wgrad", "pw_wgrad_reduce", "pw_conv_mfma", "causal_prelu_bwd",
          "causal_prelu_fold", "pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_mfma", "causal_prelu_bwd",
          "causal_prelu_fold"), 1),
        (("pw_wgrad_small", "pw_wgrad_reduce", "transpose", "pw_conv_small", "causal_pyramid_bwd", "causal_bwd_finalize",
          "causal_bwd_slope", "pw_wgrad_small", "pw_wgrad_reduce", "transpose", "pw_conv_mfma"), 2),
        (("pw_wgrad_small", "pw_wgrad_reduce", "transpose", "pw_conv_small", "frames_gather", "pw_wgrad", "pw_wgrad_reduce",
          "causal_enc_scatter", "causal_gain_fold"), 1),
    ],
    "causal train PYR_PER_LEVEL": [      # 84 launches
        (("causal_scale", "causal_encoder", "pw_conv_mfma"), 1),
        (("pw_conv_small", "causal_dwconv", "causal_dwconv", "causal_dwconv", "causal_merge_act", "pw_conv_mfma"), 2),
        (("pw_conv_mfma", "prelu_apply", "transpose", "zero_fill", "pw_conv_bf16x3_w4", "overlap_add", "causal_scale",
          "frames_gather", "prelu_apply", "pw_wgrad", "pw_wgrad_reduce", "pw_conv_mfma", "causal_prelu_bwd",
          "causal_prelu_fold", "pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_mfma", "causal_prelu_bwd",
          "causal_prelu_fold"), 1),
        (("pw_wgrad_small", "pw_wgrad_reduce", "transpose", "pw_conv_small") +
         ("causal_dw_bwd", "causal_bwd_finalize", "causal_bwd_slope") * 4 +
         ("pw_wgrad_small", "pw_wgrad_reduce", "transpose", "pw_conv_mfma"), 2),
        (("pw_wgrad_small", "pw_wgrad_reduce", "transpose", "pw_conv_small", "frames_gather", "pw_wgrad", "pw_wgrad_reduce",
          "causal_enc_scatter", "causal_gain_fold"), 1),
    ],
    "causal train kernel_mode_1": [      # 84 launches
        (("causal_scale", "causal_encoder", "pw_conv_generic"), 1),
        (("pw_conv_generic", "causal_dwconv", "causal_dwconv", "causal_dwconv", "causal_merge_act", "pw_conv_generic"), 2),
        (("pw_conv_generic", "prelu_apply", "transpose", "zero_fill", "pw_conv_generic", "overlap_add", "causal_scale",
          "frames_gather", "prelu_apply", "pw_wgrad", "pw_wgrad_reduce", "pw_conv_generic", "causal_prelu_bwd",
          "causal_prelu_fold", "pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_generic", "causal_prelu_bwd",
          "causal_prelu_fold"), 1),
        (("pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_generic") +
         ("causal_dw_bwd", "causal_bwd_finalize", "causal_bwd_slope") * 4 +
         ("pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_generic"), 2),
        (("pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_generic", "frames_gather", "pw_wgrad", "pw_wgrad_reduce",
          "causal_enc_scatter", "causal_gain_fold"), 1),
    ],
    "causal stream push": [      # 11 launches
        (("stream_encoder", "stream_pw"), 1),
        (("stream_pw", "stream_pyramid", "stream_pw"), 2),
        (("stream_pw", "stream_pw", "stream_ola"), 1),
    ],
    "causal pair 0": [      # 16 launches
        (("causal_scale", "pack_pw_weights", "causal_encoder", "pw_conv_x3p<0>", "pw_conv_x3p<0>"), 1),
        (("causal_pyramid", "pw_pair_x3f<0>"), 2),
        (("causal_pyramid", "pw_conv_x3p<0>", "pw_conv_x3p<3>", "transpose", "zero_fill", "pw_conv_bf16x3_w8", "overlap_add"), 1),
    ],
    "causal pair NO_PAIRS": [      # 18 launches
        (("causal_scale", "pack_pw_weights", "causal_encoder", "pw_conv_x3p<0>"), 1),
        (("pw_conv_x3p<0>", "causal_pyramid", "pw_conv_x3p<0>"), 3),
        (("pw_conv_x3p<3>", "transpose", "zero_fill", "pw_conv_bf16x3_w8", "overlap_add"), 1),
    ],
    "attentive tiny": [      # 33 launches
        (("zero_fill", "causal_scale", "encoder", "pw_conv_bf16x3_w4"), 1),
        (("pw_conv_small", "dwconv5_s1_fast", "dwconv5_s2_fast", "dwconv5_generic", "posenc_apply", "pw_conv_generic",
          "mha_attention_mfma", "pw_conv_generic", "pw_conv_generic", "gln_apply2_add", "merge_fast", "pw_conv_bf16x3_w4"), 2),
        (("pw_conv_mfma", "transpose", "zero_fill", "pw_conv_bf16x3_w4", "overlap_add"), 1),
    ],
    "attentive wide batch 8": [      # 32 launches
        (("zero_fill", "causal_scale", "pack_pw_weights", "encoder", "pw_conv_bf16x3_w4"), 1),
        (("pw_conv_bf16x3_w4", "dwconv5_s1_fast", "dwconv5_s2_fast", "posenc_apply", "pw_conv_bf16x3_w8", "mha_attention_mfma",
          "pw_conv_bf16x3_w4", "pw_conv_bf16x3_w4", "gln_apply2_add", "merge_fast", "pw_conv_bf16x3_w4"), 2),
        (("pw_conv_bf16x3_w4", "transpose", "zero_fill", "pw_conv_bf16x3_w4", "overlap_add"), 1),
    ],
})


EXPECTED.update({      # recorded on commit 4711e9b
    "original train orig_tiny 0": [      # 132 launches
        (("zero_fill", "mask_weight_fill", "decoder_weight_expand", "encoder_bias_relu", "pw_conv_mfma"), 1),
        (("pw_conv_small", "gln_apply_c", "dwconv5_s1_fast", "dwconv5_s2_fast", "dwconv5_generic", "merge_fast",
          "gln_apply_c", "pw_conv_mfma", "gln_apply_c", "gln_apply_c"), 2),
        (("pw_conv_small", "pw_conv_mfma", "softmax_mask", "transpose", "zero_fill", "pw_conv_mfma", "overlap_add",
          "bias_rescale", "mask_weight_fill", "decoder_weight_expand", "decoder_bias_part", "decoder_bias_fold",
          "frames_gather", "pw_conv_mfma", "softmax_mask", "pw_wgrad", "pw_wgrad_reduce", "decoder_weight_contract",
          "softmax_mask_bwd", "pw_wgrad", "pw_wgrad_reduce", "mask_weight_fold", "transpose", "pw_conv_mfma"), 1),
        (("pw_wgrad_small", "pw_wgrad_reduce", "transpose", "pw_conv_mfma", "gln_c_bwd_reduce", "gln_c_bwd_apply",
          "gln_c_bwd_reduce", "gln_c_bwd_apply", "gln_apply_c", "pw_wgrad_small", "pw_wgrad_reduce", "transpose",
          "pw_conv_small", "gln_c_bwd_reduce", "gln_c_bwd_apply", "merge_bwd", "gln_apply_c", "gln_bwd_reduce",
          "gln_bwd_params", "gln_bwd_apply", "dwconv5_bwd", "dwconv5_bwd_params", "gln_bwd_reduce", "gln_bwd_params",
          "gln_bwd_apply", "dwconv5_bwd", "dwconv5_bwd_params", "gln_bwd_reduce", "gln_bwd_params", "gln_bwd_apply",
          "dwconv5_bwd", "dwconv5_bwd_params", "gln_c_bwd_reduce", "gln_c_bwd_apply"), 2),
        (("pw_wgrad_small", "pw_wgrad_reduce", "transpose", "pw_conv_mfma", "pw_wgrad_small", "pw_wgrad_reduce",
          "transpose", "pw_conv_small", "gln_bwd_reduce", "gln_bwd_params", "gln_bwd_apply", "relu_gate",
          "frames_gather", "pw_wgrad", "pw_wgrad_reduce"), 1),
    ],
    "original train orig_tiny kernel_mode_1": [      # 132 launches
        (("zero_fill", "mask_weight_fill", "decoder_weight_expand", "encoder_bias_relu", "pw_conv_generic"), 1),
        (("pw_conv_generic", "gln_apply_c_scalar", "dwconv5_generic", "dwconv5_generic", "dwconv5_generic",
          "merge_generic", "gln_apply_c_scalar", "pw_conv_generic", "gln_apply_c_scalar", "gln_apply_c_scalar"), 2),
        (("pw_conv_generic", "pw_conv_generic", "softmax_mask", "transpose", "zero_fill", "pw_conv_generic",
          "overlap_add", "bias_rescale", "mask_weight_fill", "decoder_weight_expand", "decoder_bias_part",
          "decoder_bias_fold", "frames_gather", "pw_conv_generic", "softmax_mask", "pw_wgrad", "pw_wgrad_reduce",
          "decoder_weight_contract", "softmax_mask_bwd", "pw_wgrad", "pw_wgrad_reduce", "mask_weight_fold",
          "transpose", "pw_conv_generic"), 1),
        (("pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_generic", "gln_c_bwd_reduce_scalar",
          "gln_c_bwd_apply_scalar", "gln_c_bwd_reduce_scalar", "gln_c_bwd_apply_scalar", "gln_apply_c_scalar",
          "pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_generic", "gln_c_bwd_reduce_scalar",
          "gln_c_bwd_apply_scalar", "merge_bwd", "gln_apply_c_scalar", "gln_bwd_reduce", "gln_bwd_params",
          "gln_bwd_apply", "dwconv5_bwd", "dwconv5_bwd_params", "gln_bwd_reduce", "gln_bwd_params", "gln_bwd_apply",
          "dwconv5_bwd", "dwconv5_bwd_params", "gln_bwd_reduce", "gln_bwd_params", "gln_bwd_apply", "dwconv5_bwd",
          "dwconv5_bwd_params", "gln_c_bwd_reduce_scalar", "gln_c_bwd_apply_scalar"), 2),
        (("pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_generic"), 2),
        (("gln_bwd_reduce", "gln_bwd_params", "gln_bwd_apply", "relu_gate", "frames_gather", "pw_wgrad",
          "pw_wgrad_reduce"), 1),
    ],
    "original train orig_same 0": [      # 127 launches
        (("zero_fill", "mask_weight_fill", "decoder_weight_expand", "encoder_bias_relu", "pw_conv_small"), 1),
        (("pw_conv_small", "gln_apply_c", "dwconv5_s1_fast", "dwconv5_generic", "dwconv5_generic", "merge_fast",
          "gln_apply_c", "pw_conv_mfma", "gln_apply_c", "gln_apply_c"), 2),
        (("pw_conv_small", "softmax_mask", "transpose", "zero_fill", "pw_conv_mfma", "overlap_add", "bias_rescale",
          "mask_weight_fill", "decoder_weight_expand", "decoder_bias_part", "decoder_bias_fold", "frames_gather",
          "pw_conv_mfma", "softmax_mask", "pw_wgrad_small", "pw_wgrad_reduce", "decoder_weight_contract",
          "softmax_mask_bwd", "pw_wgrad_small", "pw_wgrad_reduce", "mask_weight_fold"), 1),
        (("transpose", "pw_conv_mfma", "gln_c_bwd_reduce", "gln_c_bwd_apply", "gln_c_bwd_reduce", "gln_c_bwd_apply",
          "gln_apply_c", "pw_wgrad_small", "pw_wgrad_reduce", "transpose", "pw_conv_small", "gln_c_bwd_reduce",
          "gln_c_bwd_apply", "merge_bwd", "gln_apply_c", "gln_bwd_reduce", "gln_bwd_params", "gln_bwd_apply",
          "dwconv5_bwd", "dwconv5_bwd_params", "gln_bwd_reduce", "gln_bwd_params", "gln_bwd_apply", "dwconv5_bwd",
          "dwconv5_bwd_params", "gln_bwd_reduce", "gln_bwd_params", "gln_bwd_apply", "dwconv5_bwd",
          "dwconv5_bwd_params", "gln_c_bwd_reduce", "gln_c_bwd_apply", "pw_wgrad_small", "pw_wgrad_reduce"), 2),
        (("transpose", "pw_conv_mfma", "pw_wgrad_small", "pw_wgrad_reduce", "transpose", "pw_conv_small",
          "gln_bwd_reduce", "gln_bwd_params", "gln_bwd_apply", "relu_gate", "frames_gather", "pw_wgrad",
          "pw_wgrad_reduce"), 1),
    ],
    "original train orig_d1 0": [      # 107 launches
        (("zero_fill", "mask_weight_fill", "decoder_weight_expand", "encoder_bias_relu", "pw_conv_generic"), 1),
        (("pw_conv_generic", "gln_apply_c", "dwconv5_generic", "merge_generic", "gln_apply_c", "pw_conv_generic",
          "gln_apply_c", "gln_apply_c"), 2),
        (("pw_conv_generic", "pw_conv_generic", "softmax_mask", "transpose", "zero_fill", "pw_conv_generic",
          "overlap_add", "bias_rescale", "mask_weight_fill", "decoder_weight_expand", "decoder_bias_part",
          "decoder_bias_fold", "frames_gather", "pw_conv_generic", "softmax_mask", "pw_wgrad", "pw_wgrad_reduce",
          "decoder_weight_contract", "softmax_mask_bwd", "pw_wgrad", "pw_wgrad_reduce", "mask_weight_fold",
          "transpose", "pw_conv_generic"), 1),
        (("pw_wgrad_small", "pw_wgrad_reduce", "transpose", "pw_conv_generic", "gln_c_bwd_reduce", "gln_c_bwd_apply",
          "gln_c_bwd_reduce", "gln_c_bwd_apply", "gln_apply_c", "pw_wgrad_small", "pw_wgrad_reduce", "transpose",
          "pw_conv_generic", "gln_c_bwd_reduce", "gln_c_bwd_apply", "gln_apply_c", "gln_bwd_reduce", "gln_bwd_params",
          "gln_bwd_apply", "dwconv5_bwd", "dwconv5_bwd_params", "gln_c_bwd_reduce", "gln_c_bwd_apply"), 2),
        (("pw_wgrad_small", "pw_wgrad_reduce", "transpose", "pw_conv_generic", "gln_apply_c", "pw_wgrad_small",
          "pw_wgrad_reduce", "transpose", "pw_conv_generic", "gln_bwd_reduce", "gln_bwd_params", "gln_bwd_apply",
          "relu_gate", "frames_gather", "pw_wgrad", "pw_wgrad_reduce"), 1),
    ],
})


EXPECTED.update({      # recorded on commit 30e11c2
    "original orig_tiny 0": [      # 33 launches
        (("zero_fill", "mask_weight_fill", "decoder_weight_expand", "encoder_bias_relu", "pw_conv_bf16x3_w4"), 1),
        (("pw_conv_small", "gln_apply_c", "dwconv5_s1_fast", "dwconv5_s2_fast", "dwconv5_generic", "merge_fast",
          "gln_apply_c", "pw_conv_bf16x3_w4", "gln_apply_c", "gln_apply_c"), 2),
        (("pw_conv_small", "pw_conv_bf16x3_w4", "softmax_mask", "transpose", "zero_fill", "pw_conv_bf16x3_w4",
          "overlap_add", "bias_rescale"), 1),
    ],
    "original orig_same 0": [      # 32 launches
        (("zero_fill", "mask_weight_fill", "decoder_weight_expand", "encoder_bias_relu", "pw_conv_small"), 1),
        (("pw_conv_small", "gln_apply_c", "dwconv5_s1_fast", "dwconv5_generic", "dwconv5_generic", "merge_fast",
          "gln_apply_c", "pw_conv_bf16x3_w4", "gln_apply_c", "gln_apply_c"), 2),
        (("pw_conv_small", "softmax_mask", "transpose", "zero_fill", "pw_conv_bf16x3_w4", "overlap_add", "bias_rescale"), 1),
    ],
    "original orig_d1 0": [      # 29 launches
        (("zero_fill", "mask_weight_fill", "decoder_weight_expand", "encoder_bias_relu", "pw_conv_generic"), 1),
        (("pw_conv_generic", "gln_apply_c", "dwconv5_generic", "merge_generic", "gln_apply_c", "pw_conv_generic",
          "gln_apply_c", "gln_apply_c"), 2),
        (("pw_conv_generic", "pw_conv_generic", "softmax_mask", "transpose", "zero_fill", "pw_conv_generic",
          "overlap_add", "bias_rescale"), 1),
    ],
    "original orig_s3_k9 0": [      # 33 launches
        (("zero_fill", "mask_weight_fill", "decoder_weight_expand", "encoder_bias_relu", "pw_conv_bf16x3_w4"), 1),
        (("pw_conv_small", "gln_apply_c", "dwconv5_s1_fast", "dwconv5_generic", "dwconv5_generic", "merge_fast",
          "gln_apply_c", "pw_conv_bf16x3_w4", "gln_apply_c", "gln_apply_c"), 2),
        (("pw_conv_small", "pw_conv_bf16x3_w4", "softmax_mask", "transpose", "zero_fill", "pw_conv_generic",
          "overlap_add", "bias_rescale"), 1),
    ],
    "original orig_default_u2 0": [      # 32 launches
        (("zero_fill", "mask_weight_fill", "decoder_weight_expand", "pack_pw_weights", "encoder_bias_relu",
          "pw_conv_bf16x3_w4"), 1),
        (("pw_conv_bf16x3_w4", "gln_apply_c", "pyramid_moments", "pyramid_finalize", "pyramid_merge", "gln_apply_c",
          "pw_conv_bf16x3_w4", "gln_apply_c", "gln_apply_c"), 2),
        (("pw_conv_bf16x3_w4", "pw_conv_bf16x3_w8", "softmax_mask", "transpose", "zero_fill", "pw_conv_bf16x3_w4",
          "overlap_add", "bias_rescale"), 1),
    ],
    "original orig_tiny PYR_PER_LEVEL": [      # 33 launches
        (("zero_fill", "mask_weight_fill", "decoder_weight_expand", "encoder_bias_relu", "pw_conv_bf16x3_w4"), 1),
        (("pw_conv_small", "gln_apply_c", "dwconv5_s1_fast", "dwconv5_s2_fast", "dwconv5_generic", "merge_fast",
          "gln_apply_c", "pw_conv_bf16x3_w4", "gln_apply_c", "gln_apply_c"), 2),
        (("pw_conv_small", "pw_conv_bf16x3_w4", "softmax_mask", "transpose", "zero_fill", "pw_conv_bf16x3_w4",
          "overlap_add", "bias_rescale"), 1),
    ],
    "original orig_tiny kernel_mode_1": [      # 33 launches
        (("zero_fill", "mask_weight_fill", "decoder_weight_expand", "encoder_bias_relu", "pw_conv_generic"), 1),
        (("pw_conv_generic", "gln_apply_c_scalar", "dwconv5_generic", "dwconv5_generic", "dwconv5_generic",
          "merge_generic", "gln_apply_c_scalar", "pw_conv_generic", "gln_apply_c_scalar", "gln_apply_c_scalar"), 2),
        (("pw_conv_generic", "pw_conv_generic", "softmax_mask", "transpose", "zero_fill", "pw_conv_generic",
          "overlap_add", "bias_rescale"), 1),
    ],
    "original separate orig_tiny mixture_consistency": [      # 34 launches
        (("wav_stats", "zero_fill", "mask_weight_fill", "decoder_weight_expand", "encoder_bias_relu", "pw_conv_bf16x3_w4"), 1),
        (("pw_conv_small", "gln_apply_c", "dwconv5_s1_fast", "dwconv5_s2_fast", "dwconv5_generic", "merge_fast",
          "gln_apply_c", "pw_conv_bf16x3_w4", "gln_apply_c", "gln_apply_c"), 2),
        (("pw_conv_small", "pw_conv_bf16x3_w4", "softmax_mask", "transpose", "zero_fill", "pw_conv_bf16x3_w4",
          "overlap_add", "bias_rescale"), 1),
    ],
    "original forward_ragged rg_c": [      # 22 launches
        (("zero_fill", "mask_weight_fill", "decoder_weight_expand", "pack_pw_weights", "encoder_bias_relu_ragged",
          "pw_conv_x3w_ragged<1>", "pw_conv_x3w_ragged<0>", "gln_apply_c_ragged", "pyramid_moments_ragged",
          "pyramid_finalize_ragged", "pyramid_merge_ragged", "gln_apply_c_ragged", "pw_conv_x3w_ragged<0>",
          "gln_apply_c_ragged", "gln_apply_c_ragged", "pw_conv_x3w_ragged<0>", "softmax_mask_ragged", "transpose",
          "zero_fill", "pw_conv_bf16x3_w4", "overlap_add_ragged", "bias_rescale_ragged"), 1),
    ],
    "original separate_ragged rg_c": [      # 23 launches
        (("wav_stats_ragged", "zero_fill", "mask_weight_fill", "decoder_weight_expand", "pack_pw_weights",
          "encoder_bias_relu_ragged", "pw_conv_x3w_ragged<1>", "pw_conv_x3w_ragged<0>", "gln_apply_c_ragged",
          "pyramid_moments_ragged", "pyramid_finalize_ragged", "pyramid_merge_ragged", "gln_apply_c_ragged",
          "pw_conv_x3w_ragged<0>", "gln_apply_c_ragged", "gln_apply_c_ragged", "pw_conv_x3w_ragged<0>",
          "softmax_mask_ragged", "transpose", "zero_fill", "pw_conv_bf16x3_w4", "overlap_add_ragged",
          "bias_rescale_ragged"), 1),
    ],
})


EXPECTED.update({      # recorded on commit 2377517
    "train improved_pairs 0": [      # 62 launches
        (("pack_pw_weights_f16", "encoder", "pw_pair_x3f4<1>", "pyramid_moments", "pyramid_finalize",
          "pyramid_merge_save", "pw_pair_x3f4<2>", "pyramid_moments", "pyramid_finalize", "pyramid_merge_save",
          "pw_conv_x3w4<2>", "pw_conv_x3w4<3>", "mask_apply", "transpose", "zero_fill", "pw_conv_bf16x3_w8",
          "overlap_add", "pack_pw_weights", "frames_gather", "pw_wgrad", "pw_wgrad_reduce", "pw_conv_bf16x3_w8",
          "mask_bwd", "pw_wgrad", "pw_wgrad_reduce", "pw_conv_x3w<0>", "prelu_bwd", "pw_wgrad", "pw_wgrad_reduce",
          "pw_conv_x3w<0>", "gln_bwd_reduce", "gln_bwd_apply", "gln_bwd_reduce", "bwd_l1h", "bwd_l0p_reduce",
          "bwd_l0p_apply", "pw_wgrad", "pw_wgrad_reduce", "pw_pair_x3f<0>", "pw_wgrad", "pw_wgrad_reduce",
          "gln_bwd_reduce", "gln_bwd_apply", "gln_bwd_reduce", "bwd_l1h", "bwd_l0p_reduce", "bwd_l0p_apply", "pw_wgrad",
          "pw_wgrad_reduce", "pw_conv_x3w<0>", "pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_bf16x3_w8",
          "gln_bwd_reduce", "gln_bwd_params", "gln_bwd_apply", "gln_bwd_params", "dwconv5_bwd_params", "frames_gather",
          "pw_wgrad", "pw_wgrad_reduce"), 1),
    ],
    "train improved_d5 PYR_PER_LEVEL": [      # 105 launches
        (("encoder",), 1),
        (("pw_conv_mfma", "pw_conv_mfma", "dwconv5_s1_fast", "dwconv5_s2_fast", "dwconv5_s2_fast", "dwconv5_s2_fast",
          "dwconv5_generic", "merge_fast"), 3),
        (("pw_conv_mfma",), 2),
        (("mask_apply", "transpose", "zero_fill", "pw_conv_bf16x3_w4", "overlap_add", "frames_gather", "pw_wgrad",
          "pw_wgrad_reduce", "pw_conv_bf16x3_w4", "mask_bwd", "pw_wgrad", "pw_wgrad_reduce", "transpose",
          "pw_conv_bf16x3_w4", "prelu_bwd"), 1),
        (("pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_bf16x3_w4", "gln_bwd_reduce", "gln_bwd_apply",
          "gln_bwd_reduce", "dwconv5_bwd", "dwconv5_bwd", "dwconv5_bwd", "bwd_l1h", "bwd_l0p_reduce", "bwd_l0p_apply",
          "pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_bf16x3_w4"), 3),
        (("pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_bf16x3_w4", "gln_bwd_reduce", "gln_bwd_params",
          "gln_bwd_apply", "gln_bwd_params", "dwconv5_bwd_params", "frames_gather", "pw_wgrad", "pw_wgrad_reduce"), 1),
    ],
    "train improved_d5 TRAIN_FWD_SPLIT_BF16": [      # 96 launches
        (("encoder",), 1),
        (("pw_conv_bf16x3_w4", "pw_conv_bf16x3_w4", "pyramid_moments", "pyramid_finalize", "pyramid_merge_save"), 3),
        (("pw_conv_bf16x3_w4",), 2),
        (("mask_apply", "transpose", "zero_fill", "pw_conv_bf16x3_w4", "overlap_add", "frames_gather", "pw_wgrad",
          "pw_wgrad_reduce", "pw_conv_bf16x3_w4", "mask_bwd", "pw_wgrad", "pw_wgrad_reduce", "transpose",
          "pw_conv_bf16x3_w4", "prelu_bwd"), 1),
        (("pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_bf16x3_w4", "gln_bwd_reduce", "gln_bwd_apply",
          "gln_bwd_reduce", "dwconv5_bwd", "dwconv5_bwd", "dwconv5_bwd", "bwd_l1h", "bwd_l0p_reduce", "bwd_l0p_apply",
          "pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_bf16x3_w4"), 3),
        (("pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_bf16x3_w4", "gln_bwd_reduce", "gln_bwd_params",
          "gln_bwd_apply", "gln_bwd_params", "dwconv5_bwd_params", "frames_gather", "pw_wgrad", "pw_wgrad_reduce"), 1),
    ],
    "train improved_d5 TRAIN_FWD_EXACT_MFMA": [      # 96 launches
        (("encoder",), 1),
        (("pw_conv_mfma", "pw_conv_mfma", "pyramid_moments", "pyramid_finalize", "pyramid_merge_save"), 3),
        (("pw_conv_mfma",), 2),
        (("mask_apply", "transpose", "zero_fill", "pw_conv_bf16x3_w4", "overlap_add", "frames_gather", "pw_wgrad",
          "pw_wgrad_reduce", "pw_conv_bf16x3_w4", "mask_bwd", "pw_wgrad", "pw_wgrad_reduce", "transpose",
          "pw_conv_bf16x3_w4", "prelu_bwd"), 1),
        (("pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_bf16x3_w4", "gln_bwd_reduce", "gln_bwd_apply",
          "gln_bwd_reduce", "dwconv5_bwd", "dwconv5_bwd", "dwconv5_bwd", "bwd_l1h", "bwd_l0p_reduce", "bwd_l0p_apply",
          "pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_bf16x3_w4"), 3),
        (("pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_bf16x3_w4", "gln_bwd_reduce", "gln_bwd_params",
          "gln_bwd_apply", "gln_bwd_params", "dwconv5_bwd_params", "frames_gather", "pw_wgrad", "pw_wgrad_reduce"), 1),
    ],
    "tiny_groupcomm kernel_mode_1": [      # 24 launches
        (("zero_fill", "encoder"), 1),
        (("pw_conv_generic", "tac", "gln_apply_add", "pw_conv_generic", "dwconv5_generic", "dwconv5_generic",
          "dwconv5_generic", "merge_generic"), 2),
        (("pw_conv_generic",), 2),
        (("transpose", "zero_fill", "pw_conv_generic", "overlap_add"), 1),
    ],
    "train groupcomm_d4 kernel_mode_1": [      # 126 launches
        (("encoder",), 1),
        (("pw_conv_generic", "tac", "gln_apply_add", "pw_conv_generic", "dwconv5_generic", "dwconv5_generic",
          "dwconv5_generic", "dwconv5_generic", "merge_generic"), 2),
        (("pw_conv_generic",), 2),
        (("mask_apply", "transpose", "zero_fill", "pw_conv_generic", "overlap_add", "frames_gather", "pw_wgrad",
          "pw_wgrad_reduce", "pw_conv_generic", "mask_bwd", "pw_wgrad", "pw_wgrad_reduce", "transpose",
          "pw_conv_generic", "prelu_bwd"), 1),
        (("pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_generic", "gln_bwd_reduce", "gln_bwd_apply", "merge_bwd",
          "gln_bwd_reduce", "gln_bwd_apply", "dwconv5_bwd", "gln_bwd_reduce", "gln_bwd_apply", "dwconv5_bwd",
          "gln_bwd_reduce", "gln_bwd_apply", "dwconv5_bwd", "gln_bwd_reduce", "gln_bwd_apply", "dwconv5_bwd",
          "gln_bwd_reduce", "gln_bwd_apply", "pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_generic",
          "gln_bwd_reduce", "gln_bwd_params", "gln_bwd_apply", "tac_bwd", "pw_wgrad", "pw_wgrad_reduce", "pw_wgrad",
          "pw_wgrad_reduce", "pw_wgrad", "pw_wgrad_reduce", "pw_wgrad", "pw_wgrad_reduce", "tac_bwd_slopes",
          "accumulate"), 2),
        (("pw_wgrad", "pw_wgrad_reduce", "transpose", "pw_conv_generic", "gln_bwd_reduce", "gln_bwd_params",
          "gln_bwd_apply", "gln_bwd_params", "dwconv5_bwd_params", "frames_gather", "pw_wgrad", "pw_wgrad_reduce"), 1),
    ],
    "forward_ragged cfg2": [      # 71 launches
        (("zero_fill", "pack_pw_weights", "encoder_ragged", "pw_pair_x3f_ragged<1>"), 1),
        (("pyramid_moments_ragged", "pyramid_finalize_ragged", "pyramid_merge_ragged", "pw_pair_x3f_ragged<2>"), 15),
        (("pyramid_moments_ragged", "pyramid_finalize_ragged", "pyramid_merge_ragged", "pw_conv_x3w_ragged<2>",
          "pack_decoder", "pw_mask_decode", "overlap_add_ragged"), 1),
    ],
    "forward_ragged cfg3": [      # 55 launches
        (("zero_fill", "pack_pw_weights", "encoder_ragged", "pw_conv_x3w_ragged<1>"), 1),
        (("tac_mfma_ragged", "pw_conv_small_ragged", "pyramid_moments_ragged", "pyramid_finalize_ragged",
          "pyramid_merge_ragged", "pw_conv_small_ragged"), 8),
        (("pack_decoder", "pw_mask_decode", "overlap_add_ragged"), 1),
    ],
    "separate_ragged cfg2 mixture_consistency": [      # 72 launches
        (("wav_stats_ragged", "zero_fill", "pack_pw_weights", "encoder_ragged", "pw_pair_x3f_ragged<1>"), 1),
        (("pyramid_moments_ragged", "pyramid_finalize_ragged", "pyramid_merge_ragged", "pw_pair_x3f_ragged<2>"), 15),
        (("pyramid_moments_ragged", "pyramid_finalize_ragged", "pyramid_merge_ragged", "pw_conv_x3w_ragged<2>",
          "pack_decoder", "pw_mask_decode", "overlap_add_ragged"), 1),
    ],
})


def _check(name, got):
    want = _expand(EXPECTED[name])
    first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    assert got == want, "%s: %d launches (expected %d), first difference at launch %d: got %s, expected %s" % (
        name, len(got), len(want), first, got[first:first + 4], want[first:first + 4])


@pytest.mark.parametrize("fn", [trace_tiny_improved, trace_tiny_groupcomm, trace_cfg3, trace_train],
                         ids=["tiny_improved", "tiny_groupcomm", "cfg3_groupcomm_u8", "train_cfg2_shape"])
def test_launch_sequence(manifest, fn):
    _check(fn.__name__[len("trace_"):], fn(manifest))


@pytest.mark.parametrize("flags", ["0", "NO_PAIRS", "PYR_PER_LEVEL", "NO_PAIRS|PYR_PER_LEVEL"])
def test_launch_sequence_cfg2_under_debug_flags(cfg2, flags):
    from sudo_rm_rf_amd import ops
    value = sum(int(getattr(ops.DebugFlag, f)) for f in flags.split("|")) if flags != "0" else 0
    _check("cfg2 " + flags, _forward_trace(*cfg2, flags=value))


@pytest.mark.parametrize("shape,setting", TRAIN_STEPS, ids=["%s-%s" % s for s in TRAIN_STEPS])
def test_launch_sequence_of_a_training_step(shape, setting):
    _check("train %s %s" % (shape, setting), train_step_trace(shape, setting))


@pytest.mark.parametrize("name", list(CAUSAL_TRACES))
def test_launch_sequence_of_the_causal_and_attentive_walks(name):
    _check(name, CAUSAL_TRACES[name]())


@pytest.mark.parametrize("name", list(ORIGINAL_TRACES))
def test_launch_sequence_of_the_original_inference_and_ragged_walks(name):
    _check(name, ORIGINAL_TRACES[name]())


@pytest.mark.parametrize("name", list(IMPROVED_WALK_TRACES))
def test_launch_sequence_of_the_improved_walk_branches(manifest, name):
    got = IMPROVED_WALK_TRACES[name](manifest)
    if name == "train improved_pairs 0":      # the shape is the right one: one forward pair per block
        assert sum(1 for n in got if n.startswith("pw_pair_x3f4<")) == TRAIN_SHAPES["improved_pairs"][0].num_blocks
    if name.endswith("kernel_mode_1"):        # ... and these take the branch without the pre-add
        assert "gln_apply_add" in got
    _check(name, got)
