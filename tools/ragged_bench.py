#!/usr/bin/env python
"""Ragged-batch forward against what it replaces, on one MI355X: cfg 2 weights (--model improved, the default), cfg 3
weights (--model groupcomm) or the original model in the README recipe's configuration, 16 blocks, opted in with
enable_ragged() (--model original), batch 32, T = 32000, seeded lengths uniform on [T/2, T].  In ONE process, warmed up,
alternating, timed with device events:

  (a) model.forward_ragged(x, lengths)                       one set of launches, single stream
  (b) the 32 batch-1 forwards it replaces                    each at its own length; all plans made in the warm-up and held (asserted)
  (c) model(x): the uniform forward of the batch padded to T a COST CEILING only -- it is not a correct answer
  (d) (c) again                                              the A/A spread of (c) is the margin for "(a) no slower than (c)"
  (c1) (c) on a single stream                                 what (a), which does not split the batch over two streams, is built like

Writes profiles/ragged_forward.txt (--model groupcomm: profiles/ragged_forward_groupcomm.txt, --model original:
profiles/ragged_forward_original.txt), or --out.  The Improved mode exits 1 unless (a) beats (b) and is no slower than (c) by
more than the spread; the GroupComm and original modes only report -- for those models the comparison that matters is (a)
against (b), the per-utterance path separate_list took before.  The original mode also lists the launches of one call of (a),
of one batch-1 forward of (b) and of (c).  --model attentive: attentive v2 at the reference defaults (16 blocks), opted in with
enable_ragged(); writes profiles/ragged_forward_attentive.txt, only reports, and adds the per-kernel table of one ragged call
and the work ratio; the padded uniform forward (c) is a floor there, not a correct answer.

--mode separate_list: pipeline.separate_list on a length-sorted list of 32 utterances, lengths on [T/2, T], both models
(--model picks one), two arms in one process, alternating, device events, median over the rounds:

  (s) pipeline.separate_list: ragged.wav_gather + model.separate_ragged, the recipe inside the kernels
  (p) the recipe as torch operators around the unchanged model.forward_ragged -- a zeroed padded tensor, mean / std / normalise /
      slice-assign per utterance, and after the forward the rescale and the mixture consistency per utterance -- restated here

with the library's launches (ops.kernel_trace) and the ATen operators that launch a kernel (a TorchDispatchMode count; views
and allocations left out) of one call of each arm.  The arms are not symmetric: (s) is the whole of separate_list, its Python
sort, bucketing and plan lookup included; (p) only the recipe on the batch already sorted and bucketed -- the ratio understates
the gain.  Writes profiles/ragged_separate_list.txt (--model original / attentive: profiles/ragged_separate_list_<model>.txt), or --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def load_original(dev):
    """the original model, README recipe with 16 blocks, seeded fixture weights, opted into the ragged forward"""
    from tests import original_fixtures as of
    from sudo_rm_rf.dnn.models.sudormrf import SuDORMRF
    model = SuDORMRF(**of.RECIPE)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in of.make_state_dict(of.RECIPE, 408).items()})
    return model.to(dev).eval().enable_ragged()


def load_attentive(dev):
    """attentive v2, the reference defaults (16 blocks), seeded fixture weights, opted into the ragged forward"""
    from tests import attentive_fixtures as af
    from sudo_rm_rf_amd.dnn.models.attentive_sudormrf_v2 import SuDORMRF
    cfg = dict(af.DEFAULT_U2, num_blocks=16)
    model = SuDORMRF(**cfg)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in af.make_state_dict(cfg, 409).items()})
    return model.to(dev).eval().enable_ragged()


OPT_IN = {"original": "original model (README recipe, 16 blocks)", "attentive": "attentive v2 (reference defaults, 16 blocks)"}


def load_model(gc, dev):
    """cfg 3 (GroupComm) or cfg 2 (Improved) with the golden weights, in eval mode on `dev`; gc == "original": load_original;
    gc == "attentive": load_attentive"""
    if gc == "original":
        return load_original(dev)
    if gc == "attentive":
        return load_attentive(dev)
    from oracle import weights
    from oracle.schema import ModelConfig
    import sudo_rm_rf.dnn.models.groupcomm_sudormrf_v2 as groupcomm_sudormrf_v2
    import sudo_rm_rf.dnn.models.improved_sudormrf as improved_sudormrf
    case = "cfg3_groupcomm_u8" if gc else "cfg2_improved_u16"
    man = json.load(open(os.path.join(ROOT, "tests", "golden", "MANIFEST.json")))["cases"][case]
    cfg = ModelConfig(**man["config"])
    sd = weights.make_state_dict(cfg, man["weight_seed"])
    model = (groupcomm_sudormrf_v2.GroupCommSudoRmRf if gc else improved_sudormrf.SuDORMRF)(**cfg.ctor_kwargs())
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return model.to(dev).eval()


def torch_op_recipe(model, mixes, mixture_consistency, T):
    """Arm (p): one length-sorted ragged batch the way separate_list ran it before separate_ragged existed -- the recipe as torch
    operators per utterance around model.forward_ragged."""
    lens = [m.numel() for m in mixes]
    x = torch.zeros((len(mixes), 1, T), dtype=torch.float32, device=mixes[0].device)
    stats = []
    for r, m in enumerate(mixes):
        mean, std = m.mean(), m.std()
        x[r, 0, :lens[r]] = (m - mean) / (std + 1e-9)
        stats.append((mean, std))
    est = model.forward_ragged(x, lens)
    out = []
    for r in range(len(mixes)):
        e = est[r, :, :lens[r]] * stats[r][1] + stats[r][0]
        if mixture_consistency:
            e = e + (x[r, :, :lens[r]] - e.sum(0, keepdim=True)) / e.shape[0]
        out.append(e)
    return out


# ATen operators that launch no kernel: views, allocations, metadata
_NO_KERNEL = {"empty", "empty_like", "empty_strided", "select", "slice", "view", "_unsafe_view", "reshape", "unsqueeze", "squeeze",
              "expand", "detach", "alias", "as_strided", "t", "transpose", "permute", "_to_copy", "lift_fresh", "resize_"}


def count_launches(fn, dev):
    """(library launches by name, kernel-launching ATen operators by name) of one call of fn"""
    from collections import Counter
    from torch.utils._python_dispatch import TorchDispatchMode
    from sudo_rm_rf_amd import ops
    aten = Counter()

    class Count(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            name = func.overloadpacket.__name__
            if name not in _NO_KERNEL:
                aten[name] += 1
            return func(*args, **(kwargs or {}))

    with ops.kernel_trace(dev) as tr, Count():
        fn()
    return Counter(n for n, _ in tr.launches), aten


def separate_list_mode(args):
    from oracle import weights
    from sudo_rm_rf_amd import pipeline
    dev = torch.device("cuda:0")
    B, T = args.batch, args.T
    lines = ["separate_list on one ragged batch: %d utterances, lengths uniform on [T/2, T], T = %d (seed 2026), sorted by length"
             % (B, T),
             "device: %s; %d alternating rounds after %d warm-up rounds; device-event times in ms: median [min .. max]"
             % (torch.cuda.get_device_name(dev), args.rounds, args.warmup),
             "(s) pipeline.separate_list: wav_gather + separate_ragged    (p) the recipe as torch operators around forward_ragged",
             "(s) times the whole call, its sort, bucketing and plan lookup included; (p) only the recipe on the sorted batch"]
    rng = np.random.default_rng(2026)
    lens = sorted(int(v) for v in rng.integers(T // 2, T + 1, B))
    gain = np.geomspace(0.05, 20.0, B)[rng.permutation(B)]
    for gc in ([False, True] if args.model is None else [args.model if args.model in OPT_IN else args.model == "groupcomm"]):
        model = load_model(gc, dev)
        mixes = [torch.from_numpy((gain[i] * weights.make_mixture(1, n, 9400 + i)[0, 0] + 0.1).astype(np.float32)).to(dev)
                 for i, n in enumerate(lens)]
        (idx, Tb), = pipeline.ragged_batches(lens, B)
        assert idx == list(range(B)) and model._engine().ragged_plan_supported(B, Tb, dev)
        runs = [("s", lambda: pipeline.separate_list(model, mixes, max_batch=B)),
                ("p", lambda: torch_op_recipe(model, mixes, gc is True, Tb))]
        times = {k: [] for k, _ in runs}
        with torch.no_grad():
            for _ in range(args.warmup):
                for _, fn in runs:
                    fn()
            torch.cuda.synchronize()
            got, want = runs[0][1](), runs[1][1]()
            worst = max(float((g - w).abs().max()) / max(1.0, float(m.std())) for g, w, m in zip(got, want, mixes))
            counts = {k: count_launches(fn, dev) for k, fn in runs}
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for k, fn in runs:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    times[k].append(e0.elapsed_time(e1))
        med = {k: float(np.median(v)) for k, v in times.items()}
        lines.append("")
        lines.append("%s weights, mixture consistency %s, padded length %d: %.1f %% of the padded samples are real"
                     % (OPT_IN[gc] if gc in OPT_IN else "cfg 3 (GroupComm)" if gc else "cfg 2 (Improved)",
                        "on" if gc is True else "off", Tb, 100 * sum(lens) / float(B * Tb)))
        lines.append("max |(s) - (p)| / max(1, std) over the utterances: %.3e" % worst)
        for k, name in (("s", "(s) separate_list"), ("p", "(p) torch-operator recipe")):
            lib, aten = counts[k]
            lines.append("%-28s %8.3f [%8.3f .. %8.3f]   library launches %3d, ATen operators with a kernel %4d"
                         % (name, med[k], min(times[k]), max(times[k]), sum(lib.values()), sum(aten.values())))
        lines.append("(p) / (s) = %.2f;  (s) faster than (p): %s" % (med["p"] / med["s"], med["s"] < med["p"]))
        lines.append("ATen operators of (s): %s" % (dict(counts["s"][1]) or "none"))
        lines.append("ATen operators of (p): %s" % dict(counts["p"][1]))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--T", type=int, default=32000)
    ap.add_argument("--mode", choices=["forward", "separate_list"], default="forward")
    ap.add_argument("--model", choices=["improved", "groupcomm", "original", "attentive"], default=None,
                    help="default: improved (--mode forward), both in turn (--mode separate_list)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.mode == "separate_list":
        if args.out is None:
            args.out = os.path.join(ROOT, "profiles", "ragged_separate_list_%s.txt" % args.model if args.model in OPT_IN
                                    else "ragged_separate_list.txt")
        return separate_list_mode(args)
    gc = args.model if args.model in OPT_IN else args.model == "groupcomm"
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "ragged_forward_%s.txt" % gc if gc in OPT_IN else
                                "ragged_forward_groupcomm.txt" if gc else "ragged_forward.txt")
    from oracle import weights
    dev = torch.device("cuda:0")
    model = load_model(gc, dev)
    B, T = args.batch, args.T
    rng = np.random.default_rng(2026)
    lens = [int(v) for v in rng.integers(T // 2, T + 1, B)]
    x = torch.from_numpy(weights.make_mixture(B, T, 9400).astype(np.float32)).to(dev)
    rows = [x[i:i + 1, :, :n].contiguous() for i, n in enumerate(lens)]
    # (b) walks 32 distinct lengths = 32 plans, next to the (B, T) plans of (a), (c), (c1) and their stream lanes: the engine's
    # plan cache must hold them ALL for the whole run, or every batch-1 call would re-create its plan inside the timed region
    from sudo_rm_rf_amd import engine as engine_mod
    engine_mod._MAX_PLANS = max(engine_mod._MAX_PLANS, 4 * B + 16)
    engine_mod._MAX_WORKSPACE_BYTES = max(engine_mod._MAX_WORKSPACE_BYTES, 64 << 30)
    created = [0]
    plan_init = engine_mod.Plan.__init__

    def counting_init(self, *a, **kw):
        created[0] += 1
        plan_init(self, *a, **kw)

    engine_mod.Plan.__init__ = counting_init
    eng = model._engine()
    assert eng.ragged_plan_supported(B, T, dev)

    def run_a():
        return model.forward_ragged(x, lens)

    def run_b():
        return [model(r) for r in rows]

    def run_c():
        return model(x)

    def run_c1():
        was = eng.multi_stream          # (the original model's engine is single-stream to begin with)
        eng.multi_stream = False
        try:
            return model(x)
        finally:
            eng.multi_stream = was

    runs = [("a", run_a), ("b", run_b), ("c", run_c), ("d", run_c), ("c1", run_c1)]
    times = {k: [] for k, _ in runs}
    with torch.no_grad():
        for _ in range(args.warmup):
            for _, fn in runs:
                fn()
        torch.cuda.synchronize()
        # sanity: the ragged rows are the batch-1 answers
        got, want = run_a(), run_b()
        worst = max(float((got[i, :, :n] - want[i][0]).abs().max()) for i, n in enumerate(lens))
        launches = {k: count_launches(fn, dev)[0] for k, fn in (("a", run_a), ("b1", lambda: model(rows[0])), ("c", run_c))} \
            if gc in OPT_IN else None
        # --model attentive: the per-kernel table of one ragged call (in-library profiler: one interval per launch)
        table = None
        if gc == "attentive":
            from sudo_rm_rf_amd import ops
            with ops.kernel_trace(dev) as tr:
                run_a()
            table = {}
            for n, ms in tr.launches:
                cnt, tot = table.get(n, (0, 0.0))
                table[n] = (cnt + 1, tot + ms)
        made_in_warmup = created[0]
        for _ in range(args.rounds):
            for k, fn in runs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1))
    assert created[0] == made_in_warmup, "%d plans were created inside the timed rounds" % (created[0] - made_in_warmup)
    med = {k: float(np.median(v)) for k, v in times.items()}
    spread = abs(med["c"] - med["d"])
    valid = sum(lens) / float(B * T)
    lines = ["ragged forward, %s weights, batch %d, T = %d, lengths uniform on [T/2, T] (seed 2026): %.1f %% of the padded samples are real"
             % (OPT_IN[gc] if gc in OPT_IN else "cfg 3 (GroupComm)" if gc else "cfg 2", B, T, 100 * valid),
             "device: %s; %d alternating rounds after %d warm-up rounds; device-event times in ms: median [min .. max]"
             % (torch.cuda.get_device_name(dev), args.rounds, args.warmup),
             "max |forward_ragged row - its batch-1 forward| over the batch: %.3e" % worst,
             "plans created before the timed rounds: %d, inside them: 0" % made_in_warmup]
    names = {"a": "(a)  forward_ragged", "b": "(b)  %d batch-1 forwards" % B, "c": "(c)  uniform forward, padded to T",
             "d": "(d)  (c) again (A/A)", "c1": "(c1) (c) on a single stream"}
    for k, _ in runs:
        lines.append("%-36s %8.3f [%8.3f .. %8.3f]" % (names[k], med[k], min(times[k]), max(times[k])))
    lines.append("A/A spread of (c): %.3f ms" % spread)
    lines.append("(b) / (a) = %.2f   (a) / (c) = %.3f   (a) / (c1) = %.3f" % (med["b"] / med["a"], med["a"] / med["c"], med["a"] / med["c1"]))
    lines.append("(a) faster than (b): %s;  (a) no slower than (c) by more than the spread: %s"
                 % (med["a"] < med["b"], med["a"] <= med["c"] + spread))
    if launches:
        lines.append("library launches: (a) %d, one batch-1 forward of (b) %d (x %d = %d), (c) %d"
                     % (sum(launches["a"].values()), sum(launches["b1"].values()), B, B * sum(launches["b1"].values()),
                        sum(launches["c"].values())))
        lines.append("launches of (a): %s" % dict(sorted(launches["a"].items())))
    if table:
        total = sum(ms for _, ms in table.values())
        lines.append("")
        lines.append("one ragged call under the in-library profiler (per launch intervals, serialised): %.3f ms in %d launches"
                     % (total, sum(c for c, _ in table.values())))
        lines.append("%-32s %8s %10s %7s" % ("kernel", "launches", "ms", "share"))
        for n, (cnt, ms) in sorted(table.items(), key=lambda kv: -kv[1][1]):
            lines.append("%-32s %8d %10.3f %6.1f%%" % (n, cnt, ms, 100 * ms / total))
        # work ratio: 128-column GEMM tiles that hold own columns / tiles of the padded batch, at full length -- frames from the
        # model's own hop, depth and padding rule (every row padded alone, as its batch-1 forward pads it)
        hop, deep, tile = model.enc_kernel_size // 2, model.upsampling_depth - 1, 128
        padded = lambda n: model.pad_to_appropriate_length(torch.zeros(1, 1, n)).shape[-1]
        L = padded(T) // hop
        fr = [padded(n) // hop for n in lens]
        tiles = sum(-(-f // tile) for f in fr) / float(B * -(-L // tile))
        lines.append("work ratio: real samples / padded samples = %.3f; %d-column tiles that hold own columns / all tiles = %.3f "
                     "(full length; the deepest level, %d columns, has %d tile(s) per row)"
                     % (valid, tile, tiles, L >> deep, -(-(L >> deep) // tile)))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    if gc is False and not (med["a"] < med["b"] and med["a"] <= med["c"] + spread):
        sys.exit(1)


if __name__ == "__main__":
    main()
