#!/usr/bin/env python
"""Ragged-batch forward against what it replaces, on one MI355X: cfg 2 weights (--model improved, the default) or cfg 3
weights (--model groupcomm), batch 32, T = 32000, seeded lengths uniform on [T/2, T].  In ONE process, warmed up,
alternating, timed with device events:

  (a) model.forward_ragged(x, lengths)                       one set of launches, single stream
  (b) the 32 batch-1 forwards it replaces                    each at its own length; all plans made in the warm-up and held (asserted)
  (c) model(x): the uniform forward of the batch padded to T a COST CEILING only -- it is not a correct answer
  (d) (c) again                                              the A/A spread of (c) is the margin for "(a) no slower than (c)"
  (c1) (c) on a single stream                                 what (a), which does not split the batch over two streams, is built like

Writes profiles/ragged_forward.txt (--model groupcomm: profiles/ragged_forward_groupcomm.txt), or --out.  The Improved mode
exits 1 unless (a) beats (b) and is no slower than (c) by more than the spread; the GroupComm mode only reports -- for that
model the comparison that matters is (a) against (b), the per-utterance path separate_list took before."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--T", type=int, default=32000)
    ap.add_argument("--model", choices=["improved", "groupcomm"], default="improved")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    gc = args.model == "groupcomm"
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "ragged_forward_groupcomm.txt" if gc else "ragged_forward.txt")
    from oracle import weights
    from oracle.schema import ModelConfig
    import sudo_rm_rf.dnn.models.groupcomm_sudormrf_v2 as groupcomm_sudormrf_v2
    import sudo_rm_rf.dnn.models.improved_sudormrf as improved_sudormrf
    case = "cfg3_groupcomm_u8" if gc else "cfg2_improved_u16"
    man = json.load(open(os.path.join(ROOT, "tests", "golden", "MANIFEST.json")))["cases"][case]
    cfg = ModelConfig(**man["config"])
    sd = weights.make_state_dict(cfg, man["weight_seed"])
    dev = torch.device("cuda:0")
    model = (groupcomm_sudormrf_v2.GroupCommSudoRmRf if gc else improved_sudormrf.SuDORMRF)(**cfg.ctor_kwargs())
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model = model.to(dev).eval()
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
        eng.multi_stream = False
        try:
            return model(x)
        finally:
            eng.multi_stream = True

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
             % ("cfg 3 (GroupComm)" if gc else "cfg 2", B, T, 100 * valid),
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
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    if not gc and not (med["a"] < med["b"] and med["a"] <= med["c"] + spread):
        sys.exit(1)


if __name__ == "__main__":
    main()
