#!/usr/bin/env python3
"""Time the attentive SuDoRM-RF (v2 or v3) inference forward on one MI355X.

    python tools/attentive_bench.py [--model v2|v3] [--blocks 16] [--batch 32] [--time 32000] [--steps 10] [--warmup 3]

Prints, for the reference's default configuration (128 / 512 channels, depth 4, 4 heads of 256): the forward time at the
given batch and at batch 1 (device events around `steps` forwards), the per-kernel table of one forward (the library's
srf_profile_* marks), the attention kernel's time and TFLOP/s against the 155 TFLOP/s the exact-fp32 MFMA measures on this
part, and the share of the per-level pyramid (depthwise levels + merge).  Weights: the seeded constructor's.
--model v3: attentive_sudormrf_v3 -- D - 1 attentions per block, level D - 2 - r asking level D - 1 - r (ceil halving)."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TF = 155.0


def timed(model, x, steps, warmup):
    with torch.no_grad():
        for _ in range(warmup):
            model(x)
        beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        beg.record()
        for _ in range(steps):
            model(x)
        end.record()
    torch.cuda.synchronize()
    return beg.elapsed_time(end) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("v2", "v3"), default="v2")
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--time", type=int, default=32000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from sudo_rm_rf_amd import ops
    v3 = a.model == "v3"
    if v3:
        from sudo_rm_rf_amd.dnn.models.attentive_sudormrf_v3 import SuDORMRF
    else:
        from sudo_rm_rf_amd.dnn.models.attentive_sudormrf_v2 import SuDORMRF
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = SuDORMRF(num_blocks=a.blocks).to(dev).eval()
    mha = (model.sm[0].attentive_resamplers[0] if v3 else model.sm[0].attention).mha
    H, d = mha.n_heads, mha.d_model
    print("attentive SuDoRM-RF %s: B 128, C 512, U %d, D 4, N 512, H %d, d %d, S 2; T = %d" % (a.model, a.blocks, H, d, a.time))
    for batch in (a.batch, 1):
        x = torch.randn(batch, 1, a.time, device=dev)
        ms = timed(model, x, a.steps, a.warmup)
        plan = model._engine().last_plan
        Ld = plan.frames >> (model.upsampling_depth - 1)
        levels = [plan.frames]
        for _ in range(1, model.upsampling_depth):
            levels.append((levels[-1] + 1) // 2)
        # (queries, keys) of every attention of one block
        pairs = list(zip(levels[:-1], levels[1:])) if v3 else [(Ld, Ld)]
        print("batch %3d: forward %.3f ms   (frames %d, deepest level %d positions, workspace %.1f MiB)"
              % (batch, ms, plan.frames, levels[-1] if v3 else Ld, plan.workspace_bytes / 2 ** 20))
        with torch.no_grad(), ops.kernel_trace(dev) as tr:
            model(x)
        total = sum(ms_ for _, ms_ in tr.launches)
        by = {}
        for n, ms_ in tr.launches:
            c, t = by.get(n, (0, 0.0))
            by[n] = (c + 1, t + ms_)
        print("  per-kernel (one profiled forward, %d launches, %.3f ms between marks):" % (len(tr.launches), total))
        for n, (c, t) in sorted(by.items(), key=lambda kv: -kv[1][1]):
            print("    %-26s x %3d  %8.3f ms  %5.1f %%" % (n, c, t, 100 * t / total))
        att = sum(t for n, (_, t) in by.items() if n.startswith("mha_attention"))
        flop = 4.0 * batch * H * d * sum(lq * lk for lq, lk in pairs) * a.blocks      # two contractions, 2 FLOP per multiply-add
        print("  attention: %.3f ms for %.1f GFLOP = %.1f TFLOP/s = %.1f %% of %.0f TF"
              % (att, flop / 1e9, flop / att / 1e9, 100 * flop / att / 1e9 / PEAK_TF, PEAK_TF))
        pyr = sum(t for n, (_, t) in by.items() if n.startswith("dwconv5") or n.startswith("merge"))
        print("  per-level pyramid (dwconv5* + merge*): %.3f ms = %.1f %% of the forward" % (pyr, 100 * pyr / total))


if __name__ == "__main__":
    main()
