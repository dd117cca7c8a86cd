#!/usr/bin/env python3
"""Measure the causal SuDoRM-RF (v3) HIP training step (CausalSuDORMRF.enable_hip_training) on cuda:0.

Reference defaults (B 128, C 512, U 16, D 4, K 21, N 512, 2 sources) at batch 32, T = 32000 unless told otherwise:
  * step time: forward + backward of a linear loss, median of --steps after --warmup;
  * per-kernel times through the in-library profiler (srf_profile_*), summed per kernel family over one step;
  * the fused pyramid backward against the per-level path (the PYR_PER_LEVEL switch), in this one process;
  * the fused kernel's rate on its algorithmic bytes: g_merged + u + sum_k d_k read, gu written = (3 + sum_k 2^-k) C L floats
    per example and block.
Prints a plain-text record (kept as profiles/causal_train.txt).  Nothing here is a pass condition.

    python tools/causal_train_bench.py [--batch 32] [--T 32000] [--blocks 16] [--steps 10] [--warmup 3]
"""
import argparse
import os
import statistics
import sys
from collections import OrderedDict

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sudo_rm_rf_amd import ops  # noqa: E402
from sudo_rm_rf_amd.dnn.models.causal_improved_sudormrf_v3 import CausalSuDORMRF  # noqa: E402


def step(model, x, g):
    for p in model.parameters():
        p.grad = None
    (model(x) * g).sum().backward()


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def families(dev, fn):
    with ops.kernel_trace(dev) as tr:
        fn()
    out = OrderedDict()
    for name, ms in tr.launches:
        n, t = out.get(name, (0, 0.0))
        out[name] = (n + 1, t + ms)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--T", type=int, default=32000)
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = CausalSuDORMRF(num_blocks=a.blocks).to(dev).train().enable_hip_training()
    with torch.no_grad():
        for b in model.sm:
            b.skipinit_gain.fill_(0.3)          # (a fresh model's gains are 0: its blocks would be the identity)
    x = torch.randn(a.batch, 1, a.T, device=dev)
    g = torch.randn(a.batch, 2, a.T, device=dev)
    run = lambda: step(model, x, g)
    print("causal training step: batch %d, T %d, %d blocks, %s" % (a.batch, a.T, a.blocks, torch.cuda.get_device_name(0)))
    plan_sizes = None
    med, lo, hi = timed(run, a.steps, a.warmup)
    plan = model._engine().last_plan
    plan_sizes = plan.train_sizes()
    L, C, D, U = plan.frames, model.in_channels, model.upsampling_depth, a.blocks
    print("saved %.2f GB, scratch %.2f GB, L = %d" % (plan_sizes[0] / 1e9, plan_sizes[1] / 1e9, L))
    print("step (forward + backward), fused pyramid backward : median %.2f ms (min %.2f, max %.2f) over %d steps" % (med, lo, hi, a.steps))
    with ops.debug_flags(ops.DebugFlag.PYR_PER_LEVEL):
        med1, lo1, hi1 = timed(run, a.steps, a.warmup)
        fam1 = families(dev, run)
    print("step (forward + backward), per-level pyramid backward: median %.2f ms (min %.2f, max %.2f)" % (med1, lo1, hi1))
    fam = families(dev, run)
    total = sum(t for _, t in fam.values())
    print("\nper kernel family, one step, fused path (profiler intervals include the launch gaps; total %.2f ms):" % total)
    for name, (n, t) in sorted(fam.items(), key=lambda kv: -kv[1][1]):
        print("  %-24s %4d launches %9.3f ms %5.1f %%" % (name, n, t, 100 * t / total))
    pyr = fam.get("causal_pyramid_bwd", (0, 0.0))
    fin = sum(fam.get(k, (0, 0.0))[1] for k in ("causal_bwd_finalize", "causal_bwd_slope"))
    lvl = sum(fam1.get(k, (0, 0.0))[1] for k in ("causal_dw_bwd", "causal_bwd_finalize", "causal_bwd_slope"))
    floats = (3.0 + sum(2.0 ** -k for k in range(D))) * C * L * a.batch
    if pyr[0]:
        per = pyr[1] / pyr[0]
        print("\nfused pyramid backward: %.3f ms per block (+ %.3f ms finalize launches per block); per-level path: %.3f ms per block"
              % (per, fin / U, lvl / U))
        print("fused kernel on its algorithmic bytes (%.1f MB per block: g_merged + u + sum d_k read, gu written): %.2f TB/s"
              % (4 * floats / 1e6, 4 * floats / (per * 1e-3) / 1e12))


if __name__ == "__main__":
    main()
