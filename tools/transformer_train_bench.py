#!/usr/bin/env python3
"""Time the attentive TransformerLayer's opt-in HIP training step on one MI355X.

    python tools/transformer_train_bench.py [--steps 20] [--warmup 5]

The layer at the attentive v2 default's deepest level: Bt 32, emb 512, 4 heads of 256, Ld 400, dropout 0.1, with the level's
lazy norm on load.  Reported, all from ONE process and one run:
  * forward (inference kernels, no autograd) and forward + backward (train() mode, autograd, dropout on): host clock around
    `steps` calls that end in a device synchronise, profiler off;
  * the per-kernel table of one training step (the library's srf_profile_* marks, mean over `steps` profiled steps);
  * posenc_apply with dropout against the plain kernel, interleaved call by call: median, minimum and maximum of `steps`
    profiled launches each.  Both move 2 * Bt * C * Ld * 4 bytes (one read of a, one write of x; the table's Ld * C floats are
    re-read per example from cache), which gives the GB/s column."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BT, EMB, HEADS, D_MODEL, LD, P = 32, 512, 4, 256, 400, 0.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    from sudo_rm_rf_amd import attention, ops
    from sudo_rm_rf_amd.dnn.models.attentive_sudormrf_v2 import TransformerLayer
    if not torch.cuda.is_available():
        raise SystemExit("transformer_train_bench needs an MI355X")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    layer = TransformerLayer(EMB, D_MODEL, HEADS, dropout=P).to(dev).enable_hip_training()
    x = torch.randn(BT, EMB, LD, device=dev)
    gout = torch.randn(BT, EMB, LD, device=dev)
    sums = ops.gln_stats(x, BT)
    in_g = torch.ones(EMB, device=dev, requires_grad=True)
    in_b = torch.zeros(EMB, device=dev, requires_grad=True)
    wrt = [in_g, in_b] + list(layer.parameters())

    def forward():
        with torch.no_grad():
            return layer(x, sums, in_g, in_b)

    def step():
        xg = x.detach().requires_grad_()
        out = layer(xg, sums, in_g, in_b)
        return torch.autograd.grad(out, [xg] + wrt, gout)

    def clock(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.steps * 1e3

    print("TransformerLayer: Bt %d, emb %d, %d heads of %d, Ld %d, dropout %.1f; %d steps after %d warm-up, one run"
          % (BT, EMB, HEADS, D_MODEL, LD, P, a.steps, a.warmup))
    layer.eval()
    fwd = clock(forward)
    layer.train()
    both = clock(step)
    print("  forward (inference kernels)      %8.3f ms per call (host clock, profiler off)" % fwd)
    print("  forward + backward (train mode)  %8.3f ms per call (host clock, profiler off)" % both)
    by, order = {}, []
    for _ in range(a.steps):
        with ops.kernel_trace(dev) as tr:
            step()
        for n, ms in tr.launches:
            if n not in by:
                order.append(n)
            c = by.setdefault(n, [0, 0.0])
            c[0] += 1
            c[1] += ms
    total = sum(ms for _, ms in by.values()) / a.steps
    print("  per kernel, one training step (mean of %d profiled steps; sum of kernels %.3f ms):" % (a.steps, total))
    for n in order:
        cnt, ms = by[n]
        print("    %-30s x%-2d %8.3f ms  %5.1f %%" % (n, cnt // a.steps, ms / a.steps, 100 * ms / a.steps / total))

    # posenc_apply: dropout against plain, interleaved in the same run
    out = torch.empty_like(x)
    g, b = in_g.detach(), in_b.detach()
    pe = layer.pos_enc.pe.detach()
    times = {"posenc_apply": [], "posenc_apply_dropout": []}
    for i in range(a.warmup + a.steps):
        for p in (0.0, P):
            with ops.kernel_trace(dev) as tr:
                attention.posenc_apply(x, pe, sums, g, b, out=out, p=p, seed=i, offset=1 << 33)
            (n, ms), = tr.launches
            if i >= a.warmup:
                times[n].append(ms)
    nbytes = 2.0 * BT * EMB * LD * 4
    print("  posenc_apply, %d interleaved profiled launches each, %.1f MB moved:" % (a.steps, nbytes / 1e6))
    for n, ts in times.items():
        med = statistics.median(ts)
        print("    %-22s median %7.2f us  min %7.2f  max %7.2f  spread %5.2f us   %7.1f GB/s at the median"
              % (n, med * 1e3, min(ts) * 1e3, max(ts) * 1e3, (max(ts) - min(ts)) * 1e3, nbytes / med / 1e6))
    d = statistics.median(times["posenc_apply_dropout"]) - statistics.median(times["posenc_apply"])
    print("    dropout - plain at the medians: %+.2f us" % (d * 1e3))


if __name__ == "__main__":
    main()
