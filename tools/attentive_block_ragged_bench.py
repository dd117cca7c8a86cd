#!/usr/bin/env python3
"""Time one AttentiveUConvBlock on a ragged batch (AttentiveUConvBlock.forward(x, lengths)) on one
MI355X against what it replaces.

    python tools/attentive_block_ragged_bench.py [--rounds 7] [--iters 3] [--warmup 2] [--seed 0]

The block at the v2 defaults (out 128, in 512, D 4, 4 heads x 256), batch 32, row stride L = 3200; lengths drawn once on
[L / 2, L] in multiples of 8 (torch.Generator().manual_seed(--seed)).  Three forms, in one process:
    ragged    one call on the padded tensor with the lengths
    (b)       the 32 batch-1 uniform calls on the examples' own slices that the ragged call replaces
    (a)       the uniform call on the padded tensor -- NOT a correct answer (the padding takes part in every norm and in the
              attention): a floor
Device events around `iters` back-to-back calls, medians over `rounds` rounds in which the forms alternate.  Then the work
ratio (own columns / padded columns; for the attention own^2 / padded^2), the per-kernel times of one ragged call from the
library's profiler marks, and the share of the added statistics passes (gln_stats_ragged, sums_scale_ragged) and of zero_past
(torch fills, timed by device events around a call on the block's output)."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=3200)
    args = ap.parse_args()
    from sudo_rm_rf_amd import attention, ops
    from sudo_rm_rf_amd.dnn.models.attentive_sudormrf_v2 import AttentiveUConvBlock
    dev = torch.device("cuda:0")
    Bt, L, D = args.batch, args.frames, 4
    g = torch.Generator().manual_seed(args.seed)
    lengths = [8 * int(n) for n in torch.randint(L // 16, L // 8 + 1, (Bt,), generator=g)]
    torch.manual_seed(args.seed)
    blk = AttentiveUConvBlock(128, 512, D, 4, 256).to(dev).eval()
    x = torch.randn(Bt, 128, L, generator=g).to(dev)
    slices = [x[b:b + 1, :, :n].contiguous() for b, n in enumerate(lengths)]

    def ragged():
        return blk(x, lengths)

    def one_by_one():
        for s in slices:
            blk(s)

    def padded():
        return blk(x)

    forms = (("ragged", ragged), ("(b) 32 batch-1 calls", one_by_one), ("(a) uniform on the padding", padded))
    with torch.no_grad():
        for _, fn in forms:
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times = [[] for _ in forms]
        for _ in range(args.rounds):
            for i, (_, fn) in enumerate(forms):
                times[i].append(timed(fn, args.iters))
        med = [statistics.median(t) for t in times]
        own, own2 = sum(lengths) / float(Bt * L), sum(n * n for n in lengths) / float(Bt * L * L)
        print("AttentiveUConvBlock(128, 512, D 4, 4 x 256), batch %d, L %d, lengths %d..%d (seed %d, multiples of 8); %d rounds x %d "
              "calls, medians" % (Bt, L, min(lengths), max(lengths), args.seed, args.rounds, args.iters))
        print("    work ratio: own / padded columns %.3f, attention own^2 / padded^2 %.3f" % (own, own2))
        for (name, _), m, t in zip(forms, med, times):
            print("    %-28s %9.3f ms   (min %.3f, max %.3f)   ragged / this = %.3f" % (name, m, min(t), max(t), med[0] / m))
        by, order = {}, []
        for _ in range(args.iters):
            with ops.kernel_trace(dev) as tr:
                y = ragged()
            for n, ms in tr.launches:
                if n not in by:
                    order.append(n)
                by[n] = by.get(n, [0, 0.0])
                by[n][0] += 1
                by[n][1] += ms / args.iters
        total = sum(v[1] for v in by.values())
        print("    per kernel, one ragged call (profiler marks; %d launches, %.3f ms in kernels):" % (sum(v[0] for v in by.values())
                                                                                                   // args.iters, total))
        for n in order:
            print("        %-36s x%-3d %9.3f ms  %5.1f %%" % (n, by[n][0] // args.iters, by[n][1], 100.0 * by[n][1] / total))
        zp = statistics.median(timed(lambda: attention.zero_past(y, lengths), args.iters) for _ in range(args.rounds))
        stats = sum(v[1] for n, v in by.items() if n in ("gln_stats_ragged", "sums_scale_ragged"))
        print("    added statistics passes (gln_stats_ragged + sums_scale_ragged): %.3f ms = %.1f %% of the ragged call" %
              (stats, 100.0 * stats / med[0]))
        print("    zero_past (%d strided fills): %.3f ms = %.1f %% of the ragged call" % (sum(n < L for n in lengths), zp,
                                                                                       100.0 * zp / med[0]))


if __name__ == "__main__":
    main()
