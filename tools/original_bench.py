#!/usr/bin/env python3
"""Time the original SuDoRM-RF inference forward on one MI355X.

    python tools/original_bench.py [--blocks 16] [--batch 32] [--time 32000] [--steps 10] [--warmup 3]

Prints, for the reference's README recipe (-X 5 -N 512 -B 256 -H 512 -L 21 -R 16: 256 / 512 channels, depth 5, 512 basis
functions, 2 sources): the forward time at the given batch and at batch 1 (device events around `steps` forwards), the per-kernel
table of one forward (the library's srf_profile_* marks), the share of the four materialising srf_gln_apply_c launches per block,
of the depthwise pyramid and of the mask tail, and -- for scale only -- the Improved model's cfg 2 forward (same channel counts,
depth and block count) in the same run, single stream like this model.  Weights: the seeded constructor's."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--time", type=int, default=32000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from sudo_rm_rf_amd import ops
    from sudo_rm_rf_amd.dnn.models import improved_sudormrf
    from sudo_rm_rf_amd.dnn.models.sudormrf import SuDORMRF
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    kw = dict(out_channels=256, in_channels=512, num_blocks=a.blocks, upsampling_depth=5, enc_kernel_size=21, enc_num_basis=512,
              num_sources=2)
    model = SuDORMRF(**kw).to(dev).eval()
    improved = improved_sudormrf.SuDORMRF(**kw).to(dev).eval()
    improved._engine().multi_stream = False            # one stream, as the original model runs
    print("original SuDoRM-RF: B 256, C 512, U %d, D 5, N 512, K 21, S 2; T = %d" % (a.blocks, a.time))
    for batch in (a.batch, 1):
        x = torch.randn(batch, 1, a.time, device=dev)
        ms = timed(model, x, a.steps, a.warmup)
        plan = model._engine().last_plan
        ms_improved = timed(improved, x, a.steps, a.warmup)
        print("batch %3d: forward %.3f ms   (frames %d, %d launches, workspace %.1f MiB)   [Improved cfg 2, one stream, same run: "
              "%.3f ms]" % (batch, ms, plan.frames, plan.num_launches, plan.workspace_bytes / 2 ** 20, ms_improved))
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
        share = lambda pred: sum(t for n, (_, t) in by.items() if pred(n))
        gln = share(lambda n: n.startswith("gln_apply_c"))
        # bytes the four launches of a block move: a and e read + write C L, g + x reads 2 B L and writes B L, the output 2 B L
        frames = plan.frames
        gbytes = 4.0 * batch * frames * a.blocks * (4 * 512 + 5 * 256)
        print("  srf_gln_apply_c (4 per block): %.3f ms = %.1f %% of the forward, %.2f GB moved = %.2f TB/s"
              % (gln, 100 * gln / total, gbytes / 1e9, gbytes / gln / 1e9))
        pyr = share(lambda n: n.startswith("pyramid_") or n.startswith("dwconv5") or n.startswith("merge"))
        print("  depthwise pyramid (pyramid_* fused, or dwconv5* + merge* level by level): %.3f ms = %.1f %% of the forward"
              % (pyr, 100 * pyr / total))
        tail = share(lambda n: n in ("softmax_mask", "transpose", "overlap_add", "bias_rescale", "mask_weight_fill",
                                     "decoder_weight_expand"))
        print("  mask tail without its GEMMs (fills, softmax_mask, overlap-add, bias): %.3f ms = %.1f %%" % (tail, 100 * tail / total))


if __name__ == "__main__":
    main()
