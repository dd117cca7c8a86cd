#!/usr/bin/env python3
"""Time the original SuDoRM-RF's HIP training step (SuDORMRF.enable_hip_training) on one MI355X.

    python tools/original_train_bench.py [--blocks 16] [--batch 32] [--time 32000] [--steps 5] [--warmup 2]

Prints, for the reference's README recipe (-X 5 -N 512 -B 256 -H 512 -L 21 -R 16: 256 / 512 channels, depth 5, 512 basis
functions, 2 sources): the saved / scratch bytes of the step, the forward + backward time (device events around `steps` steps of
out = model(x); out.backward(g)), the per-kernel table of one profiled step (the library's srf_profile_* marks) and the bytes per
second of srf_gln_c_bwd next to srf_gln_apply_c's from the same run.  Weights: the seeded constructor's."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def step(model, x, g):
    for p in model.parameters():
        p.grad = None
    model(x).backward(g)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--time", type=int, default=32000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    from sudo_rm_rf_amd import ops
    from sudo_rm_rf_amd.dnn.models.sudormrf import SuDORMRF
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, Cc = 256, 512
    kw = dict(out_channels=B, in_channels=Cc, num_blocks=a.blocks, upsampling_depth=5, enc_kernel_size=21, enc_num_basis=512,
              num_sources=2)
    model = SuDORMRF(**kw).to(dev).train().enable_hip_training()
    x = torch.randn(a.batch, 1, a.time, device=dev)
    g = torch.randn(a.batch, 2, a.time, device=dev)
    print("original SuDoRM-RF training step: B 256, C 512, U %d, D 5, N 512, K 21, S 2; batch %d, T = %d" % (a.blocks, a.batch, a.time))
    for _ in range(a.warmup):
        step(model, x, g)
    plan = model._engine().last_plan
    saved, scratch = plan.train_sizes()
    print("frames %d; saved %.2f GiB, scratch %.2f GiB" % (plan.frames, saved / 2 ** 30, scratch / 2 ** 30))
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    for _ in range(a.steps):
        step(model, x, g)
    end.record()
    torch.cuda.synchronize()
    print("forward + backward: %.3f ms per step (%d steps)" % (beg.elapsed_time(end) / a.steps, a.steps))
    for p in model.parameters():
        p.grad = None
    with ops.kernel_trace(dev) as trf:
        out = model(x)
    torch.cuda.synchronize()
    with ops.kernel_trace(dev) as trb:
        out.backward(g)
    torch.cuda.synchronize()
    tf, tb = sum(ms for _, ms in trf.launches), sum(ms for _, ms in trb.launches)
    print("one profiled step: forward %.3f ms in %d launches, backward %.3f ms in %d launches" % (tf, len(trf.launches), tb, len(trb.launches)))
    by = {}
    for n, ms in trf.launches + trb.launches:
        c, t = by.get(n, (0, 0.0))
        by[n] = (c + 1, t + ms)
    for n, (c, t) in sorted(by.items(), key=lambda kv: -kv[1][1]):
        print("    %-28s x %4d  %9.3f ms  %5.1f %%" % (n, c, t, 100 * t / (tf + tb)))
    share = lambda pred: sum(t for n, (_, t) in by.items() if pred(n))
    cols = 4.0 * a.batch * plan.frames * a.blocks
    # srf_gln_c_bwd, 4 per block (two on C channels, two on B): the reduce pass reads gout and x, the apply pass reads both and writes gx
    t_bwd = share(lambda n: n.startswith("gln_c_bwd"))
    b_bwd = cols * 5 * (2 * Cc + 2 * B)
    # srf_gln_apply_c: the forward's 4 per block (a and e read + write C, g + x reads 2 B and writes B, the output 2 B) and the
    # backward's 2 re-computations (a and e again)
    t_app = share(lambda n: n.startswith("gln_apply_c"))
    b_app = cols * ((4 * Cc + 5 * B) + 4 * Cc)
    print("srf_gln_c_bwd (reduce + apply, 4 per block): %.3f ms, %.2f GB moved = %.2f TB/s" % (t_bwd, b_bwd / 1e9, b_bwd / t_bwd / 1e9))
    print("srf_gln_apply_c (4 per block forward, 2 backward): %.3f ms, %.2f GB moved = %.2f TB/s" % (t_app, b_app / 1e9, b_app / t_app / 1e9))


if __name__ == "__main__":
    main()
