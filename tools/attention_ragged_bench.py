#!/usr/bin/env python3
"""Time the ragged attention forms (srf_mha_attention_ragged, _lse_ragged, _bwd_ragged) on one MI355X against what they replace.

    python tools/attention_ragged_bench.py [--rounds 7] [--iters 5] [--warmup 2] [--cross]

Shape (Bt, H, d, Lq, Lk) = (32, 4, 256, 400, 400), self-attention (q_len = k_len), seeded lengths uniform on [200, 400].  The
forward, the forward with lse and the backward are timed in three forms:
    ragged    one call on the padded tensors with the lengths
    (a)       the uniform call on the padded tensors -- NOT a correct answer (padded keys take softmax weight): the time to beat
    (b)       the 32 batch-1 uniform calls on the examples' own slices that the ragged call replaces
Device events around `iters` back-to-back calls, medians over `rounds` rounds in which the forms alternate, one process.  Beside
the time ratio against (a) stands the work ratio sum_b q_len[b] k_len[b] / (Bt Lq Lk); then the per-kernel times of one ragged and
one uniform pass (the library's profiler marks).  --cross adds one line for the v3 cross shape (4, 4, 256, 3200, 1600) with
q_len = 2 k_len."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def lengths_for(Bt, lo, hi, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [int(x) for x in torch.randint(lo, hi + 1, (Bt,), generator=g)]


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def bench(title, shape, ql, kl, args):
    from sudo_rm_rf_amd import attention, ops
    Bt, H, d, Lq, Lk = shape
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    q, go = (torch.randn(Bt, H * d, Lq, generator=g, device=dev) for _ in range(2))
    k, v = (torch.randn(Bt, H * d, Lk, generator=g, device=dev) for _ in range(2))
    o, lse = torch.empty_like(q), torch.empty(Bt, H, Lq, device=dev)
    gq, gk, gv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    ws = torch.empty(attention.mha_attention_bwd_workspace_bytes(Bt, H, d, Lq, Lk), dtype=torch.uint8, device=dev)
    kw = dict(q_lengths=ql, k_lengths=kl)
    # (b): every example's own contiguous slices and outputs, made once
    ex = []
    for b in range(Bt):
        qb, gob = (t[b:b + 1, :, :ql[b]].contiguous() for t in (q, go))
        kb, vb = (t[b:b + 1, :, :kl[b]].contiguous() for t in (k, v))
        ex.append((qb, kb, vb, gob, torch.empty_like(qb), torch.empty(1, H, ql[b], device=dev), torch.empty_like(qb),
                   torch.empty_like(kb), torch.empty_like(vb)))

    def each(fn):
        def run():
            for e in ex:
                fn(*e)
        return run

    forms = {
        "forward": (lambda: attention.mha_attention(q, k, v, H, out=o, **kw),
                    lambda: attention.mha_attention(q, k, v, H, out=o),
                    each(lambda qb, kb, vb, gob, ob, lb, a, b_, c: attention.mha_attention(qb, kb, vb, H, out=ob))),
        "forward with lse": (lambda: attention.mha_attention_lse(q, k, v, H, out=o, lse=lse, **kw),
                             lambda: attention.mha_attention_lse(q, k, v, H, out=o, lse=lse),
                             each(lambda qb, kb, vb, gob, ob, lb, a, b_, c: attention.mha_attention_lse(qb, kb, vb, H, out=ob, lse=lb))),
        "backward": (lambda: attention.mha_attention_bwd(q, k, v, o, lse, go, H, gq=gq, gk=gk, gv=gv, workspace=ws, **kw),
                     lambda: attention.mha_attention_bwd(q, k, v, o, lse, go, H, gq=gq, gk=gk, gv=gv, workspace=ws),
                     each(lambda qb, kb, vb, gob, ob, lb, a, b_, c: attention.mha_attention_bwd(qb, kb, vb, ob, lb, gob, H, gq=a, gk=b_,
                                                                                            gv=c, workspace=ws))),
    }
    work = sum(a * b for a, b in zip(ql, kl)) / float(Bt * Lq * Lk)
    print("%s: (Bt, H, d, Lq, Lk) = %s, q_len %d..%d, k_len %d..%d, work ratio %.3f; %d rounds x %d calls, medians"
          % (title, shape, min(ql), max(ql), min(kl), max(kl), work, args.rounds, args.iters))
    print("    %-18s %10s %10s %10s %12s %12s" % ("", "ragged ms", "(a) ms", "(b) ms", "ragged/(a)", "ragged/(b)"))
    for name, fns in forms.items():
        # every form leaves valid o / lse behind for the next (the backward reads them): run the ragged lse forward first
        attention.mha_attention_lse(q, k, v, H, out=o, lse=lse, **kw)
        for e in ex:
            attention.mha_attention_lse(e[0], e[1], e[2], H, out=e[4], lse=e[5])
        for fn in fns:
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times = [[], [], []]
        for _ in range(args.rounds):
            for i, fn in enumerate(fns):
                times[i].append(timed(fn, args.iters))
        r, a, b = (statistics.median(t) for t in times)
        print("    %-18s %10.3f %10.3f %10.3f %12.3f %12.3f" % (name, r, a, b, r / a, r / b))
    if args.kernels:
        for label, kws in (("ragged", kw), ("uniform on the padded tensors", {})):
            by = {}
            for _ in range(args.iters):
                with ops.kernel_trace(dev) as tr:
                    attention.mha_attention(q, k, v, H, out=o, **kws)
                    attention.mha_attention_lse(q, k, v, H, out=o, lse=lse, **kws)
                    attention.mha_attention_bwd(q, k, v, o, lse, go, H, gq=gq, gk=gk, gv=gv, workspace=ws, **kws)
                for n, ms in tr.launches:
                    by[n] = by.get(n, 0.0) + ms / args.iters
            print("    per kernel, %s:" % label)
            for n, ms in by.items():
                print("        %-36s %9.3f ms" % (n, ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cross", action="store_true", help="also the v3 cross shape (4, 4, 256, 3200, 1600), q_len = 2 k_len")
    a = ap.parse_args()
    a.kernels = True
    lens = lengths_for(32, 200, 400)
    bench("attentive v2, deepest level, batch 32", (32, 4, 256, 400, 400), lens, lens, a)
    if a.cross:
        kl = lengths_for(4, 800, 1600, seed=1)
        bench("attentive v3, level 0 asks level 1, batch 4", (4, 4, 256, 3200, 1600), [2 * n for n in kl], kl, a)


if __name__ == "__main__":
    main()
