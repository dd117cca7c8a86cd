#!/usr/bin/env python3
"""Time softmax attention's forward with lse and its backward (srf_mha_attention_lse / srf_mha_attention_bwd) on one MI355X.

    python tools/attention_bwd_bench.py [--steps 10] [--warmup 3]

Two shapes (Bt, H, d, Lq, Lk): the attentive v2 default's deepest level at batch 32, (32, 4, 256, 400, 400), and the v3
level-0 cross-attention of one utterance, (1, 4, 256, 3200, 1600).  Per shape: the per-kernel times (the library's
srf_profile_* marks, mean over `steps` profiled calls), the TFLOP/s of each against the 155 TFLOP/s the exact-fp32 MFMA
measures on this part, and backward / forward.  FLOP counted: 2 per multiply-add of the products a kernel EXECUTES (the
backward recomputes S, and the two-pass key side at d = 256 recomputes it twice): forward 2 products, dq 3, dkv 4, dv 2, dk 3;
the mathematical minimum of the backward is 5 products = 2.5 x the forward's."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TF = 155.0
SHAPES = (("attentive v2, deepest level, batch 32", (32, 4, 256, 400, 400)),
          ("attentive v3, level 0 asks level 1, batch 1", (1, 4, 256, 3200, 1600)))
PRODUCTS = {"mha_attention_lse_mfma": 2, "mha_attention_lse_generic": 2, "mha_attention_bwd_dq_mfma": 3,
            "mha_attention_bwd_dkv_mfma": 4, "mha_attention_bwd_dv_mfma": 2, "mha_attention_bwd_dk_mfma": 3,
            "mha_attention_bwd_dq_generic": 3, "mha_attention_bwd_dkv_generic": 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from sudo_rm_rf_amd import attention, ops
    dev = torch.device("cuda:0")
    for title, (Bt, H, d, Lq, Lk) in SHAPES:
        g = torch.Generator(device=dev).manual_seed(0)
        q, go = (torch.randn(Bt, H * d, Lq, generator=g, device=dev) for _ in range(2))
        k, v = (torch.randn(Bt, H * d, Lk, generator=g, device=dev) for _ in range(2))
        o, lse = torch.empty_like(q), torch.empty(Bt, H, Lq, device=dev)
        gq, gk, gv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        ws = torch.empty(attention.mha_attention_bwd_workspace_bytes(Bt, H, d, Lq, Lk), dtype=torch.uint8, device=dev)

        def step():
            attention.mha_attention_lse(q, k, v, H, out=o, lse=lse)
            attention.mha_attention_bwd(q, k, v, o, lse, go, H, gq=gq, gk=gk, gv=gv, workspace=ws)

        for _ in range(a.warmup):
            step()
        torch.cuda.synchronize()
        by = {}
        for _ in range(a.steps):
            with ops.kernel_trace(dev) as tr:
                step()
            for n, ms in tr.launches:
                by[n] = by.get(n, 0.0) + ms / a.steps
        unit = 2.0 * Bt * H * d * Lq * Lk          # FLOP of one product
        print("%s: (Bt, H, d, Lq, Lk) = %s, %d steps after %d warm-up" % (title, (Bt, H, d, Lq, Lk), a.steps, a.warmup))
        for n, ms in by.items():
            p = PRODUCTS.get(n)
            if p is None:
                print("    %-28s %9.3f ms" % (n, ms))
            else:
                tf = p * unit / ms / 1e9
                print("    %-28s %9.3f ms  %d products = %7.1f GFLOP  %6.1f TFLOP/s = %4.1f %% of %.0f TF"
                      % (n, ms, p, p * unit / 1e9, tf, 100 * tf / PEAK_TF, PEAK_TF))
        fwd = sum(ms for n, ms in by.items() if n.startswith("mha_attention_lse"))
        bwd = sum(ms for n, ms in by.items() if n.startswith("mha_attention_bwd"))
        print("    forward %.3f ms, backward %.3f ms: backward / forward = %.2f   (FLOP ratio 2.5; 3.5 with one recomputation "
              "of S; executed here: %.1f)" % (fwd, bwd, bwd / fwd, sum(PRODUCTS.get(n, 0) for n in by if "_bwd_" in n) / 2.0))


if __name__ == "__main__":
    main()
