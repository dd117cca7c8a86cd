#!/usr/bin/env python3
"""The FUSS recipe's per-step pieces on one MI355X (csrc/srf_loss_fuss.hip): zero-reference SNR loss forward and backward,
the stabilized SI-SDR metric and the online augmentation, at the recipe's shape (batch 4, 4 sources, 10 s @ 16 kHz) and at
batch 32 x 4 s @ 8 kHz.

    python tools/fuss_step_bench.py [--steps 200] [--warmup 20] > profiles/fuss_loss.txt

Every entry point is called straight on preallocated device buffers (no allocation, no host synchronisation inside the timed
window) and timed with HIP events over --steps calls after --warmup.  Printed per operation: microseconds per call, the
ALGORITHMIC bytes (forward 2 Bt S T 4: both inputs once; backward 3 Bt S T 4: both inputs + the gradient; metric
Bt (n_est + n_act) T 4; augmentation pass 1 reads S rows and writes S + 1, pass 2 reads and writes the mixture), the bytes/s
they amount to and their share of the 8 TB/s HBM peak, and the launches of one call as the in-library profiler lists them
(a separate, untimed call).  `pit_sisdr forward` is the existing PIT-SI-SDR loss (srf_pit_stats_kernel + finalize, after a
memset) on the same buffers in the same run, as the yardstick for the streaming pass.  One JSON line per shape at the end.
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sudo_rm_rf_amd import _lib, ops, roofline  # noqa: E402

SHAPES = [("recipe: batch 4, 4 sources, 10 s @ 16 kHz", 4, 4, 160000), ("batch 32, 4 sources, 4 s @ 8 kHz", 32, 4, 32000)]


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps * 1e3      # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs an MI355X"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    st = _lib.current_stream(dev)
    p, f = _lib.ptr, C.c_float
    out = []
    for title, Bt, S, T in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(Bt + T)
        tgt = torch.randn(Bt, S, T, generator=g)
        tgt[:, -1] = 0.0                                        # FUSS: a silent source in every example
        est = (tgt[:, torch.randperm(S, generator=g)] + 0.3 * torch.randn(Bt, S, T, generator=g)).to(dev)
        tgt = tgt.to(dev)
        u8 = lambda n: torch.empty(n, dtype=torch.uint8, device=dev)
        work = u8(lib.srf_zeroref_snr_work_bytes(Bt, S, T))
        values, perm, loss = (torch.empty(Bt, device=dev), torch.empty(Bt, dtype=torch.int32, device=dev),
                              torch.empty(2, device=dev))
        grad, up = torch.empty_like(est), torch.ones(1, device=dev)
        mwork = u8(lib.srf_stab_sisdr_work_bytes(Bt, T))
        pwork = u8(lib.srf_pit_sisdr_work_bytes(Bt, S))
        src_b = torch.stack([torch.randperm(Bt, generator=g) for _ in range(S)]).to(torch.int32).to(dev)
        src_s = torch.randperm(S, generator=g).to(torch.int32).to(dev)
        gain = (torch.rand(Bt, S, generator=g) + 0.5).to(dev)
        aout, amix, astats = torch.empty_like(tgt), torch.empty(Bt, 1, T, device=dev), torch.empty(Bt, 2, device=dev)
        ascr = u8(lib.srf_fuss_augment_scratch_bytes(Bt, T))

        def check(rc):
            if rc != 0:
                _lib.check(rc, "fuss_step_bench")

        ops_ = {
            "zeroref_snr forward": (lambda: check(lib.srf_zeroref_snr_forward(
                p(est), p(tgt), Bt, S, T, 0, f(-40.), f(1e-3), f(1e-9), p(work), p(values), p(perm), p(loss), st)),
                2 * Bt * S * T * 4),
            "zeroref_snr backward": (lambda: check(lib.srf_zeroref_snr_backward(
                p(est), p(tgt), Bt, S, T, p(work), p(up), 0, p(grad), st)), 3 * Bt * S * T * 4),
            "pit_sisdr forward": (lambda: check(lib.srf_pit_sdr_forward(
                p(est), p(tgt), Bt, S, T, f(0.0), 0, 1, 1, p(pwork), None, p(loss), st)), 2 * Bt * S * T * 4),
            "stab_sisdr metric 4 x 3": (lambda: check(lib.srf_stab_sisdr(
                p(est), p(tgt), Bt, S, S, S - 1, T, 1, 1, C.c_double(1e-9), p(mwork), p(values), p(perm), st)),
                Bt * (2 * S - 1) * T * 4),
            "fuss_augment": (lambda: check(lib.srf_fuss_augment(
                p(tgt), p(src_b), p(src_s), p(gain), Bt, S, T, f(1e-9), p(aout), p(amix), p(astats), p(ascr), st)),
                Bt * (2 * S + 1 + 2) * T * 4),
        }
        print("== %s (Bt = %d, S = %d, T = %d) ==" % (title, Bt, S, T))
        rec = {"shape": title, "Bt": Bt, "S": S, "T": T, "steps": args.steps}
        with torch.cuda.device(dev):
            for name, (fn, nbytes) in ops_.items():
                us = timed(fn, args.steps, args.warmup)
                with ops.kernel_trace(dev) as tr:
                    fn()
                tbs = nbytes / (us * 1e-6) / 1e12
                launches = ", ".join("%s %.1f us" % (n, ms * 1e3) for n, ms in tr.launches)
                print("%-26s %8.1f us/call  %6.1f MB algorithmic  %6.3f TB/s  %5.1f %% of the HBM peak  | %d launches: %s"
                      % (name, us, nbytes / 1e6, tbs, 100 * tbs * 1e3 / roofline.HBM_PEAK_GBS, len(tr.launches), launches))
                rec[name] = {"us": round(us, 2), "algorithmic_bytes": nbytes, "tb_per_s": round(tbs, 4),
                             "launches": [n for n, _ in tr.launches]}
        out.append(rec)
        print()
    for rec in out:
        print(json.dumps(rec))


if __name__ == "__main__":
    main()
