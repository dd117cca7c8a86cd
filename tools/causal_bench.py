#!/usr/bin/env python3
"""Inference speed of the causal SuDoRM-RF (v3) forward on one MI355X; prints one JSON line.

    python tools/causal_bench.py                      # reference constructor defaults, batch 32, T = 32000
    python tools/causal_bench.py --batch 1            # the latency case
    python tools/causal_bench.py --profile            # + per-kernel family table (in-library profiler, one stream)

ms per forward from HIP events over --steps timed forwards after --warmup; separated seconds per second at --rate Hz;
the roofline.py byte model of the forward and its fraction of the 8 TB/s HBM peak.  Weights: the fixture generator's
random draw for the defaults (tests/causal_fixtures.py), so that no block is the identity.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sudo_rm_rf_amd import ops, roofline  # noqa: E402
from sudo_rm_rf_amd.dnn.models.causal_improved_sudormrf_v3 import CausalSuDORMRF  # noqa: E402
from tests import causal_fixtures as cf  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--T", type=int, default=32000)
    ap.add_argument("--rate", type=int, default=8000, help="sample rate the separated seconds are counted at")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--config", choices=("default", "main"), default="default")
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps must be >= 20")
    dev = torch.device("cuda:0")
    cfg = cf.DEFAULTS if args.config == "default" else cf.MAIN
    torch.manual_seed(0)
    m = CausalSuDORMRF(**cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in cf.make_state_dict(cfg, 104).items()})
    m = m.to(dev).eval()
    A = cfg["in_audio_channels"]
    wav = torch.from_numpy(np.random.default_rng(0).standard_normal((args.batch, A, args.T)).astype(np.float32)).to(dev)
    with torch.no_grad():
        for _ in range(args.warmup):
            m(wav)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            m(wav)
        e1.record()
        e1.synchronize()
    ms = e0.elapsed_time(e1) / args.steps
    nbytes = args.batch * roofline.causal_bytes_per_example(A, cfg["out_channels"], cfg["in_channels"], cfg["num_blocks"],
                                                            cfg["upsampling_depth"], cfg["enc_kernel_size"],
                                                            cfg["enc_num_basis"], cfg["num_sources"], args.T)
    res = {"model": "causal_sudormrf_v3", "config": args.config, "batch": args.batch, "T": args.T, "steps": args.steps,
           "ms_per_forward": round(ms, 4), "separated_s_per_s": round(args.batch * args.T / args.rate / (ms * 1e-3), 1),
           "split": str(m._engine()._split_choice.get((dev.index, args.batch, args.T), (args.batch,))),
           "roofline_bytes": nbytes, "hbm_fraction": round(nbytes / (ms * 1e-3) / (roofline.HBM_PEAK_GBS * 1e9), 4)}
    if args.profile:
        eng = m._engine()
        eng.multi_stream = False
        with torch.no_grad():
            m(wav)
            with ops.kernel_trace(dev) as tr:
                m(wav)
        eng.multi_stream = True
        fam = {}
        for n, t in tr.launches:
            c, s = fam.get(n, (0, 0.0))
            fam[n] = (c + 1, s + t)
        L = roofline.frames(args.T, cfg["enc_kernel_size"], cfg["upsampling_depth"])
        pyr = fam.get("causal_pyramid", (0, 0.0))
        res["profile_ms"] = {n: [c, round(s, 4)] for n, (c, s) in sorted(fam.items(), key=lambda kv: -kv[1][1])}
        if pyr[0]:
            per = pyr[1] / pyr[0]
            res["pyramid_us"] = round(per * 1e3, 1)
            res["pyramid_tbs"] = round(roofline.causal_pyramid_bytes(args.batch, cfg["in_channels"], L) / (per * 1e-3) / 1e12, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
