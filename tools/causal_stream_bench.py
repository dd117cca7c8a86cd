#!/usr/bin/env python3
"""Latency of streaming pushes of the causal SuDoRM-RF (v3) on one MI355X; prints one JSON line per case.

    python tools/causal_stream_bench.py                 # the cases of DESIGN.md section 12
    python tools/causal_stream_bench.py --profile       # + per-kernel family table (in-library profiler)
    python tools/causal_stream_bench.py --case default:1:1      # one case (for a kernel trace of its own)
    python tools/causal_stream_bench.py --pool          # independent streams (stream_pool) against the lock-step session

Per case (config, streams, chunk in granules): ms per push from HIP events around EACH of --pushes timed pushes after
--warmup (mean, median and worst: a streaming user cares about the worst), the real-time factor at --rate (audio seconds
per stream that one second of pushes covers), the launch count, roofline.causal_stream_push_bytes and the fraction of the
HBM peak it would be -- at one granule the bound that matters is launch count x launch latency, not that fraction -- and,
IN THE SAME PROCESS, the whole-signal forward at T = 32000 and the same batch: what a caller without a streaming session
has to run to get the newest chunk.

--pool (defaults config, m = 1, 8, 32 streams; DESIGN.md section 12, "Independent streams"): median ms, same process and build,
of (a) one CausalStreamPool push of m streams x one granule, (b) the lock-step CausalStream(batch=m) push of one granule,
(c) m batch-1 CausalStreams pushed one after the other, (d) a mixed pool tick: a third of the streams deliver g, a third
2 g, a third nothing.
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

CASES = [("default", 1, 1), ("default", 1, 4), ("default", 1, 16), ("default", 32, 1), ("default", 32, 4), ("default", 32, 16),
         ("main", 1, 1)]


def full_forward_ms(m, batch, A, T, steps, warmup, dev):
    wav = torch.from_numpy(np.random.default_rng(0).standard_normal((batch, A, T)).astype(np.float32)).to(dev)
    for _ in range(warmup):
        m(wav)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        m(wav)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def timed_ms(fn, pushes, warmup):
    """ms of each of `pushes` calls of fn (HIP events around each) after `warmup` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(pushes + 1)]
    ev[0].record()
    for i in range(pushes):
        fn()
        ev[i + 1].record()
    ev[-1].synchronize()
    return np.array([ev[i].elapsed_time(ev[i + 1]) for i in range(pushes)])


def pool_cases(args, dev):
    cfg = cf.DEFAULTS
    torch.manual_seed(0)
    m = CausalSuDORMRF(**cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in cf.make_state_dict(cfg, 104).items()})
    m = m.to(dev).eval()
    A = cfg["in_audio_channels"]
    for streams in (1, 8, 32):
        pool = m.stream_pool(streams)
        g = pool.granule
        x = torch.from_numpy(np.random.default_rng(1).standard_normal((streams, A, 2 * g)).astype(np.float32)).to(dev)
        sids = [pool.open() for _ in range(streams)]
        one = {s: x[i, :, :g] for i, s in enumerate(sids)}
        third = streams // 3
        # a third g, a third 2 g, the rest nothing (one stream: it delivers g -- there is nothing to mix)
        mixed = {s: x[i, :, :g] if i < max(third, 1) else x[i, :, :2 * g] if i < 2 * third else x[i, :, :0]
                 for i, s in enumerate(sids)}
        lock = m.stream(batch=streams)
        xl = x[:, :, :g].contiguous()
        singles = [m.stream(batch=1) for _ in range(streams)]
        xs = [x[i:i + 1, :, :g].contiguous() for i in range(streams)]

        def each_single():
            for s, xi in zip(singles, xs):
                s.push(xi)

        rows = {"a_pool_push": lambda: pool.push(one), "b_lockstep_push": lambda: lock.push(xl),
                "c_batch1_sessions": each_single, "d_pool_mixed_tick": lambda: pool.push(mixed)}
        res = {"model": "causal_sudormrf_v3_stream_pool", "config": "default", "streams": streams, "granule": g,
               "pushes": args.pushes, "warmup": args.warmup,
               "mixed_rows": {"g": max(third, 1), "2g": max(2 * third - max(third, 1), 0),
                              "none": streams - max(2 * third, max(third, 1))},
               "launches_pool": pool.num_launches(streams), "launches_lockstep": lock.num_launches}
        for name, fn in rows.items():
            each = timed_ms(fn, args.pushes, args.warmup)
            res[name] = {"ms_median": round(float(np.median(each)), 4), "ms_mean": round(float(each.mean()), 4),
                         "ms_worst": round(float(each.max()), 4)}
        med = lambda k: res[k]["ms_median"]
        res["a_over_b"] = round(med("a_pool_push") / med("b_lockstep_push"), 4)
        res["c_over_a"] = round(med("c_batch1_sessions") / med("a_pool_push"), 4)
        res["d_over_a"] = round(med("d_pool_mixed_tick") / med("a_pool_push"), 4)
        print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pushes", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rate", type=int, default=8000)
    ap.add_argument("--full-T", type=int, default=32000)
    ap.add_argument("--full-steps", type=int, default=30)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--pool", action="store_true", help="independent streams: pool push vs lock-step push vs batch-1 sessions")
    ap.add_argument("--case", default=None, metavar="CONFIG:STREAMS:GRANULES",
                    help="run one case only, e.g. default:1:1 (a kernel trace of one shape)")
    args = ap.parse_args()
    if args.pushes < 200:
        ap.error("--pushes must be >= 200")
    dev = torch.device("cuda:0")
    if args.pool:
        with torch.no_grad():
            pool_cases(args, dev)
        return
    models, full = {}, {}
    with torch.no_grad():
        cases = CASES
        if args.case:
            c, b, k = args.case.split(":")
            cases = [(c, int(b), int(k))]
        for config, streams, granules in cases:
            cfg = cf.DEFAULTS if config == "default" else cf.MAIN
            if config not in models:
                torch.manual_seed(0)
                m = CausalSuDORMRF(**cfg)
                m.load_state_dict({k: torch.from_numpy(v) for k, v in cf.make_state_dict(cfg, 104).items()})
                models[config] = m.to(dev).eval()
            m = models[config]
            A = cfg["in_audio_channels"]
            s = m.stream(batch=streams)
            n = granules * s.granule
            x = torch.from_numpy(np.random.default_rng(1).standard_normal((streams, A, n)).astype(np.float32)).to(dev)
            for _ in range(args.warmup):
                s.push(x)
            torch.cuda.synchronize()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.pushes + 1)]
            ev[0].record()
            for i in range(args.pushes):
                s.push(x)
                ev[i + 1].record()
            ev[-1].synchronize()
            each = np.array([ev[i].elapsed_time(ev[i + 1]) for i in range(args.pushes)])
            ms = float(ev[0].elapsed_time(ev[-1]) / args.pushes)
            if (config, streams) not in full:
                full[(config, streams)] = full_forward_ms(m, streams, A, args.full_T, args.full_steps, 5, dev)
            nbytes = roofline.causal_stream_push_bytes(streams, A, cfg["out_channels"], cfg["in_channels"], cfg["num_blocks"],
                                                       cfg["upsampling_depth"], cfg["enc_kernel_size"], cfg["enc_num_basis"],
                                                       cfg["num_sources"], n)
            res = {"model": "causal_sudormrf_v3_stream", "config": config, "streams": streams, "chunk_granules": granules,
                   "chunk_samples": n, "pushes": args.pushes, "ms_per_push": round(ms, 4),
                   "ms_median": round(float(np.median(each)), 4), "ms_worst": round(float(each.max()), 4),
                   "real_time_factor": round(n / args.rate / (ms * 1e-3), 1), "launches": s.num_launches,
                   "us_per_launch": round(ms * 1e3 / s.num_launches, 2), "state_bytes": s.state_bytes,
                   "push_bytes": nbytes, "hbm_fraction": round(nbytes / (ms * 1e-3) / (roofline.HBM_PEAK_GBS * 1e9), 4),
                   "full_forward_T": args.full_T, "full_forward_ms": round(full[(config, streams)], 4),
                   "push_vs_full": round(ms / full[(config, streams)], 4)}
            if args.profile:
                with ops.kernel_trace(dev) as tr:
                    s.push(x)
                fam = {}
                for name, t in tr.launches:
                    c, tot = fam.get(name, (0, 0.0))
                    fam[name] = (c + 1, tot + t)
                res["profile_ms"] = {k: [c, round(t, 4)] for k, (c, t) in sorted(fam.items(), key=lambda kv: -kv[1][1])}
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
