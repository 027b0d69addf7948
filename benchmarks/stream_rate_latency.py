"""Push latency of the slot pool at a client's sample rate (ResamplingStreamPool) on the causal paper config, against the plain
FusedStreamPool at 8 kHz in ONE process.

    python benchmarks/stream_rate_latency.py [--out profiles/stream_rate_latency.json]

Protocol of benchmarks/stream_pool_latency.py: 5 warm-up + 200 timed pushes of random audio, wall clock around a synchronise, five
repetitions; median and range of ms per push.  32 slots, every slot open, 10-ms chunks (8 hops of the model; 160 samples at 16 kHz,
480 at 48 kHz), eager and graph=True (the resample launches stay outside the pool's graphs either way):
  plain          FusedStreamPool at 8 kHz, measured before and after the other forms
  16k_16k        16 kHz in, 16 kHz out        48k_48k        48 kHz in, 48 kHz out
  16k_model      16 kHz in, model-rate out    16k_16k_z8     16 kHz in and out with zeros = 8
and the two resample stages alone (StreamResampler pushes of the same shapes: 32 rows in, 64 rows in groups of 2 out).
--profile N: only N eager 16k_16k pushes (for a kernel trace).
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import resample  # noqa: E402
from conv_tasnet_amd.streaming import FusedStreamPool, ResamplingStreamPool  # noqa: E402

SR, S, HOPS, SLOTS = 8000, 10, 8, 32
WARM, TIMED, REPS = 5, 200, 5


def _stats(t):
    t = sorted(t)
    return {"ms_per_push_median": round(t[len(t) // 2], 4), "ms_per_push_min": round(t[0], 4), "ms_per_push_max": round(t[-1], 4)}


def _time(push, audio, n):
    for i in range(WARM):
        push(audio[:, i * n:(i + 1) * n])
    out = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(WARM, WARM + TIMED):
            push(audio[:, i * n:(i + 1) * n])
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0) / TIMED)
    return _stats(out)


def measure_plain(model, graph, dev):
    pool = FusedStreamPool(model, slots=SLOTS, max_chunk_frames=16, graph=graph)
    for _ in range(SLOTS):
        pool.open()
    n, each = HOPS * S, [HOPS] * SLOTS
    audio = torch.randn(SLOTS, (WARM + TIMED) * n, device=dev) * 0.1
    return _time(lambda c: pool.push(c, each), audio, n)


def measure_rate(model, graph, dev, rate_in, rate_out, zeros):
    pool = ResamplingStreamPool(model, slots=SLOTS, max_chunk_frames=16, input_rate=rate_in, output_rate=rate_out, zeros=zeros, graph=graph)
    for _ in range(SLOTS):
        pool.open()
    n = HOPS * S * rate_in // SR
    each = [n] * SLOTS
    audio = torch.randn(SLOTS, (WARM + TIMED) * n, device=dev) * 0.1
    return _time(lambda c: pool.push(c, each), audio, n)


def measure_stage(rows, groups, rate_in, rate_out, zeros, dev):
    n = HOPS * S * rate_in // SR
    r = resample.StreamResampler(rows, rate_in, rate_out, n, zeros=zeros, groups=groups, device=dev)
    for g in range(rows // groups):
        r.open(g)
    each = [n] * (rows // groups)
    audio = torch.randn(rows, (WARM + TIMED) * n, device=dev) * 0.1
    return _time(lambda c: r.push(c, each), audio, n)


def latency_ms(rate_in, rate_out, zeros):
    """Algorithmic look-ahead W / orig_sr of the resampler, in ms."""
    up, down = resample.ratio(rate_in, rate_out)
    return round(1e3 * resample.design_filter(up, down, zeros=zeros)[1] / rate_in, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--profile", type=int, default=0)
    args = ap.parse_args()
    dev = "cuda:0"
    torch.manual_seed(0)
    model = ctn.ConvTasNet(256, 20, 256, 512, 3, 8, 4, 2, norm_type="cLN", causal=True).to(dev).eval()
    if args.profile:
        pool = ResamplingStreamPool(model, slots=SLOTS, max_chunk_frames=16, input_rate=16000, output_rate=16000)
        for _ in range(SLOTS):
            pool.open()
        audio = torch.randn(SLOTS, (args.profile + 2) * 160, device=dev) * 0.1
        for i in range(args.profile + 2):
            pool.push(audio[:, i * 160:(i + 1) * 160], [160] * SLOTS)
        torch.cuda.synchronize()
        return
    forms = [("16k_16k", 16000, 16000, 32), ("48k_48k", 48000, 48000, 32), ("16k_model", 16000, None, 32), ("16k_16k_z8", 16000, 16000, 8)]
    result = {"config": "N=256 L=20 B=256 H=512 P=3 X=8 R=4 C=2 cLN causal, model at 8 kHz", "slots": SLOTS, "chunk_ms": 10.0,
              "warmup": WARM, "timed_pushes": TIMED, "repetitions": REPS, "pool": {}, "stages": {}}
    for kind, graph in (("eager", False), ("graph", True)):
        rec = {"plain_before": measure_plain(model, graph, dev)}
        for name, rate_in, rate_out, zeros in forms:
            rec[name] = measure_rate(model, graph, dev, rate_in, rate_out, zeros)
            rec[name]["lookahead_ms_in"] = latency_ms(rate_in, SR, zeros)
            rec[name]["lookahead_ms_out"] = latency_ms(SR, rate_out, zeros) if rate_out else 0.0
            torch.cuda.empty_cache()
        rec["plain_after"] = measure_plain(model, graph, dev)
        base = 0.5 * (rec["plain_before"]["ms_per_push_median"] + rec["plain_after"]["ms_per_push_median"])
        for name, _, _, _ in forms:
            rec[name]["added_ms_over_plain"] = round(rec[name]["ms_per_push_median"] - base, 4)
        result["pool"][kind] = rec
        print(json.dumps({kind: rec}), flush=True)
    for name, rows, groups, a, b, zeros in (("in_16k_to_8k", SLOTS, 1, 16000, SR, 32), ("out_8k_to_16k", 2 * SLOTS, 2, SR, 16000, 32),
                                            ("in_48k_to_8k", SLOTS, 1, 48000, SR, 32), ("out_8k_to_48k", 2 * SLOTS, 2, SR, 48000, 32),
                                            ("in_16k_to_8k_z8", SLOTS, 1, 16000, SR, 8), ("out_8k_to_16k_z8", 2 * SLOTS, 2, SR, 16000, 8)):
        result["stages"][name] = measure_stage(rows, groups, a, b, zeros, dev)
        print(json.dumps({name: result["stages"][name]}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
