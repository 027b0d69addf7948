"""SDRi throughput of the GPU BSS Eval (bss_eval.py) against the float64 numpy/scipy restatement of mir_eval's algorithm.

Seeded speech-like 2-speaker utterances at 8 kHz (AR(2)-filtered noise under a syllable-rate envelope; the estimates leak
the other speaker and carry noise).  One timed call = cal_SDRi for every utterance of a batch: bss_eval_batch on the two
estimates plus the mixture anchor row, then the SDR improvement, ended by a device synchronise.  The CPU restatement
(tests/bss_oracle.py, FFT correlations + LU as mir_eval) scores the first --cpu-utts utterances of the same inputs; the
largest |dSDRi| between the two is reported.  One JSON line per (seconds, batch).

    python benchmarks/bss_eval_bench.py [--seconds 4 8] [--batch 1 64] [--iters 5] [--warmup 2] [--cpu-utts 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd.bss_eval import bss_eval_batch, sdr_improvement  # noqa: E402
import bss_oracle as BO  # noqa: E402

SR = 8000


def make_batch(seed, B, n):
    pairs = [BO.mixtures(seed + b, 2, n, 0.9) for b in range(B)]
    ref = np.stack([p[0] for p in pairs])
    est = np.stack([p[1] for p in pairs])
    mix = ref.sum(1)
    return ref, est, mix


def gpu_sdri(ref, est_rows, lens):
    sdr, sir, _, fb = bss_eval_batch(ref, est_rows, lens)
    return sdr_improvement(sdr, sir), fb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, nargs="+", default=[4.0, 8.0])
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-utts", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bss_eval_bench needs the GPU")
    dev = torch.device("cuda:0")
    ctn.lib.load()
    for secs in a.seconds:
        n = int(secs * SR)
        for B in a.batch:
            ref, est, mix = make_batch(100, B, n)
            rt = torch.from_numpy(ref).to(dev)
            rows = torch.cat([torch.from_numpy(est), torch.from_numpy(mix)[:, None]], 1).to(dev)
            lens = torch.full((B,), n, dtype=torch.int64, device=dev)
            for _ in range(a.warmup):
                gpu_sdri(rt, rows, lens)
            torch.cuda.synchronize()
            times = []
            for _ in range(a.iters):
                t0 = time.perf_counter()
                sdri, fb = gpu_sdri(rt, rows, lens)
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
            sdri = sdri.cpu().numpy()
            k = min(a.cpu_utts, B)
            t0 = time.perf_counter()
            cpu = [BO.cal_SDRi(ref[b], est[b], mix[b]) for b in range(k)]
            cpu_ms = (time.perf_counter() - t0) / k * 1e3
            med = float(np.median(times))
            res = {"metric": "bss_eval_sdri", "seconds": secs, "batch": B, "utt_per_s": B / med,
                   "ms_per_utt": med / B * 1e3, "call_ms_median": med * 1e3, "call_ms_min": min(times) * 1e3,
                   "cpu_ms_per_utt": cpu_ms, "cpu_threads": torch.get_num_threads(), "speedup_vs_cpu": cpu_ms / (med / B * 1e3),
                   "max_abs_dsdri_db": float(np.max(np.abs(sdri[:k] - np.array(cpu)))), "fallbacks": int(fb.sum()),
                   "mean_sdri_db": float(sdri.mean())}
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
