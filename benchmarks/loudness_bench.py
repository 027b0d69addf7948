"""Cost of the integrated loudness meter (loudness.integrated_loudness_ragged, csrc/ctn_loudness.hip) on synthetic corpora, and of
the loudness draw in the dynamic mixer.

    python benchmarks/loudness_bench.py [--out profiles/loudness_bench.json] [--corpora 1h8k,10h8k,1h16k] [--no-fill]

Per corpus (utterances of 2 .. 15 s of gated noise generated on the device, the corpora of levels_bench.py):
(a) ms per integrated_loudness_ragged call: wall clock around a synchronise (tables, the launches, the copy back and the
    logarithm on the host), and the device time of its ctn_loudness calls by events; 2 warm-up + 5 timed calls, median and range.
(b) ms of ctn_dynmix_levels on the same corpus by events, the same counts: the RMS pass, one read of the corpus.
(c) scipy's lfilter chain (tests/loudness_oracle.py: scipy_k_weight, then the blocks and gates in numpy) on a 60 s subsample on
    the host (the better of two runs), scaled to the corpus' duration.
Then DynamicMixLoader.fill() at B = 8, T = 32000 over a small corpus built with level="loudness": without loudness_db, with
loudness_db=(-33, -25), and with peak="clip" beside it; events around 20 fills after 5 warm-up ones, ms per fill.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "benchmarks"))

from levels_bench import TIMED, WARM, make_corpus, summary, time_rms  # noqa: E402

CORPORA = {"1h8k": (8000, 1.0), "10h8k": (8000, 10.0), "1h16k": (16000, 1.0)}


def time_meter(flat, offsets, lens, fs):
    import torch
    from conv_tasnet_amd import loudness
    from conv_tasnet_amd._lib import lib
    wall, device = [], []
    for i in range(WARM + TIMED):
        torch.cuda.synchronize()
        lib.probe = []
        t0 = time.perf_counter()
        out = loudness.integrated_loudness_ragged(flat, offsets, lens, fs)
        torch.cuda.synchronize()
        dt = 1e3 * (time.perf_counter() - t0)
        calls, lib.probe = lib.probe, None
        if i >= WARM:
            wall.append(dt)
            device.append(sum(e0.elapsed_time(e1) for name, _, e0, e1 in calls if name == "ctn_loudness"))
    return out, summary(wall), summary(device), len([c for c in calls if c[0] == "ctn_loudness"])


def time_host(flat, fs, seconds=60):
    """scipy's lfilter chain and the gating in numpy on the first `seconds` of the corpus, on the host: ms."""
    import loudness_oracle as LO
    x = flat[:seconds * fs].cpu().numpy()
    h = fs // 10
    best = None
    for _ in range(2):                                           # the better of two: the first call also pays scipy's import
        t0 = time.perf_counter()
        y = LO.scipy_k_weight(x, fs)
        S = (y[:len(y) // h * h] ** 2).reshape(-1, h).sum(axis=1)
        z = (S[:-3] + S[1:-2] + S[2:-1] + S[3:]) / (4 * h)
        za = z[z > LO.design(fs, 1)["abs_gate"]]
        zr = za[za > za.mean() / 10.0] if len(za) else za
        lufs = -0.691 + 10.0 * np.log10(zr.mean()) if len(zr) else -np.inf
        dt = 1e3 * (time.perf_counter() - t0)
        best = dt if best is None else min(best, dt)
    return best, float(lufs)


def time_fill(dev, B=8, T=32000, fills=20, warm=5):
    import torch
    import conv_tasnet_amd as ctn
    rng = np.random.default_rng(0)
    arrays = [(0.1 * rng.standard_normal(int(n))).astype(np.float32) for n in rng.integers(5 * 8000, 12 * 8000, size=64)]
    corpus = ctn.DeviceCorpus.from_arrays(arrays, ["s%d" % (u % 16) for u in range(64)], dev, level="loudness", sample_rate=8000)
    mixture, sources = torch.empty(B, T, device=dev), torch.empty(B, 2, T, device=dev)
    out = {}
    for name, kw in (("plain", {}), ("loudness_db", dict(loudness_db=(-33, -25))), ("loudness_db_clip", dict(loudness_db=(-33, -25), peak="clip"))):
        loader = ctn.DynamicMixLoader(corpus, B, T, steps_per_epoch=1000, seed=0, rank=0, **kw)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        runs = []
        for _ in range(TIMED):
            for _ in range(warm):
                loader.fill(mixture, sources)
            e0.record()
            for _ in range(fills):
                loader.fill(mixture, sources)
            e1.record()
            torch.cuda.synchronize()
            runs.append(e0.elapsed_time(e1) / fills)
        out[name] = summary(runs)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--corpora", default="1h8k,10h8k,1h16k")
    ap.add_argument("--no-fill", action="store_true")
    args = ap.parse_args()
    import torch
    from conv_tasnet_amd import loudness
    dev = torch.device("cuda", 0)
    res = {"warmup_calls": WARM, "timed_calls": TIMED, "chunk": int(loudness.lib.ctn_loudness_chunk()), "corpora": {}}
    for name in [n for n in args.corpora.split(",") if n]:
        fs, hours = CORPORA[name]
        flat, offsets, lens = make_corpus(fs, hours, False, dev)
        out, wall, device, ncalls = time_meter(flat, offsets, lens, fs)
        rms = time_rms(flat, offsets, lens)
        host_ms, host_lufs = time_host(flat, fs)
        r = {"sample_rate": fs, "utterances": len(lens), "samples": int(lens.sum()), "hours": round(int(lens.sum()) / fs / 3600, 3),
             "integrated_loudness_ragged_wall": wall, "ctn_loudness_device": device, "ctn_loudness_calls": ncalls,
             "ctn_dynmix_levels_device": rms, "device_ratio_to_rms_pass": round(device["median_ms"] / rms["median_ms"], 2),
             "host_scipy_60s_ms": round(host_ms, 1), "host_scipy_scaled_ms": round(host_ms * int(lens.sum()) / (60 * fs), 0),
             "median_lufs": round(float(np.median(out["lufs"])), 3), "host_60s_lufs": round(host_lufs, 3)}
        res["corpora"][name] = r
        print(name, json.dumps(r), flush=True)
        del flat
        torch.cuda.empty_cache()
    if not args.no_fill:
        res["fill_B8_T32000_ms"] = time_fill(dev)
        print("fill", json.dumps(res["fill_B8_T32000_ms"]), flush=True)
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
