"""Cost of the active speech level meter (levels.active_level_ragged, csrc/ctn_levels.hip) on synthetic corpora.

    python benchmarks/levels_bench.py [--out profiles/levels_bench.json] [--corpora 1h8k,10h8k,1h16k,row1h8k] [--profile NAME]

Per corpus (utterances of 2 .. 15 s of gated noise generated on the device; row1h8k: ONE row of an hour):
(a) ms per active_level_ragged call: wall clock around a synchronise (tables, the launches, the copy back and the level on the
    host), and the device time of its ctn_active_level calls by events; 2 warm-up + 5 timed calls, median and range.
(b) ms of ctn_dynmix_levels on the same corpus by events, the same counts: the RMS pass, one read of the corpus.
(c) the numpy/scipy restatement (tests/levels_oracle.py: lfilter chains, exponents, hangover, bins) on a 60 s subsample on the
    host (the better of two runs), scaled to the corpus' duration.
--profile NAME: three calls on that corpus and nothing else (for a kernel trace in a run of its own).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WARM, TIMED = 2, 5
CORPORA = {"1h8k": (8000, 1.0, False), "10h8k": (8000, 10.0, False), "1h16k": (16000, 1.0, False), "row1h8k": (8000, 1.0, True)}


def make_corpus(fs, hours, one_row, dev, seed=0):
    """-> (flat float32 device tensor, offsets, lens): noise in bursts of 0.1 .. 0.6 s at 60 % duty, generated on the device."""
    import torch
    rng = np.random.default_rng(seed)
    total = int(hours * 3600 * fs)
    if one_row:
        lens = np.array([total], dtype=np.int64)
    else:
        lens = []
        while sum(lens) < total:
            lens.append(int(rng.integers(2 * fs, 15 * fs + 1)))
        lens = np.array(lens, dtype=np.int64)
    n = int(lens.sum())
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    flat = torch.randn(n, device=dev, generator=g) * 0.1
    block = fs // 10                                             # gate in blocks of 0.1 s
    gate = (torch.rand((n + block - 1) // block, device=dev, generator=g) < 0.6).float()
    flat *= gate.repeat_interleave(block)[:n]
    return flat.contiguous(), np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64), lens


def summary(ms):
    ms = sorted(ms)
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def time_meter(flat, offsets, lens, fs):
    import torch
    from conv_tasnet_amd import levels
    from conv_tasnet_amd._lib import lib
    wall, device = [], []
    for i in range(WARM + TIMED):
        torch.cuda.synchronize()
        lib.probe = []
        t0 = time.perf_counter()
        out = levels.active_level_ragged(flat, offsets, lens, fs)
        torch.cuda.synchronize()
        dt = 1e3 * (time.perf_counter() - t0)
        calls, lib.probe = lib.probe, None
        if i >= WARM:
            wall.append(dt)
            device.append(sum(e0.elapsed_time(e1) for name, _, e0, e1 in calls if name == "ctn_active_level"))
    return out, summary(wall), summary(device), len([c for c in calls if c[0] == "ctn_active_level"])


def time_rms(flat, offsets, lens):
    import torch
    from conv_tasnet_amd._lib import lib
    dev = flat.device
    off_d, len_d = torch.from_numpy(offsets).to(dev), torch.from_numpy(lens).to(dev)
    msq = torch.empty(len(lens), dtype=torch.float64, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for i in range(WARM + TIMED):
        e0.record()
        lib.call("ctn_dynmix_levels", flat.data_ptr(), flat.numel(), off_d.data_ptr(), len_d.data_ptr(), len(lens), msq.data_ptr(),
                 torch.cuda.current_stream(dev).cuda_stream)
        e1.record()
        torch.cuda.synchronize()
        if i >= WARM:
            ms.append(e0.elapsed_time(e1))
    return summary(ms)


def time_host(flat, fs, seconds=60):
    """The restatement's scipy form on the first `seconds` of the corpus, on the host: ms."""
    import levels_oracle as LO
    x = flat[:seconds * fs].cpu().numpy()
    best = None
    for _ in range(2):                                           # the better of two: the first call also pays scipy's import
        t0 = time.perf_counter()
        y = LO.scipy_band(x, fs)
        ssq = float(np.sum(y * y))
        e = LO.exponents(LO.scipy_envelope(y, fs))
        emax, counts = LO.occupancy(e, LO.design(fs, 1)["nh"])
        lv = LO.level(ssq, len(y), emax, counts)
        dt = 1e3 * (time.perf_counter() - t0)
        best = dt if best is None else min(best, dt)
    return best, lv["level_db"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--corpora", default="1h8k,10h8k,1h16k,row1h8k")
    ap.add_argument("--profile", default="", metavar="NAME")
    args = ap.parse_args()
    import torch
    from conv_tasnet_amd import levels
    dev = torch.device("cuda", 0)
    if args.profile:
        fs, hours, one_row = CORPORA[args.profile]
        flat, offsets, lens = make_corpus(fs, hours, one_row, dev)
        for _ in range(3):
            levels.active_level_ragged(flat, offsets, lens, fs)
        torch.cuda.synchronize()
        return
    res = {"warmup_calls": WARM, "timed_calls": TIMED, "chunk": int(levels.lib.ctn_active_level_chunk()), "corpora": {}}
    for name in args.corpora.split(","):
        fs, hours, one_row = CORPORA[name]
        flat, offsets, lens = make_corpus(fs, hours, one_row, dev)
        out, wall, device, ncalls = time_meter(flat, offsets, lens, fs)
        rms = time_rms(flat, offsets, lens)
        host_ms, host_db = time_host(flat, fs)
        r = {"sample_rate": fs, "utterances": len(lens), "samples": int(lens.sum()), "hours": round(int(lens.sum()) / fs / 3600, 3),
             "active_level_ragged_wall": wall, "ctn_active_level_device": device, "ctn_active_level_calls": ncalls,
             "ctn_dynmix_levels_device": rms, "device_ratio_to_rms_pass": round(device["median_ms"] / rms["median_ms"], 2),
             "host_scipy_60s_ms": round(host_ms, 1), "host_scipy_scaled_ms": round(host_ms * int(lens.sum()) / (60 * fs), 0),
             "median_level_db": round(float(np.median(out["level_db"])), 3), "median_activity": round(float(np.median(out["activity"])), 4)}
        res["corpora"][name] = r
        print(name, json.dumps(r), flush=True)
        del flat
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
