#!/usr/bin/env python
"""Time the flat optimiser steps alone at the paper size (flat numel of the paper model, padding included), with hip events:
ctn_clip_sgd_step (momentum 0.9 and 0), ctn_clip_adam_l2_step and the existing ctn_clip_adam_step.

Each entry point is two kernels: the sum-of-squares partials of the clip (reads the gradient once) and the update kernel.
The update kernels move 5 (SGD, momentum: p, g, buf read; p, buf written), 3 (SGD, no momentum) and 7 (Adam: p, g, m, v read;
p, m, v written) x numel x 4 bytes; a call adds one more read of the gradient for the partials.

Two timings per entry point, median of --iters calls each (after --warmup calls):
  cold: a 1 GiB buffer is rewritten before every call (outside the events), so the 35-174 MB working set comes from HBM,
        as it does in a training step after the backward pass;
  warm: back-to-back calls (the working set may stay in the 256 MiB Infinity Cache).
The update kernel's own time is in a rocprofv3 --kernel-trace --stats run of this script; --trace splits that run's
kernel trace into cold calls (the kernel follows the flush fill) and warm ones, per kernel, and needs no GPU.

    python benchmarks/optim_only.py [--iters 200] [--warmup 20] [--out FILE.json]
    python benchmarks/optim_only.py --trace prof/p_kernel_trace.csv
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd.train import PAPER  # noqa: E402

PEAK_HBM_TBS = 8.0          # MI355X_MICROARCH.md: HBM3E spec peak
MEASURED_COPY_TBS = 6.29    # the same document: float4 copy


def paper_numel():
    """Flat numel FlatAdam / FlatSGD allocate for the paper model: every tensor rounded up to 4 elements."""
    torch.manual_seed(0)
    m = ctn.ConvTasNet(PAPER['N'], PAPER['L'], PAPER['B'], PAPER['H'], PAPER['P'], PAPER['X'], PAPER['R'], PAPER['C'])
    ps = list(m.parameters())
    return sum(p.numel() for p in ps), sum((p.numel() + 3) // 4 * 4 for p in ps)


# update kernel -> bytes it moves in units of numel * 4 (sumsq: one read of the gradient)
KERNEL_WORDS = {"clip_sgd_kernel<true, false>": 5, "clip_sgd_kernel<false, false>": 3, "clip_adam_l2_kernel": 7,
                "clip_adam_kernel": 7, "sumsq_kernel": 1}


def split_trace(path, n):
    """Median kernel time of cold calls (sumsq right after the flush fill, and the update kernel after that sumsq) and of
    warm ones, with the bytes-based rate and fraction of the HBM peak."""
    import csv
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    times, cold, prev = {}, False, ""
    for r in rows:
        name = r["Kernel_Name"]
        k = name.split("namespace)::", 1)[-1].split("(")[0]        # "clip_sgd_kernel<true, false>", "sumsq_kernel", ...
        k = k if k in KERNEL_WORDS else None
        if k == "sumsq_kernel":
            cold = "FillFunctor" in prev
        if k is not None:
            times.setdefault((k, "cold" if cold else "warm"), []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
        prev = name
    out = []
    for (k, mode), ts in sorted(times.items()):
        us = statistics.median(ts) / 1e3
        b = KERNEL_WORDS[k] * n * 4
        out.append({"kernel": k, "mode": mode, "launches": len(ts), "median_us": round(us, 2), "bytes": b,
                    "GBps": round(b / us / 1e3, 1), "hbm_frac": round(b / (us * 1e-6) / (PEAK_HBM_TBS * 1e12), 3)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", default=None, help="rocprofv3 kernel trace CSV of a run of this script: print the split")
    a = ap.parse_args()
    if a.trace:
        for row in split_trace(a.trace, paper_numel()[1]):
            print(json.dumps(row))
        return
    if not torch.cuda.is_available():
        raise SystemExit("optim_only.py needs the GPU")
    nparams, n = paper_numel()
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    p = torch.randn(n, device=dev, generator=g)
    grad = torch.randn(n, device=dev, generator=g)
    buf = torch.randn(n, device=dev, generator=g)
    m = torch.zeros(n, device=dev)
    v = torch.zeros(n, device=dev)
    ws = torch.empty(ctn.lib.ctn_optim_parts(), dtype=torch.float64, device=dev)
    norm = torch.zeros(1, device=dev)
    flush = torch.empty(1 << 28, device=dev)                 # 1 GiB > the 256 MiB Infinity Cache
    st = torch.cuda.current_stream().cuda_stream
    step = [0]

    def sgd(mom):
        def run():
            ctn.lib.call("ctn_clip_sgd_step", p.data_ptr(), grad.data_ptr(), buf.data_ptr() if mom else 0, n, 1.0, 5.0,
                         1e-9, mom, 0.0, 1e-4, 0, 0, norm.data_ptr(), ws.data_ptr(), st)
        return run

    def adam(l2):
        def run():
            step[0] += 1
            if l2:
                ctn.lib.call("ctn_clip_adam_l2_step", p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), n, 1.0,
                             5.0, 1e-9, 0.9, 0.999, 1e-8, step[0], 1e-4, norm.data_ptr(), ws.data_ptr(), st)
            else:
                ctn.lib.call("ctn_clip_adam_step", p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), n, 1.0, 5.0,
                             1e-9, 0.9, 0.999, 1e-8, step[0], norm.data_ptr(), ws.data_ptr(), st)
        return run

    cases = [("ctn_clip_sgd_step momentum=0.9", sgd(0.9), 5), ("ctn_clip_sgd_step momentum=0", sgd(0.0), 3),
             ("ctn_clip_adam_l2_step", adam(True), 7), ("ctn_clip_adam_step", adam(False), 7)]
    rows = []
    for name, run, words in cases:
        res = {}
        for mode in ("cold", "warm"):
            for _ in range(a.warmup):
                run()
            ts = []
            for _ in range(a.iters):
                if mode == "cold":
                    flush.fill_(float(len(ts)))
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run()
                e1.record()
                ts.append((e0, e1))
            torch.cuda.synchronize()
            res[mode] = statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1 in ts)
        upd_bytes = words * n * 4
        call_bytes = upd_bytes + n * 4
        row = {"entry": name, "numel": n, "update_bytes": upd_bytes, "call_bytes": call_bytes,
               "call_us_cold": round(res["cold"], 2), "call_us_warm": round(res["warm"], 2),
               "call_GBps_cold": round(call_bytes / res["cold"] / 1e3, 1),
               "call_hbm_frac_cold": round(call_bytes / (res["cold"] * 1e-6) / (PEAK_HBM_TBS * 1e12), 3)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "params": nparams, "flat_numel": n, "iters": a.iters,
           "warmup": a.warmup, "peak_hbm_TBps": PEAK_HBM_TBS, "measured_copy_TBps": MEASURED_COPY_TBS, "rows": rows}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
