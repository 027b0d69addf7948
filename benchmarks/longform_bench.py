"""Cost of separating a long recording: forward passes, framing and the three stitch kernels of longform.separate_long
against a torch restatement of the stitch, in ONE process on the GPU.

    python benchmarks/longform_bench.py [--minutes 10,60] [--batch-size 8] [--reps 10] [--out profiles/longform_bench.json]

Paper gLN configuration (N256 L20 B256 H512 P3 X8 R4 C2) with seeded random weights, 8 kHz, segment 32000, hop 16000,
recordings of seeded noise.  Per recording length:
(a) the forward passes over all segments, `batch_size` at a time: host clock around a synchronise, after a warm-up of both
    batch shapes;
(b) framing and each stitch kernel: device events around the C entry point (lib.probe), once in the pipeline right behind the
    forward passes and then `reps` more times (median, min); the kernels' algorithmic bytes (computed from the shapes below)
    over the median time;
(c) a torch restatement of the stitch as a user writes it today: a loop over segment pairs, the C x C cost matrix, the best
    permutation read back per pair, the cross-fade with slice assignments; host clock around a synchronise, one warm-up run.
The device stitch and the restatement are compared (orders, largest difference).  There is no CPU path: without a GPU the
script fails."""
import argparse
import itertools
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SR, SEG, HOP = 8000, 32000, 16000
MODEL = dict(N=256, L=20, B=256, H=512, P=3, X=8, R=4, C=2)


def stitch_bytes(n_seg, n_rec, C, seg, hop, total_samples):
    """The bytes the algorithm needs (fp32): costs read both sides of every overlap and write C * C floats per segment; the
    assembly reads every output sample once, the predecessor's side of every overlap and the two fade tables (once), and
    writes every output sample once; the order reads the costs and writes C int32 per segment."""
    ov, pairs = seg - hop, n_seg - n_rec
    costs = 4 * (pairs * 2 * C * ov + n_seg * C * C)
    order = 4 * (n_seg * C * C + n_seg * C)
    assemble = 4 * (2 * C * total_samples + pairs * C * ov + 2 * ov)
    return {"ctn_longform_costs": costs, "ctn_longform_order": order, "ctn_longform_assemble": assemble}


def torch_stitch(est, T, hop, fi, fo):
    """What a user writes today: [n, C, seg] -> ([C, T], orders), one read-back per segment pair."""
    n, C, seg = est.shape
    ov = seg - hop
    perms_host = list(itertools.permutations(range(C)))
    perms = torch.tensor(perms_host, device=est.device)
    rows = torch.arange(C, device=est.device)
    out = torch.empty((C, T), device=est.device)
    g, orders = list(range(C)), [list(range(C))]
    out[:, :min(T, seg)] = est[0, :, :min(T, seg)]
    prev_local, prev_out = est[0], est[0]
    for i in range(1, n):
        cost = ((prev_local[:, None, hop:] - est[i][None, :, :ov]) ** 2).sum(-1)
        k = int(cost[rows, perms].sum(1).argmin())               # the read-back
        g = [perms_host[k][a] for a in g]
        orders.append(g)
        cur = est[i][g]
        end = T if i == n - 1 else (i + 1) * hop + ov
        out[:, i * hop:i * hop + ov] = fo * prev_out[:, hop:] + fi * cur[:, :ov]
        out[:, i * hop + ov:end] = cur[:, ov:end - i * hop]
        prev_local, prev_out = est[i], cur
    return out, orders


def probe_times(ctn, fn):
    """Run fn() with lib.probe on -> ({entry point: ms}, fn's result)."""
    ctn.lib.probe = []
    try:
        res = fn()
        torch.cuda.synchronize()
        times = {}
        for name, _, e0, e1 in ctn.lib.probe:
            if name.startswith("ctn_longform_"):
                times[name] = times.get(name, 0.0) + e0.elapsed_time(e1)
    finally:
        ctn.lib.probe = None
    return times, res


def run(ctn, model, minutes, batch_size, reps):
    from conv_tasnet_amd import longform
    dev = torch.device("cuda:0")
    C = MODEL["C"]
    T = int(minutes * 60 * SR)
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(minutes * 1000) + 1)
    x = 0.1 * torch.randn(T, device=dev, generator=gen)
    lens, offsets = np.array([T], dtype=np.int64), np.array([0], dtype=np.int64)

    # (b) framing, warmed
    segs, seg_ptr = longform.frame_ragged(x, offsets, lens, SEG, HOP)
    n_seg = int(seg_ptr[-1])
    frame_ms = []
    for _ in range(reps):
        t, _ = probe_times(ctn, lambda: longform.frame_ragged(x, offsets, lens, SEG, HOP))
        frame_ms.append(t["ctn_longform_frame"])

    # (a) forward passes
    with torch.no_grad():
        model(segs[:batch_size])
        if n_seg % batch_size:
            model(segs[:n_seg % batch_size])
        est = torch.empty((n_seg, C, SEG), device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b0 in range(0, n_seg, batch_size):
            est[b0:b0 + batch_size].copy_(model(segs[b0:b0 + batch_size]))
        torch.cuda.synchronize()
        forward_s = time.perf_counter() - t0

    # (b) the stitch: right behind the forward passes (fade tables uploaded by a tiny call first), then repeated
    longform.stitch_ragged(est[:2].contiguous(), [0, 2], [HOP + SEG], HOP)
    torch.cuda.synchronize()
    first, (outs, g) = probe_times(ctn, lambda: longform.stitch_ragged(est, seg_ptr, lens, HOP, return_order=True))
    rep = {k: [] for k in first}
    for _ in range(reps):
        t, _ = probe_times(ctn, lambda: longform.stitch_ragged(est, seg_ptr, lens, HOP))
        for k, v in t.items():
            rep[k].append(v)
    t0 = time.perf_counter()
    longform.stitch_ragged(est, seg_ptr, lens, HOP)
    torch.cuda.synchronize()
    stitch_wall_ms = 1e3 * (time.perf_counter() - t0)
    nbytes = stitch_bytes(n_seg, 1, C, SEG, HOP, T)
    kernels = {}
    for k in sorted(first):
        med = statistics.median(rep[k])
        kernels[k] = {"in_pipeline_ms": round(first[k], 4), "median_ms": round(med, 4), "min_ms": round(min(rep[k]), 4),
                      "algorithmic_bytes": nbytes[k], "gb_per_s_at_median": round(nbytes[k] / (med * 1e-3) / 1e9, 1)}
    stitch_ms = sum(v["median_ms"] for v in kernels.values())
    stitch_gbs = sum(nbytes.values()) / (stitch_ms * 1e-3) / 1e9

    # (c) the torch restatement
    fi, fo = (torch.from_numpy(t).to(dev) for t in longform.fade_tables(SEG - HOP))
    torch_stitch(est[:4], 2 * SEG + HOP, HOP, fi, fo)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ref, orders = torch_stitch(est, T, HOP, fi, fo)
    torch.cuda.synchronize()
    torch_ms = 1e3 * (time.perf_counter() - t0)
    same_order = g.cpu().tolist() == orders
    diff = float((ref - outs[0]).abs().max())

    frame_med = statistics.median(frame_ms)
    share = (stitch_ms + frame_med) / (forward_s * 1e3)
    return {"minutes": minutes, "samples": T, "segments": n_seg, "batch_size": batch_size, "forward_s": round(forward_s, 4),
            "segments_per_s": round(n_seg / forward_s, 1), "frame_median_ms": round(frame_med, 4), "frame_min_ms": round(min(frame_ms), 4),
            "frame_gb_per_s": round(4 * (T + n_seg * SEG) / (frame_med * 1e-3) / 1e9, 1), "kernels": kernels,
            "stitch_median_ms": round(stitch_ms, 4), "stitch_in_pipeline_ms": round(sum(first.values()), 4),
            "stitch_wall_ms": round(stitch_wall_ms, 4), "stitch_gb_per_s": round(stitch_gbs, 1), "torch_restatement_ms": round(torch_ms, 2),
            "stitch_plus_frame_over_forward": round(share, 6), "below_one_percent_of_forward": share < 0.01,
            "faster_than_torch": stitch_wall_ms < torch_ms, "orders_equal_torch": same_order, "max_abs_diff_to_torch": diff}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--minutes", default="10,60")
    ap.add_argument("--batch-size", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("longform_bench needs the GPU: there is no CPU path")
    import conv_tasnet_amd as ctn
    torch.manual_seed(0)
    model = ctn.ConvTasNet(**MODEL, norm_type="gLN", causal=False).to("cuda:0").eval()
    results = []
    for minutes in (float(m) for m in a.minutes.split(",")):
        r = run(ctn, model, minutes, a.batch_size, a.reps)
        results.append(r)
        print("%g min: %d segments, forward %.3f s (%.0f segments/s), framing %.3f ms, stitch %.3f ms (%s; %.0f GB/s), torch restatement "
              "%.1f ms, (stitch + framing) / forward = %.4f %%"
              % (minutes, r["segments"], r["forward_s"], r["segments_per_s"], r["frame_median_ms"], r["stitch_median_ms"],
                 ", ".join("%s %.3f" % (k.replace("ctn_longform_", ""), v["median_ms"]) for k, v in r["kernels"].items()),
                 r["stitch_gb_per_s"], r["torch_restatement_ms"], 100 * r["stitch_plus_frame_over_forward"]), flush=True)
    line = json.dumps({"bench": "longform", "model": MODEL, "sample_rate": SR, "segment": SEG, "hop": HOP, "results": results})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
