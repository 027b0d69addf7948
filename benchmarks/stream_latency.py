"""Chunk latency of streaming separation on the causal paper config: the eager-kernel StreamingSeparator(graph=True) (baseline)
against FusedStreamingSeparator, eager and graph=True, in ONE process.

    python benchmarks/stream_latency.py [--out profiles/stream_latency.json] [--chunks 8,16,80] [--batches 1,8,32]

Per (chunk frames, batch): 5 warm-up + 200 timed pushes of random audio, wall clock around a synchronise, five repetitions; prints the
median and the range of ms per chunk, the real-time factor (ms per chunk / ms of audio in a chunk) and the streams sustainable at
real time (batch / RTF), then a markdown table.  --profile N: only N fused eager pushes of 8 frames x 1 stream (for a kernel trace).
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd.streaming import FusedStreamingSeparator, StreamingSeparator  # noqa: E402

SR, S = 8000, 10
WARM, TIMED, REPS = 5, 200, 5


def measure(sep, audio, hops):
    n = hops * S
    with torch.no_grad():
        sep.reset()
        for i in range(WARM):
            sep.push(audio[:, i * n:(i + 1) * n])
        out = []
        for _ in range(REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(WARM, WARM + TIMED):
                sep.push(audio[:, i * n:(i + 1) * n])
            torch.cuda.synchronize()
            out.append(1e3 * (time.perf_counter() - t0) / TIMED)
    return sorted(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--chunks", default="8,16,80")
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--profile", type=int, default=0)
    args = ap.parse_args()
    dev = "cuda:0"
    torch.manual_seed(0)
    model = ctn.ConvTasNet(256, 20, 256, 512, 3, 8, 4, 2, norm_type="cLN", causal=True).to(dev).eval()
    if args.profile:
        sep = FusedStreamingSeparator(model, batch=1, max_chunk_frames=16)
        audio = torch.randn(1, (args.profile + 1) * 8 * S, device=dev) * 0.1
        with torch.no_grad():
            for i in range(args.profile + 1):
                sep.push(audio[:, i * 8 * S:(i + 1) * 8 * S])
        torch.cuda.synchronize()
        return
    rows = []
    for hops in [int(v) for v in args.chunks.split(",")]:
        for batch in [int(v) for v in args.batches.split(",")]:
            audio = torch.randn(batch, (WARM + TIMED) * hops * S, device=dev) * 0.1
            chunk_ms = 1e3 * hops * S / SR
            rec = {"chunk_frames": hops, "chunk_ms": chunk_ms, "batch": batch}
            for name, make in (("baseline_graph", lambda: StreamingSeparator(model, batch=batch, graph=True)),
                               ("fused_eager", lambda: FusedStreamingSeparator(model, batch=batch, max_chunk_frames=max(hops, 16))),
                               ("fused_graph", lambda: FusedStreamingSeparator(model, batch=batch, max_chunk_frames=max(hops, 16), graph=True))):
                sep = make()
                t = measure(sep, audio, hops)
                med = t[len(t) // 2]
                rec[name] = {"ms_per_chunk_median": round(med, 4), "ms_per_chunk_min": round(t[0], 4), "ms_per_chunk_max": round(t[-1], 4),
                             "real_time_factor": round(med / chunk_ms, 5), "streams_at_real_time": round(batch / (med / chunk_ms), 1)}
                del sep
                torch.cuda.empty_cache()
            rec["fused_range_below_baseline_range"] = bool(max(rec["fused_eager"]["ms_per_chunk_max"], rec["fused_graph"]["ms_per_chunk_max"])
                                                           < rec["baseline_graph"]["ms_per_chunk_min"])
            print(json.dumps(rec), flush=True)
            rows.append(rec)
    print("\n| chunk (frames / ms) | streams | baseline graph ms (range) | fused eager ms (range) | fused graph ms (range) | RTF base / fused graph | "
          "streams at real time base / fused graph |\n|---|---|---|---|---|---|---|")
    for r in rows:
        b, e, g = r["baseline_graph"], r["fused_eager"], r["fused_graph"]
        print("| %d / %g | %d | %.3f (%.3f-%.3f) | %.3f (%.3f-%.3f) | %.3f (%.3f-%.3f) | %.4f / %.4f | %.0f / %.0f |"
              % (r["chunk_frames"], r["chunk_ms"], r["batch"], b["ms_per_chunk_median"], b["ms_per_chunk_min"], b["ms_per_chunk_max"],
                 e["ms_per_chunk_median"], e["ms_per_chunk_min"], e["ms_per_chunk_max"], g["ms_per_chunk_median"], g["ms_per_chunk_min"],
                 g["ms_per_chunk_max"], b["real_time_factor"], g["real_time_factor"], b["streams_at_real_time"], g["streams_at_real_time"]))
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"config": "N=256 L=20 B=256 H=512 P=3 X=8 R=4 C=2 cLN causal, 8 kHz", "warmup": WARM, "timed_chunks": TIMED,
                       "repetitions": REPS, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
