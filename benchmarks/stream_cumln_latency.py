"""Chunk latency of streaming separation with the cumulative layer norm (norm_type 'cumLN') on the causal paper config, in ONE process:
FusedStreamingSeparator(cumLN model, cumulative=True), eager and graph=True, against
    (a) StreamingSeparator(cumLN model, graph=True): what served such a model before, and
    (b) FusedStreamingSeparator on the cLN model of the same widths: what the cumulative statistics cost on the same kernels.

    python benchmarks/stream_cumln_latency.py [--out profiles/stream_cumln_latency.json] [--chunks 8,16] [--long 80] [--batches 1,8,32]

The protocol is benchmarks/stream_latency.py's (its `measure`): per (chunk frames, batch) 5 warm-up + 200 timed pushes of random audio,
wall clock around a synchronise, five repetitions, median and range of ms per push.  --long: pushes of that many hops, which the
cumulative class runs as consecutive 16-frame steps and the cLN class (max_chunk_frames = that many) as one step: what the one-tile
limit costs.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd.streaming import FusedStreamingSeparator, StreamingSeparator  # noqa: E402
from stream_latency import REPS, S, SR, TIMED, WARM, measure  # noqa: E402

CONFIG = (256, 20, 256, 512, 3, 8, 4, 2)


def stats(t, chunk_ms, batch):
    med = t[len(t) // 2]
    return {"ms_per_chunk_median": round(med, 4), "ms_per_chunk_min": round(t[0], 4), "ms_per_chunk_max": round(t[-1], 4),
            "real_time_factor": round(med / chunk_ms, 5), "streams_at_real_time": round(batch / (med / chunk_ms), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--chunks", default="8,16")
    ap.add_argument("--long", type=int, default=80)
    ap.add_argument("--batches", default="1,8,32")
    args = ap.parse_args()
    dev = "cuda:0"
    torch.manual_seed(0)
    cum = ctn.ConvTasNet(*CONFIG, norm_type="cumLN", causal=True).to(dev).eval()
    cln = ctn.ConvTasNet(*CONFIG, norm_type="cLN", causal=True).to(dev).eval()
    cln.load_state_dict(cum.state_dict())                    # the parameters and keys of a cumLN model are a cLN model's
    chunks = [int(v) for v in args.chunks.split(",")]
    rows = []
    for hops in chunks + ([args.long] if args.long else []):
        long = hops not in chunks
        for batch in [int(v) for v in args.batches.split(",")]:
            audio = torch.randn(batch, (WARM + TIMED) * hops * S, device=dev) * 0.1
            chunk_ms = 1e3 * hops * S / SR
            rec = {"chunk_frames": hops, "chunk_ms": chunk_ms, "batch": batch, "steps_per_push_cumln": -(-hops // 16)}
            makers = [("cumln_fused_eager", lambda: FusedStreamingSeparator(cum, batch=batch, max_chunk_frames=16, cumulative=True)),
                      ("cumln_fused_graph", lambda: FusedStreamingSeparator(cum, batch=batch, max_chunk_frames=16, graph=True, cumulative=True)),
                      ("cln_fused_eager", lambda: FusedStreamingSeparator(cln, batch=batch, max_chunk_frames=max(hops, 16)))]
            if not long:
                makers.append(("cumln_chain_graph", lambda: StreamingSeparator(cum, batch=batch, graph=True)))
            for name, make in makers:
                sep = make()
                rec[name] = stats(measure(sep, audio, hops), chunk_ms, batch)
                del sep
                torch.cuda.empty_cache()
            fused = max(rec["cumln_fused_eager"]["ms_per_chunk_max"], rec["cumln_fused_graph"]["ms_per_chunk_max"])
            if not long:
                rec["fused_range_below_chain_range"] = bool(fused < rec["cumln_chain_graph"]["ms_per_chunk_min"])
            rec["cumln_over_cln_eager"] = round(rec["cumln_fused_eager"]["ms_per_chunk_median"] / rec["cln_fused_eager"]["ms_per_chunk_median"], 4)
            print(json.dumps(rec), flush=True)
            rows.append(rec)

    def cell(r):
        return "%.3f (%.3f-%.3f)" % (r["ms_per_chunk_median"], r["ms_per_chunk_min"], r["ms_per_chunk_max"])

    print("\n| push (frames / ms) | streams | chain graph ms (range) | cumLN fused eager | cumLN fused graph | cLN fused eager | cumLN / cLN | "
          "streams at real time chain / cumLN fused |\n|---|---|---|---|---|---|---|---|")
    for r in rows:
        chain = r.get("cumln_chain_graph")
        print("| %d / %g | %d | %s | %s | %s | %s | %.3f | %s / %.0f |"
              % (r["chunk_frames"], r["chunk_ms"], r["batch"], cell(chain) if chain else "-", cell(r["cumln_fused_eager"]),
                 cell(r["cumln_fused_graph"]), cell(r["cln_fused_eager"]), r["cumln_over_cln_eager"],
                 "%.0f" % chain["streams_at_real_time"] if chain else "-", r["cumln_fused_eager"]["streams_at_real_time"]))
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"config": "N=256 L=20 B=256 H=512 P=3 X=8 R=4 C=2 causal, 8 kHz; cumLN and cLN models with the same parameters",
                       "warmup": WARM, "timed_chunks": TIMED, "repetitions": REPS, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
