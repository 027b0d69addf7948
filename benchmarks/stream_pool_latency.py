"""Push latency of the streaming slot pool (FusedStreamPool) on the causal paper config, against FusedStreamingSeparator in ONE process.

    python benchmarks/stream_pool_latency.py [--out profiles/stream_pool_latency.json] [--chunks 8,16,80] [--batches 1,8,32]

Protocol of benchmarks/stream_latency.py: 5 warm-up + 200 timed pushes of random audio, wall clock around a synchronise, five
repetitions; median and range of ms per push.
  (a) uniform load: every slot opened together, equal hops -- the pool, eager and graph=True, against the class, eager and graph=True;
  (b) churn: 32 slots of 10-ms chunks (8 hops), a seeded quarter of the slots idle on each push, one slot closed and reopened every
      50 pushes;
  (c) open(): microseconds per open() (the per-slot reset) of a 32-slot pool, wall clock around a synchronise over 200 open / close.
--profile N: only N eager pool pushes of 8 frames x 1 slot (for a kernel trace).
"""
import argparse
import json
import os
import random
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd.streaming import FusedStreamingSeparator, FusedStreamPool  # noqa: E402

SR, S = 8000, 10
WARM, TIMED, REPS = 5, 200, 5


def _stats(t, chunk_ms=None, batch=None):
    t = sorted(t)
    med = t[len(t) // 2]
    rec = {"ms_per_chunk_median": round(med, 4), "ms_per_chunk_min": round(t[0], 4), "ms_per_chunk_max": round(t[-1], 4)}
    if chunk_ms:
        rec["real_time_factor"] = round(med / chunk_ms, 5)
        rec["streams_at_real_time"] = round(batch / (med / chunk_ms), 1)
    return rec


def measure_class(sep, audio, hops):
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
    return out


def measure_pool(pool, audio, hops):
    """Uniform load: every slot open, `hops` hops each."""
    n, M = hops * S, pool.M
    for _ in range(M):
        pool.open()
    each = [hops] * M
    for i in range(WARM):
        pool.push(audio[:, i * n:(i + 1) * n], each)
    out = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(WARM, WARM + TIMED):
            pool.push(audio[:, i * n:(i + 1) * n], each)
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0) / TIMED)
    return out


def measure_churn(pool, audio, hops, seed=0):
    """A seeded quarter of the slots idle on each push; one slot closed and reopened every 50 pushes (inside the timed window)."""
    n, M = hops * S, pool.M
    rng = random.Random(seed)
    plans = [[0 if m in idle else hops for m in range(M)] for idle in (set(rng.sample(range(M), M // 4)) for _ in range(WARM + TIMED))]
    for _ in range(M):
        pool.open()
    for i in range(WARM):
        pool.push(audio[:, i * n:(i + 1) * n], plans[i])
    out = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(WARM, WARM + TIMED):
            if i % 50 == 0:
                s = (i // 50) % M
                pool.close(s)
                pool.open(s)
            pool.push(audio[:, i * n:(i + 1) * n], plans[i])
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0) / TIMED)
    return out


def measure_open(pool):
    """-> microseconds per open() (device reset of one slot included), five repetitions of 200."""
    out = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(TIMED):
            pool.open(i % pool.M)
            pool.is_open[i % pool.M] = False          # free it again without the tail copy of close()
        torch.cuda.synchronize()
        out.append(1e6 * (time.perf_counter() - t0) / TIMED)
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
        pool = FusedStreamPool(model, slots=1, max_chunk_frames=16)
        pool.open()
        audio = torch.randn(1, (args.profile + 1) * 8 * S, device=dev) * 0.1
        for i in range(args.profile + 1):
            pool.push(audio[:, i * 8 * S:(i + 1) * 8 * S], [8])
        torch.cuda.synchronize()
        return
    rows = []
    for hops in [int(v) for v in args.chunks.split(",")]:
        for batch in [int(v) for v in args.batches.split(",")]:
            audio = torch.randn(batch, (WARM + TIMED) * hops * S, device=dev) * 0.1
            chunk_ms, F = 1e3 * hops * S / SR, max(hops, 16)
            rec = {"chunk_frames": hops, "chunk_ms": chunk_ms, "batch": batch}
            for name, make, fn in (("class_eager", lambda: FusedStreamingSeparator(model, batch=batch, max_chunk_frames=F), measure_class),
                                   ("pool_eager", lambda: FusedStreamPool(model, slots=batch, max_chunk_frames=F), measure_pool),
                                   ("class_graph", lambda: FusedStreamingSeparator(model, batch=batch, max_chunk_frames=F, graph=True), measure_class),
                                   ("pool_graph", lambda: FusedStreamPool(model, slots=batch, max_chunk_frames=F, graph=True), measure_pool)):
                sep = make()
                rec[name] = _stats(fn(sep, audio, hops), chunk_ms, batch)
                del sep
                torch.cuda.empty_cache()
            for kind in ("eager", "graph"):
                p, c = rec["pool_" + kind], rec["class_" + kind]
                rec["pool_over_class_" + kind] = round(p["ms_per_chunk_median"] / c["ms_per_chunk_median"], 4)
                rec["pool_range_above_class_range_" + kind] = bool(p["ms_per_chunk_min"] > c["ms_per_chunk_max"])
            print(json.dumps(rec), flush=True)
            rows.append(rec)
    # (b) churn and (c) open(), 32 slots of 10-ms chunks
    hops, batch = 8, 32
    audio = torch.randn(batch, (WARM + TIMED) * hops * S, device=dev) * 0.1
    churn = {"chunk_frames": hops, "slots": batch, "idle_per_push": batch // 4, "reopen_every": 50}
    for name, graph in (("pool_eager", False), ("pool_graph", True)):
        pool = FusedStreamPool(model, slots=batch, max_chunk_frames=16, graph=graph)
        churn[name] = _stats(measure_churn(pool, audio, hops), 1e3 * hops * S / SR, batch - batch // 4)
        del pool
        torch.cuda.empty_cache()
    print(json.dumps({"churn": churn}), flush=True)
    pool = FusedStreamPool(model, slots=batch, max_chunk_frames=16)
    t = measure_open(pool)
    opened = {"slots": batch, "us_per_open_median": round(t[len(t) // 2], 2), "us_per_open_min": round(t[0], 2), "us_per_open_max": round(t[-1], 2),
              "state_bytes_per_slot": int((pool.state_bytes - 256) // batch)}
    print(json.dumps({"open": opened}), flush=True)

    print("\n| chunk (frames / ms) | slots | class eager ms (range) | pool eager ms (range) | pool / class | class graph ms (range) | "
          "pool graph ms (range) | pool / class |\n|---|---|---|---|---|---|---|---|")
    for r in rows:
        ce, pe, cg, pg = r["class_eager"], r["pool_eager"], r["class_graph"], r["pool_graph"]
        print("| %d / %g | %d | %.3f (%.3f-%.3f) | %.3f (%.3f-%.3f) | %.3f | %.3f (%.3f-%.3f) | %.3f (%.3f-%.3f) | %.3f |"
              % (r["chunk_frames"], r["chunk_ms"], r["batch"], ce["ms_per_chunk_median"], ce["ms_per_chunk_min"], ce["ms_per_chunk_max"],
                 pe["ms_per_chunk_median"], pe["ms_per_chunk_min"], pe["ms_per_chunk_max"], r["pool_over_class_eager"],
                 cg["ms_per_chunk_median"], cg["ms_per_chunk_min"], cg["ms_per_chunk_max"],
                 pg["ms_per_chunk_median"], pg["ms_per_chunk_min"], pg["ms_per_chunk_max"], r["pool_over_class_graph"]))
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"config": "N=256 L=20 B=256 H=512 P=3 X=8 R=4 C=2 cLN causal, 8 kHz", "warmup": WARM, "timed_pushes": TIMED,
                       "repetitions": REPS, "uniform": rows, "churn": churn, "open": opened}, f, indent=1)


if __name__ == "__main__":
    main()
