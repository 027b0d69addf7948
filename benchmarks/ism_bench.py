"""Cost of simulated rooms: the image-source simulator (csrc/ctn_ism.hip) over banks of 64, 256 and 1024 responses drawn with
rt60 0.2 .. 0.6 s at 8 kHz (rir.draw_rooms, 4 positions per room, n_taps = ceil(0.6 * 8000) = 4800), and RirBank.refresh end to end.

    python benchmarks/ism_bench.py [--out profiles/ism_bench.json] [--step-ms 10.25] [--steps-per-epoch 2500] [--oracle-responses 4]

Per bank, in ONE process:
    simulate_ms         ctn_ism_simulate alone: the tables are on the device, 2 warm-up + 5 timed launches between device events
    refresh_ms          bank.refresh(rooms): host tables, upload, the launch, read-back, build_tables on the host, five uploads; wall
                        clock around a synchronise, 1 warm-up + 3 timed calls.  draw_rooms itself (pure numpy) is timed beside it
    images              contributing images (i < n_taps, amp != 0) and lattice entries the pruned walks visited, from the
                        kernel's own counters (a launch of its own, not a timed one), their ratio, and images per second
    oracle              the vectorised numpy restatement (tests/ism_oracle.py) over the first --oracle-responses responses of
                        the bank, scaled to the bank: an EXTRAPOLATION from those few, named as such in the output
    share_of_epoch      refresh_ms over --steps-per-epoch training steps of --step-ms (the README's step of the paper config)
    t60                 the Schroeder T60 of the simulated responses (a line through -5 .. -25 dB of the backward-integrated
                        energy, times 3) over the Eyring value the walls were designed for: median and range, the 64-bank only
No thresholds: nothing is asserted but that no row was flagged.
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

SR = 8000
POSITIONS = 4
BANKS = (64, 256, 1024)


def schroeder_t60(h, fs):
    """T60 from the slope of the backward-integrated energy between -5 and -25 dB; NaN where the decay does not reach -25 dB."""
    e = np.cumsum((h * h)[::-1])[::-1]
    db = 10.0 * np.log10(np.maximum(e / e[0], 1e-300))
    sel = np.nonzero((db <= -5.0) & (db >= -25.0))[0]
    if len(sel) < 8 or db[-1] > -25.0:
        return float("nan")
    slope = np.polyfit(sel / fs, db[sel], 1)[0]
    return float(-60.0 / slope)


def stats3(v):
    v = sorted(v)
    return dict(median_ms=round(v[len(v) // 2], 4), min_ms=round(v[0], 4), max_ms=round(v[-1], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--step-ms", type=float, default=10.25, help="a training step of the paper config (README: 9.9-10.6 ms)")
    ap.add_argument("--steps-per-epoch", type=int, default=2500)
    ap.add_argument("--oracle-responses", type=int, default=4)
    ap.add_argument("--banks", default=",".join(str(b) for b in BANKS))
    args = ap.parse_args()

    import torch
    import conv_tasnet_amd as ctn
    from conv_tasnet_amd import rir
    import ism_oracle as IO
    assert torch.cuda.is_available(), "ism_bench.py measures on the GPU"
    dev = torch.device("cuda", 0)
    n_taps = int(np.ceil(0.6 * SR))
    res = {"sample_rate": SR, "positions_per_room": POSITIONS, "n_taps": n_taps, "rt60": [0.2, 0.6], "banks": {}}
    for R in (int(b) for b in args.banks.split(",")):
        t0 = time.perf_counter()
        rooms = rir.draw_rooms(R // POSITIONS, POSITIONS, SR, rt60=(0.2, 0.6), seed=0, epoch=0)
        draw_ms = 1e3 * (time.perf_counter() - t0)
        other = rir.draw_rooms(R // POSITIONS, POSITIONS, SR, rt60=(0.2, 0.6), seed=0, epoch=1)
        tb = rir.ism_tables(rooms, n_taps)
        tdev = torch.from_numpy(tb["tables"]).to(dev)
        h = torch.empty(R, n_taps, dtype=torch.float64, device=dev)
        counters = torch.zeros(2, dtype=torch.int64, device=dev)
        _, status = rir.simulate_tables(tb, dev, tables_dev=tdev, out=h, stats=counters)
        assert int(status.abs().sum()) == 0
        visited, images = counters.cpu().tolist()
        sim = []
        for it in range(7):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rir.simulate_tables(tb, dev, tables_dev=tdev, out=h)
            e1.record()
            torch.cuda.synchronize()
            if it >= 2:
                sim.append(e0.elapsed_time(e1))
        bank = ctn.RirBank.from_rooms(rooms, dev, n_taps=n_taps)
        ref = []
        for it in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            bank.refresh(other if it % 2 == 0 else rooms)
            torch.cuda.synchronize()
            if it >= 1:
                ref.append(1e3 * (time.perf_counter() - t0))
        n_or = min(args.oracle_responses, R)
        t0 = time.perf_counter()
        for r in range(n_or):
            g, p = divmod(r, POSITIONS)
            IO.simulate(dict(L=rooms["L"][g], mic=rooms["mic"][g], beta=rooms["beta"][g]), rooms["src"][g, p], n_taps, SR)
        oracle_s = (time.perf_counter() - t0) / max(n_or, 1) * R
        s, f = stats3(sim), stats3(ref)
        out = {"rooms": R // POSITIONS, "simulate": s, "refresh": f, "draw_rooms_ms": round(draw_ms, 2),
               "images_contributing": images, "lattice_entries_visited": visited, "visited_per_image": round(visited / images, 3),
               "images_per_s": round(images / (s["median_ms"] * 1e-3), 0),
               "oracle_s_extrapolated_from_%d_responses" % n_or: round(oracle_s, 2),
               "refresh_share_of_epoch": round(f["median_ms"] / (args.step_ms * args.steps_per_epoch), 6)}
        if R == min(int(b) for b in args.banks.split(",")):
            hh = h.cpu().numpy()
            ratio = np.array([schroeder_t60(hh[r], SR) / rooms["rt60"][r // POSITIONS] for r in range(R)])
            ok = ratio[np.isfinite(ratio)]
            out["t60_measured_over_designed"] = dict(median=round(float(np.median(ok)), 3), min=round(float(ok.min()), 3),
                                                     max=round(float(ok.max()), 3), responses=int(len(ok)), of=R)
        res["banks"][str(R)] = out
    res["step_ms"], res["steps_per_epoch"] = args.step_ms, args.steps_per_epoch
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
