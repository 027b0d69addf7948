"""Cost of a noisy and reverberant training minibatch: DynamicMixLoader.fill() with noise, with reverberation at three response
lengths, and with everything including speed perturbation, against the plain loader, all in ONE process.

    python benchmarks/dynmix_aug_bench.py [--out profiles/dynmix_aug_bench.json] [--step-ms MS] [--profile NAME]

ms per fill() at B = 8, C = 2, T = 32000: 5 warm-up + 200 timed calls, wall clock around a synchronise, five repetitions,
alternating between the loaders inside every repetition (dynmix_bench.time_fill), median and range.  The loaders:
    plain               the loader without the options: the baseline
    noise               a noise corpus of 200 files, SNR in [-6, 3] dB
    reverb2048 / reverb4096 / reverb8192
                        a bank of 32 synthetic responses (RT60 1.5 s: the envelope outlasts 8192 taps) truncated to that many taps,
                        early_ms = 50: the early-taps targets are a second set of rows
    everything          noise + reverb4096 + speeds 95:105
Every reverb loader is set beside the VALU floor of its convolution: 2 * B * C * T * mean(n) lane-operations (one multiply and
one add per tap and output, nothing fuses: the rounding order is the contract) at 78.6e12 per second, half the 157.3 TFLOPS
vector peak.  `over_plain_ms` is what the options add to the same run's plain fill(); the floor ratio divides that by the floor.
--step-ms: a training step measured in the same session, for scale.  --profile NAME: 20 fill() calls of that loader only (for
a kernel trace).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "benchmarks"))

from dynmix_bench import C, SR, T, make_corpus, summary, time_fill  # noqa: E402

B = 8
VALU_LANE_OPS_PER_S = 78.6e12
TAPS = (2048, 4096, 8192)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--utterances", type=int, default=2000)
    ap.add_argument("--speakers", type=int, default=100)
    ap.add_argument("--step-ms", type=float, default=None)
    ap.add_argument("--profile", default="")
    args = ap.parse_args()

    import torch
    import conv_tasnet_amd as ctn
    from conv_tasnet_amd import resample, rir
    dev = torch.device("cuda", 0)
    arrays, speakers = make_corpus(args.utterances, args.speakers)
    corpus = ctn.DeviceCorpus.from_arrays(arrays, speakers, dev)
    noise_arrays, _ = make_corpus(200, 1, seed=7)
    noise = ctn.DeviceCorpus.from_arrays(noise_arrays, ["noise"] * len(noise_arrays), dev)
    long = rir.synthetic_bank(32, SR, rt60=(1.5, 1.5), seed=0)
    assert all(len(h) == rir.MAX_TAPS for h in long)
    banks = {n: ctn.RirBank.from_arrays([h[:n] for h in long], dev, SR, early_ms=50.0) for n in TAPS}
    kw = dict(num_speakers=C, steps_per_epoch=1, rank=0)
    make = {"plain": lambda: ctn.DynamicMixLoader(corpus, B, T, **kw),
            "noise": lambda: ctn.DynamicMixLoader(corpus, B, T, noise=noise, **kw),
            "everything": lambda: ctn.DynamicMixLoader(corpus, B, T, noise=noise, rirs=banks[4096],
                                                       speeds=resample.parse_speed_range("95:105"), **kw)}
    for n in TAPS:
        make["reverb%d" % n] = (lambda n=n: ctn.DynamicMixLoader(corpus, B, T, rirs=banks[n], **kw))
    bufs = (torch.empty(B, T, device=dev), torch.empty(B, C, T, device=dev))
    if args.profile:
        ld = make[args.profile]()
        for _ in range(20):
            ld.fill(*bufs)
        torch.cuda.synchronize()
        return
    ms = time_fill({k: f() for k, f in make.items()}, bufs)
    res = {"B": B, "C": C, "T": T, "fill": {k: dict(summary(v), all_ms=[round(x, 5) for x in v]) for k, v in ms.items()}}
    plain = res["fill"]["plain"]["median_ms"]
    for k, f in res["fill"].items():
        f["over_plain_ms"] = round(f["median_ms"] - plain, 5)
        taps = int(k[6:]) if k.startswith("reverb") else 4096 if k == "everything" else 0
        if taps:
            f["valu_floor_ms"] = round(1e3 * 2.0 * B * C * T * taps / VALU_LANE_OPS_PER_S, 5)
            f["over_plain_per_floor"] = round(f["over_plain_ms"] / f["valu_floor_ms"], 2)
        if args.step_ms:
            f["share_of_step"] = round(f["median_ms"] / args.step_ms, 5)
    if args.step_ms:
        res["step_ms"] = args.step_ms
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
