"""Cost of a training minibatch: DynamicMixLoader.fill() on a device-resident corpus against the wav-file path
(data.AudioDataLoader with four workers + the three host-to-device copies), in ONE process.

    python benchmarks/dynmix_bench.py [--out profiles/dynmix_bench.json] [--batches 8,64] [--step-ms MS | --run-bench]
                                      [--speeds 95:105] [--resample-utterances 500]

(a) ms per fill(): 5 warm-up + 200 timed calls, wall clock around a synchronise, five repetitions, median and range -- for
    both forms of ctn_dynmix_gather (mode 0: two launches over (T/1024, B) workgroups; mode 1: one workgroup per mixture),
    alternating between them inside every repetition.
(b) the same job through files: mixtures and sources of the same corpus as int16 wav files in a temporary directory,
    AudioDataLoader(AudioDataset(...), shuffle=True, num_workers=4) as train.py builds it, plus the .to(device) copies:
    minibatches per second over at least 200 minibatches after a warm epoch (page cache warm).  The files are removed.
(c) the training step for scale: --step-ms, or --run-bench (bench.py --gpus 1 in a child process).
(d) --speeds LO:HI: leg (a) also with speed perturbation over every integer percent of the range (loaders mode0_speeds and
    mode1_speeds, alternating with the two plain ones), and the one-off cost of a corpus that arrives at 16 kHz:
    DeviceCorpus.from_arrays(..., sample_rates=16000, target_rate=8000) over --resample-utterances utterances (upload, the
    resample on the device, levels), against the same utterances uploaded at 8 kHz.
--profile N: only N fill() calls at B = 8 (for a kernel trace; with --speeds the perturbed loader).  --dry-run: corpus and
file generation only, no device.
"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SR, T, C = 8000, 32000, 2
WARM, TIMED, REPS = 5, 200, 5


def make_corpus(n_utt, n_spk, seed=0, rate=SR):
    """n_utt utterances of 4 .. 12 s of modulated noise over n_spk speakers."""
    rng = np.random.default_rng(seed)
    arrays = []
    for u in range(n_utt):
        n = int(rng.integers(4 * rate, 12 * rate + 1))
        x = rng.standard_normal(n, dtype=np.float32) * np.float32(rng.uniform(0.02, 0.2))
        x *= (1.0 + 0.5 * np.sin(np.arange(n, dtype=np.float32) / (700.0 * rate / SR)))
        arrays.append(x)
    return arrays, ["spk%03d" % (u % n_spk) for u in range(n_utt)]


def write_mixture_files(arrays, n_mix, root, seed=1):
    """n_mix two-speaker mixtures ('min' length) of the corpus as int16 wav files + the {mix,s1,s2}.json manifests of data.py."""
    from scipy.io import wavfile
    rng = np.random.default_rng(seed)
    infos = {"mix": [], "s1": [], "s2": []}
    for k in infos:
        os.makedirs(os.path.join(root, k), exist_ok=True)
    nbytes = 0
    for i in range(n_mix):
        a, b = rng.choice(len(arrays), size=2, replace=False)
        n = min(len(arrays[a]), len(arrays[b]))
        s1, s2 = arrays[a][:n], arrays[b][:n]
        mix = s1 + s2
        scale = 0.9 / max(float(np.abs(mix).max()), float(np.abs(s1).max()), float(np.abs(s2).max()))
        for k, x in (("mix", mix), ("s1", s1), ("s2", s2)):
            p = os.path.join(root, k, "%05d.wav" % i)
            wavfile.write(p, SR, np.round(x * scale * 32767.0).astype(np.int16))
            infos[k].append([p, n])
            nbytes += 2 * n
    for k, v in infos.items():
        with open(os.path.join(root, k + ".json"), "w") as f:
            json.dump(v, f)
    return nbytes


def time_fill(loaders, bufs):
    """loaders: {name: DynamicMixLoader}; alternates between them inside every repetition -> {name: sorted ms per call}."""
    import torch
    out = {k: [] for k in loaders}
    for k, ld in loaders.items():
        for _ in range(WARM):
            ld.fill(*bufs)
    torch.cuda.synchronize()
    for _ in range(REPS):
        for k, ld in loaders.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(TIMED):
                ld.fill(*bufs)
            torch.cuda.synchronize()
            out[k].append(1e3 * (time.perf_counter() - t0) / TIMED)
    return {k: sorted(v) for k, v in out.items()}


def time_files(json_dir, B, dev, at_least=200):
    import torch
    from conv_tasnet_amd.data import AudioDataLoader, AudioDataset
    loader = AudioDataLoader(AudioDataset(json_dir, B, segment=4.0), shuffle=True, num_workers=4)
    for mixture, lengths, sources in loader:                     # the warm epoch
        mixture, lengths, sources = mixture.to(dev), lengths.to(dev), sources.to(dev)
    torch.cuda.synchronize()
    n, utts, t0 = 0, 0, time.perf_counter()
    while n < at_least:
        for mixture, lengths, sources in loader:
            mixture, lengths, sources = mixture.to(dev), lengths.to(dev), sources.to(dev)
            n += 1
            utts += int(mixture.shape[0])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"minibatches": n, "minibatches_per_epoch": len(loader), "seconds": round(dt, 3), "minibatches_per_s": round(n / dt, 2),
            "ms_per_minibatch": round(1e3 * dt / n, 3), "segments_per_minibatch": round(utts / n, 2)}


def time_resample(n_utt, n_spk, dev):
    """Seconds to build a DeviceCorpus from n_utt utterances at 16 kHz (upload at 16 kHz, resample on the device, levels)
    against the same durations at 8 kHz (upload, levels); the resample kernel alone by device events."""
    import torch
    import conv_tasnet_amd as ctn
    from conv_tasnet_amd import resample
    a16, spk = make_corpus(n_utt, n_spk, seed=3, rate=16000)
    a8 = [np.ascontiguousarray(a[::2]) for a in a16]
    out = {"utterances": n_utt, "samples_16k": int(sum(len(a) for a in a16))}
    for name, arrays, kw in (("from_8k_s", a8, {}), ("from_16k_s", a16, dict(sample_rates=[16000] * n_utt, target_rate=8000))):
        ts = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c = ctn.DeviceCorpus.from_arrays(arrays, spk, dev, **kw)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
            del c
        out[name] = round(min(ts), 3)
    lens = np.array([len(a) for a in a16], dtype=np.int64)
    offs = np.concatenate(([0], np.cumsum(lens)[:-1]))
    x = torch.from_numpy(np.concatenate(a16)).to(dev)
    out_lens = (lens + 1) // 2
    y = torch.empty(int(out_lens.sum()), device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(4):
        e0.record()
        resample.resample_rows(x, offs, lens, 1, 2, y, np.concatenate(([0], np.cumsum(out_lens)[:-1])))
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    out["resample_call_ms"] = round(min(ms[1:]), 3)              # tables upload + the kernel; the first call designs the filter
    return out


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 5), "min_ms": round(ms[0], 5), "max_ms": round(ms[-1], 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--utterances", type=int, default=2000)
    ap.add_argument("--speakers", type=int, default=100)
    ap.add_argument("--batches", default="8,64")
    ap.add_argument("--file-mixtures", type=int, default=800, help="mixtures written as wav files for leg (b)")
    ap.add_argument("--tmp", default=None, help="parent directory of the temporary wav files (default: the system's)")
    ap.add_argument("--no-files", action="store_true", help="skip leg (b)")
    ap.add_argument("--step-ms", type=float, default=None, help="leg (c): a training step time measured in the same session")
    ap.add_argument("--run-bench", action="store_true", help="leg (c): run bench.py --gpus 1 --steps 20 --warmup 5 in a child process")
    ap.add_argument("--profile", type=int, default=0)
    ap.add_argument("--speeds", default=None, metavar="LO:HI", help="leg (d): also time fill() with speed perturbation, e.g. 95:105")
    ap.add_argument("--resample-utterances", type=int, default=500, help="leg (d): utterances of the 16 kHz corpus")
    ap.add_argument("--dry-run", action="store_true")
    args = ap.parse_args()
    batches = [int(b) for b in args.batches.split(",")]

    t0 = time.perf_counter()
    arrays, speakers = make_corpus(args.utterances, args.speakers)
    nsamp = sum(len(a) for a in arrays)
    print("corpus: %d utterances, %d speakers, %d samples (%.2f h), generated in %.1f s"
          % (len(arrays), args.speakers, nsamp, nsamp / SR / 3600, time.perf_counter() - t0), flush=True)
    tmp = None
    res = {"corpus": {"utterances": len(arrays), "speakers": args.speakers, "samples": nsamp}, "T": T, "C": C,
           "warmup_calls": WARM, "timed_calls": TIMED, "repetitions": REPS, "fill": {}, "files": {}}
    try:
        if not args.no_files and not args.profile:
            tmp = tempfile.mkdtemp(prefix="ctn_dynmix_", dir=args.tmp)
            t0 = time.perf_counter()
            nbytes = write_mixture_files(arrays, args.file_mixtures, tmp)
            res["files"]["written"] = {"mixtures": args.file_mixtures, "bytes": nbytes, "seconds": round(time.perf_counter() - t0, 1)}
            print("wrote %d mixtures (%.0f MB of wav) in %.1f s" % (args.file_mixtures, nbytes / 1e6, time.perf_counter() - t0), flush=True)
        if args.dry_run:
            return
        import torch
        import conv_tasnet_amd as ctn
        from conv_tasnet_amd import dynmix
        dev = torch.device("cuda", 0)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        corpus = ctn.DeviceCorpus.from_arrays(arrays, speakers, dev)
        torch.cuda.synchronize()
        res["corpus"].update({"upload_and_levels_s": round(time.perf_counter() - t0, 2), "device_bytes": corpus.device_bytes(),
                              "formula_4_num_samples": 4 * corpus.num_samples,
                              "torch_memory_allocated_delta": torch.cuda.memory_allocated() - base})
        print("corpus on the device:", res["corpus"], flush=True)
        speeds = None
        if args.speeds:
            from conv_tasnet_amd import resample
            speeds = resample.parse_speed_range(args.speeds)
            res["speeds"] = list(speeds)
        if args.profile:
            ld = ctn.DynamicMixLoader(corpus, 8, T, num_speakers=C, steps_per_epoch=1, rank=0, speeds=speeds)
            bufs = (torch.empty(8, T, device=dev), torch.empty(8, C, T, device=dev))
            for _ in range(args.profile):
                ld.fill(*bufs)
            torch.cuda.synchronize()
            return
        for B in batches:
            bufs = (torch.empty(B, T, device=dev), torch.empty(B, C, T, device=dev))
            loaders = {"mode%d" % m: ctn.DynamicMixLoader(corpus, B, T, num_speakers=C, steps_per_epoch=1, rank=0, gather_mode=m)
                       for m in (0, 1)}
            if speeds:
                loaders.update({"mode%d_speeds" % m: ctn.DynamicMixLoader(corpus, B, T, num_speakers=C, steps_per_epoch=1, rank=0,
                                                                          gather_mode=m, speeds=speeds) for m in (0, 1)})
            ms = time_fill(loaders, bufs)
            res["fill"]["B%d" % B] = {k: dict(summary(v), all_ms=[round(x, 5) for x in v]) for k, v in ms.items()}
            res["fill"]["B%d" % B]["default_mode"] = dynmix.GATHER_MODE
            print("fill B=%d:" % B, {k: summary(v) for k, v in ms.items()}, flush=True)
            if tmp is not None:
                res["files"]["B%d" % B] = time_files(tmp, B, dev)
                print("files B=%d:" % B, res["files"]["B%d" % B], flush=True)
        if speeds:
            res["resample_16k"] = time_resample(args.resample_utterances, args.speakers, dev)
            print("corpus from 16 kHz:", res["resample_16k"], flush=True)
        step_ms = args.step_ms
        if args.run_bench:
            r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"],
                               capture_output=True, text=True, cwd=ROOT)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            if r.returncode != 0 or not line:
                raise RuntimeError("bench.py failed:\n%s\n%s" % (r.stdout[-2000:], r.stderr[-2000:]))
            step_ms = float(json.loads(line[-1])["ms_per_step"])
        if step_ms:
            res["step_ms"] = step_ms
            for B in batches:
                f = res["fill"]["B%d" % B]
                for k in [k for k in f if k.startswith("mode")]:
                    f[k]["share_of_paper_step_B8"] = round(f[k]["median_ms"] / step_ms, 5)
        print(json.dumps(res), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
    finally:
        if tmp is not None:
            shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
