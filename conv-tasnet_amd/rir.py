"""Room impulse responses for the reverberant dynamic mixing (dynmix.DynamicMixLoader(rirs=...), csrc/ctn_dynmix_aug.hip).

    bank = RirBank.from_manifest("rirs.json", 8000, "cuda:0")                      # [[wav_path, n_samples], ...]
    bank = RirBank.from_arrays(synthetic_bank(32, 8000), "cuda:0", early_ms=50.0)  # no RIR data set at hand
    loader = DynamicMixLoader(corpus, 8, 32000, rirs=bank, noise=noise_corpus, snr_db=(-6, 3))

A bank is R responses of 1 .. 8192 taps (about 1 s at 8 kHz) back to back in one flat float32 device buffer, with three
numbers per response taken on the host in float64 (include/ctn_hip.h has the contract, the tests restate it in numpy):
the direct path `direct[r]` = the first index of max |h|, and `early[r]` = the number of leading taps that make the training
target: the direct path and the reflections of the first `early_ms` behind it (early_ms=None: all of them, the target is the
fully reverberant source; 0: the direct path alone).

normalize=True divides every response by sqrt(sum h^2) before the single rounding to float32, so that the reverberant source
keeps roughly the level the plan gave it.  A deliberate approximation (and one of the RMS: a corpus built with
level="active" sees its active level move with the tail as well): it is exact for a white source only, and the early-taps target lies below that level by the energy of the late taps.
"""
import json

import numpy as np
import torch

from . import data as _data

MAX_TAPS = 8192


def build_tables(arrays, sample_rate=8000, early_ms=50.0, normalize=True):
    """The bank's host tables (pure host function, float64 until the one rounding).
    -> dict(bank float32 [sum n_r], offsets int64 [R], lens, direct, early int32 [R])."""
    if len(arrays) == 0:
        raise ValueError("a RIR bank needs at least one response")
    if int(sample_rate) < 1:
        raise ValueError("sample_rate must be positive, got %r" % (sample_rate,))
    if early_ms is not None and not (np.isfinite(early_ms) and early_ms >= 0):
        raise ValueError("early_ms must be None or a non-negative number of milliseconds, got %r" % (early_ms,))
    extra = None if early_ms is None else int(round(float(early_ms) * int(sample_rate) / 1000.0))
    taps, lens, direct, early = [], [], [], []
    for r, a in enumerate(arrays):
        h = np.asarray(a, dtype=np.float64).reshape(-1)
        n = h.shape[0]
        if n < 1:
            raise ValueError("response %d is empty" % r)
        if n > MAX_TAPS:
            raise ValueError("response %d has %d taps, at most %d are supported (truncate it)" % (r, n, MAX_TAPS))
        if not np.all(np.isfinite(h)):
            raise ValueError("response %d holds values that are not finite" % r)
        if normalize:
            energy = float(np.sum(h * h))
            if not energy > 0:
                raise ValueError("response %d is all zeros and cannot be normalised" % r)
            h = h / np.sqrt(energy)
        d = int(np.argmax(np.abs(h)))                       # the first index of the maximum
        taps.append(h.astype(np.float32))
        lens.append(n)
        direct.append(d)
        early.append(n if extra is None else min(n, d + 1 + extra))
    lens = np.asarray(lens, dtype=np.int32)
    offsets = np.concatenate(([0], np.cumsum(lens.astype(np.int64))[:-1])).astype(np.int64)
    return dict(bank=np.concatenate(taps), offsets=offsets, lens=lens, direct=np.asarray(direct, dtype=np.int32),
                early=np.asarray(early, dtype=np.int32))


def synthetic_bank(n, sample_rate=8000, rt60=(0.2, 0.6), seed=0):
    """n synthetic responses (float64 arrays, pure numpy, a function of the arguments alone): a unit direct-path spike at a
    delay of up to 2 ms, behind it Gaussian noise under the exponential envelope 10^(-3 t / RT60) of an RT60 drawn uniformly
    from `rt60` (seconds), truncated where the envelope reaches -60 dB or at 8192 taps.  The tail starts 12 dB below the
    spike, so the spike is the largest tap."""
    lo, hi = float(rt60[0]), float(rt60[1])
    if n < 1 or not 0 < lo <= hi:
        raise ValueError("synthetic_bank(n=%r, rt60=%r): n >= 1 and 0 < rt60[0] <= rt60[1]" % (n, rt60))
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(int(n)):
        delay = int(rng.randint(0, int(0.002 * sample_rate) + 1))
        t60 = float(rng.uniform(lo, hi))
        tail = min(int(np.ceil(t60 * sample_rate)), MAX_TAPS - delay - 1)
        h = np.zeros(delay + 1 + tail, dtype=np.float64)
        h[delay] = 1.0
        t = np.arange(1, tail + 1, dtype=np.float64) / sample_rate
        h[delay + 1:] = np.clip(0.25 * rng.randn(tail), -0.9, 0.9) * 10.0 ** (-3.0 * t / t60)
        out.append(h)
    return out


class RirBank:
    """R room impulse responses in device memory: bank (flat float32), offsets [R] int64, lens / direct / early [R] int32."""

    def __init__(self, arrays, device, sample_rate=8000, early_ms=50.0, normalize=True):
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("RirBank lives on the GPU: got device %s" % device)
        self.host = build_tables(arrays, sample_rate, early_ms, normalize)
        self.device, self.sample_rate, self.early_ms, self.normalize = device, int(sample_rate), early_ms, bool(normalize)
        self.bank = torch.from_numpy(self.host["bank"]).to(device)
        self.offsets = torch.from_numpy(self.host["offsets"]).to(device)
        self.lens = torch.from_numpy(self.host["lens"]).to(device)
        self.direct = torch.from_numpy(self.host["direct"]).to(device)
        self.early = torch.from_numpy(self.host["early"]).to(device)

    @classmethod
    def from_arrays(cls, arrays, device, sample_rate=8000, early_ms=50.0, normalize=True):
        return cls(arrays, device, sample_rate, early_ms, normalize)

    @classmethod
    def from_manifest(cls, json_path, sample_rate, device, early_ms=50.0, normalize=True, reader=None):
        """json list of (wav_path, n_samples): every file is read once.  A file at another rate is a ValueError."""
        with open(json_path, "r") as f:
            infos = json.load(f)
        reader = _data.read_wav if reader is None else reader
        arrays = []
        for info in infos:
            path, n = info[0], info[1]
            x = reader(path, sample_rate)
            if x.shape[0] != int(n):
                raise ValueError("%s has %d samples, the manifest says %d" % (path, x.shape[0], int(n)))
            arrays.append(x)
        return cls(arrays, device, sample_rate, early_ms, normalize)

    num_responses = property(lambda self: len(self.host["lens"]))
    # True where no response has late taps: the targets are the reverberant sources themselves, no second set of rows
    full_targets = property(lambda self: bool(np.all(self.host["early"] == self.host["lens"])))

    def device_bytes(self):
        return sum(t.numel() * t.element_size() for t in (self.bank, self.offsets, self.lens, self.direct, self.early))
