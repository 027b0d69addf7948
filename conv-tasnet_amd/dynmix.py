"""On-device dynamic mixing: the single-speaker corpus lives in device memory, every training minibatch is drawn and built
there (csrc/ctn_dynmix.hip: one plan launch + the gather per step, no host work, no host synchronisation).

    corpus = DeviceCorpus.from_manifest("tr_sources.json", 8000, "cuda:0")      # [[wav_path, n_samples, speaker], ...]
    loader = DynamicMixLoader(corpus, batch_size=8, segment_len=32000, steps_per_epoch=2500, seed=0)
    for mixture, lengths, sources in loader: ...                                 # the AudioDataLoader contract, on the device

What a mixture is (include/ctn_hip.h has the contract, the tests restate it in numpy): C distinct speakers, one
eligible utterance of each, a uniform start, levels +q / -q hundredths of a dB with q in [1, 250) as the reference's list
generator draws them (tools/create_txt_file_like_wsj0.py:21-22), sources at unit level times 10^(q/2000), summed, everything
rescaled to a peak of 0.9 (tools/matlab-code/create_wav_2speakers.m:111-112).  A minibatch is a pure function of
(seed, rank, epoch, step): a resumed run sees the minibatches of an uninterrupted one.

Files at another rate: `from_manifest(..., resample=True)` / `from_arrays(..., sample_rates=, target_rate=)` resample them on
the device (resample.py, csrc/ctn_resample.hip) before the levels are taken.  Speed perturbation: `speeds=range(95, 106)`
replays every source at a drawn integer percent of its speed, resampled on the device by 100 / pct each step.
Noise and reverberation (csrc/ctn_dynmix_aug.hip): `noise=` a second DeviceCorpus of noise recordings, one segment of it under
every mixture at an SNR drawn from `snr_db`; `rirs=` a rir.RirBank, every source convolved with a drawn room impulse response,
the training targets being its direct path and early reflections.  Both compose with `speeds`.  With a bank of simulated rooms
(rir.RirBank.from_rooms, csrc/ctn_ism.hip) `same_room=True` seats all talkers of a mixture at distinct positions of one drawn
room, and `room_schedule=` refills the bank with new rooms at every epoch.

The 0-dB level of an utterance: `level="rms"` (the default) is the plain RMS of the whole utterance; `level="active"` is the
ITU-T P.56 active speech level, what the MATLAB tool normalises with (create_wav_2speakers.m:89-97, `activlev(s, fs, 'n')`),
measured on the device when the corpus is built (levels.py, csrc/ctn_levels.hip): the energy over the time speech is active, so
pauses in a file no longer move its level.  Noise corpora keep the RMS.
The LibriMix recipe (Cosentino et al. 2020), for LibriSpeech and WHAM! noise: `level="loudness"` measures every utterance's ITU-R
BS.1770 integrated loudness on the device (loudness.py, csrc/ctn_loudness.hip) and `inv_rms` brings it to unit gated K-weighted
power; `loudness_db=(-33, -25)` then gives every source an absolute loudness drawn uniformly from the tenths of a LU in the range
(in place of the relative +-q), `noise_loudness_db=(-38, -30)` does the same for a noise corpus built with level="loudness" (in
place of the SNR), and `peak="clip"` rescales a mixture to 0.9 only if its peak exceeds 0.9.  Differences from the LibriMix
scripts, on purpose: the meter is BS.1770-4 with the Recommendation's filters and exact 100 ms hops (not pyloudnorm's), there is
no per-source clip check before mixing, and the peak is that of the drawn segment.
Difference from the MATLAB tool, on purpose: the peak rescale is per drawn segment (not per whole utterance).
There is no CPU fallback: like the rest of the product path the loader needs the GPU.
"""
import json

import numpy as np
import torch

from . import data as _data
from ._lib import lib

GATHER_MODE = 0     # ctn_dynmix_gather: 0 = chunked, two launches; 1 = one workgroup per mixture (measured)


def level_table():
    """w[q + 249] = 10^(q / 2000), q = -249 .. 249: float32 rounded from float64 on the host."""
    return np.array([10.0 ** (q / 2000.0) for q in range(-249, 250)], dtype=np.float64).astype(np.float32)


def inverse_rms(meansq):
    """1 / sqrt(meansq) in float64, rounded to float32; 0 for silent utterances (never eligible)."""
    meansq = np.asarray(meansq, dtype=np.float64)
    out = np.zeros(meansq.shape, dtype=np.float64)
    live = meansq > 0
    out[live] = 1.0 / np.sqrt(meansq[live])
    return out.astype(np.float32)


def snr_range(snr_db):
    """(lo, hi) in dB -> the integer tenths of a dB (lo10, hi10): at most 1024 values, lo10 <= hi10."""
    try:
        lo, hi = snr_db
        lo10, hi10 = int(round(float(lo) * 10.0)), int(round(float(hi) * 10.0))
    except (TypeError, ValueError, OverflowError):
        raise ValueError("snr_db must be (lo, hi) in dB, got %r" % (snr_db,))
    if lo10 > hi10:
        raise ValueError("empty SNR range %r" % (snr_db,))
    if hi10 - lo10 + 1 > 1024:
        raise ValueError("the SNR range %r holds %d tenths of a dB, at most 1024 are supported" % (snr_db, hi10 - lo10 + 1))
    return lo10, hi10


def snr_table(lo10, hi10):
    """wn[i] = 10^(-(lo10 + i) / 200), i = 0 .. hi10 - lo10: the noise gain at unit RMS for an SNR of (lo10 + i) / 10 dB relative
    to the sources' 0-dB reference level; float32 rounded from float64 on the host."""
    return np.array([10.0 ** (-(lo10 + i) / 200.0) for i in range(hi10 - lo10 + 1)], dtype=np.float64).astype(np.float32)


LOUDNESS_OFFSET_DB = 0.691      # unit gated K-weighted power reads -0.691 LUFS (loudness.OFFSET_DB)
PEAK_MODES = {"always": 0, "clip": 1}


def loudness_range(loudness_db, name="loudness_db"):
    """(lo, hi) in LUFS -> the integer tenths of a LU (lo10, hi10): at most 1024 values, lo10 <= hi10 (parsed like snr_range)."""
    try:
        lo, hi = loudness_db
        lo10, hi10 = int(round(float(lo) * 10.0)), int(round(float(hi) * 10.0))
    except (TypeError, ValueError, OverflowError):
        raise ValueError("%s must be (lo, hi) in LUFS, got %r" % (name, loudness_db))
    if lo10 > hi10:
        raise ValueError("empty %s range %r" % (name, loudness_db))
    if hi10 - lo10 + 1 > 1024:
        raise ValueError("the %s range %r holds %d tenths of a LU, at most 1024 are supported" % (name, loudness_db, hi10 - lo10 + 1))
    return lo10, hi10


def loudness_table(lo10, hi10):
    """wl[i] = 10^(((lo10 + i) / 10 + 0.691) / 20), i = 0 .. hi10 - lo10: the gain that takes an utterance of unit gated K-weighted
    power (-0.691 LUFS) to (lo10 + i) / 10 LUFS; float32 rounded from float64 on the host."""
    return np.array([10.0 ** (((lo10 + i) / 10.0 + LOUDNESS_OFFSET_DB) / 20.0) for i in range(hi10 - lo10 + 1)],
                    dtype=np.float64).astype(np.float32)


def peak_mode(peak):
    """"always" -> 0 (every mixture is rescaled to a peak of 0.9), "clip" -> 1 (only one whose peak exceeds 0.9 is)."""
    if peak not in PEAK_MODES:
        raise ValueError("peak must be 'always' or 'clip', got %r" % (peak,))
    return PEAK_MODES[peak]


def noise_table(lens, meansq, segment_len):
    """noise_ids int32: the noise utterances of at least segment_len samples that are not silent; none is a ValueError."""
    lens, meansq = np.asarray(lens, dtype=np.int64), np.asarray(meansq, dtype=np.float64)
    if int(segment_len) <= 0:
        raise ValueError("segment_len must be positive, got %d" % segment_len)
    ids = np.nonzero((lens >= int(segment_len)) & (meansq > 0))[0].astype(np.int32)
    if len(ids) == 0:
        raise ValueError("no noise utterance of at least %d samples that is not silent" % segment_len)
    if int(lens[ids].max()) - int(segment_len) + 1 >= 1 << 32:
        raise ValueError("a noise utterance of %d samples is too long for a 32-bit start draw" % int(lens[ids].max()))
    return ids


def build_tables(lens, meansq, speakers, segment_len, num_speakers=2):
    """The sampler's tables for one segment length (pure host function).

    Eligible: lens[u] >= segment_len and meansq[u] > 0.  Speakers (sorted by label) without an eligible utterance are
    dropped; fewer than `num_speakers` left is a ValueError.  -> dict(spk_ptr [S+1] int32, utt_ids int32, speakers list,
    lens int64, inv_rms float32, w float32)."""
    lens = np.asarray(lens, dtype=np.int64)
    meansq = np.asarray(meansq, dtype=np.float64)
    if not (len(lens) == len(meansq) == len(speakers)):
        raise ValueError("lens, meansq and speakers differ in length")
    if segment_len <= 0:
        raise ValueError("segment_len must be positive, got %d" % segment_len)
    if len(lens) and int(lens.max()) - segment_len + 1 >= 1 << 32:
        raise ValueError("an utterance of %d samples is too long for a 32-bit start draw" % int(lens.max()))
    by_spk = {}
    for u, s in enumerate(speakers):
        if lens[u] >= segment_len and meansq[u] > 0:
            by_spk.setdefault(str(s), []).append(u)
    names = sorted(by_spk)
    if len(names) < num_speakers:
        raise ValueError("%d speaker(s) with an utterance of at least %d samples that is not silent; mixtures of %d need "
                         "at least as many" % (len(names), segment_len, num_speakers))
    spk_ptr, utt_ids = [0], []
    for s in names:
        utt_ids.extend(by_spk[s])
        spk_ptr.append(len(utt_ids))
    return dict(spk_ptr=np.asarray(spk_ptr, dtype=np.int32), utt_ids=np.asarray(utt_ids, dtype=np.int32), speakers=names,
                lens=lens, inv_rms=inverse_rms(meansq), w=level_table())


def _ptr(t):
    return t.data_ptr() if t is not None else 0


class DeviceCorpus:
    """U single-speaker utterances back to back in one flat float32 device buffer, with their levels."""

    def __init__(self, arrays, speakers, device, sample_rates=None, target_rate=None, level="rms", sample_rate=None):
        device = torch.device(device)
        if level not in ("rms", "active", "loudness"):
            raise ValueError("level must be 'rms', 'active' or 'loudness', got %r" % (level,))
        rate = target_rate if target_rate is not None else sample_rate
        if level != "rms" and rate is None:
            raise ValueError("level=%r needs the corpus' sample rate: pass sample_rate= (or target_rate= when resampling)" % level)
        if device.type != "cuda":
            raise ValueError("DeviceCorpus lives on the GPU: got device %s" % device)
        if len(arrays) == 0 or len(arrays) != len(speakers):
            raise ValueError("%d utterances with %d speaker labels" % (len(arrays), len(speakers)))
        if (sample_rates is None) != (target_rate is None):
            raise ValueError("sample_rates and target_rate go together")
        arrays = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in arrays]
        lens = np.array([a.shape[0] for a in arrays], dtype=np.int64)
        if int(lens.min()) < 1:
            raise ValueError("empty utterance in the corpus")
        self.device = device
        self.speakers = [str(s) for s in speakers]
        if sample_rates is not None and any(int(r) != int(target_rate) for r in sample_rates):
            lens, offsets = self._upload_resampled(arrays, lens, sample_rates, int(target_rate))
        else:
            if sample_rates is not None and len(sample_rates) != len(arrays):
                raise ValueError("%d utterances with %d sample rates" % (len(arrays), len(sample_rates)))
            offsets = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64)
            self.corpus = torch.from_numpy(np.concatenate(arrays)).to(device)
        self.lens_host, self.offsets_host = lens, offsets
        self.offsets = torch.from_numpy(offsets).to(device)
        self.lens = torch.from_numpy(lens).to(device)
        msq = torch.empty(len(arrays), dtype=torch.float64, device=device)
        lib.call("ctn_dynmix_levels", _ptr(self.corpus), self.corpus.numel(), _ptr(self.offsets), _ptr(self.lens), len(arrays),
                 _ptr(msq), torch.cuda.current_stream(device).cuda_stream)
        self._meansq = msq.cpu().numpy()
        self.level = level
        self._level_power, self._activity = self._meansq, None
        if level == "active":
            from . import levels as _levels
            out = _levels.active_level_ragged(self.corpus, offsets, lens, int(rate))
            self._level_power, self._activity = out["level"], out["activity"]
        self._lufs = None
        if level == "loudness":
            from . import loudness as _loudness
            out = _loudness.integrated_loudness_ragged(self.corpus, offsets, lens, int(rate))
            self._level_power, self._lufs = out["power"], out["lufs"]
        self.inv_rms = torch.from_numpy(inverse_rms(self._level_power)).to(device)
        self.w = torch.from_numpy(level_table()).to(device)
        self._tables = {}

    def _upload_resampled(self, arrays, lens, sample_rates, target_rate):
        """Utterances at `target_rate` are uploaded as they are; the others are uploaded at their own rate, one flat buffer per
        source rate, and resampled on the device straight into their place in the corpus.  -> the corpus' (lens, offsets)."""
        from . import resample as _rs
        if len(sample_rates) != len(arrays):
            raise ValueError("%d utterances with %d sample rates" % (len(arrays), len(sample_rates)))
        rates = [int(r) for r in sample_rates]
        ratios = [_rs.ratio(r, target_rate) for r in rates]
        out_lens = np.array([_rs.out_len(n, up, down) for n, (up, down) in zip(lens, ratios)], dtype=np.int64)
        offsets = np.concatenate(([0], np.cumsum(out_lens)[:-1])).astype(np.int64)
        host = np.zeros(int(out_lens.sum()), dtype=np.float32)
        for u, r in enumerate(rates):
            if r == target_rate:
                host[offsets[u]:offsets[u] + out_lens[u]] = arrays[u]
        self.corpus = torch.from_numpy(host).to(self.device)
        for r in sorted(set(rates) - {target_rate}):
            rows = [u for u in range(len(arrays)) if rates[u] == r]
            up, down = _rs.ratio(r, target_rate)
            in_lens = lens[rows]
            in_offsets = np.concatenate(([0], np.cumsum(in_lens)[:-1])).astype(np.int64)
            x = torch.from_numpy(np.concatenate([arrays[u] for u in rows])).to(self.device)
            _rs.resample_rows(x, in_offsets, in_lens, up, down, self.corpus, offsets[rows])
        return out_lens, offsets

    @classmethod
    def from_arrays(cls, arrays, speakers, device, sample_rates=None, target_rate=None, level="rms", sample_rate=None):
        """sample_rates (one per utterance) and target_rate: utterances at another rate are resampled on the device.
        level: "rms", "active" (the ITU-T P.56 active level) or "loudness" (the ITU-R BS.1770 gated loudness); the last two need
        target_rate or sample_rate, the rate of `arrays`."""
        return cls(arrays, speakers, device, sample_rates, target_rate, level, sample_rate)

    @classmethod
    def from_manifest(cls, json_path, sample_rate, device, reader=None, resample=False, level="rms"):
        """json list of (wav_path, n_samples, speaker): every file is read once and uploaded.  reader(path, sample_rate) -> x
        (default data.read_wav: a file at another rate is a ValueError).  resample=True: reader(path) -> (x, file_rate)
        (default data.read_wav_native), files at other rates are resampled on the device; n_samples counts the FILE's samples.
        level: "rms", "active" or "loudness", the 0-dB level of every utterance (measured at `sample_rate`)."""
        with open(json_path, "r") as f:
            infos = json.load(f)
        if reader is None:
            reader = _data.read_wav_native if resample else _data.read_wav
        arrays, rates = [], []
        for path, n, _ in infos:
            if resample:
                x, sr = reader(path)
                rates.append(int(sr))
            else:
                x = reader(path, sample_rate)
            if x.shape[0] != int(n):
                raise ValueError("%s has %d samples, the manifest says %d" % (path, x.shape[0], int(n)))
            arrays.append(x)
        if resample:
            return cls(arrays, [i[2] for i in infos], device, rates, int(sample_rate), level)
        return cls(arrays, [i[2] for i in infos], device, level=level, sample_rate=int(sample_rate))

    num_utterances = property(lambda self: len(self.lens_host))
    num_speakers = property(lambda self: len(set(self.speakers)))
    num_samples = property(lambda self: int(self.corpus.numel()))
    meansq = property(lambda self: self._meansq)
    # the power an utterance's 0-dB level stands for: meansq with level="rms", the active level with "active", the gated K-weighted
    # power with "loudness" (inv_rms = float32(1 / sqrt(level_power)), eligible utterances have level_power > 0); activity: the
    # active level's share of time ("active" only); lufs: the integrated loudness of every utterance ("loudness" only)
    level_power = property(lambda self: self._level_power)
    activity = property(lambda self: self._activity)
    lufs = property(lambda self: self._lufs)

    def device_bytes(self):
        """4 * num_samples for the audio plus the per-utterance tables (offsets, lens, inv_rms) and the level table."""
        return sum(t.numel() * t.element_size() for t in (self.corpus, self.offsets, self.lens, self.inv_rms, self.w))

    def tables(self, segment_len, num_speakers):
        """Sampler tables for one segment length: (host dict of build_tables, spk_ptr and utt_ids on the device)."""
        key = (int(segment_len), int(num_speakers))
        if key not in self._tables:
            host = build_tables(self.lens_host, self._level_power, self.speakers, int(segment_len), int(num_speakers))
            self._tables[key] = (host, torch.from_numpy(host["spk_ptr"]).to(self.device),
                                 torch.from_numpy(host["utt_ids"]).to(self.device))
        return self._tables[key]


class DynamicMixLoader:
    """Yields `steps_per_epoch` minibatches (mixture [B,T] f32, lengths [B] i64 = T, sources [B,C,T] f32) per epoch, all
    on the corpus' device: the AudioDataLoader contract the Solver consumes.

    Iterating rewinds the step word and yields steps 0 .. steps_per_epoch - 1 of the current epoch into fresh tensors
    (`lengths` is one shared constant tensor).  `dataset.set_epoch(epoch)` (the Solver calls it) selects the epoch;
    with reshuffle=False the epoch stays 0: the same minibatches every time, a fixed validation set without mixture files.
    Every rank draws its own stream (`rank` enters the Philox key, the world size does not) and runs the same number of steps.
    gather_mode: the form of ctn_dynmix_gather (None: GATHER_MODE); both give the same bits.
    speeds: None, or integer percents in [50, 200]: every source is replayed at a drawn percent of its speed (one more Philox
    block per source; speaker, utterance and level draws are those of speeds=None), resampled on the device into a segment
    buffer the gather then mixes.  Eligible utterances hold ceil(segment_len * max(speeds) / 100) samples.
    rirs: None, or a rir.RirBank: every source is convolved with a drawn response (one more Philox block per source); `mixture`
    sums the reverberant sources, `sources` holds their early-taps targets (the bank's early_ms), time-aligned with the dry
    source.  The reverberation sees the drawn segment only, not the utterance before it.
    noise: None, or a DeviceCorpus of noise recordings (labels ignored): one segment under every mixture (one more Philox block
    per mixture) at an SNR drawn uniformly from the tenths of a dB in snr_db = (lo, hi), relative to the sources' 0-dB reference
    level (unit RMS or unit active level, as the corpus was built; before the plan's +-q).  The peak rescale to 0.9 covers the
    noisy mixture and the targets.
    With either option the mix is ctn_dynmix_gather_aug, which has the chunked form only (gather_mode plays no part).
    With rirs=None and noise=None the launches and the bits are those of a loader without these arguments.
    min_speakers: None, or m in [1, num_speakers]: every mixture holds a drawn number n_b in [m, C] of speakers (one more Philox
    block per mixture, csrc/ctn_dynmix_active.hip); the plan is that of min_speakers=None with gain[b, c >= n_b] = 0, so
    sources[b, c >= n_b] are zeros that add nothing to the mixture or its peak: training data for varpit.cal_varpit_loss.
    `last_active()` returns the counts.  With None the launches and the bits are those of a loader without the argument.
    same_room: with a bank of simulated rooms (rir.RirBank.from_rooms, which records positions_per_room = P >= C) all sources of a
    mixture get distinct positions of ONE drawn room (ctn_dynmix_plan_rooms in place of the RIR half of ctn_dynmix_plan_aug: same
    key and counters, every other draw of a seed keeps its bits).  A bank without positions_per_room is a ValueError.
    room_schedule: None, or a function epoch -> rooms (rir.draw_rooms): with reshuffle on, set_epoch(e) refills the bank in place
    with rirs.refresh(room_schedule(e)).  With neither argument the launches and the bits are those of a loader without them.
    loudness_db: None, or (lo, hi) in LUFS on a corpus built with level="loudness": every source gets an absolute loudness drawn
    uniformly from the tenths of a LU in the range (at most 1024; one more Philox block per source, ctn_dynmix_plan_loudness behind the
    plan): gain[b,c] = inv_rms[u] * wl[i] replaces the plan's; plan_q is still drawn and ignored, every other draw of a seed keeps its
    bits; the masking by min_speakers comes after.  `last_loudness()` returns the drawn tenths.
    noise_loudness_db: None, or (lo, hi) in LUFS with noise= a corpus built with level="loudness": the word that chooses the SNR
    chooses the noise loudness instead (snr_db plays no part, the snr10 of last_aug_plan() holds its tenths of a LU),
    ngain = noise.inv_rms[v] * wl_n[i]; noise utterance and start keep their bits.
    peak: "always" (every mixture is rescaled to a peak of 0.9) or "clip" (scale = 0.9 / peak only where peak > 0.9, the LibriMix
    rule), in every form of the gather; `last_peak()` is the unscaled peak either way.
    With the three at their defaults the launches and the bits are those of a loader without them."""

    def __init__(self, corpus, batch_size, segment_len, num_speakers=2, steps_per_epoch=1000, seed=0, rank=None,
                 reshuffle=True, gather_mode=None, speeds=None, rirs=None, noise=None, snr_db=(-6, 3), min_speakers=None,
                 same_room=False, room_schedule=None, loudness_db=None, noise_loudness_db=None, peak="always"):
        if rank is None:
            from . import parallel
            rank = torch.distributed.get_rank() if parallel.world_size() > 1 else parallel.env_world()[1]
        seed, rank = int(seed), int(rank)
        if not 0 <= seed < 1 << 48:
            raise ValueError("seed must be in [0, 2^48), got %d" % seed)
        if not 0 <= rank < 1 << 16:
            raise ValueError("rank must be in [0, 2^16), got %d" % rank)
        if not 2 <= int(num_speakers) <= 4:
            raise ValueError("mixtures of 2..4 speakers, got %d" % num_speakers)
        if batch_size < 1 or steps_per_epoch < 1:
            raise ValueError("batch_size and steps_per_epoch must be positive")
        if min_speakers is not None and not 1 <= int(min_speakers) <= int(num_speakers):
            raise ValueError("min_speakers must be in [1, %d], got %r" % (num_speakers, min_speakers))
        self.corpus, self.B, self.T, self.C = corpus, int(batch_size), int(segment_len), int(num_speakers)
        self.steps_per_epoch, self.seed, self.rank, self.reshuffle = int(steps_per_epoch), seed, rank, bool(reshuffle)
        self.gather_mode = GATHER_MODE if gather_mode is None else int(gather_mode)
        self.peak, self.peak_mode = peak, peak_mode(peak)
        self.loudness = None
        if loudness_db is not None:
            if corpus.level != "loudness":
                raise ValueError("loudness_db needs a corpus built with level='loudness', this one has level=%r" % (corpus.level,))
            self.loudness = loudness_range(loudness_db)
        if noise_loudness_db is not None and (noise is None or noise.level != "loudness"):
            raise ValueError("noise_loudness_db needs noise= a corpus built with level='loudness'")
        self.epoch = 0
        self.speeds = None
        if speeds is not None:
            from . import resample as _rs
            self.speeds = _rs.parse_speeds(speeds)
        self.eligible_len = self.T if self.speeds is None else _rs.eligible_len(self.T, self.speeds)
        self.tables, self._spk_ptr, self._utt_ids = corpus.tables(self.eligible_len, self.C)
        dev = corpus.device
        self.device = dev
        self._step = torch.zeros(1, dtype=torch.int32, device=dev)                  # the step word
        self._plan_utt = torch.zeros(self.B, self.C, dtype=torch.int32, device=dev)
        self._plan_start = torch.zeros(self.B, self.C, dtype=torch.int64, device=dev)
        self._plan_q = torch.zeros(self.B, self.C, dtype=torch.int32, device=dev)
        self._gain = torch.zeros(self.B, self.C, dtype=torch.float32, device=dev)
        self._peak = torch.zeros(self.B, dtype=torch.float32, device=dev)
        self._ws = torch.zeros(max(1, lib.ctn_dynmix_gather_workspace(self.B, self.T)), dtype=torch.uint8, device=dev)
        self._lengths = torch.full((self.B,), self.T, dtype=torch.int64, device=dev)
        if self.speeds is not None:
            self._banks = _rs.speed_banks(self.speeds, dev)
            self._pct = torch.tensor(self.speeds, dtype=torch.int32, device=dev)
            self._plan_pct = torch.zeros(self.B, self.C, dtype=torch.int32, device=dev)
            self._seg = _SegmentBuffer(self.B, self.C, self.T, dev)
        self._aug = None
        if rirs is not None or noise is not None:
            self._aug = _Augment(self.B, self.C, self.T, dev, rirs, noise, snr_db, bool(same_room), noise_loudness_db, self.peak_mode)
        elif same_room:
            raise ValueError("same_room=True needs rirs= (a rir.RirBank made by from_rooms)")
        if room_schedule is not None and (rirs is None or getattr(rirs, "_ism", None) is None):
            raise ValueError("room_schedule needs rirs= a rir.RirBank made by from_rooms")
        self.room_schedule = room_schedule
        self.min_speakers = None if min_speakers is None else int(min_speakers)
        if self.min_speakers is not None:
            self._n_active = torch.zeros(self.B, dtype=torch.int32, device=dev)
        if self.loudness is not None:
            self._wl = torch.from_numpy(loudness_table(*self.loudness)).to(dev)
            self._plan_l10 = torch.zeros(self.B, self.C, dtype=torch.int32, device=dev)

    # Solver: loader.dataset.set_epoch(epoch).  A property, not an attribute: `self.dataset = self` is a reference cycle, and a
    # dropped loader's device buffers would then stay allocated until the cyclic collector happens to run
    dataset = property(lambda self: self)

    def __len__(self):
        return self.steps_per_epoch

    def set_epoch(self, epoch):
        """Select the epoch and rewind the step word (reshuffle=False: the epoch stays 0)."""
        self.epoch = int(epoch) if self.reshuffle else 0
        self._step.zero_()
        if self.room_schedule is not None and self.reshuffle:
            self._aug.rirs.refresh(self.room_schedule(self.epoch))

    def fill(self, mixture, sources, lengths=None):
        """The next minibatch into caller buffers (float32, contiguous, on the corpus' device): the plan launch and the gather on
        the current stream, no allocation, no host synchronisation; the step word advances on the device."""
        B, C, T = self.B, self.C, self.T
        for t, shape, name in ((mixture, (B, T), "mixture"), (sources, (B, C, T), "sources")):
            if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device:
                raise ValueError("%s must be a contiguous float32 %s tensor on %s" % (name, shape, self.device))
        c, aug = self.corpus, self._aug
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if aug is not None:
            aug.plan(self.seed, self.epoch, self.rank, self._step, stream)          # reads the step word, leaves it alone
        if self.min_speakers is not None:                                           # likewise
            lib.call("ctn_dynmix_plan_active", self.seed, self.epoch, self.rank, _ptr(self._step), B, C, self.min_speakers,
                     _ptr(self._n_active), stream)
        if self.speeds is not None:
            lib.call("ctn_dynmix_plan_speed", _ptr(self._spk_ptr), _ptr(self._utt_ids), len(self.tables["spk_ptr"]) - 1,
                     _ptr(c.lens), _ptr(c.inv_rms), _ptr(c.w), _ptr(self._pct), len(self.speeds), self.seed, self.epoch, self.rank,
                     _ptr(self._step), B, C, T, _ptr(self._plan_utt), _ptr(self._plan_start), _ptr(self._plan_q), _ptr(self._gain),
                     _ptr(self._plan_pct), stream)
        else:
            lib.call("ctn_dynmix_plan", _ptr(self._spk_ptr), _ptr(self._utt_ids), len(self.tables["spk_ptr"]) - 1, _ptr(c.lens),
                     _ptr(c.inv_rms), _ptr(c.w), self.seed, self.epoch, self.rank, _ptr(self._step), B, C, T,
                     _ptr(self._plan_utt), _ptr(self._plan_start), _ptr(self._plan_q), _ptr(self._gain), stream)
        if self.loudness is not None:                                               # behind the plan: it overwrites the plan's gains
            lib.call("ctn_dynmix_plan_loudness", _ptr(self._plan_utt), _ptr(c.inv_rms), c.num_utterances, _ptr(self._wl),
                     self._wl.numel(), self.loudness[0], self.seed, self.epoch, self.rank, _ptr(self._step), B, C,
                     _ptr(self._plan_l10), _ptr(self._gain), stream)
        if self.min_speakers is not None:
            lib.call("ctn_dynmix_mask_active", _ptr(self._n_active), B, C, _ptr(self._gain), stream)
        if aug is not None:                  # speed_segments -> reverb -> gather_aug (include/ctn_hip.h: the pipeline of one step)
            if self.speeds is not None:
                self._seg.segments(c, self._banks, self._plan_utt, self._plan_start, self._plan_pct, stream)
                rows = self._seg.rows()
            else:
                rows = _Rows(c.corpus, c.offsets, c.lens, c.num_utterances, self._plan_utt, self._plan_start)
            aug.mix(rows, self._gain, mixture, sources, self._peak, self._ws, stream)
        elif self.speeds is not None:
            self._seg.mix(c, self._banks, self._plan_utt, self._plan_start, self._plan_pct, self._gain, mixture, sources,
                          self._peak, self._ws, self.gather_mode, stream, self.peak_mode)
        else:
            _gather_call(c.corpus, c.offsets, c.lens, c.num_utterances, self._plan_utt, self._plan_start, self._gain, B, C, T, mixture,
                         sources, self._peak, self._ws, self.gather_mode, self.peak_mode, stream)
        if lengths is not None:
            lengths.copy_(self._lengths)

    def last_aug_plan(self):
        """Copies of the last minibatch's extra draws: (plan_rir [B,C] i32, noise_utt [B] i32, noise_start [B] i64, snr10 [B] i32
        in tenths of a dB, ngain [B] f32); the RIR element is None without rirs, the four noise elements without noise."""
        a = self._aug
        rir = a.plan_rir.clone() if a is not None and a.rirs is not None else None
        if a is None or a.noise is None:
            return rir, None, None, None, None
        return rir, a.noise_utt.clone(), a.noise_start.clone(), a.snr10.clone(), a.ngain.clone()

    def last_plan(self):
        """Copies of the last minibatch's plan: (plan_utt [B,C] i32, plan_start [B,C] i64, plan_q [B,C] i32, gain [B,C] f32),
        and with speeds the drawn percents plan_pct [B,C] i32 as a fifth element."""
        plan = self._plan_utt.clone(), self._plan_start.clone(), self._plan_q.clone(), self._gain.clone()
        return plan if self.speeds is None else plan + (self._plan_pct.clone(),)

    def last_loudness(self):
        """A copy of the last minibatch's drawn loudness plan_l10 [B,C] i32 in tenths of a LU (loudness_db only)."""
        if self.loudness is None:
            raise ValueError("this loader was built without loudness_db")
        return self._plan_l10.clone()

    def last_active(self):
        """A copy of the last minibatch's speaker counts n_active [B] i32 (min_speakers only)."""
        if self.min_speakers is None:
            raise ValueError("this loader was built without min_speakers: every mixture holds %d speakers" % self.C)
        return self._n_active.clone()

    def last_peak(self):
        """peak [B] of the last minibatch before the rescale to 0.9."""
        return self._peak.clone()

    def __iter__(self):
        self._step.zero_()
        for _ in range(self.steps_per_epoch):
            mixture = torch.empty(self.B, self.T, dtype=torch.float32, device=self.device)
            sources = torch.empty(self.B, self.C, self.T, dtype=torch.float32, device=self.device)
            self.fill(mixture, sources)
            yield mixture, self._lengths, sources


class _SegmentBuffer:
    """seg [B,C,T]: the unit-gain speed-perturbed segments of one minibatch, laid out as a corpus of B * C utterances of T
    samples for ctn_dynmix_gather (offsets = arange * T, lens = T, start = 0; seg_utt = arange, -1 for a flagged entry)."""

    def __init__(self, B, C, T, device):
        self.B, self.C, self.T = B, C, T
        self.seg = torch.zeros(B * C * T, dtype=torch.float32, device=device)
        self.seg_utt = torch.zeros(B, C, dtype=torch.int32, device=device)
        self.offsets = torch.arange(B * C, dtype=torch.int64, device=device) * T
        self.lens = torch.full((B * C,), T, dtype=torch.int64, device=device)
        self.start = torch.zeros(B, C, dtype=torch.int64, device=device)

    def rows(self):
        return _Rows(self.seg, self.offsets, self.lens, self.B * self.C, self.seg_utt, self.start)

    def segments(self, corpus, banks, plan_utt, plan_start, plan_pct, stream):
        B, C, T = self.B, self.C, self.T
        lib.call("ctn_dynmix_speed_segments", _ptr(corpus.corpus), _ptr(corpus.offsets), _ptr(corpus.lens), corpus.num_utterances,
                 _ptr(plan_utt), _ptr(plan_start), _ptr(plan_pct), B, C, T, _ptr(banks.banks), banks.banks.numel(), _ptr(banks.table),
                 banks.span_cap, banks.bank_cap, _ptr(self.seg), _ptr(self.seg_utt), stream)

    def mix(self, corpus, banks, plan_utt, plan_start, plan_pct, gain, mixture, sources, peak, ws, mode, stream, peak_mode=0):
        B, C, T = self.B, self.C, self.T
        self.segments(corpus, banks, plan_utt, plan_start, plan_pct, stream)
        _gather_call(self.seg, self.offsets, self.lens, B * C, self.seg_utt, self.start, gain, B, C, T, mixture, sources, peak, ws,
                     mode, peak_mode, stream)


def _gather_call(data, offsets, lens, U, utt, start, gain, B, C, T, mixture, sources, peak, ws, mode, peak_mode, stream):
    """ctn_dynmix_gather, or with another peak rule than "always" ctn_dynmix_gather_peak."""
    args = (_ptr(data), _ptr(offsets), _ptr(lens), U, _ptr(utt), _ptr(start), _ptr(gain), B, C, T, _ptr(mixture), _ptr(sources),
            _ptr(peak), _ptr(ws), ws.numel(), mode)
    if peak_mode == 0:
        lib.call("ctn_dynmix_gather", *args, stream)
    else:
        lib.call("ctn_dynmix_gather_peak", *args, peak_mode, stream)


class _Rows:
    """B * C rows in the "corpus + plan" form the gather and the reverberation read: row i is T samples of `data` from
    offsets[utt[i]] + start[i] on."""

    def __init__(self, data, offsets, lens, num_utterances, utt, start):
        self.data, self.offsets, self.lens, self.U, self.utt, self.start = data, offsets, lens, int(num_utterances), utt, start


class _Augment:
    """The buffers and launches of the noise and reverberation stages of one loader (all allocated here, none per step)."""

    def __init__(self, B, C, T, device, rirs, noise, snr_db, same_room=False, noise_loudness_db=None, peak_mode=0):
        self.B, self.C, self.T, self.rirs, self.noise, self.same_room = B, C, T, rirs, noise, same_room
        self.peak_mode = peak_mode
        if same_room:
            P = None if rirs is None else getattr(rirs, "positions_per_room", None)
            if P is None:
                raise ValueError("same_room=True needs a bank that records positions_per_room (rir.RirBank.from_rooms)")
            if not C <= P <= 64 or rirs.num_responses % P:
                raise ValueError("same_room=True: %d positions per room for mixtures of %d (C <= P <= 64), %d responses"
                                 % (P, C, rirs.num_responses))
        if rirs is not None:
            if rirs.device != device:
                raise ValueError("the RIR bank is on %s, the corpus on %s" % (rirs.device, device))
            self.plan_rir = torch.zeros(B, C, dtype=torch.int32, device=device)
            self.wet = _SegmentBuffer(B, C, T, device)                       # seg = wet rows, seg_utt = out_utt
            self.tgt = None if rirs.full_targets else torch.zeros(B * C * T, dtype=torch.float32, device=device)
        if noise is not None:
            if noise.device != device:
                raise ValueError("the noise corpus is on %s, the corpus on %s" % (noise.device, device))
            if noise.level != "rms" and not (noise.level == "loudness" and noise_loudness_db is not None):
                raise ValueError("a noise corpus keeps level='rms' (the active level is a speech measure), or has level='loudness' "
                                 "together with noise_loudness_db")
            if noise_loudness_db is not None:        # the word that chooses the SNR chooses the noise loudness: snr10 holds its tenths
                if noise.level != "loudness":
                    raise ValueError("noise_loudness_db needs noise= a corpus built with level='loudness'")
                self.lo10, self.hi10 = loudness_range(noise_loudness_db, "noise_loudness_db")
                wn = loudness_table(self.lo10, self.hi10)
            else:
                self.lo10, self.hi10 = snr_range(snr_db)
                wn = snr_table(self.lo10, self.hi10)
            self.noise_ids_host = noise_table(noise.lens_host, noise.level_power, T)
            self.noise_ids = torch.from_numpy(self.noise_ids_host).to(device)
            self.wn = torch.from_numpy(wn).to(device)
            self.noise_utt = torch.zeros(B, dtype=torch.int32, device=device)
            self.noise_start = torch.zeros(B, dtype=torch.int64, device=device)
            self.snr10 = torch.zeros(B, dtype=torch.int32, device=device)
            self.ngain = torch.zeros(B, dtype=torch.float32, device=device)

    @classmethod
    def of_plan(cls, B, C, T, device, rirs, plan_rir, noise, noise_utt, noise_start, ngain):
        """The stages over a caller-written plan: nothing is drawn, so no tables."""
        self = cls.__new__(cls)
        self.B, self.C, self.T, self.rirs, self.noise, self.same_room, self.peak_mode = B, C, T, rirs, noise, False, 0
        if rirs is not None:
            self.plan_rir = plan_rir.to(device=device, dtype=torch.int32).contiguous()
            self.wet = _SegmentBuffer(B, C, T, device)
            self.tgt = None if rirs.full_targets else torch.zeros(B * C * T, dtype=torch.float32, device=device)
        if noise is not None:
            self.noise_utt = noise_utt.to(device=device, dtype=torch.int32).contiguous()
            self.noise_start = noise_start.to(device=device, dtype=torch.int64).contiguous()
            self.ngain = ngain.to(device=device, dtype=torch.float32).contiguous()
        return self

    def plan(self, seed, epoch, rank, step, stream):
        r, n = self.rirs, self.noise
        if self.same_room:                   # the RIR half from ctn_dynmix_plan_rooms, the noise half (if any) from plan_aug alone
            P = r.positions_per_room
            lib.call("ctn_dynmix_plan_rooms", seed, epoch, rank, _ptr(step), self.B, self.C, r.num_responses // P, P,
                     _ptr(self.plan_rir), stream)
            if n is None:
                return
            r = None
        if n is None:
            lib.call("ctn_dynmix_plan_aug", seed, epoch, rank, _ptr(step), self.B, self.C, self.T, r.num_responses, _ptr(self.plan_rir),
                     0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, stream)
            return
        lib.call("ctn_dynmix_plan_aug", seed, epoch, rank, _ptr(step), self.B, self.C, self.T, r.num_responses if r is not None else 0,
                 _ptr(self.plan_rir) if r is not None else 0, _ptr(self.noise_ids), len(self.noise_ids_host), _ptr(n.lens),
                 n.num_utterances, _ptr(n.inv_rms), _ptr(self.wn), self.hi10 - self.lo10 + 1, self.lo10, _ptr(self.noise_utt),
                 _ptr(self.noise_start), _ptr(self.snr10), _ptr(self.ngain), stream)

    def mix(self, rows, gain, mixture, sources, peak, ws, stream):
        B, C, T, r, n = self.B, self.C, self.T, self.rirs, self.noise
        tgt = None
        if r is not None:
            tgt = self.tgt
            lib.call("ctn_dynmix_reverb", _ptr(rows.data), _ptr(rows.offsets), _ptr(rows.lens), rows.U, _ptr(rows.utt), _ptr(rows.start),
                     B * C, T, _ptr(r.bank), r.bank.numel(), _ptr(r.offsets), _ptr(r.lens), _ptr(r.direct), _ptr(r.early),
                     r.num_responses, _ptr(self.plan_rir), _ptr(self.wet.seg), _ptr(tgt), _ptr(self.wet.seg_utt), stream)
            rows = self.wet.rows()
        if n is None:
            noise_args = (0, 0, 0, 0, 0, 0, 0)
        else:
            noise_args = (_ptr(n.corpus), _ptr(n.offsets), _ptr(n.lens), n.num_utterances, _ptr(self.noise_utt), _ptr(self.noise_start),
                          _ptr(self.ngain))
        args = (_ptr(rows.data), _ptr(rows.offsets), _ptr(rows.lens), rows.U, _ptr(rows.utt), _ptr(rows.start), _ptr(gain), B, C, T,
                _ptr(tgt)) + noise_args + (_ptr(mixture), _ptr(sources), _ptr(peak), _ptr(ws), ws.numel())
        if self.peak_mode == 0:
            lib.call("ctn_dynmix_gather_aug", *args, stream)
        else:
            lib.call("ctn_dynmix_gather_aug_peak", *args, self.peak_mode, stream)


def gather_aug(corpus, plan_utt, plan_start, gain, segment_len, rirs=None, plan_rir=None, noise=None, noise_utt=None,
               noise_start=None, ngain=None, plan_pct=None, peak="always"):
    """The minibatch of a caller-written plan with reverberation and noise: gather()'s arguments, plus rirs (a rir.RirBank) with
    plan_rir [B,C] int32, and noise (a DeviceCorpus) with noise_utt [B] int32, noise_start [B] int64, ngain [B] float32 (the noise
    gain itself, nothing is drawn or looked up) -> (mixture [B,T], sources [B,C,T], peak [B]).  Either half may be left out.
    peak: "always" or "clip", the peak rule (DynamicMixLoader)."""
    dev = corpus.device
    B, C = plan_utt.shape
    T = int(segment_len)
    if (rirs is None) != (plan_rir is None):
        raise ValueError("rirs and plan_rir go together")
    if (noise is None) != (noise_utt is None) or (noise is None) != (noise_start is None) or (noise is None) != (ngain is None):
        raise ValueError("noise, noise_utt, noise_start and ngain go together")
    plan_utt = plan_utt.to(device=dev, dtype=torch.int32).contiguous()
    plan_start = plan_start.to(device=dev, dtype=torch.int64).contiguous()
    gain = gain.to(device=dev, dtype=torch.float32).contiguous()
    stream = torch.cuda.current_stream(dev).cuda_stream
    aug = _Augment.of_plan(B, C, T, dev, rirs, plan_rir, noise, noise_utt, noise_start, ngain)
    aug.peak_mode = peak_mode(peak)
    rows = _Rows(corpus.corpus, corpus.offsets, corpus.lens, corpus.num_utterances, plan_utt, plan_start)
    if plan_pct is not None:
        from . import resample as _rs
        pcts = sorted(set(int(p) for p in plan_pct.reshape(-1).tolist()))
        banks = _rs.speed_banks([p for p in pcts if _rs.PCT_LO <= p <= _rs.PCT_HI] or [100], dev)
        seg = _SegmentBuffer(B, C, T, dev)
        seg.segments(corpus, banks, plan_utt, plan_start, plan_pct.to(device=dev, dtype=torch.int32).contiguous(), stream)
        rows = seg.rows()
    mixture = torch.empty(B, T, dtype=torch.float32, device=dev)
    sources = torch.empty(B, C, T, dtype=torch.float32, device=dev)
    peak = torch.empty(B, dtype=torch.float32, device=dev)
    ws = torch.empty(max(1, lib.ctn_dynmix_gather_workspace(B, T)), dtype=torch.uint8, device=dev)
    aug.mix(rows, gain, mixture, sources, peak, ws, stream)
    return mixture, sources, peak


def gather(corpus, plan_utt, plan_start, gain, segment_len, mode=None, plan_pct=None, peak="always"):
    """The minibatch of a caller-written plan: plan_utt [B,C] int32, plan_start [B,C] int64, gain [B,C] float32 on the
    corpus' device -> (mixture [B,T], sources [B,C,T], peak [B]).  plan_pct [B,C] int32: speed percents in [50, 200], the
    sources replayed at these (plan_start + ceil(T * pct / 100) <= the utterance's length).  peak: "always" (every mixture is
    rescaled to a peak of 0.9) or "clip" (only one whose peak exceeds 0.9 is)."""
    dev = corpus.device
    B, C = plan_utt.shape
    T = int(segment_len)
    pm = peak_mode(peak)
    plan_utt = plan_utt.to(device=dev, dtype=torch.int32).contiguous()
    plan_start = plan_start.to(device=dev, dtype=torch.int64).contiguous()
    gain = gain.to(device=dev, dtype=torch.float32).contiguous()
    mixture = torch.empty(B, T, dtype=torch.float32, device=dev)
    sources = torch.empty(B, C, T, dtype=torch.float32, device=dev)
    peak = torch.empty(B, dtype=torch.float32, device=dev)
    ws = torch.empty(max(1, lib.ctn_dynmix_gather_workspace(B, T)), dtype=torch.uint8, device=dev)
    if plan_pct is not None:
        from . import resample as _rs
        pcts = sorted(set(int(p) for p in plan_pct.reshape(-1).tolist()))
        banks = _rs.speed_banks([p for p in pcts if _rs.PCT_LO <= p <= _rs.PCT_HI] or [100], dev)
        plan_pct = plan_pct.to(device=dev, dtype=torch.int32).contiguous()
        _SegmentBuffer(B, C, T, dev).mix(corpus, banks, plan_utt, plan_start, plan_pct, gain, mixture, sources, peak, ws,
                                         GATHER_MODE if mode is None else int(mode), torch.cuda.current_stream(dev).cuda_stream, pm)
        return mixture, sources, peak
    _gather_call(corpus.corpus, corpus.offsets, corpus.lens, corpus.num_utterances, plan_utt, plan_start, gain, B, C, T, mixture,
                 sources, peak, ws, GATHER_MODE if mode is None else int(mode), pm, torch.cuda.current_stream(dev).cuda_stream)
    return mixture, sources, peak
