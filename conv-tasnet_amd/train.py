"""train(): launcher mirroring src/train.py:14-102 (paper config, Adam lr 1e-3 or SGD, L2, clip 5, half-lr, early stop).

The reference's train() hard-codes librosa/json data loading; here the loaders are arguments (any iterables of
(padded_mixture [B,T], mixture_lengths [B], padded_source [B,C,T]) -- the AudioDataLoader contract) and a synthetic
loader is provided for smoke runs and benchmarks.  One process per GPU:

    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m conv_tasnet_amd.train --epochs 1
"""
import argparse

import torch

from . import parallel
from .conv_tasnet import ConvTasNet
from .optim import FlatAdam, FlatSGD
from .solver import Solver

PAPER = dict(N=256, L=20, B=256, H=512, P=3, X=8, R=4, C=2, norm_type='gLN', causal=0, mask_nonlinear='relu')


class SyntheticLoader:
    """Deterministic harmonic 2-speaker mixtures, sharded by rank; yields AudioDataLoader-style batches."""

    def __init__(self, n_batches, batch_size, samples=32000, C=2, sample_rate=8000, first_utt=0, rank=0, world=1):
        self.n_batches, self.batch_size, self.samples, self.C, self.sr = n_batches, batch_size, samples, C, sample_rate
        self.first, self.rank, self.world = first_utt, rank, world

    def __len__(self):
        return self.n_batches

    def _utt(self, u):
        import math
        g = torch.Generator().manual_seed(1234 + u)
        t = torch.arange(self.samples, dtype=torch.float64) / self.sr
        out = torch.empty(self.C, self.samples, dtype=torch.float64)
        for c in range(self.C):
            f0 = 80 + 320 * torch.rand(1, generator=g, dtype=torch.float64)
            ph = 2 * math.pi * torch.rand(3, generator=g, dtype=torch.float64)
            s = sum(a * torch.sin(2 * math.pi * (h + 1) * f0 * t + ph[h]) for h, a in enumerate((1.0, 0.5, 0.25)))
            out[c] = s + 0.01 * torch.randn(self.samples, generator=g, dtype=torch.float64)
        return out.float()

    def __iter__(self):
        per = self.batch_size
        for b in range(self.n_batches):
            base = self.first + (b * self.world + self.rank) * per
            src = torch.stack([self._utt(base + i) for i in range(per)])
            yield src.sum(1), torch.full((per,), self.samples, dtype=torch.long), src


def train(data, epochs, model_path, save_folder="exp/models", continue_from="", config=None, lr=1e-3,
          max_grad_norm=5, half_lr=1, early_stop=1, print_freq=10, enable_checkpoint=0, optimizer_type='adam',
          momentum=0.0, l2=0.0, loss='pit', snr_max=30.0, inactive_snr_max=20.0, stoi_weight=None, stoi_extended=False,
          sample_rate=8000, mrstft_weight=None, mrstft_resolutions=None, level=None, loudness_db=None, noise_loudness_db=None,
          peak=None):
    """data = {'tr_loader': ..., 'cv_loader': ...}.  Returns the Solver after training.

    Either loader may be given as a dict instead, the description of a dynamic-mixing loader that is built here on this rank's
    device: dict(arrays=, speakers=, batch_size=, segment_len=, noise_arrays=None, **DynamicMixLoader keywords), the corpus at
    sample_rate Hz.  level ('rms', 'active', 'loudness'), loudness_db, noise_loudness_db and peak ('always', 'clip') are passed
    through to such loaders (the corpora and DynamicMixLoader: the LibriMix recipe is level='loudness', loudness_db=(-33, -25),
    peak='clip'); with loaders that are built already they are a ValueError.

    loss 'pit': the reference's permutation-invariant SI-SNR against [B,C,T] sources.  loss 'mixit': mixture invariant
    training (mixit.cal_mixit_loss, soft threshold snr_max dB or None): both loaders yield the two reference mixtures
    [B,2,T] in place of the sources (mixit.MixtureOfMixtures) and config['C'] is the number of model outputs, 2 .. 8.
    loss 'varpit': PIT with inactive sources (varpit.cal_varpit_loss, soft thresholds snr_max and inactive_snr_max dB or None)
    for loaders whose mixtures hold 1 .. config['C'] speakers, the others' sources being zeros (DynamicMixLoader(min_speakers=)).
    loss 'pit_stoi': the PIT SI-SNR loss plus stoi_weight * (1 - mean STOI) (ESTOI with stoi_extended) under the same pairing
    (stoi.StoiPitCriterion), for any loader of [B,C,T] sources at sample_rate Hz; stoi_weight has no default.
    loss 'pit_assign': the 'pit' loss with the C! search replaced by an exact assignment solver on the device
    (assign.AssignPitCriterion), for config['C'] = 2 .. 16 speakers and any loader of [B,C,T] sources.
    loss 'pit_mrstft': the PIT SI-SNR loss plus mrstft_weight * the multi-resolution STFT loss (spectral convergence plus
    log-magnitude distance, mrstft.MrStftPitCriterion) under the same pairing, at mrstft_resolutions (triples (n_fft, hop,
    win_length); None: mrstft.DEFAULT_RESOLUTIONS), for any loader of [B,C,T] sources; mrstft_weight has no default.

    optimizer_type 'sgd' -> FlatSGD(lr, momentum, weight_decay=l2), 'adam' -> FlatAdam(lr, weight_decay=l2)
    (src/train.py:87-98); any other value prints 'Not support optimizer' and returns None, as the reference does."""
    if optimizer_type not in ('sgd', 'adam'):
        print("Not support optimizer")
        return None
    if loss not in ('pit', 'mixit', 'varpit', 'pit_stoi', 'pit_assign', 'pit_mrstft'):
        raise ValueError("loss must be 'pit' or 'mixit' or 'varpit' or 'pit_stoi' or 'pit_assign' or 'pit_mrstft', got %r" % (loss,))
    if (stoi_weight is not None or stoi_extended) and loss != 'pit_stoi':
        raise ValueError("stoi_weight and stoi_extended apply to loss 'pit_stoi' only")
    if (mrstft_weight is not None or mrstft_resolutions is not None) and loss != 'pit_mrstft':
        raise ValueError("mrstft_weight and mrstft_resolutions apply to loss 'pit_mrstft' only")
    criterion = None
    if loss == 'pit_mrstft':
        if mrstft_weight is None:
            raise ValueError("loss 'pit_mrstft' needs mrstft_weight: the weight of the spectral loss beside the SI-SNR loss in dB")
        from .mrstft import DEFAULT_RESOLUTIONS, MrStftPitCriterion
        criterion = MrStftPitCriterion(mrstft_weight, DEFAULT_RESOLUTIONS if mrstft_resolutions is None else mrstft_resolutions)
    if loss == 'pit_stoi':
        if stoi_weight is None:
            raise ValueError("loss 'pit_stoi' needs stoi_weight: the weight of (1 - mean score) beside the SI-SNR loss in dB")
        from .stoi import StoiPitCriterion
        criterion = StoiPitCriterion(sample_rate, stoi_weight, stoi_extended)
    if loss == 'mixit':
        from .mixit import MixItCriterion
        criterion = MixItCriterion(snr_max)
    if loss == 'varpit':
        from .varpit import VarPitCriterion
        criterion = VarPitCriterion(snr_max, inactive_snr_max)
    if loss == 'pit_assign':
        from .assign import AssignPitCriterion, MAX_SOURCES, MIN_SOURCES
        n_out = (PAPER if config is None else config)['C']
        if not MIN_SOURCES <= n_out <= MAX_SOURCES:
            raise ValueError("loss 'pit_assign' takes %d .. %d speakers, config['C'] = %r" % (MIN_SOURCES, MAX_SOURCES, n_out))
        criterion = AssignPitCriterion()
    recipe = dict(level=level, loudness_db=loudness_db, noise_loudness_db=noise_loudness_db, peak=peak)
    specs = [k for k in ('tr_loader', 'cv_loader') if isinstance(data.get(k), dict)]
    if not specs and any(v is not None for v in recipe.values()):
        raise ValueError("level, loudness_db, noise_loudness_db and peak apply to loaders given as a dict (built here); these are built")
    world, rank, device = parallel.init_distributed()
    if specs:
        data = dict(data)
        for k in specs:
            data[k] = _loader_from_spec(data[k], device, rank, sample_rate, recipe)
    cfg = dict(PAPER if config is None else config)
    torch.manual_seed(0)
    model = ConvTasNet(cfg['N'], cfg['L'], cfg['B'], cfg['H'], cfg['P'], cfg['X'], cfg['R'], cfg['C'],
                       norm_type=cfg.get('norm_type', 'gLN'), causal=cfg.get('causal', 0),
                       mask_nonlinear=cfg.get('mask_nonlinear', 'relu')).to(device)
    if optimizer_type == 'sgd':
        optimizer = FlatSGD(model.parameters(), lr=lr, momentum=momentum, weight_decay=l2)
    else:
        optimizer = FlatAdam(model.parameters(), lr=lr, weight_decay=l2)
    parallel.broadcast_parameters(optimizer.flat_params)
    arg_solver = (1, epochs, half_lr, early_stop, max_grad_norm, save_folder, enable_checkpoint, continue_from,
                  model_path, print_freq, 0, 0, "Conv-TasNet Training")
    solver = Solver(data, model, optimizer, arg_solver, criterion=criterion)
    solver.train()
    return solver


def _loader_from_spec(spec, device, rank, sample_rate, recipe):
    """The dynamic-mixing loader a dict describes (train()): the corpus (and the noise corpus of noise_arrays) at the recipe's level."""
    from .dynmix import DeviceCorpus, DynamicMixLoader
    spec = dict(spec)
    try:
        arrays, speakers = spec.pop("arrays"), spec.pop("speakers")
        batch_size, segment_len = spec.pop("batch_size"), spec.pop("segment_len")
    except KeyError as e:
        raise ValueError("a loader given as a dict needs arrays, speakers, batch_size and segment_len: %s is missing" % e)
    level = recipe["level"] or "rms"
    corpus = DeviceCorpus.from_arrays(arrays, speakers, device, level=level, sample_rate=sample_rate)
    noise_arrays = spec.pop("noise_arrays", None)
    if noise_arrays is not None:
        spec["noise"] = DeviceCorpus.from_arrays(noise_arrays, ["noise"] * len(noise_arrays), device, sample_rate=sample_rate,
                                                 level="loudness" if recipe["noise_loudness_db"] is not None else "rms")
    spec.setdefault("rank", rank)
    return DynamicMixLoader(corpus, batch_size, segment_len, loudness_db=recipe["loudness_db"],
                            noise_loudness_db=recipe["noise_loudness_db"], peak=recipe["peak"] or "always", **spec)


def build_parser():
    ap = argparse.ArgumentParser(description="Conv-TasNet training on MI355X (synthetic data demo)")
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--batches", type=int, default=10)
    ap.add_argument("--batch-size", type=int, default=8, help="utterances per GPU per step")
    ap.add_argument("--data-dir", default=None, help="directory with tr/ and cv/ sub-directories of {mix,s1,s2}.json "
                    "(the reference's manifest layout); default: synthetic mixtures")
    ap.add_argument("--model-path", default="final.pth.tar")
    ap.add_argument("--save-folder", default="exp/models")
    ap.add_argument("--optimizer", choices=("adam", "sgd"), default="adam")
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--momentum", type=float, default=0.0, help="SGD momentum")
    ap.add_argument("--l2", type=float, default=0.0, help="weight decay (coupled L2) of either optimiser")
    ap.add_argument("--dynamic-mix", default=None, metavar="TR_SOURCES_JSON", help="train on mixtures drawn on the device "
                    "every step from this single-speaker manifest (preprocess.preprocess_sources); replaces the training loader")
    ap.add_argument("--steps-per-epoch", type=int, default=1000, help="minibatches per epoch of the dynamic-mixing loaders")
    ap.add_argument("--dynamic-mix-cv", default=None, metavar="CV_SOURCES_JSON", help="validate on a fixed set of mixtures drawn "
                    "from this second manifest (the same minibatches every epoch); default: --data-dir's cv/")
    ap.add_argument("--cv-steps", type=int, default=100, help="minibatches of the --dynamic-mix-cv validation set")
    ap.add_argument("--seed", type=int, default=0, help="seed of the dynamic-mixing draw")
    ap.add_argument("--segment-len", type=int, default=32000, help="samples per segment of the dynamic-mixing loaders")
    ap.add_argument("--tiny", action="store_true", help="a tiny model (N=64 L=20 B=32 H=64 P=3 X=2 R=2) instead of the paper's: a "
                    "quick end-to-end check of a data path")
    ap.add_argument("--norm", choices=("gLN", "cLN", "cumLN", "BN"), default=None, help="norm of the TemporalBlocks (default: the "
                    "configuration's, gLN); cumLN: the paper's cumulative layer norm, with --causal")
    ap.add_argument("--causal", action="store_true", help="the causal model (left-padded depthwise convs)")
    ap.add_argument("--speed-perturb", default=None, metavar="LO:HI", help="--dynamic-mix only: replay every source at a drawn "
                    "integer percent of its speed in [LO, HI], e.g. 95:105 (resampled on the device); validation never perturbs")
    ap.add_argument("--corpus-rate", default="8000", choices=["8000", "auto"], help="rate of the --dynamic-mix files: 8000 (any "
                    "other rate is an error), or auto: files at other rates are resampled to 8 kHz on the device")
    ap.add_argument("--level", default="rms", choices=["rms", "active", "loudness"], help="--dynamic-mix / --dynamic-mix-cv: the 0-dB "
                    "level of a source: rms, the plain RMS of the whole utterance, active, the ITU-T P.56 active speech level the wsj0-2mix "
                    "recipe normalises with (tools/matlab-code/create_wav_2speakers.m:89-97, activlev(s, fs, 'n')), or loudness, the "
                    "ITU-R BS.1770 integrated loudness the LibriMix recipe normalises with, measured on the device; noise keeps rms "
                    "unless --noise-loudness is given")
    ap.add_argument("--loudness", default=None, metavar="LO:HI", help="--level loudness: every source at an absolute loudness drawn "
                    "uniformly from the tenths of a LU in [LO, HI] LUFS, e.g. --loudness=-33:-25 (in place of the relative +-q levels)")
    ap.add_argument("--noise-loudness", default=None, metavar="LO:HI", help="with --noise: the noise at an absolute loudness drawn "
                    "from [LO, HI] LUFS, e.g. --noise-loudness=-38:-30 (in place of --snr); the noise corpus is measured with the "
                    "loudness meter")
    ap.add_argument("--peak", default=None, choices=["always", "clip"], help="--dynamic-mix / --dynamic-mix-cv: always (the default) "
                    "rescales every mixture to a peak of 0.9, clip only a mixture whose peak exceeds 0.9")
    ap.add_argument("--librimix", action="store_true", help="the LibriMix recipe: short for --level loudness --loudness=-33:-25 "
                    "--peak clip, plus --noise-loudness=-38:-30 when --noise is given (--loudness, --noise-loudness and "
                    "--peak given beside it win)")
    ap.add_argument("--checkpoint", action="store_true", help="save checkpoint_models/epochN.pth.tar under --save-folder every epoch")
    ap.add_argument("--continue-from", default="", metavar="CHECKPOINT", help="resume from this checkpoint and run --epochs + 1 "
                    "more epochs (the Solver's arithmetic); a dynamic-mixing run sees the minibatches of the uninterrupted one")
    ap.add_argument("--noise", default=None, metavar="NOISE_JSON", help="--dynamic-mix only: add a segment of a noise recording "
                    "from this manifest (the --dynamic-mix layout; labels ignored) under every mixture, at a drawn SNR")
    ap.add_argument("--snr", default="-6:3", metavar="LO:HI", help="range of the drawn SNR in dB (tenths of a dB are drawn "
                    "uniformly), relative to a source at its 0-dB reference level; with --noise")
    ap.add_argument("--rirs", default=None, metavar="RIR_JSON | synthetic:N | rooms:G[:P]", help="--dynamic-mix only: convolve every "
                    "source with a room impulse response drawn from this manifest of [wav_path, n_samples] at 8 kHz, from N synthetic "
                    "ones, or from G shoebox rooms simulated on the device by the image-source method with P source positions each "
                    "(default P = 4); with P >= the number of speakers all talkers of a mixture sit in one room (same_room)")
    ap.add_argument("--rt60", default="0.2:0.6", metavar="LO:HI", help="--rirs rooms: the range in seconds of the reverberation "
                    "time the rooms' walls are designed for (Eyring); the simulated responses decay more slowly (DESIGN.md)")
    ap.add_argument("--rooms-refresh", action="store_true", help="--rirs rooms: draw and simulate new rooms at every epoch "
                    "(rir.draw_rooms(..., seed, epoch)); the validation loader keeps rooms of its own")
    ap.add_argument("--rir-early-ms", default="50", metavar="MS | full", help="the training targets keep the direct path and the "
                    "reflections of this many milliseconds behind it; full: the reverberant sources.  --noise, --snr, --rirs and "
                    "--rir-early-ms also reach the --dynamic-mix-cv loader (the same banks, reshuffle=False: a fixed validation set)")
    ap.add_argument("--loss", choices=("pit", "mixit", "varpit", "pit_stoi", "pit_assign", "pit_mrstft"), default="pit", help="pit: permutation-invariant SI-SNR against "
                    "the sources; mixit: mixture invariant training (needs --dynamic-mix and --dynamic-mix-cv): every minibatch is a "
                    "4-speaker mixture whose two 2-speaker halves are the only references the loss sees; varpit: PIT with inactive "
                    "sources for mixtures of --min-speakers .. --speakers talkers (needs --dynamic-mix and --dynamic-mix-cv); pit_stoi: the "
                    "pit loss plus --stoi-weight times (1 - mean STOI) under the same pairing, with any loader; pit_assign: the pit loss for "
                    "--speakers 2 .. 16 talkers, the pairing found by an exact assignment solver on the device instead of the C! "
                    "search (--data-dir with s1.json .. sC.json, or the synthetic loader); pit_mrstft: the pit loss plus "
                    "--mrstft-weight times the multi-resolution STFT loss under the same pairing, with any loader")
    ap.add_argument("--mrstft-weight", type=float, default=None, metavar="W", help="--loss pit_mrstft: the weight of the spectral "
                    "loss (spectral convergence + log-magnitude distance, of order 1) beside the SI-SNR loss in dB (required, no default)")
    ap.add_argument("--mrstft-resolutions", default=None, metavar="N_FFT:HOP:WIN,...", help="--loss pit_mrstft: up to 8 analysis "
                    "resolutions, n_fft a power of two in 64 .. 2048 (default 1024:120:600,2048:240:1200,512:50:240)")
    ap.add_argument("--stoi-weight", type=float, default=None, metavar="W", help="--loss pit_stoi: the weight of (1 - mean score) "
                    "beside the SI-SNR loss in dB (required, no default)")
    ap.add_argument("--stoi-extended", action="store_true", help="--loss pit_stoi: score with ESTOI instead of STOI")
    ap.add_argument("--mixit-outputs", type=int, default=4, metavar="M", help="--loss mixit: the number of model outputs, 2 .. 8")
    ap.add_argument("--snr-max", default="30", metavar="DB | none", help="--loss mixit / varpit: the soft threshold of the SNR loss "
                    "in dB")
    ap.add_argument("--min-speakers", type=int, default=None, metavar="M", help="--dynamic-mix only: every mixture holds a drawn "
                    "number of speakers in [M, --speakers]; the sources of the others are zeros.  Also reaches --dynamic-mix-cv")
    ap.add_argument("--speakers", type=int, default=None, metavar="C", help="--loss varpit: the number of model outputs and the "
                    "largest number of speakers in a mixture, 2 .. 4 (default 2); --loss pit_assign: the number of speakers, 2 .. 16 "
                    "(default 2)")
    ap.add_argument("--inactive-snr-max", default="20", metavar="DB | none", help="--loss varpit: the soft threshold in dB of the "
                    "loss of an output paired with a silent reference")
    return ap


def parse_snr(text):
    """'LO:HI' in dB -> (lo, hi) floats (train.py --snr; '=' joins a negative LO to the flag: --snr=-3:6)."""
    try:
        lo, hi = (float(v) for v in str(text).split(":"))
    except ValueError:
        raise ValueError("SNR range must be LO:HI in dB, got %r" % (text,))
    return lo, hi


LIBRIMIX = dict(loudness="-33:-25", noise_loudness="-38:-30", peak="clip")      # Cosentino et al. 2020, the LibriMix scripts


def recipe_args(a):
    """(level, loudness_db, noise_loudness_db, peak) of --level / --loudness / --noise-loudness / --peak / --librimix; the ranges
    as (lo, hi) floats or None.  What the flags cannot mean is a SystemExit."""
    level, loud, nloud, peak = a.level, a.loudness, a.noise_loudness, a.peak
    if a.librimix:
        level = "loudness"
        loud = LIBRIMIX["loudness"] if loud is None else loud
        peak = LIBRIMIX["peak"] if peak is None else peak
        if a.noise and nloud is None:
            nloud = LIBRIMIX["noise_loudness"]
    if loud is not None and level != "loudness":
        raise SystemExit("--loudness needs --level loudness")
    if nloud is not None and not a.noise:
        raise SystemExit("--noise-loudness needs --noise")
    try:
        loud = None if loud is None else parse_snr(loud)
        nloud = None if nloud is None else parse_snr(nloud)
    except ValueError:
        raise SystemExit("--loudness and --noise-loudness must be LO:HI in LUFS")
    return level, loud, nloud, "always" if peak is None else peak


def parse_rooms(text):
    """'rooms:G[:P]' -> (G, P), P = 4 by default (train.py --rirs)."""
    parts = str(text).split(":")
    try:
        if parts[0] != "rooms" or not 2 <= len(parts) <= 3:
            raise ValueError
        G, P = int(parts[1]), int(parts[2]) if len(parts) == 3 else 4
    except ValueError:
        raise ValueError("simulated rooms are rooms:G or rooms:G:P, got %r" % (text,))
    if G < 1 or not 1 <= P <= 64:
        raise ValueError("rooms:G:P needs G >= 1 and 1 <= P <= 64, got %r" % (text,))
    return G, P


def _augmentations(a, device, speakers=2):
    """(rirs, noise, snr_db, rooms) of --rirs / --noise / --snr / --rir-early-ms for the dynamic-mixing loaders; rooms: the extra
    loader arguments of --rirs rooms:G[:P] as (train kwargs, cv kwargs), two empty dicts otherwise."""
    from .dynmix import DeviceCorpus
    import numpy as np
    from . import rir as _rir
    rirs = noise = None
    rooms = ({}, {})
    if a.rirs:
        early = None if a.rir_early_ms == "full" else float(a.rir_early_ms)
        if a.rirs.startswith("rooms:"):
            G, P = parse_rooms(a.rirs)
            try:
                rt60 = parse_snr(a.rt60)                                    # the same LO:HI form
            except ValueError:
                raise SystemExit("--rt60 must be LO:HI in seconds, got %r" % (a.rt60,))
            draw = lambda seed, epoch=0: _rir.draw_rooms(G, P, 8000, rt60=rt60, seed=seed, epoch=epoch)
            rirs = _rir.RirBank.from_rooms(draw(a.seed), device, early_ms=early, n_taps=min(_rir.MAX_TAPS, int(np.ceil(rt60[1] * 8000))))
            same = P >= speakers
            rooms = (dict(same_room=same, room_schedule=(lambda e: draw(a.seed, e)) if a.rooms_refresh else None),
                     dict(same_room=same))
            if a.rooms_refresh:                      # the validation set keeps rooms of its own: the training bank is refilled in place
                rooms[1]["rirs"] = _rir.RirBank.from_rooms(draw(a.seed + 1), device, early_ms=early, n_taps=rirs._ism["n_taps"])
        elif a.rirs.startswith("synthetic:"):
            rirs = _rir.RirBank.from_arrays(_rir.synthetic_bank(int(a.rirs.split(":", 1)[1]), 8000, seed=a.seed), device, 8000, early)
        else:
            rirs = _rir.RirBank.from_manifest(a.rirs, 8000, device, early_ms=early)
    if a.noise:
        noise = DeviceCorpus.from_manifest(a.noise, 8000, device, resample=a.corpus_rate == "auto",
                                           level="loudness" if recipe_args(a)[2] is not None else "rms")
    return rirs, noise, parse_snr(a.snr), rooms


TINY = dict(N=64, L=20, B=32, H=64, P=3, X=2, R=2, C=2)


def main(argv=None):
    import os
    a = build_parser().parse_args(argv)
    if a.norm == "cumLN" and not a.causal:
        raise SystemExit("--norm cumLN needs --causal")
    if a.speed_perturb and not a.dynamic_mix:
        raise SystemExit("--speed-perturb applies to --dynamic-mix only")
    if (a.noise or a.rirs) and not a.dynamic_mix:
        raise SystemExit("--noise and --rirs apply to --dynamic-mix only")
    if a.rooms_refresh and not (a.rirs or "").startswith("rooms:"):
        raise SystemExit("--rooms-refresh applies to --rirs rooms:G[:P] only")
    if (a.loudness or a.noise_loudness or a.peak or a.librimix) and not (a.dynamic_mix or a.dynamic_mix_cv):
        raise SystemExit("--loudness, --noise-loudness, --peak and --librimix apply to --dynamic-mix / --dynamic-mix-cv only")
    level, loudness_db, noise_loudness_db, peak = recipe_args(a)
    mixit = a.loss == "mixit"
    if mixit:
        if not a.dynamic_mix:
            raise SystemExit("--loss mixit needs --dynamic-mix: its minibatches are 4-speaker mixtures drawn on the device")
        if not a.dynamic_mix_cv:
            raise SystemExit("--loss mixit needs --dynamic-mix-cv: every other validation set would be scored with the PIT "
                             "criterion against isolated sources, which is not the loss being trained")
        if not 2 <= a.mixit_outputs <= 8:
            raise SystemExit("--mixit-outputs must be 2 .. 8")
    if (a.stoi_weight is not None or a.stoi_extended) and a.loss != "pit_stoi":
        raise SystemExit("--stoi-weight and --stoi-extended apply to --loss pit_stoi only")
    if a.loss == "pit_stoi" and (a.stoi_weight is None or not a.stoi_weight >= 0):
        raise SystemExit("--loss pit_stoi needs --stoi-weight W with W >= 0")
    if (a.mrstft_weight is not None or a.mrstft_resolutions is not None) and a.loss != "pit_mrstft":
        raise SystemExit("--mrstft-weight and --mrstft-resolutions apply to --loss pit_mrstft only")
    if a.loss == "pit_mrstft" and (a.mrstft_weight is None or not a.mrstft_weight >= 0):
        raise SystemExit("--loss pit_mrstft needs --mrstft-weight W with W >= 0")
    mrstft_res = None
    if a.mrstft_resolutions is not None:
        from .mrstft import parse_resolutions
        try:
            mrstft_res = parse_resolutions(a.mrstft_resolutions)
        except ValueError as e:
            raise SystemExit("--mrstft-resolutions: %s" % e)
    varpit = a.loss == "varpit"
    if a.min_speakers is not None and not a.dynamic_mix:
        raise SystemExit("--min-speakers applies to --dynamic-mix only")
    assign = a.loss == "pit_assign"
    if a.speakers is not None and not (varpit or assign):
        raise SystemExit("--speakers applies to --loss varpit only (and to --loss pit_assign)")
    speakers = 4 if mixit else 2
    if assign:
        speakers = 2 if a.speakers is None else a.speakers
        if not 2 <= speakers <= 16:
            raise SystemExit("--loss pit_assign: --speakers must be 2 .. 16")
        if (a.dynamic_mix or a.dynamic_mix_cv) and speakers > 4:
            raise SystemExit("--loss pit_assign with --dynamic-mix takes --speakers 2 .. 4: the dynamic mixer plans at most 4 sources "
                             "per mixture; train %d speakers from --data-dir (s1.json .. s%d.json)" % (speakers, speakers))
    if varpit:
        if not a.dynamic_mix or not a.dynamic_mix_cv:
            raise SystemExit("--loss varpit needs --dynamic-mix and --dynamic-mix-cv: mixtures with silent sources are drawn on "
                             "the device, and every other validation set would be scored with the PIT criterion")
        speakers = 2 if a.speakers is None else a.speakers
        if not 2 <= speakers <= 4:
            raise SystemExit("--speakers must be 2 .. 4")
    if a.min_speakers is not None and not 1 <= a.min_speakers <= speakers:
        raise SystemExit("--min-speakers must be 1 .. %d" % speakers)
    world, rank, device = parallel.init_distributed()
    tr = cv = None
    if a.dynamic_mix or a.dynamic_mix_cv:
        from .dynmix import DeviceCorpus, DynamicMixLoader
        auto = a.corpus_rate == "auto"
        rirs, noise, snr_db, rooms = _augmentations(a, device, speakers) if a.dynamic_mix else (None, None, (-6, 3), ({}, {}))
        if a.dynamic_mix:
            speeds = None
            if a.speed_perturb:
                from .resample import parse_speed_range
                speeds = parse_speed_range(a.speed_perturb)
            tr = DynamicMixLoader(DeviceCorpus.from_manifest(a.dynamic_mix, 8000, device, resample=auto, level=level), a.batch_size,
                                  a.segment_len, num_speakers=speakers, steps_per_epoch=a.steps_per_epoch, seed=a.seed, rank=rank,
                                  speeds=speeds, rirs=rirs, noise=noise, snr_db=snr_db, min_speakers=a.min_speakers,
                                  loudness_db=loudness_db, noise_loudness_db=noise_loudness_db, peak=peak, **rooms[0])
        if a.dynamic_mix_cv:
            cv = DynamicMixLoader(DeviceCorpus.from_manifest(a.dynamic_mix_cv, 8000, device, resample=auto, level=level), a.batch_size,
                                  a.segment_len, num_speakers=speakers, steps_per_epoch=a.cv_steps, seed=a.seed + 1, rank=rank,
                                  reshuffle=False, noise=noise, snr_db=snr_db, loudness_db=loudness_db,
                                  noise_loudness_db=noise_loudness_db if noise is not None else None, peak=peak,
                                  min_speakers=a.min_speakers if a.dynamic_mix else None, **dict(dict(rirs=rirs), **rooms[1]))
        if mixit:
            from .mixit import MixtureOfMixtures
            tr, cv = MixtureOfMixtures(tr), MixtureOfMixtures(cv)
    n_src, n_syn = (dict(num_speakers=speakers), dict(C=speakers)) if assign else ({}, {})    # (every other loss: the loaders' defaults)
    if a.data_dir:
        from .data import AudioDataLoader, AudioDataset
        if tr is None:
            tr = AudioDataLoader(AudioDataset(os.path.join(a.data_dir, "tr"), a.batch_size, segment=4.0, rank=rank, world=world,
                                              **n_src), shuffle=True, num_workers=4)
        if cv is None:
            cv = AudioDataLoader(AudioDataset(os.path.join(a.data_dir, "cv"), 1, segment=-1, cv_maxlen=6, rank=rank, world=world,
                                              **n_src), num_workers=0)
    if tr is None:
        tr = SyntheticLoader(a.batches, a.batch_size, rank=rank, world=world, **n_syn)
    if cv is None:
        cv = SyntheticLoader(1, a.batch_size, first_utt=10 ** 6, rank=rank, world=world, **n_syn)
    config = TINY if a.tiny else None
    extra = {}
    if mixit:
        config = dict(TINY if a.tiny else PAPER, C=a.mixit_outputs)
        extra = dict(loss="mixit", snr_max=None if a.snr_max.lower() == "none" else float(a.snr_max))
    if varpit:
        config = dict(TINY if a.tiny else PAPER, C=speakers)
        extra = dict(loss="varpit", snr_max=None if a.snr_max.lower() == "none" else float(a.snr_max),
                     inactive_snr_max=None if a.inactive_snr_max.lower() == "none" else float(a.inactive_snr_max))
    if a.loss == "pit_stoi":
        extra = dict(loss="pit_stoi", stoi_weight=a.stoi_weight, stoi_extended=a.stoi_extended)
    if a.loss == "pit_mrstft":
        extra = dict(loss="pit_mrstft", mrstft_weight=a.mrstft_weight, mrstft_resolutions=mrstft_res)
    if assign:
        config = dict(TINY if a.tiny else PAPER, C=speakers)
        extra = dict(loss="pit_assign")
    if a.norm is not None or a.causal:          # (untouched otherwise: the configurations above as they are)
        config = dict(config if config is not None else PAPER)
        if a.norm is not None:
            config['norm_type'] = a.norm
        if a.causal:
            config['causal'] = 1
    return train({'tr_loader': tr, 'cv_loader': cv}, a.epochs, a.model_path, save_folder=a.save_folder, lr=a.lr,
                 optimizer_type=a.optimizer, momentum=a.momentum, l2=a.l2, config=config,
                 enable_checkpoint=int(a.checkpoint), continue_from=a.continue_from, **extra)


if __name__ == "__main__":
    main()
