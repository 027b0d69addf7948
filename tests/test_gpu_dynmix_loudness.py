"""GPU: the LibriMix recipe in the dynamic mixer -- DeviceCorpus(level="loudness"), DynamicMixLoader(loudness_db=,
noise_loudness_db=, peak=) -- against the numpy restatements (loudness_oracle.py for the corpus' levels, dynmix_loudness_oracle.py
for the draw, the gains and the peak rule, on top of the mixer's older oracles): gain, mixture, sources and peak BITWISE.

World: 8 utterances of 0.55 .. 1 s at 8 kHz over 4 speakers, 3 noise recordings; B = 3, C = 2, T = 4000."""
import numpy as np
import pytest
import torch

import dynmix_active_oracle as CO
import dynmix_loudness_oracle as XO
import dynmix_oracle as DO
import loudness_oracle as LO
import resample_oracle as RO

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import dynmix, loudness  # noqa: E402

DEV = "cuda:0"
FS, B, C, T = 8000, 3, 2, 4000
SEED, RANK = 0x5EED_0123_4567, 2
SPEEDS = tuple(range(95, 106))
LIBRI, NOISE_LIBRI = (-33, -25), (-38, -30)
ULP09 = float(np.nextafter(np.float32(0.9), np.float32(1.0)) - np.float32(0.9))


def _inv(arrays, ch):
    return dynmix.inverse_rms(np.array([LO.loudness(LO.stats(x, FS, ch))["power"] for x in arrays]))


@pytest.fixture(scope="module")
def world():
    rng = np.random.RandomState(8)
    arrays, speakers = [], []
    for u in range(8):
        n = int(rng.randint(4400, 8001))
        x = (rng.randn(n) * rng.uniform(0.02, 0.3)).astype(np.float32)
        arrays.append(x * (1.0 + 0.5 * np.sin(np.arange(n) / 700.0)).astype(np.float32))
        speakers.append("spk%d" % (u % 4))
    noise = [(rng.randn(n) * a).astype(np.float32) for n, a in ((4100, 0.05), (6000, 0.2), (5000, 0.01))]
    ch = int(loudness.lib.ctn_loudness_chunk())
    corpus = ctn.DeviceCorpus.from_arrays(arrays, speakers, DEV, level="loudness", sample_rate=FS)
    ncorpus = ctn.DeviceCorpus.from_arrays(noise, ["n"] * len(noise), DEV, level="loudness", sample_rate=FS)
    return dict(arrays=arrays, speakers=speakers, noise=noise, corpus=corpus, ncorpus=ncorpus, flat=np.concatenate(arrays),
                nflat=np.concatenate(noise), inv=_inv(arrays, ch), ninv=_inv(noise, ch))


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _assert_bitwise(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = int((_bits(got) != _bits(want)).sum())
    assert bad == 0, "%s: %d of %d values differ in their bits" % (what, bad, want.size)


def _loader(w, **kw):
    kw = dict(dict(num_speakers=C, steps_per_epoch=4, seed=SEED, rank=RANK), **kw)
    return ctn.DynamicMixLoader(w["corpus"], B, T, **kw)


def _fill(loader):
    mixture, sources = torch.empty(B, T, device=DEV), torch.empty(B, C, T, device=DEV)
    loader.fill(mixture, sources)
    return mixture, sources


def test_the_corpora_hold_the_oracles_levels(world):
    w = world
    _assert_bitwise(w["corpus"].inv_rms, w["inv"], "inv_rms")
    _assert_bitwise(w["ncorpus"].inv_rms, w["ninv"], "noise inv_rms")
    assert (w["inv"] > 0).all() and (w["ninv"] > 0).all() and w["corpus"].level == "loudness"


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("peak", ["always", "clip"])
def test_loudness_alone(world, mode, peak):
    w = world
    loader = _loader(w, loudness_db=LIBRI, peak=peak, gather_mode=mode)
    plain = ctn.DynamicMixLoader(ctn.DeviceCorpus.from_arrays(w["arrays"], w["speakers"], DEV), B, T, num_speakers=C, steps_per_epoch=4,
                                 seed=SEED, rank=RANK)
    tb = dict(loader.tables, inv_rms=w["inv"])
    wl = XO.loudness_table(-330, -250)
    _assert_bitwise(loader._wl, wl, "wl")
    seen = set()
    for epoch in (0, 3):
        loader.set_epoch(epoch)
        plain.set_epoch(epoch)
        for step in range(3):
            mixture, sources = _fill(loader)
            _fill(plain)
            utt, start, q, gain = loader.last_plan()
            w_utt, w_start, w_q, _ = DO.plan(SEED, RANK, epoch, step, B, C, T, tb)
            for got, want, other in zip((utt, start, q), (w_utt, w_start, w_q), plain.last_plan()[:3]):
                assert np.array_equal(got.cpu().numpy(), want) and torch.equal(got, other), (epoch, step)    # those draws keep their bits
            l10, w_gain = XO.plan_loudness(SEED, RANK, epoch, step, w_utt, w["inv"], wl, -330)
            assert np.array_equal(loader.last_loudness().cpu().numpy(), l10)
            _assert_bitwise(gain, w_gain, "gain, epoch %d step %d" % (epoch, step))
            seen.update(l10.reshape(-1).tolist())
            w_mix, w_src, w_peak = XO.mix(w["flat"], w["corpus"].offsets_host, w_utt, w_start, w_gain, T, peak)
            _assert_bitwise(loader.last_peak(), w_peak, "peak")
            _assert_bitwise(mixture, w_mix, "mixture, epoch %d step %d" % (epoch, step))
            _assert_bitwise(sources, w_src, "sources, epoch %d step %d" % (epoch, step))
    assert len(seen) >= 12 and min(seen) >= -330 and max(seen) <= -250                          # 36 draws over 81 tenths
    with pytest.raises(ValueError, match="loudness_db"):
        plain.last_loudness()


@pytest.mark.parametrize("peak", ["always", "clip"])
def test_with_a_noise_loudness(world, peak):
    w = world
    loader = _loader(w, loudness_db=LIBRI, noise=w["ncorpus"], noise_loudness_db=NOISE_LIBRI, peak=peak)
    snr = ctn.DynamicMixLoader(ctn.DeviceCorpus.from_arrays(w["arrays"], w["speakers"], DEV), B, T, num_speakers=C, steps_per_epoch=4,
                               seed=SEED, rank=RANK, noise=ctn.DeviceCorpus.from_arrays(w["noise"], ["n"] * 3, DEV), snr_db=(-6, 3))
    tb = dict(loader.tables, inv_rms=w["inv"])
    wl = XO.loudness_table(-330, -250)
    ids = dynmix.noise_table(w["ncorpus"].lens_host, w["ninv"], T)
    assert ids.tolist() == [0, 1, 2]
    for step in range(3):
        mixture, sources = _fill(loader)
        _fill(snr)
        w_utt, w_start, _, _ = DO.plan(SEED, RANK, 0, step, B, C, T, tb)
        _, w_gain = XO.plan_loudness(SEED, RANK, 0, step, w_utt, w["inv"], wl, -330)
        v, st, l10, ng = XO.noise_plan(SEED, RANK, 0, step, B, C, T, ids, w["ncorpus"].lens_host, w["ninv"], -380, -300)
        _, n_utt, n_start, n_l10, n_gain = loader.last_aug_plan()
        assert np.array_equal(n_utt.cpu().numpy(), v) and np.array_equal(n_start.cpu().numpy(), st) and np.array_equal(n_l10.cpu().numpy(), l10)
        other = snr.last_aug_plan()
        assert torch.equal(n_utt, other[1]) and torch.equal(n_start, other[2])                       # noise entry and start keep their bits
        assert l10.min() >= -380 and l10.max() <= -300
        _assert_bitwise(n_gain, ng, "ngain, step %d" % step)
        _assert_bitwise(loader.last_plan()[3], w_gain, "gain, step %d" % step)
        w_mix, w_src, w_peak = XO.mix(w["flat"], w["corpus"].offsets_host, w_utt, w_start, w_gain, T, peak, noise=w["nflat"],
                                      noise_offsets=w["ncorpus"].offsets_host, noise_utt=v, noise_start=st, ngain=ng)
        _assert_bitwise(loader.last_peak(), w_peak, "peak")
        _assert_bitwise(mixture, w_mix, "mixture, step %d" % step)
        _assert_bitwise(sources, w_src, "sources, step %d" % step)
        assert not np.array_equal(w_mix, XO.mix(w["flat"], w["corpus"].offsets_host, w_utt, w_start, w_gain, T, peak)[0])     # the noise is in
    rms_noise = ctn.DeviceCorpus.from_arrays(w["noise"], ["n"] * 3, DEV)
    with pytest.raises(ValueError, match="noise_loudness_db"):
        _loader(w, loudness_db=LIBRI, noise=rms_noise, noise_loudness_db=NOISE_LIBRI)
    with pytest.raises(ValueError, match="noise"):
        _loader(w, loudness_db=LIBRI, noise=w["ncorpus"])                                           # a loudness noise corpus at an SNR
    with pytest.raises(ValueError, match="level='loudness'"):
        ctn.DynamicMixLoader(rms_noise, B, T, loudness_db=LIBRI, rank=0)


@pytest.mark.parametrize("mode", [0, 1])
def test_with_speed_perturbation(world, mode):
    w = world
    loader = _loader(w, loudness_db=LIBRI, speeds=SPEEDS, peak="clip", gather_mode=mode)
    tb = dict(loader.tables, inv_rms=w["inv"])
    wl = XO.loudness_table(-330, -250)
    c = w["corpus"]
    for step in range(2):
        mixture, sources = _fill(loader)
        utt, start, q, gain, pct = loader.last_plan()
        w_utt, w_start, w_q, _, w_pct = RO.plan_speed(SEED, RANK, 0, step, B, C, T, tb, SPEEDS)
        for got, want in zip((utt, start, q, pct), (w_utt, w_start, w_q, w_pct)):
            assert np.array_equal(got.cpu().numpy(), want), step
        _, w_gain = XO.plan_loudness(SEED, RANK, 0, step, w_utt, w["inv"], wl, -330)
        _assert_bitwise(gain, w_gain, "gain, step %d" % step)
        seg = RO.speed_segments(w["flat"], c.offsets_host, c.lens_host, w_utt, w_start, w_pct, T)
        w_mix, w_src, w_peak = XO.mix_segments(seg, w_gain, "clip")
        _assert_bitwise(loader.last_peak(), w_peak, "peak")
        _assert_bitwise(mixture, w_mix, "mixture, step %d" % step)
        _assert_bitwise(sources, w_src, "sources, step %d" % step)
        assert (w_peak < 0.9).all()


def test_with_a_drawn_number_of_speakers(world):
    w = world
    loader = _loader(w, loudness_db=LIBRI, min_speakers=1, peak="clip")
    tb = dict(loader.tables, inv_rms=w["inv"])
    wl = XO.loudness_table(-330, -250)
    masked = 0
    for step in range(4):
        mixture, sources = _fill(loader)
        w_utt, w_start, _, _ = DO.plan(SEED, RANK, 0, step, B, C, T, tb)
        n = CO.counts(SEED, RANK, 0, step, B, C, 1)
        assert np.array_equal(loader.last_active().cpu().numpy(), n)
        w_gain = CO.masked(XO.plan_loudness(SEED, RANK, 0, step, w_utt, w["inv"], wl, -330)[1], n)       # the masking comes after
        masked += int((w_gain == 0).sum())
        _assert_bitwise(loader.last_plan()[3], w_gain, "gain, step %d" % step)
        w_mix, w_src, w_peak = XO.mix(w["flat"], w["corpus"].offsets_host, w_utt, w_start, w_gain, T, "clip")
        _assert_bitwise(loader.last_peak(), w_peak, "peak")
        _assert_bitwise(mixture, w_mix, "mixture, step %d" % step)
        _assert_bitwise(sources, w_src, "sources, step %d" % step)
    assert masked > 0


def test_the_peak_rule(world):
    w = world
    flat = torch.from_numpy(w["flat"]).to(DEV)
    offsets = torch.from_numpy(w["corpus"].offsets_host).to(DEV)
    idx = torch.arange(T, device=DEV)

    def run(loudness_db, peak):
        loader = _loader(w, loudness_db=loudness_db, peak=peak)
        mixture, sources = _fill(loader)
        utt, start, _, gain = loader.last_plan()
        seg = flat[(offsets[utt.long()] + start).unsqueeze(-1) + idx]                               # [B, C, T]
        top = torch.maximum(mixture.abs().amax(-1), sources.abs().amax((-2, -1)))
        return mixture, sources, gain.unsqueeze(-1) * seg, loader.last_peak(), top

    # LibriMix levels: no mixture comes near clipping, "clip" leaves everything as gains times samples, summed
    mixture, sources, raw, peak, top = run(LIBRI, "clip")
    assert float(peak.max()) < 0.9 and torch.equal(sources, raw) and torch.equal(mixture, raw[:, 0] + raw[:, 1])
    assert torch.equal(top, peak)
    # "always" rescales the same minibatch
    m2, s2, _, p2, top2 = run(LIBRI, "always")
    assert torch.equal(p2, peak) and not torch.equal(m2, mixture)
    assert all(abs(float(t) - float(np.float32(0.9))) <= ULP09 for t in top2)
    # at -3 LUFS every mixture would clip: both rules rescale, to the same bits, and last_peak() is the unscaled peak
    m3, s3, raw3, p3, top3 = run((-3, -3), "clip")
    m4, s4, _, p4, top4 = run((-3, -3), "always")
    assert float(p3.min()) > 0.9 and torch.equal(p3, p4) and torch.equal(m3, m4) and torch.equal(s3, s4)
    assert all(abs(float(t) - float(np.float32(0.9))) <= ULP09 for t in top3)
    assert torch.equal(p3, torch.maximum((raw3[:, 0] + raw3[:, 1]).abs().amax(-1), raw3.abs().amax((-2, -1))))
    # the caller-written plan takes the rule too
    loader = _loader(w, loudness_db=(-3, -3), peak="clip")
    mixture, sources = _fill(loader)
    utt, start, _, gain = loader.last_plan()
    for mode in (0, 1):
        g = dynmix.gather(w["corpus"], utt, start, gain, T, mode=mode, peak="clip")
        assert torch.equal(g[0], mixture) and torch.equal(g[1], sources) and torch.equal(g[2], loader.last_peak())
    quiet = dynmix.gather(w["corpus"], utt, start, gain * 0.01, T, peak="clip")
    assert float(quiet[2].max()) < 0.9 and torch.equal(quiet[0], quiet[1][:, 0] + quiet[1][:, 1])
    with pytest.raises(ValueError, match="peak"):
        dynmix.gather(w["corpus"], utt, start, gain, T, peak="never")


def test_the_defaults_give_the_bits_of_a_loader_without_the_arguments(world, monkeypatch):
    w = world
    kw = dict(num_speakers=C, steps_per_epoch=3, seed=SEED, rank=RANK)
    for extra in (dict(), dict(speeds=SPEEDS), dict(noise=ctn.DeviceCorpus.from_arrays(w["noise"], ["n"] * 3, DEV))):
        a = ctn.DynamicMixLoader(w["corpus"], B, T, loudness_db=None, noise_loudness_db=None, peak="always", **kw, **extra)
        b = ctn.DynamicMixLoader(w["corpus"], B, T, **kw, **extra)
        calls = []
        real = dynmix.lib.call
        monkeypatch.setattr(dynmix.lib, "call", lambda name, *args: (calls.append(name), real(name, *args))[1])
        out = []
        for loader in (a, b):
            calls.append("loader")
            out.append([(m.clone(), s.clone(), loader.last_peak()) + loader.last_plan() for m, _, s in loader])
        monkeypatch.undo()
        for x, y in zip(*out):
            assert all(torch.equal(p, q) for p, q in zip(x, y))
        half = len(calls) // 2
        assert half > 3 and calls[:half] == calls[half:], calls                                    # the same launches, and the old ones
        assert not [n for n in calls if n.endswith("_peak") or n == "ctn_dynmix_plan_loudness"], calls


def test_train_runs_with_the_recipe(world, tmp_path):
    from conv_tasnet_amd.train import train
    w = world
    spec = lambda seed, **kw: dict(arrays=w["arrays"], speakers=w["speakers"], batch_size=B, segment_len=T, steps_per_epoch=2, seed=seed,
                                   **kw)
    tiny = dict(N=64, L=20, B=32, H=64, P=3, X=2, R=2, C=2)
    solver = train(dict(tr_loader=spec(1), cv_loader=spec(2, reshuffle=False)), 1, "final.pth.tar", save_folder=str(tmp_path), config=tiny,
                   sample_rate=FS, level="loudness", loudness_db=LIBRI, peak="clip")
    assert solver.tr_loader.corpus.level == "loudness" and solver.tr_loader.loudness == (-330, -250) and solver.tr_loader.peak == "clip"
    assert float(solver.tr_loader.last_peak().max()) < 0.9
    got = list(solver.iter_losses)
    print("losses (two training steps, two validation steps):", got)
    assert len(got) == 4 and all(np.isfinite(got))
