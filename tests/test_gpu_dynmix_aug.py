"""GPU: noisy and reverberant dynamic mixing (ctn_dynmix_plan_aug, ctn_dynmix_reverb, ctn_dynmix_gather_aug) against the host
restatement in dynmix_aug_oracle.py -- the reverberation kernel alone BITWISE on hand-written plans, flagged rows, the sampler's
extra draws equal and its minibatches bitwise, the composition with speed perturbation, the identities that tie the new path
to the old one, graph replay, and train.py end to end with a resumed run.

World: the small random corpus of test_gpu_dynmix_speed.py (samples below 2^-15 zeroed), six noise files of which one is
shorter than the segment and one is silent, RIR taps that are 0 or at least 2^-20 in magnitude: no product is subnormal."""
import json

import numpy as np
import pytest
import torch

import dynmix_aug_oracle as AO
import dynmix_oracle as DO
import resample_oracle as RO

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import dynmix, rir  # noqa: E402

DEV = "cuda:0"
SR = 8000
SPEEDS = tuple(range(95, 106))
SNR_DB = (-3, 6)


def _arrays(seed=11, n_utt=60, n_spk=12):
    """About 60 utterances of 1 .. 12 s at 8 kHz over 12 speakers (the world of test_gpu_dynmix_speed.py)."""
    rng = np.random.RandomState(seed)
    arrays, speakers = [], []
    for u in range(n_utt):
        n = int(rng.randint(1 * SR, 12 * SR + 1))
        if u < 4:
            n = int(rng.randint(6 * SR, 12 * SR))             # the utterances of the hand-written plans are long
        x = (rng.randn(n) * rng.uniform(0.01, 0.3)).astype(np.float32)
        x *= (1.0 + 0.5 * np.sin(np.arange(n) / 900.0)).astype(np.float32)
        x[np.abs(x) < 2.0 ** -15] = 0.0
        arrays.append(x)
        speakers.append("spk%02d" % (u % n_spk))
    arrays[7][:] = 0.0                                        # a silent utterance: never eligible
    return arrays, speakers


def _noise_arrays():
    rng = np.random.RandomState(23)
    out = []
    for n in (9000, 3000, 12000, 8000, 20000, 5000):          # 3000 is shorter than every sampler segment
        x = (rng.randn(n) * rng.uniform(0.02, 0.2)).astype(np.float32)
        x[np.abs(x) < 2.0 ** -15] = 0.0
        out.append(x)
    out[3][:] = 0.0                                           # silent
    return out


def _clean_taps(h):
    """float64 taps -> float32 taps that are 0 or at least 2^-20 in magnitude."""
    h = np.asarray(h, dtype=np.float64).astype(np.float32)
    h[np.abs(h) < 2.0 ** -20] = 0.0
    return h


def _bank_arrays():
    """Six short synthetic responses (240 .. 960 taps), normalised here in float64 so that the small taps can be zeroed after it."""
    return [_clean_taps(h / np.sqrt(np.sum(h * h))) for h in rir.synthetic_bank(6, SR, rt60=(0.03, 0.12), seed=2)]


@pytest.fixture(scope="module")
def world():
    arrays, speakers = _arrays()
    corpus = ctn.DeviceCorpus.from_arrays(arrays, speakers, DEV)
    noise_arrays = _noise_arrays()
    noise = ctn.DeviceCorpus.from_arrays(noise_arrays, ["n"] * len(noise_arrays), DEV)
    bank = ctn.RirBank.from_arrays(_bank_arrays(), DEV, SR, early_ms=10.0, normalize=False)
    return dict(arrays=arrays, speakers=speakers, corpus=corpus, flat=np.concatenate(arrays), noise=noise,
                noise_flat=np.concatenate(noise_arrays), bank=bank)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _assert_bitwise(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = int((_bits(got) != _bits(want)).sum())
    assert bad == 0, "%s: %d of %d values differ in their bits" % (what, bad, want.size)


def _noise_tables(w, T, snr_db=SNR_DB):
    lo10, hi10 = dynmix.snr_range(snr_db)
    n = w["noise"]
    return dict(noise_ids=dynmix.noise_table(n.lens_host, n.meansq, T), lens=n.lens_host, inv_rms=dynmix.inverse_rms(n.meansq),
                wn=AO.snr_table(lo10, hi10), lo10=lo10)


# ---- 1. the reverberation kernel alone ------------------------------------------------------------------------------------
def _tables(lens, direct, early, seed):
    rng = np.random.RandomState(seed)
    taps = []
    for n in lens:
        h = rng.randn(n) * np.exp(-np.arange(n) / (0.3 * n + 2.0)) * rng.choice([1.0, 1.0, 0.0], size=n)   # exact zeros among them
        taps.append(_clean_taps(h))
    offsets = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64)
    return dict(bank=np.concatenate(taps), offsets=offsets, lens=np.array(lens, np.int32), direct=np.array(direct, np.int32),
                early=np.array(early, np.int32))


# lengths the issue names; direct cycles through {0, middle, n - 1}, early through {d + 1, between, n}
TABLES_A = dict(lens=[1, 2, 255, 256, 257, 1000, 8192], direct=[0, 1, 127, 0, 128, 999, 4096], early=[1, 2, 200, 1, 257, 1000, 6000])
# the kernel's own edges: 4 taps per unrolled group, 1024 taps per staged chunk, `early` on either side of a chunk edge
TABLES_B = dict(lens=[3, 4, 5, 1023, 1024, 1025, 2049], direct=[2, 0, 4, 511, 1023, 0, 1000], early=[3, 2, 5, 1020, 1024, 1024, 1025])


def _run_reverb(w, utt, start, T, tb, plan_rir, with_tgt=True, bank_floats=None):
    c = w["corpus"]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    N = len(utt)
    d = {k: dev(v) for k, v in tb.items()}
    p_utt, p_start, p_rir = dev(np.asarray(utt, np.int32)), dev(np.asarray(start, np.int64)), dev(np.asarray(plan_rir, np.int32))
    wet = torch.full((N, T), 7.0, device=DEV)
    tgt = torch.full((N, T), 7.0, device=DEV) if with_tgt else None
    out_utt = torch.full((N,), 99, dtype=torch.int32, device=DEV)
    ctn.lib.call("ctn_dynmix_reverb", c.corpus.data_ptr(), c.offsets.data_ptr(), c.lens.data_ptr(), c.num_utterances, p_utt.data_ptr(),
                 p_start.data_ptr(), N, T, d["bank"].data_ptr(), d["bank"].numel() if bank_floats is None else bank_floats,
                 d["offsets"].data_ptr(), d["lens"].data_ptr(), d["direct"].data_ptr(), d["early"].data_ptr(), len(tb["lens"]),
                 p_rir.data_ptr(), wet.data_ptr(), tgt.data_ptr() if with_tgt else 0, out_utt.data_ptr(),
                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return wet.cpu().numpy(), tgt.cpu().numpy() if with_tgt else None, out_utt.cpu().numpy()


def _hand_rows(w, T):
    """Seven rows over the long utterances 0 .. 3 and the corpus' last one: starts 0, len - T and in between."""
    n = [int(v) for v in w["corpus"].lens_host]
    last = len(n) - 1
    assert n[last] >= T
    utt = [0, 1, 2, 3, last, 1, 2]
    start = [0, n[1] - T, 17, 4001, n[last] - T, 1, n[2] - T - 1]
    return utt, start


@pytest.mark.parametrize("T,tables", [(700, "A"), (4099, "A"), (700, "B"), (4099, "B"), (1024, "B"), (1025, "B")])
def test_reverb_of_hand_written_plans_is_bitwise_the_oracle(world, T, tables):
    """N = 7 rows, T = 700 (shorter than the longest responses) and 4099 (five output tiles, the last of 3 samples, no multiple
    of 4), responses of 1, 2, 255, 256, 257, 1000 and 8192 taps.  The kernel's own edges (set B): 3, 4, 5 taps around its group of
    4, 1023, 1024, 1025 and 2049 taps around its staged chunk of 1024 with `early` at 1020, 1024 and 1025, and T = 1024 and 1025
    around its output tile of 1024."""
    spec = TABLES_A if tables == "A" else TABLES_B
    tb = _tables(spec["lens"], spec["direct"], spec["early"], seed=T)
    utt, start = _hand_rows(world, T)
    plan_rir = [(i * 3) % 7 for i in range(7)]                                  # every response once
    want_wet, want_tgt = AO.reverb_rows(world["flat"], world["corpus"].offsets_host, utt, start, T, tb, plan_rir)
    wet, tgt, out_utt = _run_reverb(world, utt, start, T, tb, plan_rir)
    assert list(out_utt) == list(range(7))
    _assert_bitwise(wet, want_wet, "wet")
    _assert_bitwise(tgt, want_tgt, "tgt")
    assert np.abs(want_wet).max() > 0 and not np.array_equal(want_wet, want_tgt)
    full = [i for i in range(7) if tb["early"][plan_rir[i]] == tb["lens"][plan_rir[i]]]
    assert full and all(np.array_equal(_bits(wet[i]), _bits(tgt[i])) for i in full)
    wet_only, _, _ = _run_reverb(world, utt, start, T, tb, plan_rir, with_tgt=False)      # a null tgt: one pass over the taps
    _assert_bitwise(wet_only, want_wet, "wet without tgt")


# ---- 2. flagged rows --------------------------------------------------------------------------------------------------------
def test_flagged_rows_are_zeros_and_leave_their_neighbours_alone(world):
    """Not a fault test: the kernel checks every plan entry and table row before it forms an address."""
    T = 700
    c = world["corpus"]
    tb = _tables([5, 300, 40], [0, 10, 39], [3, 300, 40], seed=1)
    n1 = int(c.lens_host[1])
    utt = [1, c.num_utterances, -1, 1, 1, 2, 2, 3, 2]
    start = [5, 0, 0, -1, n1 - T + 1, 9, 9, 0, 30]
    plan_rir = [1, 0, 0, 0, 0, -1, 3, 2, 0]
    good = [0, 7, 8]
    wet, tgt, out_utt = _run_reverb(world, utt, start, T, tb, plan_rir)
    assert list(out_utt) == [i if i in good else -1 for i in range(9)]
    w_wet, w_tgt = AO.reverb_rows(world["flat"], c.offsets_host, [utt[i] for i in good], [start[i] for i in good], T, tb,
                                  [plan_rir[i] for i in good])
    for k, i in enumerate(good):
        _assert_bitwise(wet[i], w_wet[k], "wet row %d" % i)
        _assert_bitwise(tgt[i], w_tgt[k], "tgt row %d" % i)
    for i in set(range(9)) - set(good):
        assert not wet[i].any() and not tgt[i].any(), i
    # a response whose table entry leaves the bank buffer: rows that drew it are flagged, the others are not touched by it
    wet2, tgt2, out2 = _run_reverb(world, utt, start, T, tb, plan_rir, bank_floats=len(tb["bank"]) - 1)
    assert list(out2) == [0, -1, -1, -1, -1, -1, -1, -1, 8] and not wet2[7].any() and not tgt2[7].any()
    _assert_bitwise(wet2[0], w_wet[0], "wet row 0")
    _assert_bitwise(wet2[8], w_wet[2], "wet row 8")
    # after the mix: peak = -1 for the mixture of a flagged row, the other mixtures bitwise the oracle
    bank = ctn.RirBank.from_arrays([tb["bank"][o:o + n] for o, n in zip(tb["offsets"], tb["lens"])], DEV, SR, early_ms=None, normalize=False)
    g_utt = np.array([[1, 2], [3, 2], [1, c.num_utterances], [2, 3], [3, 1]], np.int32)
    g_start = np.array([[5, 30], [0, 9], [5, 0], [9, 0], [0, n1 - T + 1]], np.int64)
    g_rir = np.array([[1, 0], [2, 1], [1, 0], [3, 2], [-1, 0]], np.int32)
    gain = np.random.RandomState(0).uniform(0.5, 8.0, size=g_utt.shape).astype(np.float32)
    nz = _noise_tables(world, T)
    n_utt, n_start = np.array([0, 2, 4, 0, 5], np.int32), np.array([0, 11000, 3, 8000, 100], np.int64)
    ngain = np.array([0.5, 2.0, 1.0, 1.0, 1.0], np.float32)
    mixture, sources, peak = dynmix.gather_aug(c, torch.from_numpy(g_utt), torch.from_numpy(g_start), torch.from_numpy(gain), T, rirs=bank,
                                               plan_rir=torch.from_numpy(g_rir), noise=world["noise"], noise_utt=torch.from_numpy(n_utt),
                                               noise_start=torch.from_numpy(n_start), ngain=torch.from_numpy(ngain))
    peak, sources = peak.cpu().numpy(), sources.cpu().numpy()
    assert peak[0] > 0 and peak[1] > 0 and list(peak[2:]) == [-1.0] * 3
    assert not sources[2, 1].any() and sources[2, 0].any() and not sources[3, 0].any() and not sources[4].any()
    ok = [0, 1]
    assert bank.full_targets
    w_wet, _ = AO.reverb_rows(world["flat"], c.offsets_host, g_utt[ok], g_start[ok], T, bank.host, g_rir[ok])
    w_mix, w_src, w_peak = AO.mix_rows(w_wet, None, gain[ok], noise=world["noise_flat"], noise_offsets=world["noise"].offsets_host,
                                       noise_utt=n_utt[ok], noise_start=n_start[ok], ngain=ngain[ok])
    _assert_bitwise(peak[ok], w_peak, "peak")
    _assert_bitwise(mixture.cpu().numpy()[ok], w_mix, "mixture")
    _assert_bitwise(sources[ok], w_src, "sources")
    # a noise entry outside its utterance: silence under the mixture, peak = -1
    n_bad = np.array([1, 6, -1, 0, 0], np.int32)                                  # utterance 1 holds 3000 < T + 2500 samples
    s_bad = np.array([2500, 0, 0, -1, 9000 - T + 1], np.int64)
    _, _, peak = dynmix.gather_aug(c, torch.from_numpy(g_utt[:2].repeat(3, 0)[:5]), torch.from_numpy(g_start[:2].repeat(3, 0)[:5]),
                                   torch.from_numpy(gain), T, noise=world["noise"], noise_utt=torch.from_numpy(n_bad),
                                   noise_start=torch.from_numpy(s_bad), ngain=torch.from_numpy(ngain))
    assert list(peak.cpu().numpy()) == [-1.0] * 5


# ---- 3. the sampler ---------------------------------------------------------------------------------------------------------
def _oracle_step(w, tb, nz, seed, rank, epoch, step, B, C, T, speeds=None, rirs=True, noise=True):
    """The oracle chain of one step -> (plan, aug plan, (mixture, sources, peak))."""
    c, bank = w["corpus"], w["bank"].host
    if speeds is None:
        plan = DO.plan(seed, rank, epoch, step, B, C, T, tb)
        rows = (w["flat"], c.offsets_host, plan[0], plan[1])
    else:
        plan = RO.plan_speed(seed, rank, epoch, step, B, C, T, tb, speeds)
        seg = RO.speed_segments(w["flat"], c.offsets_host, c.lens_host, plan[0], plan[1], plan[4], T)
        rows = (seg.reshape(-1), np.arange(B * C, dtype=np.int64) * T, np.arange(B * C, dtype=np.int32).reshape(B, C), np.zeros((B, C), np.int64))
    aug = AO.plan_aug(seed, rank, epoch, step, B, C, T, R=len(bank["lens"]) if rirs else None, noise=nz if noise else None)
    kw = {}
    if noise:
        kw = dict(noise=w["noise_flat"], noise_offsets=w["noise"].offsets_host, noise_utt=aug[1], noise_start=aug[2], ngain=aug[4])
    if rirs:
        wet, tgt = AO.reverb_rows(rows[0], rows[1], rows[2], rows[3], T, bank, aug[0])
        return plan, aug, AO.mix_rows(wet, tgt, plan[3], **kw)
    return plan, aug, AO.mix_aug(rows[0], rows[1], rows[2], rows[3], plan[3], T, **kw)


def _assert_plans(loader, plan, aug, what):
    got = loader.last_plan()
    for g, want, name in zip(got, plan, ("utt", "start", "q", "gain", "pct")):
        if name == "gain":
            _assert_bitwise(g, want, "gain, " + what)
        else:
            assert torch.equal(g.cpu(), torch.from_numpy(want)), (name, what)
    got = loader.last_aug_plan()
    assert len(got) == 5
    for g, want, name in zip(got, aug, ("plan_rir", "noise_utt", "noise_start", "snr10", "ngain")):
        if want is None:
            assert g is None, (name, what)
        elif name == "ngain":
            _assert_bitwise(g, want, "ngain, " + what)
        else:
            assert g.dtype == torch.from_numpy(want).dtype and torch.equal(g.cpu(), torch.from_numpy(want)), (name, what)


@pytest.mark.parametrize("B,C", [(8, 2), (5, 3)])
def test_sampler_draws_and_minibatches_equal_the_oracle(world, B, C):
    c = world["corpus"]
    T, seed, rank = 4000, 0x1234_5678_9ABC, 3
    kw = dict(num_speakers=C, steps_per_epoch=50, seed=seed, rank=rank)
    loader = ctn.DynamicMixLoader(c, B, T, rirs=world["bank"], noise=world["noise"], snr_db=SNR_DB, **kw)
    plain = ctn.DynamicMixLoader(c, B, T, **kw)
    tb, nz = loader.tables, _noise_tables(world, T)
    assert list(nz["noise_ids"]) == [0, 2, 4, 5]                               # 3000 samples are too few, utterance 3 is silent
    mixture, sources = torch.empty(B, T, device=DEV), torch.empty(B, C, T, device=DEV)
    pm, ps = torch.empty(B, T, device=DEV), torch.empty(B, C, T, device=DEV)
    seen_rir, seen_snr, seen_noise = set(), set(), set()
    for epoch in (0, 2):
        loader.set_epoch(epoch)
        plain.set_epoch(epoch)
        for step in range(6):
            loader.fill(mixture, sources)
            plain.fill(pm, ps)
            what = "epoch %d step %d" % (epoch, step)
            if step in (0, 5):
                plan, aug, (w_mix, w_src, w_peak) = _oracle_step(world, tb, nz, seed, rank, epoch, step, B, C, T)
                _assert_bitwise(loader.last_peak(), w_peak, "peak, " + what)
                _assert_bitwise(mixture, w_mix, "mixture, " + what)
                _assert_bitwise(sources, w_src, "sources, " + what)
                assert np.all(w_peak > 0)
            else:
                plan = DO.plan(seed, rank, epoch, step, B, C, T, tb)
                aug = AO.plan_aug(seed, rank, epoch, step, B, C, T, R=6, noise=nz)
            _assert_plans(loader, plan, aug, what)
            # speaker, utterance, start and level draws are those of a loader without the options
            assert all(torch.equal(a, b) for a, b in zip(loader.last_plan(), plain.last_plan()))
            assert np.all(aug[3] >= -30) and np.all(aug[3] <= 60)
            seen_rir.update(int(v) for v in aug[0].reshape(-1))
            seen_snr.update(int(v) for v in aug[3])
            seen_noise.update(int(v) for v in aug[1])
    assert seen_rir == set(range(6)) and len(seen_snr) >= 3 and seen_noise <= {0, 2, 4, 5} and len(seen_noise) >= 2


def test_either_half_alone_is_bitwise_the_oracle(world):
    c = world["corpus"]
    B, C, T, seed, rank, epoch = 3, 2, 2500, 77, 0, 1
    nz = _noise_tables(world, T)
    mixture, sources = torch.empty(B, T, device=DEV), torch.empty(B, C, T, device=DEV)
    for rirs, noise in ((True, False), (False, True)):
        loader = ctn.DynamicMixLoader(c, B, T, steps_per_epoch=4, seed=seed, rank=rank, rirs=world["bank"] if rirs else None,
                                      noise=world["noise"] if noise else None, snr_db=SNR_DB)
        loader.set_epoch(epoch)
        for step in range(2):
            loader.fill(mixture, sources)
            plan, aug, (w_mix, w_src, w_peak) = _oracle_step(world, loader.tables, nz, seed, rank, epoch, step, B, C, T, rirs=rirs, noise=noise)
            _assert_plans(loader, plan, aug, "rirs %s noise %s step %d" % (rirs, noise, step))
            _assert_bitwise(loader.last_peak(), w_peak, "peak")
            _assert_bitwise(mixture, w_mix, "mixture")
            _assert_bitwise(sources, w_src, "sources")
    with pytest.raises(ValueError, match="noise"):
        ctn.DynamicMixLoader(c, B, 21000, noise=world["noise"])                # no noise file holds 21000 samples
    with pytest.raises(ValueError):
        ctn.DynamicMixLoader(c, B, T, noise=world["noise"], snr_db=(3, -6))


# ---- 4. composition with speed perturbation -----------------------------------------------------------------------------------
def test_speeds_then_reverb_then_noise_is_bitwise_the_oracle_chain(world):
    c = world["corpus"]
    B, C, T, seed, rank, epoch = 4, 2, 4000, 5, 1, 3
    loader = ctn.DynamicMixLoader(c, B, T, steps_per_epoch=4, seed=seed, rank=rank, speeds=SPEEDS, rirs=world["bank"], noise=world["noise"],
                                  snr_db=SNR_DB)
    loader.set_epoch(epoch)
    nz = _noise_tables(world, T)
    mixture, sources = torch.empty(B, T, device=DEV), torch.empty(B, C, T, device=DEV)
    for step in range(2):
        loader.fill(mixture, sources)
        plan, aug, (w_mix, w_src, w_peak) = _oracle_step(world, loader.tables, nz, seed, rank, epoch, step, B, C, T, speeds=SPEEDS)
        assert len(loader.last_plan()) == 5
        _assert_plans(loader, plan, aug, "step %d" % step)
        _assert_bitwise(loader.last_peak(), w_peak, "peak")
        _assert_bitwise(mixture, w_mix, "mixture")
        _assert_bitwise(sources, w_src, "sources")
    assert len(set(int(p) for p in plan[4].reshape(-1))) > 1


# ---- 5. identities --------------------------------------------------------------------------------------------------------------
def test_identities_tie_the_new_path_to_the_old_one(world):
    c = world["corpus"]
    B, C, T = 4, 2, 3001
    kw = dict(steps_per_epoch=3, seed=9, rank=2)
    plain = ctn.DynamicMixLoader(c, B, T, **kw)
    none = ctn.DynamicMixLoader(c, B, T, rirs=None, noise=None, **kw)
    assert none._aug is None and none.last_aug_plan() == (None,) * 5
    unit = ctn.DynamicMixLoader(c, B, T, rirs=ctn.RirBank.from_arrays([np.array([1.0])], DEV), **kw)
    assert unit._aug is not None and unit._aug.tgt is None
    for (pm, _, ps), (nm, _, ns), (um, _, us) in zip(plain, none, unit):
        assert torch.equal(pm, nm) and torch.equal(ps, ns)
        _assert_bitwise(nm, pm.cpu().numpy(), "mixture of rirs=None, noise=None")
        _assert_bitwise(ns, ps.cpu().numpy(), "sources of rirs=None, noise=None")
        # a bank of the one response [1.0]: the plain minibatch by value (the sign of a zero is the only licence)
        assert np.array_equal(um.cpu().numpy(), pm.cpu().numpy()) and np.array_equal(us.cpu().numpy(), ps.cpu().numpy())
        assert torch.equal(plain.last_peak(), unit.last_peak())
    utt, start, _, gain = plain.last_plan()
    a = dynmix.gather(c, utt, start, gain, T)
    zeros = torch.zeros(B)
    b = dynmix.gather_aug(c, utt, start, gain, T, noise=world["noise"], noise_utt=torch.zeros(B, dtype=torch.int32),
                          noise_start=torch.arange(B, dtype=torch.int64), ngain=zeros)
    assert all(np.array_equal(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(a, b))
    b = dynmix.gather_aug(c, utt, start, gain, T)                                # neither half: the plain gather, bit for bit
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError):
        dynmix.gather_aug(c, utt, start, gain, T, rirs=world["bank"])


# ---- 6. graph replay --------------------------------------------------------------------------------------------------------------
def test_captured_fill_replays_consecutive_steps_of_the_oracle(world):
    c = world["corpus"]
    B, C, T, seed = 3, 2, 2500, 31
    loader = ctn.DynamicMixLoader(c, B, T, steps_per_epoch=8, seed=seed, rank=0, rirs=world["bank"], noise=world["noise"], snr_db=SNR_DB)
    nz = _noise_tables(world, T)
    want = [_oracle_step(world, loader.tables, nz, seed, 0, 0, step, B, C, T)[2] for step in range(4)]
    mixture, sources = torch.empty(B, T, device=DEV), torch.empty(B, C, T, device=DEV)
    loader.fill(mixture, sources)                                              # step 0 eagerly
    _assert_bitwise(mixture, want[0][0], "mixture, step 0")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loader.fill(mixture, sources)
    for k in (1, 2, 3):
        graph.replay()
        torch.cuda.synchronize()
        _assert_bitwise(mixture, want[k][0], "mixture, step %d" % k)
        _assert_bitwise(sources, want[k][1], "sources, step %d" % k)
        _assert_bitwise(loader.last_peak(), want[k][2], "peak, step %d" % k)
    del graph
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    loader.fill(mixture, sources)
    assert torch.cuda.memory_allocated() == before                             # fill() allocates nothing


# ---- 7. train.py end to end --------------------------------------------------------------------------------------------------------
def test_train_cli_with_noise_rirs_and_speeds_runs_and_resumes(world, tmp_path, monkeypatch):
    """Two epochs of 3 steps on the tiny config with every option, finite losses; the run resumed from the first epoch's
    checkpoint draws the uninterrupted run's second epoch."""
    from scipy.io import wavfile
    from conv_tasnet_amd.train import main
    arrays, speakers = world["arrays"], world["speakers"]

    def write(name, x, sr=SR):
        p = str(tmp_path / name)
        wavfile.write(p, sr, np.round(x / np.abs(x).max() * 20000.0).astype(np.int16))
        return p

    infos = [[write("%d.wav" % u, np.resize(arrays[u], 3 * SR)), 3 * SR, speakers[u]] for u in (1, 2, 3, 8, 9, 10)]
    (tmp_path / "tr.json").write_text(json.dumps(infos))
    rng = np.random.RandomState(1)
    ninfos = [[write("n%d.wav" % k, rng.randn(n)), n, "noise"] for k, n in enumerate((9000, 2000, 6000))]
    (tmp_path / "noise.json").write_text(json.dumps(ninfos))
    first = []
    plain_iter = dynmix.DynamicMixLoader.__iter__

    def recorded(self):
        for k, batch in enumerate(plain_iter(self)):
            if k == 0:
                first.append((self.epoch, batch[0].clone(), batch[2].clone(), [None if t is None else t.cpu() for t in self.last_aug_plan()]))
            yield batch

    monkeypatch.setattr(dynmix.DynamicMixLoader, "__iter__", recorded)
    flags = ["--dynamic-mix", str(tmp_path / "tr.json"), "--noise", str(tmp_path / "noise.json"), "--snr=-3:6", "--rirs", "synthetic:8",
             "--speed-perturb", "95:105", "--tiny", "--segment-len", "4000", "--batch-size", "2", "--steps-per-epoch", "3", "--batches", "1"]
    solver = main(flags + ["--epochs", "2", "--checkpoint", "--save-folder", str(tmp_path / "full")])
    tr = solver.tr_loader
    assert tr.speeds == SPEEDS and tr._aug.rirs.num_responses == 8 and tr._aug.tgt is not None and (tr._aug.lo10, tr._aug.hi10) == (-30, 60)
    assert list(tr._aug.noise_ids_host) == [0, 2]
    assert len(solver.iter_losses) == 2 * (3 + 1) and all(np.isfinite(solver.iter_losses))
    assert [f[0] for f in first] == [0, 1] and not torch.equal(first[0][1], first[1][1])
    assert all(bool(torch.isfinite(f[1]).all()) and bool(torch.isfinite(f[2]).all()) for f in first)
    ck = tmp_path / "full" / "checkpoint_models" / "epoch1.pth.tar"
    assert ck.exists()
    resumed = main(flags + ["--epochs", "0", "--continue-from", str(ck), "--save-folder", str(tmp_path / "resumed")])
    assert resumed.start_epoch == 1 and len(first) == 3 and first[2][0] == 1
    assert torch.equal(first[2][1], first[1][1]) and torch.equal(first[2][2], first[1][2])
    assert all(torch.equal(a, b) for a, b in zip(first[2][3], first[1][3]))
    assert all(np.isfinite(resumed.iter_losses))
