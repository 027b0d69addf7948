"""GPU: speed perturbation in the on-device dynamic mixing (ctn_dynmix_plan_speed, ctn_dynmix_speed_segments, then the unchanged
gather) against the host restatement in resample_oracle.py / dynmix_oracle.py -- plans and percents equal, minibatches
BITWISE equal, speeds=(100,) bitwise the unperturbed loader, the other draws untouched, hand-written plans whose taps fall
off both ends of an utterance, flagged plans, graph replay, and train.py end to end."""
import json

import numpy as np
import pytest
import torch

import dynmix_oracle as DO
import resample_oracle as RO

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import dynmix, resample  # noqa: E402

DEV = "cuda:0"
SR = 8000
SPEEDS = tuple(range(95, 106))


def _arrays(seed=11, n_utt=60, n_spk=12):
    """About 60 utterances of 1 .. 12 s at 8 kHz over 12 speakers (the world of test_gpu_dynmix.py)."""
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


@pytest.fixture(scope="module")
def world():
    arrays, speakers = _arrays()
    corpus = ctn.DeviceCorpus.from_arrays(arrays, speakers, DEV)
    flat = np.concatenate(arrays)
    return arrays, speakers, corpus, flat


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _assert_bitwise(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = int((_bits(got) != _bits(want)).sum())
    assert bad == 0, "%s: %d of %d values differ in their bits" % (what, bad, want.size)


def _oracle_minibatch(corpus, flat, utt, start, pct, gain, T):
    seg = RO.speed_segments(flat, corpus.offsets_host, corpus.lens_host, utt, start, pct, T)
    return RO.mix_segments(seg, gain)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("B,C", [(8, 2), (5, 3)])
def test_sampler_plans_percents_and_minibatches_equal_the_oracle(world, B, C, mode):
    arrays, speakers, corpus, flat = world
    T, seed, rank = 12000, 0x1234_5678_9ABC, 3
    loader = ctn.DynamicMixLoader(corpus, B, T, num_speakers=C, steps_per_epoch=50, seed=seed, rank=rank, gather_mode=mode, speeds=SPEEDS)
    tb = loader.tables
    assert loader.eligible_len == 12600 and loader.speeds == SPEEDS
    assert all(corpus.lens_host[u] >= 12600 for u in tb["utt_ids"])
    mixture = torch.empty(B, T, device=DEV)
    sources = torch.empty(B, C, T, device=DEV)
    seen = set()
    for epoch in (0, 2):
        loader.set_epoch(epoch)
        for step in range(6):
            loader.fill(mixture, sources)
            utt, start, q, gain, pct = loader.last_plan()
            w_utt, w_start, w_q, w_gain, w_pct = RO.plan_speed(seed, rank, epoch, step, B, C, T, tb, SPEEDS)
            assert torch.equal(utt.cpu(), torch.from_numpy(w_utt)), (epoch, step)
            assert torch.equal(pct.cpu(), torch.from_numpy(w_pct)), (epoch, step)
            assert torch.equal(start.cpu(), torch.from_numpy(w_start)), (epoch, step)
            assert torch.equal(q.cpu(), torch.from_numpy(w_q)), (epoch, step)
            _assert_bitwise(gain, w_gain, "gain, epoch %d step %d" % (epoch, step))
            seen.update(int(p) for p in w_pct.reshape(-1))
            if step in (0, 5):
                w_mix, w_src, w_peak = _oracle_minibatch(corpus, flat, w_utt, w_start, w_pct, w_gain, T)
                _assert_bitwise(loader.last_peak(), w_peak, "peak, epoch %d step %d" % (epoch, step))
                _assert_bitwise(mixture, w_mix, "mixture, epoch %d step %d" % (epoch, step))
                _assert_bitwise(sources, w_src, "sources, epoch %d step %d" % (epoch, step))
                assert np.all(w_peak > 0)
    assert len(seen) >= 9                                        # at least 120 draws over 11 percents


@pytest.mark.parametrize("mode", [0, 1])
def test_identity_speed_is_bitwise_the_unperturbed_loader_and_other_draws_do_not_move(world, mode, monkeypatch):
    arrays, speakers, corpus, flat = world
    B, C, T = 6, 2, 8000
    kw = dict(num_speakers=C, steps_per_epoch=8, seed=5, rank=1, gather_mode=mode)
    ident = ctn.DynamicMixLoader(corpus, B, T, speeds=(100,), **kw)
    # the sampler's tables of a loader with speeds are those of the longest span it can draw
    wide = ctn.DynamicMixLoader(corpus, B, T, speeds=SPEEDS, **kw)
    same_tables = ctn.DynamicMixLoader(corpus, B, resample.eligible_len(T, SPEEDS), **kw)
    # speeds=None never enters the new code
    for name in ("parse_speeds", "speed_banks", "device_filter"):
        monkeypatch.setattr(resample, name, lambda *a, **k: pytest.fail("speeds=None reached resample.%s" % name))
    probe = ctn.DynamicMixLoader(corpus, B, T, **kw)
    probe.fill(torch.empty(B, T, device=DEV), torch.empty(B, C, T, device=DEV))
    assert probe.speeds is None and len(probe.last_plan()) == 4
    monkeypatch.undo()
    plain = ctn.DynamicMixLoader(corpus, B, T, **kw)
    bufs = [(torch.empty(B, T, device=DEV), torch.empty(B, C, T, device=DEV)) for _ in range(2)]
    for ld in (ident, wide, plain, same_tables):
        ld.set_epoch(1)
    for step in range(8):
        plain.fill(*bufs[0])
        ident.fill(*bufs[1])
        assert torch.equal(bufs[0][0], bufs[1][0]) and torch.equal(bufs[0][1], bufs[1][1]), step
        assert torch.equal(plain.last_peak(), ident.last_peak())
        p, i = plain.last_plan(), ident.last_plan()
        assert len(p) == 4 and len(i) == 5 and all(torch.equal(a, b) for a, b in zip(p, i[:4])) and bool((i[4] == 100).all())
        big = torch.empty(B, same_tables.T, device=DEV), torch.empty(B, C, same_tables.T, device=DEV)
        wide.fill(*bufs[1])
        same_tables.fill(*big)
        w, s = wide.last_plan(), same_tables.last_plan()
        assert torch.equal(w[0], s[0]) and torch.equal(w[2], s[2]) and torch.equal(w[3], s[3])       # speaker, utterance, level
        assert bool(((w[4] >= 95) & (w[4] <= 105)).all())


def _hand_plans(corpus, T):
    """Rows of (utterances, starts, percents): starts 0 and len - need, so taps fall off both ends of the utterance, starts
    inside it, where they read real samples beyond the nominal segment, and every percent of {95, 100, 103, 105}."""
    n = [int(v) for v in corpus.lens_host]
    end = lambda u, p: n[u] - resample.need(T, p)
    rows = [([1, 2], [0, 0], [95, 103]),
            ([2, 3], [end(2, 105), end(3, 100)], [105, 100]),
            ([3, 1], [end(3, 95), end(1, 103)], [95, 103]),
            ([1, 1], [end(1, 100), end(1, 105)], [100, 105]),
            ([2, 3], [17, 4001], [103, 95]),
            ([3, 2], [1, end(2, 103) - 1], [105, 103])]
    last = corpus.num_utterances - 1                                       # ends on the last sample of the corpus buffer
    rows.append(([last, 1], [end(last, 105), 3], [105, 100]))
    return (np.array([r[0] for r in rows], np.int32), np.array([r[1] for r in rows], np.int64), np.array([r[2] for r in rows], np.int32))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("T", [1, 63, 4000, 4001])
def test_gather_of_hand_written_plans_with_speeds_is_bitwise_the_oracle(world, T, mode):
    arrays, speakers, corpus, flat = world
    utt, start, pct = _hand_plans(corpus, T)
    assert np.all(start >= 0)
    gain = np.random.RandomState(T).uniform(0.5, 20.0, size=utt.shape).astype(np.float32)
    mixture, sources, peak = dynmix.gather(corpus, torch.from_numpy(utt), torch.from_numpy(start), torch.from_numpy(gain), T, mode=mode,
                                           plan_pct=torch.from_numpy(pct))
    torch.cuda.synchronize()
    w_mix, w_src, w_peak = _oracle_minibatch(corpus, flat, utt, start, pct, gain, T)
    _assert_bitwise(peak, w_peak, "peak")
    _assert_bitwise(mixture, w_mix, "mixture")
    _assert_bitwise(sources, w_src, "sources")
    # the same plan at 100 % everywhere is the plain gather
    hundred = np.full_like(pct, 100)
    a = dynmix.gather(corpus, torch.from_numpy(utt), torch.from_numpy(start), torch.from_numpy(gain), T, mode=mode,
                      plan_pct=torch.from_numpy(hundred))
    b = dynmix.gather(corpus, torch.from_numpy(utt), torch.from_numpy(start), torch.from_numpy(gain), T, mode=mode)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_three_sources_and_a_bank_read_through_the_cache(world):
    """C = 3, and 199 %: 100 phases of 137 words do not fit the LDS beside the input span, so that bank is read from memory."""
    arrays, speakers, corpus, flat = world
    T = 1500
    utt = np.array([[1, 2, 3], [3, 1, 2]], np.int32)
    pct = np.array([[199, 50, 97], [100, 199, 200]], np.int32)
    start = np.array([[0, 5, int(corpus.lens_host[3]) - resample.need(T, 97)], [9, int(corpus.lens_host[1]) - resample.need(T, 199), 0]], np.int64)
    banks = resample.speed_banks([50, 97, 199, 200], DEV)
    assert banks.bank_cap < 100 * 137 and banks.bank_cap >= 100 * 69 and 4 * (banks.span_cap + banks.bank_cap) <= 60 * 1024
    gain = np.random.RandomState(3).uniform(0.5, 2.0, size=utt.shape).astype(np.float32)
    for mode in (0, 1):
        mixture, sources, peak = dynmix.gather(corpus, torch.from_numpy(utt), torch.from_numpy(start), torch.from_numpy(gain), T, mode=mode,
                                               plan_pct=torch.from_numpy(pct))
        w_mix, w_src, w_peak = _oracle_minibatch(corpus, flat, utt, start, pct, gain, T)
        _assert_bitwise(peak, w_peak, "peak")
        _assert_bitwise(mixture, w_mix, "mixture")
        _assert_bitwise(sources, w_src, "sources")


def test_a_plan_whose_span_leaves_the_utterance_is_flagged_and_reads_nothing_there(world):
    """Not a fault test: the kernel checks every plan entry against the tables before it forms an address."""
    arrays, speakers, corpus, flat = world
    T = 64
    n1 = int(corpus.lens_host[1])
    utt = np.array([[1, 2], [1, 2], [corpus.num_utterances, 2], [1, -1], [1, 2], [1, 2], [1, 2]], dtype=np.int32)
    pct = np.array([[105, 95], [105, 95], [100, 95], [100, 95], [95, 100], [49, 100], [100, 201]], dtype=np.int32)
    start = np.array([[n1 - resample.need(T, 105), 0], [n1 - resample.need(T, 105) + 1, 0], [0, 0], [0, 0], [-1, 0], [0, 0], [0, 0]],
                     dtype=np.int64)
    gain = np.ones(utt.shape, dtype=np.float32)
    for mode in (0, 1):
        mixture, sources, peak = dynmix.gather(corpus, torch.from_numpy(utt), torch.from_numpy(start), torch.from_numpy(gain), T, mode=mode,
                                               plan_pct=torch.from_numpy(pct))
        peak = peak.cpu().numpy()
        assert peak[0] > 0 and list(peak[1:]) == [-1.0] * 6
        src = sources.cpu().numpy()
        assert not src[1, 0].any() and not src[2, 0].any() and not src[3, 1].any() and not src[4, 0].any()
        assert not src[5, 0].any() and not src[6, 1].any()
        assert src[0, 0].any() and src[1, 1].any() and src[5, 1].any()


def test_captured_fill_with_speeds_replays_consecutive_steps(world):
    arrays, speakers, corpus, flat = world
    B, T = 4, 8000

    def make():
        return ctn.DynamicMixLoader(corpus, B, T, steps_per_epoch=6, seed=9, rank=0, speeds=SPEEDS)

    eager = [(m.clone(), s.clone()) for m, _, s in make()]
    assert len(eager) == 6 and not torch.equal(eager[0][0], eager[1][0])
    loader = make()
    mixture, sources = torch.empty(B, T, device=DEV), torch.empty(B, 2, T, device=DEV)
    loader.fill(mixture, sources)
    loader.fill(mixture, sources)                                    # steps 0 and 1 eagerly: k = 2
    assert torch.equal(mixture, eager[1][0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loader.fill(mixture, sources)
    for k in (2, 3, 4):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(mixture, eager[k][0]) and torch.equal(sources, eager[k][1]), k
    loader.fill(mixture, sources)                                    # and eagerly again where the replays left the step word
    assert torch.equal(mixture, eager[5][0])
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    loader.fill(mixture, sources)
    assert torch.cuda.memory_allocated() == before                   # fill() allocates nothing
    with pytest.raises(ValueError):
        ctn.DynamicMixLoader(corpus, B, T, speeds=(40, 100))
    with pytest.raises(ValueError):
        ctn.DynamicMixLoader(corpus, B, 12 * SR, speeds=(100, 110))  # no utterance holds 13.2 s


def test_train_cli_with_speed_perturbation_runs_end_to_end(world, tmp_path):
    """train.py --dynamic-mix ... --speed-perturb 95:105 --corpus-rate auto: two steps of the tiny model on a corpus with one
    file at 16 kHz, finite losses."""
    from scipy.io import wavfile
    from conv_tasnet_amd.train import main
    arrays, speakers, corpus, flat = world
    infos = []
    for u in (1, 2, 3, 8, 9, 10):
        x = np.round(np.resize(arrays[u], 3 * SR) / np.abs(arrays[u]).max() * 20000.0).astype(np.int16)
        sr = 16000 if u == 3 else SR
        p = str(tmp_path / ("%d.wav" % u))
        wavfile.write(p, sr, x)
        infos.append([p, len(x), speakers[u]])
    (tmp_path / "tr.json").write_text(json.dumps(infos))
    solver = main(["--dynamic-mix", str(tmp_path / "tr.json"), "--speed-perturb", "95:105", "--corpus-rate", "auto", "--tiny",
                   "--segment-len", "4000", "--batch-size", "2", "--steps-per-epoch", "2", "--epochs", "1", "--batches", "1",
                   "--save-folder", str(tmp_path / "exp")])
    assert solver.tr_loader.speeds == SPEEDS and list(solver.tr_loader.corpus.lens_host) == [24000, 24000, 12000, 24000, 24000, 24000]
    assert len(solver.iter_losses) == 3 and all(np.isfinite(solver.iter_losses))
