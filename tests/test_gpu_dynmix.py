"""GPU: on-device dynamic mixing (csrc/ctn_dynmix.hip, dynmix.py) against the host restatement in dynmix_oracle.py -- levels
within the fp64 summation-order bound, plans equal, gains and minibatches BITWISE equal, the loader's epoch / rank / resume
semantics, graph replay, and a Solver run end to end."""
import gc

import numpy as np
import pytest
import torch

import dynmix_oracle as DO
from conftest import DEFAULT_ARITH, set_arith

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import dynmix  # noqa: E402

DEV = "cuda:0"
SR = 8000
ZERO_HEAD = 4200                     # utterance 0 starts with this many exact zeros
ULP09 = float(np.nextafter(np.float32(0.9), np.float32(1.0)) - np.float32(0.9))


def _arrays(seed=11, n_utt=60, n_spk=12):
    """About 60 utterances of 1 .. 12 s at 8 kHz over 12 speakers; every value is 0 or at least 2^-15 in magnitude."""
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
    arrays[0][:ZERO_HEAD] = 0.0
    arrays[7][:] = 0.0                                        # a silent utterance: never eligible
    return arrays, speakers


@pytest.fixture(scope="module")
def world():
    arrays, speakers = _arrays()
    corpus = ctn.DeviceCorpus.from_arrays(arrays, speakers, DEV)
    flat = np.concatenate(arrays)
    return arrays, speakers, corpus, flat


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else np.uint64)


def _assert_bitwise(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = int((_bits(got) != _bits(want)).sum())
    assert bad == 0, "%s: %d of %d values differ in their bits" % (what, bad, want.size)


def test_levels_within_the_summation_order_bound(world):
    arrays, speakers, corpus, flat = world
    assert corpus.num_utterances == len(arrays) and corpus.num_speakers == 12 and corpus.num_samples == flat.size
    got = corpus.meansq
    want = DO.meansq(flat, corpus.offsets_host, corpus.lens_host)
    assert got.dtype == np.float64 and got.shape == want.shape
    worst = 0.0
    for u, n in enumerate(corpus.lens_host):
        if want[u] == 0:
            assert got[u] == 0
            continue
        rel = abs(got[u] - want[u]) / want[u]
        bound = 2.0 * (int(n) + 1) * 2.0 ** -53
        worst = max(worst, rel / bound)
        assert rel <= bound, (u, int(n), rel, bound)
    print("levels: worst relative difference / bound = %.3e" % worst)
    # an utterance alone in a corpus has bitwise the level it has among its neighbours
    for u in (0, 3, 7, 31, len(arrays) - 1):
        alone = ctn.DeviceCorpus.from_arrays([arrays[u]], [speakers[u]], DEV)
        assert _bits(alone.meansq)[0] == _bits(got)[u], u


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("B,C", [(8, 2), (5, 3)])
def test_sampler_plans_gains_and_minibatches_equal_the_oracle(world, B, C, mode):
    arrays, speakers, corpus, flat = world
    T, seed, rank, epoch = 12000, 0x1234_5678_9ABC, 3, 2
    loader = ctn.DynamicMixLoader(corpus, B, T, num_speakers=C, steps_per_epoch=50, seed=seed, rank=rank, gather_mode=mode)
    loader.set_epoch(epoch)
    tb = loader.tables
    assert len(tb["utt_ids"]) < len(arrays)                    # T = 1.5 s: some utterances are too short, one is silent
    mixture = torch.empty(B, T, device=DEV)
    sources = torch.empty(B, C, T, device=DEV)
    for step in range(50):
        loader.fill(mixture, sources)
        utt, start, q, gain = loader.last_plan()
        w_utt, w_start, w_q, w_gain = DO.plan(seed, rank, epoch, step, B, C, T, tb)
        assert torch.equal(utt.cpu(), torch.from_numpy(w_utt)), step
        assert torch.equal(start.cpu(), torch.from_numpy(w_start)), step
        assert torch.equal(q.cpu(), torch.from_numpy(w_q)), step
        host_gain = tb["w"][w_q + 249] * tb["inv_rms"][w_utt]
        assert host_gain.dtype == np.float32
        _assert_bitwise(gain, host_gain, "gain, step %d" % step)
        _assert_bitwise(gain, w_gain, "gain vs oracle, step %d" % step)
        if step % 5 == 0 or step == 49:
            w_mix, w_src, w_peak = DO.mix(flat, corpus.offsets_host, w_utt, w_start, w_gain, T)
            _assert_bitwise(mixture, w_mix, "mixture, step %d" % step)
            _assert_bitwise(sources, w_src, "sources, step %d" % step)
            _assert_bitwise(loader.last_peak(), w_peak, "peak, step %d" % step)
            _check_peak(w_mix, w_src)


def _check_peak(mixture, sources):
    """Largest magnitude over mix and sources of every non-silent mixture: 0.9f or one float32 ulp to either side, and
    nothing above that."""
    for b in range(mixture.shape[0]):
        top = max(float(np.abs(mixture[b]).max()), float(np.abs(sources[b]).max()))
        if top == 0.0:
            continue
        assert abs(top - float(np.float32(0.9))) <= ULP09, (b, top)


def _hand_plans(corpus, T, C):
    """Rows of (utterances, starts) that exercise every misalignment of a 16-byte load, the end of the corpus buffer, an
    utterance used twice and an all-zero segment."""
    last = corpus.num_utterances - 1
    end = int(corpus.lens_host[last]) - T
    assert end >= 0 and int(corpus.offsets_host[last]) + end + T == corpus.num_samples
    rows = [([1, 2, 3, 1][:C], [0, 1, 2, 3][:C]),
            ([2, 3, 1, 2][:C], [5, 0, 3, 1][:C]),
            ([1, 3, 2, 3][:C], [3, 2, 5, 0][:C]),
            ([3, 2, 1, 2][:C], [2, 5, 1, 2][:C]),
            ([last, 1, last, 2][:C], [end, 1, end, 7][:C]),             # ends on the last sample of the corpus buffer
            ([2, 1, 2, 1][:C], [5, 0, 3, 1][:C]),                       # utterances 1 and 2 again in this batch
            ([1, 1, 1, 1][:C], [0, 6001, 13, 40000][:C]),               # one utterance for every source
            ([0, 0, 0, 0][:C], [0, 10, 3, 100][:C]),                    # all zeros (ZERO_HEAD): peak 0, scale 1
            ([0, 2, 0, 0][:C], [0, 9, 17, 5][:C])]                      # one silent source beside a live one
    utt = np.array([r[0] for r in rows], dtype=np.int32)
    start = np.array([r[1] for r in rows], dtype=np.int64)
    return utt, start


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("C", [2, 3, 4])
@pytest.mark.parametrize("T", [1, 63, 4001, 4000])
def test_gather_of_hand_written_plans_is_bitwise_the_oracle(world, T, C, mode):
    arrays, speakers, corpus, flat = world
    utt, start = _hand_plans(corpus, T, C)
    rng = np.random.RandomState(T + C)
    gain = rng.uniform(0.5, 20.0, size=utt.shape).astype(np.float32)
    gain[3] = np.float32(1.0)
    mixture, sources, peak = dynmix.gather(corpus, torch.from_numpy(utt), torch.from_numpy(start), torch.from_numpy(gain), T, mode=mode)
    torch.cuda.synchronize()
    w_mix, w_src, w_peak = DO.mix(flat, corpus.offsets_host, utt, start, gain, T)
    _assert_bitwise(peak, w_peak, "peak")
    _assert_bitwise(mixture, w_mix, "mixture")
    _assert_bitwise(sources, w_src, "sources")
    assert w_peak[7] == 0 and not w_mix[7].any() and not w_src[7].any()
    assert not w_src[8, 0].any() and (T < 8 or w_src[8, 1].any())
    _check_peak(w_mix, w_src)


def test_gather_flags_a_plan_outside_its_utterance_and_reads_nothing_there(world):
    """Not a fault test: the kernel checks every plan entry against the tables before it forms an address."""
    arrays, speakers, corpus, flat = world
    T = 64
    n1 = int(corpus.lens_host[1])
    utt = np.array([[1, 2], [1, 2], [corpus.num_utterances, 2], [1, -1], [1, 2]], dtype=np.int32)
    start = np.array([[0, 0], [n1 - T + 1, 0], [0, 0], [0, 0], [-1, 0]], dtype=np.int64)
    gain = np.ones(utt.shape, dtype=np.float32)
    for mode in (0, 1):
        mixture, sources, peak = dynmix.gather(corpus, torch.from_numpy(utt), torch.from_numpy(start), torch.from_numpy(gain), T, mode=mode)
        peak = peak.cpu().numpy()
        assert peak[0] > 0 and list(peak[1:]) == [-1.0] * 4
        src = sources.cpu().numpy()
        assert not src[1, 0].any() and not src[2, 0].any() and not src[3, 1].any() and not src[4, 0].any()
        assert src[1, 1].any()


def _take(loader, n=None):
    out = []
    for i, (mix, lens, src) in enumerate(loader):
        out.append((mix.clone(), lens.clone(), src.clone()))
        if n is not None and i + 1 == n:
            break
    return out


def _same(a, b):
    return all(torch.equal(x[0], y[0]) and torch.equal(x[2], y[2]) for x, y in zip(a, b)) and len(a) == len(b)


def test_loader_contract_epochs_ranks_and_fill(world):
    arrays, speakers, corpus, flat = world
    B, T = 4, 8000

    def make(**kw):
        return ctn.DynamicMixLoader(corpus, B, T, steps_per_epoch=6, **dict(dict(seed=5, rank=0), **kw))

    a, b = make(), make()
    assert len(a) == 6 and a.dataset is a
    ea = _take(a)
    assert len(ea) == 6
    mix, lens, src = ea[0]
    assert mix.shape == (B, T) and src.shape == (B, 2, T) and mix.dtype == src.dtype == torch.float32
    assert lens.dtype == torch.int64 and lens.tolist() == [T] * B and mix.device == src.device == lens.device == corpus.device
    assert _same(ea, _take(b))                                       # same arguments: identical streams
    assert not torch.equal(ea[0][0], ea[1][0])                       # consecutive steps differ
    assert not _same(ea, _take(make(rank=1)))                        # every rank draws its own stream
    assert not _same(ea, _take(make(seed=6)))
    # rank=None takes the process's rank: 0 in a single-process run
    assert _same(ea, _take(ctn.DynamicMixLoader(corpus, B, T, steps_per_epoch=6, seed=5)))
    # set_epoch(3) on a used loader reproduces a fresh loader's epoch 3; iterating again repeats the selected epoch
    a.dataset.set_epoch(3)
    e3 = _take(a)
    fresh = make()
    fresh.dataset.set_epoch(3)
    assert _same(e3, _take(fresh)) and not _same(e3, ea)
    a.dataset.set_epoch(0)
    assert _same(ea, _take(a))
    # reshuffle=False: epoch 0 whatever the Solver sets
    fixed = make(reshuffle=False)
    f0 = _take(fixed)
    fixed.dataset.set_epoch(4)
    assert _same(f0, _take(fixed)) and _same(f0, ea)
    # a loop that stops early and starts again begins at step 0 again
    assert _same(_take(a, 2), ea[:2])
    # fill() into caller buffers == iteration, with no allocation and the lengths written when asked for
    c = make()
    mixture, sources = torch.empty(B, T, device=DEV), torch.empty(B, 2, T, device=DEV)
    lengths = torch.zeros(B, dtype=torch.int64, device=DEV)
    c.fill(mixture, sources, lengths)
    assert torch.equal(mixture, ea[0][0]) and torch.equal(sources, ea[0][2]) and lengths.tolist() == [T] * B
    gc.collect()                        # cyclic garbage of earlier tests must not be freed inside the window that counts allocations
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for step in range(1, 6):
        c.fill(mixture, sources)
        assert torch.cuda.memory_allocated() == before
        assert torch.equal(mixture, ea[step][0]) and torch.equal(sources, ea[step][2])
    for _ in range(5):
        c.fill(mixture, sources)
    assert torch.cuda.memory_allocated() == before
    with pytest.raises(ValueError):
        c.fill(mixture[:, :-1], sources)
    with pytest.raises(ValueError):
        c.fill(mixture.double(), sources)
    with pytest.raises(ValueError):
        ctn.DynamicMixLoader(corpus, B, 13 * SR, steps_per_epoch=1)             # no utterance is that long
    with pytest.raises(ValueError):
        ctn.DynamicMixLoader(corpus, B, T, seed=1 << 48)
    # memory: 4 bytes per sample plus the per-utterance tables
    U = corpus.num_utterances
    assert corpus.device_bytes() == 4 * corpus.num_samples + U * (8 + 8 + 4) + 4 * 499


def test_from_manifest_reads_every_file_once(tmp_path, world):
    import json
    from scipy.io import wavfile
    from conv_tasnet_amd.data import read_wav
    rng = np.random.RandomState(2)
    infos, arrays = [], []
    for spk in ("a", "b"):
        (tmp_path / spk).mkdir()
        for k in range(2):
            x = (rng.randn(3000 + 100 * k) * 3000).astype(np.int16)
            p = str(tmp_path / spk / ("%d.wav" % k))
            wavfile.write(p, SR, x)
            infos.append([p, len(x), spk])
            arrays.append(x.astype(np.float32) / 32768.0)
    (tmp_path / "m.json").write_text(json.dumps(infos))
    seen = []

    def reader(path, sr):
        seen.append(path)
        return read_wav(path, sr)

    corpus = ctn.DeviceCorpus.from_manifest(str(tmp_path / "m.json"), SR, DEV, reader=reader)
    assert seen == [i[0] for i in infos] and corpus.num_speakers == 2 and corpus.num_utterances == 4
    assert np.array_equal(corpus.corpus.cpu().numpy(), np.concatenate(arrays))
    loader = ctn.DynamicMixLoader(corpus, 3, 2500, steps_per_epoch=2)
    mix, lens, src = next(iter(loader))
    utt = loader.last_plan()[0].cpu().numpy()
    assert all(infos[u0][2] != infos[u1][2] for u0, u1 in utt)
    infos[0][1] += 1
    (tmp_path / "bad.json").write_text(json.dumps(infos))
    with pytest.raises(ValueError, match="manifest"):
        ctn.DeviceCorpus.from_manifest(str(tmp_path / "bad.json"), SR, DEV)


def test_captured_fill_replays_consecutive_steps(world):
    """fill() captured once (a straight chain on one stream) and replayed three times gives steps k, k+1, k+2: the step word
    lives in device memory and the plan kernel advances it."""
    arrays, speakers, corpus, flat = world
    B, T = 4, 8000
    eager = _take(ctn.DynamicMixLoader(corpus, B, T, steps_per_epoch=6, seed=9, rank=0))
    loader = ctn.DynamicMixLoader(corpus, B, T, steps_per_epoch=6, seed=9, rank=0)
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
        assert torch.equal(mixture, eager[k][0]) and torch.equal(sources, eager[k][2]), k
    loader.fill(mixture, sources)                                    # and eagerly again where the replays left the step word
    assert torch.equal(mixture, eager[5][0])


class _Recorded:
    """A loader that records what it hands out."""

    def __init__(self, loader):
        self.loader, self.dataset = loader, loader.dataset
        self.epochs = []

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        rec = []
        self.epochs.append(rec)
        for batch in self.loader:
            rec.append(dict(plan=[t.cpu() for t in self.loader.last_plan()], mixture=batch[0].clone(), sources=batch[2].clone()))
            yield batch


def _same_plans(a, b):
    return len(a) == len(b) and all(all(torch.equal(x, y) for x, y in zip(p["plan"], q["plan"])) for p, q in zip(a, b))


def test_train_end_to_end_and_resume_sees_the_same_minibatches(world, tmp_path):
    """train() on the tiny config with a DynamicMixLoader for training and a reshuffle=False one for validation, then the
    same run resumed from the first epoch's checkpoint: the resumed run's minibatches are the uninterrupted run's (the
    loader's property), and under the fp32 arithmetic its losses are too (fixed-order step, float32 state stored exactly)."""
    from conv_tasnet_amd.train import train
    arrays, speakers, corpus, flat = world
    cfg = dict(N=64, L=20, B=32, H=64, P=3, X=2, R=2, C=2)
    T, B = 4000, 2

    def loaders():
        tr = _Recorded(ctn.DynamicMixLoader(corpus, B, T, steps_per_epoch=4, seed=21, rank=0))
        cv = _Recorded(ctn.DynamicMixLoader(corpus, B, T, steps_per_epoch=2, seed=22, rank=0, reshuffle=False))
        return tr, cv

    set_arith("fp32")
    try:
        tr, cv = loaders()
        full = train({"tr_loader": tr, "cv_loader": cv}, 2, "final.pth.tar", save_folder=str(tmp_path / "full"), config=cfg,
                     print_freq=1000, enable_checkpoint=1)
        assert len(full.iter_losses) == 2 * (4 + 2) and all(np.isfinite(full.iter_losses))
        assert len(tr.epochs) == 2 and len(tr.epochs[0]) == 4 and len(cv.epochs) == 2 and len(cv.epochs[0]) == 2
        assert not _same_plans(tr.epochs[0], tr.epochs[1])
        assert not any(torch.equal(p["mixture"], q["mixture"]) for p, q in zip(tr.epochs[0], tr.epochs[1]))
        assert _same_plans(cv.epochs[0], cv.epochs[1])
        assert all(torch.equal(p["mixture"], q["mixture"]) and torch.equal(p["sources"], q["sources"])
                   for p, q in zip(cv.epochs[0], cv.epochs[1]))
        ck = tmp_path / "full" / "checkpoint_models" / "epoch1.pth.tar"
        assert ck.exists()
        tr2, cv2 = loaders()
        resumed = train({"tr_loader": tr2, "cv_loader": cv2}, 0, "final.pth.tar", save_folder=str(tmp_path / "resumed"), config=cfg,
                        print_freq=1000, continue_from=str(ck))
        assert resumed.start_epoch == 1 and len(tr2.epochs) == 1
        # the loader's property, exact: the resumed run's first epoch is the uninterrupted run's second
        assert _same_plans(tr2.epochs[0], tr.epochs[1])
        assert all(torch.equal(p["mixture"], q["mixture"]) and torch.equal(p["sources"], q["sources"])
                   for p, q in zip(tr2.epochs[0], tr.epochs[1]))
        assert _same_plans(cv2.epochs[0], cv.epochs[1])
        print("losses, uninterrupted epoch 2:", full.iter_losses[6:], "resumed:", resumed.iter_losses)
        assert resumed.iter_losses == full.iter_losses[6:]
    finally:
        set_arith(DEFAULT_ARITH)
