"""GPU: streaming.ResamplingStreamPool -- the slot pool fed at a client's sample rate -- and separate(file_rate=...).
The yardstick is the offline pipeline of code that existed before: resample.resample -> FusedStreamingSeparator(batch=1) on the
zero-padded model-rate signal as one push plus flush() -> cut -> resample.resample.  Every comparison is torch.equal."""
import os

import numpy as np
import pytest
import torch

from oracle import ctn_oracle as O

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import resample  # noqa: E402
from conv_tasnet_amd.streaming import FusedStreamingSeparator, ResamplingStreamPool  # noqa: E402

DEV = "cuda:0"
S, L, C = 10, 20, 2
RATES = [(16000, 16000), (48000, None), (11025, 16000)]         # 11025 -> 8000 is 320 / 441: a bank that goes through the cache
_CACHE = {}


def _model(seed=2):
    if seed not in _CACHE:
        torch.manual_seed(seed)
        _CACHE[seed] = ctn.ConvTasNet(32, 20, 16, 32, 3, 4, 2, 2, norm_type="cLN", causal=True).to(DEV).eval()
    return _CACHE[seed]


def _offline(m, x, rate_in, rate_out):
    """The contract's pipeline for one signal x [T] (a CPU tensor) -> [C, n] on the device."""
    if x.numel() == 0:
        return torch.zeros((C, 0), device=DEV)
    x8 = resample.resample(x.to(DEV), rate_in, 8000)
    n8 = x8.shape[0]
    padded = torch.zeros(max(L, -(-n8 // S) * S), device=DEV)
    padded[:n8] = x8
    s = FusedStreamingSeparator(m, batch=1, max_chunk_frames=64)
    y8 = torch.cat([s.push(padded[None]), s.flush()], dim=2)[0, :, :n8].contiguous()
    return y8 if rate_out is None else resample.resample(y8, 8000, rate_out)


def _streams(rate_in):
    """(slot, push at which it opens, sample counts per push, signal).  Slot 0 runs throughout; slot 1 joins late; slot 2 serves a
    signal scaled by 100, is closed and reopened with another one; slot 3's first stream gives fewer than L model-rate samples, its
    second is empty (closed right after open)."""
    k = rate_in // 8000 if rate_in % 8000 == 0 else 1
    short = 7 * k + 1                                           # at most 11 model-rate samples
    plan = [(0, 0, [163, 0, 7, 1200 * k, 480, 1, 900 * k, 333]),
            (1, 3, [81, 2 * k, 700 * k, 0, 160]),
            (2, 0, [500, 37, 0]),
            (2, 4, [1, 159, 1000 * k, 16]),
            (3, 1, [3, short - 3]),
            (3, 5, [])]
    mix, _, _ = O.synth_batch(8, len(plan), max(sum(c) for _, _, c in plan) + 1)
    return [(slot, opens, cuts, mix[i, :sum(cuts)] * (100.0 if (slot, opens) == (2, 0) else 1.0)) for i, (slot, opens, cuts) in enumerate(plan)]


def _drive(pool, streams, slots=4):
    got, total = [[] for _ in streams], [0] * len(streams)
    at = [0] * len(streams)
    n_push = max(o + max(len(c), 1) for _, o, c, _ in streams)
    for p in range(n_push):
        counts, live = [0] * slots, {}
        for i, (slot, opens, cuts, x) in enumerate(streams):
            if p == opens:
                assert pool.open(slot) == slot
            if opens <= p < opens + len(cuts):
                counts[slot], live[slot] = cuts[p - opens], i
        chunk = torch.full((slots, max(counts) + 5), float("nan"))              # NaN beyond every count and in idle rows
        for slot, i in live.items():
            chunk[slot, :counts[slot]] = streams[i][3][at[i]:at[i] + counts[slot]]
            at[i] += counts[slot]
        out, lengths = pool.push(chunk.to(DEV), counts)
        assert out.shape == (slots, C, max(lengths)) and len(lengths) == slots
        for slot in range(slots):
            assert not out[slot, :, lengths[slot]:].any()                       # zeros beyond each slot's length
            assert slot in live or lengths[slot] == 0
        for slot, i in live.items():
            got[i].append(out[slot, :, :lengths[slot]])
            total[i] += lengths[slot]
        for i, (slot, opens, cuts, x) in enumerate(streams):
            if p == opens + max(len(cuts), 1) - 1:
                tail = pool.close(slot)
                assert tail.dim() == 2 and tail.shape[0] == C
                got[i].append(tail)
                total[i] += tail.shape[1]
    assert at == [s[3].numel() for s in streams]
    return [torch.cat(g, dim=1) for g in got], total


@pytest.mark.parametrize("rate_in,rate_out", RATES)
def test_pool_at_a_client_rate_is_bitwise_the_offline_pipeline(rate_in, rate_out):
    m = _model()
    streams = _streams(rate_in)
    pool = ResamplingStreamPool(m, slots=4, max_chunk_frames=16, input_rate=rate_in, output_rate=rate_out)
    got, total = _drive(pool, streams)
    for (slot, opens, cuts, x), y, n in zip(streams, got, total):
        n8 = resample.out_len(x.numel(), *resample.ratio(rate_in, 8000))
        assert n == (n8 if rate_out is None else resample.out_len(n8, *resample.ratio(8000, rate_out)))
        if (slot, opens) == (3, 1):
            assert 0 < n8 < L
        want = _offline(m, x, rate_in, rate_out)
        assert y.shape == want.shape == (C, n), (slot, opens)
        assert torch.isfinite(y).all()
        assert torch.equal(y, want), (slot, opens, int((y != want).sum()))
    assert not any(pool.is_open)
    if rate_in == 16000:
        _CACHE["eager"] = got


def test_graph_replay_gives_the_same_bits():
    m = _model()
    streams = _streams(16000)
    if "eager" not in _CACHE:
        _CACHE["eager"], _ = _drive(ResamplingStreamPool(m, slots=4, max_chunk_frames=16, input_rate=16000, output_rate=16000), streams)
    pool = ResamplingStreamPool(m, slots=4, max_chunk_frames=16, input_rate=16000, output_rate=16000, graph=True)
    got, _ = _drive(pool, streams)
    assert pool.pool._graphs, "no step was replayed"
    for a, b in zip(_CACHE["eager"], got):
        assert torch.equal(a, b)


def test_zeros_8_and_errors():
    m = _model()
    pool = ResamplingStreamPool(m, slots=2, max_chunk_frames=16, input_rate=16000, output_rate=16000, zeros=8)
    x = O.synth_batch(9, 1, 2000)[0][0]
    pool.open(1)
    chunk = torch.zeros(2, 2000)
    chunk[1] = x
    out, lengths = pool.push(chunk.to(DEV), [0, 2000])
    got = torch.cat([out[1, :, :lengths[1]], pool.close(1)], dim=1)
    # the same pipeline with the zeros = 8 filter: a one-row StreamResampler in one push plus close is that sum
    def rs(sig, a, b):
        r = resample.StreamResampler(sig.shape[0], a, b, 1 << 20, zeros=8, device=DEV)
        for row in range(sig.shape[0]):
            r.open(row)
        y, n = r.push(sig, [sig.shape[1]] * sig.shape[0])
        return torch.cat([y, torch.stack([r.close(row) for row in range(sig.shape[0])])], dim=1)
    x8 = rs(x[None].to(DEV), 16000, 8000)[0]
    s = FusedStreamingSeparator(m, batch=1, max_chunk_frames=64)
    y8 = torch.cat([s.push(x8[None]), s.flush()], dim=2)[0].contiguous()
    assert x8.shape[0] == 1000 and torch.equal(got, rs(y8, 8000, 16000))
    with pytest.raises(ValueError):
        pool.push(chunk.to(DEV), [0, 5])                        # slot 1 is closed
    with pytest.raises(ValueError):
        pool.close(1)
    with pytest.raises(ValueError):
        pool.push(chunk.to(DEV), [0])
    pool.open(0)
    with pytest.raises(ValueError):
        pool.push(chunk, [5, 0])                                # a CPU tensor
    with pytest.raises(ValueError):
        ResamplingStreamPool(m, slots=2, input_rate=0)
    assert pool.close(0).shape == (C, 0)


def test_separate_on_files_at_another_rate(tmp_path):
    from scipy.io import wavfile
    from conv_tasnet_amd.separate import separate
    torch.manual_seed(0)
    m = ctn.ConvTasNet(32, 20, 16, 32, 3, 2, 1, 2)
    path = str(tmp_path / "m.pth.tar")
    torch.save(ctn.ConvTasNet.serialize(m, torch.optim.Adam(m.parameters()), 1), path)
    mixdir = tmp_path / "mix"
    mixdir.mkdir()
    mix, _, _ = O.synth_batch(0, 3, 6001)
    lens = {"one": 6001, "two": 4444, "six": 2999}
    for i, (name, n) in enumerate(lens.items()):
        wavfile.write(str(mixdir / (name + ".wav")), 16000, mix[i, :n].numpy())
    out = tmp_path / "out"
    separate(path, str(mixdir), None, str(out), 1, 8000, 3, file_rate=16000)
    assert sorted(os.listdir(out)) == sorted(n + s + ".wav" for n in lens for s in ("", "_s1", "_s2"))
    # the offline pipeline: every file resampled on its own, one zero-padded batch (longest first), the estimates resampled back
    order = sorted(lens, key=lambda n: -lens[n])
    m = m.to(DEV).eval()
    low = [resample.resample(mix[list(lens).index(n), :lens[n]].to(DEV), 16000, 8000) for n in order]
    batch = torch.zeros((3, low[0].shape[0]), device=DEV)
    for i, x in enumerate(low):
        batch[i, :x.shape[0]] = x
    with torch.no_grad():
        est = m(batch)
    for i, n in enumerate(order):
        sr, x = wavfile.read(str(out / (n + ".wav")))
        assert sr == 16000 and np.array_equal(x, mix[list(lens).index(n), :lens[n]].numpy())
        want = resample.resample(est[i, :, :low[i].shape[0]].contiguous(), 8000, 16000)[:, :lens[n]].cpu().numpy()
        for c in range(2):
            sr, y = wavfile.read(str(out / ("%s_s%d.wav" % (n, c + 1))))
            assert sr == 16000 and y.dtype == np.float32 and y.shape == (lens[n],)
            assert np.array_equal(y.view(np.uint32), want[c].view(np.uint32)), (n, c)
    # a file at another rate raises, and names it
    wavfile.write(str(mixdir / "odd.wav"), 44100, mix[0, :3000].numpy())
    with pytest.raises(ValueError, match="odd.wav"):
        separate(path, str(mixdir), None, str(tmp_path / "out2"), 1, 8000, 3, file_rate=16000)


def test_separate_default_call_is_unchanged(tmp_path):
    from scipy.io import wavfile
    from conv_tasnet_amd.separate import separate
    torch.manual_seed(0)
    m = ctn.ConvTasNet(32, 20, 16, 32, 3, 2, 1, 2)
    path = str(tmp_path / "m.pth.tar")
    torch.save(ctn.ConvTasNet.serialize(m, torch.optim.Adam(m.parameters()), 1), path)
    mixdir = tmp_path / "mix"
    mixdir.mkdir()
    mix, _, _ = O.synth_batch(0, 2, 4000)
    wavfile.write(str(mixdir / "long.wav"), 8000, mix[0].numpy())
    wavfile.write(str(mixdir / "short.wav"), 8000, mix[1, :3000].numpy())
    separate(path, str(mixdir), None, str(tmp_path / "a"), 1, 8000, 2)
    separate(path, str(mixdir), None, str(tmp_path / "b"), 1, 8000, 2, file_rate=None)
    separate(path, str(mixdir), None, str(tmp_path / "c"), 1, 8000, 2, file_rate=8000)
    with torch.no_grad():
        padded = mix.clone()
        padded[1, 3000:] = 0
        ref = m.to(DEV)(padded.to(DEV))
    for i, (name, n) in enumerate((("long", 4000), ("short", 3000))):
        for c in range(2):
            f = "%s_s%d.wav" % (name, c + 1)
            sr, y = wavfile.read(str(tmp_path / "a" / f))
            assert sr == 8000 and y.shape == (n,)
            np.testing.assert_allclose(y, ref[i, c, :n].cpu().numpy(), atol=1e-5)
            for other in ("b", "c"):
                assert np.array_equal(y, wavfile.read(str(tmp_path / other / f))[1])
