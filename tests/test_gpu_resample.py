"""GPU: the sinc resampler (csrc/ctn_resample.hip, resample.py) against the host restatement in resample_oracle.py -- ragged
rows BITWISE equal to the sequential float32 sum, within the rounding bound of the float64 sum, rows isolated from their
neighbours, bad row tables refused, and a corpus built from utterances at several rates."""
import json

import numpy as np
import pytest
import torch

import dynmix_oracle as DO
import resample_oracle as RO

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import resample  # noqa: E402

DEV = "cuda:0"
RATIOS = [(1, 2), (2, 1), (80, 441), (100, 103)]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _ragged_case(up, down, seed):
    """Rows of 1, 2W - 1, 2W, 1023, 1024, 1025, 4097 and 8000 samples (the last two cross a workgroup's 1024 outputs at every
    ratio here) in one flat buffer whose gaps and both ends hold NaN; the output buffer is laid out the same way."""
    h, W = resample.design_filter(up, down)
    rng = np.random.RandomState(seed)
    lens = np.array([1, 2 * W - 1, 2 * W, 1023, 1024, 1025, 4097, 8000], dtype=np.int64)
    gaps = rng.randint(1, 40, size=len(lens) + 1)
    rows = [(rng.randn(n) * rng.uniform(0.05, 1.0)).astype(np.float32) for n in lens]
    out_lens = np.array([RO.out_len(n, up, down) for n in lens], dtype=np.int64)
    assert out_lens.max() > 1024

    def layout(ns):
        offs, at = [], int(gaps[0])
        for n, g in zip(ns, gaps[1:]):
            offs.append(at)
            at += int(n) + int(g)
        return np.array(offs, dtype=np.int64), at

    in_offsets, n_x = layout(lens)
    out_offsets, n_y = layout(out_lens)
    x = np.full(n_x, np.nan, dtype=np.float32)
    for o, r in zip(in_offsets, rows):
        x[o:o + len(r)] = r
    return h, W, rows, lens, in_offsets, x, out_lens, out_offsets, n_y


@pytest.mark.parametrize("up,down", RATIOS)
def test_ragged_rows_are_bitwise_the_oracle_and_never_read_their_neighbours(up, down):
    h, W, rows, lens, in_offsets, x, out_lens, out_offsets, n_y = _ragged_case(up, down, 7 + up)
    xd = torch.from_numpy(x).to(DEV)
    yd = torch.full((n_y,), float("nan"), dtype=torch.float32, device=DEV)
    got_lens = resample.resample_rows(xd, in_offsets, lens, up, down, yd, out_offsets)
    y = yd.cpu().numpy()
    assert np.array_equal(got_lens, out_lens)
    written = np.zeros(n_y, dtype=bool)
    worst = 0.0
    for r, o, n in zip(rows, out_offsets, out_lens):
        got = y[o:o + n]
        assert np.isfinite(got).all(), "a row read NaN from beyond its ends"
        want = RO.resample_f32(r, up, down, h, W)
        assert want.shape == got.shape
        bad = int((_bits(got) != _bits(want)).sum())
        assert bad == 0, "row of %d samples: %d of %d outputs differ in their bits" % (len(r), bad, n)
        y64 = RO.resample_f64(r, up, down, h, W)
        bound = (2 * W + 2) * 2.0 ** -24 * RO.tap_abs_sum(r, up, down, h, W)
        err = np.abs(got.astype(np.float64) - y64)
        assert np.all(err <= bound)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        written[o:o + n] = True
    assert np.isnan(y[~written]).all(), "the kernel wrote outside its rows"
    print("%d/%d: worst error / rounding bound = %.3f" % (up, down, worst))


def test_resample_of_a_batch_and_the_packed_ragged_form():
    rng = np.random.RandomState(1)
    x = rng.randn(2, 3, 2500).astype(np.float32)
    y = resample.resample(torch.from_numpy(x).to(DEV), 16000, 8000)
    h, W = resample.design_filter(1, 2)
    assert y.shape == (2, 3, 1250) and y.dtype == torch.float32 and y.device == torch.device(DEV)
    for a in range(2):
        for b in range(3):
            assert np.array_equal(_bits(y[a, b].cpu().numpy()), _bits(RO.resample_f32(x[a, b], 1, 2, h, W)))
    same = resample.resample(torch.from_numpy(x).to(DEV), 8000, 8000)
    assert np.array_equal(same.cpu().numpy(), x)
    flat = torch.from_numpy(x.reshape(-1)).to(DEV)
    out, offs, lens = resample.resample_ragged(flat, [2500, 0, 10000], [2500, 700, 333], 8000, 44100)
    h, W = resample.design_filter(441, 80)
    assert list(lens) == [RO.out_len(n, 441, 80) for n in (2500, 700, 333)] and list(offs) == [0, lens[0], lens[0] + lens[1]]
    got = out.cpu().numpy()
    for o, n, (i0, ni) in zip(offs, lens, ((2500, 2500), (0, 700), (10000, 333))):
        want = RO.resample_f32(x.reshape(-1)[i0:i0 + ni], 441, 80, h, W)
        assert np.array_equal(_bits(got[o:o + n]), _bits(want))


def test_a_row_table_outside_the_buffers_is_refused_before_the_launch_and_flagged_in_the_kernel():
    """Not a fault test: the host checks its copy of the tables before it launches, and the kernel checks the device copy
    before it forms an address."""
    h, W = resample.device_filter(1, 2, DEV)
    x = torch.ones(1000, device=DEV)
    y = torch.full((600,), -7.0, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(host, dev, status=0):
        host = np.ascontiguousarray(np.array(host, dtype=np.int64))
        d = torch.from_numpy(np.ascontiguousarray(np.array(dev, dtype=np.int64))).to(DEV)
        rc = ctn.lib.ctn_resample_ragged(x.data_ptr(), x.numel(), d[0].data_ptr(), d[1].data_ptr(), host.shape[1], 1, 2, h.data_ptr(), W,
                                         y.data_ptr(), y.numel(), d[2].data_ptr(), d[3].data_ptr(), host.ctypes.data, status, stream)
        torch.cuda.synchronize()
        return rc

    good = [[0, 500], [500, 400], [0, 300], [250, 200]]
    for bad in ([[0, 700], [500, 400], [0, 300], [250, 200]],           # 700 + 400 > 1000
                [[0, -4], [500, 400], [0, 300], [250, 200]],
                [[0, 500], [500, 400], [0, 450], [250, 200]],           # 450 + 200 > 600
                [[0, 500], [500, 400], [0, 300], [250, 201]]):          # not ceil(400 / 2)
        assert call(bad, bad) == -1 and b"ctn_resample_ragged" in ctn.lib.ctn_last_error()
        assert bool((y == -7.0).all()), "something was launched"
    # the host copy is fine, the device copy is not: row 1 is flagged and neither read nor written
    status = torch.full((2,), 5, dtype=torch.int32, device=DEV)
    assert call(good, [[0, 700], [500, 400], [0, 300], [250, 200]], status.data_ptr()) == 0
    assert status.tolist() == [0, -1]
    got = y.cpu().numpy()
    assert np.all(got[300:] == -7.0) and np.all(got[:250] != -7.0) and np.all(got[250:300] == -7.0)
    with pytest.raises(ctn.CtnError, match="outside the input buffer"):
        resample.resample_rows(x, [900], [200], 1, 2, y, [0])


def _mixed_rate_world():
    rng = np.random.RandomState(5)
    rates = [16000, 8000, 16000, 44100, 8000, 48000, 16000, 8000]
    arrays = [(rng.randn(int(rng.randint(r // 4, r))) * rng.uniform(0.05, 0.3)).astype(np.float32) for r in rates]
    speakers = ["s%d" % (u % 3) for u in range(len(rates))]
    want, lens = [], []
    for x, r in zip(arrays, rates):
        if r == 8000:
            want.append(x)
        else:
            up, down = resample.ratio(r, 8000)
            h, W = resample.design_filter(up, down)
            want.append(RO.resample_f32(x, up, down, h, W))
        lens.append(len(want[-1]))
    return arrays, speakers, rates, np.concatenate(want), np.array(lens, dtype=np.int64)


def test_corpus_from_arrays_at_several_rates_is_the_oracles_corpus():
    arrays, speakers, rates, want, lens = _mixed_rate_world()
    corpus = ctn.DeviceCorpus.from_arrays(arrays, speakers, DEV, sample_rates=rates, target_rate=8000)
    assert np.array_equal(corpus.lens_host, lens) and corpus.num_samples == want.size
    offsets = np.concatenate(([0], np.cumsum(lens)[:-1]))
    assert np.array_equal(corpus.offsets_host, offsets) and np.array_equal(corpus.offsets.cpu().numpy(), offsets)
    assert np.array_equal(_bits(corpus.corpus.cpu().numpy()), _bits(want))
    msq = DO.meansq(want, offsets, lens)
    for u, n in enumerate(lens):                                 # the levels are those of the RESAMPLED audio
        assert abs(corpus.meansq[u] - msq[u]) / msq[u] <= 2.0 * (int(n) + 1) * 2.0 ** -53, u
    # every utterance already at the target rate: the plain corpus
    plain = ctn.DeviceCorpus.from_arrays(arrays[:2], speakers[:2], DEV)
    same = ctn.DeviceCorpus.from_arrays(arrays[:2], speakers[:2], DEV, sample_rates=[8000, 8000], target_rate=8000)
    assert torch.equal(plain.corpus, same.corpus) and np.array_equal(plain.meansq, same.meansq)
    with pytest.raises(ValueError):
        ctn.DeviceCorpus.from_arrays(arrays, speakers, DEV, sample_rates=rates)
    with pytest.raises(ValueError):
        ctn.DeviceCorpus.from_arrays(arrays, speakers, DEV, sample_rates=rates[:-1], target_rate=8000)


def test_from_manifest_resamples_files_at_other_rates(tmp_path):
    from scipy.io import wavfile
    rng = np.random.RandomState(2)
    infos, arrays, rates = [], [], []
    for k, (spk, sr) in enumerate((("a", 16000), ("b", 8000), ("a", 8000), ("b", 16000))):
        x = (rng.randn(3000 + 101 * k) * 3000).astype(np.int16)
        p = str(tmp_path / ("%d.wav" % k))
        wavfile.write(p, sr, x)
        infos.append([p, len(x), spk])                           # n_samples counts the file's samples
        arrays.append(x.astype(np.float32) / 32768.0)
        rates.append(sr)
    (tmp_path / "m.json").write_text(json.dumps(infos))
    with pytest.raises(ValueError, match="expected 8000"):
        ctn.DeviceCorpus.from_manifest(str(tmp_path / "m.json"), 8000, DEV)
    corpus = ctn.DeviceCorpus.from_manifest(str(tmp_path / "m.json"), 8000, DEV, resample=True)
    ref = ctn.DeviceCorpus.from_arrays(arrays, [i[2] for i in infos], DEV, sample_rates=rates, target_rate=8000)
    assert torch.equal(corpus.corpus, ref.corpus) and np.array_equal(corpus.lens_host, ref.lens_host)
    assert list(corpus.lens_host) == [1500, 3101, 3202, 1652] and np.array_equal(corpus.meansq, ref.meansq)
    infos[0][1] = 1500
    (tmp_path / "bad.json").write_text(json.dumps(infos))
    with pytest.raises(ValueError, match="manifest"):
        ctn.DeviceCorpus.from_manifest(str(tmp_path / "bad.json"), 8000, DEV, resample=True)
