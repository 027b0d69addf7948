"""CPU-only checks of the sinc resampling: the package's filter design against the oracle's, the design's own quality
(passband, aliasing, DC) through the float64 restatement, lengths, the host-side arithmetic of the speed perturbation, the
argument checks that sit in front of every launch, and the paths that must not change."""
import json
import math

import numpy as np
import pytest
import torch

import dynmix_oracle as DO
import resample_oracle as RO

import conv_tasnet_amd as ctn
from conv_tasnet_amd import _lib, dynmix, resample

SPEED_RATIOS = [RO.speed_ratio(p) for p in range(95, 106) if p != 100] + [(1, 1)]
RATIOS = [(1, 2), (2, 1), (80, 441), (1, 6)] + SPEED_RATIOS
DOWN = [(1, 2), (80, 441), (1, 6)]
ENTRY_POINTS = ["ctn_resample_span", "ctn_resample_ragged", "ctn_dynmix_plan_speed", "ctn_dynmix_speed_segments"]


@pytest.fixture(scope="module")
def filters():
    return {r: RO.design_filter(*r) for r in RATIOS}


@pytest.mark.parametrize("up,down", RATIOS)
def test_table_equals_the_oracle_within_one_ulp_and_keeps_dc(filters, up, down):
    h, W = resample.design_filter(up, down)
    want, wW = filters[(up, down)]
    fc = 0.95 * min(1.0, up / down)
    assert W == wW == int(math.ceil(32 / fc)) and h.shape == want.shape == (up, 2 * W) and h.dtype == np.float32
    ulp = np.spacing(np.abs(want))
    assert np.all(np.abs(h.astype(np.float64) - want.astype(np.float64)) <= ulp)
    sums = h.astype(np.float64).sum(axis=1)
    assert np.all(np.abs(sums - 1.0) <= 2.0 ** -22), float(np.abs(sums - 1.0).max())
    # tau = 0 is tap W - 1 of phase 0: the centre tap is the largest, and the phase is symmetric about it
    assert int(np.argmax(h[0])) == W - 1 and np.array_equal(h[0, :W - 1], h[0, W:2 * W - 1][::-1])


def test_tap_counts_and_table_sizes():
    taps = {r: 2 * RO.design_filter(*r)[1] for r in [(1, 2), (80, 441)] + SPEED_RATIOS[:-1]}
    assert taps[(1, 2)] == 136 and taps[(80, 441)] == 372
    assert all(68 <= taps[r] <= 72 for r in SPEED_RATIOS[:-1])
    assert max(r[0] * taps[r] * 4 for r in SPEED_RATIOS[:-1]) <= 28 * 1024 and 80 * 372 * 4 < 117 * 1024


def test_lengths():
    for n in (1, 2, 7, 1023, 1024, 1025, 4097, 31999):
        for up, down in RATIOS:
            want = int(math.ceil(n * up / down - 1e-9))
            assert resample.out_len(n, up, down) == RO.out_len(n, up, down) == want, (n, up, down)
    assert resample.ratio(16000, 8000) == (1, 2) and resample.ratio(8000, 16000) == (2, 1)
    assert resample.ratio(44100, 8000) == (80, 441) and resample.ratio(48000, 8000) == (1, 6) and resample.ratio(8000, 8000) == (1, 1)
    x = np.ones(10, dtype=np.float32)
    h, W = RO.design_filter(2, 1)
    assert RO.resample_f32(x, 2, 1, h, W).shape == (20,) and RO.resample_f64(x, 1, 2, *RO.design_filter(1, 2)).shape == (5,)


def _interior(n_in, n_out, up, down, W):
    i = np.arange(n_out, dtype=np.int64) * down // up
    return (i - W + 1 >= 0) & (i + W <= n_in - 1)


@pytest.mark.parametrize("up,down", RATIOS)
def test_passband_sinusoids_are_reproduced_to_1e_6(filters, up, down):
    """A sinusoid at or below 0.85 fc (fc in units of the input Nyquist frequency) comes out at its own samples."""
    h, W = filters[(up, down)]
    fc = 0.95 * min(1.0, up / down)
    n_in = 8 * W + 600
    n_out = RO.out_len(n_in, up, down)
    keep = _interior(n_in, n_out, up, down, W)
    assert keep.sum() >= 100
    worst = 0.0
    for frac in (0.0, 0.03, 0.4, 0.85):
        f = frac * fc / 2.0                                     # cycles per input sample
        x = np.sin(2 * np.pi * f * np.arange(n_in) + 0.3)
        y = RO.resample_f64(x, up, down, h, W)
        ref = np.sin(2 * np.pi * f * (np.arange(n_out) * down / up) + 0.3)
        worst = max(worst, float(np.abs(y - ref)[keep].max()))
    print("passband %d/%d: worst error %.3e" % (up, down, worst))
    assert worst <= 1e-6


@pytest.mark.parametrize("up,down", DOWN)
def test_tones_that_would_alias_into_the_passband_leave_1e_6(filters, up, down):
    """An input tone between sr_out - 0.85 fc and the input Nyquist frequency would fold onto [0, 0.85 fc]: it is removed."""
    h, W = filters[(up, down)]
    fc = 0.95 * up / down
    lo = 2.0 * up / down - 0.85 * fc                            # in units of the input Nyquist frequency
    n_in = 8 * W + 1200
    n_out = RO.out_len(n_in, up, down)
    keep = _interior(n_in, n_out, up, down, W)
    assert keep.sum() >= 100 and lo < 1.0
    worst = 0.0
    for f in (lo, 0.5 * (lo + 1.0), 0.25 * lo + 0.75, 0.999):
        x = np.sin(np.pi * f * np.arange(n_in) + 0.3)
        y = RO.resample_f64(x, up, down, h, W)
        worst = max(worst, float(np.abs(y)[keep].max()))
    print("alias %d/%d: worst residue %.3e" % (up, down, worst))
    assert worst <= 1e-6


def test_sequential_float32_sum_stays_within_its_rounding_bound(filters):
    rng = np.random.RandomState(0)
    x = rng.randn(3000).astype(np.float32)
    for r in [(1, 2), (2, 1), (100, 103)]:
        h, W = filters[r]
        y32, y64 = RO.resample_f32(x, *r, h, W), RO.resample_f64(x, *r, h, W)
        bound = (2 * W + 2) * 2.0 ** -24 * RO.tap_abs_sum(x, *r, h, W)
        assert y32.dtype == np.float32 and np.all(np.abs(y32.astype(np.float64) - y64) <= bound)
        # a row is its own world: zeros beyond both ends
        first = float(np.dot(h[0, W - 1:].astype(np.float64), x[:W + 1].astype(np.float64)))
        assert abs(y64[0] - first) <= 1e-12


def test_speed_arithmetic():
    assert resample.speed_ratio(100) == (1, 1) and resample.speed_ratio(95) == (20, 19) and resample.speed_ratio(103) == (100, 103)
    assert resample.speed_ratio(50) == (2, 1) and resample.speed_ratio(200) == (1, 2) and resample.speed_ratio(96) == (25, 24)
    for p in range(50, 201):
        up, down = resample.speed_ratio(p)
        assert math.gcd(up, down) == 1 and up * p == down * 100 and (up, down) == RO.speed_ratio(p)
    for T in (1, 63, 4000, 4001, 32000):
        for p in (50, 95, 100, 103, 105, 200):
            assert resample.need(T, p) == RO.need(T, p) == -((-T * p) // 100)
            # the last tap centre of a segment lies inside the need() samples
            up, down = resample.speed_ratio(p)
            assert (T - 1) * down // up <= resample.need(T, p) - 1
    assert resample.need(4001, 103) == 4122 and resample.need(63, 95) == 60 and resample.need(1, 105) == 2
    assert resample.eligible_len(32000, (95, 100, 105)) == 33600 and resample.eligible_len(4001, (100,)) == 4001
    assert resample.span(100, 103, 35) == (99 + 1023 * 103) // 100 + 70
    assert ctn.lib.ctn_resample_span(100, 103, 35, 1024) == resample.span(100, 103, 35)
    assert ctn.lib.ctn_resample_span(1, 2, 68, 1024) == 1023 * 2 + 136 and ctn.lib.ctn_resample_span(0, 1, 3, 1024) == 0


def test_speeds_argument():
    assert resample.parse_speeds(None) is None                   # speeds=None: the loader never enters the new code
    assert resample.parse_speeds([105, 95, 100, 95]) == (95, 100, 105) and resample.parse_speeds(range(95, 106)) == tuple(range(95, 106))
    for bad in ([], [49], [201], [99.5], [True], [100, 300]):
        with pytest.raises(ValueError):
            resample.parse_speeds(bad)
    assert resample.parse_speed_range("95:105") == tuple(range(95, 106)) and resample.parse_speed_range("100:100") == (100,)
    for bad in ("95", "105:95", "a:b", "40:60", "95:105:2"):
        with pytest.raises(ValueError):
            resample.parse_speed_range(bad)
    with pytest.raises(ValueError):
        resample.design_filter(2, 4)
    with pytest.raises(ValueError):
        resample.design_filter(0, 1)
    with pytest.raises(ValueError):
        resample.ratio(0, 8000)


def test_plan_speed_oracle_keeps_the_draws_of_the_plain_plan():
    rng = np.random.RandomState(3)
    lens = rng.randint(300, 900, size=40)
    msq = rng.uniform(1e-3, 1e-1, size=40)
    spk = ["s%d" % (u % 8) for u in range(40)]
    T, speeds = 200, tuple(range(95, 106))
    tb = dynmix.build_tables(lens, msq, spk, resample.eligible_len(T, speeds), 3)
    seen = set()
    for step in range(6):
        utt, start, q, gain, pct = RO.plan_speed(77, 1, 2, step, 16, 3, T, tb, speeds)
        p_utt, p_start, p_q, p_gain = DO.plan(77, 1, 2, step, 16, 3, resample.eligible_len(T, speeds), tb)
        assert np.array_equal(utt, p_utt) and np.array_equal(q, p_q) and np.array_equal(gain, p_gain)
        assert np.all(start >= 0) and np.all(start + (T * pct + 99) // 100 <= lens[utt])
        seen.update(int(p) for p in pct.reshape(-1))
        same = RO.plan_speed(77, 1, 2, step, 16, 3, T, tb, (100,))
        plain = DO.plan(77, 1, 2, step, 16, 3, T, tb)
        assert all(np.array_equal(a, b) for a, b in zip(same[:4], plain)) and np.all(same[4] == 100)
    assert seen == set(speeds)                                   # 288 draws over 11 percents


def test_speed_segments_oracle_on_a_toy_case():
    x = np.arange(1, 41, dtype=np.float32)
    seg = RO.speed_segments(x, [0, 10], [10, 30], np.array([[1, 0]], np.int32), np.array([[5, 2]], np.int64),
                            np.array([[100, 100]], np.int32), 8)
    assert np.array_equal(seg[0, 0], x[15:23]) and np.array_equal(seg[0, 1], x[2:10])
    seg = RO.speed_segments(x, [0, 10], [10, 30], np.array([[1, 1]], np.int32), np.array([[0, 22]], np.int64),
                            np.array([[50, 200]], np.int32), 4)
    h, W = RO.design_filter(2, 1)
    assert np.array_equal(seg[0, 0], RO.resample_f32(x[10:], 2, 1, h, W)[:4])
    h, W = RO.design_filter(1, 2)
    assert np.array_equal(seg[0, 1], RO.resample_f32(x[10:], 1, 2, h, W)[11:15])


def test_cpu_tensors_and_bad_arguments_are_refused():
    with pytest.raises(ValueError, match="GPU"):
        resample.resample(torch.zeros(100), 16000, 8000)
    with pytest.raises(ValueError, match="GPU"):
        resample.resample_ragged(torch.zeros(100), [0], [100], 16000, 8000)
    with pytest.raises(ValueError, match="GPU"):
        dynmix.DeviceCorpus.from_arrays([np.ones(10, np.float32)], ["a"], "cpu", sample_rates=[16000], target_rate=8000)


def test_library_symbols_and_argument_checks_in_front_of_every_launch():
    protos = _lib.parse_header()
    assert not [n for n in ENTRY_POINTS if n not in protos]
    lib, err = ctn.lib, ctn.lib.ctn_last_error
    p = 4096                                                     # fake non-null device pointers: never read

    def ragged(tables, x=p, up=1, down=2, W=68, xs=1000, ys=1000, U=None):
        host = np.ascontiguousarray(np.array(tables, dtype=np.int64))
        return lib.ctn_resample_ragged(x, xs, p, p, host.shape[1] if U is None else U, up, down, p, W, p, ys, p, p, host.ctypes.data, 0, 0)

    good = [[0, 100], [100, 50], [0, 50], [50, 25]]              # in_offsets, in_lens, out_offsets, out_lens
    assert ragged(good, x=0) == -1 and b"null" in err()
    assert ragged(good, U=0) == -1 and b"rows" in err()
    assert ragged(good, up=2, down=4) == -1 and b"lowest terms" in err()
    assert ragged(good, up=0) == -1 and b"ratio" in err()
    assert ragged(good, W=0) == -1 and b"W =" in err()
    assert ragged([[0, 960], [100, 50], [0, 50], [50, 25]]) == -1 and b"outside the input buffer" in err()
    assert ragged([[-1, 100], [100, 50], [0, 50], [50, 25]]) == -1 and b"outside the input buffer" in err()
    assert ragged([[0, 100], [100, 50], [0, 980], [50, 25]]) == -1 and b"outside the output buffer" in err()
    assert ragged([[0, 100], [100, 50], [0, 50], [50, 26]]) == -1 and b"expected" in err()
    assert ragged([[0, 100], [100, 0], [0, 50], [50, 0]]) == -1 and b"samples" in err()
    assert ragged([[0], [100], [0], [1]], up=1, down=1 << 19, W=1 << 16) == -1 and b"does not fit" in err()

    def plan(n=3, pct=p, C=2, plan_pct=p):
        return lib.ctn_dynmix_plan_speed(p, p, 8, p, p, p, pct, n, 0, 0, 0, p, 8, C, 100, p, p, p, p, plan_pct, 0)

    assert plan(n=0) == -1 and b"speed percents" in err()
    assert plan(n=152) == -1 and b"speed percents" in err()
    assert plan(pct=0) == -1 and b"null" in err()
    assert plan(plan_pct=0) == -1 and b"null" in err()
    assert plan(C=5) == -1 and b"sources per mixture" in err()

    def segments(B=8, C=2, T=100, banks=p, span_cap=2000, bank_cap=8000, seg_utt=p):
        return lib.ctn_dynmix_speed_segments(p, p, p, 4, p, p, p, B, C, T, banks, 100, p, span_cap, bank_cap, p, seg_utt, 0)

    assert segments(banks=0) == -1 and b"null" in err()
    assert segments(seg_utt=0) == -1 and b"null" in err()
    assert segments(C=1) == -1 and b"sources per mixture" in err()
    assert segments(T=0) == -1 and b"seg_len" in err()
    assert segments(B=40000) == -1 and b"mixtures" in err()
    assert segments(span_cap=0) == -1 and b"LDS" in err()
    assert segments(span_cap=8000, bank_cap=8000) == -1 and b"LDS" in err()


def test_train_parser_has_the_new_flags_and_keeps_the_defaults():
    from conv_tasnet_amd.train import build_parser
    a = build_parser().parse_args([])
    assert a.speed_perturb is None and a.corpus_rate == "8000" and a.segment_len == 32000 and not a.tiny
    a = build_parser().parse_args(["--dynamic-mix", "tr.json", "--speed-perturb", "95:105", "--corpus-rate", "auto"])
    assert (a.speed_perturb, a.corpus_rate) == ("95:105", "auto")


def test_from_manifest_without_resample_still_refuses_a_16_khz_file(tmp_path):
    from scipy.io import wavfile
    from conv_tasnet_amd.data import read_wav, read_wav_native
    x = (np.random.RandomState(0).randn(3000) * 3000).astype(np.int16)
    path = str(tmp_path / "a.wav")
    wavfile.write(path, 16000, x)
    (tmp_path / "m.json").write_text(json.dumps([[path, 3000, "a"]]))
    with pytest.raises(ValueError, match="expected 8000"):
        ctn.DeviceCorpus.from_manifest(str(tmp_path / "m.json"), 8000, "cuda:0")
    with pytest.raises(ValueError, match="expected 8000"):
        read_wav(path, 8000)
    y, sr = read_wav_native(path)
    assert sr == 16000 and y.dtype == np.float32 and np.array_equal(y, x.astype(np.float32) / 32768.0)
    assert np.array_equal(read_wav(path, 16000), y)
