"""GPU: resample.StreamResampler (ctn_stream_resample) -- rows that are opened, fed in ragged pushes and closed on their own
lives.  The yardstick is resample_oracle.resample_f32 of each row's WHOLE signal; every comparison is bitwise."""
import numpy as np
import pytest
import torch

import resample_oracle as RO

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import resample  # noqa: E402

DEV = "cuda:0"
RATIOS = [(1, 2), (2, 1), (80, 441), (100, 103), (1, 6)]
MAX_CHUNK = 1000
_RUNS = {}


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _streams(up, down, W, seed):
    """(row, push at which it opens, cuts, signal): six rows whose last occupants hold 1, W, 2W - 1, 2W, ceil(1025 * down / up)
    and 3001 samples.  Row 0's first stream ends with N = 1 < W (all of its output is flush); then a stream that is closed
    right after `open`.  Row 1 first serves a signal scaled by 100 that is closed in the middle of the run, then the W-sample
    stream in three pushes shorter than W.  Pushes of 0, 1, W and W + 1 samples; 2500 > MAX_CHUNK is split inside."""
    rng = np.random.RandomState(seed)
    big = -((-1025 * down) // up)

    def sig(n, scale=1.0):
        return (rng.randn(n) * 0.3 * scale).astype(np.float32)
    return [(0, 0, [0, 1], sig(1)),
            (0, 3, [], sig(0)),
            (1, 0, [50, 0, 100], sig(150, 100.0)),
            (1, 4, [2, 1, W - 3], sig(W)),
            (2, 1, [W, W - 1], sig(2 * W - 1)),
            (3, 0, [W + 1, W - 1], sig(2 * W)),
            (4, 2, [big], sig(big)),
            (5, 0, [1, 5, 7, 2500, 0, 488], sig(3001))]


def _drive(r, streams, rows, reps=1):
    """Run the schedule; `reps` consecutive rows carry each stream (the group form).  -> per stream [reps, n] numpy."""
    got = [[] for _ in streams]
    n_push = max(o + max(len(c), 1) for _, o, c, _ in streams)
    at = [0] * len(streams)
    for p in range(n_push):
        counts, live = [0] * rows, {}
        for k, (row, opens, cuts, x) in enumerate(streams):
            if p == opens:
                assert r.open(row) == row
            if opens <= p < opens + len(cuts):
                counts[row], live[row] = cuts[p - opens], k
        chunk = np.full((rows * reps, max(counts) + 3), np.nan, dtype=np.float32)     # NaN beyond every count and in idle rows
        for row, k in live.items():
            x = streams[k][3]
            chunk[row * reps:(row + 1) * reps, :counts[row]] = x[at[k]:at[k] + counts[row]]
            at[k] += counts[row]
        y, lengths = r.push(torch.from_numpy(chunk).to(DEV), counts)
        assert y.shape == (rows * reps, max(lengths)) and len(lengths) == rows
        y = y.cpu().numpy()
        assert np.isfinite(y).all(), "a row read NaN from beyond its count"
        for row in range(rows):
            assert not y[row * reps:(row + 1) * reps, lengths[row]:].any()              # zeros beyond each row's length
            if row not in live:
                assert lengths[row] == 0
        for row, k in live.items():
            got[k].append(y[row * reps:(row + 1) * reps, :lengths[row]])
        for k, (row, opens, cuts, x) in enumerate(streams):
            if p == opens + max(len(cuts), 1) - 1:
                tail = r.close(row).cpu().numpy().reshape(reps, -1)
                assert np.isfinite(tail).all()
                got[k].append(tail)
    assert at == [len(s[3]) for s in streams]
    return [np.concatenate(g, axis=1) for g in got]


def _run(up, down, zeros):
    key = (up, down, zeros)
    if key not in _RUNS:
        h, W = RO.design_filter(up, down, zeros=zeros)
        streams = _streams(up, down, W, 11 + up + zeros)
        r = resample.StreamResampler(6, down, up, MAX_CHUNK, zeros=zeros, device=DEV)
        assert r.W == W
        _RUNS[key] = (h, W, streams, _drive(r, streams, 6))
    return _RUNS[key]


def _check_against_the_oracle(up, down, zeros):
    h, W, streams, got = _run(up, down, zeros)
    assert [len(s[3]) for s in streams if s[0] != 0 and s[2] != [50, 0, 100]] == [W, 2 * W - 1, 2 * W, -((-1025 * down) // up), 3001]
    for (row, _, cuts, x), y in zip(streams, got):
        want = RO.resample_f32(x, up, down, h, W) if len(x) else np.zeros(0, np.float32)
        assert y.shape == (1, len(want)), (row, len(x))
        bad = int((_bits(y[0]) != _bits(want)).sum())
        assert bad == 0, "row %d, stream of %d samples: %d of %d outputs differ in their bits" % (row, len(x), bad, len(want))


@pytest.mark.parametrize("up,down", RATIOS)
def test_ragged_streams_are_bitwise_the_oracle_of_the_whole_signal(up, down):
    _check_against_the_oracle(up, down, 32)


@pytest.mark.parametrize("up,down", RATIOS)
def test_the_same_streams_with_zeros_8(up, down):
    _check_against_the_oracle(up, down, 8)


@pytest.mark.parametrize("up,down", RATIOS)
def test_every_row_equals_its_stream_pushed_alone(up, down):
    """One push plus close on a 1-row resampler whose max_chunk exceeds every stream: the 3001-sample row (and at 2 / 1 the
    1025 * down / up one with its flush) spreads over several workgroups of one launch there."""
    h, W, streams, got = _run(up, down, 32)
    for (row, _, cuts, x), y in zip(streams, got):
        alone = resample.StreamResampler(1, down, up, 1 << 20, device=DEV)
        alone.open(0)
        parts = []
        if len(x):
            out, lengths = alone.push(torch.from_numpy(x[None]).to(DEV), [len(x)])
            parts.append(out[0, :lengths[0]])
        parts.append(alone.close(0))
        assert torch.equal(torch.cat(parts).cpu(), torch.from_numpy(y[0])), (row, len(x))


@pytest.mark.parametrize("up,down", RATIOS)
def test_a_long_push_spreads_over_several_workgroups(up, down):
    """One row, one push that emits more than 2048 outputs in a single launch, against the oracle."""
    h, W = RO.design_filter(up, down)
    n = -((-2100 * down) // up) + W
    x = (np.random.RandomState(up).randn(n) * 0.3).astype(np.float32)
    r = resample.StreamResampler(1, down, up, n, device=DEV)
    r.open(0)
    out, lengths = r.push(torch.from_numpy(x[None]).to(DEV), [n])
    assert lengths[0] >= 2100
    got = torch.cat([out[0, :lengths[0]], r.close(0)]).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(RO.resample_f32(x, up, down, h, W)))


def test_the_rows_of_a_group_equal_single_rows():
    up, down, C = 2, 1, 3
    h, W = RO.design_filter(up, down)
    streams = [s for s in _streams(up, down, W, 5) if s[0] in (0, 1)]
    grouped = _drive(resample.StreamResampler(2 * C, down, up, MAX_CHUNK, groups=C, device=DEV), streams, 2, reps=C)
    single = _drive(resample.StreamResampler(2, down, up, MAX_CHUNK, device=DEV), streams, 2)
    for g, s in zip(grouped, single):
        assert g.shape == (C, s.shape[1])
        for c in range(C):
            assert np.array_equal(_bits(g[c]), _bits(s[0]))
    # the sources of a group are rows of their own: three different signals through one group
    r = resample.StreamResampler(C, down, up, MAX_CHUNK, groups=C, device=DEV)
    x = (np.random.RandomState(9).randn(C, 500) * 0.3).astype(np.float32)
    r.open(0)
    wide = torch.full((C, 700), float("nan"), device=DEV)           # the rows of a wider tensor are read in place
    wide[:, 100:600] = torch.from_numpy(x).to(DEV)
    out, lengths = r.push(wide[:, 100:600], [500])
    got = torch.cat([out[:, :lengths[0]], r.close(0)], dim=1).cpu().numpy()
    for c in range(C):
        assert np.array_equal(_bits(got[c]), _bits(RO.resample_f32(x[c], up, down, h, W)))


def test_equal_rates_pass_through():
    r = resample.StreamResampler(3, 8000, 8000, 100, device=DEV)
    x = np.random.RandomState(2).randn(3, 400).astype(np.float32)
    r.open(0)
    r.open(2)
    chunk = np.full((3, 260), np.nan, dtype=np.float32)
    chunk[0, :250], chunk[2, :7] = x[0, :250], x[2, :7]
    y, lengths = r.push(torch.from_numpy(chunk).to(DEV), [250, 0, 7])               # 250 > max_chunk: split inside
    assert lengths == [250, 0, 7] and y.shape == (3, 250)
    y = y.cpu().numpy()
    assert np.array_equal(y[0], x[0, :250]) and np.array_equal(y[2, :7], x[2, :7]) and not y[1].any() and not y[2, 7:].any()
    assert r.close(0).shape == (0,) and r.close(2).shape == (0,)


def test_a_table_outside_the_chunk_buffer_is_refused_and_the_neighbours_are_untouched():
    """Not a fault test: the host checks its copy of the table before it launches, and the kernel checks the device copy before
    it forms an address."""
    h, W = resample.device_filter(1, 2, DEV)
    rows, n = 3, 200
    n_out = resample.plan_stream_resample(0, n, 1, 2, W)[1]
    assert n_out > 0
    x = torch.ones(rows * n, device=DEV)
    hist = torch.zeros((2, rows, 2 * W - 1), device=DEV)
    y = torch.full((rows * 100,), -7.0, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    good = np.array([[0, n, 0, n_out, r * n, r * 100, 0, 0] for r in range(rows)], dtype=np.int64)
    bad = good.copy()
    bad[1, 4] = 500                                                  # 500 + 200 > 600

    def call(host, dev, status=0):
        d = torch.from_numpy(np.ascontiguousarray(dev)).to(DEV)
        host = np.ascontiguousarray(host)
        rc = ctn.lib.ctn_stream_resample(x.data_ptr(), x.numel(), hist.data_ptr(), rows, 1, 2, h.data_ptr(), W, y.data_ptr(), y.numel(),
                                         d.data_ptr(), host.ctypes.data, status, stream)
        torch.cuda.synchronize()
        return rc

    worse = good.copy()
    worse[2, 5] = 250                                                # 250 + n_out > 300
    early = good.copy()
    early[0, 0], early[0, 2] = 5000, 0                               # output 0 needs samples long gone from the history
    for table in (bad, worse, early):
        assert call(table, table) == -1 and b"ctn_stream_resample" in ctn.lib.ctn_last_error()
        assert bool((y == -7.0).all()) and not bool(hist.any()), "something was launched"
    # the host copy is fine, the device copy is not: row 1 is flagged and neither read nor written
    status = torch.full((rows,), 5, dtype=torch.int32, device=DEV)
    assert call(good, bad, status.data_ptr()) == 0
    assert status.tolist() == [0, -1, 0]
    got = y.cpu().numpy().reshape(rows, 100)
    assert np.all(got[1] == -7.0) and np.all(got[0, :n_out] != -7.0) and np.all(got[2, :n_out] != -7.0)
    assert np.all(got[0, n_out:] == -7.0) and np.all(got[2, n_out:] == -7.0)
    hh = hist.cpu().numpy()
    assert not hh[0].any() and not hh[1, 1].any() and np.all(hh[1, 0] == 1.0) and np.all(hh[1, 2] == 1.0)
    with pytest.raises(ValueError):
        resample.StreamResampler(2, 16000, 8000, 100, device=DEV).push(torch.zeros(2, 10), [0, 0])     # a CPU tensor


def test_carry_moves_every_rows_leftover_to_its_front():
    """ctn_stream_carry: overlapping spans (off < n), off = 0 and offsets outside the row (left alone), n above one pass of the
    workgroup."""
    ld, n = 1500, 1000
    offs = [0, 1, 7, 499, 500, 501, -3, 2000, 300]
    buf = torch.arange(len(offs) * ld, dtype=torch.float32, device=DEV).view(len(offs), ld)
    want = buf.clone()
    for r, o in enumerate(offs):
        if 0 < o <= ld - n:
            want[r, :n] = buf[r, o:o + n]
    tab = torch.zeros((len(offs), 8), dtype=torch.int64)
    tab[:, 7] = torch.tensor(offs)
    tab = tab.to(DEV)
    ctn.lib.call("ctn_stream_carry", buf.data_ptr(), ld, len(offs), tab.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    assert torch.equal(buf, want)
    small = torch.arange(40, dtype=torch.float32, device=DEV).view(2, 20)
    tab2 = torch.tensor([[0] * 7 + [11], [0] * 7 + [12]], dtype=torch.int64, device=DEV)
    ctn.lib.call("ctn_stream_carry", small.data_ptr(), 20, 2, tab2.data_ptr(), 9, torch.cuda.current_stream().cuda_stream)
    assert small[0, :9].tolist() == list(range(11, 20)) and small[1].tolist() == list(range(20, 40))     # 12 + 9 > 20: left alone
