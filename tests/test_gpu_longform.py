"""GPU: long-recording separation (csrc/ctn_longform.hip, longform.py) against the numpy restatement in longform_oracle.py.
Framing, costs, orders and assembled recordings are BITWISE the oracle's (uint32 views) at the smallest shapes at which the
kernels can go wrong; bad tables are refused before the launch and flagged in the kernel; nothing synchronises; and
separate_long / separate() are the test's own frame -> model -> oracle stitch."""
import os

import numpy as np
import pytest
import torch

import longform_oracle as LO
from oracle import ctn_oracle as O

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import longform, resample  # noqa: E402

DEV = "cuda:0"
NAN = float("nan")
# (seg, hop): ov = 1, 4, 1023, 1024, 1025, 2049 -- both sides of one and of two rounds of the 1024 partial sums -- with hops of
# both alignments modulo 4, and one 16-byte aligned geometry whose last round is partial (ov = 2052)
STITCH_GEOMETRIES = [(8, 7), (12, 8), (2048, 1025), (2048, 1024), (2052, 1027), (4100, 2051), (4104, 2052)]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _layout(sizes, rng, lo=1, hi=9):
    """Offsets of rows of `sizes` floats with drawn gaps before, between and behind them -> (offsets, total)."""
    gaps = rng.integers(lo, hi, size=len(sizes) + 1)
    offs, at = [], int(gaps[0])
    for n, gp in zip(sizes, gaps[1:]):
        offs.append(at)
        at += int(n) + int(gp)
    return np.array(offs, dtype=np.int64), at


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- framing -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seg,hop", [(8, 4), (64, 63), (2050, 1025)])
def test_frames_are_bitwise_the_oracle_and_never_read_beyond_a_recording(seg, hop):
    rng = np.random.default_rng(seg)
    lens = np.array([1, seg, seg + 1, 2 * hop + seg, int(3.3 * seg)], dtype=np.int64)
    rows = [rng.standard_normal(int(n)).astype(np.float32) for n in lens]
    offsets, total = _layout(lens, rng)
    x = np.full(total, np.nan, dtype=np.float32)
    for o, r in zip(offsets, rows):
        x[o:o + len(r)] = r
    segs, seg_ptr = longform.frame_ragged(torch.from_numpy(x).to(DEV), offsets, lens, seg, hop)
    assert np.array_equal(seg_ptr, LO.seg_ptr(lens, seg, hop)) and list(np.diff(seg_ptr)[:4]) == [1, 1, 2, 3]
    got = segs.cpu().numpy()
    assert got.shape == (int(seg_ptr[-1]), seg) and np.isfinite(got).all(), "a segment read NaN from beyond its recording"
    for r, row in enumerate(rows):
        want = LO.frame(row, seg, hop)
        assert np.array_equal(_bits(got[seg_ptr[r]:seg_ptr[r + 1]]), _bits(want)), r


# ---- the stitch on synthetic estimates -----------------------------------------------------------------------------------
def _stitch_case(seg, hop, C, seed, noise=1e-3):
    """Recordings of 1, 2, 3, 1 and 7 segments: T = seg, seg + 1, the exact cover of three segments, one T < seg, and a padded
    seven.  Sources with a drawn local permutation per segment plus seeded noise."""
    rng = np.random.default_rng(seed)
    lens = np.array([seg, seg + 1, 2 * hop + seg, max(1, seg // 3), 5 * hop + seg + hop // 2 + 1], dtype=np.int64)
    ests, locals_ = [], []
    for T in lens:
        src = rng.standard_normal((C, int(T))).astype(np.float32)
        e, loc = LO.permuted_segments(src, seg, hop, rng, noise=noise)
        ests.append(e)
        locals_.append(loc)
    seg_ptr = LO.seg_ptr(lens, seg, hop)
    assert list(np.diff(seg_ptr)) == [1, 2, 3, 1, 7]
    return lens, seg_ptr, ests, locals_


def _raw_stitch(est, seg_ptr, lens, hop, window, out_off, out):
    """The three entry points on caller-owned buffers -> (cost, g, status of order, status of assemble)."""
    Nseg, C, seg = est.shape
    R = len(lens)
    host = np.ascontiguousarray(np.concatenate([seg_ptr, lens, out_off]).astype(np.int64))
    dev = torch.from_numpy(host).to(DEV)
    fi, fo = (torch.from_numpy(t).to(DEV) for t in LO.fade_tables(seg - hop, window))
    cost = torch.full((Nseg, C, C), NAN, device=DEV)
    g = torch.full((Nseg, C), -1, dtype=torch.int32, device=DEV)
    st = torch.full((2, R), 5, dtype=torch.int32, device=DEV)
    ctn.lib.call("ctn_longform_costs", est.data_ptr(), dev.data_ptr(), R, Nseg, C, seg, hop, cost.data_ptr(), host.ctypes.data, _stream())
    ctn.lib.call("ctn_longform_order", cost.data_ptr(), dev.data_ptr(), R, Nseg, C, g.data_ptr(), host.ctypes.data, st[0].data_ptr(), _stream())
    ctn.lib.call("ctn_longform_assemble", est.data_ptr(), g.data_ptr(), dev.data_ptr(), dev[R + 1:].data_ptr(), dev[2 * R + 1:].data_ptr(), R,
                 Nseg, C, seg, hop, fi.data_ptr(), fo.data_ptr(), out.data_ptr(), out.numel(), host.ctypes.data, st[1].data_ptr(), _stream())
    torch.cuda.synchronize()
    return cost.cpu().numpy(), g.cpu().numpy(), st.cpu().numpy()


@pytest.mark.parametrize("C", [2, 3, 4])
@pytest.mark.parametrize("seg,hop", STITCH_GEOMETRIES)
def test_costs_orders_and_recordings_are_bitwise_the_oracle(seg, hop, C):
    window = "hann" if C == 3 else "linear"
    lens, seg_ptr, ests, locals_ = _stitch_case(seg, hop, C, seed=seg * 10 + C)
    est = torch.from_numpy(np.concatenate(ests)).to(DEV)
    rng = np.random.default_rng(1)
    out_off, total = _layout(C * lens, rng)
    out = torch.full((total,), NAN, device=DEV)
    cost, g, status = _raw_stitch(est, seg_ptr, lens, hop, window, out_off, out)
    got = out.cpu().numpy()
    assert np.all(status == 0)
    written = np.zeros(total, dtype=bool)
    for r, T in enumerate(lens):
        want_out, want_g, want_cost = LO.stitch(ests[r], int(T), hop, window)
        lo, hi = seg_ptr[r], seg_ptr[r + 1]
        assert np.array_equal(_bits(cost[lo:hi]), _bits(want_cost)), "recording %d: costs differ" % r
        assert np.array_equal(g[lo:hi], want_g), "recording %d: orders differ" % r
        assert np.array_equal(g[lo:hi], locals_[r]), "recording %d: the order is not the composition of the drawn permutations" % r
        mine = got[out_off[r]:out_off[r] + C * T].reshape(C, T)
        bad = int((_bits(mine) != _bits(want_out)).sum())
        assert bad == 0, "recording %d: %d of %d samples differ in their bits" % (r, bad, C * T)
        written[out_off[r]:out_off[r] + C * T] = True
    assert np.isnan(got[~written]).all(), "the assembly wrote outside its recordings"
    # the public form: its own tables and buffer, the same bits
    outs, g2 = longform.stitch_ragged(est, seg_ptr, lens, hop, window=window, return_order=True)
    assert g2.dtype == torch.int32 and np.array_equal(g2.cpu().numpy(), g)
    for r, T in enumerate(lens):
        assert outs[r].shape == (C, T)
        assert np.array_equal(_bits(outs[r].cpu().numpy()), _bits(got[out_off[r]:out_off[r] + C * T].reshape(C, T)))
    c2 = longform.segment_costs(est, seg_ptr, hop)
    assert np.array_equal(_bits(c2.cpu().numpy()), _bits(cost))


def test_an_exact_tie_takes_the_first_permutation_on_the_device():
    rng = np.random.default_rng(3)
    seg, hop, T = 64, 40, 150
    for C in (2, 3, 4):
        src = rng.standard_normal((C, T)).astype(np.float32)
        est, _ = LO.permuted_segments(src, seg, hop, rng)
        est[1, 1, :seg - hop] = est[1, 0, :seg - hop]
        want_out, want_g, want_cost = LO.stitch(est, T, hop)
        assert np.array_equal(want_cost[1, :, 0], want_cost[1, :, 1])
        outs, g = longform.stitch_ragged(torch.from_numpy(est).to(DEV), [0, len(est)], [T], hop, return_order=True)
        assert np.array_equal(g.cpu().numpy(), want_g)
        assert np.array_equal(_bits(outs[0].cpu().numpy()), _bits(want_out))
    # all costs equal (silence): every segment keeps the identity
    outs, g = longform.stitch_ragged(torch.zeros((4, 3, 16), device=DEV), [0, 4], [40], 8, return_order=True)
    assert g.cpu().numpy().tolist() == [[0, 1, 2]] * 4 and not outs[0].any()


def test_a_table_row_outside_its_buffer_is_refused_before_the_launch_and_flagged_in_the_kernel():
    """Not a fault test: the host checks its copy of the tables before it launches, and the kernels check the device copy before
    they form an address."""
    rng = np.random.default_rng(5)
    C, seg, hop = 2, 8, 4
    lens = np.array([16, 20], dtype=np.int64)
    seg_ptr = LO.seg_ptr(lens, seg, hop)                          # 0, 3, 7
    est = torch.from_numpy(rng.standard_normal((7, C, seg)).astype(np.float32)).to(DEV)
    g = torch.zeros((7, C), dtype=torch.int32, device=DEV)
    g[:, 1] = 1
    fi, fo = (torch.from_numpy(t).to(DEV) for t in LO.fade_tables(seg - hop))
    out = torch.full((72,), -7.0, device=DEV)
    status = torch.full((2,), 5, dtype=torch.int32, device=DEV)

    def assemble(host, dev, st=0):
        host = np.ascontiguousarray(np.array(host, dtype=np.int64))
        d = torch.from_numpy(np.ascontiguousarray(np.array(dev, dtype=np.int64))).to(DEV)
        rc = ctn.lib.ctn_longform_assemble(est.data_ptr(), g.data_ptr(), d.data_ptr(), d[3:].data_ptr(), d[5:].data_ptr(), 2, 7, C, seg, hop,
                                           fi.data_ptr(), fo.data_ptr(), out.data_ptr(), out.numel(), host.ctypes.data, st, _stream())
        torch.cuda.synchronize()
        return rc

    good = [0, 3, 7, 16, 20, 0, 32]                               # seg_ptr, T, out_off
    for bad in ([0, 3, 7, 16, 20, 0, 33],                         # 33 + 2 * 20 > 72
                [0, 3, 7, 16, 20, -1, 32],
                [0, 3, 7, 16, 21, 0, 32],                         # 21 samples are 5 segments
                [0, 4, 7, 16, 20, 0, 32],
                [0, 3, 8, 16, 20, 0, 32]):                        # seg_ptr[R] is not Nseg
        assert assemble(bad, bad) == -1 and b"ctn_longform_assemble" in ctn.lib.ctn_last_error()
        assert bool((out == -7.0).all()), "something was launched"
    # the host copy is fine, the device copy is not: recording 1 is flagged and neither read nor written
    for bad in ([0, 3, 7, 16, 20, 0, 33], [0, 3, 7, 16, 2000, 0, 32], [0, 3, 9, 16, 20, 0, 32]):
        out.fill_(-7.0)
        status.fill_(5)
        assert assemble(good, bad, status.data_ptr()) == 0
        assert status.tolist() == [0, -1]
        got = out.cpu().numpy()
        assert np.all(got[32:] == -7.0) and np.all(got[:32] != -7.0)
    want = LO.assemble(est[:3].cpu().numpy(), g[:3].cpu().numpy(), 16, hop, *LO.fade_tables(seg - hop))
    assert np.array_equal(_bits(got[:32].reshape(2, 16)), _bits(want))
    # an order entry outside [0, C) never forms an address: that channel stays unwritten where the segment, or the cross-fade of
    # its successor, would have read it
    g[4, 1] = 7
    out.fill_(-7.0)
    assert assemble(good, good) == 0
    got = out.cpu().numpy()[32:].reshape(2, 20)
    assert np.all(got[0] != -7.0) and np.all(got[1, 4:12] == -7.0) and np.all(got[1, :4] != -7.0) and np.all(got[1, 12:] != -7.0)

    # framing: the same two checks
    x = torch.ones(40, device=DEV)
    segs = torch.full((7, seg), -7.0, device=DEV)

    def frame(host, dev, st=0):
        host = np.ascontiguousarray(np.array(host, dtype=np.int64))
        d = torch.from_numpy(np.ascontiguousarray(np.array(dev, dtype=np.int64))).to(DEV)
        rc = ctn.lib.ctn_longform_frame(x.data_ptr(), x.numel(), d.data_ptr(), d[3:].data_ptr(), d[5:].data_ptr(), 2, 7, seg, hop,
                                        segs.data_ptr(), host.ctypes.data, st, _stream())
        torch.cuda.synchronize()
        return rc

    good = [0, 3, 7, 16, 20, 0, 20]
    bad = [0, 3, 7, 16, 20, 0, 21]                                # 21 + 20 > 40
    assert frame(bad, bad) == -1 and b"outside the input buffer" in ctn.lib.ctn_last_error()
    assert bool((segs == -7.0).all()), "something was launched"
    status.fill_(5)
    assert frame(good, bad, status.data_ptr()) == 0
    assert status.tolist() == [0, -1]
    got = segs.cpu().numpy()
    assert np.all(got[:3] == 1.0) and np.all(got[3:] == -7.0)
    with pytest.raises(ctn.CtnError, match="outside the input buffer"):
        longform.frame_ragged(x, [0, 30], [16, 20], seg, hop)
    with pytest.raises(ValueError, match="seg_ptr"):
        longform.stitch_ragged(est, [0, 3, 7], [16, 21], hop)
    with pytest.raises(ValueError, match="speakers"):
        longform.stitch_ragged(torch.zeros((3, 5, 8), device=DEV), [0, 3], [16], 4)


def test_framing_and_stitching_neither_read_back_nor_synchronise():
    seg, hop, C = 2048, 1024, 2
    lens, seg_ptr, ests, _ = _stitch_case(seg, hop, C, seed=9)
    est = torch.from_numpy(np.concatenate(ests)).to(DEV)
    flat = torch.randn(int(lens.sum()), device=DEV)
    offsets = np.concatenate(([0], np.cumsum(lens)[:-1]))
    ref = longform.stitch_ragged(est, seg_ptr, lens, hop)         # the warm-up: fade tables, allocator blocks
    ref_segs, _ = longform.frame_ragged(flat, offsets, lens, seg, hop)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):                         # the mode is enforced: a read-back raises
            est[0, 0, 0].item()
        outs, g = longform.stitch_ragged(est, seg_ptr, lens, hop, return_order=True)
        segs, _ = longform.frame_ragged(flat, offsets, lens, seg, hop)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(torch.equal(a, b) for a, b in zip(outs, ref)) and torch.equal(segs, ref_segs)


# ---- end to end ------------------------------------------------------------------------------------------------------------
def _tiny_model():
    torch.manual_seed(0)
    return ctn.ConvTasNet(32, 20, 16, 32, 3, 2, 1, 2)


def test_separate_long_is_frame_model_and_the_oracles_stitch():
    seg, hop, bs = 1000, 500, 4
    m = _tiny_model().to(DEV).eval()
    mix, _, _ = O.synth_batch(0, 2, 3300)
    x0, x1 = mix[0].to(DEV), mix[1, :600].contiguous().to(DEV)
    got0, got1 = longform.separate_long(m, [x0, x1], seg, hop, batch_size=bs)
    assert got0.shape == (2, 3300) and got1.shape == (2, 600)
    with torch.no_grad():
        segs = torch.from_numpy(LO.frame(mix[0].numpy(), seg, hop)).to(DEV)
        assert segs.shape[0] == 6                                 # two forward batches: 4 + 2 segments
        est = torch.cat([m(segs[b:b + bs]) for b in range(0, 6, bs)]).cpu().numpy()
        short = m(x1[None])[0]
    want, _, _ = LO.stitch(est, 3300, hop)
    assert np.array_equal(_bits(got0.cpu().numpy()), _bits(want))
    assert np.array_equal(_bits(got1.cpu().numpy()), _bits(short.cpu().numpy()))
    # one tensor in, one tensor out; the default hop is segment // 2
    alone = longform.separate_long(m, x0, seg, batch_size=bs)
    assert torch.is_tensor(alone) and np.array_equal(_bits(alone.cpu().numpy()), _bits(want))


def test_a_separator_that_swaps_the_speakers_on_odd_segments_is_undone():
    """|out[t] - x[t]| <= 4 * 2^-24 * |x[t]| (the fade tables' rounding, two products and one sum)."""
    seg, hop, T, C = 1000, 500, 3300, 2
    rng = np.random.default_rng(11)
    src = rng.standard_normal((C, T)).astype(np.float32)
    framed = torch.from_numpy(np.stack([LO.frame(src[a], seg, hop) for a in range(C)], axis=1)).to(DEV)     # [n, C, seg]
    seen = [0]

    def model(batch):
        k = seen[0]
        seen[0] += batch.shape[0]
        y = framed[k:k + batch.shape[0]].clone()
        odd = torch.arange(k, k + batch.shape[0], device=DEV) % 2 == 1
        y[odd] = y[odd].flip(1)
        return y

    out = longform.separate_long(model, torch.from_numpy(src.sum(0)).to(DEV), seg, hop, batch_size=4, window="hann")
    assert seen[0] == framed.shape[0] == 6
    err = np.abs(out.cpu().numpy().astype(np.float64) - src.astype(np.float64))
    assert np.all(err <= 4.0 * 2.0 ** -24 * np.abs(src.astype(np.float64)))


def test_separate_with_a_segment_length(tmp_path):
    from scipy.io import wavfile
    from conv_tasnet_amd.separate import separate
    seg, hop = 1000, 500
    m = _tiny_model()
    path = str(tmp_path / "m.pth.tar")
    torch.save(ctn.ConvTasNet.serialize(m, torch.optim.Adam(m.parameters()), 1), path)
    mix, _, _ = O.synth_batch(0, 2, 6600)
    lens = {"long": 6600, "short": 1100}
    for rate, sub in ((8000, "mix8"), (16000, "mix16")):
        (tmp_path / sub).mkdir()
        for i, (name, n) in enumerate(lens.items()):
            n = n // 2 if rate == 8000 else n
            wavfile.write(str(tmp_path / sub / (name + ".wav")), rate, mix[i, :n].numpy())
    m = m.to(DEV).eval()
    names = sorted(n + s + ".wav" for n in lens for s in ("", "_s1", "_s2"))

    # files at the model's rate
    separate(path, str(tmp_path / "mix8"), None, str(tmp_path / "a"), 1, 8000, 1, segment=seg, hop=hop, segment_batch=4)
    assert sorted(os.listdir(tmp_path / "a")) == names
    for i, (name, n) in enumerate(lens.items()):
        x = mix[i, :n // 2].contiguous().to(DEV)
        want = longform.separate_long(m, x, seg, hop, batch_size=4).cpu().numpy()
        sr, y = wavfile.read(str(tmp_path / "a" / (name + ".wav")))
        assert sr == 8000 and np.array_equal(y, x.cpu().numpy())
        for c in range(2):
            sr, y = wavfile.read(str(tmp_path / "a" / ("%s_s%d.wav" % (name, c + 1))))
            assert sr == 8000 and y.dtype == np.float32 and y.shape == (n // 2,)
            assert np.array_equal(_bits(y), _bits(want[c])), (name, c)

    # files at 16 kHz: resample -> long-form -> resample back
    separate(path, str(tmp_path / "mix16"), None, str(tmp_path / "b"), 1, 8000, 1, file_rate=16000, segment=seg, segment_batch=4)
    assert sorted(os.listdir(tmp_path / "b")) == names
    for i, (name, n) in enumerate(lens.items()):
        low = resample.resample(mix[i, :n].contiguous().to(DEV), 16000, 8000)
        est = longform.separate_long(m, low, seg, batch_size=4)
        want = resample.resample(est.contiguous(), 8000, 16000)[:, :n].cpu().numpy()
        for c in range(2):
            sr, y = wavfile.read(str(tmp_path / "b" / ("%s_s%d.wav" % (name, c + 1))))
            assert sr == 16000 and y.shape == (n,)
            assert np.array_equal(_bits(y), _bits(want[c])), (name, c)

    # segment=None: the files of a call without the argument
    separate(path, str(tmp_path / "mix8"), None, str(tmp_path / "c"), 1, 8000, 2)
    separate(path, str(tmp_path / "mix8"), None, str(tmp_path / "d"), 1, 8000, 2, segment=None, hop=None)
    for f in names:
        assert (tmp_path / "c" / f).read_bytes() == (tmp_path / "d" / f).read_bytes()
    with pytest.raises(ValueError):
        separate(path, str(tmp_path / "mix8"), None, str(tmp_path / "e"), 1, 8000, 1, segment=1000, hop=400)
