"""CPU: the integrated loudness meter's host side (loudness.py) and its numpy restatement (loudness_oracle.py): the design
against the Recommendation's table, the standard's test signals, the gates, the block edges, and the chunk-and-carry filter
against scipy's sequential one."""
import math

import numpy as np
import pytest

import loudness_oracle as LO
from conv_tasnet_amd import _lib, loudness

CH = 1024
# ITU-R BS.1770-4, tables 1 and 2 (48 kHz): b0 b1 b2 a1 a2 of the two stages
BS1770_SHELF = (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585)
BS1770_HP = (1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621)
# the largest |oracle - lfilter| / max |lfilter| measured on 10 s of noise (seed = rate): 1.75e-14 at 8 kHz, 3.09e-13 at 48 kHz; the two
# differ only in the summation order across the chunk carries.  The test allows ten times that.
LFILTER_MEASURED = {8000: 1.75e-14, 48000: 3.09e-13}


def _db(x):
    return 10.0 ** (x / 20.0)


def test_design_gives_the_recommendations_table_at_48_khz():
    d = loudness.design(48000, CH)
    got = np.concatenate((d["shelf"], d["hp"]))
    want = np.array(BS1770_SHELF + BS1770_HP)
    print("largest difference from the table: %.3g" % np.abs(got - want).max())
    assert np.abs(got - want).max() < 1e-13
    assert d["hop"] == 4800 and d["block"] == 19200 and d["chunk"] == CH
    assert d["abs_gate"] == 10.0 ** ((-70.0 + 0.691) / 10.0)
    assert d["table"].shape == (loudness.TABLE_DOUBLES,) and d["table"][26] == d["abs_gate"]
    assert np.array_equal(d["table"][0:5], d["shelf"]) and np.array_equal(d["table"][5:10], d["hp"])
    assert np.array_equal(d["table"][10:26].reshape(4, 4), d["t"])


@pytest.mark.parametrize("fs", [8000, 16000, 22050, 44100, 48000])
def test_design_is_the_oracles_bit_for_bit(fs):
    a, b = loudness.design(fs, 64), LO.design(fs, 64)
    for k in ("shelf", "hp", "t"):
        assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), k
    assert a["hop"] == b["hop"] == fs // 10 and a["abs_gate"] == b["abs_gate"]
    # T is A^chunk: the state 64 zero-input samples after a state s is T s
    s0 = np.array([0.3, -0.2, 0.7, 0.1])
    z = [np.array([v]) for v in s0]
    for _ in range(64):
        _, z = LO.k_step(b, np.zeros(1), z)
    assert np.allclose(np.concatenate(z), a["t"] @ s0, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("rate", [7990, 48010, 11025, 8001, 44105, 16000.5])
def test_an_unsupported_rate_raises(rate):
    with pytest.raises(ValueError):
        loudness.design(rate, CH)


@pytest.mark.parametrize("fs,want", [(48000, -3.01), (16000, -2.970), (8000, -2.996)])
def test_full_scale_997_hz_sine(fs, want):
    """-3.01 LKFS at 48 kHz (BS.1770: a full-scale 997 Hz sine in one channel); the bilinear warp moves it at lower rates."""
    st = LO.stats(LO.tone(fs, 997.0, 5.0, 1.0), fs, CH)
    got = LO.loudness(st)["lufs"]
    print("%d Hz: %.4f LKFS, %d blocks" % (fs, got, st["n_blocks"]))
    assert abs(got - want) <= 0.01
    assert st["n_blocks"] == st["n_abs"] == st["n_rel"] == 47


def test_gating_ebu_tech_3341_case_3_in_mono():
    """1 kHz at -36 dBFS for 10 s, -23 dBFS for 60 s, -36 dBFS for 10 s: -23.0 +- 0.1 LUFS in stereo, 3.01 less in mono."""
    fs = 48000
    seq = lambda q: np.concatenate([LO.tone(fs, 1000.0, 10.0, _db(q)), LO.tone(fs, 1000.0, 60.0, _db(-23.0)), LO.tone(fs, 1000.0, 10.0, _db(q))])
    st = LO.stats(seq(-36.0), fs, CH)
    got = LO.loudness(st)
    print("quiet parts at -36 dBFS: %.4f LUFS (ungated %.4f), blocks %d / abs %d / rel %d" % (
        got["lufs"], got["ungated"], st["n_blocks"], st["n_abs"], st["n_rel"]))
    assert abs(got["lufs"] - (-26.01)) <= 0.1
    assert st["n_rel"] < st["n_abs"] == st["n_blocks"] == 797
    assert got["ungated"] < got["lufs"]
    st = LO.stats(seq(-80.0), fs, CH)
    got = LO.loudness(st)
    print("quiet parts at -80 dBFS: %.4f LUFS, blocks %d / abs %d / rel %d" % (got["lufs"], st["n_blocks"], st["n_abs"], st["n_rel"]))
    assert st["n_abs"] < st["n_blocks"] and st["n_rel"] <= st["n_abs"]
    assert abs(got["lufs"] - (-26.01)) <= 0.1


@pytest.mark.parametrize("fs", [8000, 48000])
def test_chunked_filter_against_scipy_lfilter(fs):
    pytest.importorskip("scipy")
    x = (0.1 * np.random.default_rng(fs).standard_normal(10 * fs)).astype(np.float32)
    Y, N = LO.k_weight(x, fs, CH)
    y, ref = Y.reshape(-1)[:N], LO.scipy_k_weight(x, fs)
    rel = float(np.abs(y - ref).max() / np.abs(ref).max())
    print("%d Hz: largest relative difference %.3g (measured %.3g)" % (fs, rel, LFILTER_MEASURED[fs]))
    assert rel <= 10.0 * LFILTER_MEASURED[fs]


@pytest.mark.parametrize("chunk", [512, 700, 1601])
def test_the_chunk_length_moves_rounding_only(chunk):
    """Any chunk that meets at most three sub-blocks (chunk < 2 h + 2) gives the same blocks up to rounding."""
    fs = 8000
    x = (0.1 * np.random.default_rng(3).standard_normal(3 * fs + 17)).astype(np.float32)
    a, b = LO.stats(x, fs, CH), LO.stats(x, fs, chunk)
    assert a["n_blocks"] == b["n_blocks"] == 27 and a["n_rel"] == b["n_rel"]
    assert np.allclose(a["z"], b["z"], rtol=1e-11)


def test_block_edges():
    fs, h = 8000, 800
    n = 4 * h
    rng = np.random.default_rng(0)
    for length, blocks in ((n - 1, 0), (n, 1), (n + h - 1, 1), (n + h, 2)):
        st = LO.stats((0.1 * rng.standard_normal(length)).astype(np.float32), fs, CH)
        assert st["n_blocks"] == blocks and st["ns"] == length, (length, st["n_blocks"])
        assert (LO.loudness(st)["power"] > 0) == (blocks > 0)
    # a block is 4 h samples every h: the first block of a signal is the whole loudness of its first 4 h samples
    x = (0.1 * rng.standard_normal(n + h)).astype(np.float32)
    a, b = LO.stats(x, fs, CH), LO.stats(x[:n], fs, CH)
    assert a["z"][0] == b["z"][0]


def test_silence_and_a_tone_below_the_absolute_gate_have_no_loudness():
    for x in (np.zeros(8000, dtype=np.float32), LO.tone(8000, 440.0, 1.0, 1e-5)):
        st = LO.stats(x, 8000, CH)
        got = LO.loudness(st)
        assert st["n_blocks"] == 7 and st["n_abs"] == 0 and st["n_rel"] == 0 and st["sum_rel"] == 0.0
        assert got["power"] == 0.0 and got["lufs"] == -math.inf
        host = loudness.loudness_from_stats(st["n_blocks"], st["n_abs"], st["n_rel"], st["sum_all"], st["sum_abs"], st["sum_rel"])
        assert host["power"][0] == 0.0 and host["lufs"][0] == -np.inf


def test_loudness_from_stats_is_the_oracles():
    st = LO.stats(dict(LO.cases(8000, CH))["loud_quiet"], 8000, CH)         # the relative gate bites
    assert 0 < st["n_rel"] < st["n_abs"] == st["n_blocks"]
    want = LO.loudness(st)
    got = loudness.loudness_from_stats([st["n_blocks"], 0], [st["n_abs"], 0], [st["n_rel"], 0], [st["sum_all"], 0.0],
                                       [st["sum_abs"], 0.0], [st["sum_rel"], 0.0])
    assert got["power"][0] == want["power"] and abs(got["lufs"][0] - want["lufs"]) < 1e-12
    assert abs(got["ungated"][0] - want["ungated"]) < 1e-12
    assert got["power"][1] == 0.0 and got["lufs"][1] == -np.inf and got["ungated"][1] == -np.inf


def test_c_abi_is_declared():
    protos = _lib.parse_header()
    assert all(n in protos for n in ("ctn_loudness", "ctn_loudness_workspace", "ctn_loudness_chunk"))
    assert protos["ctn_loudness_workspace"][0] is _lib.ctypes.c_size_t and protos["ctn_loudness"][0] is _lib.ctypes.c_int
    assert protos["ctn_loudness"][2] == ["samples", "num_samples", "offsets", "lens", "chunk_ptr", "U", "total_chunks", "table", "hop", "ns",
                                         "n_blocks", "n_abs", "n_rel", "sum_all", "sum_abs", "sum_rel", "workspace", "workspace_bytes",
                                         "stream"]
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("_b", os.path.join(os.path.dirname(_lib.__file__), "_build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "ctn_loudness.hip" in mod.SOURCES and "ctn_dynmix_loudness.hip" in mod.SOURCES
