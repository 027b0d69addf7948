"""CPU: the active speech level meter's host side (conv_tasnet_amd/levels.py) and its numpy restatement (levels_oracle.py):
the design against scipy, the sequential form against scipy.signal.lfilter, the properties that make the number a P.56 active
level, and the chunk-and-carry form (what the device computes) against the sequential one."""
import math

import numpy as np
import pytest

import levels_oracle as LO
from conv_tasnet_amd import levels

RATES = (8000, 16000)
# form (b) against form (a) over cases(): measured on the host that wrote this test, at CH = 256, 1024 and the library's:
# no exponent and no count differs, and the level moves by at most this many dB
RECORDED_DIFFERING_COUNTS = 0
RECORDED_MAX_DLEVEL_DB = 4.3e-14


def _level(st):
    return LO.level(st["ssq"], st["ns"], st["emax"], st["counts"])


@pytest.fixture(scope="module")
def sequential():
    """Form (a) of every shared case, computed once: {(fs, name): stats}."""
    ch = int(levels.lib.ctn_active_level_chunk())
    return {(fs, name): LO.stats_sequential(x, fs) for fs in RATES for name, x in LO.cases(fs, ch)}


def test_prototype_constants_are_scipys_chebyshev_ii():
    from scipy.signal import cheby2
    z, p, k = cheby2(5, 50, levels.W0, "high", analog=True, output="zpk")
    for mine, ref in ((levels.PROTO_ZEROS, z), (levels.PROTO_POLES, p)):
        full = np.concatenate(([mine[0]], mine[1:], np.conj(mine[1:])))
        assert len(full) == len(ref) == 5
        for v in full:
            assert np.abs(ref - v).min() <= 1e-12, (v, ref)
    assert abs(k - 1.0) <= 1e-12
    gain_db = 20.0 * math.log10(abs(np.prod(1j - z)) / abs(np.prod(1j - p)))          # -0.25 dB at the edge w = 1
    assert abs(gain_db + 0.25) <= 1e-9
    assert levels.PROTO_ZEROS == LO.PROTO_ZEROS and levels.PROTO_POLES == LO.PROTO_POLES and levels.W0 == LO.W0


@pytest.mark.parametrize("fs", RATES + (11025, 12100, 12101, 48000))      # 2.2 * 5500 rounds to just above 12100
@pytest.mark.parametrize("chunk", [256, 1024])
def test_design_is_the_restatements_design_bitwise(fs, chunk):
    a, b = levels.design(fs, chunk), LO.design(fs, chunk)
    assert (a["nz"], a["nh"], a["use_lp"], a["chunk"]) == (b["nz"], b["nh"], b["use_lp"], b["chunk"])
    assert a["nz"] == math.ceil(0.35 * fs) and a["nh"] == math.ceil(0.2 * fs) + 1 and a["use_lp"] == (fs > 12100)
    for k, v in a["sections"].items():
        assert (v is None and b["sections"][k] is None) or np.array_equal(v, b["sections"][k]), k
    assert np.array_equal(a["t_band"], b["t_band"]) and np.array_equal(a["t_env"], b["t_env"])
    S = 10 if a["use_lp"] else 5
    t = a["table"]
    assert t.shape == (levels.TABLE_DOUBLES,) and np.array_equal(t[27:27 + S * S].reshape(S, S), a["t_band"])
    assert np.array_equal(t[127:131].reshape(2, 2), a["t_env"]) and np.array_equal(t[24:27], a["sections"]["env"])
    assert np.array_equal(t[0:3], a["sections"]["hp1"]) and np.array_equal(t[3:8], a["sections"]["bq1"])
    assert np.array_equal(t[8:13], a["sections"]["bq2"]) and (not a["use_lp"] or np.array_equal(t[13:24], a["sections"]["lp"]))


@pytest.mark.parametrize("fs", RATES)
def test_design_has_unit_gain_where_the_meter_says(fs):
    sec = levels.design(fs, 64)["sections"]
    at = lambda z: ((sec["hp1"][0] + sec["hp1"][1] / z) / (1 + sec["hp1"][2] / z)
                    * np.prod([(sec[n][0] + sec[n][1] / z + sec[n][2] / z ** 2) / (1 + sec[n][3] / z + sec[n][4] / z ** 2)
                               for n in ("bq1", "bq2")]))
    assert abs(abs(at(-1.0)) - 1.0) <= 1e-12                                         # Nyquist gain of the high-pass
    edge = np.exp(2j * np.pi * 200.0 / fs)
    assert abs(20 * math.log10(abs(at(edge))) + 0.25) <= 1e-6                         # -0.25 dB at 200 Hz
    if sec["lp"] is not None:
        assert abs(sec["lp"][:6].sum() / (1.0 + sec["lp"][6:].sum()) - 1.0) <= 1e-12  # DC gain of the low-pass
    b0, a1, a2 = sec["env"]
    assert abs(b0 / (1.0 + a1 + a2) - 1.0) <= 1e-9                                    # DC gain of the envelope


def test_rates_outside_the_range_are_refused():
    for fs in (7999, 48001, 0):
        with pytest.raises(ValueError):
            levels.design(fs, 1024)


@pytest.mark.parametrize("fs", RATES)
def test_sequential_form_is_scipys_lfilter_chain(fs, sequential):
    for name in ("long", "3nh", "pad1_int16"):
        st = sequential[(fs, name)]
        x = dict(LO.cases(fs, int(levels.lib.ctn_active_level_chunk())))[name]
        y = LO.scipy_band(x, fs)
        assert np.abs(st["y"] - y).max() <= 1e-12 * np.abs(y).max(), name
        differ = int((LO.exponents(LO.scipy_envelope(y, fs)) != st["e"]).sum())
        print("%s at %d Hz: %d envelope exponents differ from scipy's" % (name, fs, differ))
        assert differ == 0, name


@pytest.mark.parametrize("fs", RATES)
@pytest.mark.parametrize("k", [10, -10])
def test_a_power_of_two_gain_shifts_the_exponents_and_nothing_else(fs, k, sequential):
    x = dict(LO.cases(fs, 1024))["3nh"]
    a, b = sequential[(fs, "3nh")], LO.stats_sequential(x * np.float32(2.0 ** k), fs)
    assert b["ssq"] == a["ssq"] * 4.0 ** k and b["emax"] == a["emax"] + 2 * k and np.array_equal(a["counts"], b["counts"])
    assert b["ns"] == a["ns"]


@pytest.mark.parametrize("fs", RATES)
def test_appended_silence_moves_the_long_term_level_not_the_active_level(fs):
    rng = np.random.default_rng(3)
    x = LO.bursts(rng, 4 * fs)
    a, b = LO.stats_sequential(x, fs), LO.stats_sequential(np.concatenate((x, np.zeros(2 * fs, dtype=np.float32))), fs)
    la, lb = _level(a), _level(b)
    print("active %.5f -> %.5f dB, long term %+.4f dB" % (la["level_db"], lb["level_db"],
                                                           10 * math.log10(lb["long_term"] / la["long_term"])))
    assert abs(lb["level_db"] - la["level_db"]) <= 1e-9
    assert abs(10 * math.log10(lb["long_term"] / la["long_term"]) - 10 * math.log10(a["ns"] / b["ns"])) <= 1e-9
    # (the lengths are the padded ones: -1.643 dB for 4.35 s -> 6.35 s; the plain RMS of the unpadded file drops by
    # 10 log10(6 / 4) = 1.7609 dB)


@pytest.mark.parametrize("fs", RATES)
def test_a_sine_reads_its_own_power(fs):
    """4 s of a 1 kHz sine of amplitude 0.5: 0.29 dB +- 0.01 below A^2 / 2 (the band filter's ripple and the meter's 0.35 s of
    padding), activity 0.98.  The figure comes from this restatement, not from the MATLAB meter."""
    x = (0.5 * np.sin(2 * np.pi * 1000.0 * np.arange(4 * fs) / fs)).astype(np.float32)
    lv = _level(LO.stats_sequential(x, fs))
    rel = lv["level_db"] - 10 * math.log10(0.5 ** 2 / 2)
    print("sine at %d Hz: %.4f dB re A^2/2, activity %.4f" % (fs, rel, lv["activity"]))
    assert abs(rel + 0.29) <= 0.01 and abs(lv["activity"] - 0.98) <= 0.005


@pytest.mark.parametrize("fs", RATES)
def test_silence_has_level_zero(fs):
    st = LO.stats_sequential(np.zeros(1000, dtype=np.float32), fs)
    assert st["ssq"] == 0.0 and st["emax"] == LO.EMPTY + 1 and st["counts"][0] == st["ns"] and st["counts"][1:].sum() == 0
    lv = _level(st)
    assert lv["level"] == 0.0 and lv["activity"] == 0.0 and lv["long_term"] == 0.0
    got = levels.level_from_counts([st["ssq"]], [st["ns"]], [st["emax"]], [st["counts"]])
    assert got["level"][0] == 0.0 and got["activity"][0] == 0.0 and got["level_db"][0] == -np.inf


def test_level_from_counts_is_the_restatements_level(sequential):
    keys = sorted(sequential)
    got = levels.level_from_counts([sequential[k]["ssq"] for k in keys], [sequential[k]["ns"] for k in keys],
                                   [sequential[k]["emax"] for k in keys], np.stack([sequential[k]["counts"] for k in keys]))
    for i, k in enumerate(keys):
        want = _level(sequential[k])
        for name in ("level", "level_db", "long_term", "activity"):
            assert got[name][i] == want[name] or abs(got[name][i] - want[name]) <= 1e-12 * abs(want[name]), (k, name)
    # the two ends without a crossing: every bin above the margin -> the top bin's level; every bin below -> the last bin's
    flat = np.zeros(20, dtype=np.int64)
    flat[0] = 1000
    hi = levels.level_from_counts([1000.0 * 2.0 ** 40], [1000], [0], [flat])
    assert abs(hi["level_db"][0] - 10 * math.log10(2.0 ** 40)) <= 1e-9
    lo = levels.level_from_counts([1000.0 * 2.0 ** -80], [1000], [0], [flat])
    assert abs(lo["level_db"][0] - 10 * math.log10(2.0 ** -80)) <= 1e-9


@pytest.mark.parametrize("fs", RATES)
@pytest.mark.parametrize("chunk", [256, 1024, None])
def test_chunk_and_carry_form_against_the_sequential_form(fs, chunk, sequential):
    lib_ch = int(levels.lib.ctn_active_level_chunk())
    ch = lib_ch if chunk is None else chunk
    differing, worst = 0, 0.0
    for name, x in LO.cases(fs, lib_ch):
        a, b = sequential[(fs, name)], LO.stats_chunked(x, fs, ch)
        assert a["ns"] == b["ns"] == len(x) + math.ceil(0.35 * fs), name
        differing += int((a["counts"] != b["counts"]).sum()) + int(a["emax"] != b["emax"])
        la, lb = _level(a), _level(b)
        if la["level"] > 0 or lb["level"] > 0:
            worst = max(worst, abs(la["level_db"] - lb["level_db"]))
        else:
            assert la["level"] == lb["level"] == 0.0, name
    print("fs %d CH %d: %d differing counts, max |dlevel_db| %.3e" % (fs, ch, differing, worst))
    assert differing <= RECORDED_DIFFERING_COUNTS
    assert worst <= 10 * RECORDED_MAX_DLEVEL_DB and worst <= 1e-4


def test_bad_sizes_are_refused_before_any_launch():
    """Fake 64-byte-aligned pointers: every such call must be refused before any HIP call (this runs without a GPU)."""
    ok = dict(samples=64, num_samples=8, offsets=64, lens=64, chunk_ptr=64, U=1, total_chunks=1, table=64, use_lp=0, nz=2800, nh=1601,
              ssq=64, ns=64, emax=64, counts=64, workspace=64, workspace_bytes=0, stream=0)
    names = levels.lib.protos["ctn_active_level"][2]
    assert set(names) == set(ok)
    call = levels.lib.load().ctn_active_level
    ch = levels.lib.ctn_active_level_chunk()
    # nh = CH - 1: a hangover window inside a chunk, which the one-split hangover kernel would get wrong; 2^24 chunks: its grid
    for bad in (dict(U=0), dict(total_chunks=0), dict(total_chunks=1 << 31), dict(total_chunks=1 << 24, U=1), dict(nh=9602), dict(nh=0),
                dict(nh=ch - 1), dict(nz=-1), dict(use_lp=2), dict(num_samples=0), dict(table=0),
                dict(workspace=68, workspace_bytes=1 << 20)):
        assert call(*[dict(ok, **bad)[k] for k in names]) == -1 and levels.lib.ctn_last_error().startswith(b"ctn_active_level:"), bad
    assert call(*[ok[k] for k in names]) == -3 and b"workspace" in levels.lib.ctn_last_error()       # too small a workspace
    assert call(*[dict(ok, nh=ch)[k] for k in names]) == -3                                            # the smallest nh is a valid size
    assert ch >= 64 and levels.lib.ctn_active_level_workspace(0, 1) == 0
    assert levels.lib.ctn_active_level_workspace(10, 3) >= 10 * (2 * ch + 8 * 13)
