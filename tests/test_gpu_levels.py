"""GPU: the active speech level meter (csrc/ctn_levels.hip, levels.py) against the chunk-and-carry form of levels_oracle.py at
the library's chunk length -- ssq BITWISE, ns, emax and all 20 counts exactly --, its independence of neighbours, order and
workspace grouping, the flag for entries outside the buffer, and level="active" through DeviceCorpus and DynamicMixLoader."""
import numpy as np
import pytest
import torch

import levels_oracle as LO

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import dynmix, levels  # noqa: E402

DEV = "cuda:0"
RATES = (8000, 16000)
HEAD = 37                            # samples in front of the first utterance: offsets are not a running sum from 0
_WORLD = {}


def _world(fs):
    """The shared cases at one rate, their flat device buffer and the oracle's statistics, computed once."""
    if fs not in _WORLD:
        ch = int(levels.lib.ctn_active_level_chunk())
        named = LO.cases(fs, ch)
        arrays = [x for _, x in named]
        lens = np.array([len(x) for x in arrays], dtype=np.int64)
        offsets = HEAD + np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64)
        flat = torch.from_numpy(np.concatenate([np.full(HEAD, 7.0, dtype=np.float32)] + arrays)).to(DEV)
        want = [LO.stats_chunked(x, fs, ch) for x in arrays]
        _WORLD[fs] = dict(names=[n for n, _ in named], arrays=arrays, lens=lens, offsets=offsets, flat=flat, want=want, ch=ch)
    return _WORLD[fs]


def _same(a, b, rows_a=None, rows_b=None, what=""):
    """The device statistics of rows_a of result a and rows_b of result b are the same bits."""
    ra = slice(None) if rows_a is None else rows_a
    rb = slice(None) if rows_b is None else rows_b
    assert np.array_equal(a["ssq"][ra].view(np.uint64), b["ssq"][rb].view(np.uint64)), what
    for k in ("ns", "emax", "counts"):
        assert np.array_equal(a[k][ra], b[k][rb]), (what, k)


@pytest.mark.parametrize("fs", RATES)
def test_statistics_are_the_oracles_bit_for_bit(fs):
    w = _world(fs)
    assert len(w["arrays"]) >= 12 and int(w["lens"].sum()) < 70000
    got = levels.active_level_ragged(w["flat"], w["offsets"], w["lens"], fs)
    for u, (name, st) in enumerate(zip(w["names"], w["want"])):
        print("%-12s len %6d  ssq %.17g (device %.17g)  emax %d (%d)  counts differing %d" % (
            name, w["lens"][u], st["ssq"], got["ssq"][u], st["emax"], got["emax"][u], int((st["counts"] != got["counts"][u]).sum())))
    for u, (name, st) in enumerate(zip(w["names"], w["want"])):
        assert got["ns"][u] == st["ns"], name
        assert got["emax"][u] == st["emax"], name
        assert np.array_equal(got["counts"][u], st["counts"]), (name, got["counts"][u], st["counts"])
        assert np.float64(got["ssq"][u]).view(np.uint64) == np.float64(st["ssq"]).view(np.uint64), (name, got["ssq"][u], st["ssq"])
        lv = LO.level(st["ssq"], st["ns"], st["emax"], st["counts"])
        for k in ("level", "long_term", "activity"):
            assert got[k][u] == lv[k] or abs(got[k][u] - lv[k]) <= 1e-12 * abs(lv[k]), (name, k)
    names = w["names"]
    assert (got["counts"][names.index("lead_zeros")][19] >= 2 * (int(0.2 * fs) + 1)            # -inf exponents under a finite emax
            and got["emax"][names.index("lead_zeros")] > -100)
    assert got["emax"][names.index("ch_zero")] == levels.EMPTY + 1 and got["level"][names.index("ch_zero")] == 0.0
    a, b = names.index("3nh"), names.index("3nh_x1024")
    assert got["ssq"][b] == got["ssq"][a] * 4.0 ** 10 and got["emax"][b] == got["emax"][a] + 20
    assert np.array_equal(got["counts"][a], got["counts"][b])


@pytest.mark.parametrize("fs", RATES)
def test_an_utterance_does_not_depend_on_neighbours_order_or_grouping(fs):
    w = _world(fs)
    U = len(w["lens"])
    base = levels.active_level_ragged(w["flat"], w["offsets"], w["lens"], fs)
    for u in range(U):                                                          # alone
        one = levels.active_level_ragged(w["flat"], w["offsets"][u:u + 1], w["lens"][u:u + 1], fs)
        _same(one, base, None, slice(u, u + 1), "alone %s" % w["names"][u])
    order = np.random.default_rng(5).permutation(U)                             # another order (of the table: the buffer stays)
    perm = levels.active_level_ragged(w["flat"], w["offsets"][order], w["lens"][order], fs)
    _same(perm, base, None, order, "permuted")
    nchunks = (w["lens"] + levels.design(fs)["nz"] + w["ch"] - 1) // w["ch"]
    total = int(levels.lib.ctn_active_level_workspace(int(nchunks.sum()), U))
    for bound, groups in ((total, 1), (total * 6 // 10, 2), (1, U)):
        assert len(levels._groups(nchunks, bound)) == groups
        _same(levels.active_level_ragged(w["flat"], w["offsets"], w["lens"], fs, workspace_bytes=bound), base, what="%d groups" % groups)


def test_an_entry_outside_the_buffer_is_flagged_and_nothing_else_changes():
    fs = 8000
    w = _world(fs)
    base = levels.active_level_ragged(w["flat"], w["offsets"], w["lens"], fs)
    n = w["flat"].numel()
    for u, off in ((3, -1), (0, n - int(w["lens"][0]) + 1), (len(w["lens"]) - 1, n)):
        offsets = w["offsets"].copy()
        offsets[u] = off
        got = levels.active_level_ragged(w["flat"], offsets, w["lens"], fs)
        keep = np.arange(len(offsets)) != u
        _same(got, base, keep, keep, "flag at %d" % u)
        assert got["ns"][u] == -1 and got["ssq"][u] == 0.0 and got["counts"][u].sum() == 0 and got["level"][u] == 0.0
    lens = w["lens"].copy()
    lens[2] = -5
    got = levels.active_level_ragged(w["flat"], w["offsets"], lens, fs)
    assert got["ns"][2] == -1
    keep = np.arange(len(lens)) != 2
    _same(got, base, keep, keep, "negative length")


def test_the_shortest_hangover_the_entry_point_takes_is_one_chunk():
    """nh = CH through the C ABI (the Python surface starts at 1601): every window then reaches exactly to the seam the hangover
    kernel splits at, in the first chunk, in full chunks and in the partial last one; one less is refused before any launch."""
    fs = 8000
    w = _world(fs)
    d, ch = levels.design(fs), w["ch"]
    rows = [w["names"].index(n) for n in ("long", "lead_zeros", "ch-1", "len1")]
    lens, offsets = w["lens"][rows], w["offsets"][rows]
    nch = (lens + d["nz"] + ch - 1) // ch
    U, G = len(rows), int(nch.sum())
    dev_i64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(DEV)
    off_d, len_d, cp_d, table = dev_i64(offsets), dev_i64(lens), dev_i64(np.concatenate(([0], np.cumsum(nch)))), torch.from_numpy(d["table"]).to(DEV)
    ssq = torch.zeros(U, dtype=torch.float64, device=DEV)
    ns, emax = torch.zeros(U, dtype=torch.int64, device=DEV), torch.zeros(U, dtype=torch.int32, device=DEV)
    counts = torch.zeros(U, 20, dtype=torch.int64, device=DEV)
    ws = torch.zeros(int(levels.lib.ctn_active_level_workspace(G, U)), dtype=torch.uint8, device=DEV)
    args = lambda nh: (w["flat"].data_ptr(), w["flat"].numel(), off_d.data_ptr(), len_d.data_ptr(), cp_d.data_ptr(), U, G, table.data_ptr(),
                       int(d["use_lp"]), d["nz"], nh, ssq.data_ptr(), ns.data_ptr(), emax.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                       ws.numel(), torch.cuda.current_stream().cuda_stream)
    with pytest.raises(ctn.CtnError, match="nh = %d" % (ch - 1)):
        levels.lib.call("ctn_active_level", *args(ch - 1))
    for nh in (ch, ch + 1):
        levels.lib.call("ctn_active_level", *args(nh))
        got_emax, got_counts = emax.cpu().numpy(), counts.cpu().numpy()
        for i, u in enumerate(rows):
            want_emax, want_counts = LO.occupancy(w["want"][u]["e"], nh)
            assert got_emax[i] == want_emax and np.array_equal(got_counts[i], want_counts), (nh, w["names"][u], got_counts[i], want_counts)
        assert not np.array_equal(got_counts[0], w["want"][rows[0]]["counts"])             # (and the window length matters)


@pytest.mark.parametrize("fs", RATES)
def test_padded_batch_equals_the_ragged_call(fs):
    w = _world(fs)
    rows = [u for u in range(len(w["lens"])) if w["lens"][u] <= 5000]
    T = int(max(w["lens"][u] for u in rows)) + 3
    x = np.full((len(rows), T), 9.0, dtype=np.float32)                          # what lies behind lengths[r] must not count
    for r, u in enumerate(rows):
        x[r, :w["lens"][u]] = w["arrays"][u]
    got = levels.active_level(torch.from_numpy(x).to(DEV), torch.from_numpy(w["lens"][rows]), fs)
    base = levels.active_level_ragged(w["flat"], w["offsets"], w["lens"], fs)
    _same(got, base, None, np.array(rows), "padded")
    assert np.array_equal(got["level"], base["level"][rows])


# ---- level="active" end to end ---------------------------------------------------------------------------------------------
SEG = 4000


@pytest.fixture(scope="module")
def speech():
    rng = np.random.default_rng(21)
    arrays = [LO.bursts(rng, int(n), amp=float(a)) for n, a in zip(rng.integers(5000, 9000, size=8), rng.uniform(0.02, 0.4, size=8))]
    arrays[5][:] = 0.0                                                          # silent: level 0, never eligible
    speakers = ["s%d" % (u % 4) for u in range(8)]
    want = [LO.stats_chunked(x, 8000, int(levels.lib.ctn_active_level_chunk())) for x in arrays]
    lp = np.array([LO.level(s["ssq"], s["ns"], s["emax"], s["counts"])["level"] for s in want])
    return arrays, speakers, lp


def test_device_corpus_takes_the_active_level(speech):
    arrays, speakers, lp = speech
    c = ctn.DeviceCorpus.from_arrays(arrays, speakers, DEV, level="active", sample_rate=8000)
    want = np.zeros(len(lp), dtype=np.float32)
    want[lp > 0] = (1.0 / np.sqrt(lp[lp > 0])).astype(np.float32)
    assert np.array_equal(c.inv_rms.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(c.level_power > 0, lp > 0) and c.level_power[5] == 0.0 and c.activity.shape == lp.shape
    ratio_db = 10 * np.log10(c.level_power[lp > 0] / c.meansq[lp > 0])          # another level than the RMS, not another scale
    assert np.all(np.abs(ratio_db) < 6.0) and np.abs(ratio_db).max() > 0.1
    host, _, _ = c.tables(SEG, 2)
    assert 5 not in host["utt_ids"].tolist() and len(host["utt_ids"]) == 7
    with pytest.raises(ValueError):
        ctn.DeviceCorpus.from_arrays(arrays, speakers, DEV, level="active")       # no rate
    with pytest.raises(ValueError):
        ctn.DeviceCorpus.from_arrays(arrays, speakers, DEV, level="peak", sample_rate=8000)
    r = ctn.DeviceCorpus.from_arrays(arrays, speakers, DEV)
    assert r.level == "rms" and r.activity is None and r.level_power is r.meansq


@pytest.mark.parametrize("level", ["active", "rms"])
def test_loader_mixes_at_the_corpus_level(speech, level):
    """One fill equals the gather of the loader's own plan with gain = w[q + 249] * inv_rms[u] (one fp32 multiply) from the
    level table in question; with "rms" that table is the parent's 1 / sqrt(meansq), so those bits are the parent's."""
    import dynmix_oracle as DO
    arrays, speakers, lp = speech
    c = ctn.DeviceCorpus.from_arrays(arrays, speakers, DEV, level=level, sample_rate=8000)
    if level == "rms":
        msq = DO.meansq(np.concatenate(arrays), c.offsets_host, c.lens_host)
        assert np.allclose(c.meansq, msq, rtol=1e-12)
        table = dynmix.inverse_rms(c.meansq)
    else:
        table = dynmix.inverse_rms(lp)
    assert np.array_equal(c.inv_rms.cpu().numpy().view(np.uint32), table.view(np.uint32))
    loader = ctn.DynamicMixLoader(c, batch_size=5, segment_len=SEG, steps_per_epoch=2, seed=9, rank=0)
    mixture = torch.empty(5, SEG, dtype=torch.float32, device=DEV)
    sources = torch.empty(5, 2, SEG, dtype=torch.float32, device=DEV)
    loader.fill(mixture, sources)
    utt, start, q, gain = loader.last_plan()
    w = DO.level_table()
    want_gain = (w[q.cpu().numpy() + 249] * table[utt.cpu().numpy()]).astype(np.float32)
    assert np.array_equal(gain.cpu().numpy().view(np.uint32), want_gain.view(np.uint32))
    m, s, _ = dynmix.gather(c, utt, start, torch.from_numpy(want_gain).to(DEV), SEG)
    assert torch.equal(m, mixture) and torch.equal(s, sources)
    assert float(mixture.abs().max()) > 0.5
