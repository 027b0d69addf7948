"""GPU: the integrated loudness meter (csrc/ctn_loudness.hip, loudness.py) against loudness_oracle.py at the library's chunk
length -- the three sums BITWISE, the four counts exactly --, its independence of neighbours, order and workspace grouping, the
flag for entries outside the buffer, the padded call, and level="loudness" through DeviceCorpus."""
import numpy as np
import pytest
import torch

import loudness_oracle as LO

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import dynmix, loudness  # noqa: E402

DEV = "cuda:0"
RATES = (8000, 16000)
HEAD = 37                            # samples in front of the first utterance: offsets are odd and not a running sum from 0
STATS = ("ns", "n_blocks", "n_abs", "n_rel")
SUMS = ("sum_all", "sum_abs", "sum_rel")
_WORLD = {}


def _world(fs):
    """The shared cases at one rate, their flat device buffer and the oracle's statistics, computed once."""
    if fs not in _WORLD:
        ch = int(loudness.lib.ctn_loudness_chunk())
        named = LO.cases(fs, ch)
        arrays = [x for _, x in named]
        lens = np.array([len(x) for x in arrays], dtype=np.int64)
        offsets = HEAD + np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64)
        flat = torch.from_numpy(np.concatenate([np.full(HEAD, 7.0, dtype=np.float32)] + arrays)).to(DEV)
        want = [LO.stats(x, fs, ch) for x in arrays]
        _WORLD[fs] = dict(names=[n for n, _ in named], arrays=arrays, lens=lens, offsets=offsets, flat=flat, want=want, ch=ch)
    return _WORLD[fs]


def _same(a, b, rows_a=None, rows_b=None, what=""):
    """The device statistics of rows_a of result a and rows_b of result b are the same bits."""
    ra = slice(None) if rows_a is None else rows_a
    rb = slice(None) if rows_b is None else rows_b
    for k in SUMS:
        assert np.array_equal(a[k][ra].view(np.uint64), b[k][rb].view(np.uint64)), (what, k)
    for k in STATS:
        assert np.array_equal(a[k][ra], b[k][rb]), (what, k)


@pytest.mark.parametrize("fs", RATES)
def test_statistics_are_the_oracles_bit_for_bit(fs):
    w = _world(fs)
    assert len(w["arrays"]) >= 12 and int(w["lens"].sum()) < 200000 and (w["offsets"] % 2 == 1).any()
    got = loudness.integrated_loudness_ragged(w["flat"], w["offsets"], w["lens"], fs)
    for u, (name, st) in enumerate(zip(w["names"], w["want"])):
        print("%-10s len %6d  blocks %3d/%3d/%3d (device %3d/%3d/%3d)  sum_rel %.17g (device %.17g)  %.3f LUFS" % (
            name, w["lens"][u], st["n_blocks"], st["n_abs"], st["n_rel"], got["n_blocks"][u], got["n_abs"][u], got["n_rel"][u],
            st["sum_rel"], got["sum_rel"][u], got["lufs"][u]))
    for u, (name, st) in enumerate(zip(w["names"], w["want"])):
        for k in STATS:
            assert got[k][u] == st[k], (name, k, got[k][u], st[k])
        for k in SUMS:
            assert np.float64(got[k][u]).view(np.uint64) == np.float64(st[k]).view(np.uint64), (name, k, got[k][u], st[k])
        lo = LO.loudness(st)
        assert got["power"][u] == lo["power"], name
        for k in ("lufs", "ungated"):
            assert got[k][u] == lo[k] or abs(got[k][u] - lo[k]) <= 1e-12, (name, k)
    names, h = w["names"], fs // 10
    blocks = dict(zip(names, got["n_blocks"].tolist()))
    assert [blocks[n] for n in ("n-1", "n", "n+h-1", "n+h")] == [0, 1, 1, 2] and blocks["len1"] == 0
    assert all(blocks[n] >= 2 for n in ("kch-1", "kch", "kch+1"))
    lq = names.index("loud_quiet")
    assert 0 < got["n_rel"][lq] < got["n_abs"][lq] == got["n_blocks"][lq]                     # the relative gate bites
    for n in ("zeros", "below_abs"):
        u = names.index(n)
        assert got["n_blocks"][u] > 0 and got["n_abs"][u] == 0 and got["power"][u] == 0.0 and got["lufs"][u] == -np.inf
    assert got["sum_all"][names.index("below_abs")] > 0.0 and got["sum_all"][names.index("zeros")] == 0.0
    assert abs(got["lufs"][names.index("tone")] - (-3.0 + 20 * np.log10(0.5))) < 0.1         # a 997 Hz sine at half scale


@pytest.mark.parametrize("fs", RATES)
def test_an_utterance_does_not_depend_on_neighbours_order_or_grouping(fs):
    w = _world(fs)
    U = len(w["lens"])
    base = loudness.integrated_loudness_ragged(w["flat"], w["offsets"], w["lens"], fs)
    for u in range(U):                                                          # alone
        one = loudness.integrated_loudness_ragged(w["flat"], w["offsets"][u:u + 1], w["lens"][u:u + 1], fs)
        _same(one, base, None, slice(u, u + 1), "alone %s" % w["names"][u])
    order = np.random.default_rng(5).permutation(U)                             # another order (of the table: the buffer stays)
    perm = loudness.integrated_loudness_ragged(w["flat"], w["offsets"][order], w["lens"][order], fs)
    _same(perm, base, None, order, "permuted")
    nchunks = (w["lens"] + w["ch"] - 1) // w["ch"]
    total = int(loudness.lib.ctn_loudness_workspace(int(nchunks.sum()), U))
    seen = set()
    for bound in (total, total * 6 // 10, total // 4, 1):
        groups = len(loudness._groups(nchunks, bound))
        seen.add(groups)
        _same(loudness.integrated_loudness_ragged(w["flat"], w["offsets"], w["lens"], fs, workspace_bytes=bound), base,
              what="%d groups" % groups)
    assert 1 in seen and U in seen and len(seen) >= 3


def test_an_entry_outside_the_buffer_is_flagged_and_nothing_else_changes():
    fs = 8000
    w = _world(fs)
    base = loudness.integrated_loudness_ragged(w["flat"], w["offsets"], w["lens"], fs)
    assert (base["ns"] == w["lens"]).all()
    n = w["flat"].numel()
    for u, off in ((3, -1), (0, n - int(w["lens"][0]) + 1), (len(w["lens"]) - 1, n)):
        offsets = w["offsets"].copy()
        offsets[u] = off
        got = loudness.integrated_loudness_ragged(w["flat"], offsets, w["lens"], fs)
        keep = np.arange(len(offsets)) != u
        _same(got, base, keep, keep, "flag at %d" % u)
        assert got["ns"][u] == -1 and got["n_blocks"][u] == 0 and got["sum_all"][u] == 0.0 and got["power"][u] == 0.0
    lens = w["lens"].copy()
    lens[2] = -5
    got = loudness.integrated_loudness_ragged(w["flat"], w["offsets"], lens, fs)
    assert got["ns"][2] == -1
    keep = np.arange(len(lens)) != 2
    _same(got, base, keep, keep, "negative length")


def test_the_entry_point_refuses_what_it_cannot_run():
    w = _world(8000)
    d = loudness.design(8000)
    table = torch.from_numpy(d["table"]).to(DEV)
    i64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int64)).to(DEV)
    off, ln, cp = i64(w["offsets"][:1]), i64(w["lens"][:1]), i64([0, (int(w["lens"][0]) + w["ch"] - 1) // w["ch"]])
    out = torch.zeros(4, 1, dtype=torch.int64, device=DEV)
    sums = torch.zeros(3, 1, dtype=torch.float64, device=DEV)
    G = int(cp[1])
    ws = torch.zeros(int(loudness.lib.ctn_loudness_workspace(G, 1)), dtype=torch.uint8, device=DEV)
    args = lambda hop, nbytes: (w["flat"].data_ptr(), w["flat"].numel(), off.data_ptr(), ln.data_ptr(), cp.data_ptr(), 1, G, table.data_ptr(),
                                hop, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), sums[0].data_ptr(),
                                sums[1].data_ptr(), sums[2].data_ptr(), ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    for hop in (799, 4801):
        with pytest.raises(ctn.CtnError, match="hop = %d" % hop):
            loudness.lib.call("ctn_loudness", *args(hop, ws.numel()))
    with pytest.raises(ctn.CtnError, match="workspace"):
        loudness.lib.call("ctn_loudness", *args(800, ws.numel() - 1))
    with pytest.raises(ValueError):
        loudness.integrated_loudness_ragged(w["flat"], w["offsets"], w["lens"], 11025)
    with pytest.raises(ValueError):
        loudness.integrated_loudness_ragged(w["flat"].cpu(), w["offsets"], w["lens"], 8000)


@pytest.mark.parametrize("fs", RATES)
def test_padded_batch_equals_the_ragged_call(fs):
    w = _world(fs)
    rows = [u for u in range(len(w["lens"])) if w["lens"][u] <= 10000]
    T = int(max(w["lens"][u] for u in rows)) + 3
    x = np.full((len(rows) + 1, T), 9.0, dtype=np.float32)                      # what lies behind lengths[r] must not count
    for r, u in enumerate(rows):
        x[r, :w["lens"][u]] = w["arrays"][u]
    lengths = np.concatenate((w["lens"][rows], [0]))                            # and an empty row: no chunk at all
    got = loudness.integrated_loudness(torch.from_numpy(x).to(DEV), torch.from_numpy(lengths), fs)
    base = loudness.integrated_loudness_ragged(w["flat"], w["offsets"], w["lens"], fs)
    _same(got, base, slice(0, len(rows)), np.array(rows), "padded")
    assert np.array_equal(got["power"][:-1], base["power"][rows])
    assert got["ns"][-1] == 0 and got["n_blocks"][-1] == 0 and got["power"][-1] == 0.0
    empty = loudness.integrated_loudness(torch.zeros(2, 5, device=DEV), [0, 0], fs)                   # no chunk in the whole call
    assert empty["ns"].tolist() == [0, 0] and empty["n_blocks"].tolist() == [0, 0]


# ---- level="loudness" in the corpus ------------------------------------------------------------------------------------------
def test_device_corpus_takes_the_gated_loudness():
    fs = 8000
    w = _world(fs)
    keep = [u for u, n in enumerate(w["names"]) if n != "len1"]
    arrays = [w["arrays"][u] for u in keep]
    power = np.array([LO.loudness(w["want"][u])["power"] for u in keep])
    speakers = ["s%d" % (u % 4) for u in range(len(arrays))]
    c = ctn.DeviceCorpus.from_arrays(arrays, speakers, DEV, level="loudness", sample_rate=fs)
    want = dynmix.inverse_rms(power)
    assert np.array_equal(c.inv_rms.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert c.level == "loudness" and np.array_equal(c.level_power, power) and c.activity is None
    assert np.array_equal(np.isfinite(c.lufs), power > 0)
    silent = [i for i, u in enumerate(keep) if w["names"][u] in ("zeros", "below_abs", "n-1")]
    assert len(silent) == 3 and not want[silent].any() and (want[[i for i in range(len(keep)) if i not in silent]] > 0).all()
    host, _, _ = c.tables(1000, 2)
    assert not set(silent) & set(host["utt_ids"].tolist())                    # no loudness: never eligible
    # an utterance times inv_rms reads -0.691 LUFS: unit gated power (float32 samples: to 1e-5 dB)
    u = keep.index(w["names"].index("loud_quiet"))
    scaled = (arrays[u] * want[u]).astype(np.float32)
    again = loudness.integrated_loudness_ragged(torch.from_numpy(scaled).to(DEV), [0], [len(scaled)], fs)
    assert abs(again["lufs"][0] - (-0.691)) < 1e-4
    with pytest.raises(ValueError):
        ctn.DeviceCorpus.from_arrays(arrays, speakers, DEV, level="loudness")     # no rate
    with pytest.raises(ValueError):
        ctn.DeviceCorpus.from_arrays(arrays, speakers, DEV, level="loudness", sample_rate=11025)
    r = ctn.DeviceCorpus.from_arrays(arrays, speakers, DEV)
    assert r.level == "rms" and r.lufs is None and r.level_power is r.meansq
