"""CPU-only checks of the long-recording path: the segment arithmetic, the cross-fade tables, the contract's own consistency
through its numpy restatement (longform_oracle.py: sources cut into segments with a drawn speaker order per segment come back
in segment 0's order), the tie rule, and the argument checks that sit in front of every launch."""
import itertools

import numpy as np
import pytest
import torch

import longform_oracle as LO

import conv_tasnet_amd as ctn
from conv_tasnet_amd import _lib, longform

GEOMETRIES = [(8, 4), (64, 63), (96, 56)]
ENTRY_POINTS = ["ctn_longform_nseg", "ctn_longform_frame", "ctn_longform_costs", "ctn_longform_order", "ctn_longform_assemble"]
# (seg, hop, T, C)
RECONSTRUCTIONS = [(64, 32, 200, 2), (96, 56, 301, 3), (64, 40, 64, 2), (64, 40, 65, 2), (600, 300, 2000, 4), (520, 263, 1700, 2)]


@pytest.mark.parametrize("seg,hop", GEOMETRIES)
def test_segment_counts_cover_the_recording_and_pad_only_the_last_segment(seg, hop):
    for T in range(1, 4 * seg + 1):
        n = LO.n_segments(T, seg, hop)
        assert n == (1 if T <= seg else 1 + -((seg - T) // hop))
        assert (n - 1) * hop + seg >= T                          # the segments cover the recording
        assert (n - 1) * hop < T                                 # the last segment starts inside it
        if n >= 2:
            assert (n - 2) * hop + seg < T                       # the one before it is not padded
        assert longform.plan_segments(T, seg, hop) == n == ctn.lib.ctn_longform_nseg(T, seg, hop)
        assert LO.frame(np.ones(T, np.float32), seg, hop).shape == (n, seg)
    assert ctn.lib.ctn_longform_nseg(0, seg, hop) == 0 and ctn.lib.ctn_longform_nseg(10, hop, hop) == 0


@pytest.mark.parametrize("window", ["linear", "hann"])
def test_fade_tables_sum_to_one_and_ascend(window):
    for ov in (1, 2, 4, 7, 1023, 1024, 16000):
        fi, fo = longform.fade_tables(ov, window)
        wi, wo = LO.fade_tables(ov, window)
        assert fi.dtype == fo.dtype == np.float32 and fi.shape == fo.shape == (ov,)
        assert np.array_equal(fi, wi) and np.array_equal(fo, wo)
        assert np.all(np.abs(fi.astype(np.float64) + fo.astype(np.float64) - 1.0) <= 2.0 ** -24)
        assert np.all(np.diff(fi) >= 0) and 0.0 < fi[0] and fi[-1] <= 1.0 and (ov == 1 or fi[0] < fi[-1])
    with pytest.raises(ValueError):
        longform.fade_tables(0)
    with pytest.raises(ValueError):
        longform.fade_tables(4, "triangle")


@pytest.mark.parametrize("seg,hop,T,C", RECONSTRUCTIONS)
@pytest.mark.parametrize("window", ["linear", "hann"])
def test_sources_in_drawn_orders_come_back_in_the_order_of_segment_zero(seg, hop, T, C, window):
    """|out[t] - x[t]| <= 4 * 2^-24 * |x[t]|: the table rounding gives |fi + fo - 1| <= 2^-24, and the two products and the sum
    give 2^-24 each."""
    rng = np.random.default_rng(seg * 1000 + T + C)
    src = rng.standard_normal((C, T)).astype(np.float32)
    est, local = LO.permuted_segments(src, seg, hop, rng)
    out, g, cost = LO.stitch(est, T, hop, window)
    assert np.array_equal(g, local)
    assert out.shape == (C, T) and out.dtype == np.float32
    err = np.abs(out.astype(np.float64) - src.astype(np.float64))
    bound = 4.0 * 2.0 ** -24 * np.abs(src.astype(np.float64))
    print("worst error / bound: %.3f" % float((err / np.maximum(bound, 1e-300)).max()))
    assert np.all(err <= bound)
    assert np.all(cost[0] == 0) and cost.shape == (len(est), C, C)


def test_an_exact_tie_takes_the_first_permutation():
    rng = np.random.default_rng(3)
    seg, hop, T = 64, 40, 150
    for C in (2, 3, 4):
        src = rng.standard_normal((C, T)).astype(np.float32)
        est, _ = LO.permuted_segments(src, seg, hop, rng)
        est[1, 1, :seg - hop] = est[1, 0, :seg - hop]           # channels 0 and 1 of segment 1 are equal over the whole overlap
        cost = LO.costs(est, hop)
        assert np.array_equal(cost[1, :, 0], cost[1, :, 1])
        k, p = LO.best_perm(cost[1])
        sums = [sum(float(cost[1, a, q[a]]) for a in range(C)) for q in itertools.permutations(range(C))]
        ties = [i for i, v in enumerate(sums) if v == min(sums)]
        assert len(ties) >= 2 and k == ties[0]
    assert LO.best_perm(np.zeros((3, 3), np.float32)) == (0, (0, 1, 2))
    assert LO.best_perm(np.full((2, 2), np.nan, np.float32))[0] == 0


def test_cost_order_is_the_1024_partials_then_the_tree():
    rng = np.random.default_rng(0)
    for ov in (1, 4, 1023, 1024, 1025, 2049):
        a, b = rng.standard_normal(ov).astype(np.float32), rng.standard_normal(ov).astype(np.float32)
        q = (a - b) * (a - b)
        acc = [np.float32(0)] * 1024
        for t in range(ov):
            acc[t % 1024] = np.float32(acc[t % 1024] + q[t])
        s = 512
        while s:
            for j in range(s):
                acc[j] = np.float32(acc[j] + acc[j + s])
            s //= 2
        assert LO.cost_pair(a, b).view(np.uint32) == acc[0].view(np.uint32)
        # q carries three roundings, and an element passes through ceil(ov / 1024) + 10 additions
        exact = float(np.sum((a.astype(np.float64) - b.astype(np.float64)) ** 2))
        assert abs(float(acc[0]) - exact) <= (-(-ov // 1024) + 14) * 2.0 ** -24 * exact


def test_bad_geometry_and_speaker_counts_are_refused_without_a_device():
    assert not [n for n in ENTRY_POINTS if n not in _lib.parse_header()]
    for seg, hop in ((8, 8), (8, 9), (9, 4), (8, 0), (8.5, 4)):  # ov < 1, seg > 2 hop
        with pytest.raises(ValueError):
            longform.plan_segments(10, seg, hop)
        with pytest.raises(ValueError):
            longform.separate_long(lambda x: x, torch.zeros(100), seg, hop)
    with pytest.raises(ValueError):
        longform.plan_segments(0, 8, 4)
    m = ctn.ConvTasNet(16, 20, 8, 16, 3, 2, 1, 2)
    with pytest.raises(ValueError, match="multiples of L / 2"):  # L / 2 = 10
        longform.separate_long(m, torch.zeros(1000), 205, 110)
    with pytest.raises(ValueError, match="multiples of L / 2"):
        longform.separate_long(m, torch.zeros(1000), 200, 105)
    with pytest.raises(ValueError, match="speakers"):
        longform.separate_long(ctn.ConvTasNet(16, 20, 8, 16, 3, 2, 1, 5), torch.zeros(1000), 200, 100)
    with pytest.raises(ValueError, match="GPU"):                 # there is no CPU path
        longform.separate_long(m, torch.zeros(1000), 200, 100)
    with pytest.raises(ValueError, match="GPU"):
        longform.frame_ragged(torch.zeros(100), [0], [100], 8, 4)
    with pytest.raises(ValueError, match="GPU"):
        longform.stitch_ragged(torch.zeros(3, 2, 8), [0, 3], [16], 4)

    lib, err = ctn.lib, ctn.lib.ctn_last_error
    p = 4096                                                     # fake non-null device pointers: never read
    sp = np.array([0, 3], dtype=np.int64)

    def costs(C=2, seg=8, hop=4, host=sp, est=p, Nseg=3):
        return lib.ctn_longform_costs(est, p, 1, Nseg, C, seg, hop, p, host.ctypes.data, 0)

    assert costs(est=0) == -1 and b"null" in err()
    assert costs(C=5) == -1 and b"speakers" in err()
    assert costs(C=1) == -1 and b"speakers" in err()
    assert costs(seg=8, hop=8) == -1 and b"seg - hop" in err()
    assert costs(seg=9, hop=4) == -1 and b"seg - hop" in err()
    assert costs(Nseg=4) == -1 and b"seg_ptr" in err()
    assert lib.ctn_longform_order(p, p, 1, 3, 5, p, sp.ctypes.data, 0, 0) == -1 and b"speakers" in err()
    assert lib.ctn_longform_order(p, p, 1, 3, 2, p, np.array([1, 3], np.int64).ctypes.data, 0, 0) == -1 and b"seg_ptr" in err()

    def frame(T=16, off=0, x_samples=16, n=3, seg=8, hop=4):
        host = np.array([0, n, T, off], dtype=np.int64)
        return lib.ctn_longform_frame(p, x_samples, p, p, p, 1, n, seg, hop, p, host.ctypes.data, 0, 0)

    assert frame(off=1) == -1 and b"outside the input buffer" in err()
    assert frame(off=-1) == -1 and b"outside the input buffer" in err()
    assert frame(T=17) == -1 and b"segments" in err()            # 17 samples are 4 segments
    assert frame(T=0) == -1 and b"samples" in err()
    assert frame(seg=8, hop=3) == -1 and b"seg - hop" in err()

    def assemble(T=16, off=0, out_samples=32, n=3, C=2):
        host = np.array([0, n, T, off], dtype=np.int64)
        return lib.ctn_longform_assemble(p, p, p, p, p, 1, n, C, 8, 4, p, p, p, out_samples, host.ctypes.data, 0, 0)

    assert assemble(off=1) == -1 and b"outside the output buffer" in err()
    assert assemble(out_samples=31) == -1 and b"outside the output buffer" in err()
    assert assemble(n=2) == -1 and b"segments" in err()
    assert assemble(C=5) == -1 and b"speakers" in err()


def test_separate_keeps_its_defaults_and_has_the_new_arguments():
    import inspect
    from conv_tasnet_amd import separate as sep
    sig = inspect.signature(sep.separate)
    assert sig.parameters["segment"].default is None and sig.parameters["hop"].default is None
    assert list(sig.parameters)[:8] == ["model_path", "mix_dir", "mix_json", "out_dir", "use_cuda", "sample_rate", "batch_size", "file_rate"]
    called = {}
    orig = sep.separate
    try:
        sep.separate = lambda *a, **k: called.update(a=a, k=k)
        sep.main(["--model-path", "m", "--mix-dir", "d", "--out-dir", "o", "--segment-s", "4", "--hop-s", "2.5"])
        assert called["k"]["segment"] == 32000 and called["k"]["hop"] == 20000
        sep.main(["--model-path", "m", "--mix-dir", "d", "--out-dir", "o", "--sample-rate", "16000", "--segment-s", "4"])
        assert called["k"]["segment"] == 64000 and called["k"]["hop"] is None
        sep.main(["--model-path", "m", "--mix-dir", "d", "--out-dir", "o"])
        assert called["k"]["segment"] is None and called["k"]["hop"] is None
    finally:
        sep.separate = orig
