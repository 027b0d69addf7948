"""GPU: the image-source room simulator (ctn_ism_simulate, rir.simulate) BITWISE against the numpy restatement in ism_oracle.py:
the uint64 views of h are compared, over rooms, tap counts and tables that reach every path of the kernel (a last chunk that is
not full, fewer taps than the interpolator is wide, spans cut at tap 0, dead walls, one and seven delay phases, the narrowest and
the widest interpolator, chunks whose images overflow the LDS list, several rooms and positions in one launch), then that a
response does not depend on its neighbours, and that a row the kernel finds broken is zeros with status -1."""
import numpy as np
import pytest
import torch

import ism_oracle as IO

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import rir  # noqa: E402

DEV = "cuda:0"
FS = 8000
SMALL = dict(L=[3.0, 2.5, 2.2], mic=[1.1, 1.3, 1.2], beta=[0.9, 0.85, 0.8, 0.75, 0.7, 0.6])
SMALL_SRC = [2.2, 0.9, 1.5]
BIG = dict(L=[6.0, 5.0, 3.0], mic=[0.6, 4.3, 0.7], beta=[0.93, 0.9, 0.88, 0.91, 0.8, 0.85])
BIG_SRC = [5.5, 0.6, 2.6]


def rooms_of(room_list, src_lists, fs=FS):
    """[room dict], [[src, ...] per room] -> the rooms dict of rir.draw_rooms"""
    return dict(L=np.array([r["L"] for r in room_list], np.float64), mic=np.array([r["mic"] for r in room_list], np.float64),
                beta=np.array([r["beta"] for r in room_list], np.float64), src=np.array(src_lists, np.float64),
                rt60=np.zeros(len(room_list)), sample_rate=fs, positions=len(src_lists[0]))


def frac_of(tb):
    return tb["tables"][-tb["Q"] * 2 * tb["W"]:].reshape(tb["Q"], 2 * tb["W"])


def oracle(rooms, tb):
    G, P = rooms["src"].shape[:2]
    return np.stack([IO.simulate(dict(L=rooms["L"][g], mic=rooms["mic"][g], beta=rooms["beta"][g]), rooms["src"][g, p], tb["n_taps"],
                                 rooms["sample_rate"], IO.C_SOUND, tb["Q"], tb["W"], frac=frac_of(tb))
                     for g in range(G) for p in range(P)])


def assert_bitwise(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64, (what, got.shape, want.shape, got.dtype)
    bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))
    assert len(bad[0]) == 0, "%s: %d of %d taps differ in their bits, the first at %s: %r against %r" % (
        what, len(bad[0]), want.size, tuple(int(b[0]) for b in bad), got[tuple(b[0] for b in bad)], want[tuple(b[0] for b in bad)])


def run(rooms, n_taps, Q=1024, W=8):
    tb = rir.ism_tables(rooms, n_taps, Q, W)
    h, status = rir.simulate_tables(tb, DEV)
    assert status.cpu().tolist() == [0] * tb["R"]
    return tb, h


CASES = {
    "six walls, 1024 taps": (SMALL, SMALL_SRC, 1024, 1024, 8),
    "six walls, 1000 taps": (SMALL, SMALL_SRC, 1000, 1024, 8),                       # the last chunk is not full
    "5 taps": (SMALL, [1.15, 1.36, 1.24], 5, 1024, 8),                               # fewer taps than 2W; the source 8.8 cm away
    "source 3 cm away": (SMALL, [1.12, 1.32, 1.21], 600, 1024, 8),                   # i = 0 < W: the spans are cut at tap 0
    "dead walls": (dict(SMALL, beta=[0.0] * 6), SMALL_SRC, 600, 1024, 8),
    "one dead wall": (dict(SMALL, beta=[0.9, 0.85, 0.0, 0.75, 0.7, 0.6]), SMALL_SRC, 600, 1024, 8),
    "Q = 1": (SMALL, SMALL_SRC, 600, 1, 8),
    "Q = 7": (SMALL, SMALL_SRC, 600, 7, 8),
    "W = 1": (SMALL, SMALL_SRC, 600, 1024, 1),
    "W = 32": (SMALL, SMALL_SRC, 600, 1024, 32),
}


@pytest.mark.parametrize("name", list(CASES))
def test_one_response_bitwise(name):
    room, src, n_taps, Q, W = CASES[name]
    rooms = rooms_of([room], [[src]])
    tb, h = run(rooms, n_taps, Q, W)
    want = oracle(rooms, tb)
    assert np.count_nonzero(want) >= min(n_taps, 2 * W) // 2, "the case is empty"
    assert_bitwise(h, want, name)
    assert_bitwise(rir.simulate(rooms, DEV, n_taps, Q, W), want, name + " (rir.simulate)")


def test_list_overflow_bitwise():
    """6 x 5 x 3 m at 3000 taps: about 99 000 contributing images, and chunks that need more images than the LDS list holds, so
    the list is drained and refilled in the middle of a walk.  The capacity is the one the library exports."""
    n_taps, W = 3000, 8
    rooms = rooms_of([BIG], [[BIG_SRC]])
    tb = rir.ism_tables(rooms, n_taps)
    im = IO.images(BIG, BIG_SRC, n_taps, FS)
    live = (im["i"] < n_taps) & (im["amp"] != 0)
    cap, chunk = ctn.lib.ctn_ism_list_capacity(), ctn.lib.ctn_ism_chunk_taps()
    need = [int(np.sum(live & (im["i"] + W >= k0) & (im["i"] - W + 1 < min(k0 + chunk, n_taps)))) for k0 in range(0, n_taps, chunk)]
    assert cap >= 256 and chunk >= 1 and max(need) > 2 * cap, (cap, chunk, need)
    stats = torch.zeros(2, dtype=torch.int64, device=DEV)
    h, status = rir.simulate_tables(tb, DEV, stats=stats)
    assert status.cpu().tolist() == [0]
    assert_bitwise(h, oracle(rooms, tb), "list overflow")
    visited, contributing = stats.cpu().tolist()
    assert contributing == int(live.sum()) and 90000 < contributing < 110000
    assert contributing <= visited <= im["amp"].size * len(need)          # never more than the whole lattice per chunk
    print("6 x 5 x 3 m, 3000 taps: %d images contribute, %d lattice entries visited (%.2f each), the fullest chunk needs %d"
          % (contributing, visited, visited / contributing, max(need)))


ROOMS3 = [SMALL, dict(L=[4.5, 3.2, 2.6], mic=[2.0, 1.0, 1.4], beta=[0.7, 0.75, 0.8, 0.85, 0.5, 0.9]),
          dict(L=[2.4, 5.1, 3.1], mic=[0.5, 4.4, 2.5], beta=[0.95, 0.6, 0.9, 0.65, 0.85, 0.7])]
SRC3 = [[[2.2, 0.9, 1.5], [0.6, 2.0, 0.5], [1.4, 1.3, 2.0]], [[3.9, 2.7, 0.8], [0.5, 0.5, 2.1], [2.1, 1.1, 1.5]],
        [[1.9, 0.6, 0.7], [0.6, 4.0, 2.4], [1.2, 2.5, 1.5]]]


@pytest.fixture(scope="module")
def bank3():
    rooms = rooms_of(ROOMS3, SRC3)
    tb, h = run(rooms, 700)
    return rooms, tb, h.cpu().numpy()


def test_rooms_and_positions_in_one_launch(bank3):
    rooms, tb, h = bank3
    assert h.shape == (9, 700)
    assert_bitwise(h, oracle(rooms, tb), "three rooms of three positions")


def test_a_response_does_not_depend_on_its_neighbours(bank3):
    _, _, h = bank3
    for g, p in ((0, 0), (1, 2), (2, 1)):                                            # alone
        _, alone = run(rooms_of([ROOMS3[g]], [[SRC3[g][p]]]), 700)
        assert_bitwise(alone, h[3 * g + p][None], "response (%d, %d) alone" % (g, p))
    _, rev = run(rooms_of(ROOMS3[::-1], [s[::-1] for s in SRC3[::-1]]), 700)        # in another order
    assert_bitwise(rev, h[::-1].copy(), "rooms and positions reversed")
    _, flat = run(rooms_of([ROOMS3[g] for g in range(3) for _ in range(3)], [[SRC3[g][p]] for g in range(3) for p in range(3)]), 700)
    assert_bitwise(flat, h, "nine rooms of one position")                            # in another grouping


def test_a_broken_row_is_zeros_and_its_neighbours_are_untouched(bank3):
    """The host copy is sound, so the launch happens; the device copy holds rows only the kernel's own checks can find."""
    rooms, tb, h = bank3
    G, R, K = tb["G"], tb["R"], tb["K"]
    resp0 = G * 16 + G * 6 * K
    for what, index, value, rows in (("a source outside its room", resp0 + 4 * 4 + 2, 9.0, [4]),
                                     ("a source on a wall", resp0 + 4 * 0 + 1, 0.0, [0]),
                                     ("a room index beyond the bank", resp0 + 4 * 8, 3.0, [8]),
                                     ("a NaN coordinate", resp0 + 4 * 7 + 3, float("nan"), [7]),
                                     ("a wall coefficient above 1 (the whole room)", 16 * 1 + 6 + 2, 1.25, [3, 4, 5]),
                                     ("lattice bounds beyond the power table", 16 * 2 + 12, K - 1.0, [6, 7, 8])):
        dev = torch.from_numpy(tb["tables"]).to(DEV)
        dev[index] = value
        out = torch.full((R, 700), float("nan"), dtype=torch.float64, device=DEV)
        got, status = rir.simulate_tables(tb, DEV, tables_dev=dev, out=out)
        want = h.copy()
        want[rows] = 0.0
        assert status.cpu().tolist() == [-1 if r in rows else 0 for r in range(R)], what
        assert_bitwise(got, want, what)
