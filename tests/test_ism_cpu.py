"""CPU-only: the numpy oracle of the image-source room simulator (ism_oracle.py) checked against what the method must give, the
host side of the new Python surface (rir.draw_rooms, rir.design_fractional_delay, rir.ism_tables), the plan oracle of same_room,
and the argument checks of ctn_ism_simulate / ctn_dynmix_plan_rooms that run before any launch.

Limits.  Mirror symmetry: the two runs hold the same real numbers summed in another order, 1e-12 * sum |amp| per tap (fp64 sums of
a few thousand terms).  The fractional-delay table against exact delays: the delay error of the floor phase is below 1 / Q of a
sample and |d/dx| of the Hann-windowed sinc is at most 1.372 + pi / (2 W) (|sinc'| <= 0.4362 * pi, the window's slope at most
pi / (2 W)), 1.57 at W = 8: at most 1.6 / Q times the sum of |amp| of the images touching the tap."""
import ctypes

import numpy as np
import pytest

import ism_oracle as IO

import conv_tasnet_amd as ctn
from conv_tasnet_amd import rir

FS = 8000
ROOM = dict(L=[3.0, 2.5, 2.2], mic=[1.1, 1.3, 1.2], beta=[0.9, 0.85, 0.8, 0.75, 0.7, 0.6])
SRC = [2.2, 0.9, 1.5]
N_TAPS = 512


@pytest.fixture(scope="module")
def h_ref():
    return IO.simulate(ROOM, SRC, N_TAPS, FS)


def test_vectorised_oracle_is_the_loop_bitwise():
    room = dict(L=[2.0, 1.8, 1.6], mic=[0.7, 0.9, 0.8], beta=[0.9, 0.5, 0.8, 0.0, 0.7, 0.6])
    a = IO.simulate(room, [1.3, 0.6, 1.1], 100, FS, Q=16, W=3)
    b = IO.simulate_loop(room, [1.3, 0.6, 1.1], 100, FS, Q=16, W=3)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)) and np.abs(a).max() > 0


def test_direct_path_is_the_largest_tap(h_ref):
    dist = np.sqrt(np.sum((np.array(SRC) - np.array(ROOM["mic"])) ** 2))
    first = int(np.argmax(np.abs(h_ref)))
    assert first in (int(np.floor(dist * FS / IO.C_SOUND)), int(np.floor(dist * FS / IO.C_SOUND)) + 1)


def test_dead_walls_leave_the_direct_image_alone():
    room = dict(ROOM, beta=[0.0] * 6)
    h = IO.simulate(room, SRC, N_TAPS, FS)
    dist = np.sqrt(np.sum((np.array(SRC, np.float64) - np.array(ROOM["mic"], np.float64)) ** 2))
    im = IO.images(room, SRC, N_TAPS, FS)
    live = np.nonzero(im["amp"])[0]
    assert len(live) == 1
    amp, i, q = im["amp"][live[0]], int(im["i"][live[0]]), int(im["q"][live[0]])
    assert abs(amp - 1.0 / (IO.FOUR_PI * dist)) <= 1e-15 and i == int(np.floor(dist * FS / IO.C_SOUND))
    want = np.zeros(N_TAPS)
    want[i - 8 + 1:i + 8 + 1] = amp * IO.fractional_delay(1024, 8)[q]
    assert np.array_equal(h.view(np.uint64), want.view(np.uint64))


def test_mirror_symmetry(h_ref):
    L = ROOM["L"][0]
    b = ROOM["beta"]
    room = dict(L=ROOM["L"], mic=[L - ROOM["mic"][0]] + ROOM["mic"][1:], beta=[b[1], b[0]] + b[2:])
    h = IO.simulate(room, [L - SRC[0]] + SRC[1:], N_TAPS, FS)
    _, s = IO.simulate_exact(ROOM, SRC, N_TAPS, FS)
    worst = float(np.max(np.abs(h - h_ref) / np.maximum(s, 1e-300)))
    print("mirror symmetry: max |dh| / sum |amp| = %.3e" % worst)
    assert np.all(np.abs(h - h_ref) <= 1e-12 * s)


@pytest.mark.parametrize("Q", [1, 7, 128, 1024])
def test_table_against_exact_delays(Q):
    n = 400
    exact, s = IO.simulate_exact(ROOM, SRC, n, FS, W=8)
    h = IO.simulate(ROOM, SRC, n, FS, Q=Q, W=8)
    ratio = float(np.max(np.abs(h - exact) / np.maximum(s, 1e-300)) * Q)
    print("Q = %d: max |h - exact| / sum |amp| = %.3f / Q" % (Q, ratio))
    assert np.all(np.abs(h - exact) <= 1.6 / Q * s)


def test_fractional_delay_design():
    for Q, W in ((1, 1), (7, 3), (1024, 8), (5, 32)):
        f = rir.design_fractional_delay(Q, W)
        assert f.shape == (Q, 2 * W) and f.dtype == np.float64
        assert np.array_equal(f.view(np.uint64), IO.fractional_delay(Q, W).view(np.uint64))
        # no delay: the unit impulse at tap i.  numpy's sinc of a whole number x is not an exact zero: the argument pi * x carries a
        # relative error of up to 2^-52 (pi's rounding and the product's), so |sin| <= pi x 2^-52 and |sinc| <= 2^-52
        assert f[0, W - 1] == 1.0 and np.all(np.abs(np.delete(f[0], W - 1)) <= 2.0 ** -52)
    assert rir.design_fractional_delay(4, 2)[2, 1] == pytest.approx(np.sinc(-0.5) * 0.5 * (1 + np.cos(np.pi * 0.25)))
    for bad in ((0, 8), (4097, 8), (8, 0), (8, 33)):
        with pytest.raises(ValueError):
            rir.design_fractional_delay(*bad)


def test_draw_rooms_is_reproducible_and_meets_its_constraints():
    kw = dict(rt60=(0.2, 0.6), dims=((3, 3, 2.5), (10, 8, 4)), distance=(0.5, 3.0), margin=0.5)
    a = rir.draw_rooms(12, 4, FS, seed=3, epoch=2, **kw)
    b = rir.draw_rooms(12, 4, FS, seed=3, epoch=2, **kw)
    c = rir.draw_rooms(12, 4, FS, seed=3, epoch=3, **kw)
    for k in ("L", "mic", "beta", "src", "rt60"):
        assert np.array_equal(a[k], b[k]) and a[k].dtype == np.float64
    assert not np.array_equal(a["L"], c["L"]) and not np.array_equal(a["src"], rir.draw_rooms(12, 4, FS, seed=4, epoch=2, **kw)["src"])
    assert a["positions"] == 4 and a["sample_rate"] == FS and a["src"].shape == (12, 4, 3)
    assert np.all(a["L"] >= [3, 3, 2.5]) and np.all(a["L"] <= [10, 8, 4])
    assert np.all(a["mic"] >= 0.5) and np.all(a["mic"] <= a["L"] - 0.5)
    assert np.all(a["src"] >= 0.5) and np.all(a["src"] <= a["L"][:, None, :] - 0.5)
    dist = np.sqrt(np.sum((a["src"] - a["mic"][:, None, :]) ** 2, axis=-1))
    assert np.all(dist >= 0.5) and np.all(dist <= 3.0)
    for g in range(12):
        for p in range(4):
            for o in range(p):
                assert np.sqrt(np.sum((a["src"][g, p] - a["src"][g, o]) ** 2)) >= 0.3
    V, S = np.prod(a["L"], axis=1), 2 * (a["L"][:, 0] * a["L"][:, 1] + a["L"][:, 1] * a["L"][:, 2] + a["L"][:, 0] * a["L"][:, 2])
    assert np.all((a["rt60"] >= 0.2) & (a["rt60"] <= 0.6))
    assert np.allclose(a["beta"], np.sqrt(np.exp(-0.161 * V / (S * a["rt60"])))[:, None], rtol=1e-12) and np.all(a["beta"] < 1)
    with pytest.raises(ValueError):                                     # twelve sources 0.3 m apart within 0.31 m of the microphone
        rir.draw_rooms(1, 12, FS, distance=(0.3, 0.31))
    with pytest.raises(ValueError):
        rir.draw_rooms(1, 2, FS, dims=((1, 1, 1), (2, 2, 2)), margin=0.5)


def test_tables_follow_the_contract():
    rooms = rir.draw_rooms(3, 2, FS, seed=5)
    tb = rir.ism_tables(rooms, n_taps=700, Q=7, W=3)
    G, R, K = tb["G"], tb["R"], tb["K"]
    assert (G, R, tb["Q"], tb["W"], tb["n_taps"]) == (3, 6, 7, 3, 700)
    t = tb["tables"]
    assert t.size == ctn.lib.ctn_ism_table_doubles(G, R, K, 7, 3) == G * 16 + G * 6 * K + R * 4 + 7 * 6
    room, pw = t[:G * 16].reshape(G, 16), t[G * 16:G * 16 + G * 6 * K].reshape(G, 6, K)
    resp = t[G * 16 + G * 6 * K:][:R * 4].reshape(R, 4)
    for g in range(G):
        N = IO.lattice_bounds(rooms["L"][g], 700, FS)
        assert list(room[g, 12:15]) == N and K >= max(N) + 2
        assert np.array_equal(pw[g].view(np.uint64), IO.power_table(rooms["beta"][g], K).view(np.uint64))
    assert list(resp[:, 0]) == [0, 0, 1, 1, 2, 2] and np.array_equal(resp[:, 1:], rooms["src"].reshape(R, 3))
    assert tb["fs_over_c"] == FS / 343.0 and tb["four_pi"] == 4 * np.pi
    assert rir.default_taps(rooms) == min(8192, int(np.ceil(rooms["rt60"].max() * FS)))
    assert ctn.lib.ctn_ism_table_doubles(0, 1, 4, 8, 8) == 0 and ctn.lib.ctn_ism_table_doubles(1, 1, 4, 4097, 8) == 0


def test_plan_oracle_same_room():
    for (B, C, G, P) in ((64, 2, 5, 2), (64, 3, 7, 8), (32, 4, 1, 4)):
        plan = IO.plan_rooms(seed=11, rank=1, epoch=2, step=3, B=B, C=C, G=G, P=P)
        room, pos = plan // P, plan % P
        assert np.all(room == room[:, :1]) and np.all((room >= 0) & (room < G))
        assert all(len(set(row)) == C for row in pos.tolist())
        if G > 1:
            assert len(set(room[:, 0].tolist())) > 1
    assert len({tuple(r) for r in (IO.plan_rooms(11, 1, 2, 3, 64, 3, 7, 8) % 8).tolist()}) > 8       # the positions vary too
    assert not np.array_equal(IO.plan_rooms(11, 1, 2, 3, 8, 2, 5, 4), IO.plan_rooms(11, 1, 2, 4, 8, 2, 5, 4))


def test_host_checks_run_before_any_launch():
    """Every error below is found on the host tables: CTN_ERR_ARG, nothing is launched (the device pointers are never used)."""
    lib = ctn.lib
    err = lambda: lib.ctn_last_error()
    rooms = rir.draw_rooms(2, 2, FS, seed=1)
    tb = rir.ism_tables(rooms, n_taps=256)
    fake = ctypes.c_void_p(64)

    def call(t=None, **kw):
        a = dict(tb, **kw)
        t = a["tables"] if t is None else t
        return lib.ctn_ism_simulate(t.ctypes.data, fake, a["G"], a["R"], a["K"], a["Q"], a["W"], a["n_taps"], float(a["fs_over_c"]),
                                    float(a["four_pi"]), fake, fake, None, None)

    assert call(n_taps=0) == -1 and b"n_taps" in err()
    assert call(n_taps=8193) == -1 and call(Q=0) == -1 and call(Q=4097) == -1 and call(W=33) == -1 and call(G=0) == -1
    assert call(fs_over_c=0.0) == -1 and call(four_pi=float("nan")) == -1
    assert lib.ctn_ism_simulate(None, fake, 2, 4, tb["K"], 1024, 8, 256, 1.0, 1.0, fake, fake, None, None) == -1
    G, K = tb["G"], tb["K"]
    resp0 = G * 16 + G * 6 * K

    def broken(index, value):
        t = tb["tables"].copy()
        t[index] = value
        return t
    near = tb["tables"].copy()                             # response 1 (room 0) half a millimetre from its microphone
    near[resp0 + 5:resp0 + 8] = near[3:6] + [5e-4, 0, 0]
    cases = {"source on a wall": broken(resp0 + 4 + 1, 0.0), "source outside": broken(resp0 + 4 + 2, 1e3),
             "source at the microphone": near,
             "beta above 1": broken(6, 1.5), "beta negative": broken(16 + 11, -0.1), "beta NaN": broken(7, np.nan),
             "room index": broken(resp0, 2.0), "room index not whole": broken(resp0, 0.5), "L = 0": broken(1, 0.0),
             "N beyond the powers": broken(12, K - 1.0), "N not whole": broken(13, 2.5), "microphone outside": broken(16 + 3, -1.0)}
    for name, t in cases.items():
        assert call(t) == -1 and b"breaks its tables" in err(), name
    step = ctypes.c_void_p(64)
    assert lib.ctn_dynmix_plan_rooms(0, 0, 0, step, 4, 3, 2, 2, fake, None) == -1 and b"P = 2" in err()
    assert lib.ctn_dynmix_plan_rooms(0, 0, 0, step, 4, 2, 2, 65, fake, None) == -1
    assert lib.ctn_dynmix_plan_rooms(0, 0, 0, step, 4, 2, 0, 4, fake, None) == -1
    assert lib.ctn_dynmix_plan_rooms(0, 0, 0, None, 4, 2, 2, 4, fake, None) == -1 and b"null" in err()
    assert lib.ctn_dynmix_plan_rooms(1 << 48, 0, 0, step, 4, 2, 2, 4, fake, None) == -1


def test_loader_arguments_are_checked_without_a_gpu():
    from conv_tasnet_amd import dynmix, train
    assert train.parse_rooms("rooms:16") == (16, 4) and train.parse_rooms("rooms:16:2") == (16, 2)
    for bad in ("rooms:", "rooms:0", "rooms:4:65", "rooms:4:2:1", "room:4"):
        with pytest.raises(ValueError):
            train.parse_rooms(bad)
    a = train.build_parser().parse_args(["--rirs", "rooms:8:3", "--rt60", "0.3:0.5", "--rooms-refresh"])
    assert a.rirs == "rooms:8:3" and train.parse_snr(a.rt60) == (0.3, 0.5) and a.rooms_refresh

    class Bank:                                            # what _Augment reads of a bank before it touches the device
        device, num_responses, full_targets, positions_per_room = "cuda:0", 8, True, None
    with pytest.raises(ValueError, match="positions_per_room"):
        dynmix._Augment(2, 2, 100, "cuda:0", Bank(), None, (-6, 3), same_room=True)
    Bank.positions_per_room = 3                            # 8 responses are no whole number of rooms of 3
    with pytest.raises(ValueError, match="positions per room"):
        dynmix._Augment(2, 2, 100, "cuda:0", Bank(), None, (-6, 3), same_room=True)
    Bank.positions_per_room = 2
    with pytest.raises(ValueError, match="positions per room"):
        dynmix._Augment(2, 3, 100, "cuda:0", Bank(), None, (-6, 3), same_room=True)
