"""No GPU: the streaming sinc resampler's host side -- the numpy streaming oracle against the one-shot oracle (bitwise), the
E(N) arithmetic of resample.plan_stream_resample, the remainder / hop accounting of ResamplingStreamPool, and the errors that
are raised before anything touches a device."""
import ctypes
import math

import numpy as np
import pytest
import torch

import resample_oracle as RO
import stream_resample_oracle as SO

import conv_tasnet_amd as ctn
from conv_tasnet_amd import resample
from conv_tasnet_amd.streaming import plan_rate_close, plan_rate_push

RATIOS = [(1, 2), (2, 1), (1, 6), (80, 441), (147, 160)]
ZEROS = [32, 8, 4]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _cuts(rng, W, total):
    """Seeded random cuts from {0, 1, 2, W - 1, W, W + 1, 37, 160} that sum to `total` (the last one is what is left)."""
    menu, cuts, left = [0, 1, 2, W - 1, W, W + 1, 37, 160], [], total
    while left:
        k = min(int(menu[rng.randint(len(menu))]), left)
        cuts.append(k)
        left -= k
    return cuts


@pytest.mark.parametrize("zeros", ZEROS)
@pytest.mark.parametrize("up,down", RATIOS)
def test_streaming_oracle_is_bitwise_the_one_shot_oracle(up, down, zeros):
    h, W = RO.design_filter(up, down, zeros=zeros)
    rng = np.random.RandomState(1000 * zeros + up + down)
    for total in (0, 1, W, W + 1, 2 * W, 3 * W + 211):
        x = (rng.randn(total) * 0.3).astype(np.float32)
        cuts = _cuts(rng, W, total)
        outs, tail, s = SO.run(x, cuts, up, down, h, W)
        got = np.concatenate(outs + [tail])
        want = RO.resample_f32(x, up, down, h, W) if total else np.zeros(0, np.float32)
        assert got.shape == want.shape == (RO.out_len(total, up, down),)
        assert np.array_equal(_bits(got), _bits(want)), (total, cuts)
        assert s.deepest <= 2 * W - 1
        at = 0
        for k, o in zip(cuts, outs):                            # a push that ends at N <= W samples emits nothing
            at += k
            assert at > W or len(o) == 0


@pytest.mark.parametrize("zeros", ZEROS)
@pytest.mark.parametrize("up,down", RATIOS)
def test_plan_stream_resample(up, down, zeros):
    _, W = resample.design_filter(up, down, zeros=zeros)
    rng = np.random.RandomState(7 * zeros + up)
    for total in (0, 1, W - 1, W, W + 1, 2 * W + 5, 2000):
        n, emitted, cuts = 0, 0, _cuts(rng, W, total)
        for k in cuts:
            t0, n_out = resample.plan_stream_resample(n, k, up, down, W)
            assert t0 == emitted == SO.ready(n, up, down, W) and n_out >= 0
            if n + k <= W:
                assert n_out == 0
            if n_out:
                assert (t0 * down) // up - W + 1 >= n - (2 * W - 1)              # the oldest sample read: inside the history
                assert ((t0 + n_out - 1) * down) // up + W <= n + k - 1          # the newest: has arrived
            if (n + k) > W:
                assert (((t0 + n_out) * down) // up + W > n + k - 1)             # and the next output's has not
            n += k
            emitted += n_out
        t0, n_out = resample.plan_stream_resample(n, 0, up, down, W, final=True)
        assert t0 == emitted and emitted + n_out == -((-total * up) // down) == resample.out_len(total, up, down)
        if n_out:
            assert (t0 * down) // up - W + 1 >= n - (2 * W - 1)
    # a push and the flush in one table row
    assert resample.plan_stream_resample(0, 5, up, down, W, final=True) == (0, resample.out_len(5, up, down))
    with pytest.raises(ValueError):
        resample.plan_stream_resample(-1, 5, up, down, W)


def test_algorithmic_latency_figures_of_the_docstring():
    for (a, b, zeros), ms in {(16000, 8000, 32): 4.25, (8000, 16000, 32): 4.25, (48000, 8000, 32): 4.23, (16000, 8000, 8): 1.06,
                              (48000, 8000, 8): 1.06}.items():
        up, down = resample.ratio(a, b)
        W = resample.design_filter(up, down, zeros=zeros)[1]
        assert round(1000.0 * W / a, 2) == ms
        assert "%.2f" % ms in resample.StreamResampler.__doc__


def test_remainder_and_hop_accounting():
    rng = np.random.RandomState(3)
    S, L = 10, 20
    for trial in range(200):
        rem = fed = total = 0
        for _ in range(int(rng.randint(0, 12))):
            new = int(rng.choice([0, 1, 3, 9, 10, 11, 81, 600]))
            hops, rem = plan_rate_push(rem, new, S)
            fed += hops
            total += new
            assert 0 <= rem < S and fed * S + rem == total
        flush = int(rng.choice([0, 1, 5, 17, 34]))                 # the input resampler's flush lands behind the remainder
        hops, pad = plan_rate_close(fed, rem + flush, S, L)
        n8 = total + flush
        if n8 == 0:
            assert (hops, pad) == (0, 0)
            continue
        padded = n8 + pad
        assert padded % S == 0 and padded >= L and padded == max(L, -(-n8 // S) * S) and 0 <= pad
        assert (fed + hops) * S == padded
    with pytest.raises(ValueError):
        plan_rate_push(10, 1, S)
    with pytest.raises(ValueError):
        plan_rate_push(0, -1, S)


def test_errors_without_a_gpu():
    with pytest.raises(ValueError):
        resample.StreamResampler(2, 0, 8000, 160)                   # bad rate
    with pytest.raises(ValueError):
        resample.StreamResampler(2, 16000, -8000, 160)
    with pytest.raises(ValueError):
        resample.StreamResampler(2, 16000, 8000, 160, zeros=0)      # bad zeros
    with pytest.raises(ValueError):
        resample.StreamResampler(2, 16000, 8000, 160, zeros=2.5)
    with pytest.raises(ValueError):
        resample.StreamResampler(3, 16000, 8000, 160, groups=2)     # rows not a multiple of groups
    with pytest.raises(ValueError):
        resample.StreamResampler(2, 16000, 8000, 0)
    with pytest.raises(ValueError):
        resample.StreamResampler(2, 16000, 8000, 160, device="cpu")
    r = resample.StreamResampler(2, 16000, 8000, 160)
    chunk = torch.zeros(2, 160)
    with pytest.raises(ValueError):
        r.push(chunk, [1, 0])                                       # row 0 is not open
    assert r.open(0) == 0
    with pytest.raises(ValueError):
        r.open(0)                                                   # already open
    with pytest.raises(ValueError):
        r.open(2)
    with pytest.raises(ValueError):
        r.push(chunk, [1])                                          # counts of the wrong length
    with pytest.raises(ValueError):
        r.push(chunk, [-1, 0])
    with pytest.raises(ValueError):
        r.push(chunk, [1, 1])                                       # row 1 is closed
    with pytest.raises(ValueError):
        r.close(1)
    with pytest.raises(ValueError, match="no CPU path"):
        r.push(chunk, [160, 0])                                     # a CPU tensor
    assert r.n == [0, 0] and r.is_open == [True, False]             # none of the refused calls touched the row


def test_c_entry_point_rejects_bad_arguments_before_any_launch():
    """Null pointers and a ratio not in lowest terms: rc == -1, nothing launched, so this is safe without a GPU."""
    rc = ctn.lib.ctn_stream_resample(0, 1, 0, 1, 1, 2, 0, 34, 0, 1, 0, 0, 0, 0)
    assert rc == -1 and b"null" in ctn.lib.ctn_last_error()
    buf = (ctypes.c_longlong * 64)()                                # stands in for every pointer: the checks come before any use
    p = ctypes.addressof(buf)
    rc = ctn.lib.ctn_stream_resample(p, 8, p, 1, 2, 4, p, 34, p, 8, p, p, 0, 0)
    assert rc == -1 and b"lowest terms" in ctn.lib.ctn_last_error()
    rc = ctn.lib.ctn_stream_resample(p, 8, p, 0, 1, 2, p, 34, p, 8, p, p, 0, 0)
    assert rc == -1 and b"rows" in ctn.lib.ctn_last_error()
    buf[1], buf[4] = 4, 6                                           # a row whose 4 new samples end beyond a chunk buffer of 8
    rc = ctn.lib.ctn_stream_resample(p, 8, p, 1, 1, 2, p, 34, p, 8, p, p, 0, 0)
    assert rc == -1 and b"row 0" in ctn.lib.ctn_last_error()
    assert math.gcd(2, 4) != 1
    rc = ctn.lib.ctn_stream_carry(0, 16, 1, p, 4, 0)
    assert rc == -1 and b"null" in ctn.lib.ctn_last_error()
    for ld, rows, n in ((16, 0, 4), (16, 1, 0), (16, 1, 1025), (3, 1, 4)):
        assert ctn.lib.ctn_stream_carry(p, ld, rows, p, n, 0) == -1 and b"ctn_stream_carry" in ctn.lib.ctn_last_error()
