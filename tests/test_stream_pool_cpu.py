"""CPU-only checks of the streaming slot pool: the ragged entry points of csrc/ctn_stream.hip (ABI surface, argument errors in front of
the first launch) and `plan_steps`, the host function that cuts a ragged push into per-slot step tables."""
import ctypes
import random
import subprocess

import conv_tasnet_amd as ctn
from conv_tasnet_amd import _lib
from conv_tasnet_amd.streaming import TAB, plan_steps

RAGGED_ENTRY_POINTS = ["ctn_stream_load_ragged", "ctn_stream_front_ragged", "ctn_stream_tcn_cln_ragged", "ctn_stream_back_ragged",
                       "ctn_stream_store_ragged", "ctn_stream_reset_slots"]


def _ints(*d):
    return (ctypes.c_int * len(d))(*d)


def test_header_declares_and_library_exports_the_ragged_entry_points():
    protos = _lib.parse_header()
    assert not [n for n in RAGGED_ENTRY_POINTS if n not in protos]
    out = subprocess.run(["nm", "-D", "--defined-only", ctn.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert not [n for n in RAGGED_ENTRY_POINTS if n not in exported]
    assert all(protos[n][0] is ctypes.c_int for n in RAGGED_ENTRY_POINTS)
    assert protos["ctn_stream_tcn_cln_ragged"][2] == ["packed", "dilation", "nblocks", "y", "state", "tab", "pos", "M", "B", "H", "P",
                                                      "frames", "max_frames", "stream"]
    # the ragged calls take the arguments of the plain ones plus the table (and the position array)
    for plain, extra in (("ctn_stream_front", ["tab"]), ("ctn_stream_back", ["tab"]), ("ctn_stream_tcn_cln", ["tab", "pos"])):
        assert sorted(protos[plain + "_ragged"][2]) == sorted(protos[plain][2] + extra)
    assert "#define CTN_STREAM_TAB %d" % TAB in open(_lib.HEADER).read()
    from conv_tasnet_amd.streaming import FusedStreamPool
    assert ctn.FusedStreamPool is FusedStreamPool


def test_bad_arguments_return_error_codes_and_launch_nothing():
    # every check sits in front of the first launch, so this is safe without a GPU (fake non-null pointers are never read)
    lib, err = ctn.lib, ctn.lib.ctn_last_error
    d, p = _ints(1, 2), 4096
    # null table / null position array
    assert lib.ctn_stream_tcn_cln_ragged(p, d, 2, p, p, 0, p, 1, 16, 32, 3, 8, 16, 0) == -1 and b"tab" in err()
    assert lib.ctn_stream_tcn_cln_ragged(p, d, 2, p, p, p, 0, 1, 16, 32, 3, 8, 16, 0) == -1 and b"pos" in err()
    assert lib.ctn_stream_front_ragged(p, 100, p, p, p, p, p, p, 0, 1, 32, 20, 16, 4, 0) == -1 and b"tab" in err()
    assert lib.ctn_stream_back_ragged(p, p, p, p, p, p, p, p, 100, 0, 1, 32, 20, 16, 2, 4, 0, 0) == -1 and b"tab" in err()
    assert lib.ctn_stream_load_ragged(p, 100, 10, p, 170, 0, 2, 10, 17, 0) == -1 and b"tab" in err()
    assert lib.ctn_stream_store_ragged(p, p, 100, 0, 2, 2, 10, 4, 0) == -1 and b"tab" in err()
    assert lib.ctn_stream_tcn_cln_ragged(p, d, 2, 0, p, p, p, 1, 16, 32, 3, 8, 16, 0) == -1 and b"null" in err()
    # frames out of range
    assert lib.ctn_stream_tcn_cln_ragged(p, d, 2, p, p, p, p, 1, 16, 32, 3, 17, 16, 0) == -1 and b"max_frames" in err()
    assert lib.ctn_stream_tcn_cln_ragged(p, d, 2, p, p, p, p, 1, 16, 32, 3, 0, 16, 0) == -1 and b"max_frames" in err()
    assert lib.ctn_stream_front_ragged(p, 100, p, p, p, p, p, p, p, 1, 32, 20, 16, 0, 0) == -1 and b"frames" in err()
    assert lib.ctn_stream_front_ragged(p, 40, p, p, p, p, p, p, p, 1, 32, 20, 16, 4, 0) == -1 and b"sample buffer" in err()
    assert lib.ctn_stream_back_ragged(p, p, p, p, p, p, p, p, 40, p, 1, 32, 20, 16, 2, 4, 0, 0) == -1 and b"sample buffer" in err()
    assert lib.ctn_stream_back_ragged(p, p, p, p, p, p, p, p, 100, p, 1, 32, 20, 16, 2, 0, 0, 0) == -1 and b"frames" in err()
    assert lib.ctn_stream_store_ragged(p, p, 100, p, 2, 2, 10, 0, 0) == -1 and b"frames" in err()
    assert lib.ctn_stream_load_ragged(p, 100, 10, p, 170, p, 2, 10, 18, 0) == -1 and b"max_hops" in err()
    assert lib.ctn_stream_load_ragged(p, 90, 10, p, 170, p, 2, 10, 17, 0) == -1 and b"cld" in err()
    # widths that are no multiples of 16
    assert lib.ctn_stream_tcn_cln_ragged(p, d, 2, p, p, p, p, 1, 16, 40, 3, 8, 16, 0) == -1 and b"multiples of 16" in err()
    assert lib.ctn_stream_tcn_cln_ragged(p, d, 2, p, p, p, p, 1, 24, 32, 3, 8, 16, 0) == -1 and b"multiples of 16" in err()
    assert lib.ctn_stream_front_ragged(p, 100, p, p, p, p, p, p, p, 1, 24, 20, 16, 4, 0) == -1 and b"multiples of 16" in err()
    assert lib.ctn_stream_back_ragged(p, p, p, p, p, p, p, p, 100, p, 1, 32, 20, 24, 2, 4, 0, 0) == -1 and b"multiples of 16" in err()
    assert lib.ctn_stream_reset_slots(p, p, 170, p, p, _ints(0), 1, 4, 40, 3, d, 2, 16, 2, 20, 0) == -1 and b"multiple of 16" in err()
    # the rest of the checks of the plain calls
    assert lib.ctn_stream_tcn_cln_ragged(p, d, 2, p, p, p, p, 1, 16, 32, 9, 8, 16, 0) == -1 and b"kernel size" in err()
    assert lib.ctn_stream_tcn_cln_ragged(p, _ints(1, 0), 2, p, p, p, p, 1, 16, 32, 3, 8, 16, 0) == -1 and b"dilation" in err()
    assert lib.ctn_stream_tcn_cln_ragged(p, d, 2, p, p, p, p, 1, 512, 1024, 3, 8, 16, 0) == -1 and b"LDS" in err()
    assert lib.ctn_stream_back_ragged(p, p, p, p, p, p, p, p, 100, p, 1, 32, 20, 16, 2, 4, 2, 0) == -1 and b"mask" in err()
    # the reset list: a slot index out of range, an empty list, a null list
    assert lib.ctn_stream_reset_slots(p, p, 170, p, p, _ints(0, 4), 2, 4, 32, 3, d, 2, 16, 2, 20, 0) == -1 and b"slot 4" in err()
    assert lib.ctn_stream_reset_slots(p, p, 170, p, p, _ints(-1), 1, 4, 32, 3, d, 2, 16, 2, 20, 0) == -1 and b"slot -1" in err()
    assert lib.ctn_stream_reset_slots(p, p, 170, p, p, _ints(0), 0, 4, 32, 3, d, 2, 16, 2, 20, 0) == -1 and b"nslots" in err()
    assert lib.ctn_stream_reset_slots(p, p, 170, p, p, 0, 1, 4, 32, 3, d, 2, 16, 2, 20, 0) == -1 and b"null" in err()
    assert lib.ctn_stream_reset_slots(p, p, 170, p, 0, _ints(0), 1, 4, 32, 3, d, 2, 16, 2, 20, 0) == -1 and b"null" in err()
    try:
        ctn.lib.call("ctn_stream_tcn_cln_ragged", p, d, 2, p, p, p, p, 1, 16, 32, 3, 99, 16, 0)
    except ctn.CtnError as e:
        assert "max_frames" in str(e)
    else:
        raise AssertionError("no CtnError")


def _simulate(h, fresh, F):
    """One stream on its own: the pieces (hops, frames, landing offset) a push of h hops is cut into."""
    pieces = []
    while h:
        if fresh:
            n = min(h, F + 1)
            pieces.append((n, n - 1, 0))
            fresh = False
        else:
            n = min(h, F)
            pieces.append((n, n, 1))
        h -= n
    return pieces


def test_plan_steps_against_a_per_stream_simulation():
    rng = random.Random(7)
    seen = set()
    for trial in range(200):
        F = rng.choice([1, 2, 5, 16])
        M = rng.randint(1, 9)
        hops = [rng.choice([0, 0, 1, 1, 2, F, F + 1, F + 2, 2 * F + 1, rng.randint(0, 4 * F + 5)]) for _ in range(M)]
        fresh = [rng.random() < 0.5 for _ in range(M)]
        before = list(hops), list(fresh)
        steps = plan_steps(hops, fresh, F)
        assert (list(hops), list(fresh)) == before                  # pure: the arguments are left alone
        assert (steps == []) == (not any(hops))
        for m in range(M):
            rows = [rows[m] for _, _, rows in steps]
            assert all(len(r) == TAB and r[5:] == [0, 0, 0] for r in rows)
            pieces = [(r[1], r[0], r[3]) for r in rows if r[1]]
            assert pieces == _simulate(hops[m], fresh[m], F)         # same pieces, in the first steps, nothing after them
            assert all(r[0] == 0 for r in rows if not r[1])
            assert [bool(r[1]) for r in rows] == sorted([bool(r[1]) for r in rows], reverse=True)
            assert sum(r[1] for r in rows) == hops[m]                # the hops consumed sum to hops[m]
            assert sum(r[1] - r[0] for r in rows) == (1 if fresh[m] and hops[m] else 0)    # hops - 1 frames exactly once, if fresh
            src = out = 0
            for nf, nh, s, dst, o in (r[:5] for r in rows):
                assert 0 <= nf <= F and 0 <= nh <= F + 1 and dst + nh <= F + 1     # fits the (F + 1)-hop sample buffer
                assert (s, o) == (src, out)                           # offsets tile the rows without gap or overlap
                assert dst in (0, 1) and (dst == 0) == (nh == nf + 1)
                src, out = src + nh, out + nf
            seen |= {"zero"} if hops[m] == 0 else set()
            seen |= {"one_fresh"} if hops[m] == 1 and fresh[m] else set()
            seen |= {"split_fresh"} if hops[m] > F + 1 and fresh[m] else set()
            seen |= {"split_running"} if hops[m] > F + 1 and not fresh[m] else set()
        for frames, max_hops, rows in steps:
            assert frames == max(r[0] for r in rows) <= F and max_hops == max(r[1] for r in rows) >= 1
    assert seen == {"zero", "one_fresh", "split_fresh", "split_running"}
