"""CPU-only checks of the fused streaming entry points (csrc/ctn_stream.hip): ABI surface, state sizing, argument errors."""
import ctypes
import subprocess

import conv_tasnet_amd as ctn
from conv_tasnet_amd import _lib

STREAM_ENTRY_POINTS = ["ctn_stream_state_bytes", "ctn_stream_pack_bytes", "ctn_stream_pack", "ctn_stream_tcn_cln", "ctn_stream_reset",
                       "ctn_stream_pack_gemm_bytes", "ctn_stream_pack_gemm", "ctn_stream_front", "ctn_stream_back"]


def _dil(*d):
    return (ctypes.c_int * len(d))(*d)


def test_header_declares_and_library_exports_the_stream_entry_points():
    protos = _lib.parse_header()
    assert not [n for n in STREAM_ENTRY_POINTS if n not in protos]
    out = subprocess.run(["nm", "-D", "--defined-only", ctn.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert not [n for n in STREAM_ENTRY_POINTS if n not in exported]
    assert protos["ctn_stream_state_bytes"][0] is ctypes.c_size_t and protos["ctn_stream_tcn_cln"][0] is ctypes.c_int
    assert protos["ctn_stream_tcn_cln"][2] == ["packed", "dilation", "nblocks", "y", "state", "M", "B", "H", "P", "frames", "max_frames", "stream"]
    from conv_tasnet_amd.streaming import FusedStreamingSeparator, StreamingSeparator       # noqa: F401
    assert ctn.FusedStreamingSeparator is FusedStreamingSeparator


def test_state_bytes_counts_the_rings():
    f = ctn.lib.ctn_stream_state_bytes
    M, H, P, F = 3, 32, 3, 16
    dil = [1, 2, 4, 8, 1, 2, 4, 8]
    base = f(M, H, P, _dil(*dil), len(dil), F)
    assert base >= 4 * M * H * sum((P - 1) * d + F for d in dil)
    # ring j holds the power of two >= (P-1)*d_j + max_frames frames: (P-1)*8 + 16 = 32 -> dilation 9 needs 34 -> 64
    grown = f(M, H, P, _dil(1, 2, 4, 9, 1, 2, 4, 8), len(dil), F)
    assert grown - base == 4 * M * H * (64 - 32)
    assert f(2 * M, H, P, _dil(*dil), len(dil), F) - 256 == 2 * (base - 256)          # 256-byte header with the position word
    # the paper configuration, one stream, 16-frame chunks
    paper = [2 ** x for x in range(8)] * 4
    need = 4 * 512 * sum(2 * d + 16 for d in paper)
    assert need <= f(1, 512, 3, _dil(*paper), 32, 16) <= 2 * need + 256
    assert f(1, 512, 3, 0, 32, 16) == 0 and f(1, 512, 3, _dil(*paper), 32, 0) == 0
    assert ctn.lib.ctn_stream_pack_bytes(256, 512, 3, 32) == 32 * 4 * (2 * 512 * 256 + 4 + 4 * 512 + 3 * 512)
    assert ctn.lib.ctn_stream_pack_gemm_bytes(20, 256) == 4 * 32 * 256               # rows zero-filled to a multiple of 16


def test_bad_arguments_return_error_codes_and_launch_nothing():
    # every check sits in front of the first launch, so this is safe without a GPU (fake non-null pointers are never read)
    lib, err = ctn.lib, ctn.lib.ctn_last_error
    d = _dil(1, 2)
    p = 4096
    assert lib.ctn_stream_tcn_cln(0, d, 2, p, p, 1, 16, 32, 3, 8, 16, 0) == -1 and b"null" in err()
    assert lib.ctn_stream_tcn_cln(p, d, 2, p, 0, 1, 16, 32, 3, 8, 16, 0) == -1 and b"null" in err()
    assert lib.ctn_stream_tcn_cln(p, d, 2, p, p, 1, 16, 32, 3, 17, 16, 0) == -1 and b"max_frames" in err()
    assert lib.ctn_stream_tcn_cln(p, d, 2, p, p, 1, 16, 32, 3, 0, 16, 0) == -1 and b"max_frames" in err()
    assert lib.ctn_stream_tcn_cln(p, d, 2, p, p, 1, 16, 40, 3, 8, 16, 0) == -1 and b"multiples of 16" in err()
    assert lib.ctn_stream_tcn_cln(p, d, 2, p, p, 1, 24, 32, 3, 8, 16, 0) == -1 and b"multiples of 16" in err()
    assert lib.ctn_stream_tcn_cln(p, d, 2, p, p, 1, 16, 32, 9, 8, 16, 0) == -1 and b"kernel size" in err()
    assert lib.ctn_stream_tcn_cln(p, _dil(1, 0), 2, p, p, 1, 16, 32, 3, 8, 16, 0) == -1 and b"dilation" in err()
    assert lib.ctn_stream_tcn_cln(p, d, 2, p, p, 1, 512, 1024, 3, 8, 16, 0) == -1 and b"LDS" in err()
    assert lib.ctn_stream_pack(0, 2, 16, 32, 3, p, 0) == -1 and b"null" in err()
    assert lib.ctn_stream_pack((ctypes.c_void_p * 18)(), 2, 16, 32, 3, p, 0) == -1 and b"parameter 0 is null" in err()
    assert lib.ctn_stream_pack((ctypes.c_void_p * 18)(*([p] * 18)), 2, 16, 32, 9, p, 0) == -1 and b"kernel size" in err()
    assert lib.ctn_stream_reset(0, 1024, 0) == -1 and b"null" in err()
    assert lib.ctn_stream_pack_gemm(0, 16, 16, p, 0) == -1 and b"null" in err()
    assert lib.ctn_stream_front(p, 100, p, p, p, p, p, p, 1, 24, 20, 16, 4, 0) == -1 and b"multiples of 16" in err()
    assert lib.ctn_stream_front(p, 40, p, p, p, p, p, p, 1, 32, 20, 16, 4, 0) == -1 and b"sample buffer" in err()
    assert lib.ctn_stream_back(p, p, p, p, p, p, p, 0, 100, 1, 32, 20, 16, 2, 4, 0, 0) == -1 and b"null" in err()
    assert lib.ctn_stream_back(p, p, p, p, p, p, p, p, 100, 1, 32, 20, 16, 2, 4, 2, 0) == -1 and b"mask" in err()
    try:
        ctn.lib.call("ctn_stream_tcn_cln", p, d, 2, p, p, 1, 16, 32, 3, 99, 16, 0)
    except ctn.CtnError as e:
        assert "max_frames" in str(e)
    else:
        raise AssertionError("no CtnError")
