"""CPU-only: the C-ABI surface of the composite cumLN stack -- the header declares it, the library exports it, and its workspace
functions are host arithmetic that covers the cLN stack's layouts plus the cumulative norm's scan work regions."""
import subprocess

import pytest

import conv_tasnet_amd as ctn
from conv_tasnet_amd import _lib

STACK = ["ctn_tcn_cumln_fwd", "ctn_tcn_cumln_bwd", "ctn_tcn_cumln_fwd_workspace", "ctn_tcn_cumln_bwd_workspace"]
NORM = ["ctn_cumln_fwd_amax", "ctn_cumln_bwd_amax"]


def test_header_declares_and_library_exports_the_cumln_stack():
    protos = _lib.parse_header()
    assert not [n for n in STACK + NORM if n not in protos]
    out = subprocess.run(["nm", "-D", "--defined-only", ctn.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert not [n for n in STACK + NORM if n not in exported]
    # the parameter lists of the cLN stack; the tracked norm passes: the untracked ones plus amax_out ahead of the stream
    for tail in ("_fwd", "_bwd", "_fwd_workspace", "_bwd_workspace"):
        assert protos["ctn_tcn_cumln" + tail] == protos["ctn_tcn_cln" + tail], tail
    for plain in ("ctn_cumln_fwd", "ctn_cumln_bwd"):
        assert protos[plain + "_amax"][2] == protos[plain][2][:-1] + ["amax_out", "stream"]
        assert protos[plain + "_amax"][0] is protos[plain][0]


@pytest.mark.parametrize("M,B,H,K,nblocks", [(1, 16, 32, 13, 1), (3, 64, 128, 200, 3), (4, 256, 512, 3199, 32)])
def test_workspace_functions_are_host_arithmetic(M, B, H, K, nblocks):
    lib = ctn.lib
    Kp = lib.ctn_padded_frames(K)
    work = lib.ctn_cumln_work_bytes(M, Kp)
    assert work >= M * Kp * (2 * 8 + 4 * 4)
    assert lib.ctn_tcn_cumln_fwd_workspace(M, B, H, Kp, nblocks) >= lib.ctn_tcn_cln_fwd_workspace(M, B, H, Kp, nblocks) + 2 * work
    assert lib.ctn_tcn_cumln_bwd_workspace(M, B, H, Kp, 3, nblocks) >= lib.ctn_tcn_cln_bwd_workspace(M, B, H, Kp, 3, nblocks) + work
