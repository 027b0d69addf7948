"""CPU checks of the BSS Eval surface: the numpy oracle's two forms agree, and the new C ABI entry points are declared,
exported, host-callable where they should be, and reject bad arguments before any launch."""
import subprocess

import numpy as np
import pytest

import conv_tasnet_amd as ctn
from conv_tasnet_amd import _lib
import bss_oracle as BO

NEW = ("ctn_bss_workspace", "ctn_bss_eval", "ctn_bss_corr_workspace", "ctn_bss_corr", "ctn_bss_factor_doubles",
       "ctn_bss_factor", "ctn_bss_solve", "ctn_bss_project_workspace", "ctn_bss_project")
F = 512


@pytest.mark.parametrize("C,n,pole", [(2, 1000, 0.9), (2, 3000, 0.98), (3, 1500, 0.9)])
def test_oracle_fft_lu_form_equals_direct_cholesky_form(C, n, pole):
    ref, est = BO.mixtures(5 + C, C, n, pole)
    a = BO.bss_matrices(ref, est, "fft")
    b = BO.bss_matrices(ref, est, "direct")
    for x, y in zip(a, b):
        assert np.all(np.isfinite(x))
        np.testing.assert_allclose(x, y, rtol=0, atol=1e-9)
    sa, sb = BO.bss_eval_sources(ref, est[::-1], "fft"), BO.bss_eval_sources(ref, est[::-1], "direct")
    assert list(sa[3]) == list(sb[3]) == list(range(C))[::-1]


def test_bss_entry_points_declared_and_exported():
    protos = _lib.parse_header()
    assert all(n in protos for n in NEW), [n for n in NEW if n not in protos]
    out = subprocess.run(["nm", "-D", "--defined-only", ctn.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert not set(NEW) - exported
    text = open(_lib.HEADER).read()
    assert "src/evaluate.py:76-91" in text and "bss_eval_sources" in text and "CTN_BSS_FLEN 512" in text


def test_bss_workspace_is_host_callable():
    one = ctn.lib.ctn_bss_workspace(1, 2, 3, 32000)
    assert one >= (2 * F) ** 2 * 8 + F * F * 8            # G plus G_11, fp64
    assert ctn.lib.ctn_bss_workspace(8, 2, 3, 32000) >= 8 * (2 * F) ** 2 * 8
    assert ctn.lib.ctn_bss_workspace(1, 3, 4, 32000) > one
    assert ctn.lib.ctn_bss_factor_doubles(2, 2) == 2 * ((2 * F) ** 2 + F * F)
    assert ctn.lib.ctn_bss_factor_doubles(1, 4) == (4 * F) ** 2 + 3 * F * F
    assert ctn.lib.ctn_bss_corr_workspace(1, 2, 3, 4096) > 0 and ctn.lib.ctn_bss_project_workspace(1, 2, 3, 4096) > 0
    for bad in ((1, 5, 3, 100), (1, 1, 3, 100), (0, 2, 3, 100), (1, 2, 0, 100), (1, 2, 3, 0)):
        assert ctn.lib.ctn_bss_workspace(*bad) == 0, bad


def test_bss_bad_arguments_return_err_arg_without_launch():
    p = 4096                                                # a non-null dummy: never dereferenced, the checks come first
    assert ctn.lib.ctn_bss_eval(p, p, p, 1, 5, 3, 100, p, p, p, p, p, 1 << 30, 0) == -1
    assert b"C = 5" in ctn.lib.ctn_last_error()
    assert ctn.lib.ctn_bss_eval(p, p, p, 1, 1, 3, 100, p, p, p, p, p, 1 << 30, 0) == -1
    assert ctn.lib.ctn_bss_eval(p, p, p, 1, 2, 3, 0, p, p, p, p, p, 1 << 30, 0) == -1
    assert ctn.lib.ctn_bss_eval(0, p, p, 1, 2, 3, 100, p, p, p, p, p, 1 << 30, 0) == -1
    assert b"null" in ctn.lib.ctn_last_error()
    assert ctn.lib.ctn_bss_eval(p, p, p, 1, 2, 3, 100, p, p, p, 0, p, 1 << 30, 0) == -1
    assert ctn.lib.ctn_bss_corr(p, p, p, 1, 2, 3, 100, 0, p, p, p, 1 << 30, 0) == -1
    assert ctn.lib.ctn_bss_factor(p, 1, 5, p, p, 0) == -1
    assert ctn.lib.ctn_bss_factor(0, 1, 2, p, p, 0) == -1
    assert ctn.lib.ctn_bss_solve(p, p, 1, 2, 0, p, p, 0) == -1
    assert ctn.lib.ctn_bss_project(p, p, p, p, p, 1, 2, 3, 0, p, p, p, 0, p, 1 << 30, 0) == -1
    assert ctn.lib.ctn_bss_eval(p, p, p, 1, 2, 3, 100, p, p, p, p, p, 16, 0) == -3     # workspace too small
    assert b"workspace" in ctn.lib.ctn_last_error()
