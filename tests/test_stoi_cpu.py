"""CPU checks of the STOI / ESTOI surface: the numpy oracle's two forms agree, its band table, framing and limiting cases are
pinned, and the new C ABI entry points are declared, exported, host-callable where they should be, and reject bad arguments
before any launch."""
import subprocess

import numpy as np
import pytest

import conv_tasnet_amd as ctn
from conv_tasnet_amd import _lib
import bss_oracle as BO
import stoi_oracle as SO

NEW = ("ctn_stoi_max_frames", "ctn_stoi_workspace", "ctn_stoi_eval", "ctn_stoi_frames", "ctn_stoi_bands",
       "ctn_stoi_score_workspace", "ctn_stoi_score")
BANDS = [(7, 2), (9, 2), (11, 3), (14, 3), (17, 5), (22, 5), (27, 7), (34, 9), (43, 12), (55, 14), (69, 18), (87, 22), (109, 29),
         (138, 36), (174, 45)]


@pytest.mark.parametrize("fs,n,kind,seed", SO.CASES)
def test_oracle_fft_form_equals_dft_matrix_form(fs, n, kind, seed):
    ref, est = SO.case_signals(n, kind, seed)
    for c in range(2):
        for e in range(2):
            a, b = SO.details(ref[c], est[e], fs, "fft"), SO.details(ref[c], est[e], fs, "dft")
            assert a["M"] == b["M"] and a["K"] == b["K"]
            assert abs(a["stoi"] - b["stoi"]) <= 1e-12 and abs(a["estoi"] - b["estoi"]) <= 1e-12
            assert np.abs(a["env_x"] - b["env_x"]).max() <= 1e-12 * a["env_x"].max()
            assert np.isfinite(a["stoi"]) and np.isfinite(a["estoi"])
            if a["M"] >= SO.N and c == e:
                assert a["stoi"] > 0.4, a["stoi"]


def test_constants_and_band_table_are_pinned():
    assert (SO.FS, SO.N_FRAME, SO.HOP, SO.NFFT, SO.NUMBAND, SO.N, SO.BETA, SO.DYN_RANGE) == (10000, 256, 128, 512, 15, 30, -15, 40)
    assert SO.EPS == np.finfo(np.float64).eps and SO.TOO_SHORT == 1e-5
    assert np.array_equal(SO.WINDOW, np.hanning(258)[1:-1]) and len(SO.WINDOW) == 256
    assert SO.band_table() == BANDS
    assert BANDS[-1][0] + BANDS[-1][1] == 219                # bins 7 .. 218: the DFT of the kernel is restricted to them


@pytest.mark.parametrize("extended", [False, True])
def test_identity_scores_one_and_noise_lowers_the_score(extended):
    x = BO.speech_like(3, 1, 9000, sr=10000)[0]
    assert abs(SO.stoi(x, x, 10000, extended) - 1.0) <= 1e-12
    assert abs(SO.stoi(x, x, 8000, extended) - 1.0) <= 1e-12
    rng = np.random.RandomState(0)
    noise = rng.randn(len(x)).astype(np.float32)
    d = [SO.stoi(x, x + np.float32(g) * noise, 10000, extended) for g in (0.01, 0.05, 0.2, 0.8)]
    assert all(a > b for a, b in zip(d, d[1:])), d
    assert d[0] < 1.0 and d[-1] > -1.0


def test_framing_is_strict_at_exact_fit_lengths():
    """Frames start at i < n - 256, strictly (range(0, n - 256, 128), as pystoi and the MATLAB code frame): the frame that would
    end exactly on the last sample is dropped.  3968 / 3969 give 29 / 30 frames and 4096 / 4097 give 30 / 31; 4095 gives 30
    as well (starts 0 .. 3712 < 3839), not the 29 one gets by also dropping the last frame that fits."""
    assert [SO.frame_count(n) for n in (256, 257, 384, 385, 3968, 3969, 4095, 4096, 4097)] == [0, 1, 1, 2, 29, 30, 30, 30, 31]
    for n in (3968, 3969, 4095, 4096, 4097):
        x = BO.speech_like(5, 1, n, sr=10000)[0].astype(np.float64)
        assert len(SO.frames_of(x)) == SO.frame_count(n) == len(SO.frame_energies(x))
        assert ctn.lib.ctn_stoi_max_frames(n) == SO.frame_count(n)
    # 4096 samples without a silent frame: 30 kept frames overlap-add to 3968 samples, which frame into 29 < 30
    x = BO.speech_like(5, 1, 4096, sr=10000)[0]
    d = SO.details(x, x, 10000)
    assert d["frames"] == 30 and d["K"] == 30 and bool(d["keep"].all()) and d["M"] == 29
    assert d["stoi"] == 1e-5 and d["estoi"] == 1e-5
    d = SO.details(np.concatenate([x, x[:128]]), np.concatenate([x, x[:128]]), 10000)
    assert d["frames"] == 31 and d["M"] == 30 and abs(d["stoi"] - 1.0) <= 1e-12


def test_silent_frames_follow_the_reference():
    ref, est = SO.case_signals(7000, "pause", 1)
    d = SO.details(ref[0], est[0], 10000)
    assert 0 < d["K"] < d["frames"] and d["M"] == d["K"] - 1
    assert np.array_equal(d["index"], np.nonzero(d["energies"] > d["energies"].max() - 40)[0])
    assert d["margin"] >= 1e-6
    # the mask is the clean signal's: swapping the roles changes it
    assert SO.details(est[0] + np.float32(0.01), ref[0], 10000)["K"] != d["K"]


def test_stoi_entry_points_declared_and_exported():
    protos = _lib.parse_header()
    assert all(n in protos for n in NEW), [n for n in NEW if n not in protos]
    out = subprocess.run(["nm", "-D", "--defined-only", ctn.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert not set(NEW) - exported
    text = open(_lib.HEADER).read()
    assert "Taal" in text and "Jensen" in text and "IEEE TASLP 19(7), 2011" in text and "24(11), 2016" in text
    assert "CTN_STOI_FS 10000" in text and "CTN_STOI_FRAME 256" in text and "CTN_STOI_SEGMENT 30" in text
    assert "hanning(258)[1:-1]" in text and "pystoi" in text
    assert callable(ctn.stoi) and callable(ctn.stoi_batch)


def test_stoi_workspace_is_host_callable_and_monotone():
    one = ctn.lib.ctn_stoi_workspace(1, 2, 3, 40000)
    nf = ctn.lib.ctn_stoi_max_frames(40000)
    assert nf == SO.frame_count(40000) == 311
    assert one >= (2 + 3 * 2) * 15 * (nf - 1) * 8                     # the envelope sets alone, fp64
    sizes = [ctn.lib.ctn_stoi_workspace(b, 2, 3, 40000) for b in (1, 2, 3, 8, 64)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    assert ctn.lib.ctn_stoi_workspace(1, 3, 4, 40000) > one and ctn.lib.ctn_stoi_workspace(1, 2, 3, 80000) > one
    assert ctn.lib.ctn_stoi_workspace(1, 1, 1, 1) > 0 and ctn.lib.ctn_stoi_score_workspace(1, 2, 3, 40000) > 0
    for bad in ((0, 2, 3, 100), (1, 0, 3, 100), (1, 2, 0, 100), (1, 2, 3, 0), (1, 65, 3, 100)):
        assert ctn.lib.ctn_stoi_workspace(*bad) == 0, bad
    assert ctn.lib.ctn_stoi_max_frames(0) == 0 and ctn.lib.ctn_stoi_max_frames(256) == 1    # never an empty table


def test_stoi_bad_arguments_return_err_arg_without_launch():
    p = 4096                                                # a non-null dummy: never dereferenced, the checks come first
    big = 1 << 30
    assert ctn.lib.ctn_stoi_eval(p, p, p, 1, 0, 3, 100, p, p, p, p, p, big, 0) == -1
    assert b"C = 0" in ctn.lib.ctn_last_error()
    assert ctn.lib.ctn_stoi_eval(p, p, p, 1, 2, 0, 100, p, p, p, p, p, big, 0) == -1
    assert b"E = 0" in ctn.lib.ctn_last_error()
    assert ctn.lib.ctn_stoi_eval(p, p, p, 1, 2, 3, 0, p, p, p, p, p, big, 0) == -1
    assert b"T = 0" in ctn.lib.ctn_last_error()
    assert ctn.lib.ctn_stoi_eval(p, p, p, 0, 2, 3, 100, p, p, p, p, p, big, 0) == -1
    for k in (0, 1, 2, 7, 8):
        args = [p, p, p, 1, 2, 3, 100, p, p, p, p, p, big, 0]
        args[k] = 0
        assert ctn.lib.ctn_stoi_eval(*args) == -1, k
        assert b"null" in ctn.lib.ctn_last_error()
    assert ctn.lib.ctn_stoi_frames(0, p, 1, 2, 100, p, p, p, 0) == -1
    assert ctn.lib.ctn_stoi_frames(p, p, 1, 0, 100, p, p, p, 0) == -1
    assert ctn.lib.ctn_stoi_frames(p, p, 1, 2, 0, p, p, p, 0) == -1
    assert ctn.lib.ctn_stoi_bands(p, p, p, p, p, 1, 2, 3, 100, 0, 0) == -1
    assert ctn.lib.ctn_stoi_bands(p, p, p, p, p, 1, 2, 0, 100, p, 0) == -1
    assert ctn.lib.ctn_stoi_score(p, p, 1, 2, 3, 100, p, 0, p, p, p, big, 0) == -1
    assert ctn.lib.ctn_stoi_score(p, p, 1, 2, 3, 0, p, p, p, p, p, big, 0) == -1
    assert ctn.lib.ctn_stoi_eval(p, p, p, 1, 2, 3, 100, p, p, p, p, p, 16, 0) == -3      # workspace too small
    assert b"workspace" in ctn.lib.ctn_last_error()
    assert ctn.lib.ctn_stoi_eval(p, p, p, 1, 2, 3, 100, p, p, p, p, 0, big, 0) == -3


def test_python_surface_rejects_cpu_tensors_and_mismatches():
    import torch
    from conv_tasnet_amd.stoi import stoi, stoi_batch, stoi_improvement
    x = torch.zeros(1, 2, 5000)
    with pytest.raises(ValueError):
        stoi_batch(x, x, torch.tensor([5000]), 8000)                  # CPU tensors: there is no CPU path
    with pytest.raises(ValueError):
        stoi(np.zeros(5000, np.float32), np.zeros(4999, np.float32), 8000)
    with pytest.raises(ValueError):
        stoi(np.zeros((2, 5000), np.float32), np.zeros((2, 5000), np.float32), 8000)
    with pytest.raises(ValueError):
        stoi_improvement(torch.zeros(2, 2, 2))
    d = torch.tensor([[[0.9, 0.1], [0.2, 0.8], [0.5, 0.6]]], dtype=torch.float64)
    assert abs(float(stoi_improvement(d)[0]) - ((0.9 - 0.5) + (0.8 - 0.6)) / 2) <= 1e-15
