"""CPU-only: the numpy fp64 oracle of the multi-resolution STFT loss (mrstft_oracle.py) against a torch.stft restatement in
value and in gradient, the conditions on the inputs of every test case (these and the GPU tests'), the C-ABI surface of
csrc/ctn_mrstft.hip and the argument checks that need no GPU.

The limits.  Oracle and restatement are both fp64 and differ in the order of the FFT's additions only: 1e-10 max(1, |v|) on a
term, 1e-10 of the row's largest entry on a gradient."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

import mrstft_oracle as MO

import conv_tasnet_amd as ctn
from conv_tasnet_amd import _lib

ENTRY_POINTS = ["ctn_mrstft_workspace", "ctn_mrstft_bwd_workspace", "ctn_mrstft_pairs_fwd", "ctn_mrstft_pairs_bwd"]
RESOLUTIONS = [(64, 16, 48), (256, 50, 240), (2048, 240, 1200)]
LENGTHS = {(64, 16, 48): (4096, 1003, 33), (256, 50, 240): (4096, 2051, 129), (2048, 240, 1200): (4096, 3121, 1025)}
LIMIT = 1e-10
G = (1.0, 0.75, 0.5)           # upstream weights of (sc, logmag, linmag) in the gradient tests: every term takes part


def _torch_terms(ref, est, res, eps=MO.EPS):
    """torch.stft + clamp + sqrt + norms, as auraloss states the loss; ref, est fp64 tensors of the row's own n samples"""
    n_fft, hop, win = res
    w = torch.hann_window(win, dtype=torch.float64)
    mags = []
    for x in (ref, est):
        X = torch.stft(x, n_fft, hop, win, w, center=True, pad_mode="reflect", return_complex=True)
        mags.append(torch.sqrt(torch.clamp(X.real ** 2 + X.imag ** 2, min=eps)))
    a, b = mags
    sc = torch.norm(a - b, p="fro") / torch.norm(a, p="fro")
    return torch.stack([sc, (torch.log(a) - torch.log(b)).abs().mean(), (a - b).abs().mean()]), a.shape[1]


def _rows(res):
    ref, est = MO.signals(7 + res[0], 1, 1, 4096)
    return [(ref[0, :n], est[0, :n]) for n in LENGTHS[res]]


@pytest.mark.parametrize("res", RESOLUTIONS, ids=str)
def test_oracle_values_and_gradient_are_those_of_torch_stft(res):
    worst_v = worst_g = 0.0
    for x, y in _rows(res):
        out = MO.run(x, y, res, G)
        MO.conditions([out])
        yt = torch.from_numpy(y.astype(np.float64)).requires_grad_(True)
        terms, frames = _torch_terms(torch.from_numpy(x.astype(np.float64)), yt, res)
        assert frames == out["frames"] == 1 + x.shape[0] // res[1]
        (terms * torch.tensor(G, dtype=torch.float64)).sum().backward()
        want = terms.detach().numpy()
        worst_v = max(worst_v, float((np.abs(out["terms"] - want) / np.maximum(1.0, np.abs(want))).max()))
        g = yt.grad.numpy()
        assert np.abs(g).max() > 0
        worst_g = max(worst_g, float(np.abs(out["grad"] - g).max() / np.abs(g).max()))
    print("largest term deviation %.3g, largest gradient deviation / row maximum %.3g" % (worst_v, worst_g))
    assert worst_v <= LIMIT and worst_g <= LIMIT


def test_oracle_gives_zeros_where_reflect_padding_is_undefined():
    x, y = MO.signals(3, 1, 1, 64)
    for n in (0, 1, 32):
        out = MO.run(x[0, :n], y[0, :n], (64, 16, 48))
        assert not out["terms"].any() and not out["grad"].any() and out["grad"].shape == (n,)
    assert MO.run(x[0, :33], y[0, :33], (64, 16, 48))["terms"].all()


@pytest.mark.parametrize("name", sorted(MO.CASES))
def test_conditions_on_the_inputs_of_the_gpu_tests(name):
    """No bin's power within a relative 1e-6 of eps and no bin with | |S| - |S^| | < 1e-9 |S|, on every cell of the shared cases."""
    runs = [r for r in MO.case_runs(name).values() if r["frames"]]
    cm, em = MO.conditions(runs)
    print("smallest |power / eps - 1| %.3g, smallest | |S| - |S^| | / |S| %.3g, clamped bins %d"
          % (cm, em, sum(r["clamped"] for r in runs)))
    res, lens = MO.CASES[name][:2]
    empty = [k for k, r in MO.case_runs(name).items() if not r["frames"]]
    assert sorted(empty) == sorted((b, c, r) for b, n in enumerate(lens) for c in range(MO.CASES[name][2])
                                   for r, rr in enumerate(res) if n <= rr[0] // 2)


def test_header_declares_and_library_exports_the_entry_points():
    protos = _lib.parse_header()
    assert not [n for n in ENTRY_POINTS if n not in protos]
    out = subprocess.run(["nm", "-D", "--defined-only", ctn.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert not [n for n in ENTRY_POINTS if n not in exported]
    assert protos["ctn_mrstft_workspace"][0] is ctypes.c_size_t and protos["ctn_mrstft_pairs_bwd"][0] is ctypes.c_int
    assert protos["ctn_mrstft_pairs_fwd"][2] == ["ref", "est", "lengths", "est_of_ref", "B", "C", "E", "T", "resolutions", "R", "eps",
                                                  "terms", "workspace", "workspace_bytes", "stream"]
    from conv_tasnet_amd.mrstft import MrStftPitCriterion, cal_mrstft_loss, mrstft_pairs
    assert ctn.mrstft_pairs is mrstft_pairs and ctn.MrStftPitCriterion is MrStftPitCriterion and ctn.cal_mrstft_loss is cal_mrstft_loss


def _res(*triples):
    return np.ascontiguousarray(np.array(triples, dtype=np.int32).reshape(-1, 3))


BAD = {"n_fft no power of two": [(1000, 100, 400)], "n_fft too small": [(32, 8, 32)], "n_fft too large": [(4096, 512, 2048)],
       "win_length > n_fft": [(512, 128, 513)], "win_length 0": [(512, 128, 0)], "hop 0": [(512, 0, 256)],
       "ceil(win / hop) > 64": [(1024, 9, 600)], "nine resolutions": [(64, 16, 48)] * 9, "no resolution": []}


def test_workspace_sizes_and_refusals_before_any_launch():
    # every check sits in front of the first launch, so this is safe without a GPU (fake non-null pointers are never read;
    # `resolutions` is a host array and is real)
    lib, err = ctn.lib, ctn.lib.ctn_last_error
    p, T = 4096, 4000
    ok = _res(*MO.DEFAULT_RESOLUTIONS)
    frames = sum(1 + T // r[1] for r in MO.DEFAULT_RESOLUTIONS)
    taps = sum((1 + T // r[1]) * r[2] for r in MO.DEFAULT_RESOLUTIONS)
    assert lib.ctn_mrstft_workspace(2, 2, T, 3, ok.ctypes.data) >= 4 * frames * 32 + 2048 * 16 + 3 * 2048 * 8
    assert taps * 4 * 8 <= lib.ctn_mrstft_bwd_workspace(2, 2, T, 3, ok.ctypes.data) < taps * 4 * 8 + 4096
    assert _res((1024, 10, 640)).ctypes.data and lib.ctn_mrstft_workspace(1, 1, T, 1, _res((1024, 10, 640)).ctypes.data) > 0   # ceil = 64
    for f in (lib.ctn_mrstft_workspace, lib.ctn_mrstft_bwd_workspace):
        assert f(0, 2, T, 3, ok.ctypes.data) == 0 and f(40000, 2, T, 3, ok.ctypes.data) == 0 and f(1, 65, T, 3, ok.ctypes.data) == 0
        assert f(1, 1, 0, 3, ok.ctypes.data) == 0 and f(1, 1, (1 << 24) + 1, 3, ok.ctypes.data) == 0 and f(1, 1, T, 3, 0) == 0
    fwd, bwd = lib.ctn_mrstft_pairs_fwd, lib.ctn_mrstft_pairs_bwd
    for name, triples in BAD.items():
        bad = _res(*triples) if triples else _res((64, 16, 48))
        R = len(triples)
        assert lib.ctn_mrstft_workspace(1, 2, T, R, bad.ctypes.data) == 0, name
        assert lib.ctn_mrstft_bwd_workspace(1, 2, T, R, bad.ctypes.data) == 0, name
        assert fwd(p, p, p, p, 1, 2, 2, T, bad.ctypes.data, R, 1e-7, p, p, 1 << 40, 0) == -1 and b"resolution" in err(), name
        assert bwd(p, 1 << 40, p, p, p, p, 1, 2, 2, T, bad.ctypes.data, R, 1e-7, p, p, p, 1 << 40, 0) == -1 and b"resolution" in err(), name
    r = ok.ctypes.data
    for k in (0, 1, 2, 3, 8, 11):                       # ref, est, lengths, est_of_ref, resolutions, terms
        args = [p, p, p, p, 1, 2, 2, T, r, 3, 1e-7, p, p, 1 << 40, 0]
        args[k] = 0
        assert fwd(*args) == -1 and b"null" in err(), k
    for k in (0, 2, 3, 4, 5, 10, 13, 14):               # fwd_workspace, ref, est, lengths, est_of_ref, resolutions, g_terms, g_est
        args = [p, 1 << 40, p, p, p, p, 1, 2, 2, T, r, 3, 1e-7, p, p, p, 1 << 40, 0]
        args[k] = 0
        assert bwd(*args) == -1 and b"null" in err(), k
    assert fwd(p, p, p, p, 1, 2, 2, T, r, 3, 1e-7, p, p, 16, 0) == -3 and b"workspace" in err()
    assert fwd(p, p, p, p, 1, 2, 2, T, r, 3, 1e-7, p, 0, 1 << 40, 0) == -3 and b"workspace" in err()
    assert bwd(p, 16, p, p, p, p, 1, 2, 2, T, r, 3, 1e-7, p, p, p, 1 << 40, 0) == -3 and b"workspace" in err()
    assert bwd(p, 1 << 40, p, p, p, p, 1, 2, 2, T, r, 3, 1e-7, p, p, p, 16, 0) == -3 and b"workspace" in err()
    assert fwd(p, p, p, p, 40000, 2, 2, T, r, 3, 1e-7, p, p, 1 << 40, 0) == -1 and b"B * C" in err()
    assert fwd(p, p, p, p, 1, 2, 0, T, r, 3, 1e-7, p, p, 1 << 40, 0) == -1 and b"E =" in err()
    assert fwd(p, p, p, p, 1, 2, 2, T, r, 3, 0.0, p, p, 1 << 40, 0) == -1 and b"eps" in err()


def test_python_surface_refuses_bad_arguments_without_a_gpu():
    from conv_tasnet_amd import train
    from conv_tasnet_amd.mrstft import (DEFAULT_RESOLUTIONS, MrStftPitCriterion, cal_mrstft_loss, check_resolutions, mrstft_pairs,
                                        parse_resolutions)
    assert DEFAULT_RESOLUTIONS == MO.DEFAULT_RESOLUTIONS == ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))
    for name, triples in BAD.items():
        with pytest.raises(ValueError):
            check_resolutions(triples)
    for bad in ([(512, 128)], [(512.5, 128, 256)], 7, [(512, True, 256)]):
        with pytest.raises(ValueError):
            check_resolutions(bad)
    assert check_resolutions([[1024, 10, 640]]) == ((1024, 10, 640),)
    assert parse_resolutions("1024:120:600,2048:240:1200,512:50:240") == DEFAULT_RESOLUTIONS
    for bad in ("1024:120", "a:b:c", "1000:100:400", ""):
        with pytest.raises(ValueError):
            parse_resolutions(bad)
    x = torch.zeros(1, 2, 4000)
    eo = torch.zeros(1, 2, dtype=torch.int32)
    with pytest.raises(ValueError):
        mrstft_pairs(x, x, torch.tensor([4000]), eo)                        # not on the GPU
    with pytest.raises(ValueError):
        cal_mrstft_loss(x, x[:, :1], torch.tensor([4000]))
    with pytest.raises(ValueError):
        cal_mrstft_loss(x, x, torch.tensor([4000]), perm="best")
    with pytest.raises(ValueError):
        cal_mrstft_loss(x, x, torch.tensor([4000]), w_log=-1.0)
    with pytest.raises(TypeError):
        MrStftPitCriterion()                                                # the weight has no default
    for bad in (-1.0, None, "1", True):
        with pytest.raises(ValueError):
            MrStftPitCriterion(bad)
    with pytest.raises(ValueError):
        MrStftPitCriterion(1.0, resolutions=[(1000, 100, 400)])
    c = MrStftPitCriterion(2, [(256, 64, 256)], w_lin=1)
    assert (c.weight, c.resolutions, c.w_sc, c.w_log, c.w_lin) == (2.0, ((256, 64, 256),), 1.0, 1.0, 1.0)
    with pytest.raises(ValueError):
        train.train({}, 1, "m.pth", loss="pit_mrstft")                      # no weight
    with pytest.raises(ValueError):
        train.train({}, 1, "m.pth", loss="pit", mrstft_weight=1.0)
    with pytest.raises(ValueError):
        train.train({}, 1, "m.pth", loss="pit_stoi", stoi_weight=1.0, mrstft_resolutions=DEFAULT_RESOLUTIONS)
    with pytest.raises(ValueError):
        train.train({}, 1, "m.pth", loss="pit_mrstft", mrstft_weight=1.0, mrstft_resolutions=[(1000, 100, 400)])
    for argv in (["--mrstft-weight", "1"], ["--mrstft-resolutions", "512:50:240"], ["--loss", "pit_mrstft"],
                 ["--loss", "pit_mrstft", "--mrstft-weight", "-1"], ["--loss", "pit_stoi", "--stoi-weight", "1", "--mrstft-weight", "1"],
                 ["--loss", "pit_mrstft", "--mrstft-weight", "1", "--mrstft-resolutions", "1000:100:400"],
                 ["--loss", "pit_mrstft", "--mrstft-weight", "1", "--stoi-weight", "1"]):
        with pytest.raises(SystemExit):
            train.main(argv)
    a = train.build_parser().parse_args(["--loss", "pit_mrstft", "--mrstft-weight", "5", "--mrstft-resolutions", "256:64:256"])
    assert (a.loss, a.mrstft_weight, a.mrstft_resolutions) == ("pit_mrstft", 5.0, "256:64:256")
