"""CPU-only: the float64 torch oracle of the STOI / ESTOI gradient (stoi_grad_oracle.py) against the numpy oracle and against
finite differences, the conditions on the shared inputs that the GPU tests rely on, the C-ABI surface of csrc/ctn_stoi_grad.hip
and the argument checks of the Python surface that need no GPU.

The finite-difference limit: central differences with step h = 1e-5 on samples of amplitude a ~ 1 have a truncation error of
about (h / a)^2 = 1e-10 of the gradient and a rounding error of about 1e-16 * d / h = 1e-11 absolute against gradient entries of
1e-2 .. 1e-1 at the largest; 1e-6 of the largest entry leaves three orders of magnitude to both."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

import stoi_grad_oracle as GO
import stoi_oracle as SO

import conv_tasnet_amd as ctn
from conv_tasnet_amd import _lib

ENTRY_POINTS = ["ctn_stoi_score_bwd_workspace", "ctn_stoi_score_bwd", "ctn_stoi_bands_bwd_workspace", "ctn_stoi_bands_bwd",
                "ctn_resample_rows_adjoint_workspace", "ctn_resample_rows_adjoint_f64", "ctn_stoi_pairs_workspace", "ctn_stoi_pairs_bwd_workspace", "ctn_stoi_pairs_fwd",
                "ctn_stoi_pairs_bwd"]
FD_STEP = 1e-5
FD_LIMIT = 1e-6

RUNS = {}


def _run(case, key):
    """The oracle on pair (reference 0, estimate 0) of a shared case, once per (case, weights)."""
    if (case, key) not in RUNS:
        fs, n, kind, seed = case
        ref, est = SO.case_signals(n, kind, seed)
        RUNS[case, key] = GO.run(ref[0], est[0], fs, *key)
    return RUNS[case, key]


@pytest.mark.parametrize("case", SO.CASES)
def test_oracle_forward_is_the_numpy_oracle(case):
    fs, n, kind, seed = case
    ref, est = SO.case_signals(n, kind, seed)
    want = SO.details(ref[0], est[0], fs)
    got = _run(case, (1.0, 0.0))
    dev = max(abs(got["stoi"] - want["stoi"]), abs(got["estoi"] - want["estoi"]))
    print("largest |d - numpy oracle| %.3g" % dev)
    assert dev <= 1e-14 and (got["M"], got["K"]) == (want["M"], want["K"])
    if want["M"] >= SO.N:
        assert np.abs(got["env_y"] - want["env_y"]).max() <= 1e-12 * want["env_y"].max()
    else:
        assert got["stoi"] == 1e-5 and not got["g"].any() and not got["g10"].any()


def test_conditions_on_the_inputs_of_the_gpu_tests():
    """What the GPU tests rely on, on the very pairs and rows they use: the crossed pairs (reference c, estimate 1 - c) of the
    shared cases (end to end), both references against estimate 0 of CASES[1] (the pairing that is no permutation) and the
    stage rows.  No cell near the clip bound (the project's 1e-6 margin), no zero envelope."""
    runs = []
    for fs, n, kind, seed in SO.CASES:
        if n != 3100:
            ref, est = SO.case_signals(n, kind, seed)
            runs += [GO.run(ref[c], est[1 - c], fs) for c in range(2)]
    fs, n, kind, seed = SO.CASES[1]
    ref, est = SO.case_signals(n, kind, seed)
    runs.append(GO.run(ref[1], est[0], fs))
    ref, est = GO.stage_rows()
    rows = [GO.run(ref[p, :m], est[p, :m], 10000) for p, m in enumerate(GO.STAGE_LENS)]
    assert [r["M"] for r in rows][:3] == [29, 29, 30] and 30 <= rows[3]["M"] < 52 and rows[4]["M"] >= 94
    runs += [r for r in rows if r["M"] >= SO.N]
    margins, env_min = [r["clip_margin"] for r in runs], [r["env_min"] for r in runs]
    print("clip margins %s\nsmallest envelopes %s" % (margins, env_min))
    assert min(margins) >= 1e-6 and min(env_min) > 0
    assert max(r["clipped"] for r in runs) >= 0.05


def test_conditions_on_the_shared_cases():
    """The same on pair (reference 0, estimate 0) of the shared cases, with a case with clipped cells and a case with removed
    frames."""
    live = [_run(c, (1.0, 0.0)) for c in SO.CASES if c[1] != 3100]
    margins, env_min, clipped = [r["clip_margin"] for r in live], [r["env_min"] for r in live], [r["clipped"] for r in live]
    print("clip margins %s\nsmallest envelopes %s\nclipped shares %s" % (margins, env_min, clipped))
    assert min(margins) >= 1e-6 and min(env_min) > 0
    assert max(clipped) >= 0.05
    assert any(r["K"] < SO.frame_count(r["n10"]) for r in live)


@pytest.mark.parametrize("case", SO.CASES[:6])
@pytest.mark.parametrize("key", [(1.0, 0.0), (0.0, 1.0)], ids=["stoi", "estoi"])
def test_oracle_gradient_matches_finite_differences(case, key):
    """On the linear-resampler form of the function (straight_through=False: the fp32 resampler's roundings are no function to
    take differences of), whose gradient is the same R^T chain."""
    fs, n, kind, seed = case
    ref, est = SO.case_signals(n, kind, seed)
    x, y = ref[0], est[0].astype(np.float64)
    base = GO.run(x, y, fs, *key, straight_through=False)
    g = base["g"]
    name = "stoi" if key[0] else "estoi"
    coords = [n // 7, n // 3 + 1, n // 2, (2 * n) // 3 + 5, n - 300, int(np.argmax(np.abs(g)))]
    worst = 0.0
    for i in coords:
        hi, lo = y.copy(), y.copy()
        hi[i] += FD_STEP
        lo[i] -= FD_STEP
        fd = (GO.run(x, hi, fs, *key, straight_through=False)[name] - GO.run(x, lo, fs, *key, straight_through=False)[name]) / (2 * FD_STEP)
        worst = max(worst, abs(fd - g[i]) / np.abs(g).max())
    print("largest |finite difference - gradient| / max |gradient| %.3g" % worst)
    assert worst <= FD_LIMIT
    st = _run(case, key)["g"]
    # the straight-through form has the same chain at the fp32 resampler's point: the two gradients differ by that displacement only
    print("straight-through against linear: %.3g of max |gradient|" % (np.abs(st - g).max() / np.abs(g).max()))
    assert np.abs(st - g).max() <= 1e-4 * np.abs(g).max()


def test_adjoint_is_the_transpose_of_the_linear_resampler():
    rng = np.random.RandomState(5)
    for up, down, n in ((5, 4, 700), (5, 8, 900)):
        n10 = -((-n * up) // down)
        y, g10 = rng.randn(n), rng.randn(n10)
        lhs = float((GO.resample_linear(torch.from_numpy(y), up, down).numpy() * g10).sum())
        rhs = float((GO.adjoint(g10, n, up, down) * y).sum())
        assert abs(lhs - rhs) <= 1e-12 * (np.abs(y).sum() + 1)


def test_header_declares_and_library_exports_the_gradient_entry_points():
    protos = _lib.parse_header()
    assert not [n for n in ENTRY_POINTS if n not in protos]
    out = subprocess.run(["nm", "-D", "--defined-only", ctn.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert not [n for n in ENTRY_POINTS if n not in exported]
    assert protos["ctn_stoi_pairs_workspace"][0] is ctypes.c_size_t and protos["ctn_stoi_pairs_bwd"][0] is ctypes.c_int
    assert protos["ctn_stoi_score_bwd"][2] == ["env", "kcount", "w_stoi", "w_estoi", "P", "T", "g_env", "workspace", "workspace_bytes",
                                                "stream"]
    from conv_tasnet_amd.stoi import StoiPitCriterion, cal_stoi_loss, stoi_pairs
    assert ctn.stoi_pairs is stoi_pairs and ctn.StoiPitCriterion is StoiPitCriterion and ctn.cal_stoi_loss is cal_stoi_loss


def test_workspace_sizes_and_refusals_before_any_launch():
    # every check sits in front of the first launch, so this is safe without a GPU (fake non-null pointers are never read)
    lib, err = ctn.lib, ctn.lib.ctn_last_error
    p = 4096
    T = 7100                                            # 54 first-pass frames, 53 envelope frames, 24 segments: one chunk
    assert lib.ctn_stoi_score_bwd_workspace(3, T) >= 3 * 64 * 450 * 8
    assert lib.ctn_stoi_bands_bwd_workspace(3, T) >= 3 * 53 * 256 * 8
    assert lib.ctn_stoi_pairs_workspace(2, 2, T) >= 4 * (T * 4 + 2 * 15 * 53 * 8)
    assert lib.ctn_stoi_pairs_bwd_workspace(2, 2, T) >= lib.ctn_stoi_score_bwd_workspace(4, T) + lib.ctn_stoi_bands_bwd_workspace(4, T) + 4 * T * 8
    for f in (lib.ctn_stoi_score_bwd_workspace, lib.ctn_stoi_bands_bwd_workspace):
        assert f(0, T) == 0 and f(65536, T) == 0 and f(1, 0) == 0
    assert lib.ctn_stoi_pairs_workspace(40000, 2, T) == 0 and lib.ctn_stoi_pairs_bwd_workspace(1, 65, T) == 0
    assert lib.ctn_stoi_score_bwd(0, p, p, p, 1, T, p, p, 1 << 30, 0) == -1 and b"null" in err()
    assert lib.ctn_stoi_score_bwd(p, p, p, p, 0, T, p, p, 1 << 30, 0) == -1 and b"ctn_stoi_score_bwd" in err()
    assert lib.ctn_stoi_score_bwd(p, p, p, p, 1, T, p, p, 16, 0) == -3 and b"workspace" in err()
    assert lib.ctn_stoi_bands_bwd(p, p, p, p, p, 0, 1, T, p, p, 1 << 30, 0) == -1 and b"null" in err()
    assert lib.ctn_stoi_bands_bwd(p, p, p, p, p, p, 1, T, p, 0, 0, 0) == -3 and b"workspace" in err()
    assert lib.ctn_resample_rows_adjoint_workspace(2, 2, 2, 8000) == 0       # the gather needs none
    adj = lib.ctn_resample_rows_adjoint_f64
    assert adj(p, p, p, 1, 2, 2, 8000, 10000, 5, 4, p, 34, 0, 0, 0) == -1 and b"null" in err()
    assert adj(p, p, p, 1, 2, 2, 8000, 10000, 10, 8, p, 34, p, 0, 0) == -1 and b"lowest terms" in err()
    assert adj(p, p, p, 1, 2, 2, 8000, 9999, 5, 4, p, 34, p, 0, 0) == -1 and b"T10" in err()
    assert adj(p, p, p, 1, 2, 2, 8000, 10000, 5, 4, 0, 34, p, 0, 0) == -1 and b"filter" in err()
    assert adj(p, p, p, 1, 2, 2, 8000, 8001, 1, 1, 0, 0, p, 0, 0) == -1 and b"equal rates" in err()
    assert adj(p, p, p, 40000, 2, 2, 8000, 10000, 5, 4, p, 34, p, 0, 0) == -1 and b"B * C" in err()
    assert lib.ctn_stoi_pairs_fwd(p, p, p, 0, 1, 2, 2, T, p, p, 0, p, 1 << 30, 0) == -1 and b"null" in err()
    assert lib.ctn_stoi_pairs_fwd(p, p, p, p, 1, 2, 2, T, p, p, 0, p, 16, 0) == -3 and b"workspace" in err()
    assert lib.ctn_stoi_pairs_bwd(p, 1 << 30, p, p, p, p, 1, 2, 2, 8000, 10000, 5, 4, p, 34, p, p, 16, 0) == -3 and b"workspace" in err()
    assert lib.ctn_stoi_pairs_bwd(p, 1 << 30, p, p, p, p, 1, 2, 0, 8000, 10000, 5, 4, p, 34, p, p, 1 << 30, 0) == -1 and b"E =" in err()


def test_python_surface_refuses_bad_arguments_without_a_gpu():
    from conv_tasnet_amd.stoi import StoiPitCriterion, cal_stoi_loss, stoi_pairs
    from conv_tasnet_amd import train
    x = torch.zeros(1, 2, 4000)
    with pytest.raises(ValueError):
        stoi_pairs(x, x, torch.tensor([4000]), 8000, torch.zeros(1, 2, dtype=torch.int32))          # not on the GPU
    with pytest.raises(ValueError):
        cal_stoi_loss(x, x[:, :1], torch.tensor([4000]), 8000)
    with pytest.raises(ValueError):
        cal_stoi_loss(x, x, torch.tensor([4000]), 8000, perm="best")
    with pytest.raises(ValueError):
        cal_stoi_loss(torch.zeros(1, 5, 4000), torch.zeros(1, 5, 4000), torch.tensor([4000]), 8000, perm="stoi")
    with pytest.raises(TypeError):
        StoiPitCriterion(8000)                          # the weight has no default
    for bad in (-1.0, None, "1", True):
        with pytest.raises(ValueError):
            StoiPitCriterion(8000, bad)
    with pytest.raises(ValueError):
        StoiPitCriterion(0, 1.0)
    c = StoiPitCriterion(8000, 2, extended=True)
    assert (c.sample_rate, c.weight, c.extended) == (8000, 2.0, True)
    with pytest.raises(ValueError):
        train.train({}, 1, "m.pth", loss="pit_stoi")                        # no weight
    with pytest.raises(ValueError):
        train.train({}, 1, "m.pth", loss="pit", stoi_weight=1.0)
    for argv in (["--stoi-weight", "1"], ["--stoi-extended"], ["--loss", "pit_stoi"], ["--loss", "pit_stoi", "--stoi-weight", "-1"]):
        with pytest.raises(SystemExit):
            train.main(argv)
    a = train.build_parser().parse_args(["--loss", "pit_stoi", "--stoi-weight", "5", "--stoi-extended"])
    assert (a.loss, a.stoi_weight, a.stoi_extended) == ("pit_stoi", 5.0, True)
