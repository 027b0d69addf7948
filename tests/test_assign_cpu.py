"""CPU: the numpy restatement of optimal-assignment PIT (tests/assign_oracle.py) against scipy and against itself, and the host side
of the new entry points.  What the GPU tests rely on is established here: the restated solver is exact (and terminates on
non-finite input), the moment form the kernels use is the direct form, and every GPU case has a margin that makes an exact
comparison of the permutation meaningful."""
import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

import assign_oracle as AO

import conv_tasnet_amd as ctn

SOLVER_C = [1, 2, 3, 5, 8, 13, 16]


@pytest.mark.parametrize("C", SOLVER_C)
def test_restated_solver_reaches_scipys_optimum(C):
    """200 random matrices, every fourth rounded to integers (many exact ties), plus an all-equal one, both senses: a valid
    permutation of scipy's optimum value (within 1e-9: the sums are added in different orders)."""
    mats = AO.solver_matrices(C)
    assert len(mats) == 201 and (mats[-1] == mats[-1, 0, 0]).all()
    if C > 1:
        assert any(len(np.unique(m)) < m.size for m in mats[:-1:4])             # the rounded ones do hold ties
    mismatches = 0
    for maximize in (True, False):
        perms = AO.solve(mats, maximize)
        assert perms.shape == (201, C)
        for p in perms:
            assert AO.is_permutation(p)
        d = np.abs(AO.value(mats, perms) - AO.scipy_value(mats, maximize))
        mismatches += int((d > 1e-9).sum())
    print("C = %d: %d mismatches in 402" % (C, mismatches))
    assert mismatches == 0


def test_restated_solver_terminates_on_non_finite_input():
    """Bounded loops: a NaN row, +-inf entries, all NaN, all +inf -- each returns SOME valid permutation."""
    rng = np.random.default_rng(7)
    for C in (1, 2, 5, 16):
        base = rng.standard_normal((C, C))
        nan_row, infs = base.copy(), base.copy()
        nan_row[C // 2] = np.nan
        infs[0, 0], infs[-1, 0], infs[C // 2, -1] = np.inf, -np.inf, np.inf
        for m in (nan_row, infs, np.full((C, C), np.nan), np.full((C, C), np.inf), np.full((C, C), -np.inf)):
            for maximize in (True, False):
                assert AO.is_permutation(AO.solve(m, maximize)), (C, maximize, m)


@pytest.fixture(scope="module")
def cases():
    """(s, e, lens, planted, direct) of every GPU shape for seeds 0 and 1, computed once."""
    out = {}
    for shape in AO.SHAPES:
        for seed in (0, 1):
            s, e, lens, planted = AO.make_case(*shape, seed=seed)
            out[shape, seed] = (s, e, lens, planted, AO.direct(s, e, lens))
    return out


def test_moment_form_is_the_direct_form(cases):
    """Observed worst difference: 2e-12 dB (raw moments in fp64, then centred: the cancellation is far below the 5e-6 dB of the
    GPU tests)."""
    worst = 0.0
    for (shape, seed), (s, e, lens, _, ref) in cases.items():
        worst = max(worst, float(np.abs(AO.moment_form(s, e, lens) - ref["pair"]).max()))
    print("moment form against direct form: worst %.2e dB" % worst)
    assert worst <= 1e-9


def test_every_gpu_case_has_a_margin_and_its_planted_optimum(cases):
    smallest = {}
    for (shape, seed), (s, e, lens, planted, ref) in cases.items():
        smallest[shape] = min(smallest.get(shape, np.inf), float(ref["margin"].min()))
        assert np.array_equal(ref["perm"], planted), (shape, seed)
        assert np.abs(ref["pair"]).max() < 128
        # the restated solver on the fp32-rounded matrix, which is what the device solves
        assert np.array_equal(AO.solve(ref["pair"].astype(np.float32), True), ref["perm"]), (shape, seed)
    for shape, m in smallest.items():
        print("%s: smallest margin %.3f dB" % (shape, m))
    assert min(smallest.values()) >= 1e-3


@pytest.mark.parametrize("C", [8, 16])
def test_mixed_estimates_need_a_real_solver(C):
    """Every estimate a random mixture of all references: the row-wise argmax is no permutation, so a greedy "solver" fails here;
    the restated solver equals scipy's assignment."""
    s, e, lens = AO.make_mixed_case(4, C, 2049, seed=C)
    ref = AO.direct(s, e, lens)
    print("C = %d: margins %s dB" % (C, np.array2string(ref["margin"], precision=4)))
    assert ref["margin"].min() >= 1e-3
    for b in range(4):
        assert not AO.is_permutation(ref["pair"][b].argmax(1)), b
        assert np.array_equal(AO.solve(ref["pair"][b].astype(np.float32), True), ref["perm"][b]), b
        r, c = linear_sum_assignment(ref["pair"][b], maximize=True)
        assert np.array_equal(c, ref["perm"][b])


def test_gradient_of_the_direct_form_is_its_finite_difference():
    """The oracle's own gradient (the chain rule on the vectors) against central differences of its own max_snr, and A sc + B ec
    against it: the coefficient form the bound is stated in is the same gradient."""
    s, e, lens, _ = AO.make_case(2, 3, 64, seed=5)
    g_max = np.array([1.0, -0.5])
    ref = AO.direct(s, e, lens, g_max=g_max)
    e64 = e.astype(np.float64)
    rng = np.random.default_rng(0)
    for _ in range(12):
        b, i, t = rng.integers(2), rng.integers(3), rng.integers(32)
        h = 1e-6
        ep, em = e64.copy(), e64.copy()
        ep[b, i, t] += h
        em[b, i, t] -= h
        fd = ((AO.direct(s, ep, lens)["max_snr"] - AO.direct(s, em, lens)["max_snr"]) * g_max).sum() / (2 * h)
        assert abs(fd - ref["grad"][b, i, t]) <= 1e-5 * max(1.0, abs(fd)), (b, i, t, fd, ref["grad"][b, i, t])
    for b in range(2):
        n = int(lens[b])
        for i in range(3):
            j = ref["perm"][b, i]
            form = g_max[b] / 3 * (ref["A"][b, i] * (s[b, j, :n] - ref["ms"][b, i]) + ref["Bc"][b, i] * (e64[b, i, :n] - ref["me"][b, i]))
            assert np.abs(form - ref["grad"][b, i, :n]).max() <= 1e-9 * np.abs(ref["grad"][b, i]).max()
    assert (ref["grad"][1, :, int(lens[1]):] == 0).all()


def _call(name, **kw):
    """An entry point on fake 16-byte-aligned pointers with valid arguments except for `kw` (by the header's parameter names): such
    a call must be refused before any HIP call.  -> (status, message)"""
    dflt = {"B": 2, "N": 2, "C": 8, "T": 4096, "maximize": 1, "stream": 0, "workspace_bytes": 1 << 30}
    names = ctn.lib.protos[name][2]
    assert set(kw) <= set(names), (name, kw)
    rc = getattr(ctn.lib.load(), name)(*[kw[nm] if nm in kw else dflt.get(nm, 16) for nm in names])
    return rc, ctn.lib.ctn_last_error().decode()


@pytest.mark.parametrize("name,kw,code,word", [
    ("ctn_sisnr_assign_fwd", {"C": 17}, -1, "C = 17"),
    ("ctn_sisnr_assign_fwd", {"C": 1}, -1, "C = 1"),
    ("ctn_sisnr_assign_fwd", {"perm": 0}, -1, "null"),
    ("ctn_sisnr_assign_fwd", {"estimate": 0}, -1, "null"),
    ("ctn_sisnr_assign_fwd", {"workspace_bytes": 8}, -3, "workspace"),
    ("ctn_sisnr_assign_fwd", {"workspace": 0}, -3, "workspace"),
    ("ctn_sisnr_assign_fwd", {"T": 0}, -1, "bad sizes"),
    ("ctn_sisnr_assign_bwd", {"C": 17}, -1, "C = 17"),
    ("ctn_sisnr_assign_bwd", {"C": 1}, -1, "C = 1"),
    ("ctn_sisnr_assign_bwd", {"coef": 0}, -1, "null"),
    ("ctn_assign_solve", {"C": 17}, -1, "C = 17"),
    ("ctn_assign_solve", {"C": 0}, -1, "C = 0"),
    ("ctn_assign_solve", {"score": 0}, -1, "null"),
    ("ctn_assign_solve", {"N": 0}, -1, "bad sizes"),
])
def test_entry_points_refuse_before_any_launch(name, kw, code, word):
    rc, msg = _call(name, **kw)
    assert rc == code and msg.startswith(name + ":") and word in msg, (rc, msg)


def test_workspace_size_and_exports():
    L = ctn.lib
    assert L.ctn_sisnr_assign_workspace(8, 16, 32000) == 8 * L.ctn_sisnr_chunks(32000) * (4 * 16 + 256) * 8
    assert L.ctn_sisnr_assign_workspace(8, 2, 32000) == L.ctn_sisnr_workspace(8, 2, 32000)
    assert L.ctn_sisnr_assign_workspace(8, 17, 32000) == 0 and L.ctn_sisnr_assign_workspace(8, 1, 32000) == 0
    for fn in (ctn.cal_assign_loss, ctn.linear_assignment, ctn.reorder_estimate, ctn.AssignPitCriterion, ctn.assign.SiSnrAssign):
        assert callable(fn)


def test_python_wrappers_refuse_bad_shapes_and_cpu_tensors():
    import torch
    with pytest.raises(ValueError, match="2 .. 16"):
        ctn.cal_assign_loss(torch.zeros(1, 17, 64), torch.zeros(1, 17, 64), torch.tensor([64]))
    with pytest.raises(ValueError, match="2 .. 16"):
        ctn.cal_assign_loss(torch.zeros(1, 1, 64), torch.zeros(1, 1, 64), torch.tensor([64]))
    with pytest.raises(ValueError, match="1 .. 16"):
        ctn.linear_assignment(torch.zeros(2, 17, 17))
    with pytest.raises(ValueError):
        ctn.linear_assignment(torch.zeros(2, 3, 4))
    with pytest.raises(ctn.CtnError):                                    # no CPU fallback
        ctn.cal_assign_loss(torch.zeros(1, 8, 64), torch.zeros(1, 8, 64), torch.tensor([64]))
    with pytest.raises(ctn.CtnError):
        ctn.linear_assignment(torch.zeros(2, 3, 3))


def test_reorder_estimate_applies_the_inverse_permutation():
    """A 3-cycle, where the inverse differs from the permutation itself (the case reorder_source gets wrong)."""
    import torch
    from conv_tasnet_amd.pit_criterion import reorder_source
    est = torch.arange(2 * 3 * 4, dtype=torch.float32).view(2, 3, 4)
    perm = torch.tensor([[1, 2, 0], [0, 2, 1]])
    out = ctn.reorder_estimate(est, perm)
    for b in range(2):
        for i in range(3):
            assert torch.equal(out[b, perm[b, i]], est[b, i])
    legacy = reorder_source(est, perm, torch.tensor([0, 1]))
    assert not torch.equal(legacy[0], out[0]) and torch.equal(legacy[1], out[1])      # the 3-cycle differs, the swap does not
    assert torch.equal(ctn.reorder_estimate(est, perm.int()), out)
    with pytest.raises(ValueError):
        ctn.reorder_estimate(est, perm[:, :2])


def test_train_cli_refuses_what_the_loss_does_not_take():
    from conv_tasnet_amd import train as TR
    with pytest.raises(SystemExit, match="--speakers must be 2 .. 16"):
        TR.main(["--loss", "pit_assign", "--speakers", "17"])
    with pytest.raises(SystemExit, match="--speakers must be 2 .. 16"):
        TR.main(["--loss", "pit_assign", "--speakers", "1"])
    with pytest.raises(SystemExit, match="the dynamic mixer plans at most 4 sources"):
        TR.main(["--loss", "pit_assign", "--speakers", "8", "--dynamic-mix", "tr.json"])
    with pytest.raises(SystemExit, match="--speakers applies to --loss varpit only"):
        TR.main(["--loss", "pit_stoi", "--stoi-weight", "1", "--speakers", "3"])
    assert TR.build_parser().parse_args(["--loss", "pit_assign", "--speakers", "12"]).speakers == 12
    with pytest.raises(ValueError, match="2 .. 16 speakers"):
        TR.train({}, 1, "x.pth.tar", config=dict(TR.TINY, C=17), loss="pit_assign")
    with pytest.raises(ValueError, match="pit_assign"):
        TR.train({}, 1, "x.pth.tar", loss="hungarian")
