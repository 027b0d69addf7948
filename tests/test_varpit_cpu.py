"""CPU checks of the variable-speaker-count surface: the numpy oracle's three forms against each other (direct against moment
form, the gradient against central finite differences), the exact ties inside a tie class, the count draw's oracle, the new C ABI
entry points (declared, exported, host-callable where they should be, bad arguments rejected before any launch) and the options
of train() and the command line."""
import subprocess

import numpy as np
import pytest
import torch

import conv_tasnet_amd as ctn
from conv_tasnet_amd import _lib
import dynmix_active_oracle as AO
import dynmix_oracle as DO
import varpit_oracle as VO

NEW = ("ctn_varpit_workspace", "ctn_varpit_fwd", "ctn_varpit_bwd", "ctn_dynmix_plan_active", "ctn_dynmix_mask_active")


@pytest.mark.parametrize("shape", VO.SHAPES)
def test_moment_form_equals_direct_form_and_the_planted_cases_have_a_margin(shape):
    """The shapes and seeds of the GPU tests: the margin those rely on, and the kernels' algebra against the direct sums."""
    for seed in (0, 1):
        s, e, lens, planted = VO.make_case(*shape, seed=seed)
        d, m = VO.direct(s, e, lens), VO.moment_form(s, e, lens)
        worst = max(np.abs(d["per_utt"] - m["per_utt"]).max(), np.abs(d["pair"] - m["pair"]).max())
        print("%s seed %d: moment form against direct form %.3e dB, smallest margin %.3f dB" % (shape, seed, worst, d["margin"].min()))
        assert np.array_equal(d["idx"], m["idx"])
        assert worst <= 1e-8
        assert d["margin"].min() >= 1e-3
        # the planted pairing on the active references, and the planted outputs on the inactive ones
        for b in range(shape[0]):
            assert VO.tie_key(d["ref_of"][b], d["active"][b]) == VO.tie_key(planted[b], d["active"][b]), b
        assert (d["active"].sum(1) == 1 + np.arange(shape[0]) % shape[1]).all()


@pytest.mark.parametrize("C", [3, 4, 6])
def test_ties_inside_a_class_are_exact_and_the_first_in_table_order_wins(C):
    s, e, lens, planted = VO.make_case(4, C, 300, seed=7, active_counts=[1, C - 2, 0, C])
    d = VO.direct(s, e, lens)
    perms = VO.perm_table(C)
    for b, n_in in enumerate([C - 1, 2, C, 0]):
        key = VO.tie_key(perms[d["idx"][b]], d["active"][b])
        cls = [k for k in range(len(perms)) if VO.tie_key(perms[k], d["active"][b]) == key]
        n_ties = int(np.prod(np.arange(1, n_in + 1)))
        assert len(cls) == n_ties                                      # n_in! ways to hand out the inactive references
        assert all(d["L"][b, k] == d["L"][b, d["idx"][b]] for k in cls)            # bitwise equal sums
        assert d["idx"][b] == min(cls)
        m = VO.moment_form(s, e, lens)
        assert all(m["L"][b, k] == m["L"][b, m["idx"][b]] for k in cls) and m["idx"][b] == d["idx"][b]
    assert d["margin"][2] == np.inf and len(set(d["L"][2])) == 1       # every reference silent: one class


def test_oracle_gradient_against_central_finite_differences():
    s, e, lens, _ = VO.make_case(3, 3, 60, seed=5)
    s, e = s.astype(np.float64), e.astype(np.float64)
    g_per = np.array([0.5, -1.25, 2.0])
    ref = VO.direct(s, e, lens, g_loss=0.75, g_per=g_per)
    assert ref["margin"].min() >= 1.0                                  # the winner does not change under the probe

    def objective(x):
        o = VO.direct(s, x, lens)
        return 0.75 * o["loss"] + float((g_per * o["per_utt"]).sum())

    rng = np.random.default_rng(0)
    worst, h = 0.0, 1e-6
    for _ in range(40):
        b, i, t = rng.integers(3), rng.integers(3), rng.integers(60)
        up, dn = e.copy(), e.copy()
        up[b, i, t] += h
        dn[b, i, t] -= h
        fd = (objective(up) - objective(dn)) / (2 * h)
        g = ref["grad"][b, i, t]
        assert (g == 0) == (t >= lens[b])
        worst = max(worst, abs(fd - g) / max(abs(g), 1e-3))
    print("oracle gradient against central differences: worst relative difference %.2e" % worst)
    assert worst <= 1e-5


@pytest.mark.parametrize("shape", [(4, 2, 1033), (4, 3, 1033), (5, 4, 1033), (3, 6, 777)])
def test_fp32_backward_order_stays_inside_the_gradient_bound(shape):
    s, e, lens, _ = VO.make_case(*shape, seed=0)
    g_per = np.linspace(0.5, 1.5, shape[0]).astype(np.float32)
    ref = VO.direct(s, e, lens, g_loss=0.75, g_per=g_per)
    got = VO.grad_fp32(s, e, lens, ref, g_loss=0.75, g_per=g_per)
    bound = VO.grad_bound(s, e, lens, ref, g_loss=0.75, g_per=g_per)
    inside = np.broadcast_to(np.arange(shape[2])[None, None, :] < lens[:, None, None], got.shape)
    ratio = (np.abs(got - ref["grad"])[inside] / bound[inside]).max()
    print("fp32 emulation of the backward order: worst |d| / bound = %.3f" % ratio)
    assert ratio <= 1.0 and (got[~inside] == 0).all()


def test_oracle_limits_and_zero_length():
    s, e, lens, _ = VO.make_case(3, 3, 400, seed=2, active_counts=[3, 2, 1])
    d = VO.direct(s, s, lens, snr_max=30.0, inactive_snr_max=20.0)    # exact estimates: the thresholds are what is left
    assert abs(d["pair"][0, 0, 0] + 30.0) <= 1e-2
    lens0 = lens.copy()
    lens0[1] = 0
    z = VO.direct(s, e, lens0)
    assert z["per_utt"][1] == 0.0 and z["idx"][1] == 0 and (z["grad"][1] == 0).all() and (z["active"][1] == 0).all()
    # an output paired with an inactive reference is scored by its level in the clean mixture alone
    b, o = 2, VO.direct(s, e, lens)
    n = int(lens[b])
    silent = np.nonzero(o["act_of"][b] == 0)[0]
    assert len(silent) == 2
    xx = (s[b, :, :n].astype(np.float64).sum(0) ** 2).sum()
    for i in silent:
        ee = (e[b, i, :n].astype(np.float64) ** 2).sum()
        assert abs(o["pair"][b, i, o["ref_of"][b, i]] - 10 * np.log10((ee + 0.01 * xx + VO.EPS) / (xx + VO.EPS))) <= 1e-9
    two = VO.make_case(3, 2, 500, seed=3, active_counts=[2, 2, 2])
    plain = VO.plain_snr_pit(*two[:3])
    assert np.abs(VO.direct(*two[:3], snr_max=None)["per_utt"] + plain).max() <= 1e-9


# ---- the count draw ---------------------------------------------------------------------------------------------------------
def test_count_draw_stays_in_range_and_leaves_the_other_blocks_alone():
    for C in (2, 3, 4):
        assert AO.COUNT_WORD not in AO.other_words(C) and max(AO.other_words(C)) < AO.COUNT_WORD
        for m in range(1, C + 1):
            n = np.concatenate([AO.counts(5, 1, 2, step, 200, C, m) for step in range(3)])
            assert n.min() >= m and n.max() <= C and n.dtype == np.int32
            assert set(n.tolist()) == set(range(m, C + 1))
    assert (AO.counts(0, 0, 0, 0, 16, 3, 3) == 3).all()
    a, b = AO.counts(5, 1, 2, 0, 64, 3, 1), AO.counts(5, 1, 2, 1, 64, 3, 1)
    assert not np.array_equal(a, b) and np.array_equal(a, AO.counts(5, 1, 2, 0, 64, 3, 1))
    assert not np.array_equal(a, AO.counts(5, 0, 2, 0, 64, 3, 1)) and not np.array_equal(a, AO.counts(5, 1, 3, 0, 64, 3, 1))
    # the draw is the first word of its own block, nothing of the plan's
    r = DO.philox4x32((1024, 7, 0, 2), (5, 1 << 16))
    assert a[7] == 1 + DO.below(r[0], 3)
    g = np.arange(12, dtype=np.float32).reshape(4, 3) + 1
    assert AO.masked(g, [1, 2, 3, 1]).tolist() == [[1, 0, 0], [4, 5, 0], [7, 8, 9], [10, 0, 0]] and g[0, 1] == 2


def test_loader_validates_min_speakers_before_touching_the_device():
    class _Corpus:
        device = torch.device("cpu")

    for bad in (0, 4, -1):
        with pytest.raises(ValueError, match="min_speakers"):
            ctn.DynamicMixLoader(_Corpus(), 2, 100, num_speakers=3, rank=0, min_speakers=bad)


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_and_exported():
    protos = _lib.parse_header()
    assert all(n in protos for n in NEW), [n for n in NEW if n not in protos]
    out = subprocess.run(["nm", "-D", "--defined-only", ctn.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert not set(NEW) - exported
    assert protos["ctn_varpit_fwd"][2] == ["sources", "estimates", "lengths", "perms", "nperm", "B", "C", "T", "tau", "tau0", "per_utt",
                                           "perm_idx", "pair", "active", "loss", "coef", "workspace", "workspace_bytes", "stream"]
    assert protos["ctn_varpit_bwd"][2] == ["sources", "estimates", "lengths", "perms", "perm_idx", "coef", "g_loss", "g_per", "B", "C",
                                           "T", "d_estimates", "stream"]
    text = open(_lib.HEADER).read()
    assert "ICASSP 2021" in text and "csrc/ctn_varpit.hip" in text and "csrc/ctn_dynmix_active.hip" in text
    for name in ("cal_varpit_loss", "VarPitCriterion", "output_levels", "count_sources", "evaluate_variable"):
        assert callable(getattr(ctn, name)), name


def test_workspace_is_host_callable_and_scales_with_the_batch():
    one = ctn.lib.ctn_varpit_workspace(1, 6, 32000)
    assert one == ctn.lib.ctn_sisnr_chunks(32000) * 49 * 8               # 49 fp64 moments per chunk at C = 6
    assert [ctn.lib.ctn_varpit_workspace(b, 6, 32000) for b in (2, 3, 8, 257)] == [one * b for b in (2, 3, 8, 257)]
    assert ctn.lib.ctn_varpit_workspace(1, 2, 64) == (4 + 4 + 1) * 8
    assert ctn.lib.ctn_varpit_workspace(1, 3, 4133) == 3 * 16 * 8
    for bad in ((0, 4, 100), (-1, 4, 100), (1, 1, 100), (1, 7, 100), (1, 0, 100), (1, 4, 0), (1, 4, -5)):
        assert ctn.lib.ctn_varpit_workspace(*bad) == 0, bad


def test_bad_arguments_return_err_arg_without_launch():
    p = 4096                                                # a non-null dummy: never dereferenced, the checks come first
    big = 1 << 30
    fwd = [p, p, p, p, 24, 2, 4, 100, 1e-3, 1e-2, p, p, p, p, p, p, p, big, 0]
    for k in (0, 1, 2, 3, 10, 11, 12, 13, 14, 15):
        args = list(fwd)
        args[k] = 0
        assert ctn.lib.ctn_varpit_fwd(*args) == -1, k
        assert b"null" in ctn.lib.ctn_last_error()
    for c in (-1, 0, 1, 7, 64):
        args = list(fwd)
        args[6] = c
        assert ctn.lib.ctn_varpit_fwd(*args) == -1, c
        assert b"outside 2 .. 6" in ctn.lib.ctn_last_error()
    for k, v in ((4, 23), (4, 6), (5, 0), (5, -2), (7, 0), (8, -1.0), (9, -1e-3)):
        args = list(fwd)
        args[k] = v
        assert ctn.lib.ctn_varpit_fwd(*args) == -1, (k, v)
    args = list(fwd)
    args[17] = 16
    assert ctn.lib.ctn_varpit_fwd(*args) == -3                            # workspace too small
    assert b"workspace" in ctn.lib.ctn_last_error()
    args = list(fwd)
    args[16] = 0
    assert ctn.lib.ctn_varpit_fwd(*args) == -3
    bwd = [p, p, p, p, p, p, 0, 0, 2, 4, 100, p, 0]                       # both upstream gradients may be null
    for k in (0, 1, 2, 3, 4, 5, 11):
        args = list(bwd)
        args[k] = 0
        assert ctn.lib.ctn_varpit_bwd(*args) == -1, k
        assert b"null" in ctn.lib.ctn_last_error()
    for c in (1, 7):
        args = list(bwd)
        args[9] = c
        assert ctn.lib.ctn_varpit_bwd(*args) == -1, c
        assert b"outside 2 .. 6" in ctn.lib.ctn_last_error()
    for k in (8, 10):
        args = list(bwd)
        args[k] = 0
        assert ctn.lib.ctn_varpit_bwd(*args) == -1, k
    plan = [0, 0, 0, p, 8, 3, 1, p, 0]
    for k, v in ((3, 0), (7, 0), (4, 0), (5, 1), (5, 5), (6, 0), (6, 4), (0, -1), (0, 1 << 48), (1, -1), (2, -1), (2, 1 << 16)):
        args = list(plan)
        args[k] = v
        assert ctn.lib.ctn_dynmix_plan_active(*args) == -1, (k, v)
    mask = [p, 8, 3, p, 0]
    for k, v in ((0, 0), (3, 0), (1, 0), (2, 1), (2, 5)):
        args = list(mask)
        args[k] = v
        assert ctn.lib.ctn_dynmix_mask_active(*args) == -1, (k, v)


def test_python_surface_rejects_bad_shapes_and_cpu_tensors():
    s, e, lens = torch.zeros(2, 3, 64), torch.zeros(2, 3, 64), torch.tensor([64, 64])
    with pytest.raises(ctn.CtnError):
        ctn.cal_varpit_loss(s, e, lens)                                 # CPU tensors: there is no CPU path
    for bs, be in ((torch.zeros(2, 2, 64), e), (torch.zeros(2, 1, 64), torch.zeros(2, 1, 64)), (torch.zeros(2, 7, 64), torch.zeros(2, 7, 64)),
                   (torch.zeros(3, 3, 64), e), (torch.zeros(2, 3, 65), e), (s[0], e)):
        with pytest.raises(ValueError):
            ctn.cal_varpit_loss(bs, be, lens)
    with pytest.raises(ValueError):
        ctn.cal_varpit_loss(s, e, torch.tensor([64]))
    lev = ctn.output_levels(torch.ones(1, 2, 8) * torch.tensor([1.0, 0.1]).view(1, 2, 1), torch.ones(1, 8), torch.tensor([4]))
    assert torch.allclose(lev, torch.tensor([[0.0, -20.0]], dtype=torch.float64), atol=1e-6)
    assert ctn.count_sources(torch.ones(1, 2, 8) * torch.tensor([1.0, 0.05]).view(1, 2, 1), torch.ones(1, 8), torch.tensor([8])).tolist() == [1]
    with pytest.raises(ValueError):
        ctn.output_levels(torch.ones(1, 2, 8), torch.ones(1, 9), torch.tensor([8]))


# ---- train and the command line ---------------------------------------------------------------------------------------------
def test_train_and_the_command_line_validate_the_varpit_options():
    from conv_tasnet_amd import train as TR
    with pytest.raises(ValueError, match="got 'bogus'"):
        TR.train({}, 1, "m.pth.tar", loss="bogus")
    with pytest.raises(SystemExit, match="--min-speakers applies to --dynamic-mix only"):
        TR.main(["--min-speakers", "1"])
    with pytest.raises(SystemExit, match="--min-speakers applies to --dynamic-mix only"):
        TR.main(["--loss", "varpit", "--min-speakers", "1", "--dynamic-mix-cv", "cv.json"])
    with pytest.raises(SystemExit, match="--loss varpit needs --dynamic-mix"):
        TR.main(["--loss", "varpit"])
    with pytest.raises(SystemExit, match="--loss varpit needs --dynamic-mix"):
        TR.main(["--loss", "varpit", "--dynamic-mix", "tr.json", "--min-speakers", "1"])
    with pytest.raises(SystemExit, match="--min-speakers must be 1 .. 3"):
        TR.main(["--loss", "varpit", "--dynamic-mix", "tr.json", "--dynamic-mix-cv", "cv.json", "--speakers", "3", "--min-speakers", "4"])
    with pytest.raises(SystemExit, match="--speakers must be 2 .. 4"):
        TR.main(["--loss", "varpit", "--dynamic-mix", "tr.json", "--dynamic-mix-cv", "cv.json", "--speakers", "5"])
    with pytest.raises(SystemExit, match="--speakers applies to --loss varpit only"):
        TR.main(["--speakers", "3"])
    a = TR.build_parser().parse_args([])
    assert a.loss == "pit" and a.min_speakers is None and a.inactive_snr_max == "20" and a.speakers is None
    c = ctn.VarPitCriterion()
    assert c.snr_max == 30.0 and c.inactive_snr_max == 20.0 and ctn.VarPitCriterion(None, None).inactive_snr_max is None
