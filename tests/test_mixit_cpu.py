"""CPU checks of the MixIT surface: the numpy oracle against torch fp64 autograd, its properties and limiting cases, the
moment form (the kernels' algebra) against the direct form in fp64, the fp32 order of the backward pass against its bound,
the host logic of MixtureOfMixtures / pair_batch / remix, the new C ABI entry points (declared, exported, host-callable
where they should be, bad arguments rejected before any launch) and Solver's optional criterion."""
import subprocess

import numpy as np
import pytest
import torch

import conv_tasnet_amd as ctn
from conv_tasnet_amd import _lib, mixit
import mixit_oracle as MO

NEW = ("ctn_mixit_workspace", "ctn_mixit_fwd", "ctn_mixit_bwd")
SMALL = [(3, 2, 1033), (3, 3, 1033), (3, 4, 1033), (2, 8, 1033), (3, 5, 1033), (3, 6, 777), (9, 2, 64)]
_CASES = {}


def case(shape, seed=0, noise=0.03):
    key = (shape, seed, noise)
    if key not in _CASES:
        x, e, lens, planted = MO.make_case(*shape, seed=seed, noise=noise)
        _CASES[key] = (x, e, lens, planted, MO.direct(x, e, lens))
    return _CASES[key]


def torch_mixit(x, e, lens, snr_max):
    """The definition written with torch fp64 ops: every remix through the [2^M, 2, M] assignment matrices."""
    B, M, T = e.shape
    A = torch.from_numpy(MO.assign_matrices(M))
    tau = MO.threshold(snr_max)
    keep = (torch.arange(T)[None, None, :] < torch.as_tensor(lens).clamp(0, T)[:, None, None]).double()
    res = (torch.einsum("anm,bmt->bant", A, e) - x[:, None]) * keep[:, None]
    err = (res * res).sum(-1)
    xx = ((x * keep) ** 2).sum(-1)[:, None, :]
    L = (10.0 * torch.log10((err + tau * xx + MO.EPS) / (xx + MO.EPS))).mean(-1)
    per_utt, assign = L.min(dim=1)
    return per_utt.mean(), per_utt, assign


@pytest.mark.parametrize("shape", SMALL)
def test_oracle_equals_torch_fp64_autograd(shape):
    x, e, lens, planted, o = case(shape)
    et = torch.from_numpy(e).double().requires_grad_(True)
    loss, per_utt, assign = torch_mixit(torch.from_numpy(x).double(), et, lens, 30.0)
    loss.backward()
    assert np.array_equal(assign.numpy(), o["assign"])
    assert np.abs(per_utt.detach().numpy() - o["per_utt"]).max() <= 1e-12
    assert abs(float(loss.detach()) - o["loss"]) <= 1e-12
    d = np.abs(et.grad.numpy() - o["grad"]).max()
    print("oracle gradient against torch fp64 autograd: %.2e (largest element %.2e)" % (d, np.abs(o["grad"]).max()))
    assert d <= 1e-13 * max(1.0, np.abs(o["grad"]).max())
    # upstream gradient of per_utt alone
    g = np.linspace(-1.0, 2.0, shape[0])
    et.grad = None
    _, per_utt, _ = torch_mixit(torch.from_numpy(x).double(), et, lens, 30.0)
    (per_utt * torch.from_numpy(g)).sum().backward()
    o2 = MO.direct(x, e, lens, g_per=g)
    assert np.abs(et.grad.numpy() - o2["grad"]).max() <= 1e-13 * max(1.0, np.abs(o2["grad"]).max())


@pytest.mark.parametrize("shape", SMALL)
def test_oracle_finds_the_planted_assignment_with_a_margin(shape):
    x, e, lens, planted, o = case(shape)
    assert np.array_equal(o["assign"], planted)
    print("smallest margin %.3f dB" % o["margin"].min())
    assert o["margin"].min() >= 1.0
    assert (o["per_utt"] >= -30.0 - 1e-9).all() and (o["snr"] <= 30.0 + 1e-9).all()
    assert np.abs(o["per_utt"] + o["snr"].mean(-1)).max() <= 1e-12
    assert (o["grad"][np.broadcast_to(np.arange(shape[2])[None, None, :] >= lens[:, None, None], e.shape)] == 0).all()
    # swapping the two mixtures complements the assignment and keeps the loss
    s = MO.direct(x[:, ::-1], e, lens)
    assert np.array_equal(s["assign"], ((1 << shape[1]) - 1) ^ o["assign"])
    assert np.abs(s["per_utt"] - o["per_utt"]).max() <= 1e-12 and np.abs(s["snr"][:, ::-1] - o["snr"]).max() <= 1e-12


def test_oracle_threshold_bounds_the_loss_and_none_removes_it():
    x, e, lens, planted, _ = case((3, 4, 1033), noise=0.0)             # exact estimates: the threshold is what is left
    for snr_max in (10.0, 30.0, 60.0):
        o = MO.direct(x, e, lens, snr_max)
        assert (o["per_utt"] >= -snr_max - 1e-9).all() and (o["per_utt"] <= -snr_max + 1e-2).all(), o["per_utt"]
    assert (MO.direct(x, e, lens, None)["per_utt"] < -80.0).all()


def test_oracle_zero_length_and_silent_reference():
    x, e, lens, planted, _ = case((3, 4, 1033))
    lens0 = lens.copy()
    lens0[1] = 0
    o = MO.direct(x, e, lens0)
    assert o["per_utt"][1] == 0.0 and o["assign"][1] == 0 and (o["grad"][1] == 0).all() and (o["snr"][1] == 0).all()
    assert abs(o["loss"] - (o["per_utt"][0] + o["per_utt"][2]) / 3) <= 1e-15
    xs = x.copy()
    xs[2, 1] = 0.0                                                     # one silent reference mixture
    for snr_max in (30.0, None):
        s = MO.direct(xs, e, lens, snr_max)
        assert np.isfinite(s["per_utt"]).all() and np.isfinite(s["grad"]).all() and np.isfinite(s["snr"]).all()
        m = MO.moment_form(xs, e, lens, snr_max)
        assert np.isfinite(m["per_utt"]).all()
    z = MO.direct(x, np.zeros_like(e), lens)                           # silent estimates: 0 dB, every assignment ties -> a = 0
    assert np.isfinite(z["grad"]).all() and (z["assign"] == 0).all() and np.abs(z["per_utt"]).max() <= 0.01
    # lengths beyond T are clamped, negative ones count as 0
    c = MO.direct(x, e, np.array([5000, -3, lens[2]]))
    assert c["per_utt"][1] == 0.0 and c["per_utt"][0] == MO.direct(x, e, np.array([1033, 0, lens[2]]))["per_utt"][0]


@pytest.mark.parametrize("snr_max", [30.0, 60.0])
def test_moment_form_equals_direct_form_in_fp64(snr_max):
    """The cancellation in err = Xx - 2 Xe + G is the worst with exact estimates (noise 0), where err is a rounding residue and
    only tau Xx is left: the two forms must still agree to 1e-8 dB."""
    worst = 0.0
    for shape in SMALL:
        for noise in (0.0, 0.03):
            x, e, lens, planted = MO.make_case(*shape, seed=3, noise=noise)
            d, m = MO.direct(x, e, lens, snr_max), MO.moment_form(x, e, lens, snr_max)
            assert np.array_equal(d["assign"], m["assign"])
            worst = max(worst, np.abs(d["per_utt"] - m["per_utt"]).max(), np.abs(d["snr"] - m["snr"]).max())
    print("snr_max %g: moment form against direct form, worst %.3e dB" % (snr_max, worst))
    assert worst <= 1e-8


@pytest.mark.parametrize("shape", SMALL)
def test_fp32_backward_order_stays_inside_the_gradient_bound(shape):
    x, e, lens, planted, o = case(shape)
    g_per = np.linspace(0.5, 1.5, shape[0]).astype(np.float32)
    ref = MO.direct(x, e, lens, g_loss=0.75, g_per=g_per)
    got = MO.grad_fp32(x, e, lens, ref["assign"], ref["coef"].astype(np.float32), g_loss=0.75, g_per=g_per)
    bound = MO.grad_bound(x, e, lens, ref["assign"], ref["coef"], g_loss=0.75, g_per=g_per)
    ratio = (np.abs(got - ref["grad"]) / np.maximum(bound, 1e-300))[bound > 0].max()
    print("fp32 emulation of the backward order: worst |d| / bound = %.3f" % ratio)
    assert ratio <= 1.0
    assert (got[np.broadcast_to(np.arange(shape[2])[None, None, :] >= lens[:, None, None], got.shape)] == 0).all()


# ---- host logic -------------------------------------------------------------------------------------------------------------
class _Loader:
    def __init__(self, C, n=3, B=2, T=50):
        g = torch.Generator().manual_seed(5)
        self.batches = [(torch.randn(B, T, generator=g), torch.full((B,), T, dtype=torch.long), torch.randn(B, C, T, generator=g))
                        for _ in range(n)]
        self.epochs = []
        self.dataset = self

    def set_epoch(self, epoch):
        self.epochs.append(epoch)

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)


def test_mixture_of_mixtures_sums_groups_and_passes_the_mixture_through():
    inner = _Loader(4)
    mom = ctn.MixtureOfMixtures(inner)
    assert len(mom) == 3 and mom.dataset is mom
    mom.dataset.set_epoch(7)
    assert inner.epochs == [7]
    out = list(mom)
    assert len(out) == 3
    for (mix, lens, refs), (m0, l0, s0) in zip(out, inner.batches):
        assert mix is m0 and lens is l0 and refs.shape == (2, 2, 50) and refs.dtype == torch.float32
        assert torch.equal(refs[:, 0], s0[:, 0] + s0[:, 1]) and torch.equal(refs[:, 1], s0[:, 2] + s0[:, 3])
    refs = next(iter(ctn.MixtureOfMixtures(inner, groups=((3, 0, 2), (1,)))))[2]
    s0 = inner.batches[0][2]
    assert torch.equal(refs[:, 0], (s0[:, 0] + s0[:, 2]) + s0[:, 3]) and torch.equal(refs[:, 1], s0[:, 1])   # ascending index order
    for bad in (((0, 1), (1, 2)), ((0, 1), (3, 4)), ((0, 1),), ((0,), (1,), (2, 3)), ((0, 1), ()), ((0, 2), (3,))):
        with pytest.raises(ValueError):
            ctn.MixtureOfMixtures(inner, groups=bad)
    with pytest.raises(ValueError, match="cover 4 sources"):
        next(iter(ctn.MixtureOfMixtures(_Loader(3))))
    plain = ctn.MixtureOfMixtures(inner.batches)                        # a loader without a dataset: set_epoch is a no-op
    plain.set_epoch(1)
    assert len(plain) == 3


def test_pair_batch_adds_neighbouring_rows_up_to_the_shorter_length():
    g = torch.Generator().manual_seed(1)
    mix, lens = torch.randn(6, 40, generator=g), torch.tensor([40, 31, 12, 40, 0, 25])
    mom, plen, refs = ctn.pair_batch(mix, lens)
    assert mom.shape == (3, 40) and refs.shape == (3, 2, 40) and plen.tolist() == [31, 12, 0]
    for k in range(3):
        n = plen[k]
        assert torch.equal(refs[k, 0, :n], mix[2 * k, :n]) and torch.equal(refs[k, 1, :n], mix[2 * k + 1, :n])
        assert (refs[k, :, n:] == 0).all() and torch.equal(mom[k], refs[k, 0] + refs[k, 1])
        assert torch.equal(mom[k, :n], mix[2 * k, :n] + mix[2 * k + 1, :n])
    for bad in ((mix[:5], lens[:5]), (mix[:0], lens[:0]), (mix, lens[:4]), (mix.view(6, 1, 40), lens)):
        with pytest.raises(ValueError):
            ctn.pair_batch(*bad)


def test_remix_applies_an_assignment():
    g = torch.Generator().manual_seed(2)
    e = torch.randn(2, 4, 30, generator=g)
    assign = torch.tensor([[0, 1, 1, 0], [1, 1, 1, 1]])
    r = ctn.remix(e, assign)
    assert r.shape == (2, 2, 30)
    assert torch.allclose(r[0, 0], e[0, 0] + e[0, 3], atol=1e-6) and torch.allclose(r[0, 1], e[0, 1] + e[0, 2], atol=1e-6)
    assert (r[1, 0] == 0).all() and torch.allclose(r[1, 1], e[1].sum(0), atol=1e-6)
    with pytest.raises(ValueError):
        ctn.remix(e, assign[:, :3])
    assert mixit.unpack_assign(torch.tensor([0b0110, 0b1111, 0]), 4).tolist() == [[0, 1, 1, 0], [1, 1, 1, 1], [0, 0, 0, 0]]
    assert mixit.threshold(None) == 0.0 and mixit.threshold(30.0) == MO.threshold(30.0) == 10.0 ** -3.0


def test_python_surface_rejects_bad_shapes_and_cpu_tensors():
    x, e, lens = torch.zeros(2, 2, 64), torch.zeros(2, 4, 64), torch.tensor([64, 64])
    with pytest.raises(ctn.CtnError):
        ctn.cal_mixit_loss(x, e, lens)                                  # CPU tensors: there is no CPU path
    for bx, be in ((torch.zeros(2, 3, 64), e), (x, torch.zeros(2, 1, 64)), (x, torch.zeros(2, 9, 64)), (x, torch.zeros(3, 4, 64)),
                   (x, torch.zeros(2, 4, 65)), (x[0], e)):
        with pytest.raises(ValueError):
            ctn.cal_mixit_loss(bx, be, lens)
    with pytest.raises(ValueError):
        ctn.cal_mixit_loss(x, e, torch.tensor([64]))
    with pytest.raises(ctn.CtnError):
        ctn.cal_mixit_loss(x, e.transpose(1, 2).contiguous().transpose(1, 2), lens)


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
def test_mixit_entry_points_declared_and_exported():
    protos = _lib.parse_header()
    assert all(n in protos for n in NEW), [n for n in NEW if n not in protos]
    out = subprocess.run(["nm", "-D", "--defined-only", ctn.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert not set(NEW) - exported
    assert protos["ctn_mixit_fwd"][2] == ["mixtures", "estimates", "lengths", "B", "M", "T", "tau", "per_utt", "assign", "snr", "loss",
                                          "coef", "workspace", "workspace_bytes", "stream"]
    assert protos["ctn_mixit_bwd"][2] == ["mixtures", "estimates", "lengths", "assign", "coef", "g_loss", "g_per", "B", "M", "T",
                                          "d_estimates", "stream"]
    text = open(_lib.HEADER).read()
    assert "Wisdom" in text and "NeurIPS 2020" in text and "csrc/ctn_mixit.hip" in text
    for name in ("cal_mixit_loss", "remix", "pair_batch", "MixtureOfMixtures", "MixItCriterion"):
        assert callable(getattr(ctn, name)), name


def test_mixit_workspace_is_host_callable_and_scales_with_the_batch():
    one = ctn.lib.ctn_mixit_workspace(1, 8, 32000)
    assert one == ctn.lib.ctn_sisnr_chunks(32000) * 54 * 8               # 54 fp64 moments per chunk at M = 8
    assert [ctn.lib.ctn_mixit_workspace(b, 8, 32000) for b in (2, 3, 8, 257)] == [one * b for b in (2, 3, 8, 257)]
    assert ctn.lib.ctn_mixit_workspace(1, 2, 64) == (3 + 4 + 2) * 8
    assert ctn.lib.ctn_mixit_workspace(1, 4, 32000) < one < ctn.lib.ctn_mixit_workspace(1, 8, 64000)
    for bad in ((0, 4, 100), (-1, 4, 100), (1, 1, 100), (1, 9, 100), (1, 0, 100), (1, 4, 0), (1, 4, -5)):
        assert ctn.lib.ctn_mixit_workspace(*bad) == 0, bad


def test_mixit_bad_arguments_return_err_arg_without_launch():
    p = 4096                                                # a non-null dummy: never dereferenced, the checks come first
    big = 1 << 30
    fwd = [p, p, p, 2, 4, 100, 1e-3, p, p, p, p, p, p, big, 0]
    for k in (0, 1, 2, 7, 8, 9, 10, 11):
        args = list(fwd)
        args[k] = 0
        assert ctn.lib.ctn_mixit_fwd(*args) == -1, k
        assert b"null" in ctn.lib.ctn_last_error()
    for m in (-1, 0, 1, 9, 64):
        args = list(fwd)
        args[4] = m
        assert ctn.lib.ctn_mixit_fwd(*args) == -1, m
        assert b"outside 2 .. 8" in ctn.lib.ctn_last_error()
    for k, v in ((3, 0), (3, -2), (5, 0), (6, -1.0)):
        args = list(fwd)
        args[k] = v
        assert ctn.lib.ctn_mixit_fwd(*args) == -1, (k, v)
    args = list(fwd)
    args[13] = 16
    assert ctn.lib.ctn_mixit_fwd(*args) == -3                             # workspace too small
    assert b"workspace" in ctn.lib.ctn_last_error()
    args = list(fwd)
    args[12] = 0
    assert ctn.lib.ctn_mixit_fwd(*args) == -3
    bwd = [p, p, p, p, p, 0, 0, 2, 4, 100, p, 0]                          # both upstream gradients may be null
    for k in (0, 1, 2, 3, 4, 10):
        args = list(bwd)
        args[k] = 0
        assert ctn.lib.ctn_mixit_bwd(*args) == -1, k
        assert b"null" in ctn.lib.ctn_last_error()
    for m in (1, 9):
        args = list(bwd)
        args[8] = m
        assert ctn.lib.ctn_mixit_bwd(*args) == -1, m
        assert b"outside 2 .. 8" in ctn.lib.ctn_last_error()
    for k in (7, 9):
        args = list(bwd)
        args[k] = 0
        assert ctn.lib.ctn_mixit_bwd(*args) == -1, k


# ---- Solver and train ------------------------------------------------------------------------------------------------------
class _Net(torch.nn.Module):
    def __init__(self, C):
        super().__init__()
        self.w = torch.nn.Parameter(torch.linspace(0.5, 1.5, C).view(1, C, 1))

    def forward(self, mixture):
        return mixture.unsqueeze(1) * self.w


def _solver(tmp_path, C, criterion="default"):
    from conv_tasnet_amd.solver import Solver
    net = _Net(C)
    loader = _Loader(C)
    args = (0, 1, 0, 0, 5, str(tmp_path), 0, "", "final.pth.tar", 1000, 0, 0, "t")
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    data = {"tr_loader": loader, "cv_loader": loader}
    return (Solver(data, net, opt, args) if criterion == "default" else Solver(data, net, opt, args, criterion=criterion)), loader


def test_solver_without_a_criterion_calls_cal_loss(tmp_path, monkeypatch):
    from conv_tasnet_amd import solver as S
    calls = []

    def spy(sources, estimate, lengths):
        calls.append((sources, estimate.shape, lengths))
        return ((estimate - sources) ** 2).mean(), None, None, None

    monkeypatch.setattr(S, "cal_loss", spy)
    for kind in ("default", None):
        del calls[:]
        s, loader = _solver(tmp_path, 2, kind)
        assert s.criterion is None
        w0 = s.model.w.detach().clone()
        s._run_one_epoch(0)
        assert len(calls) == 3 and all(c[0] is b[2] and c[2] is b[1] for c, b in zip(calls, loader.batches))
        assert not torch.equal(s.model.w.detach(), w0) and len(s.iter_losses) == 3
        s._run_one_epoch(0, cross_valid=True)
        assert len(calls) == 6


def test_solver_with_a_criterion_never_calls_cal_loss(tmp_path, monkeypatch):
    from conv_tasnet_amd import solver as S

    def boom(*a):
        raise AssertionError("cal_loss called although a criterion was given")

    monkeypatch.setattr(S, "cal_loss", boom)
    seen = []

    def criterion(sources, estimate, lengths):
        seen.append((sources, lengths))
        return (estimate ** 2).mean()

    s, loader = _solver(tmp_path, 4, criterion)
    s._run_one_epoch(0)
    s._run_one_epoch(0, cross_valid=True)
    assert len(seen) == 6 and all(c[0] is b[2] and c[1] is b[1] for c, b in zip(seen, loader.batches + loader.batches))
    assert len(s.iter_losses) == 6 and all(np.isfinite(s.iter_losses))


def test_train_and_the_command_line_validate_the_mixit_options():
    from conv_tasnet_amd import train as TR
    with pytest.raises(ValueError, match="'pit' or 'mixit'"):
        TR.train({}, 1, "m.pth.tar", loss="sisdr")
    with pytest.raises(SystemExit, match="--dynamic-mix"):
        TR.main(["--loss", "mixit"])
    with pytest.raises(SystemExit, match="--dynamic-mix-cv"):
        TR.main(["--loss", "mixit", "--dynamic-mix", "tr.json"])
    with pytest.raises(SystemExit, match="2 .. 8"):
        TR.main(["--loss", "mixit", "--dynamic-mix", "tr.json", "--dynamic-mix-cv", "cv.json", "--mixit-outputs", "9"])
    a = TR.build_parser().parse_args([])
    assert a.loss == "pit" and a.mixit_outputs == 4 and a.snr_max == "30"
    c = ctn.MixItCriterion(None)
    assert c.snr_max is None and ctn.MixItCriterion().snr_max == 30.0
