"""GPU: the MixIT loss kernels (csrc/ctn_mixit.hip, mixit.py) against the numpy fp64 direct-form oracle in mixit_oracle.py.

Limits (none of them comes from what the kernels give):
  * assign: exact.  Every case first asserts that the ORACLE's margin between the best and the second-best assignment is at
    least 1e-3 dB, so a tie can never excuse a mismatch.
  * per_utt, snr, loss: 5e-6 dB.  Each is one fp32 rounding of a value below 64 in magnitude (half an ulp: 1.9e-6); the fp64
    summation-order and moment-form difference is bounded by tests/test_mixit_cpu.py (1e-8 dB).
  * gradient, elementwise: (M + 6) 2^-24 |scale_b c_n| (sum_{k in A_n} |e_k[t]| + |x_n[t]|)  (mixit_oracle.grad_bound: M - 1
    fp32 adds, one subtraction, the roundings of c_n, of the scale and of the two products); exactly 0 for t >= len.
"""
import numpy as np
import pytest
import torch

import mixit_oracle as MO
from conftest import DEFAULT_ARITH, set_arith

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402

DEV = "cuda:0"
TOL_DB = 5e-6
_CASES = {}


def case(shape, seed=0, snr_max=30.0, noise=0.03):
    """(x, e, lens) and the oracle's result for g_loss = 1, computed once per module."""
    key = (shape, seed, snr_max, noise)
    if key not in _CASES:
        x, e, lens, planted = MO.make_case(*shape, seed=seed, noise=noise)
        _CASES[key] = (x, e, lens, MO.direct(x, e, lens, snr_max))
    return _CASES[key]


def _dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays)


def _run(x, e, lens, snr_max=30.0, g_loss=None, g_per=None):
    """cal_mixit_loss on device tensors and the gradient of g_loss * loss + sum g_per * per_utt -> numpy results."""
    e = e.detach().requires_grad_(True)
    before = e.detach().clone()
    loss, per_utt, snr, assign = ctn.cal_mixit_loss(x, e, lens, snr_max)
    obj = 0.0
    if g_loss is not None:
        obj = obj + loss * g_loss
    if g_per is not None:
        obj = obj + (per_utt * g_per).sum()
    (grad,) = torch.autograd.grad(obj, e)
    assert torch.equal(e.detach(), before), "the estimate was modified"
    return dict(loss=float(loss.detach()), per_utt=per_utt.detach().cpu().numpy(), snr=snr.cpu().numpy(), assign=assign.cpu().numpy(),
                grad=grad.cpu().numpy())


def _check(got, ref, x, e, lens, M, g_loss=None, g_per=None, tag=""):
    assert ref["margin"].min() >= 1e-3, "the oracle's own margin is too small for an exact comparison: %g" % ref["margin"].min()
    d_utt = np.abs(got["per_utt"].astype(np.float64) - ref["per_utt"]).max()
    d_snr = np.abs(got["snr"].astype(np.float64) - ref["snr"]).max()
    d_loss = abs(got["loss"] - ref["loss"])
    bound = MO.grad_bound(x, e, lens, ref["assign"], ref["coef"], g_loss=g_loss, g_per=g_per)
    diff = np.abs(got["grad"].astype(np.float64) - ref["grad"])
    ratio = float((diff[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print("%s per_utt %.2e dB, snr %.2e dB, loss %.2e dB (limit %.0e); gradient worst |d| / bound = %.3f, margin %.2f dB"
          % (tag, d_utt, d_snr, d_loss, TOL_DB, ratio, ref["margin"].min()))
    assert np.array_equal(got["assign"], MO.unpack(ref["assign"], M))
    assert d_utt <= TOL_DB and d_snr <= TOL_DB and d_loss <= TOL_DB
    assert (diff <= bound).all(), ratio
    beyond = np.broadcast_to(np.arange(e.shape[2])[None, None, :] >= np.clip(lens, 0, e.shape[2])[:, None, None], e.shape)
    assert (got["grad"][beyond] == 0).all()


@pytest.mark.parametrize("shape", MO.SHAPES)
def test_loss_assignment_and_gradient_equal_the_oracle(shape):
    x, e, lens, ref = case(shape)
    got = _run(*_dev(x, e, lens), g_loss=1.0)
    _check(got, ref, x, e, lens, shape[1], g_loss=1.0, tag=str(shape))


@pytest.mark.parametrize("shape,offset", [((3, 4, 4133), 1), ((3, 4, 4133), 3), ((2, 4, 8192), 1), ((2, 4, 8192), 0)])
def test_misaligned_rows_take_the_scalar_path_and_give_the_same_bits(shape, offset):
    """T = 4133: no row but the first is 16-byte aligned; a view `offset` floats into a buffer misaligns the base as well
    (also at T = 8192, where the aligned tensor takes the 16-byte loads).  The result is bitwise that of the aligned tensors."""
    B, M, T = shape
    x, e, lens, ref = case(shape)
    xd, ed, ld = _dev(x, e, lens)
    xo = torch.zeros(B * 2 * T + 4, device=DEV)[offset:offset + B * 2 * T].view(B, 2, T).copy_(xd)
    eo = torch.zeros(B * M * T + 4, device=DEV)[offset:offset + B * M * T].view(B, M, T).copy_(ed)
    assert eo.is_contiguous() and (eo.data_ptr() % 16 != 0) == (offset != 0)
    got = _run(xo, eo, ld, g_loss=1.0)
    _check(got, ref, x, e, lens, M, g_loss=1.0, tag="%s offset %d" % (shape, offset))
    base = _run(xd, ed, ld, g_loss=1.0)
    assert base["per_utt"].tobytes() == got["per_utt"].tobytes() and np.array_equal(base["assign"], got["assign"])
    assert base["grad"].tobytes() == got["grad"].tobytes() and base["snr"].tobytes() == got["snr"].tobytes()


@pytest.mark.parametrize("which", ["g_per", "g_loss", "both"])
def test_upstream_gradients(which):
    shape = (3, 4, 4133)
    x, e, lens, _ = case(shape)
    g_per = np.array([0.25, -1.5, 3.0], np.float32) if which != "g_loss" else None
    g_loss = 0.75 if which != "g_per" else None
    ref = MO.direct(x, e, lens, 30.0, g_loss=g_loss, g_per=g_per)
    got = _run(*_dev(x, e, lens), g_loss=g_loss, g_per=None if g_per is None else torch.from_numpy(g_per).to(DEV))
    _check(got, ref, x, e, lens, shape[1], g_loss=g_loss, g_per=g_per, tag=which)


@pytest.mark.parametrize("shape", [(5, 4, 8192), (5, 8, 4133)])
def test_an_utterance_gives_the_same_bits_alone_and_in_a_batch(shape):
    x, e, lens, _ = case(shape, seed=4)
    g = np.linspace(0.5, 2.5, shape[0]).astype(np.float32)
    xd, ed, ld, gd = _dev(x, e, lens, g)
    full = _run(xd, ed, ld, g_per=gd)
    for b in range(shape[0]):
        one = _run(xd[b:b + 1], ed[b:b + 1].contiguous(), ld[b:b + 1], g_per=gd[b:b + 1])
        assert one["per_utt"].tobytes() == full["per_utt"][b:b + 1].tobytes(), b
        assert np.array_equal(one["assign"], full["assign"][b:b + 1]) and one["snr"].tobytes() == full["snr"][b:b + 1].tobytes()
        assert one["grad"].tobytes() == full["grad"][b:b + 1].tobytes(), b


def test_no_threshold_on_noisy_estimates():
    shape = (3, 4, 4133)
    x, e, lens, ref = case(shape, seed=2, snr_max=None)
    got = _run(*_dev(x, e, lens), snr_max=None, g_loss=1.0)
    _check(got, ref, x, e, lens, shape[1], g_loss=1.0, tag="snr_max=None")
    assert (ref["snr"] > 0).all() and (ref["snr"] < 64).all()


def test_zero_length_and_clamped_lengths():
    shape = (3, 4, 4133)
    x, e, lens, _ = case(shape)
    lens = np.array([9000, 0, -7], np.int64)
    ref = MO.direct(x, e, lens)
    got = _run(*_dev(x, e, lens), g_loss=1.0)
    assert ref["margin"][0] >= 1e-3
    assert got["per_utt"][1] == 0 and got["per_utt"][2] == 0 and (got["assign"][1:] == 0).all() and (got["grad"][1:] == 0).all()
    assert abs(float(got["per_utt"][0]) - ref["per_utt"][0]) <= TOL_DB and abs(got["loss"] - ref["loss"]) <= TOL_DB
    assert np.array_equal(got["assign"][0], MO.unpack(ref["assign"], 4)[0])
    bound = MO.grad_bound(x, e, lens, ref["assign"], ref["coef"], g_loss=1.0)
    assert (np.abs(got["grad"] - ref["grad"]) <= bound).all()
    xs = x.copy()
    xs[2, 1] = 0.0                                                      # a silent reference: finite values
    s = _run(*_dev(xs, e, np.array([4133, 4133, 4133])), g_loss=1.0)
    assert np.isfinite(s["per_utt"]).all() and np.isfinite(s["grad"]).all() and np.isfinite(s["snr"]).all()


def test_graph_replay_equals_the_eager_call():
    """Forward plus backward captured once and replayed over new samples written into the same buffers: bitwise the eager
    results, which a read-back or a synchronisation inside the calls would make impossible to capture."""
    shape = (3, 4, 4133)
    sets = [case(shape, seed=s)[:3] for s in (0, 5, 6)]
    xs, es, ls = _dev(*sets[0])
    es.requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                      # warm up outside the capture
        loss, per_utt, snr, assign = ctn.cal_mixit_loss(xs, es, ls)
        torch.autograd.grad(loss, es)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, per_utt, snr, assign = ctn.cal_mixit_loss(xs, es, ls)
        (grad,) = torch.autograd.grad(loss, es)
    for x, e, lens in sets[1:] + sets[:1]:
        xd, ed, ld = _dev(x, e, lens)
        with torch.no_grad():
            xs.copy_(xd), es.copy_(ed), ls.copy_(ld)
        graph.replay()
        torch.cuda.synchronize()
        eager = _run(xd, ed, ld, g_loss=1.0)
        assert float(loss) == eager["loss"] and per_utt.detach().cpu().numpy().tobytes() == eager["per_utt"].tobytes()
        assert np.array_equal(assign.cpu().numpy(), eager["assign"]) and snr.cpu().numpy().tobytes() == eager["snr"].tobytes()
        assert grad.cpu().numpy().tobytes() == eager["grad"].tobytes()


def test_remix_reproduces_the_reported_snr():
    shape = (3, 6, 777)
    x, e, lens, ref = case(shape)
    xd, ed, ld = _dev(x, e, lens)
    loss, per_utt, snr, assign = ctn.cal_mixit_loss(xd, ed, ld)
    r = ctn.remix(ed, assign).double().cpu().numpy()
    tau = MO.threshold(30.0)
    worst = 0.0
    for b in range(shape[0]):
        n = int(lens[b])
        xb = x[b, :, :n].astype(np.float64)
        err, xx = ((r[b, :, :n] - xb) ** 2).sum(-1), (xb ** 2).sum(-1)
        worst = max(worst, np.abs(-10.0 * np.log10((err + tau * xx + MO.EPS) / (xx + MO.EPS)) - snr[b].cpu().numpy()).max())
    print("SNR of remix(e, assign) against the reported snr: %.2e dB" % worst)
    assert worst <= 1e-4


def test_rejects_what_the_kernels_do_not_take():
    x, e, lens = torch.zeros(2, 2, 64, device=DEV), torch.zeros(2, 4, 64, device=DEV), torch.tensor([64, 64], device=DEV)
    with pytest.raises(ctn.CtnError):
        ctn.cal_mixit_loss(x, e.double(), lens)
    with pytest.raises(ctn.CtnError):
        ctn.cal_mixit_loss(x, torch.zeros(2, 64, 4, device=DEV).transpose(1, 2), lens)
    loss, per_utt, snr, assign = ctn.cal_mixit_loss(x.cpu(), e, lens.cpu())        # references and lengths are moved over
    assert float(loss) == 0.0 and assign.shape == (2, 4) and assign.dtype == torch.int64 and assign.device == e.device


# ---- end to end --------------------------------------------------------------------------------------------------------------
def _corpus():
    rng = np.random.RandomState(3)
    arrays, speakers = [], []
    for u in range(16):
        n = int(rng.randint(6000, 12000))
        a = (rng.randn(n) * rng.uniform(0.05, 0.3)).astype(np.float32)
        arrays.append(a * (1.0 + 0.5 * np.sin(np.arange(n) / 300.0)).astype(np.float32))
        speakers.append("spk%d" % (u % 8))
    return ctn.DeviceCorpus.from_arrays(arrays, speakers, DEV)


CFG = dict(N=64, L=20, B=32, H=64, P=3, X=2, R=2)
ARGS = (1, 2, 0, 0, 5, None, 0, "", "final.pth.tar", 1000, 0, 0, "mixit")


def _solver(corpus, tmp_path, C, speakers, criterion):
    from conv_tasnet_amd.optim import FlatAdam
    from conv_tasnet_amd.solver import Solver
    torch.manual_seed(0)
    model = ctn.ConvTasNet(CFG["N"], CFG["L"], CFG["B"], CFG["H"], CFG["P"], CFG["X"], CFG["R"], C).to(DEV)
    opt = FlatAdam(model.parameters(), lr=1e-3)

    def loaders():
        tr = ctn.DynamicMixLoader(corpus, 2, 4000, num_speakers=speakers, steps_per_epoch=3, seed=31, rank=0)
        cv = ctn.DynamicMixLoader(corpus, 2, 4000, num_speakers=speakers, steps_per_epoch=1, seed=32, rank=0, reshuffle=False)
        return (ctn.MixtureOfMixtures(tr), ctn.MixtureOfMixtures(cv)) if speakers == 4 else (tr, cv)

    tr, cv = loaders()
    args = ARGS[:5] + (str(tmp_path),) + ARGS[6:]
    solver = Solver({"tr_loader": tr, "cv_loader": cv}, model, opt, args) if criterion is None else \
        Solver({"tr_loader": tr, "cv_loader": cv}, model, opt, args, criterion=criterion)
    return solver, model, opt, loaders


def _by_hand(model, opt, loaders, loss_of):
    """The Solver's epochs written out: set_epoch, forward, loss, zero_grad / backward / clipped step; validation without grad."""
    tr, cv = loaders()
    losses = []
    for epoch in range(2):
        model.train()
        tr.dataset.set_epoch(epoch)
        for mixture, lengths, refs in tr:
            loss = loss_of(refs, model(mixture), lengths)
            opt.zero_grad()
            loss.backward()
            opt.step(max_grad_norm=5, grad_scale=1.0)
            losses.append(loss.item())
        model.eval()
        with torch.no_grad():
            for mixture, lengths, refs in cv:
                losses.append(loss_of(refs, model(mixture), lengths).item())
    return losses


def test_solver_trains_with_the_mixit_criterion_end_to_end(tmp_path):
    corpus = _corpus()
    set_arith("fp32")
    try:
        solver, model, opt, loaders = _solver(corpus, tmp_path / "a", 4, 4, ctn.MixItCriterion(30.0))
        solver.train()
        got = list(solver.iter_losses)
        assert len(got) == 2 * (3 + 1) and all(np.isfinite(got)), got
        assert all(-30.0 - 1e-4 <= v <= 10.0 for v in got), got
        _, model2, opt2, loaders2 = _solver(corpus, tmp_path / "b", 4, 4, ctn.MixItCriterion(30.0))
        hand = _by_hand(model2, opt2, loaders2, lambda refs, est, lengths: ctn.cal_mixit_loss(refs, est, lengths, 30.0)[0])
        print("MixIT losses, Solver:", got, "by hand:", hand)
        assert got == hand
        # criterion=None on a 2-speaker loader: the losses cal_loss gives
        solver, model, opt, loaders = _solver(corpus, tmp_path / "c", 2, 2, None)
        solver.train()
        _, model2, opt2, loaders2 = _solver(corpus, tmp_path / "d", 2, 2, None)
        hand = _by_hand(model2, opt2, loaders2, lambda src, est, lengths: ctn.cal_loss(src, est, lengths)[0])
        print("PIT losses, Solver:", solver.iter_losses, "by hand:", hand)
        assert list(solver.iter_losses) == hand and len(hand) == 8
    finally:
        set_arith(DEFAULT_ARITH)
