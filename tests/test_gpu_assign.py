"""GPU: optimal-assignment PIT (csrc/ctn_assign.hip, assign.py) against the numpy fp64 direct-form oracle in assign_oracle.py.

Limits (none of them comes from what the kernels give):
  * perm: exact.  Every case first asserts that the ORACLE's margin -- the loss in mean SI-SNR of the best other assignment -- is at
    least 1e-3 dB, so a near-tie can never excuse a mismatch.  The returned perm also equals assign_oracle.solve applied to the
    device's own returned pair matrix, exactly: the solver is a function of the stored fp32 matrix and is restated bit for bit.
    tests/test_assign_cpu.py runs these shapes with seeds 0 and 1 on the CPU: the smallest margin is 0.32 dB at (5,16,129), the
    moment form is within 2e-12 dB of the direct form, the planted permutation is the optimum everywhere.
  * pair, max_snr, loss: 5e-6 dB.  Each is one fp32 rounding of a value asserted below 128 in magnitude (half an ulp: 3.8e-6).
  * gradient, elementwise: assign_oracle.grad_bound (10 half-ulps of |scale_b| (|A| (|s_j| + |mean s_j|) + |B| (|e_i| + |mean e_i|)),
    its docstring counts the roundings); exactly 0 for t >= len.
"""
import numpy as np
import pytest
import torch

import assign_oracle as AO

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402

DEV = "cuda:0"
TOL_DB = 5e-6
SOLVER_C = [1, 2, 3, 5, 8, 13, 16]
_CASES = {}


def case(shape, seed=0):
    """(s, e, lens) and the oracle's result for g_loss = 1, computed once per module."""
    key = (shape, seed)
    if key not in _CASES:
        s, e, lens, _ = AO.make_case(*shape, seed=seed)
        _CASES[key] = (s, e, lens, AO.direct(s, e, lens))
    return _CASES[key]


def _dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays)


def _run(s, e, lens, g_loss=None, g_max=None):
    """cal_assign_loss on device tensors and the gradient of g_loss * loss + sum g_max * max_snr -> numpy results."""
    e = e.detach().requires_grad_(True)
    before = e.detach().clone()
    loss, max_snr, pair, perm = ctn.cal_assign_loss(s, e, lens)
    obj = 0.0
    if g_loss is not None:
        obj = obj + loss * g_loss
    if g_max is not None:
        obj = obj + (max_snr[:, 0] * g_max).sum()
    (grad,) = torch.autograd.grad(obj, e)
    assert torch.equal(e.detach(), before), "the estimate was modified"
    assert perm.dtype == torch.int64 and max_snr.shape == (e.size(0), 1) and pair.shape == (e.size(0), e.size(1), e.size(1))
    return dict(loss=float(loss.detach()), max_snr=max_snr.detach().cpu().numpy()[:, 0], pair=pair.cpu().numpy(),
                perm=perm.cpu().numpy(), grad=grad.cpu().numpy())


def _check(got, ref, s, e, lens, g_loss=None, g_max=None, tag=""):
    assert ref["margin"].min() >= 1e-3, "the oracle's own margin is too small for an exact comparison: %g" % ref["margin"].min()
    d_max = np.abs(got["max_snr"].astype(np.float64) - ref["max_snr"]).max()
    d_pair = np.abs(got["pair"].astype(np.float64) - ref["pair"]).max()
    d_loss = abs(got["loss"] - ref["loss"])
    bound = AO.grad_bound(s, e, lens, ref, g_loss=g_loss, g_max=g_max)
    diff = np.abs(got["grad"].astype(np.float64) - ref["grad"])
    inside = np.broadcast_to(np.arange(e.shape[2])[None, None, :] < np.clip(lens, 0, e.shape[2])[:, None, None], e.shape)
    sel = inside & (bound > 0)
    ratio = float((diff[sel] / bound[sel]).max()) if sel.any() else 0.0
    print("%s max_snr %.2e dB, pair %.2e dB, loss %.2e dB (limit %.0e); gradient worst |d| / bound = %.3f, margin %.3f dB, largest "
          "|value| %.1f dB" % (tag, d_max, d_pair, d_loss, TOL_DB, ratio, ref["margin"].min(), np.abs(ref["pair"]).max()))
    assert np.array_equal(got["perm"], ref["perm"])
    assert np.array_equal(got["perm"], AO.solve(got["pair"], True))        # a function of the stored matrix, restated bit for bit
    assert np.abs(ref["pair"]).max() < 128
    assert d_max <= TOL_DB and d_pair <= TOL_DB and d_loss <= TOL_DB
    assert (diff[inside] <= bound[inside]).all(), ratio
    assert (got["grad"][~inside] == 0).all()


@pytest.mark.parametrize("shape", AO.SHAPES)
def test_loss_pair_matrix_permutation_and_gradient_equal_the_oracle(shape):
    s, e, lens, ref = case(shape)
    got = _run(*_dev(s, e, lens), g_loss=1.0)
    _check(got, ref, s, e, lens, g_loss=1.0, tag=str(shape))


@pytest.mark.parametrize("which", ["g_max", "both"])
def test_upstream_gradients(which):
    shape = (3, 7, 777)
    s, e, lens, _ = case(shape)
    g_max = np.array([0.25, -1.5, 0.0], np.float32)
    g_loss = 0.75 if which == "both" else None
    ref = AO.direct(s, e, lens, g_loss=g_loss, g_max=g_max)
    got = _run(*_dev(s, e, lens), g_loss=g_loss, g_max=torch.from_numpy(g_max).to(DEV))
    _check(got, ref, s, e, lens, g_loss=g_loss, g_max=g_max, tag=which)
    if which == "g_max":
        assert (got["grad"][2] == 0).all() and (got["grad"][0] != 0).any()


@pytest.mark.parametrize("shape,offset", [((3, 16, 4133), 1), ((3, 16, 4133), 3), ((2, 16, 8192), 1), ((2, 16, 8192), 3)])
def test_misaligned_rows_take_the_scalar_path_and_give_the_same_bits(shape, offset):
    """T = 4133: no row but the first is 16-byte aligned; a view `offset` floats into a buffer misaligns the base as well (also
    at T = 8192, where the aligned tensor takes the 16-byte loads).  The result is bitwise that of the aligned tensors."""
    B, C, T = shape
    s, e, lens, ref = case(shape)
    sd, ed, ld = _dev(s, e, lens)
    so = torch.zeros(B * C * T + 4, device=DEV)[offset:offset + B * C * T].view(B, C, T).copy_(sd)
    eo = torch.zeros(B * C * T + 4, device=DEV)[offset:offset + B * C * T].view(B, C, T).copy_(ed)
    assert eo.is_contiguous() and eo.data_ptr() % 16 != 0 and so.data_ptr() % 16 != 0
    got = _run(so, eo, ld, g_loss=1.0)
    _check(got, ref, s, e, lens, g_loss=1.0, tag="%s offset %d" % (shape, offset))
    base = _run(sd, ed, ld, g_loss=1.0)
    assert sd.data_ptr() % 16 == 0 and ed.data_ptr() % 16 == 0
    assert base["max_snr"].tobytes() == got["max_snr"].tobytes() and np.array_equal(base["perm"], got["perm"])
    assert base["grad"].tobytes() == got["grad"].tobytes() and base["pair"].tobytes() == got["pair"].tobytes()
    assert base["loss"] == got["loss"]


def test_an_utterance_gives_the_same_bits_alone_and_in_a_batch():
    shape = (3, 16, 4133)
    s, e, lens, _ = case(shape, seed=1)
    g = np.linspace(0.5, 2.5, shape[0]).astype(np.float32)                # g_max: no 1 / B in the gradient
    sd, ed, ld, gd = _dev(s, e, lens, g)
    full = _run(sd, ed, ld, g_max=gd)
    for b in range(shape[0]):
        one = _run(sd[b:b + 1], ed[b:b + 1].contiguous(), ld[b:b + 1], g_max=gd[b:b + 1])
        assert one["max_snr"].tobytes() == full["max_snr"][b:b + 1].tobytes(), b
        assert np.array_equal(one["perm"], full["perm"][b:b + 1]) and one["pair"].tobytes() == full["pair"][b:b + 1].tobytes()
        assert one["grad"].tobytes() == full["grad"][b:b + 1].tobytes(), b
    # and at another index: the batch reversed
    rev = _run(sd.flip(0).contiguous(), ed.flip(0).contiguous(), ld.flip(0).contiguous(), g_max=gd.flip(0).contiguous())
    assert rev["max_snr"][::-1].tobytes() == full["max_snr"].tobytes() and rev["grad"][::-1].tobytes() == full["grad"].tobytes()
    assert rev["pair"][::-1].tobytes() == full["pair"].tobytes() and np.array_equal(rev["perm"][::-1], full["perm"])


@pytest.mark.parametrize("C", SOLVER_C)
def test_linear_assignment_is_the_restated_solver_and_reaches_scipys_optimum(C):
    """The CPU test's matrices, ties included, both senses: the device's permutation equals assign_oracle.solve exactly and has
    scipy's optimum value."""
    mats = AO.solver_matrices(C)
    (md,) = _dev(mats)
    for maximize in (True, False):
        perm = ctn.linear_assignment(md, maximize=maximize)
        assert perm.dtype == torch.int32 and perm.shape == (len(mats), C)
        got = perm.cpu().numpy().astype(np.int64)
        assert np.array_equal(got, AO.solve(mats, maximize))
        assert np.abs(AO.value(mats, got) - AO.scipy_value(mats, maximize)).max() <= 1e-9
    assert torch.equal(ctn.linear_assignment(md[3]), ctn.linear_assignment(md)[3])


def test_linear_assignment_over_more_matrices_than_one_round_of_waves():
    mats = AO.solver_matrices(16, count=256, seed=1)
    assert mats.shape == (257, 16, 16)
    got = ctn.linear_assignment(_dev(mats)[0]).cpu().numpy().astype(np.int64)
    assert np.array_equal(got, AO.solve(mats, True))
    assert np.abs(AO.value(mats, got) - AO.scipy_value(mats, True)).max() <= 1e-9


def test_mixed_estimates_where_greedy_matching_fails():
    """Every estimate a mixture of all references (tests/test_assign_cpu.py: the row-wise argmax is no permutation, margins from
    0.002 dB): the loss path finds scipy's assignment."""
    s, e, lens = AO.make_mixed_case(4, 16, 2049, seed=16)
    ref = AO.direct(s, e, lens)
    got = _run(*_dev(s, e, lens), g_loss=1.0)
    assert not any(AO.is_permutation(got["pair"][b].argmax(1)) for b in range(4))
    _check(got, ref, s, e, lens, g_loss=1.0, tag="mixed")


@pytest.mark.parametrize("shape", [(4, 2, 4133), (4, 3, 4133), (3, 6, 777)])
def test_agrees_with_cal_loss_where_both_run(shape):
    """perm is the permutation cal_loss picks; max_snr within the two paths' documented limits against fp64 (1e-4 dB for cal_loss,
    tests/test_gpu_loss.py; 5e-6 dB here); and the reordered estimate really is in its references' order: scored row by row with
    evaluate.cal_SISNR it reproduces the matched entries of pair to 1e-4 dB."""
    from conv_tasnet_amd import ops
    from conv_tasnet_amd.evaluate import cal_SISNR
    B, C, T = shape
    s, e, lens, _ = AO.make_case(B, C, T, seed=2)
    sd, ed, ld = _dev(s, e, lens)
    loss_a, max_a, pair, perm = ctn.cal_assign_loss(sd, ed, ld)
    loss_p, max_p, _, _ = ctn.cal_loss(sd, ed.clone(), ld)
    _, perms, idx = ctn.cal_si_snr_with_pit(sd, ed.clone(), ld)
    assert torch.equal(perm, ops._perms(C, sd.device)[1][idx])
    assert (max_a - max_p).abs().max().item() <= 1e-4 + TOL_DB and abs(float(loss_a) - float(loss_p)) <= 1e-4 + TOL_DB
    out = ctn.reorder_estimate(ed, perm).double().cpu().numpy()
    worst = 0.0
    for b in range(B):
        n = int(lens[b])
        for i in range(C):
            j = int(perm[b, i])
            worst = max(worst, abs(cal_SISNR(s[b, j, :n].astype(np.float64), out[b, j, :n]) - float(pair[b, i, j])))
    print("%s: reordered rows against pair: %.2e dB" % (shape, worst))
    assert worst <= 1e-4


def test_forward_and_backward_neither_read_back_nor_synchronise():
    s, e, lens, _ = case((3, 7, 777))
    sd, ed, ld = _dev(s, e, lens)
    ref = _run(sd, ed, ld, g_loss=1.0)                                    # the warm-up: allocator blocks, the library
    score = _dev(AO.solver_matrices(5))[0]
    ref_perm = ctn.linear_assignment(score)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):                                 # the mode is enforced: a read-back raises
            ed[0, 0, 0].item()
        er = ed.detach().requires_grad_(True)
        loss, max_snr, pair, perm = ctn.cal_assign_loss(sd, er, ld)
        (grad,) = torch.autograd.grad(loss, er)
        out = ctn.reorder_estimate(ed, perm)
        perm5 = ctn.linear_assignment(score)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert float(loss) == ref["loss"] and grad.cpu().numpy().tobytes() == ref["grad"].tobytes()
    assert np.array_equal(perm.cpu().numpy(), ref["perm"]) and torch.equal(perm5, ref_perm) and out.shape == ed.shape


def test_graph_replay_equals_the_eager_call():
    """Forward plus backward captured once on one stream and replayed over new samples written into the same buffers: bitwise the
    eager results, which a read-back or a synchronisation inside the calls would make impossible to capture."""
    shape = (3, 7, 777)
    sets = [case(shape, seed=k)[:3] for k in (0, 1, 2)]
    ss, es, ls = _dev(*sets[0])
    es.requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                      # warm up outside the capture
        loss, max_snr, pair, perm = ctn.cal_assign_loss(ss, es, ls)
        torch.autograd.grad(loss, es)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, max_snr, pair, perm = ctn.cal_assign_loss(ss, es, ls)
        (grad,) = torch.autograd.grad(loss, es)
    for s, e, lens in sets[1:] + sets[:1]:
        sd, ed, ld = _dev(s, e, lens)
        with torch.no_grad():
            ss.copy_(sd), es.copy_(ed), ls.copy_(ld)
        graph.replay()
        torch.cuda.synchronize()
        eager = _run(sd, ed, ld, g_loss=1.0)
        assert float(loss) == eager["loss"] and max_snr.detach().cpu().numpy()[:, 0].tobytes() == eager["max_snr"].tobytes()
        assert np.array_equal(perm.cpu().numpy(), eager["perm"]) and pair.cpu().numpy().tobytes() == eager["pair"].tobytes()
        assert grad.cpu().numpy().tobytes() == eager["grad"].tobytes()


def test_rejects_what_the_kernels_do_not_take():
    s, e, lens = torch.zeros(2, 8, 64, device=DEV), torch.zeros(2, 8, 64, device=DEV), torch.tensor([64, 64], device=DEV)
    with pytest.raises(ctn.CtnError):
        ctn.cal_assign_loss(s, e.double(), lens)
    with pytest.raises(ctn.CtnError):
        ctn.cal_assign_loss(s, torch.zeros(2, 64, 8, device=DEV).transpose(1, 2), lens)
    with pytest.raises(ValueError):
        ctn.cal_assign_loss(torch.zeros(2, 17, 64, device=DEV), torch.zeros(2, 17, 64, device=DEV), lens)
    with pytest.raises(ctn.CtnError, match="C <= 6"):                    # what a user met before this loss existed
        ctn.cal_loss(s, e.clone(), lens)


def test_eight_speaker_model_trains_and_evaluates(tmp_path):
    """A TINY Conv-TasNet with 8 outputs: every parameter gets a gradient through the loss, two Solver steps run with
    AssignPitCriterion, and evaluate_loader scores the model through the solver's pairing and reorder_estimate."""
    from conv_tasnet_amd.evaluate import evaluate_loader
    from conv_tasnet_amd.optim import FlatAdam
    from conv_tasnet_amd.solver import Solver
    from conv_tasnet_amd.train import TINY
    C, B, T = 8, 2, 4000
    rng = np.random.default_rng(3)
    batches = []
    for k in range(2):
        src = torch.from_numpy((rng.standard_normal((B, C, T)) * rng.uniform(0.1, 0.5, (B, C, 1))).astype(np.float32))
        lens = torch.tensor([T, T - 37 * (k + 1)])
        for b in range(B):
            src[b, :, int(lens[b]):] = 0
        batches.append((src.sum(1), lens, src))
    torch.manual_seed(0)
    cfg = dict(TINY, C=C)
    m = ctn.ConvTasNet(cfg['N'], cfg['L'], cfg['B'], cfg['H'], cfg['P'], cfg['X'], cfg['R'], cfg['C']).to(DEV)
    mixture, lens, src = batches[0]
    loss = ctn.AssignPitCriterion()(src.to(DEV), m(mixture.to(DEV)), lens.to(DEV))
    loss.backward()
    assert torch.isfinite(loss)
    for name, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, name
    m.zero_grad()
    opt = FlatAdam(m.parameters(), lr=1e-3)
    args = (1, 1, 0, 0, 5, str(tmp_path), 0, "", "final.pth.tar", 1000, 0, 0, "assign")
    before = next(m.parameters()).detach().clone()
    s = Solver({"tr_loader": batches, "cv_loader": batches[:1]}, m, opt, args, criterion=ctn.AssignPitCriterion())
    s.train()
    assert np.isfinite(float(s.tr_loss[0])) and np.isfinite(float(s.cv_loss[0]))
    assert not torch.equal(before, next(m.parameters()).detach())
    sisnri = evaluate_loader(m, batches[:1], verbose=False)
    assert isinstance(sisnri, float) and np.isfinite(sisnri)
