"""GPU: the PIT-with-inactive-sources loss kernels (csrc/ctn_varpit.hip, varpit.py) against the numpy fp64 direct-form oracle in
varpit_oracle.py.

Limits (none of them comes from what the kernels give):
  * idx and active: exact.  Every case first asserts that the ORACLE's margin between the winner and the best permutation outside
    its tie class is at least 1e-3 dB, so a near-tie can never excuse a mismatch; inside a tie class the sums are bitwise equal
    and the first permutation in table order wins, in the oracle and in the kernel alike.  tests/test_varpit_cpu.py runs these
    shapes with seeds 0 and 1 on the CPU: the smallest margin is 2.2 dB, the moment form is within 3e-12 dB of the direct form.
  * per_utt, pair, loss: 5e-6 dB.  Each is one fp32 rounding of a value below 64 in magnitude (half an ulp: 1.9e-6).
  * gradient, elementwise: 8 * 2^-24 |scale_b / C c_i| (|e_i[t]| + a_i |s_j[t]|)  (varpit_oracle.grad_bound counts the roundings);
    exactly 0 for t >= len.
"""
import numpy as np
import pytest
import torch

import varpit_oracle as VO

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402

DEV = "cuda:0"
TOL_DB = 5e-6
_CASES = {}


def case(shape, seed=0, snr_max=30.0, counts=None):
    """(s, e, lens) and the oracle's result for g_loss = 1, computed once per module."""
    key = (shape, seed, snr_max, counts)
    if key not in _CASES:
        s, e, lens, planted = VO.make_case(*shape, seed=seed, active_counts=counts)
        _CASES[key] = (s, e, lens, VO.direct(s, e, lens, snr_max))
    return _CASES[key]


def _dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays)


def _run(s, e, lens, snr_max=30.0, inactive_snr_max=20.0, g_loss=None, g_per=None):
    """cal_varpit_loss on device tensors and the gradient of g_loss * loss + sum g_per * per_utt -> numpy results."""
    e = e.detach().requires_grad_(True)
    before = e.detach().clone()
    loss, per_utt, pair, idx, active = ctn.cal_varpit_loss(s, e, lens, snr_max, inactive_snr_max)
    obj = 0.0
    if g_loss is not None:
        obj = obj + loss * g_loss
    if g_per is not None:
        obj = obj + (per_utt * g_per).sum()
    (grad,) = torch.autograd.grad(obj, e)
    assert torch.equal(e.detach(), before), "the estimate was modified"
    assert idx.dtype == torch.int64 and active.dtype == torch.int32
    return dict(loss=float(loss.detach()), per_utt=per_utt.detach().cpu().numpy(), pair=pair.cpu().numpy(), idx=idx.cpu().numpy(),
                active=active.cpu().numpy(), grad=grad.cpu().numpy())


def _check(got, ref, s, e, lens, g_loss=None, g_per=None, tag=""):
    assert ref["margin"].min() >= 1e-3, "the oracle's own margin is too small for an exact comparison: %g" % ref["margin"].min()
    d_utt = np.abs(got["per_utt"].astype(np.float64) - ref["per_utt"]).max()
    d_pair = np.abs(got["pair"].astype(np.float64) - ref["pair"]).max()
    d_loss = abs(got["loss"] - ref["loss"])
    bound = VO.grad_bound(s, e, lens, ref, g_loss=g_loss, g_per=g_per)
    diff = np.abs(got["grad"].astype(np.float64) - ref["grad"])
    inside = np.broadcast_to(np.arange(e.shape[2])[None, None, :] < np.clip(lens, 0, e.shape[2])[:, None, None], e.shape)
    sel = inside & (bound > 0)
    ratio = float((diff[sel] / bound[sel]).max()) if sel.any() else 0.0
    print("%s per_utt %.2e dB, pair %.2e dB, loss %.2e dB (limit %.0e); gradient worst |d| / bound = %.3f, margin %.2f dB, largest "
          "|value| %.1f dB" % (tag, d_utt, d_pair, d_loss, TOL_DB, ratio, ref["margin"].min(), np.abs(ref["pair"]).max()))
    assert np.array_equal(got["idx"], ref["idx"])
    assert np.array_equal(got["active"], ref["active"])
    assert np.abs(ref["pair"]).max() < 64
    assert d_utt <= TOL_DB and d_pair <= TOL_DB and d_loss <= TOL_DB
    assert (diff[inside] <= bound[inside]).all(), ratio
    assert (got["grad"][~inside] == 0).all()


@pytest.mark.parametrize("shape", VO.SHAPES)
def test_loss_assignment_and_gradient_equal_the_oracle(shape):
    s, e, lens, ref = case(shape)
    got = _run(*_dev(s, e, lens), g_loss=1.0)
    _check(got, ref, s, e, lens, g_loss=1.0, tag=str(shape))
    assert (ref["active"].sum(1) == 1 + np.arange(shape[0]) % shape[1]).all()      # counts 1 .. C all occur (B >= C)


@pytest.mark.parametrize("shape,offset", [((4, 3, 4133), 1), ((4, 3, 4133), 3), ((5, 3, 8192), 1), ((5, 3, 8192), 3)])
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
    assert base["per_utt"].tobytes() == got["per_utt"].tobytes() and np.array_equal(base["idx"], got["idx"])
    assert base["grad"].tobytes() == got["grad"].tobytes() and base["pair"].tobytes() == got["pair"].tobytes()
    assert base["loss"] == got["loss"]


@pytest.mark.parametrize("which", ["g_per", "both"])
def test_upstream_gradients(which):
    shape = (4, 3, 4133)
    s, e, lens, _ = case(shape)
    g_per = np.array([0.25, -1.5, 3.0, 0.0], np.float32)
    g_loss = 0.75 if which == "both" else None
    ref = VO.direct(s, e, lens, g_loss=g_loss, g_per=g_per)
    got = _run(*_dev(s, e, lens), g_loss=g_loss, g_per=torch.from_numpy(g_per).to(DEV))
    _check(got, ref, s, e, lens, g_loss=g_loss, g_per=g_per, tag=which)
    if which == "g_per":
        assert (got["grad"][3] == 0).all()


@pytest.mark.parametrize("shape", [(5, 3, 8192), (3, 6, 777)])
def test_an_utterance_gives_the_same_bits_alone_and_in_a_batch(shape):
    s, e, lens, _ = case(shape, seed=1)
    g = np.linspace(0.5, 2.5, shape[0]).astype(np.float32)
    sd, ed, ld, gd = _dev(s, e, lens, g)
    full = _run(sd, ed, ld, g_per=gd)
    for b in range(shape[0]):
        one = _run(sd[b:b + 1], ed[b:b + 1].contiguous(), ld[b:b + 1], g_per=gd[b:b + 1])
        assert one["per_utt"].tobytes() == full["per_utt"][b:b + 1].tobytes(), b
        assert np.array_equal(one["idx"], full["idx"][b:b + 1]) and one["pair"].tobytes() == full["pair"][b:b + 1].tobytes()
        assert np.array_equal(one["active"], full["active"][b:b + 1])
        assert one["grad"].tobytes() == full["grad"][b:b + 1].tobytes(), b
    # and at another index: the batch reversed
    rev = _run(sd.flip(0).contiguous(), ed.flip(0).contiguous(), ld.flip(0).contiguous(), g_per=gd.flip(0).contiguous())
    assert rev["per_utt"][::-1].tobytes() == full["per_utt"].tobytes() and rev["grad"][::-1].tobytes() == full["grad"].tobytes()
    assert rev["pair"][::-1].tobytes() == full["pair"].tobytes()


def test_no_threshold():
    shape = (4, 3, 4133)
    s, e, lens, ref = case(shape, seed=1, snr_max=None)
    got = _run(*_dev(s, e, lens), snr_max=None, g_loss=1.0)
    _check(got, ref, s, e, lens, g_loss=1.0, tag="snr_max=None")
    ref0 = VO.direct(s, e, lens, 30.0, None)
    got0 = _run(*_dev(s, e, lens), inactive_snr_max=None, g_loss=1.0)
    _check(got0, ref0, s, e, lens, g_loss=1.0, tag="inactive_snr_max=None")


def test_zero_length_clamped_lengths_and_a_row_with_every_reference_silent():
    shape = (4, 3, 777)
    s, e, _, _ = case(shape, counts=(2, 3, 0, 1))
    lens = np.array([9000, 0, 700, -7], np.int64)
    ref = VO.direct(s, e, lens)
    got = _run(*_dev(s, e, lens), g_loss=1.0)
    _check(got, ref, s, e, lens, g_loss=1.0, tag="len 0 / all silent")
    assert got["per_utt"][1] == 0 and got["per_utt"][3] == 0 and (got["idx"][[1, 3]] == 0).all()
    assert (got["grad"][[1, 3]] == 0).all() and (got["active"][[1, 3]] == 0).all() and (got["pair"][[1, 3]] == 0).all()
    # every reference silent: one tie class, the first permutation, a finite loss that pushes every output down
    assert (ref["active"][2] == 0).all() and ref["margin"][2] == np.inf and got["idx"][2] == 0
    assert np.isfinite(got["per_utt"]).all() and np.isfinite(got["grad"]).all()
    assert (np.sign(got["grad"][2, :, :700]) == np.sign(e[2, :, :700])).all()


def test_graph_replay_equals_the_eager_call():
    """Forward plus backward captured once on one stream and replayed over new samples written into the same buffers: bitwise the
    eager results, which a read-back or a synchronisation inside the calls would make impossible to capture."""
    shape = (4, 3, 4133)
    sets = [case(shape, seed=k)[:3] for k in (0, 1, 2)]
    ss, es, ls = _dev(*sets[0])
    es.requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                      # warm up outside the capture
        loss, per_utt, pair, idx, active = ctn.cal_varpit_loss(ss, es, ls)
        torch.autograd.grad(loss, es)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, per_utt, pair, idx, active = ctn.cal_varpit_loss(ss, es, ls)
        (grad,) = torch.autograd.grad(loss, es)
    for s, e, lens in sets[1:] + sets[:1]:
        sd, ed, ld = _dev(s, e, lens)
        with torch.no_grad():
            ss.copy_(sd), es.copy_(ed), ls.copy_(ld)
        graph.replay()
        torch.cuda.synchronize()
        eager = _run(sd, ed, ld, g_loss=1.0)
        assert float(loss) == eager["loss"] and per_utt.detach().cpu().numpy().tobytes() == eager["per_utt"].tobytes()
        assert np.array_equal(idx.cpu().numpy(), eager["idx"]) and pair.cpu().numpy().tobytes() == eager["pair"].tobytes()
        assert np.array_equal(active.cpu().numpy(), eager["active"])
        assert grad.cpu().numpy().tobytes() == eager["grad"].tobytes()


def test_every_reference_active_without_threshold_is_the_plain_snr():
    """Guards against wiring the inactive branch everywhere: C = 2, both references active, tau = 0."""
    shape = (4, 2, 4133)
    s, e, lens, ref = case(shape, seed=3, snr_max=None, counts=(2, 2, 2, 2))
    got = _run(*_dev(s, e, lens), snr_max=None, g_loss=1.0)
    _check(got, ref, s, e, lens, g_loss=1.0, tag="plain SNR")
    plain = VO.plain_snr_pit(s, e, lens)
    assert (got["active"] == 1).all()
    assert np.abs(-got["per_utt"].astype(np.float64) - plain).max() <= TOL_DB
    assert (plain > 0).all() and (plain < 64).all()


def test_rejects_what_the_kernels_do_not_take():
    s, e, lens = torch.zeros(2, 3, 64, device=DEV), torch.zeros(2, 3, 64, device=DEV), torch.tensor([64, 64], device=DEV)
    with pytest.raises(ctn.CtnError):
        ctn.cal_varpit_loss(s, e.double(), lens)
    with pytest.raises(ctn.CtnError):
        ctn.cal_varpit_loss(s, torch.zeros(2, 64, 3, device=DEV).transpose(1, 2), lens)
    loss, per_utt, pair, idx, active = ctn.cal_varpit_loss(s.cpu(), e, lens.cpu())          # references and lengths are moved over
    assert float(loss) == 0.0 and idx.tolist() == [0, 0] and active.tolist() == [[0, 0, 0]] * 2 and pair.device == e.device
    assert ctn.varpit.assignment(torch.tensor([0, 5, 3], device=DEV), 3).tolist() == [[0, 1, 2], [2, 1, 0], [1, 2, 0]]
