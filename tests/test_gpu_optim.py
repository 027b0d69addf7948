"""GPU: FlatSGD and FlatAdam(weight_decay > 0) -- ctn_clip_sgd_step / ctn_clip_adam_l2_step against torch.optim.SGD / Adam,
the untouched weight_decay = 0 path, state interchange, the Solver trajectory against the CPU oracle, checkpoints, graph
replay and the bucketed backward."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import ctn_oracle as O

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd.optim import FlatAdam, FlatSGD  # noqa: E402
from conv_tasnet_amd.solver import Solver  # noqa: E402

DEV = "cuda:0"
SHAPES = [(7,), (3, 5), (64,), (13, 3), (1,), (4, 4, 2)]      # numel 7, 15, 39, 1: the flat tails of the kernels


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g).to(DEV) for s in SHAPES]


def _grads(seed, step):
    g = torch.Generator().manual_seed(1000 * seed + step)
    return [torch.randn(s, generator=g).to(DEV) for s in SHAPES]


def _twins(seed):
    """(flat-side parameters, torch-side parameters): equal values, separate storage."""
    base = _params(seed)
    return [torch.nn.Parameter(p.clone()) for p in base], [torch.nn.Parameter(p.clone()) for p in base]


def _feed(flat_opt, flat_ps, torch_ps, grads, grad_scale, max_norm):
    """The same gradient to both sides; the torch side gets grad_scale and clip_grad_norm_ applied first, as the fused
    kernels do.  -> the torch-side total norm."""
    for p, g in zip(flat_ps, grads):
        p.grad.copy_(g)                             # the .grad views into flat_grads
    for p, g in zip(torch_ps, grads):
        p.grad = g.clone() * grad_scale
    if max_norm > 0:
        return float(torch.nn.utils.clip_grad_norm_(torch_ps, max_norm))
    return float(torch.linalg.vector_norm(torch.cat([p.grad.reshape(-1) for p in torch_ps])))


def _flat_seg(opt, buf, i):
    p, o, n = opt._segments()[i]
    return buf[o:o + n].view(p.shape)


def _close(a, b, atol, what):
    d = float((a - b).abs().max())
    assert d <= atol, "%s differs by %.3e" % (what, d)


SGD_CASES = [  # momentum, dampening, nesterov, weight_decay, max_norm, grad_scale
    (0.0, 0.0, False, 0.0, 0.0, 1.0),
    (0.0, 0.0, False, 1e-4, 1.0, 0.5),
    (0.9, 0.0, False, 0.0, 1.0, 1.0),
    (0.9, 0.1, False, 1e-4, 0.0, 0.5),
    (0.9, 0.1, False, 0.0, 1.0, 1.0),
    (0.9, 0.0, True, 1e-4, 1.0, 1.0),
    (0.9, 0.0, True, 0.0, 0.0, 0.5),
]


@pytest.mark.parametrize("momentum,dampening,nesterov,wd,max_norm,gs", SGD_CASES)
def test_flat_sgd_matches_torch_sgd_on_identical_gradients(momentum, dampening, nesterov, wd, max_norm, gs):
    fp, tp = _twins(1)
    opt = FlatSGD(fp, lr=0.1, momentum=momentum, dampening=dampening, weight_decay=wd, nesterov=nesterov)
    ref = torch.optim.SGD(tp, lr=0.1, momentum=momentum, dampening=dampening, weight_decay=wd, nesterov=nesterov)
    assert (opt.momentum_buffer is None) == (momentum == 0)
    clipped = 0
    for step in range(10):
        total = _feed(opt, fp, tp, _grads(1, step), gs, max_norm)
        clipped += max_norm > 0 and total > max_norm
        opt.step(max_grad_norm=max_norm, grad_scale=gs)
        ref.step()
        assert abs(float(opt.last_total_norm) - total) <= 1e-6 * total
        for i, (a, b) in enumerate(zip(fp, tp)):
            _close(a.detach(), b.detach(), 2e-6, "param %d at step %d" % (i, step))
            if momentum != 0:
                _close(_flat_seg(opt, opt.momentum_buffer, i), ref.state[b]["momentum_buffer"], 2e-6,
                       "momentum buffer %d at step %d" % (i, step))
    assert clipped == (10 if max_norm > 0 else 0)             # unit-scale gradients of 128 elements: the clip is active
    moved = max(float((a.detach() - p0).abs().max()) for a, p0 in zip(fp, _params(1)))
    assert moved > 0.05


@pytest.mark.parametrize("max_norm,gs", [(0.0, 1.0), (1.0, 0.5), (1.0, 1.0), (0.0, 0.5)])
def test_flat_adam_l2_matches_torch_adam_weight_decay(max_norm, gs):
    fp, tp = _twins(2)
    opt = FlatAdam(fp, lr=1e-3, weight_decay=1e-4)
    ref = torch.optim.Adam(tp, lr=1e-3, weight_decay=1e-4)
    for step in range(10):
        total = _feed(opt, fp, tp, _grads(2, step), gs, max_norm)
        opt.step(max_grad_norm=max_norm, grad_scale=gs)
        ref.step()
        assert abs(float(opt.last_total_norm) - total) <= 1e-6 * total
    for i, (a, b) in enumerate(zip(fp, tp)):
        _close(a.detach(), b.detach(), 2e-6, "param %d" % i)
        _close(_flat_seg(opt, opt.exp_avg, i), ref.state[b]["exp_avg"], 2e-6, "exp_avg %d" % i)
        _close(_flat_seg(opt, opt.exp_avg_sq, i), ref.state[b]["exp_avg_sq"], 2e-6, "exp_avg_sq %d" % i)


def _sgd_rule(p, g, buf, gs, coef, lr, mom, damp, wd, nest, first):
    d = g * (gs * coef) + wd * p
    if mom != 0:
        buf = d.clone() if first else buf * mom + d * (1 - damp)
        d = d + mom * buf if nest else buf
    return p - lr * d, buf


@pytest.mark.parametrize("n", [1, 3, 4, 1027, 3 * 2 ** 20 + 3])
def test_sgd_and_adam_l2_kernels_on_raw_buffers_with_tails(n):
    """The C ABI directly on n not a multiple of 4 (the flat optimisers always pass multiples of 4) and on more vectors than one
    grid of 2048 blocks covers (grid-stride); two runs are bitwise equal (no atomics)."""
    g = torch.Generator().manual_seed(n)
    p0, grad, b0 = (torch.randn(n, generator=g).to(DEV) for _ in range(3))
    ws = torch.empty(ctn.lib.ctn_optim_parts(), dtype=torch.float64, device=DEV)
    norm = torch.zeros(1, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    total = float(torch.linalg.vector_norm(grad.double())) * 0.5
    coef = min(1.0, 2.0 / (total + 1e-6))
    outs = []
    for _ in range(2):
        p, buf = p0.clone(), b0.clone()
        ctn.lib.call("ctn_clip_sgd_step", p.data_ptr(), grad.data_ptr(), buf.data_ptr(), n, 0.5, 2.0, 0.1, 0.9, 0.1,
                     1e-4, 0, 0, norm.data_ptr(), ws.data_ptr(), stream)
        outs.append((p, buf))
    rp, rb = _sgd_rule(p0, grad, b0, 0.5, coef, 0.1, 0.9, 0.1, 1e-4, False, False)
    _close(outs[0][0], rp, 2e-6, "params")
    _close(outs[0][1], rb, 2e-6, "momentum buffer")
    assert abs(float(norm) - total) <= 1e-6 * total
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    # momentum 0: no buffer at all
    p = p0.clone()
    ctn.lib.call("ctn_clip_sgd_step", p.data_ptr(), grad.data_ptr(), 0, n, 0.5, 2.0, 0.1, 0.0, 0.0, 1e-4, 0, 1,
                 norm.data_ptr(), ws.data_ptr(), stream)
    _close(p, _sgd_rule(p0, grad, None, 0.5, coef, 0.1, 0.0, 0.0, 1e-4, False, True)[0], 2e-6, "params (momentum 0)")
    # Adam + L2, first step
    p, m, v = p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    ctn.lib.call("ctn_clip_adam_l2_step", p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), n, 0.5, 2.0, 1e-3,
                 0.9, 0.999, 1e-8, 1, 1e-4, norm.data_ptr(), ws.data_ptr(), stream)
    gi = grad * (0.5 * coef) + 1e-4 * p0
    rm, rv = 0.1 * gi, 0.001 * gi * gi
    rp = p0 - 1e-3 / 0.1 * rm / (rv.sqrt() / 0.001 ** 0.5 + 1e-8)
    _close(m, rm, 1e-7, "exp_avg")
    _close(v, rv, 1e-7, "exp_avg_sq")
    _close(p, rp, 2e-6, "params (Adam + L2)")


def test_flat_adam_without_weight_decay_is_bitwise_the_existing_kernel():
    fp, _ = _twins(3)
    opt = FlatAdam(fp, lr=1e-3, weight_decay=0)
    params, m, v = opt.flat_params.clone(), torch.zeros_like(opt.exp_avg), torch.zeros_like(opt.exp_avg_sq)
    ws = torch.empty_like(opt._ws)
    norm = torch.zeros(1, device=DEV)
    for step in range(1, 4):
        for p, g in zip(fp, _grads(3, step)):
            p.grad.copy_(g)
        grads = opt.flat_grads.clone()
        opt.step(max_grad_norm=1.0, grad_scale=0.5)
        ctn.lib.call("ctn_clip_adam_step", params.data_ptr(), grads.data_ptr(), m.data_ptr(), v.data_ptr(), opt.numel,
                     0.5, 1.0, 1e-3, 0.9, 0.999, 1e-8, step, norm.data_ptr(), ws.data_ptr(),
                     torch.cuda.current_stream().cuda_stream)
    assert torch.equal(opt.flat_params, params)
    assert torch.equal(opt.exp_avg, m) and torch.equal(opt.exp_avg_sq, v)
    assert torch.equal(opt.last_total_norm, norm)


def _run_pair(opt_a, ps_a, opt_b, ps_b, seed, step, flat_a=True):
    """One more step of both with the same gradient, clip 1."""
    grads = _grads(seed, step)
    for opt, ps, flat in ((opt_a, ps_a, flat_a), (opt_b, ps_b, not flat_a)):
        for p, g in zip(ps, grads):
            if flat:
                p.grad.copy_(g)
            else:
                p.grad = g.clone()
        if flat:
            opt.step(max_grad_norm=1.0)
        else:
            torch.nn.utils.clip_grad_norm_(ps, 1.0)
            opt.step()


@pytest.mark.parametrize("momentum", [0.9, 0.0])
def test_flat_sgd_state_interchanges_with_torch_sgd(momentum):
    fp, tp = _twins(4)
    opt = FlatSGD(fp, lr=0.1, momentum=momentum, weight_decay=1e-4)
    for step in range(3):
        for p, g in zip(fp, _grads(4, step)):
            p.grad.copy_(g)
        opt.step(max_grad_norm=1.0)
    sd = opt.state_dict()
    ref_keys = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))]).state_dict()["param_groups"][0].keys()
    assert sd["param_groups"][0].keys() == ref_keys
    assert sd["param_groups"][0]["params"] == list(range(len(SHAPES)))
    if momentum == 0:
        assert sd["state"] == {}
    else:
        assert sorted(sd["state"]) == list(range(len(SHAPES)))
        assert all(set(st) == {"momentum_buffer"} for st in sd["state"].values())
    with torch.no_grad():
        for a, b in zip(tp, fp):
            a.copy_(b)
    ref = torch.optim.SGD(tp, lr=0.5, momentum=momentum)
    ref.load_state_dict(sd)
    assert ref.param_groups[0]["lr"] == 0.1 and ref.param_groups[0]["weight_decay"] == 1e-4
    _run_pair(opt, fp, ref, tp, 4, 3)
    for a, b in zip(fp, tp):
        _close(a.detach(), b.detach(), 2e-6, "param after the torch step")
    # and back: torch.optim.SGD state -> FlatSGD
    fp2 = [torch.nn.Parameter(b.detach().clone()) for b in tp]
    opt2 = FlatSGD(fp2, lr=0.5)
    opt2.load_state_dict(ref.state_dict())
    g = opt2.param_groups[0]
    assert (g["lr"], g["momentum"], g["weight_decay"]) == (0.1, momentum, 1e-4)
    if momentum != 0:
        for i, b in enumerate(tp):
            assert torch.equal(_flat_seg(opt2, opt2.momentum_buffer, i), ref.state[b]["momentum_buffer"])
    _run_pair(opt2, fp2, ref, tp, 4, 4)
    for a, b in zip(fp2, tp):
        _close(a.detach(), b.detach(), 2e-6, "param after the reloaded flat step")


def test_flat_adam_state_round_trips_weight_decay():
    fp, tp = _twins(5)
    opt = FlatAdam(fp, lr=1e-3, weight_decay=1e-4)
    for step in range(2):
        for p, g in zip(fp, _grads(5, step)):
            p.grad.copy_(g)
        opt.step(max_grad_norm=1.0)
    sd = opt.state_dict()
    assert sd["param_groups"][0]["weight_decay"] == 1e-4
    ref = torch.optim.Adam(tp, lr=1e-3)
    ref.load_state_dict(sd)
    assert ref.param_groups[0]["weight_decay"] == 1e-4
    opt2 = FlatAdam([torch.nn.Parameter(p.detach().clone()) for p in fp], lr=1e-3)
    opt2.load_state_dict(ref.state_dict())
    assert opt2.param_groups[0]["weight_decay"] == 1e-4 and opt2._step == 2
    assert torch.equal(opt2.exp_avg, opt.exp_avg)


# ---- the training loop -----------------------------------------------------------------------------------------------------
LR, MOM, WD, CLIP = 1e-2, 0.9, 1e-4, 5.0


def _traj_setup():
    g = load_golden("solver_traj")
    N, L, B, H, P, X, R, C = [int(v) for v in g["cfg"]]
    m = ctn.ConvTasNet(N, L, B, H, P, X, R, C)
    m.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("p0:")})
    T = int(g["T"])
    batches = [O.synth_batch(900 + 2 * i, 2, T) for i in range(3)]
    return g, m.to(DEV), batches


def _oracle_sgd_trajectory(g, batches, epochs):
    """fp32 CPU oracle: forward, PIT loss, autograd, clip_grad_norm_ rule, then torch.optim.SGD's update (momentum,
    weight decay) written out; fixed LR.  -> (training losses, final parameters)."""
    cfg = O.Config(*[int(v) for v in g["cfg"]])
    names = list(O.param_shapes(cfg).keys())
    sd = {n: torch.from_numpy(g["p0:" + n]).clone() for n in names}
    bufs, losses = {}, []
    for _ in range(epochs):
        for mix, lens, src in batches:
            leaves = {n: sd[n].detach().requires_grad_(True) for n in names}
            loss = O.cal_loss(src, O.forward(cfg, leaves, mix), lens)[0]
            grads = torch.autograd.grad(loss, [leaves[n] for n in names])
            _, coef = O.clip_coef(list(grads), CLIP)
            with torch.no_grad():
                for n, gr in zip(names, grads):
                    d = gr * coef + WD * sd[n]
                    bufs[n] = d.clone() if n not in bufs else bufs[n] * MOM + d
                    sd[n] = sd[n] - LR * bufs[n]
            losses.append(float(loss.detach()))
    return losses, sd


def _solver(m, opt, batches, folder, epochs=2, checkpoint=0, continue_from=""):
    arg = (1, epochs, 0, 0, CLIP, str(folder), checkpoint, continue_from, "final.pth.tar", 1000, 0, 0, "x")
    return Solver({"tr_loader": batches, "cv_loader": batches[:1]}, m, opt, arg)


def _train_losses(s, n_train, n_cv, epochs):
    per = n_train + n_cv
    return [v for i, v in enumerate(s.iter_losses) if i % per < n_train][:n_train * epochs]


def test_solver_with_flat_sgd_follows_the_oracle_and_torch_sgd(tmp_path):
    g, m, batches = _traj_setup()
    opt = FlatSGD(m.parameters(), lr=LR, momentum=MOM, weight_decay=WD)
    s = _solver(m, opt, batches, tmp_path / "flat")
    s.train()
    assert len(s.iter_losses) == 2 * 4
    losses = _train_losses(s, 3, 1, 2)
    ref_losses, ref_sd = _oracle_sgd_trajectory(g, batches, 2)
    np.testing.assert_allclose(losses, ref_losses, atol=1e-3)
    assert abs(ref_losses[-1] - ref_losses[0]) > 1e-2             # the trajectory moved
    for k, v in m.state_dict().items():
        np.testing.assert_allclose(v.cpu().numpy(), ref_sd[k].numpy(), atol=3e-4, err_msg=k)
    # the generic branch of Solver._optimise with torch.optim.SGD over the same model
    _, m2, _ = _traj_setup()
    s2 = _solver(m2, torch.optim.SGD(m2.parameters(), lr=LR, momentum=MOM, weight_decay=WD), batches, tmp_path / "torch")
    s2.train()
    np.testing.assert_allclose(_train_losses(s2, 3, 1, 2), losses, atol=1e-3)
    for (k, a), (_, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), atol=3e-4, err_msg=k)


def test_checkpoint_resume_with_flat_sgd(tmp_path):
    g, m, batches = _traj_setup()
    opt = FlatSGD(m.parameters(), lr=LR, momentum=MOM, weight_decay=WD)
    _solver(m, opt, batches, tmp_path, checkpoint=1).train()
    ck = tmp_path / "checkpoint_models" / "epoch2.pth.tar"
    assert ck.exists()
    m2 = ctn.ConvTasNet.load_model(str(ck)).to(DEV)
    opt2 = FlatSGD(m2.parameters(), lr=0.5, momentum=MOM)
    s2 = _solver(m2, opt2, batches, tmp_path, epochs=1, continue_from=str(ck))
    assert s2.start_epoch == 2 and s2.epochs == 1 + 2 + 1
    assert opt2.param_groups[0]["lr"] == LR and opt2.param_groups[0]["weight_decay"] == WD
    assert opt2._buf_init and torch.equal(opt2.momentum_buffer, opt.momentum_buffer)
    assert torch.equal(opt2.flat_params, opt.flat_params)
    s2.train()
    assert len(s2.iter_losses) == 2 * 4 and np.isfinite(s2.iter_losses).all()
    assert not torch.equal(opt2.flat_params, opt.flat_params)

    # a checkpoint written with torch.optim.SGD loads into FlatSGD
    _, m3, _ = _traj_setup()
    opt3 = torch.optim.SGD(m3.parameters(), lr=LR, momentum=MOM, weight_decay=WD)
    _solver(m3, opt3, batches, tmp_path / "torch", epochs=1, checkpoint=1).train()
    ck3 = tmp_path / "torch" / "checkpoint_models" / "epoch1.pth.tar"
    m4 = ctn.ConvTasNet.load_model(str(ck3)).to(DEV)
    opt4 = FlatSGD(m4.parameters(), lr=0.5)
    s4 = _solver(m4, opt4, batches, tmp_path / "torch", epochs=1, continue_from=str(ck3))
    assert opt4.param_groups[0]["momentum"] == MOM and opt4.param_groups[0]["lr"] == LR
    for i, p in enumerate(m3.parameters()):
        assert torch.equal(_flat_seg(opt4, opt4.momentum_buffer, i), opt3.state[p]["momentum_buffer"])
    s4.train()
    assert np.isfinite(s4.iter_losses).all()


def test_graphed_backprop_with_flat_sgd_replays_the_eager_step():
    from conv_tasnet_amd.graphed import GraphedBackprop
    from conv_tasnet_amd.train import SyntheticLoader
    cfg = dict(N=64, L=20, B=32, H=64, P=3, X=3, R=2, C=2)
    batches = list(SyntheticLoader(3, 2, samples=8000))

    def run(graph):
        torch.manual_seed(3)
        model = ctn.ConvTasNet(**cfg).to(DEV)
        opt = FlatSGD(model.parameters(), lr=1e-2, momentum=0.9)
        stepper = GraphedBackprop(model, opt, batches[0]) if graph else None
        losses, grads = [], []
        for mix, lens, src in batches:
            mix, lens, src = mix.to(DEV), lens.to(DEV), src.to(DEV)
            if graph:
                loss = stepper(mix, lens, src)
            else:
                opt.zero_grad()
                loss = ctn.cal_loss(src, model(mix), lens)[0]
                loss.backward()
            losses.append(float(loss.detach()))
            opt.step(max_grad_norm=5.0)
            grads.append(opt.flat_grads.clone())
        return losses, grads, opt.flat_params.clone(), opt.momentum_buffer.clone()

    l0, g0, p0, b0 = run(False)
    l1, g1, p1, b1 = run(True)
    assert l0 == l1
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)
    assert torch.equal(p0, p1) and torch.equal(b0, b1)


def test_solver_installs_the_bucketed_backward_for_flat_sgd(tmp_path, monkeypatch):
    from conv_tasnet_amd import ops, parallel

    class Stub:
        calls = 0

        def __init__(self, optimizer, blocks_per_bucket):
            self.opt, self.blocks_per_bucket = optimizer, blocks_per_bucket
            self.works, self.covered = [], []

        def bucket_ready(self, sinks):
            Stub.calls += 1

    torch.manual_seed(4)
    m = ctn.ConvTasNet(64, 20, 64, 128, 3, 2, 3, 2).to(DEV)
    opt = FlatSGD(m.parameters(), lr=1e-2, momentum=0.9)
    monkeypatch.setattr(parallel, "world_size", lambda: 2)         # what enable_overlap sees in an N-rank job
    monkeypatch.setattr(parallel, "GradientBuckets", Stub)
    try:
        _solver(m, opt, [], tmp_path)
        gb = opt._ctn_buckets
        assert isinstance(gb, Stub) and ops._GRAD_BUCKETS is gb and gb.blocks_per_bucket == 2
        monkeypatch.undo()
        mix, lens, src = O.synth_batch(40, 3, 4005)
        mix, lens, src = mix.to(DEV), lens.to(DEV), src.to(DEV)
        grads = []
        for buckets in (None, gb):
            ops.set_grad_buckets(buckets)
            opt.zero_grad()
            ctn.cal_loss(src, m(mix), lens)[0].backward()
            ops.join_side_stream(opt.flat_grads.device)
            torch.cuda.synchronize()
            grads.append(opt.flat_grads.clone())
        assert Stub.calls == 3                                      # X = 2 blocks per bucket, R = 3 repeats
        assert float(grads[0].abs().max()) > 0
        assert torch.equal(grads[0], grads[1]), "%d gradient elements differ" % int((grads[0] != grads[1]).sum())
    finally:
        ops.set_grad_buckets(None)
