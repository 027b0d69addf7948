"""GPU: the cumulative LayerNorm (csrc/ctn_cumln.hip) -- its four entry points against the fp64 closed forms of tests/cumln_oracle.py
under the cLN family's limits (out / mean / rstd 2e-5, dY / dgamma / dbeta 5e-5, sums 1e-5 of the sum of |terms|), the device-side
carry (a stream cut anywhere gives the bits of one call), causality, the TemporalBlock chain (ops.CumLnBlock) against an fp64 torch
restatement, and the model level: streaming, graph replay, the fused classes' refusal, one Solver epoch."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cumln_oracle as C  # noqa: E402
import norm_oracle as N  # noqa: E402
from oracle import ctn_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import ops  # noqa: E402
from conv_tasnet_amd._lib import lib  # noqa: E402

DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
ID = lambda c: "Ch%d-K%d-Kp%d-M%d%s%s%s" % (c.Ch, c.K, c.Kp, c.M, "-prelu" if c.prelu else "", "-mis" if c.mis else "",  # noqa: E731
                                         "-alias" if c.alias else "")


def _dev(t, mis=False):
    """fp32 on the device; mis: the first element one float off a 16-byte boundary."""
    t = t.float()
    if not mis:
        return t.to(DEV).contiguous()
    buf = torch.empty(t.numel() + 1, dtype=F32, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _alpha(i, pre):
    return torch.tensor([i.alpha], dtype=F32, device=DEV) if pre else None


def _check(e):
    for name, (err, lim) in e.items():
        print("%-12s %.3e  (limit %.0e)" % (name, err, lim))
    for name, (err, lim) in e.items():
        assert err <= lim, (name, err, lim)


@pytest.mark.parametrize("case", C.cases(), ids=ID)
def test_cumln_fwd_bwd_against_fp64(case):
    i = C.make_inputs(case.Ch, case.K, case.Kp, case.M, case.seed)
    K, Kp, M, Ch = case.K, case.Kp, case.M, case.Ch
    al = _alpha(i, case.prelu)
    gamma, beta = _dev(i.gamma), _dev(i.beta)
    Y = _dev(i.Y, case.mis)
    out, mean, rstd = ops.cumln_fwd(Y, gamma, beta, al, K)
    ref = C.run_fwd(i, case.prelu)
    _check(C.errors({"out": out, "mean": mean, "rstd": rstd}, ref, K))
    assert float(out[..., K:].abs().max() if Kp > K else 0.0) == 0.0
    assert float(mean[:, K:].abs().max() if Kp > K else 0.0) == 0.0
    assert Kp == K or float((rstd[:, K:].double().cpu() - N.RSTD_PAD).abs().max()) <= 1e-6 * N.RSTD_PAD
    # backward on the fp64 statistics rounded to fp32 (what the oracle's reference is handed too)
    mean_i, rstd_i = _dev(i.stats[case.prelu][0]), _dev(i.stats[case.prelu][1])
    dOut = _dev(i.dOut, case.mis)
    dY = dOut if case.alias else torch.empty_like(dOut)
    pc = torch.empty((lib.ctn_cln_bwd_pc_floats(M, Ch, Kp),), dtype=F32, device=DEV)
    dap = torch.empty((lib.ctn_cln_bwd_blocks(M, Kp),), dtype=F32, device=DEV) if case.prelu else None
    work = torch.empty((lib.ctn_cumln_work_bytes(M, Kp),), dtype=torch.uint8, device=DEV)
    p = ops._p
    lib.call("ctn_cumln_bwd", p(dOut), p(Y), p(dY), p(mean_i), p(rstd_i), M, Ch, K, Kp, p(gamma), p(al), p(dap), p(pc), p(work),
             ops._stream())
    dg, db = torch.empty(Ch, dtype=F32, device=DEV), torch.empty(Ch, dtype=F32, device=DEV)
    da = torch.empty(1, dtype=F32, device=DEV) if case.prelu else None
    lib.call("ctn_cln_bwd_finalize", p(pc), p(dap), M, Ch, Kp, p(dg), p(db), p(da), ops._stream())
    got = {"dY": dY, "dgamma": dg, "dbeta": db}
    if case.prelu:
        got["dalpha"] = da
    _check(C.errors(got, C.run_bwd(i, case.prelu), K))
    assert bool(torch.isfinite(dY).all()) and bool(torch.isfinite(out).all())
    assert float(dY[..., K:].abs().max() if Kp > K else 0.0) == 0.0          # the 1e30 of dOut's pad frames reached nothing
    if not case.alias and not case.mis:                                       # the wrapper runs the same calls
        dY2, dg2, db2, da2 = ops.cumln_bwd(dOut, Y, mean_i, rstd_i, gamma, al, K)
        assert torch.equal(dY2, dY) and torch.equal(dg2, dg) and torch.equal(db2, db) and (da is None or torch.equal(da2, da))


def _fwd_bwd_errors(i, K, pre):
    al, gamma, beta, Y = _alpha(i, pre), _dev(i.gamma), _dev(i.beta), _dev(i.Y)
    out, mean, rstd = ops.cumln_fwd(Y, gamma, beta, al, K)
    e = C.errors({"out": out, "mean": mean, "rstd": rstd}, C.run_fwd(i, pre), K)
    dY, dg, db, da = ops.cumln_bwd(_dev(i.dOut), Y, _dev(i.stats[pre][0]), _dev(i.stats[pre][1]), gamma, al, K)
    got = {"dY": dY, "dgamma": dg, "dbeta": db}
    if pre:
        got["dalpha"] = da
    e.update(C.errors(got, C.run_bwd(i, pre), K))
    assert bool(torch.isfinite(dY).all()) and (i.Kp == K or float(dY[..., K:].abs().max()) == 0.0)
    return e, (Y, gamma, beta, al, out, mean, rstd)


def test_more_frames_than_one_round_of_the_scans():
    """K = 4200: the forward scan stages 3584 frames a round and the backward scan 4096, so both carry their running sums into a
    second round; and a stream cut at the round's edge gives the same bits."""
    Ch, K, Kp, M = 8, 4200, 4224, 2
    i = C.make_inputs(Ch, K, Kp, M, 0)
    e, (Y, gamma, beta, al, out, mean, rstd) = _fwd_bwd_errors(i, K, True)
    _check(e)
    state = ops.cumln_state(M, DEV)
    o, mu, rs = [], [], []
    for c, n in _chunks(Y, (3583, 1, 616)):
        oc, mc, rc = ops.cumln_fwd(c, gamma, beta, al, n, state)
        o.append(oc[..., :n]); mu.append(mc[:, :n]); rs.append(rc[:, :n])
    assert torch.equal(torch.cat(mu, -1), mean[:, :K]) and torch.equal(torch.cat(rs, -1), rstd[:, :K])
    assert torch.equal(torch.cat(o, -1), out[..., :K])


def test_backward_with_32_frame_workgroups():
    """ctn_tune("cln_fr", 32) changes the partial buffers' rows (ctn_cln_bwd_blocks): the backward then runs its 512-thread form."""
    i = C.make_inputs(65, 130, 192, 2, 0)
    lib.call("ctn_tune", b"cln_fr", 32)
    try:
        e, _ = _fwd_bwd_errors(i, 130, True)
    finally:
        lib.call("ctn_tune", b"cln_fr", 16)
    _check(e)


def _split(s, nparts, gen):
    """[M,Kp] fp64 -> [M,nparts,Kp] partials that add up to s (to fp64 rounding)."""
    if nparts == 1:
        return s[:, None].clone()
    w = torch.rand(s.shape[0], nparts - 1, s.shape[1], generator=gen, dtype=F64) - 0.3
    parts = w * s[:, None]
    return torch.cat([parts, (s - parts.sum(1))[:, None]], 1)


@pytest.mark.parametrize("nparts", [1, 3])
@pytest.mark.parametrize("Ch,K,Kp,M,pre", [(64, 130, 192, 2, True), (3, 65, 128, 2, False), (65, 200, 256, 3, True), (512, 1, 64, 2, False)])
def test_frame_kernels_from_column_partials(Ch, K, Kp, M, pre, nparts):
    i = C.make_inputs(Ch, K, Kp, M, N.CHECKED_SEEDS.get(Ch, 0))
    gen = torch.Generator().manual_seed(77)
    ok = torch.arange(Kp) < K
    a = N._act(i.Y, i.alpha if pre else None)
    junk = torch.full((M, Kp), 1e30, dtype=F64)                   # what a pad frame's partials hold must reach nothing
    s1, s2 = torch.where(ok, a.sum(1), junk), torch.where(ok, (a * a).sum(1), junk)
    colp = torch.stack([_split(s1, nparts, gen), _split(s2, nparts, gen)], -1).to(DEV).contiguous()
    mean, rstd = ops.cumln_stats_frame(colp, Ch, K)
    ref = C.run_fwd(i, pre)
    _check(C.errors({"mean": mean, "rstd": rstd}, ref, K))
    assert Kp == K or (float(mean[:, K:].abs().max()) == 0.0 and float((rstd[:, K:].double().cpu() - N.RSTD_PAD).abs().max()) <= 1e-6 * N.RSTD_PAD)
    mean_i, rstd_i = i.stats[pre]
    fs = C.frame_sums(i.dOut, i.Y, mean_i, rstd_i, K, i.gamma, i.alpha if pre else None)
    p1, p2 = torch.where(ok, fs["p1"], junk), torch.where(ok, fs["p2"], junk)
    colp = torch.stack([_split(p1, nparts, gen), _split(p2, nparts, gen)], -1).to(DEV).contiguous()
    fc = ops.cumln_bwd_frame(colp, _dev(mean_i), _dev(rstd_i), Ch, K)
    want = C.cumln_fc(fs["p1"], fs["p2"], mean_i, rstd_i, K, Ch)
    _check(C.fc_errors(fc[..., :K], want[..., :K]))
    assert bool(torch.isfinite(fc).all())
    assert Kp == K or float(fc[:, 1:, K:].abs().max()) == 0.0


def _chunks(Y, cuts):
    pos = 0
    for n in cuts:
        Kp = ops.padded_frames(n)
        c = torch.zeros(Y.shape[:-1] + (Kp,), dtype=Y.dtype, device=Y.device)
        c[..., :n] = Y[..., pos:pos + n]
        yield c, n
        pos += n


def test_carry_gives_the_bits_of_one_call():
    Ch, K, Kp, M = 64, 200, 256, 2
    i = C.make_inputs(Ch, K, Kp, M, 0)
    Y, gamma, beta, al = _dev(i.Y), _dev(i.gamma), _dev(i.beta), _alpha(i, True)
    out, mean, rstd = ops.cumln_fwd(Y, gamma, beta, al, K)
    a = N._act(i.Y, i.alpha)
    colp = torch.stack([a.sum(1), (a * a).sum(1)], -1)[:, None].to(DEV).contiguous()        # [M,1,Kp,2]
    mean_f, rstd_f = ops.cumln_stats_frame(colp, Ch, K)
    state, fstate = ops.cumln_state(M, DEV), ops.cumln_state(M, DEV)
    for rnd, cuts in enumerate(((1, 62, 1, 64, 7, 65), (70, 130), (1, 62, 1, 64, 7, 65))):
        for st in state + fstate:                                   # zeroed and reused
            st.zero_()
        o, mu, rs, mf, rf = [], [], [], [], []
        pos = 0
        for c, n in _chunks(Y, cuts):
            oc, mc, rc = ops.cumln_fwd(c, gamma, beta, al, n, state)
            o.append(oc[..., :n]); mu.append(mc[:, :n]); rs.append(rc[:, :n])
            cp = torch.zeros((M, 1, c.shape[-1], 2), dtype=F64, device=DEV)
            cp[:, :, :n] = colp[:, :, pos:pos + n]
            m2, r2 = ops.cumln_stats_frame(cp, Ch, n, fstate)
            mf.append(m2[:, :n]); rf.append(r2[:, :n])
            pos += n
        assert torch.equal(torch.cat(mu, -1), mean[:, :K]), (rnd, "mean")
        assert torch.equal(torch.cat(rs, -1), rstd[:, :K]), (rnd, "rstd")
        assert torch.equal(torch.cat(o, -1), out[..., :K]), (rnd, "out")
        assert torch.equal(torch.cat(mf, -1), mean_f[:, :K]) and torch.equal(torch.cat(rf, -1), rstd_f[:, :K]), (rnd, "stats_frame")
        assert state[1].tolist() == [K] * M and fstate[1].tolist() == [K] * M
    # the numpy statement of the canonical order, from the same per-frame sums: the kernel's statistics are its values in fp32
    for m in range(M):
        mu, rs = C.stats_of_scan(C.canonical_scan(colp[m, 0, :K].cpu().numpy()), Ch)
        assert C.rel_err(mean_f[m:m + 1, :K], torch.from_numpy(mu)[None], "utt") <= 2e-7
        assert C.rel_err(rstd_f[m:m + 1, :K], torch.from_numpy(rs)[None], "utt") <= 2e-7


def test_causality_later_frames_change_nothing_earlier():
    Ch, K, Kp, M = 65, 130, 192, 2
    i = C.make_inputs(Ch, K, Kp, M, 0)
    gamma, beta, al = _dev(i.gamma), _dev(i.beta), _alpha(i, True)
    Y = _dev(i.Y)
    out, mean, rstd = ops.cumln_fwd(Y, gamma, beta, al, K)
    Y2 = Y.clone()
    Y2[..., 70:K] = Y2[..., 70:K] * -3.0 + 1.0
    out2, mean2, rstd2 = ops.cumln_fwd(Y2, gamma, beta, al, K)
    assert torch.equal(out2[..., :70], out[..., :70]) and torch.equal(mean2[:, :70], mean[:, :70]) and torch.equal(rstd2[:, :70], rstd[:, :70])
    assert not torch.equal(mean2[:, 70:K], mean[:, 70:K])


# ---- the TemporalBlock chain -------------------------------------------------------------------------------------------------------
def _rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


def _block(dil_x, K, seed=0):
    B, H, P, M = 16, 32, 3, 2
    cfg = O.Config(N=16, L=20, B=B, H=H, P=P, X=dil_x + 1, R=1, C=2, norm_type="cumLN", causal=True)
    sd = O.init_params(cfg, seed=seed, dtype=F64)
    keys = O.block_keys(cfg, 0, dil_x)
    sd[keys["a1"]] = torch.tensor([0.2], dtype=F64)
    sd[keys["a2"]] = torch.tensor([0.3], dtype=F64)
    x = torch.randn(M, B, K, generator=torch.Generator().manual_seed(seed + 1), dtype=F64)
    blk = ctn.conv_tasnet.TemporalBlock(B, H, P, 1, 0, 2 ** dil_x, "cumLN", True).to(DEV)
    ds = blk.net[3]
    params = {"w1": blk.net[0].weight, "a1": blk.net[1].weight, "g1": blk.net[2].gamma, "b1": blk.net[2].beta, "dw": ds.net[0].weight,
              "a2": ds.prelu().weight, "g2": ds.norm().gamma, "b2": ds.norm().beta, "w2": ds.pointwise().weight}
    with torch.no_grad():
        for k, p in params.items():
            p.copy_(sd[keys[k]].float())
    return cfg, sd, keys, x, blk, params


@pytest.mark.usefixtures("gemm_arith")
@pytest.mark.parametrize("dil_x,K", [(0, 130), (2, 200), (3, 799)])
def test_temporal_block_fwd_bwd(dil_x, K):
    """The limits of test_gpu_parity.py::test_temporal_block_fwd_bwd: 1e-5 forward, 5e-5 input gradient, 1e-4 parameter gradients."""
    cfg, sd, keys, x, blk, params = _block(dil_x, K)
    leaves = {k: sd[v].clone().requires_grad_(True) for k, v in keys.items()}
    xr = x.clone().requires_grad_(True)
    full = dict(sd)
    full.update({v: leaves[k] for k, v in keys.items()})
    ref = C.temporal_block(O, cfg, xr, full, dil_x)
    dout = torch.randn(ref.shape, generator=torch.Generator().manual_seed(9), dtype=F64)
    ref.backward(dout)

    def run():
        for p in blk.parameters():
            p.grad = None
        xg = x.float().to(DEV).requires_grad_(True)
        out = blk(xg)
        out.backward(dout.float().to(DEV))
        return [out.detach().clone(), xg.grad.clone()] + [params[k].grad.clone() for k in sorted(params)]

    first, second = run(), run()
    e = {"out": (_rel(first[0], ref), 1e-5), "dx": (_rel(first[1], xr.grad), 5e-5)}
    e.update({"d" + k: (_rel(g, leaves[k].grad), 1e-4) for k, g in zip(sorted(params), first[2:])})
    _check(e)
    assert all(torch.equal(a, b) for a, b in zip(first, second))             # bitwise reproducible run to run
    # a flat optimiser attached: the gradients land in its flat buffer, bit for bit the plain-autograd ones
    from conv_tasnet_amd.optim import FlatAdam
    opt = FlatAdam(blk.parameters(), lr=1e-3)
    opt.zero_grad()
    xg = x.float().to(DEV).requires_grad_(True)
    blk(xg).backward(dout.float().to(DEV))
    ops.join_side_stream()
    torch.cuda.synchronize()
    assert torch.equal(xg.grad, first[1])
    for k, g in zip(sorted(params), first[2:]):
        assert params[k].grad.data_ptr() >= opt.flat_grads.data_ptr() and torch.equal(params[k].grad, g), k


# ---- the model level ---------------------------------------------------------------------------------------------------------------
TINY = (32, 20, 16, 32, 3, 4, 2, 2)


def _model(seed):
    torch.manual_seed(seed)
    return ctn.ConvTasNet(*TINY, norm_type="cumLN", causal=True).to(DEV)


@pytest.mark.usefixtures("gemm_arith")
def test_streaming_equals_full_forward():
    """The plan and the bound (2e-6 of the largest magnitude) of test_gpu_train.py::test_streaming_causal_inference_equals_full_forward."""
    from conv_tasnet_amd.streaming import StreamingSeparator
    m = _model(2).eval()
    S, T = 10, 10 * 537
    mix, _, _ = O.synth_batch(3, 2, T)
    with torch.no_grad():
        full = m(mix.to(DEV))
    s = StreamingSeparator(m, batch=2)
    for rnd in range(2):                                            # the second round after reset(): the carry records start again
        outs, pos = [], 0
        for n in (40, 7, 133, 2, 64, 291):
            outs.append(s.push(mix[:, pos:pos + n * S]))
            pos += n * S
        assert pos == T
        outs.append(s.flush())
        got = torch.cat(outs, dim=2)
        assert got.shape == full.shape
        err = float((got - full).abs().max()) / float(full.abs().max())
        print("round %d: max |stream - full| / max |full| = %.3e (limit 2e-6)" % (rnd, err))
        assert err <= 2e-6
        s.reset()


def test_streaming_graph_replay_equals_eager_chunks():
    """The plan of test_gpu_train.py::test_streaming_graph_replay_equals_eager_chunks: the carry records live on the device and the scan
    kernel advances them, so a replayed chunk step is bitwise the eager one."""
    from conv_tasnet_amd.streaming import StreamingSeparator
    m = _model(3).eval()
    S = 10
    plan = [40, 40, 40, 40, 7, 40, 40, 7, 7, 7, 40]
    mix, _, _ = O.synth_batch(6, 2, S * sum(plan))
    eager, graphed = StreamingSeparator(m, batch=2), StreamingSeparator(m, batch=2, graph=True)
    for rnd in range(2):
        pos = 0
        for n in plan:
            a, b = eager.push(mix[:, pos:pos + n * S]), graphed.push(mix[:, pos:pos + n * S])
            assert torch.equal(a, b), (rnd, pos)
            pos += n * S
        assert torch.equal(eager.flush(), graphed.flush())
        assert sorted(graphed._graphs) == [7 * S, 40 * S]
        eager.reset()
        graphed.reset()


def test_fused_streaming_classes_refuse_cumln():
    from conv_tasnet_amd.streaming import FusedStreamingSeparator, FusedStreamPool, ResamplingStreamPool
    m = _model(4).eval()
    for make in (lambda: FusedStreamingSeparator(m, batch=2), lambda: FusedStreamPool(m, slots=2), lambda: ResamplingStreamPool(m, slots=2)):
        with pytest.raises(ValueError, match="cumLN"):
            make()


def test_one_solver_epoch_lowers_the_loss(tmp_path):
    from conv_tasnet_amd.optim import FlatAdam
    from conv_tasnet_amd.solver import Solver
    m = _model(5)
    batches = [O.synth_batch(700 + 2 * i, 2, 4000) for i in range(3)]

    def loss():
        with torch.no_grad():
            return sum(float(ctn.cal_loss(src.to(DEV), m(mix.to(DEV)), lens.to(DEV))[0]) for mix, lens, src in batches) / 3

    before = loss()
    opt = FlatAdam(m.parameters(), lr=1e-3)
    s = Solver({"tr_loader": batches, "cv_loader": batches[:1]}, m, opt, (1, 1, 1, 0, 5, str(tmp_path), 0, "", "final.pth.tar", 1000, 0, 0, "x"))
    s.train()
    after = loss()
    print("loss over the three minibatches: %.4f -> %.4f" % (before, after))
    assert len(s.iter_losses) == 3 + 1 and all(torch.isfinite(torch.tensor(s.iter_losses)))      # three training steps, one validation
    assert after < before
    assert ctn.ConvTasNet.load_model(str(tmp_path / "final.pth.tar")).norm_type == "cumLN"
