"""The cumulative LayerNorm's closed forms (tests/cumln_oracle.py) checked on the CPU: against torch autograd, against the per-frame
norm at K = 1, against fp32 arithmetic (the limits of tests/test_gpu_cumln.py are reachable) and against deliberately wrong models
(the limits can tell a defect from rounding); the canonical scan order; and the model-level plumbing of norm_type="cumLN"."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cumln_oracle as C  # noqa: E402
import norm_oracle as N  # noqa: E402

F64 = torch.float64


@pytest.mark.parametrize("Ch,K,pre", [(3, 1, True), (3, 65, False), (64, 63, True), (65, 130, False), (16, 200, True)])
def test_closed_form_backward_is_autograd_of_the_cumsum_restatement(Ch, K, pre):
    i = C.make_inputs(Ch, K, N.padded(K), 2, N.CHECKED_SEEDS.get(Ch, 0))
    y = i.Y[..., :K].clone().requires_grad_(True)
    gamma, beta = i.gamma.clone().requires_grad_(True), i.beta.clone().requires_grad_(True)
    alpha = torch.tensor(i.alpha, dtype=F64, requires_grad=True) if pre else None
    out = C.cumln_autograd(y, gamma, beta, alpha)
    fwd = C.run_fwd(i, pre)
    assert C.rel_err(fwd["out"][..., :K], out, "utt") <= 1e-10
    out.backward(i.dOut[..., :K])
    # the closed form on the un-rounded fp64 statistics
    for form in ("closed", "fc"):
        b = C.cumln_bwd(i.dOut, i.Y, fwd["mean"], fwd["rstd"], K, i.gamma, i.alpha if pre else None, form=form)
        assert C.rel_err(b["dY"][..., :K], y.grad, "utt") <= 1e-10, form
        assert C.rel_err(b["dgamma"], gamma.grad, "all") <= 1e-10 and C.rel_err(b["dbeta"], beta.grad, "all") <= 1e-10
        if pre:
            assert C.sum_err(b["dalpha"], alpha.grad.reshape(1), b["dalpha|abs"]) <= 1e-10
        assert float(b["dY"][..., K:].abs().max()) == 0.0 if i.Kp > K else True


@pytest.mark.parametrize("Ch", [3, 64, 65])
def test_one_frame_is_the_per_frame_norm(Ch):
    i = C.make_inputs(Ch, 1, 64, 2, N.CHECKED_SEEDS.get(Ch, 0))
    for pre in (False, True):
        f, g = C.run_fwd(i, pre), N.run_fwd(N.make_inputs(Ch, 1, 64, 2, N.CHECKED_SEEDS.get(Ch, 0)), pre)
        for n in ("out", "mean", "rstd"):
            assert C.rel_err(f[n][..., :1], g[n][..., :1], "utt") <= 1e-12, n
        b = C.cumln_bwd(i.dOut, i.Y, f["mean"], f["rstd"], 1, i.gamma, i.alpha if pre else None)
        r = N.cln_bwd(i.dOut, i.Y, g["mean"], g["rstd"], 1, i.gamma, i.alpha if pre else None)
        # (at one frame da is the remainder of a cancellation: compared in units of the terms, rstd |t|)
        scale = float((g["rstd"][:, :1].abs().amax() * i.dOut[..., :1].abs().amax() * i.gamma.abs().amax()))
        assert float((b["dY"][..., :1] - r["dY"][..., :1]).abs().max()) <= 1e-12 * scale
        assert C.rel_err(b["dgamma"], r["dgamma"], "all") <= 1e-10


@pytest.mark.parametrize("case", C.cases(), ids=lambda c: "Ch%d-K%d-M%d%s" % (c.Ch, c.K, c.M, "-prelu" if c.prelu else ""))
def test_limits_are_reachable_in_fp32(case):
    """fp32 torch (cumsum, one-pass variance) stays below half of every limit at every case of the GPU table."""
    i = C.make_inputs(case.Ch, case.K, case.Kp, case.M, case.seed)
    e = C.errors(C.run_fwd(i, case.prelu, torch.float32), C.run_fwd(i, case.prelu), case.K)
    e.update(C.errors(C.run_bwd(i, case.prelu, torch.float32), C.run_bwd(i, case.prelu), case.K))
    for name, (err, lim) in e.items():
        assert err <= 0.5 * lim, (name, err, lim)
    f32 = C.run_bwd(i, case.prelu, torch.float32, form="fc")
    for name, (err, lim) in C.errors(f32, C.run_bwd(i, case.prelu), case.K).items():
        assert err <= 0.5 * lim, ("fc", name, err, lim)


def _worst(e):
    return max(err / lim for err, lim in e.values())


@pytest.mark.parametrize("name", C.DEFECTS)
def test_limits_catch_defects(name):
    i = C.make_inputs(64, 130, 192, 2, 0)
    ref_f, ref_b = C.run_fwd(i, True), C.run_bwd(i, True)
    if name == "count_ignored":         # the second of two calls, with the first one's prefix sums but not its frame count
        first = C.cumln_fwd(i.Y[..., :70].contiguous(), 70, i.gamma, i.beta, i.alpha)
        tail = torch.nn.functional.pad(i.Y[..., 70:130], (0, 4))
        ok = C.cumln_fwd(tail, 60, i.gamma, i.beta, i.alpha, carry=first["carry"])
        want = {n: ref_f[n][..., 70:130] for n in ("out", "mean", "rstd")}
        assert _worst(C.errors({n: ok[n][..., :60] for n in want}, want, 60)) <= 1e-6
        with C.defect(name):
            bad = C.cumln_fwd(tail, 60, i.gamma, i.beta, i.alpha, carry=first["carry"])
        assert _worst(C.errors({n: bad[n][..., :60] for n in want}, want, 60)) > 1.0
        return
    with C.defect(name):
        e = C.errors(C.run_fwd(i, True), ref_f, i.K)
        e.update(C.errors(C.run_bwd(i, True), ref_b, i.K))
    assert _worst(e) > 1.0, e


def test_canonical_scan_does_not_depend_on_the_cuts():
    rng = np.random.default_rng(5)
    s = np.stack([rng.standard_normal(200) * 30, rng.random(200) * 900], 1)
    whole = C.canonical_scan(s)
    assert np.array_equal(C.blocked_scan(s), whole)
    for cuts in ((1, 62, 1, 64, 7, 65), (70, 130), (64, 64, 72), (63, 1, 136), (200,)) + tuple(
            tuple(int(v) for v in np.diff(np.concatenate([[0], np.sort(rng.choice(np.arange(1, 200), 5, replace=False)), [200]])))
            for _ in range(4)):
        assert sum(cuts) == 200
        for scan in (C.canonical_scan, C.blocked_scan):
            st, parts, k = C.scan_state(), [], 0
            for n in cuts:
                parts.append(scan(s[k:k + n], st))
                k += n
            assert np.array_equal(np.concatenate(parts), whole), (scan.__name__, cuts)
            assert st["a"] == 200
    # and the scan is the prefix sum, to fp64 rounding
    assert np.allclose(whole, np.cumsum(s, 0), rtol=1e-13, atol=0)
    mu, rs = C.stats_of_scan(whole, 1)
    assert mu.shape == (200,) and np.all(np.isfinite(rs))


def test_model_level_plumbing_of_cumln():
    import conv_tasnet_amd as ctn
    from conv_tasnet_amd.conv_tasnet import BatchNorm1d, ChannelwiseLayerNorm, CumulativeLayerNorm, GlobalLayerNorm, chose_norm
    assert isinstance(chose_norm("cumLN", 8), CumulativeLayerNorm)
    assert isinstance(chose_norm("BN", 8), BatchNorm1d) and isinstance(chose_norm("anything else", 8), BatchNorm1d)
    assert isinstance(chose_norm("cLN", 8), ChannelwiseLayerNorm) and isinstance(chose_norm("gLN", 8), GlobalLayerNorm)
    args = (32, 20, 16, 32, 3, 4, 2, 2)
    torch.manual_seed(0)
    cum = ctn.ConvTasNet(*args, norm_type="cumLN", causal=True)
    cln = ctn.ConvTasNet(*args, norm_type="cLN", causal=True)
    a, b = cum.state_dict(), cln.state_dict()
    assert list(a.keys()) == list(b.keys())
    assert all(a[k].shape == b[k].shape for k in a)
    norms = [m for m in cum.modules() if isinstance(m, CumulativeLayerNorm)]
    assert len(norms) == 2 * 4 * 2
    assert type(cum.separator.network[0]) is ChannelwiseLayerNorm       # the encoder-output norm stays per frame
    assert all(float((m.gamma.detach() - 1).abs().max()) > 0 for m in norms)     # the xavier init reaches gamma / beta (D10)
    pkg = ctn.ConvTasNet.serialize(cum, torch.optim.SGD(cum.parameters(), lr=0.1), 1)
    back = ctn.ConvTasNet.load_model_from_package(pkg)
    assert back.norm_type == "cumLN" and back.causal
    assert all(torch.equal(back.state_dict()[k], a[k]) for k in a)
    with pytest.raises(ValueError):
        ctn.ConvTasNet(*args, norm_type="cumLN", causal=False)


def test_train_cli_flags():
    from conv_tasnet_amd.train import build_parser, main
    with pytest.raises(SystemExit, match="--norm cumLN needs --causal"):
        main(["--norm", "cumLN"])
    a = build_parser().parse_args([])
    assert a.norm is None and a.causal is False
    a = build_parser().parse_args(["--norm", "cumLN", "--causal"])
    assert a.norm == "cumLN" and a.causal is True
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--norm", "nope"])
