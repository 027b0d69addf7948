"""csrc/ctn_loss.hip through the C ABI against the fp64 oracle with autograd, at the shapes where its kernels change path.

Reference: O.cal_loss / O.pairwise_si_snr / O.si_snr_pit on .double() inputs (tests/loss_oracle.py: reference()).  A length
beyond T means T to the kernels, so the reference of the `len_gt_T` row is taken at min(len, T).  T = 1 (`chunk_T1`) leaves
nothing after centring: every snr is 10 log10(EPS), every permutation ties, and it is checked like the exact-tie rows.

Limits.  snr_out, max_snr: 1e-4 dB (fp32 outputs: one ulp at 100 dB is 7.6e-6; the fp32 sum over C <= 6 terms adds a few).
loss: 1e-4.  d_est for t < len, per utterance, max |d| / max |ref|:  max(8 * e_model, 4e-6), where e_model is the same error
of tests/loss_oracle.py (an independent numpy model of the moment form) on the same inputs: the limit comes from the reference
and the model, never from the kernel.  The 8 covers what the model does not reproduce (order of the fp64 partial sums, FMA
contraction in the fp32 backward expression, the device's log / log10); 4e-6 is a floor of a few fp32 ulp.

Measured (the utterance and upstream combination closest to its limit).  e_model is from the CPU; the e_gpu column is
empty because no MI355X run of this module has been made yet: fill it from the `ROW` lines that the test prints (-s).

    row            e_gpu      e_model    limit
    chunk_T1       -          0.00e+00   4.00e-06
    chunk_T255     -          1.27e-06   1.02e-05
    chunk_T2048    -          1.10e-06   8.80e-06
    chunk_T2049    -          1.06e-06   8.49e-06
    chunk_T4097    -          1.35e-06   1.08e-05
    chunk_cap      -          1.07e-06   8.60e-06
    spk_C1         -          7.08e-07   5.66e-06
    spk_C4         -          1.39e-06   1.11e-05
    spk_C5         -          1.10e-06   8.78e-06
    spk_C6         -          1.13e-06   9.04e-06
    batch_stride   -          5.73e-07   4.58e-06
    snr_0          -          2.00e-07   4.00e-06
    snr_20         -          8.53e-07   6.82e-06
    snr_40         -          9.41e-06   7.52e-05
    snr_60         -          1.23e-04   9.83e-04
    dc_100         -          1.25e-05   1.00e-04
    dc_1000        -          7.15e-05   5.72e-04
    tiny_1e-4      -          1.25e-06   9.99e-06
    tiny_1e-6      -          2.37e-07   4.00e-06
    silent_src     -          1.15e-06   9.24e-06
    silent_est     -          1.09e-06   8.75e-06
    tie_C2         -          7.99e-07   6.39e-06
    tie_C3         -          8.22e-07   6.58e-06
    len_gt_T       -          1.34e-06   1.07e-05
"""
import numpy as np
import pytest
import torch

import loss_oracle as LO
from oracle import ctn_oracle as O

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import ops  # noqa: E402

DEV = "cuda:0"
FACTOR, FLOOR = 8.0, 4e-6


def pit_fwd(src, est, lengths, snr_out=True):
    """ctn_sisnr_pit_fwd on device tensors (est is masked in place) -> dict of outputs and the backward tables."""
    Bn, C, T = src.shape
    p32, _ = ops._perms(C, src.device)
    o = dict(max_snr=torch.full((Bn,), float("nan"), device=DEV), idx=torch.full((Bn,), -1, dtype=torch.int64, device=DEV),
             loss=torch.full((1,), float("nan"), device=DEV), coef=torch.empty((Bn, C, 4), device=DEV),
             jsel=torch.empty((Bn, C), dtype=torch.int32, device=DEV),
             snr=torch.full((Bn, C, C), float("nan"), device=DEV) if snr_out else None)
    nbytes = ctn.lib.ctn_sisnr_workspace(Bn, C, T)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
    ctn.lib.call("ctn_sisnr_pit_fwd", ops._p(src), ops._p(est), ops._p(lengths), ops._p(p32), p32.shape[0], Bn, C, T,
                 ops._p(o["max_snr"]), ops._p(o["idx"]), ops._p(o["loss"]), ops._p(o["snr"]), ops._p(o["coef"]), ops._p(o["jsel"]),
                 ops._p(ws), nbytes, ops._stream())
    torch.cuda.synchronize()
    return o


def pit_bwd(src, est, lengths, o, g_loss, g_max):
    d = torch.full_like(src, float("nan"))
    ctn.lib.call("ctn_sisnr_pit_bwd", ops._p(src), ops._p(est), ops._p(lengths), ops._p(o["coef"]), ops._p(o["jsel"]),
                 ops._p(g_loss), ops._p(g_max), src.shape[0], src.shape[1], src.shape[2], ops._p(d), ops._stream())
    torch.cuda.synchronize()
    return d


@pytest.mark.parametrize("name", LO.CASES)
def test_sisnr_pit_fwd_bwd_vs_fp64(name):
    LO.check_inputs(name)                                     # conditions on the inputs, from the reference alone
    ref = LO.reference(name)
    src, est, lengths = LO.case_inputs(name)
    Bn, C, T = src.shape
    src_d, est_d, len_d = src.to(DEV), est.to(DEV), lengths.to(DEV)
    o = pit_fwd(src_d, est_d, len_d)
    d_snr = float((o["snr"].double().cpu() - ref["snr"]).abs().max())
    d_max = float((o["max_snr"].double().cpu() - ref["max_snr"]).abs().max())
    d_loss = abs(float(o["loss"]) - float(ref["loss"]))
    print("%s: |d snr_out| %.2e dB, |d max_snr| %.2e dB, |d loss| %.2e" % (name, d_snr, d_max, d_loss))
    assert bool(torch.isfinite(o["snr"]).all())
    assert d_snr < 1e-4 and d_max < 1e-4 and d_loss < 1e-4
    assert torch.equal(o["idx"].cpu(), ref["idx"])
    if LO.is_tie(name):
        assert not bool(o["idx"].any())
    t = torch.arange(T).view(1, 1, T)
    keep = t < ref["lengths"].view(-1, 1, 1)
    assert torch.equal(est_d.cpu(), est * keep.float())       # masked in place, nothing else touched
    assert torch.equal(src_d.cpu(), src)
    wgt = ref["wgt"].float()
    g_loss_d, wgt_d = torch.tensor([LO.G_LOSS], device=DEV), wgt.to(DEV)
    worst = (0.0, 0.0, FLOOR)
    for tag, gl, gm, gref in (("g_loss", LO.G_LOSS, None, ref["g_loss"]), ("g_max", None, wgt, ref["g_max"]),
                              ("both", LO.G_LOSS, wgt, ref["g_loss"] + ref["g_max"])):
        d = pit_bwd(src_d, est_d, len_d, o, None if gl is None else g_loss_d, None if gm is None else wgt_d).cpu()
        assert bool(torch.isfinite(d).all()), tag
        assert float(d[(~keep).expand_as(d)].abs().sum()) == 0.0, tag      # exactly zero beyond the length
        m = LO.sisnr_pit_model(src.numpy(), est.numpy(), lengths.tolist(), g_loss=gl, g_max=None if gm is None else gm.numpy())
        e_model = LO.rel_err_per_utt(torch.from_numpy(m["d_est"]), gref, ref["lengths"])
        e_gpu = LO.rel_err_per_utt(d, gref, ref["lengths"])
        print("%s %s: e_gpu %.2e, e_model %.2e" % (name, tag, max(e_gpu), max(e_model)))
        for b in range(Bn):
            lim = max(FACTOR * e_model[b], FLOOR)
            if e_gpu[b] / lim > worst[0] / worst[2]:
                worst = (e_gpu[b], e_model[b], lim)
            assert e_gpu[b] <= lim, (tag, b, e_gpu[b], e_model[b])
    print("ROW %s | %.2e | %.2e | %.2e" % (name, worst[0], worst[1], worst[2]))


def test_batch_position_does_not_change_an_utterance():
    """The chunk partition depends on T alone: bitwise the same max_snr and d_est at index 0 of B = 1 and index 2 of B = 3."""
    src, est, lengths = LO.make_inputs(3, 2, 4097, (4097, 3000, 4000), seed=31)
    wgt = torch.tensor([0.5, -1.25, 0.75])
    res = []
    for sl in (slice(0, 3), slice(2, 3)):
        s, e, n, w = src[sl].contiguous().to(DEV), est[sl].contiguous().to(DEV), lengths[sl].to(DEV), wgt[sl].contiguous().to(DEV)
        o = pit_fwd(s, e, n)
        res.append((o["max_snr"][-1].cpu(), o["snr"][-1].cpu(), pit_bwd(s, e, n, o, None, w)[-1].cpu()))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert float(res[0][2].abs().max()) > 0.0


def test_source_beyond_length_is_never_read():
    """Bitwise the same outputs for a source with garbage at t >= len and for the same source zeroed there (the contract
    written in include/ctn_hip.h; the reference divides the full-length sum by len instead)."""
    src, est, lengths = LO.make_inputs(3, 2, 2049, (2049, 1500, 64), seed=601)
    t = torch.arange(2049).view(1, 1, -1)
    junk = torch.where(t >= lengths.view(-1, 1, 1), torch.randn(src.shape, generator=torch.Generator().manual_seed(3)) * 5 + 2, src)
    junk[1, 0, 2000] = float("nan")
    wgt_d, gl_d, len_d = LO.g_max_weight(3).to(DEV), torch.tensor([LO.G_LOSS], device=DEV), lengths.to(DEV)
    outs = []
    for s in (src, junk):
        s_d, e_d = s.to(DEV), est.to(DEV)
        o = pit_fwd(s_d, e_d, len_d)
        outs.append([o[k].cpu() for k in ("snr", "max_snr", "idx", "loss", "coef", "jsel")] + [e_d.cpu(), pit_bwd(s_d, e_d, len_d, o, gl_d, wgt_d).cpu()])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ the autograd wrapper
WB, WC, WT = 3, 3, 2049
WLENS = (2049, 2000, 64)


def test_wrapper_gradient_through_masked_estimate_and_reorder():
    """The g_est path of ops.SiSnrPit: d/d est of loss + (reorder * w1).sum() + (est_masked * w2).sum() against fp64 autograd
    of the same expression on the oracle.  w1, w2 are scaled to the size of the loss gradient so that neither part hides
    the other.  Limit: as above, with the model's d_est plus the fp32 (scatter of w1 + w2) * mask as e_model."""
    src, est, lengths = LO.make_inputs(WB, WC, WT, WLENS, seed=41)
    gen = torch.Generator().manual_seed(42)
    w1, w2 = torch.randn(WB, WC, WT, generator=gen) * 1e-3, torch.randn(WB, WC, WT, generator=gen) * 1e-3
    e64 = est.double().requires_grad_(True)
    loss, _, est_m, reord = O.cal_loss(src.double(), e64, lengths)
    (loss + (reord * w1.double()).sum() + (est_m * w2.double()).sum()).backward()
    _, perms, idx, _ = O.si_snr_pit(src.double(), est.double(), lengths)
    assert bool((idx != 0).all())
    est0 = est.to(DEV).requires_grad_(True)
    e = est0 * 1.0
    l_d, max_d, em_d, re_d = ctn.cal_loss(src.to(DEV), e, lengths.to(DEV))
    assert em_d.data_ptr() == e.data_ptr()
    assert abs(float(l_d) - float(loss)) < 1e-4
    assert torch.equal(re_d.detach().cpu(), O.reorder(em_d.detach().cpu(), perms, idx))
    (l_d + (re_d * w1.to(DEV)).sum() + (em_d * w2.to(DEV)).sum()).backward()
    m = LO.sisnr_pit_model(src.numpy(), est.numpy(), lengths.tolist(), g_loss=1.0)
    sel = perms[idx].unsqueeze(-1).expand(WB, WC, WT)
    keep = (torch.arange(WT).view(1, 1, WT) < lengths.view(-1, 1, 1)).float()
    model = torch.from_numpy(m["d_est"]) + (torch.zeros(WB, WC, WT).scatter_add_(1, sel, w1) + w2) * keep
    e_model = LO.rel_err_per_utt(model, e64.grad, lengths)
    e_gpu = LO.rel_err_per_utt(est0.grad.cpu(), e64.grad, lengths)
    print("g_est path: e_gpu %s, e_model %s" % (e_gpu, e_model))
    assert float((est0.grad.cpu() * (1 - keep)).abs().sum()) == 0.0
    for b in range(WB):
        assert e_gpu[b] <= max(FACTOR * e_model[b], FLOOR), (b, e_gpu[b], e_model[b])
    # the weights alone must matter at this size: without them the error would be of order one
    assert max(LO.rel_err_per_utt(torch.from_numpy(m["d_est"]), e64.grad, lengths)) > 1e-2


def test_wrapper_refuses_estimates_it_cannot_mask_in_place():
    src, est, lengths = LO.make_inputs(WB, WC, WT, WLENS, seed=41)
    src_d, len_d = src.to(DEV), lengths.to(DEV)
    with pytest.raises(ctn.CtnError):
        ctn.cal_loss(src_d, est.to(DEV).half(), len_d)
    nc = est.to(DEV).transpose(1, 2).contiguous().transpose(1, 2)
    assert nc.shape == src_d.shape and not nc.is_contiguous()
    with pytest.raises(ctn.CtnError):
        ctn.cal_loss(src_d, nc, len_d)
    with pytest.raises(ctn.CtnError):
        ops.SiSnrPit.apply(src_d, nc, len_d)


@pytest.mark.parametrize("dtype", [torch.float64, torch.int8])
def test_wrapper_converts_the_source(dtype):
    """A source given as fp64 or int8 (the reference's own example is integer) is converted to fp32: bitwise the same
    results as for the fp32 tensor of the same values, and within 1e-4 dB of the fp64 oracle."""
    gen = torch.Generator().manual_seed(43)
    lengths = torch.tensor(WLENS)
    keep = torch.arange(WT).view(1, 1, WT) < lengths.view(-1, 1, 1)
    src_i = torch.randint(-100, 101, (WB, WC, WT), generator=gen) * keep
    est = torch.roll(src_i.float() + 10.0 * torch.randn(WB, WC, WT, generator=gen), 1, dims=1).contiguous()
    ref_loss, ref_max, _, _ = O.cal_loss(src_i.double(), est.double(), lengths)
    outs = []
    for s in (src_i.float(), src_i.to(dtype)):
        l_d, max_d, em_d, re_d = ctn.cal_loss(s.to(DEV), est.to(DEV), lengths.to(DEV))
        outs.append((l_d.cpu(), max_d.cpu(), em_d.cpu(), re_d.cpu()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert abs(float(outs[1][0]) - float(ref_loss)) < 1e-4
    assert float((outs[1][1].double() - ref_max).abs().max()) < 1e-4
