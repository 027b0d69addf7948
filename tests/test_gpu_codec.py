"""The mask and overlap-add kernels of csrc/ctn_codec.hip through the C ABI against plain torch in fp64 (softmax(dim=1), relu,
O.overlap_and_add, autograd for the adjoints), with hand-made Kp and Lp so that the padding cases do not depend on
ops.padded_frames.

Limits (of the largest reference element).  mask forward 4e-7, backward 2e-6: a correctly rounded product is 6e-8, softmax
adds expf and a division within a couple of ulp each, the backward a C-term dot product.  ola forward 2e-7: each output
sample is at most two fp32 adds.  unfold is a pure gather: bitwise.

Measured on the MI355X: nothing yet; no MI355X run of this module has been made.  The tests print their figures
(`MASK ...`, `OLA ...` lines, with -s); torch's fp32 softmax on the CPU gives 1.5e-7 forward and 4.6e-7 backward on
the same inputs.
"""
import pytest
import torch

from oracle import ctn_oracle as O

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import ops  # noqa: E402

DEV = "cuda:0"
FWD_TOL, BWD_TOL = 4e-7, 2e-6
NAN = float("nan")


def g(seed):
    return torch.Generator().manual_seed(seed)


def rel(got, ref):
    """max |got - ref| / max |ref| (the absolute error where the reference is all zero: the softmax gradient at C = 1)."""
    ref = ref.detach().double().cpu()
    d, m = float((got.detach().double().cpu() - ref).abs().max()), float(ref.abs().max())
    return d / m if m > 0 else d


# ---------------------------------------------------------------------------------------------------------------- mask
def mask_fwd(score, w, mode):
    M, C, N, Kp = score.shape
    sw = torch.full_like(score, NAN)
    ctn.lib.call("ctn_mask_apply", ops._p(score), ops._p(w), ops._p(sw), M, C, N, Kp, mode, ops._stream())
    return sw


def mask_bwd(dsw, score, w, mode, alias):
    """-> (dscore, dw); alias: dscore is written over dsw, as ops.Backend.backward does."""
    M, C, N, Kp = score.shape
    dsw = dsw.clone()
    dscore = dsw if alias else torch.full_like(score, NAN)
    dw = torch.full_like(w, NAN)
    ctn.lib.call("ctn_mask_apply_bwd", ops._p(dsw), ops._p(score), ops._p(w), ops._p(dscore), ops._p(dw), M, C, N, Kp, mode,
                 ops._stream())
    return dscore, dw


def mask_ref(score, w, dsw, mode):
    """fp64 torch with autograd -> (sw, mask, dscore, dw)."""
    s = score.double().requires_grad_(True)
    ww = w.double().requires_grad_(True)
    mask = torch.relu(s) if mode == 0 else (torch.softmax(s, dim=1) if mode == 1 else s)
    sw = ww.unsqueeze(1) * mask
    sw.backward(dsw.double())
    return sw.detach(), mask.detach(), s.grad, ww.grad


def check_mask(score, w, dsw, mode, tag):
    sw_r, mask_r, ds_r, dw_r = mask_ref(score, w, dsw, mode)
    score_d, w_d, dsw_d = score.to(DEV), w.to(DEV), dsw.to(DEV)
    sw = mask_fwd(score_d, w_d, mode)
    assert bool(torch.isfinite(sw).all())
    ds1, dw1 = mask_bwd(dsw_d, score_d, w_d, mode, alias=False)
    ds2, dw2 = mask_bwd(dsw_d, score_d, w_d, mode, alias=True)
    assert torch.equal(ds1, ds2) and torch.equal(dw1, dw2)            # in place over dsw == into a separate buffer, bitwise
    assert bool(torch.isfinite(ds1).all()) and bool(torch.isfinite(dw1).all())
    assert torch.equal(score_d.cpu(), score) and torch.equal(w_d.cpu(), w) and torch.equal(dsw_d.cpu(), dsw)
    e = (rel(sw, sw_r), rel(ds1, ds_r), rel(dw1, dw_r), rel(dw1, (dsw.double() * mask_r).sum(1)))
    print("MASK %s mode %d %s: fwd %.2e dscore %.2e dw %.2e" % (tag, mode, tuple(score.shape), e[0], e[1], e[2]))
    assert e[0] < FWD_TOL and e[1] < BWD_TOL and e[2] < BWD_TOL and e[3] < BWD_TOL, e
    return sw, ds1, dw1


# every shape in the three modes; C = 5 and C = 8 (the whole MAXC = 8 register table) for the softmax
MASK_CASES = [(M, C, N, Kp, mode) for (M, C, N, Kp) in ((1, 1, 4, 4), (2, 2, 8, 12), (3, 3, 20, 260)) for mode in (0, 1, 2)] + \
             [(2, 5, 8, 12, 1), (2, 8, 8, 12, 1)]


@pytest.mark.parametrize("M,C,N,Kp,mode", MASK_CASES)
def test_mask_apply_fwd_bwd(M, C, N, Kp, mode):
    score = torch.randn(M, C, N, Kp, generator=g(1)) * 2.0
    w = torch.rand(M, N, Kp, generator=g(2)) + 0.1
    dsw = torch.randn(M, C, N, Kp, generator=g(3))
    check_mask(score, w, dsw, mode, "plain")


def test_mask_softmax_refuses_more_than_eight_speakers():
    """C = 9 in softmax mode: the argument error, and nothing is launched (the outputs keep their fill)."""
    M, C, N, Kp = 1, 9, 4, 4
    score, w = torch.randn(M, C, N, Kp, generator=g(1)).to(DEV), torch.ones(M, N, Kp, device=DEV)
    sw, dw = torch.full_like(score, 7.0), torch.full_like(w, 7.0)
    dsw = torch.full_like(score, 3.0)
    dscore = torch.full_like(score, 7.0)
    with pytest.raises(ctn.CtnError, match="at most 8"):
        ctn.lib.call("ctn_mask_apply", ops._p(score), ops._p(w), ops._p(sw), M, C, N, Kp, 1, ops._stream())
    with pytest.raises(ctn.CtnError, match="at most 8"):
        ctn.lib.call("ctn_mask_apply_bwd", ops._p(dsw), ops._p(score), ops._p(w), ops._p(dscore), ops._p(dw), M, C, N, Kp, 1,
                     ops._stream())
    torch.cuda.synchronize()
    assert bool((sw == 7.0).all()) and bool((dw == 7.0).all()) and bool((dscore == 7.0).all()) and bool((dsw == 3.0).all())
    ctn.lib.call("ctn_mask_apply", ops._p(score), ops._p(w), ops._p(sw), M, C, N, Kp, 0, ops._stream())   # relu takes any C
    assert torch.equal(sw, torch.relu(score))


@pytest.mark.parametrize("C", [3, 8])
def test_mask_softmax_large_scores(C):
    """Scores up to +-80 (expf underflows to 0 in most lanes) and one column whose C scores are all equal."""
    M, N, Kp = 2, 8, 12
    score = (torch.rand(M, C, N, Kp, generator=g(4)) * 2 - 1) * 80.0
    score[:, :, 3, 5] = 80.0
    score[:, :, 4, 6] = -80.0
    w = torch.rand(M, N, Kp, generator=g(5)) + 0.1
    dsw = torch.randn(M, C, N, Kp, generator=g(6))
    sw, _, _ = check_mask(score, w, dsw, 1, "large")
    assert torch.equal(sw[:, :, 3, 5].cpu(), (w[:, 3, 5] * (torch.ones(()) / C)).view(M, 1).expand(M, C))


def test_mask_relu_at_zero():
    """Scores of exactly 0.0 and -0.0: the forward value and dscore are 0 there, as for torch's ReLU."""
    M, C, N, Kp = 2, 3, 8, 12
    score = torch.randn(M, C, N, Kp, generator=g(7))
    pz = torch.rand(M, C, N, Kp, generator=g(8))
    score[pz < 0.2] = 0.0
    score[pz > 0.8] = -0.0
    zero = score == 0
    assert int(zero.sum()) > 100 and bool(torch.signbit(score[zero]).any()) and not bool(torch.signbit(score[zero]).all())
    w = torch.rand(M, N, Kp, generator=g(9)) + 0.1
    dsw = torch.randn(M, C, N, Kp, generator=g(10))
    sw, ds, _ = check_mask(score, w, dsw, 0, "zeros")
    assert float(sw.cpu()[zero].abs().max()) == 0.0 and float(ds.cpu()[zero].abs().max()) == 0.0
    pos = score > 0
    assert torch.equal(ds.cpu()[pos], (dsw * w.unsqueeze(1))[pos])


@pytest.mark.parametrize("mode", [0, 1])
def test_mask_grid_stride_wrap(mode):
    """More float4 groups (1 057 284) than the 4096 x 256 threads of the capped grid; checked in full on the device
    against the same expression in torch fp32 at 1e-6 of the maximum."""
    M, C, N, Kp = 1, 2, 516, 8196
    assert M * N * Kp // 4 > 4096 * 256
    i = torch.arange(M * C * N * Kp, device=DEV, dtype=torch.int64)
    score = (((i * 7919) % 1013).float() / 1013.0 * 6.0 - 3.0).view(M, C, N, Kp)
    dsw = (((i * 104729) % 997).float() / 997.0 - 0.5).view(M, C, N, Kp)
    w = (((i[: M * N * Kp] * 611953) % 1009).float() / 1009.0 + 0.25).view(M, N, Kp)
    mask = torch.relu(score) if mode == 0 else torch.softmax(score, dim=1)
    sw = mask_fwd(score, w, mode)
    ref = w.unsqueeze(1) * mask
    assert float((sw - ref).abs().max() / ref.abs().max()) < 1e-6
    ds, dw = mask_bwd(dsw, score, w, mode, alias=True)
    gm = dsw * w.unsqueeze(1)
    ds_ref = gm * (score > 0).float() if mode == 0 else mask * (gm - (gm * mask).sum(1, keepdim=True))
    dw_ref = (dsw * mask).sum(1)
    assert float((ds - ds_ref).abs().max() / ds_ref.abs().max()) < 1e-6
    assert float((dw - dw_ref).abs().max() / dw_ref.abs().max()) < 1e-6


# ------------------------------------------------------------------------------------------- ola / unfold (50 % overlap)
def make_frames(Bn, L, Lp, K, Kp, seed):
    """[Bn, Lp, Kp] with NaN in the padding rows and columns, and the [Bn, K, L] fp64 view of its payload."""
    fr = torch.full((Bn, Lp, Kp), NAN)
    fr[:, :L, :K] = torch.randn(Bn, L, K, generator=g(seed))
    return fr, fr[:, :L, :K].double().transpose(1, 2).contiguous()


def run_ola(fr_d, Bn, T, L, Lp, K, Kp):
    est = torch.full((Bn, T), NAN, device=DEV)
    ctn.lib.call("ctn_ola", ops._p(fr_d), ops._p(est), Bn, T, L, Lp, K, Kp, ops._stream())
    return est


def run_unfold(dest_d, Bn, T, L, Lp, K, Kp):
    dfr = torch.full((Bn, Lp, Kp), NAN, device=DEV)
    ctn.lib.call("ctn_unfold", ops._p(dest_d), ops._p(dfr), Bn, T, L, Lp, K, Kp, ops._stream())
    return dfr


def check_ola_unfold(Bn, L, Lp, K, Kp, T, seed):
    S = L // 2
    T0 = (K - 1) * S + L
    fr, payload = make_frames(Bn, L, Lp, K, Kp, seed)
    f64 = payload.clone().requires_grad_(True)
    ref = O.overlap_and_add(f64, S)                                           # [Bn, T0]
    dest = torch.randn(Bn, T, generator=g(seed + 1))
    (ref * dest[:, :T0].double()).sum().backward()
    est = run_ola(fr.to(DEV), Bn, T, L, Lp, K, Kp).cpu()
    e = float((est[:, :T0].double() - ref.detach()).abs().max() / ref.detach().abs().max())
    assert e < 2e-7, (e, Lp, Kp, T)
    assert bool((est[:, T0:] == 0).all())                                     # the tail is exactly zero, NaN nowhere
    dfr = run_unfold(dest.to(DEV), Bn, T, L, Lp, K, Kp).cpu()
    assert torch.equal(dfr[:, :L, :K], f64.grad.transpose(1, 2).float())      # a pure gather: bitwise
    pad = torch.ones(Lp, Kp, dtype=torch.bool)
    pad[:L, :K] = False
    assert bool((dfr[:, pad] == 0).all())
    # <ola(f), g> == <f, unfold(g)> with the two kernels' own outputs, in fp64
    lhs = float((est.double() * dest.double()).sum())
    rhs = float((payload.transpose(1, 2) * dfr[:, :L, :K].double()).sum())
    scale = float((payload.transpose(1, 2).abs() * dfr[:, :L, :K].double().abs()).sum())
    assert abs(lhs - rhs) <= 1e-6 * scale, (lhs, rhs, scale)
    return e


@pytest.mark.parametrize("lpad", [0, 4])
@pytest.mark.parametrize("Bn,L,K", [(1, 4, 1), (3, 16, 7), (2, 20, 130), (2, 40, 33),
                                    (2, 5, 9)])      # odd L (S = 2): three frames cover a sample and the l < L bound decides
def test_ola_and_unfold(Bn, L, K, lpad):
    worst = 0.0
    T0 = (K - 1) * (L // 2) + L
    for Kp in (K, (K + 3 + 3) // 4 * 4):
        for T in (T0, T0 + 1, T0 + L + 3):
            worst = max(worst, check_ola_unfold(Bn, L, L + lpad, K, Kp, T, seed=20 + K))
    print("OLA (%d, %d, %d) Lp=L+%d: fwd %.2e" % (Bn, L, K, lpad, worst))


def test_ola_and_unfold_grid_stride_wrap():
    """Bn * T and Bn * Lp * Kp beyond the 4096 x 256 threads of the capped grid."""
    Bn, L, T = 2, 16, 600003
    K = (T - L) // (L // 2) + 1
    assert Bn * T > 4096 * 256 and (K - 1) * (L // 2) + L < T
    e = check_ola_unfold(Bn, L, L, K, K + 1, T, seed=60)
    print("OLA wrap: fwd %.2e" % e)


def test_ola_refuses_a_short_output():
    fr = torch.zeros(1, 16, 8, device=DEV)
    est = torch.zeros(1, 7 * 8 + 16, device=DEV)
    with pytest.raises(ctn.CtnError):
        ctn.lib.call("ctn_ola", ops._p(fr), ops._p(est), 1, 7 * 8 + 15, 16, 16, 8, 8, ops._stream())
    with pytest.raises(ctn.CtnError):
        ctn.lib.call("ctn_unfold", ops._p(est), ops._p(fr), 1, 7 * 8 + 15, 16, 16, 8, 8, ops._stream())


# ----------------------------------------------------------------------------------- general overlap-add (any frame step)
@pytest.mark.parametrize("Bn,F,L,step", [(2, 1, 20, 10),          # a single frame
                                         (2, 50000, 8, 11),      # step > L (gaps of zeros) with Bn * T beyond the grid cap
                                         (3, 70, 33, 1)])        # step 1: every sample sums up to 33 frames
def test_overlap_add_general_edges(Bn, F, L, step):
    """ctn_overlap_add against O.overlap_and_add in fp64; ctn_overlap_add_bwd, a pure gather, bitwise against autograd.
    Limit: a sample sums q = ceil(L / step) frames in fp32, so q * 2^-24 of the largest sum of magnitudes."""
    T = (F - 1) * step + L
    if F == 50000:
        assert Bn * T > 4096 * 256
    sig = torch.randn(Bn, F, L, generator=g(70))
    s64 = sig.double().requires_grad_(True)
    ref = O.overlap_and_add(s64, step)
    assert ref.shape == (Bn, T)
    dout = torch.randn(Bn, T, generator=g(71))
    (ref * dout.double()).sum().backward()
    sig_d, dout_d = sig.to(DEV), dout.to(DEV)
    out = torch.full((Bn, T), NAN, device=DEV)
    ctn.lib.call("ctn_overlap_add", ops._p(sig_d), ops._p(out), Bn, F, L, step, ops._stream())
    q = -(-L // step)
    lim = q * 2.0 ** -24 * float(O.overlap_and_add(sig.double().abs(), step).max())
    err = float((out.double().cpu() - ref.detach()).abs().max())
    print("OLA general (%d, %d, %d, %d): |d| %.2e, limit %.2e" % (Bn, F, L, step, err, lim))
    assert err <= lim
    if step > L:
        gap = (torch.arange(T) % step) >= L
        assert bool((out.cpu()[:, gap] == 0).all())
    if F == 1:
        assert torch.equal(out.cpu(), sig[:, 0])
    dsig = torch.full((Bn, F, L), NAN, device=DEV)
    ctn.lib.call("ctn_overlap_add_bwd", ops._p(dout_d), ops._p(dsig), Bn, F, L, step, ops._stream())
    assert torch.equal(dsig.cpu(), s64.grad.float())
