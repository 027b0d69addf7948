"""tests/loss_oracle.py (the numpy moment-form model of csrc/ctn_loss.hip) against the fp64 oracle with autograd.  CPU only.

The model is the independent yardstick that tests/test_gpu_loss.py sizes the kernel's gradient limit with, so it is pinned
here first: over the whole case table, and at the SNR levels where its fp32 coefficients A and B nearly cancel.  The limits
below are the figures of the model's arithmetic (fp64 moments of fp32 inputs, fp32 coefficients, fp32 backward expression)
against fp64 autograd, times 4:

    max_snr   2e-5 dB from 0 to 100 dB, 6e-4 dB at 115 dB
    gradient  1e-6 at 20 dB, 8e-6 at 40 dB, 9e-5 at 60 dB, 1.1e-3 at 80 dB, 1.6e-2 at 100 dB   (max |d| / max |ref|)
    DC offset of 1000 on both signals: 1.4e-4 in the gradient, 5e-7 dB in the forward value
"""
import numpy as np
import pytest
import torch

import loss_oracle as LO
from oracle import ctn_oracle as O

MARGIN = 4.0


def _model(name, g_loss=None, g_max=None):
    src, est, lengths = LO.case_inputs(name)
    return LO.sisnr_pit_model(src.numpy(), est.numpy(), lengths.tolist(), g_loss=g_loss, g_max=g_max)


@pytest.mark.parametrize("name", LO.CASES)
def test_model_matches_fp64_oracle_over_the_case_table(name):
    LO.check_inputs(name)
    ref = LO.reference(name)
    src, est, lengths = LO.case_inputs(name)
    Bn, C, T = src.shape
    wgt = ref["wgt"].float().numpy()
    for g_loss, g_max, gref in ((LO.G_LOSS, None, ref["g_loss"]), (None, wgt, ref["g_max"]),
                                (LO.G_LOSS, wgt, ref["g_loss"] + ref["g_max"])):
        m = LO.sisnr_pit_model(src.numpy(), est.numpy(), lengths.tolist(), g_loss=g_loss, g_max=g_max)
        assert np.abs(m["snr"].astype(np.float64) - ref["snr"].numpy()).max() < 1e-4
        assert np.abs(m["max_snr"].astype(np.float64) - ref["max_snr"].numpy()).max() < 1e-4
        assert np.array_equal(m["idx"], ref["idx"].numpy())
        assert abs(float(m["loss"]) - float(ref["loss"])) < 1e-4
        if LO.is_tie(name):
            assert not m["idx"].any()
        d = torch.from_numpy(m["d_est"])
        t = torch.arange(T).view(1, 1, T)
        assert float(d[(t >= ref["lengths"].view(-1, 1, 1)).expand_as(d)].abs().sum()) == 0.0
        errs = LO.rel_err_per_utt(d, gref, ref["lengths"])
        print(name, "g_loss" if g_max is None else ("g_max" if g_loss is None else "both"), "e_model max %.2e" % max(errs))
        # the table's SNR is <= 60 dB: the 60 dB figure bounds every row (the sweep below pins each level on its own)
        assert max(errs) < MARGIN * 9e-5, errs


SWEEP = {0: (2e-5, 1e-6), 20: (2e-5, 1e-6), 40: (2e-5, 8e-6), 60: (2e-5, 9e-5), 80: (2e-5, 1.1e-3), 100: (2e-5, 1.6e-2),
         115: (6e-4, None)}


@pytest.mark.parametrize("db", sorted(SWEEP))
def test_model_error_by_snr_level(db):
    """A and B nearly cancel when est ~ src: the model's (and the kernel's) fp32 coefficients lose digits as the SNR grows."""
    fwd_lim, grad_lim = SWEEP[db]
    src, est, lengths = LO.make_inputs(3, 2, 4000, (4000, 3877, 2000), seed=500 + db, snr=float(db))
    e = est.double().requires_grad_(True)
    loss, max_snr, _, _ = O.cal_loss(src.double(), e, lengths)
    loss.backward()
    m = LO.sisnr_pit_model(src.numpy(), est.numpy(), lengths.tolist(), g_loss=1.0)
    dfwd = float(np.abs(m["max_snr"].astype(np.float64) - max_snr.detach().view(-1).numpy()).max())
    errs = LO.rel_err_per_utt(torch.from_numpy(m["d_est"]), e.grad, lengths)
    print("snr %d dB: |d max_snr| %.2e dB, gradient rel err %.2e" % (db, dfwd, max(errs)))
    assert dfwd < MARGIN * fwd_lim
    if grad_lim is not None:
        assert max(errs) < MARGIN * grad_lim


def test_model_dc_offset_1000():
    src, est, lengths = LO.make_inputs(2, 2, 4000, (4000, 3877), seed=600, dc=1000.0)
    e = est.double().requires_grad_(True)
    loss, max_snr, _, _ = O.cal_loss(src.double(), e, lengths)
    loss.backward()
    m = LO.sisnr_pit_model(src.numpy(), est.numpy(), lengths.tolist(), g_loss=1.0)
    dfwd = float(np.abs(m["max_snr"].astype(np.float64) - max_snr.detach().view(-1).numpy()).max())
    errs = LO.rel_err_per_utt(torch.from_numpy(m["d_est"]), e.grad, lengths)
    print("dc 1000: |d max_snr| %.2e dB, gradient rel err %.2e" % (dfwd, max(errs)))
    assert dfwd < MARGIN * 5e-7
    assert max(errs) < MARGIN * 1.4e-4


def test_model_ignores_source_beyond_length():
    """The model's (and the kernel's) contract: source samples at t >= len are never read.  The fp64 oracle, like the
    reference, divides the source's full-length sum by len, so it agrees only for zero-padded sources."""
    src, est, lengths = LO.make_inputs(3, 2, 2049, (2049, 1500, 64), seed=601)
    t = torch.arange(2049).view(1, 1, -1)
    junk = torch.where(t >= lengths.view(-1, 1, 1), torch.randn(src.shape, generator=torch.Generator().manual_seed(3)) * 5 + 2, src)
    assert not torch.equal(junk, src)
    wgt = LO.g_max_weight(3).numpy()
    a = LO.sisnr_pit_model(src.numpy(), est.numpy(), lengths.tolist(), g_loss=LO.G_LOSS, g_max=wgt)
    b = LO.sisnr_pit_model(junk.numpy(), est.numpy(), lengths.tolist(), g_loss=LO.G_LOSS, g_max=wgt)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    ra, _ = O.pairwise_si_snr(src.double(), est.double(), lengths)
    rb, _ = O.pairwise_si_snr(junk.double(), est.double(), lengths)
    assert float((ra - rb)[1:].abs().max()) > 0.1      # whole dB apart on the utterances that have a tail
