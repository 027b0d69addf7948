"""Optimal-assignment PIT: the SI-SNR loss for 2 .. 16 speakers on the HIP kernels of csrc/ctn_assign.hip.

`cal_loss` scores all C! permutations, which caps it at C = 6.  Here the pair matrix goes to an exact linear-assignment solver on
the device (the Hungarian method in its shortest-augmenting-path form, O(C^3), per utterance, no read-back), as in Dovrat, Nachmani
& Wolf, "Many-speakers single channel speech separation with optimal permutation training" (2021) and asteroid's PITLossWrapper
with scipy's linear_sum_assignment.  `linear_assignment` is that solver on its own, `cal_assign_loss` the loss, `reorder_estimate`
puts the estimates into the order of their references, `AssignPitCriterion` is the Solver criterion.  include/ctn_hip.h
("optimal-assignment PIT") fixes the definitions.
"""
import torch

from . import ops
from ._lib import lib

F32 = torch.float32
MIN_SOURCES, MAX_SOURCES = 2, 16


def linear_assignment(score, maximize=True):
    """score [N,C,C] (or [C,C]) fp32 on the GPU, 1 <= C <= 16 -> perm [N,C] (or [C]) int32: perm[n,i] = j pairs row i with column j
    so that sum_i score[n,i,perm[n,i]] is largest (smallest with maximize=False).  Exact; among optimal assignments the one the
    solver's fixed order reaches (rows in index order, first column of least slack), which the tests restate in numpy."""
    single = score.dim() == 2
    if single:
        score = score.unsqueeze(0)
    if score.dim() != 3 or score.size(1) != score.size(2):
        raise ValueError("score must be [N, C, C], got %s" % (tuple(score.shape),))
    N, C = score.size(0), score.size(1)
    if not 1 <= C <= MAX_SOURCES:
        raise ValueError("linear_assignment over 1 .. %d rows, got %d" % (MAX_SOURCES, C))
    if N < 1:
        raise ValueError("empty batch")
    score = ops._c(score)
    ops._chk(score)
    perm = torch.empty((N, C), dtype=torch.int32, device=score.device)
    lib.call("ctn_assign_solve", ops._p(score), N, C, 1 if maximize else 0, ops._p(perm), ops._stream())
    return perm[0] if single else perm


class SiSnrAssign(torch.autograd.Function):
    """(source [B,C,T], estimate [B,C,T], lengths [B]) -> (loss [], max_snr [B,1], pair [B,C,C], perm [B,C] int32).  Differentiable
    in `estimate` through `loss` and `max_snr`; `estimate` is not modified."""

    @staticmethod
    def forward(ctx, source, estimate, lengths):
        if source.dim() != 3 or estimate.dim() != 3 or source.shape != estimate.shape:
            raise ValueError("source and estimate_source must both be [B, C, T], got %s and %s"
                             % (tuple(source.shape), tuple(estimate.shape)))
        Bn, C, T = estimate.shape
        if not MIN_SOURCES <= C <= MAX_SOURCES:
            raise ValueError("optimal-assignment PIT over %d .. %d speakers, got %d" % (MIN_SOURCES, MAX_SOURCES, C))
        if Bn < 1 or T < 1:
            raise ValueError("empty batch or zero-length signals")
        source, lengths = ops._loss_inputs(source, estimate, lengths)
        dev = estimate.device
        loss = torch.empty((), dtype=F32, device=dev)
        max_snr = torch.empty((Bn, 1), dtype=F32, device=dev)
        pair = torch.empty((Bn, C, C), dtype=F32, device=dev)
        perm = torch.empty((Bn, C), dtype=torch.int32, device=dev)
        coef = torch.empty((Bn, C, 4), dtype=F32, device=dev)
        nbytes = lib.ctn_sisnr_assign_workspace(Bn, C, T)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        lib.call("ctn_sisnr_assign_fwd", ops._p(source), ops._p(estimate), ops._p(lengths), Bn, C, T, ops._p(max_snr), ops._p(perm),
                 ops._p(loss), ops._p(pair), ops._p(coef), ops._p(ws), nbytes, ops._stream())
        ctx.mark_non_differentiable(pair, perm)
        ctx.save_for_backward(source, estimate, lengths, perm, coef)
        ctx.set_materialize_grads(False)
        return loss, max_snr, pair, perm

    @staticmethod
    def backward(ctx, g_loss, g_max, _g_pair, _g_perm):
        source, estimate, lengths, perm, coef = ctx.saved_tensors
        Bn, C, T = estimate.shape
        d_est = torch.empty_like(estimate)
        g_loss, g_max = ops._upstream(g_loss, g_max)
        lib.call("ctn_sisnr_assign_bwd", ops._p(source), ops._p(estimate), ops._p(lengths), ops._p(perm), ops._p(coef), ops._p(g_loss),
                 ops._p(g_max), Bn, C, T, ops._p(d_est), ops._stream())
        return None, d_est, None


def cal_assign_loss(source, estimate_source, source_lengths):
    """-> (loss, max_snr [B,1], pair [B,C,C], perm [B,C] int64).

    source [B,C,T]: the references; estimate_source [B,C,T], 2 <= C <= 16, contiguous fp32 on the GPU and NOT modified (cal_loss
    masks it in place; this loss reads t < length only); source_lengths [B].  pair[b,i,j] is the SI-SNR in dB of estimate i against
    reference j, perm[b,i] = j the reference estimate i is matched to (the assignment of largest mean SI-SNR), max_snr that mean,
    loss = -mean(max_snr).  loss and max_snr are differentiable in estimate_source.  No read-back, no synchronisation."""
    loss, max_snr, pair, perm = SiSnrAssign.apply(source, estimate_source, source_lengths)
    return loss, max_snr, pair, perm.long()


def reorder_estimate(estimate, perm):
    """out[b, perm[b,i]] = estimate[b,i]: out[b,j] is the estimate of source[b,j].

    This is the inverse permutation, which pit_criterion.reorder_source does not apply: that function keeps the reference's rule
    out[b,c] = estimate[b, perm[b,c]], which is the same thing only for permutations that are their own inverse --
    every one at C = 2, but not the 3-cycles from C = 3 up.  `perm` [B,C]: what cal_assign_loss or linear_assignment returns."""
    if estimate.dim() != 3 or perm.shape != estimate.shape[:2]:
        raise ValueError("estimate must be [B, C, T] and perm [B, C], got %s and %s" % (tuple(estimate.shape), tuple(perm.shape)))
    index = perm.to(device=estimate.device, dtype=torch.int64).unsqueeze(-1).expand_as(estimate)
    return torch.zeros_like(estimate).scatter_(1, index, estimate)


class AssignPitCriterion:
    """Solver criterion: (sources [B,C,T], estimate [B,C,T], lengths) -> the scalar loss, 2 <= C <= 16."""

    def __call__(self, sources, estimate, lengths):
        return cal_assign_loss(sources, estimate, lengths)[0]
