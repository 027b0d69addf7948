"""Variable-speaker-count training: permutation invariant training with inactive sources (Wisdom et al., "What's all the FUSS
about free universal sound separation data?", ICASSP 2021) on the HIP loss kernels of csrc/ctn_varpit.hip.

A model with C outputs is trained on mixtures of 1 .. C speakers (`DynamicMixLoader(min_speakers=)` yields them: the references
of the speakers left out are all zeros).  Active references get the soft-thresholded SNR, silent ones a loss that pushes the
assigned output towards silence, and the permutation search runs over both kinds together.  At inference the number of speakers
is the number of outputs that are not silent: `count_sources`.  `cal_varpit_loss` is the criterion, `evaluate_variable` scores a
model on a loader of such mixtures.  include/ctn_hip.h ("PIT with inactive sources") fixes the definition.
"""
import numpy as np
import torch

from . import ops
from ._lib import lib
from .mixit import threshold

F32 = torch.float32
MIN_SOURCES, MAX_SOURCES = 2, 6
EPS = 1e-8


class VarPit(torch.autograd.Function):
    """(sources [B,C,T], estimates [B,C,T], lengths [B], tau, tau0) -> (loss [], per_utt [B], pair [B,C,C], perm_idx [B] int64,
    active [B,C] int32).  Differentiable in `estimates` through `loss` and `per_utt`; `estimates` is not modified."""

    @staticmethod
    def forward(ctx, sources, estimates, lengths, tau, tau0):
        if sources.dim() != 3 or estimates.dim() != 3 or sources.shape != estimates.shape:
            raise ValueError("sources and estimates must both be [B, C, T], got %s and %s"
                             % (tuple(sources.shape), tuple(estimates.shape)))
        Bn, C, T = estimates.shape
        if not MIN_SOURCES <= C <= MAX_SOURCES:
            raise ValueError("PIT with inactive sources over %d .. %d outputs, got %d" % (MIN_SOURCES, MAX_SOURCES, C))
        if Bn < 1 or T < 1:
            raise ValueError("empty batch or zero-length signals")
        sources, lengths = ops._loss_inputs(sources, estimates, lengths)
        dev = estimates.device
        perms = ops._perms(C, dev)[0]
        loss = torch.empty((), dtype=F32, device=dev)
        per_utt = torch.empty((Bn,), dtype=F32, device=dev)
        pair = torch.empty((Bn, C, C), dtype=F32, device=dev)
        perm_idx = torch.empty((Bn,), dtype=torch.int64, device=dev)
        active = torch.empty((Bn, C), dtype=torch.int32, device=dev)
        coef = torch.empty((Bn, C, 2), dtype=F32, device=dev)
        nbytes = lib.ctn_varpit_workspace(Bn, C, T)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        lib.call("ctn_varpit_fwd", ops._p(sources), ops._p(estimates), ops._p(lengths), ops._p(perms), perms.size(0), Bn, C, T,
                 float(tau), float(tau0), ops._p(per_utt), ops._p(perm_idx), ops._p(pair), ops._p(active), ops._p(loss), ops._p(coef),
                 ops._p(ws), nbytes, ops._stream())
        ctx.mark_non_differentiable(pair, perm_idx, active)
        ctx.save_for_backward(sources, estimates, lengths, perms, perm_idx, coef)
        ctx.set_materialize_grads(False)
        return loss, per_utt, pair, perm_idx, active

    @staticmethod
    def backward(ctx, g_loss, g_per, _g_pair, _g_idx, _g_active):
        sources, estimates, lengths, perms, perm_idx, coef = ctx.saved_tensors
        Bn, C, T = estimates.shape
        d_est = torch.empty_like(estimates)
        g_loss, g_per = ops._upstream(g_loss, g_per)
        lib.call("ctn_varpit_bwd", ops._p(sources), ops._p(estimates), ops._p(lengths), ops._p(perms), ops._p(perm_idx), ops._p(coef),
                 ops._p(g_loss), ops._p(g_per), Bn, C, T, ops._p(d_est), ops._stream())
        return None, d_est, None, None, None


def cal_varpit_loss(source, estimate_source, lengths, snr_max=30.0, inactive_snr_max=20.0):
    """-> (loss, per_utt [B], pair [B,C,C], perm_idx [B], active [B,C]).

    source [B,C,T]: the references, a silent speaker being a row of zeros; estimate_source [B,C,T], 2 <= C <= 6, contiguous fp32
    on the GPU and NOT modified; lengths [B]: only t < length counts.  snr_max / inactive_snr_max: the soft thresholds in dB of
    the active and the inactive pair loss (None: none).  loss = mean(per_utt); per_utt = the mean over the C outputs of the pair
    losses at the best permutation; pair[b,i,j] = the loss of estimate i against reference j in dB; perm_idx indexes
    itertools.permutations(range(C)), perm[i] = the reference of estimate i; active[b,j] = 1 where reference j is not silent.
    loss and per_utt are differentiable in estimate_source."""
    return VarPit.apply(source, estimate_source, lengths, threshold(snr_max), threshold(inactive_snr_max))


def assignment(perm_idx, C):
    """[B] permutation indices -> [B,C] int64: the reference that estimate i is paired with."""
    return torch.index_select(ops._perms(C, perm_idx.device)[1], 0, perm_idx)


class VarPitCriterion:
    """Solver criterion: (sources [B,C,T] with silent rows, estimate [B,C,T], lengths) -> the scalar loss."""

    def __init__(self, snr_max=30.0, inactive_snr_max=20.0):
        self.snr_max, self.inactive_snr_max = snr_max, inactive_snr_max

    def __call__(self, sources, estimate, lengths):
        return cal_varpit_loss(sources, estimate, lengths, self.snr_max, self.inactive_snr_max)[0]


def output_levels(estimate, mixture, lengths):
    """[B,C] float64: 10 log10((sum e_i^2 + 1e-8) / (sum mix^2 + 1e-8)) over t < length, the level of every output relative to
    the mixture in dB.  Plain torch: a few reductions per minibatch."""
    if estimate.dim() != 3 or mixture.shape != (estimate.size(0), estimate.size(2)):
        raise ValueError("estimate must be [B, C, T] and mixture [B, T], got %s and %s" % (tuple(estimate.shape), tuple(mixture.shape)))
    T = estimate.size(2)
    lens = lengths.to(estimate.device).clamp(0, T)
    if lens.shape != (estimate.size(0),):
        raise ValueError("lengths must be [B]")
    keep = (torch.arange(T, device=estimate.device).view(1, T) < lens.view(-1, 1)).double()
    ee = (estimate.detach().double() ** 2 * keep.unsqueeze(1)).sum(-1)
    mm = (mixture.to(estimate.device).double() ** 2 * keep).sum(-1, keepdim=True)
    return 10.0 * torch.log10((ee + EPS) / (mm + EPS))


def count_sources(estimate, mixture, lengths, threshold_db=-20.0):
    """[B] int64: the number of outputs whose level is above threshold_db relative to the mixture.  The default is a starting
    point: tune it on validation data (evaluate_variable prints the confusion matrix it gives)."""
    return (output_levels(estimate, mixture, lengths) > float(threshold_db)).sum(1)


def evaluate_variable(model, loader, threshold_db=-20.0, verbose=True, snr_max=30.0, inactive_snr_max=20.0):
    """Scores `model` on a loader of (mixture [B,T], lengths [B], sources [B,C,T]) minibatches whose silent speakers are rows of
    zeros -> (confusion [C+1,C+1] int64 numpy: confusion[n_true, n_counted] utterances, the average SI-SNRi in dB by
    evaluate.cal_SISNR over the active references under the loss's assignment, the mean level in dB relative to the mixture of
    the outputs assigned to inactive references; NaN where there was none)."""
    from .evaluate import cal_SISNR
    model.eval()
    dev = next(model.parameters()).device
    confusion = None
    total, pairs, level, silent = 0.0, 0, 0.0, 0
    with torch.no_grad():
        for mixture, lengths, sources in loader:
            mixture, lengths, sources = mixture.to(dev), lengths.to(dev), sources.to(dev)
            est = model(mixture)
            C, T = est.size(1), est.size(2)
            _, _, _, perm_idx, active = cal_varpit_loss(sources, est, lengths, snr_max, inactive_snr_max)
            levels = output_levels(est, mixture, lengths)
            counted = (levels > float(threshold_db)).sum(1).tolist()
            ref_of, act = assignment(perm_idx, C).tolist(), active.tolist()
            if confusion is None:
                confusion = np.zeros((C + 1, C + 1), dtype=np.int64)
            lens = lengths.clamp(0, T).tolist()
            mix_h, src_h, est_h, lev_h = mixture.double().cpu().numpy(), sources.double().cpu().numpy(), \
                est.double().cpu().numpy(), levels.cpu().numpy()
            for b in range(est.size(0)):
                confusion[sum(act[b]), counted[b]] += 1
                n = lens[b]
                for i in range(C):
                    j = ref_of[b][i]
                    if act[b][j] and n > 0:
                        total += cal_SISNR(src_h[b, j, :n], est_h[b, i, :n]) - cal_SISNR(src_h[b, j, :n], mix_h[b, :n])
                        pairs += 1
                    elif not act[b][j]:
                        level += float(lev_h[b, i])
                        silent += 1
    if confusion is None:
        raise ValueError("the loader yielded no minibatch")
    sisnri = total / pairs if pairs else float("nan")
    inactive_db = level / silent if silent else float("nan")
    if verbose:
        print("Speaker count, rows = true, columns = counted at %.1f dB:" % float(threshold_db))
        for r in range(confusion.shape[0]):
            print("\t%d: %s" % (r, " ".join("%6d" % v for v in confusion[r])))
        print("Average SISNR improvement over %d active references: %.2f" % (pairs, sisnri))
        print("Average level of %d outputs assigned to inactive references: %.2f dB relative to the mixture" % (silent, inactive_db))
    return confusion, sisnri, inactive_db
