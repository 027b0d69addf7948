"""Mixture invariant training (MixIT: Wisdom et al., NeurIPS 2020) on the HIP loss kernels of csrc/ctn_mixit.hip.

Training without isolated sources: two mixtures are added, the model separates the sum into M outputs, and the loss is the
soft-thresholded SNR of the best assignment of the outputs to the two mixtures.  `cal_mixit_loss` is the criterion,
`MixtureOfMixtures` and `pair_batch` produce the (mixture of mixtures, lengths, two references) minibatches, `remix` applies
an assignment.  include/ctn_hip.h ("mixture invariant training loss") fixes the definition.
"""
import torch

from . import ops
from ._lib import lib

F32 = torch.float32
MIN_OUTPUTS, MAX_OUTPUTS = 2, 8


def threshold(snr_max):
    """tau = 10^(-snr_max / 10) of the soft threshold; None -> 0 (plain SNR)."""
    if snr_max is None:
        return 0.0
    return 10.0 ** (-float(snr_max) / 10.0)


class MixIt(torch.autograd.Function):
    """(mixtures [B,2,T], estimates [B,M,T], lengths [B], tau) -> (loss [], per_utt [B], snr [B,2], assign [B] packed: bit i =
    the mixture of source i).  Differentiable in `estimates` through `loss` and `per_utt`; `estimates` is not modified."""

    @staticmethod
    def forward(ctx, mixtures, estimates, lengths, tau):
        if mixtures.dim() != 3 or estimates.dim() != 3 or mixtures.size(1) != 2:
            raise ValueError("mixtures must be [B, 2, T] and estimates [B, M, T], got %s and %s"
                             % (tuple(mixtures.shape), tuple(estimates.shape)))
        Bn, M, T = estimates.shape
        if mixtures.size(0) != Bn or mixtures.size(2) != T:
            raise ValueError("mixtures %s and estimates %s differ in batch or length" % (tuple(mixtures.shape), tuple(estimates.shape)))
        if not MIN_OUTPUTS <= M <= MAX_OUTPUTS:
            raise ValueError("MixIT over %d .. %d outputs, got %d" % (MIN_OUTPUTS, MAX_OUTPUTS, M))
        if Bn < 1 or T < 1:
            raise ValueError("empty batch or zero-length signals")
        mixtures, lengths = ops._loss_inputs(mixtures, estimates, lengths)
        dev = estimates.device
        loss = torch.empty((), dtype=F32, device=dev)
        per_utt = torch.empty((Bn,), dtype=F32, device=dev)
        snr = torch.empty((Bn, 2), dtype=F32, device=dev)
        assign = torch.empty((Bn,), dtype=torch.int64, device=dev)
        coef = torch.empty((Bn, 2), dtype=F32, device=dev)
        nbytes = lib.ctn_mixit_workspace(Bn, M, T)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        lib.call("ctn_mixit_fwd", ops._p(mixtures), ops._p(estimates), ops._p(lengths), Bn, M, T, float(tau), ops._p(per_utt),
                 ops._p(assign), ops._p(snr), ops._p(loss), ops._p(coef), ops._p(ws), nbytes, ops._stream())
        ctx.mark_non_differentiable(snr, assign)
        ctx.save_for_backward(mixtures, estimates, lengths, assign, coef)
        ctx.set_materialize_grads(False)
        return loss, per_utt, snr, assign

    @staticmethod
    def backward(ctx, g_loss, g_per, _g_snr, _g_assign):
        mixtures, estimates, lengths, assign, coef = ctx.saved_tensors
        Bn, M, T = estimates.shape
        d_est = torch.empty_like(estimates)
        g_loss, g_per = ops._upstream(g_loss, g_per)
        lib.call("ctn_mixit_bwd", ops._p(mixtures), ops._p(estimates), ops._p(lengths), ops._p(assign), ops._p(coef),
                 ops._p(g_loss), ops._p(g_per), Bn, M, T, ops._p(d_est), ops._stream())
        return None, d_est, None, None


def unpack_assign(packed, M):
    """[B] packed assignments -> [B, M] int64: the mixture index (0 or 1) of every source."""
    bits = torch.arange(M, device=packed.device, dtype=torch.int64)
    return (packed.unsqueeze(1) >> bits) & 1


def cal_mixit_loss(mixtures, estimate_source, lengths, snr_max=30.0):
    """-> (loss, per_utt [B], snr [B,2], assign [B,M]).

    mixtures [B,2,T]: the two reference mixtures; estimate_source [B,M,T], 2 <= M <= 8, contiguous fp32 on the GPU and NOT
    modified; lengths [B]: only t < length counts.  snr_max: the soft threshold in dB (None: none).  loss = mean(per_utt),
    per_utt = the mean over the two mixtures of -SNR at the best assignment, snr = those two SNRs in dB, assign[b, i] = the
    mixture source i belongs to.  loss and per_utt are differentiable in estimate_source."""
    loss, per_utt, snr, packed = MixIt.apply(mixtures, estimate_source, lengths, threshold(snr_max))
    return loss, per_utt, snr, unpack_assign(packed, estimate_source.size(1))


def remix(estimate_source, assign):
    """[B,M,T] sources and assign [B,M] (0 / 1 per source) -> [B,2,T]: the two remixed mixtures, for listening and scoring."""
    if assign.shape != estimate_source.shape[:2]:
        raise ValueError("assign must be [B, M] = %s, got %s" % (tuple(estimate_source.shape[:2]), tuple(assign.shape)))
    one = assign.to(device=estimate_source.device).bool().unsqueeze(-1)
    zero = torch.zeros((), dtype=estimate_source.dtype, device=estimate_source.device)
    return torch.stack((torch.where(one, zero, estimate_source).sum(1), torch.where(one, estimate_source, zero).sum(1)), dim=1)


def pair_batch(mixture, lengths):
    """Mixtures of mixtures when there are no sources at all: rows 2k and 2k+1 of mixture [B,T] are added.

    -> (mom [B/2,T], lengths [B/2] = the pair's shorter length, refs [B/2,2,T]); samples at or beyond that length are zeroed in
    both references, so mom = refs[:,0] + refs[:,1] exactly."""
    if mixture.dim() != 2 or lengths.shape != (mixture.size(0),):
        raise ValueError("mixture must be [B, T] and lengths [B]")
    Bn, T = mixture.shape
    if Bn < 2 or Bn % 2:
        raise ValueError("pair_batch needs an even number of mixtures, got %d" % Bn)
    lens = lengths.to(mixture.device).view(Bn // 2, 2).min(dim=1).values
    keep = torch.arange(T, device=mixture.device).view(1, 1, T) < lens.view(-1, 1, 1)
    refs = torch.where(keep, mixture.view(Bn // 2, 2, T), torch.zeros((), dtype=mixture.dtype, device=mixture.device))
    return refs[:, 0] + refs[:, 1], lens, refs


class MixtureOfMixtures:
    """Wraps a loader of the AudioDataLoader contract whose sources are [B,C,T] (e.g. DynamicMixLoader(num_speakers=4)) and
    yields (mixture, lengths, refs [B,2,T]): refs[:, n] is the fp32 sum of the sources of groups[n], added in ascending index
    order; `mixture` (the model input) passes through untouched.  With 4 speakers and the default groups every minibatch is
    a mixture of two 2-speaker mixtures, and the isolated sources are never shown to the criterion."""

    def __init__(self, loader, groups=((0, 1), (2, 3))):
        groups = tuple(tuple(sorted(int(i) for i in g)) for g in groups)
        if len(groups) != 2:
            raise ValueError("MixIT takes two reference mixtures: 2 groups, got %d" % len(groups))
        flat = [i for g in groups for i in g]
        if any(len(g) == 0 for g in groups) or len(set(flat)) != len(flat):
            raise ValueError("groups must be non-empty and must not overlap: %r" % (groups,))
        if sorted(flat) != list(range(len(flat))):
            raise ValueError("groups must cover sources 0 .. C-1 exactly: %r" % (groups,))
        self.loader, self.groups = loader, groups

    dataset = property(lambda self: self)        # Solver: loader.dataset.set_epoch(epoch)

    def __len__(self):
        return len(self.loader)

    def set_epoch(self, epoch):
        ds = getattr(self.loader, "dataset", None)
        if hasattr(ds, "set_epoch"):
            ds.set_epoch(epoch)

    def references(self, sources):
        C = sum(len(g) for g in self.groups)
        if sources.dim() != 3 or sources.size(1) != C:
            raise ValueError("the groups %r cover %d sources, the loader yields %s" % (self.groups, C, tuple(sources.shape)))
        refs = []
        for g in self.groups:
            r = sources[:, g[0]].to(F32)
            for i in g[1:]:
                r = r + sources[:, i].to(F32)
            refs.append(r)
        return torch.stack(refs, dim=1)

    def __iter__(self):
        for mixture, lengths, sources in self.loader:
            yield mixture, lengths, self.references(sources)


class MixItCriterion:
    """Solver criterion: (refs [B,2,T], estimate [B,M,T], lengths) -> the scalar MixIT loss."""

    def __init__(self, snr_max=30.0):
        self.snr_max = snr_max

    def __call__(self, sources, estimate, lengths):
        return cal_mixit_loss(sources, estimate, lengths, self.snr_max)[0]
