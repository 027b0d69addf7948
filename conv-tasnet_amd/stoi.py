"""STOI and ESTOI intelligibility scores on the GPU in fp64 (csrc/ctn_stoi.hip): what pystoi.stoi computes per utterance on
the host, for padded batches in device memory.

    d = stoi_batch(ref, est, lengths, 8000)                   # [B,C,T], [B,E,T], [B] -> [B,E,C] fp64 on the device
    d = stoi_batch(ref, est, lengths, 8000, extended=True)    # ESTOI
    st, es, M, K = stoi_both(ref, est, lengths, 8000)         # both measures of one pass, with the frame counts
    d = stoi(x, y, fs_sig)                                    # pystoi's call form: 1-D numpy or torch in, float out
    d = stoi_pairs(ref, est, lengths, 8000, est_of_ref)       # [B,C] fp64 of the chosen pairs, differentiable in est
    loss, d, est_of_ref = cal_stoi_loss(src, est, lengths, 8000)      # 1 - mean score under the SI-SNR PIT pairing
    crit = StoiPitCriterion(8000, weight=10.0)                # Solver criterion: PIT SI-SNR + weight * (1 - mean score)

C. H. Taal et al., "An Algorithm for Intelligibility Prediction of Time-Frequency Weighted Noisy Speech", IEEE TASLP 2011
(STOI); J. Jensen and C. H. Taal, "An Algorithm for Predicting the Intelligibility of Speech Masked by Modulated Noise
Maskers", IEEE/ACM TASLP 2016 (ESTOI).  The measure is defined at 10 kHz: signals at another rate are first resampled on the
device by resample.resample_rows (the project's Kaiser-windowed sinc; pystoi uses a MATLAB-compatible polyphase design, so
scores at other rates differ from pystoi's by the resampling filter).  Every estimate row is scored against every reference;
the silent-frame mask is the reference's.  There is no CPU path.

The training loss (csrc/ctn_stoi_grad.hip; Kolbaek et al., ICASSP 2018; Fu et al., IEEE/ACM TASLP 2018) differentiates the score
of chosen (reference, estimate) pairs with respect to the estimate only: the reference's silent-frame mask, envelopes and clip
bound are constants, a clipped cell passes no gradient, the resampler is the linear map of its fp32 tap table.
"""
import itertools
import warnings

import numpy as np
import torch

from . import resample as rs
from ._lib import lib

FS = 10000
N_SEGMENT = 30                 # frames per segment: an utterance with fewer frames after silent-frame removal scores TOO_SHORT
TOO_SHORT = 1e-5               # pystoi's value for it
WORKSPACE_BUDGET = 1 << 30     # bytes of workspace per ctn_stoi_eval call; larger batches are split


def _ptr(t):
    return t.data_ptr()


def _check_inputs(ref, est, lengths, sample_rate):
    if not torch.is_tensor(ref) or not torch.is_tensor(est):
        raise ValueError("stoi_batch takes torch tensors on the GPU")
    if ref.device.type != "cuda" or est.device != ref.device:
        raise ValueError("stoi_batch runs on the GPU: got tensors on %s and %s" % (ref.device, est.device))
    if ref.dim() != 3 or est.dim() != 3 or ref.shape[0] != est.shape[0] or ref.shape[2] != est.shape[2]:
        raise ValueError("ref [B,C,T] and est [B,E,T] do not match: %s vs %s" % (tuple(ref.shape), tuple(est.shape)))
    if min(ref.shape) < 1 or est.shape[1] < 1:
        raise ValueError("empty input: ref %s, est %s" % (tuple(ref.shape), tuple(est.shape)))
    if isinstance(sample_rate, bool) or int(sample_rate) != sample_rate or int(sample_rate) <= 0:
        raise ValueError("sample_rate must be a positive integer, got %r" % (sample_rate,))
    lengths = torch.as_tensor(lengths)
    if lengths.dim() != 1 or lengths.shape[0] != ref.shape[0]:
        raise ValueError("lengths must be [B] = [%d], got %s" % (ref.shape[0], tuple(lengths.shape)))
    return lengths


def _check_nonsilent(ref, lengths):
    t = torch.arange(ref.shape[-1], device=ref.device)
    live = ((ref != 0) & (t < lengths.view(-1, 1, 1))).any(-1)
    if not bool(live.all()):
        raise ValueError("every reference must be non-silent over its length, but at least one of them is all zeros: "
                         "its frame energies give no silent-frame threshold")


def _to_10k(x, lens_host, up, down, T10):
    """x [B,R,T] fp32 on the GPU, row b valid over lens_host[b] samples -> [B,R,T10] at 10 kHz (zeros beyond each row)."""
    B, R, T = x.shape
    y = torch.zeros(B, R, T10, dtype=torch.float32, device=x.device)
    rows = np.arange(B * R, dtype=np.int64)
    rs.resample_rows(x.reshape(-1), rows * T, np.repeat(lens_host, R), up, down, y.view(-1), rows * T10)
    return y


def stoi_both(ref, est, lengths, sample_rate):
    """ref [B,C,T], est [B,E,T] (fp32 on the GPU; other dtypes are cast), lengths [B], at sample_rate Hz ->
    (stoi, estoi, M, K): stoi / estoi [B,E,C] fp64 on the device, estimate e scored against reference c over the first
    lengths[b] samples; M, K [B,E,C] int32: the frames left after silent-frame removal and the first-pass frames kept.
    A pair with M < 30 scores 1e-5 (pystoi's value) with a warning."""
    lengths = _check_inputs(ref, est, lengths, sample_rate)
    dev = ref.device
    B, C, T = ref.shape
    E = est.shape[1]
    ref = ref.to(dtype=torch.float32).contiguous()
    est = est.to(dtype=torch.float32).contiguous()
    lengths = lengths.to(device=dev, dtype=torch.int64).clamp(0, T).contiguous()
    _check_nonsilent(ref, lengths)
    if int(sample_rate) != FS:
        up, down = rs.ratio(int(sample_rate), FS)
        lens_host = lengths.cpu().numpy()
        T = rs.out_len(T, up, down)
        ref, est = _to_10k(ref, lens_host, up, down, T), _to_10k(est, lens_host, up, down, T)
        lengths = torch.from_numpy((lens_host * up + down - 1) // down).to(dev)
    d_stoi = torch.empty(B, E, C, dtype=torch.float64, device=dev)
    d_estoi = torch.empty_like(d_stoi)
    M = torch.empty(B, E, C, dtype=torch.int32, device=dev)
    K = torch.empty_like(M)
    per = lib.ctn_stoi_workspace(1, C, E, T)
    if per == 0:
        raise ValueError("stoi_batch: sizes out of range (C = %d, E = %d, T = %d)" % (C, E, T))
    step = max(1, min(B, WORKSPACE_BUDGET // per, 65535))
    stream = torch.cuda.current_stream(dev).cuda_stream
    ws = torch.empty(lib.ctn_stoi_workspace(step, C, E, T), dtype=torch.uint8, device=dev)
    for b0 in range(0, B, step):
        nb = min(step, B - b0)
        lib.call("ctn_stoi_eval", _ptr(ref[b0:b0 + nb]), _ptr(est[b0:b0 + nb]), _ptr(lengths[b0:b0 + nb]), nb, C, E, T,
                 _ptr(d_stoi[b0:b0 + nb]), _ptr(d_estoi[b0:b0 + nb]), _ptr(M[b0:b0 + nb]), _ptr(K[b0:b0 + nb]), _ptr(ws),
                 ws.numel(), stream)
    if bool((M < N_SEGMENT).any()):
        warnings.warn("Not enough STFT frames to compute intermediate intelligibility measure after removing silent frames. "
                      "Returning 1e-5. Please check your wav files", RuntimeWarning, stacklevel=2)
    return d_stoi, d_estoi, M, K


def stoi_batch(ref, est, lengths, sample_rate, extended=False):
    """-> [B,E,C] fp64 on the device: STOI (ESTOI with `extended`) of estimate row e against reference c; see stoi_both."""
    d_stoi, d_estoi, _, _ = stoi_both(ref, est, lengths, sample_rate)
    return d_estoi if extended else d_stoi


def _as_row(x, name):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not torch.is_tensor(x):
        raise ValueError("%s: expected a numpy array or a torch tensor, got %s" % (name, type(x).__name__))
    return x


def stoi(x, y, fs_sig, extended=False):
    """pystoi.stoi(x, y, fs_sig, extended) on the current GPU: x the clean signal, y the processed one, 1-D numpy or torch of one
    length -> float."""
    x, y = _as_row(x, "x"), _as_row(y, "y")
    if x.shape != y.shape or x.dim() != 1:
        raise ValueError("x and y should be 1-D and have the same length, found %s and %s" % (tuple(x.shape), tuple(y.shape)))
    dev = torch.device("cuda", torch.cuda.current_device())
    d = stoi_batch(x.to(dev, torch.float32).view(1, 1, -1), y.to(dev, torch.float32).view(1, 1, -1),
                   torch.tensor([x.shape[0]], device=dev), fs_sig, extended)
    return float(d[0, 0, 0])


def stoi_improvement(d):
    """d [B,C+1,C]: the scores of the C estimates, already in PIT order, plus the mixture anchor as row C -> [B] fp64: the mean
    over k of d[k,k] - d[C,k]."""
    if d.dim() != 3 or d.shape[1] != d.shape[2] + 1:
        raise ValueError("stoi_improvement takes [B,C+1,C], got %s" % (tuple(d.shape),))
    C = d.shape[2]
    tot = d[:, 0, 0] - d[:, C, 0]
    for k in range(1, C):
        tot = tot + (d[:, k, k] - d[:, C, k])
    return tot / C


# ---- the scores as a training loss ----------------------------------------------------------------------------------------------
class _StoiPairs(torch.autograd.Function):
    """(ref10 [B,C,T10], est [B,E,T] at its own rate, est10 [B,E,T10], lengths, lengths10, est_of_ref int32 [B,C], up, down,
    extended) -> d [B,C] fp64.  Differentiable in est (fp32 gradient); est10 is est at 10 kHz (est itself when up = down)."""

    @staticmethod
    def forward(ctx, ref10, est, est10, lengths, lengths10, est_of_ref, up, down, extended):
        dev = est.device
        B, C, T10 = ref10.shape
        E = est.shape[1]
        per = lib.ctn_stoi_pairs_workspace(1, C, T10) + lib.ctn_stoi_pairs_bwd_workspace(1, C, T10)
        if lib.ctn_stoi_pairs_workspace(1, C, T10) == 0 or E > 65535:
            raise ValueError("stoi_pairs: sizes out of range (C = %d, E = %d, T = %d)" % (C, E, T10))
        step = max(1, min(B, WORKSPACE_BUDGET // per, 65535 // max(C, E)))
        stream = torch.cuda.current_stream(dev).cuda_stream
        d_stoi = torch.empty(B, C, dtype=torch.float64, device=dev)
        d_estoi = torch.empty_like(d_stoi)
        saved = []
        for b0 in range(0, B, step):
            nb = min(step, B - b0)
            ws = torch.empty(lib.ctn_stoi_pairs_workspace(nb, C, T10), dtype=torch.uint8, device=dev)
            lib.call("ctn_stoi_pairs_fwd", _ptr(ref10[b0:b0 + nb]), _ptr(est10[b0:b0 + nb]), _ptr(lengths10[b0:b0 + nb]),
                     _ptr(est_of_ref[b0:b0 + nb]), nb, C, E, T10, _ptr(d_stoi[b0:b0 + nb]), _ptr(d_estoi[b0:b0 + nb]), 0, _ptr(ws),
                     ws.numel(), stream)
            saved.append(ws)
        ctx.save_for_backward(lengths, est_of_ref, *saved)
        ctx.geom = (B, C, E, est.shape[2], T10, up, down, step, bool(extended))
        return d_estoi if extended else d_stoi

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        lengths, est_of_ref = ctx.saved_tensors[:2]
        saved = ctx.saved_tensors[2:]
        B, C, E, T, T10, up, down, step, extended = ctx.geom
        dev = g.device
        g = g.to(torch.float64).contiguous()
        zero = torch.zeros_like(g)
        w_stoi, w_estoi = (zero, g) if extended else (g, zero)
        h, W = rs.device_filter(up, down, dev) if up != down else (None, 0)
        g_est = torch.empty(B, E, T, dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        ws = torch.empty(lib.ctn_stoi_pairs_bwd_workspace(min(step, B), C, T10), dtype=torch.uint8, device=dev)
        for k, b0 in enumerate(range(0, B, step)):
            nb = min(step, B - b0)
            lib.call("ctn_stoi_pairs_bwd", _ptr(saved[k]), saved[k].numel(), _ptr(w_stoi[b0:b0 + nb]), _ptr(w_estoi[b0:b0 + nb]),
                     _ptr(est_of_ref[b0:b0 + nb]), _ptr(lengths[b0:b0 + nb]), nb, C, E, T, T10, up, down,
                     _ptr(h) if h is not None else 0, W, _ptr(g_est[b0:b0 + nb]), _ptr(ws), ws.numel(), stream)
        return None, g_est, None, None, None, None, None, None, None


def _check_pairing(est_of_ref, B, C, E, dev):
    if not torch.is_tensor(est_of_ref) or est_of_ref.dim() != 2 or tuple(est_of_ref.shape) != (B, C):
        raise ValueError("est_of_ref must be a [B,C] = [%d,%d] integer tensor" % (B, C))
    if est_of_ref.dtype not in (torch.int32, torch.int64) or est_of_ref.device != dev:
        raise ValueError("est_of_ref must be int32 or int64 on %s, got %s on %s" % (dev, est_of_ref.dtype, est_of_ref.device))
    return est_of_ref.to(torch.int32).contiguous()


def stoi_pairs(ref, est, lengths, sample_rate, est_of_ref, extended=False):
    """ref [B,C,T], est [B,E,T] fp32 on the GPU, lengths [B], est_of_ref [B,C] integer on the GPU -> [B,C] fp64: the STOI
    (ESTOI with `extended`) of reference c against estimate row est_of_ref[b,c] (entries outside [0,E) are clamped; rows need not
    form a permutation), bitwise the matching entries of stoi_both.  Differentiable in est: the backward pass returns an fp32
    gradient of est's shape, exactly zero at t >= lengths[b] and for pairs with fewer than 30 frames (which score 1e-5, without a
    warning: nothing is read back for it).  A reference that requires grad raises ValueError.
    WORKSPACE_BUDGET bounds the workspace of one C call, not what the autograd node retains: the forward workspace of every chunk
    (ctn_stoi_pairs_workspace: about 6 bytes per 10 kHz sample and pair) stays alive until the backward pass, so the retained
    memory grows with B."""
    lengths = _check_inputs(ref, est, lengths, sample_rate)
    if ref.requires_grad:
        raise ValueError("stoi_pairs differentiates the estimate only: the reference must not require grad")
    dev = ref.device
    B, C, T = ref.shape
    E = est.shape[1]
    est_of_ref = _check_pairing(est_of_ref, B, C, E, dev)
    ref = ref.detach().to(dtype=torch.float32).contiguous()
    est = est.to(dtype=torch.float32).contiguous()
    lengths = lengths.to(device=dev, dtype=torch.int64).clamp(0, T).contiguous()
    _check_nonsilent(ref, lengths)
    up, down = (1, 1) if int(sample_rate) == FS else rs.ratio(int(sample_rate), FS)
    if up == down:
        ref10, est10, lengths10 = ref, est.detach(), lengths
    else:
        lens_host = lengths.cpu().numpy()
        T10 = rs.out_len(T, up, down)
        with torch.no_grad():
            ref10, est10 = _to_10k(ref, lens_host, up, down, T10), _to_10k(est.detach(), lens_host, up, down, T10)
        lengths10 = torch.from_numpy((lens_host * up + down - 1) // down).to(dev)
    return _StoiPairs.apply(ref10, est, est10, lengths, lengths10, est_of_ref, up, down, extended)


MAX_PERM_SOURCES = 4           # perm="stoi" searches all C! permutations with torch ops


def _best_permutation(d):
    """d [B,C,C] (estimate e against reference c) -> est_of_ref [B,C] int32: the permutation with the largest mean score, the
    first one in itertools order on ties."""
    C = d.shape[1]
    table = torch.tensor(list(itertools.permutations(range(C))), dtype=torch.int64, device=d.device)      # [C!, C]: e of c
    tot = d.transpose(1, 2).gather(2, table.t().unsqueeze(0).expand(d.shape[0], C, -1)).sum(1)            # [B, C!]
    best = (tot == tot.max(dim=1, keepdim=True).values).to(torch.int32).argmax(dim=1)                     # first maximum
    return table[best].to(torch.int32)


def cal_stoi_loss(source, estimate_source, source_lengths, sample_rate, extended=False, perm="sisnr"):
    """-> (loss, scores [B,C] fp64, est_of_ref [B,C] int32) with loss = 1 - mean(scores), differentiable in estimate_source.

    source, estimate_source [B,C,T] on the GPU.  perm "sisnr": the pairing of the SI-SNR PIT kernel (cal_si_snr_with_pit):
    reference c goes with the estimate whose SI-SNR against it was averaged into max_snr, i.e. the INVERSE of the permutation row
    (reorder_source applies the row un-inverted, which differs for three-cycles at C = 3); the kernel runs on a copy, so
    estimate_source is not modified.  perm "stoi": the permutation with the best mean score (C <= 4; ties: the first in
    itertools order).  perm may also be an explicit [B,C] integer tensor of estimate rows."""
    if source.dim() != 3 or source.shape != estimate_source.shape:
        raise ValueError("source and estimate_source must both be [B,C,T], got %s and %s"
                         % (tuple(source.shape), tuple(estimate_source.shape)))
    C = source.shape[1]
    if torch.is_tensor(perm):
        est_of_ref = perm
    elif perm == "sisnr":
        from .pit_criterion import cal_si_snr_with_pit
        with torch.no_grad():
            _, perms, idx = cal_si_snr_with_pit(source, estimate_source.detach().to(torch.float32).clone(), source_lengths)
        # perms[idx][i] is the reference of estimate i: invert the row
        est_of_ref = torch.argsort(perms.index_select(0, idx).to(torch.int64), dim=1).to(torch.int32)
    elif perm == "stoi":
        if C > MAX_PERM_SOURCES:
            raise ValueError('perm="stoi" searches C! permutations: C <= %d, got %d' % (MAX_PERM_SOURCES, C))
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            d = stoi_batch(source, estimate_source.detach(), source_lengths, sample_rate, extended)
        est_of_ref = _best_permutation(d)
    else:
        raise ValueError('perm must be "sisnr", "stoi" or a [B,C] tensor, got %r' % (perm,))
    scores = stoi_pairs(source, estimate_source, source_lengths, sample_rate, est_of_ref, extended)
    return 1.0 - scores.mean(), scores, est_of_ref.to(torch.int32)


class StoiPitCriterion:
    """Solver criterion: cal_loss's PIT SI-SNR loss plus weight * (1 - mean STOI) (ESTOI with `extended`) under the same pairing.
    `weight` is the user's hyper-parameter: the SI-SNR term is in dB, the score in [0, 1].  weight = 0 is cal_loss alone."""

    def __init__(self, sample_rate, weight, extended=False):
        if isinstance(sample_rate, bool) or int(sample_rate) != sample_rate or int(sample_rate) <= 0:
            raise ValueError("sample_rate must be a positive integer, got %r" % (sample_rate,))
        if isinstance(weight, bool) or not isinstance(weight, (int, float)) or not weight >= 0:
            raise ValueError("weight must be a non-negative number, got %r" % (weight,))
        self.sample_rate, self.weight, self.extended = int(sample_rate), float(weight), bool(extended)

    def __call__(self, sources, estimate, lengths):
        from . import ops
        from .pit_criterion import _pit
        loss, _, est, idx = _pit(sources, estimate, lengths)          # cal_loss's loss; est is estimate, length-masked in place
        if self.weight == 0.0:
            return loss
        perms = ops._perms(sources.size(1), sources.device)[1]
        est_of_ref = torch.argsort(perms.index_select(0, idx).to(torch.int64), dim=1).to(torch.int32)
        scores = stoi_pairs(sources, est, lengths, self.sample_rate, est_of_ref, self.extended)
        return loss + (self.weight * (1.0 - scores.mean())).to(loss.dtype)
