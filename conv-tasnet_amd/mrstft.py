"""Multi-resolution STFT loss on the GPU in fp64 (csrc/ctn_mrstft.hip): spectral convergence plus log-magnitude (and, optionally,
linear-magnitude) distance over several analysis windows, for padded batches in device memory, differentiable in the estimate.

    t = mrstft_pairs(ref, est, lengths, est_of_ref)           # [B,C,T], [B,E,T], [B], [B,C] -> [B,C,R,3] fp64 on the device
    loss, t, est_of_ref = cal_mrstft_loss(src, est, lengths)  # the mean loss under the SI-SNR PIT pairing
    crit = MrStftPitCriterion(weight=1.0)                     # Solver criterion: PIT SI-SNR + weight * the spectral loss

R. Yamamoto, E. Song and J.-M. Kim, "Parallel WaveGAN: a fast waveform generation model based on generative adversarial networks
with multi-resolution spectrogram", ICASSP 2020; the values are those of auraloss's MultiResolutionSTFTLoss on an unpadded
utterance.  A resolution is (n_fft, hop, win_length).  Row b is transformed over its own lengths[b] samples as
torch.stft(x[:n], n_fft, hop, win_length, hann_window(win_length), center=True, pad_mode='reflect') does: F = 1 + n // hop frames,
reflect padding about the utterance's own ends.  |X| = sqrt(max(re^2 + im^2, eps)).  Per (pair, resolution), over all bins:

    terms[..., 0] = sc     = || |S| - |S^| ||_F / || |S| ||_F
    terms[..., 1] = logmag = mean | log|S| - log|S^| |
    terms[..., 2] = linmag = mean | |S| - |S^| |

A cell with n <= n_fft / 2, where reflect padding is undefined, has terms and gradient exactly 0 (nothing is read back to warn).
The reference is a constant; a clamped bin passes no gradient.  There is no CPU path.
"""
import numpy as np
import torch

from ._lib import lib
from .stoi import _check_pairing

DEFAULT_RESOLUTIONS = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))
EPS = 1e-7                     # auraloss's clamp on re^2 + im^2
MAX_RESOLUTIONS = 8
MIN_FFT, MAX_FFT = 64, 2048
MAX_COVER = 64                 # frames over one sample: ceil(win_length / hop)
WORKSPACE_BUDGET = 1 << 30     # bytes of workspace per C call; larger batches are split


def _ptr(t):
    return t.data_ptr()


def check_resolutions(resolutions):
    """-> a tuple of (n_fft, hop, win_length) int triples, or ValueError for anything the kernels do not take."""
    try:
        res = tuple(tuple(r) for r in resolutions)
    except TypeError:
        raise ValueError("resolutions must be a sequence of (n_fft, hop, win_length) triples, got %r" % (resolutions,))
    if not 1 <= len(res) <= MAX_RESOLUTIONS:
        raise ValueError("1 .. %d resolutions, got %d" % (MAX_RESOLUTIONS, len(res)))
    out = []
    for r in res:
        if len(r) != 3 or any(isinstance(v, bool) or int(v) != v for v in r):
            raise ValueError("a resolution is three integers (n_fft, hop, win_length), got %r" % (r,))
        n_fft, hop, win = (int(v) for v in r)
        if not MIN_FFT <= n_fft <= MAX_FFT or n_fft & (n_fft - 1):
            raise ValueError("n_fft must be a power of two in %d .. %d, got %d" % (MIN_FFT, MAX_FFT, n_fft))
        if not 1 <= win <= n_fft:
            raise ValueError("1 <= win_length <= n_fft = %d, got %d" % (n_fft, win))
        if hop < 1 or -(-win // hop) > MAX_COVER:
            raise ValueError("1 <= hop and ceil(win_length / hop) <= %d, got hop %d for win_length %d" % (MAX_COVER, hop, win))
        out.append((n_fft, hop, win))
    return tuple(out)


def parse_resolutions(text):
    """'1024:120:600,2048:240:1200' -> ((1024, 120, 600), (2048, 240, 1200)) (train.py --mrstft-resolutions)."""
    try:
        res = tuple(tuple(int(v) for v in item.split(":")) for item in str(text).split(","))
    except ValueError:
        raise ValueError("resolutions must be N_FFT:HOP:WIN[,N_FFT:HOP:WIN...], got %r" % (text,))
    return check_resolutions(res)


def _check_weight(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not v >= 0:
        raise ValueError("%s must be a non-negative number, got %r" % (name, v))
    return float(v)


def _check_inputs(ref, est, lengths):
    if not torch.is_tensor(ref) or not torch.is_tensor(est):
        raise ValueError("mrstft_pairs takes torch tensors on the GPU")
    if ref.device.type != "cuda" or est.device != ref.device:
        raise ValueError("mrstft_pairs runs on the GPU: got tensors on %s and %s" % (ref.device, est.device))
    if ref.dim() != 3 or est.dim() != 3 or ref.shape[0] != est.shape[0] or ref.shape[2] != est.shape[2]:
        raise ValueError("ref [B,C,T] and est [B,E,T] do not match: %s vs %s" % (tuple(ref.shape), tuple(est.shape)))
    if min(ref.shape) < 1 or est.shape[1] < 1:
        raise ValueError("empty input: ref %s, est %s" % (tuple(ref.shape), tuple(est.shape)))
    lengths = torch.as_tensor(lengths)
    if lengths.dim() != 1 or lengths.shape[0] != ref.shape[0]:
        raise ValueError("lengths must be [B] = [%d], got %s" % (ref.shape[0], tuple(lengths.shape)))
    return lengths


class _MrStftPairs(torch.autograd.Function):
    """(ref [B,C,T], est [B,E,T] fp32, lengths int64 [B], est_of_ref int32 [B,C], resolutions, eps) -> terms [B,C,R,3] fp64.
    Differentiable in est (fp32 gradient)."""

    @staticmethod
    def forward(ctx, ref, est, lengths, est_of_ref, resolutions, eps):
        dev = est.device
        B, C, T = ref.shape
        E = est.shape[1]
        R = len(resolutions)
        res = np.ascontiguousarray(np.asarray(resolutions, dtype=np.int32).reshape(R, 3))
        per_f, per_b = lib.ctn_mrstft_workspace(1, C, T, R, res.ctypes.data), lib.ctn_mrstft_bwd_workspace(1, C, T, R, res.ctypes.data)
        if per_f == 0 or per_b == 0 or E > 65535:
            raise ValueError("mrstft_pairs: sizes out of range (C = %d, E = %d, T = %d)" % (C, E, T))
        step = max(1, min(B, WORKSPACE_BUDGET // max(per_f, per_b), 65535 // max(C, E)))
        stream = torch.cuda.current_stream(dev).cuda_stream
        terms = torch.empty(B, C, R, 3, dtype=torch.float64, device=dev)
        saved = []
        for b0 in range(0, B, step):
            nb = min(step, B - b0)
            ws = torch.empty(lib.ctn_mrstft_workspace(nb, C, T, R, res.ctypes.data), dtype=torch.uint8, device=dev)
            lib.call("ctn_mrstft_pairs_fwd", _ptr(ref[b0:b0 + nb]), _ptr(est[b0:b0 + nb]), _ptr(lengths[b0:b0 + nb]),
                     _ptr(est_of_ref[b0:b0 + nb]), nb, C, E, T, res.ctypes.data, R, eps, _ptr(terms[b0:b0 + nb]), _ptr(ws), ws.numel(),
                     stream)
            saved.append(ws)
        ctx.save_for_backward(ref, est, lengths, est_of_ref, *saved)
        ctx.geom = (B, C, E, T, R, res, step, eps)
        return terms

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        ref, est, lengths, est_of_ref = ctx.saved_tensors[:4]
        saved = ctx.saved_tensors[4:]
        B, C, E, T, R, res, step, eps = ctx.geom
        dev = g.device
        g = g.to(torch.float64).contiguous()
        g_est = torch.empty(B, E, T, dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        ws = torch.empty(lib.ctn_mrstft_bwd_workspace(min(step, B), C, T, R, res.ctypes.data), dtype=torch.uint8, device=dev)
        for k, b0 in enumerate(range(0, B, step)):
            nb = min(step, B - b0)
            lib.call("ctn_mrstft_pairs_bwd", _ptr(saved[k]), saved[k].numel(), _ptr(ref[b0:b0 + nb]), _ptr(est[b0:b0 + nb]),
                     _ptr(lengths[b0:b0 + nb]), _ptr(est_of_ref[b0:b0 + nb]), nb, C, E, T, res.ctypes.data, R, eps, _ptr(g[b0:b0 + nb]),
                     _ptr(g_est[b0:b0 + nb]), _ptr(ws), ws.numel(), stream)
        return None, g_est, None, None, None, None


def mrstft_pairs(ref, est, lengths, est_of_ref, resolutions=DEFAULT_RESOLUTIONS, eps=EPS):
    """ref [B,C,T], est [B,E,T] fp32 on the GPU (other dtypes are cast), lengths [B], est_of_ref [B,C] integer on the GPU ->
    [B,C,R,3] fp64: (sc, logmag, linmag) of reference c against estimate row est_of_ref[b,c] (entries outside [0,E) are clamped;
    rows need not form a permutation) at every resolution.  Differentiable in est: the backward pass returns an fp32 gradient of
    est's shape, exactly zero at t >= lengths[b] and for rows no reference chose.  A reference that requires grad raises
    ValueError.  Samples beyond lengths[b] are never read.  The forward workspace (the per-frame sums: 32 bytes per frame) and the
    two input tensors stay alive until the backward pass; the backward pass allocates 8 bytes per frame and window tap."""
    lengths = _check_inputs(ref, est, lengths)
    if ref.requires_grad:
        raise ValueError("mrstft_pairs differentiates the estimate only: the reference must not require grad")
    resolutions = check_resolutions(resolutions)
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not eps > 0:
        raise ValueError("eps must be a positive number, got %r" % (eps,))
    dev = ref.device
    B, C, T = ref.shape
    est_of_ref = _check_pairing(est_of_ref, B, C, est.shape[1], dev)
    ref = ref.detach().to(dtype=torch.float32).contiguous()
    est = est.to(dtype=torch.float32).contiguous()
    lengths = lengths.to(device=dev, dtype=torch.int64).clamp(0, T).contiguous()
    return _MrStftPairs.apply(ref, est, lengths, est_of_ref, resolutions, float(eps))


def combine(terms, w_sc=1.0, w_log=1.0, w_lin=0.0):
    """terms [B,C,R,3] -> the batch loss: the mean over pairs of the mean over resolutions of w_sc sc + w_log logmag + w_lin linmag."""
    return (w_sc * terms[..., 0] + w_log * terms[..., 1] + w_lin * terms[..., 2]).mean()


def cal_mrstft_loss(source, estimate_source, source_lengths, resolutions=DEFAULT_RESOLUTIONS, w_sc=1.0, w_log=1.0, w_lin=0.0,
                    perm="sisnr"):
    """-> (loss, terms [B,C,R,3] fp64, est_of_ref [B,C] int32), loss differentiable in estimate_source.

    source, estimate_source [B,C,T] on the GPU.  perm "sisnr": the pairing of the SI-SNR PIT kernel (cal_si_snr_with_pit):
    reference c goes with the estimate whose SI-SNR against it was averaged into max_snr, i.e. the INVERSE of the permutation row,
    as cal_stoi_loss pairs; the kernel runs on a copy, so estimate_source is not modified.  perm may also be an explicit [B,C]
    integer tensor of estimate rows."""
    if source.dim() != 3 or source.shape != estimate_source.shape:
        raise ValueError("source and estimate_source must both be [B,C,T], got %s and %s"
                         % (tuple(source.shape), tuple(estimate_source.shape)))
    w_sc, w_log, w_lin = _check_weight("w_sc", w_sc), _check_weight("w_log", w_log), _check_weight("w_lin", w_lin)
    if torch.is_tensor(perm):
        est_of_ref = perm
    elif perm == "sisnr":
        from .pit_criterion import cal_si_snr_with_pit
        with torch.no_grad():
            _, perms, idx = cal_si_snr_with_pit(source, estimate_source.detach().to(torch.float32).clone(), source_lengths)
        # perms[idx][i] is the reference of estimate i: invert the row
        est_of_ref = torch.argsort(perms.index_select(0, idx).to(torch.int64), dim=1).to(torch.int32)
    else:
        raise ValueError('perm must be "sisnr" or a [B,C] tensor, got %r' % (perm,))
    terms = mrstft_pairs(source, estimate_source, source_lengths, est_of_ref, resolutions)
    return combine(terms, w_sc, w_log, w_lin), terms, est_of_ref.to(torch.int32)


class MrStftPitCriterion:
    """Solver criterion: cal_loss's PIT SI-SNR loss plus weight * the multi-resolution STFT loss under the same pairing.
    `weight` is the user's hyper-parameter: the SI-SNR term is in dB, the spectral terms are of order 1.  weight = 0 is cal_loss
    alone."""

    def __init__(self, weight, resolutions=DEFAULT_RESOLUTIONS, w_sc=1.0, w_log=1.0, w_lin=0.0):
        self.weight = _check_weight("weight", weight)
        self.resolutions = check_resolutions(resolutions)
        self.w_sc, self.w_log, self.w_lin = _check_weight("w_sc", w_sc), _check_weight("w_log", w_log), _check_weight("w_lin", w_lin)

    def __call__(self, sources, estimate, lengths):
        from . import ops
        from .pit_criterion import _pit
        loss, _, est, idx = _pit(sources, estimate, lengths)          # cal_loss's loss; est is estimate, length-masked in place
        if self.weight == 0.0:
            return loss
        perms = ops._perms(sources.size(1), sources.device)[1]
        est_of_ref = torch.argsort(perms.index_select(0, idx).to(torch.int64), dim=1).to(torch.int32)
        terms = mrstft_pairs(sources, est, lengths, est_of_ref, self.resolutions)
        return loss + (self.weight * combine(terms, self.w_sc, self.w_log, self.w_lin)).to(loss.dtype)
