"""STOI and ESTOI intelligibility scores on the GPU in fp64 (csrc/ctn_stoi.hip): what pystoi.stoi computes per utterance on
the host, for padded batches in device memory.

    d = stoi_batch(ref, est, lengths, 8000)                   # [B,C,T], [B,E,T], [B] -> [B,E,C] fp64 on the device
    d = stoi_batch(ref, est, lengths, 8000, extended=True)    # ESTOI
    st, es, M, K = stoi_both(ref, est, lengths, 8000)         # both measures of one pass, with the frame counts
    d = stoi(x, y, fs_sig)                                    # pystoi's call form: 1-D numpy or torch in, float out

C. H. Taal et al., "An Algorithm for Intelligibility Prediction of Time-Frequency Weighted Noisy Speech", IEEE TASLP 2011
(STOI); J. Jensen and C. H. Taal, "An Algorithm for Predicting the Intelligibility of Speech Masked by Modulated Noise
Maskers", IEEE/ACM TASLP 2016 (ESTOI).  The measure is defined at 10 kHz: signals at another rate are first resampled on the
device by resample.resample_rows (the project's Kaiser-windowed sinc; pystoi uses a MATLAB-compatible polyphase design, so
scores at other rates differ from pystoi's by the resampling filter).  Every estimate row is scored against every reference;
the silent-frame mask is the reference's.  There is no CPU path.
"""
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
