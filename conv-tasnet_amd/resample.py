"""On-device sinc resampling (csrc/ctn_resample.hip): a Kaiser-windowed-sinc polyphase resampler for ragged batches in
device memory -- what `librosa.load(path, sr=sample_rate)` does for the reference's loaders, and the primitive behind the
dynamic mixer's speed perturbation.

    y = resample(x, 16000, 8000)                                              # GPU tensor [..., T] -> [..., ceil(T / 2)]
    flat, offsets, lens = resample_ragged(flat, offsets, lens, 16000, 8000)   # rows of one flat device buffer

The filter is designed here on the host in float64 and rounded once to float32 (include/ctn_hip.h has the contract, the
tests restate it in numpy); the device sums the taps in a stated order with one rounding per operation, so an output is a
bitwise function of the table and the input.  There is no CPU fallback: a CPU tensor raises.
"""
import math

import numpy as np
import torch

from ._lib import lib

ZEROS, ROLLOFF, BETA = 32, 0.95, 14.77
PCT_LO, PCT_HI = 50, 200            # speed percents the dynamic mixer accepts
CHUNK = 1024                        # outputs per workgroup of the segments kernel
LDS_BYTES = 60 * 1024               # dynamic LDS of one workgroup at most (csrc/ctn_resample.hip)


def ratio(orig_sr, new_sr):
    """(up, down) = new_sr / orig_sr in lowest terms."""
    orig_sr, new_sr = int(orig_sr), int(new_sr)
    if orig_sr < 1 or new_sr < 1:
        raise ValueError("sample rates must be positive, got %d -> %d" % (orig_sr, new_sr))
    g = math.gcd(orig_sr, new_sr)
    return new_sr // g, orig_sr // g


def out_len(n_in, up, down):
    """ceil(n_in * up / down)."""
    return (int(n_in) * int(up) + int(down) - 1) // int(down)


def design_filter(up, down, zeros=ZEROS, rolloff=ROLLOFF, beta=BETA):
    """-> (h float32 [up, 2W], W): the polyphase bank of up / down (lowest terms), float64 rounded once to float32."""
    up, down = int(up), int(down)
    if up < 1 or down < 1 or math.gcd(up, down) != 1:
        raise ValueError("up / down must be positive and in lowest terms, got %d / %d" % (up, down))
    if zeros < 1 or not 0.0 < rolloff <= 1.0 or beta < 0:
        raise ValueError("zeros >= 1, 0 < rolloff <= 1 and beta >= 0 expected")
    fc = rolloff * min(1.0, up / down)
    W = int(math.ceil(zeros / fc))
    j = np.arange(2 * W, dtype=np.float64)[None, :]
    phase = np.arange(up, dtype=np.float64)[:, None]
    tau = (j - W + 1) - phase / up
    inside = np.abs(tau) < W
    window = np.where(inside, np.i0(beta * np.sqrt(np.clip(1.0 - (tau / W) ** 2, 0.0, None))) / np.i0(beta), 0.0)
    h = fc * np.sinc(fc * tau) * window
    h = h / h.sum(axis=1, keepdims=True)
    return h.astype(np.float32), W


# ---- speed perturbation: host-side arithmetic ---------------------------------------------------------------------------
def parse_speeds(speeds):
    """None, or the sorted distinct integer percents of `speeds`, each in [50, 200]."""
    if speeds is None:
        return None
    out = []
    for p in speeds:
        if isinstance(p, bool) or int(p) != p:
            raise ValueError("speeds are integer percents, got %r" % (p,))
        p = int(p)
        if not PCT_LO <= p <= PCT_HI:
            raise ValueError("speed percent %d outside [%d, %d]" % (p, PCT_LO, PCT_HI))
        out.append(p)
    if not out:
        raise ValueError("speeds is empty: pass None for no speed perturbation")
    return tuple(sorted(set(out)))


def parse_speed_range(text):
    """'LO:HI' -> every integer percent of the range (train.py --speed-perturb)."""
    try:
        lo, hi = (int(v) for v in str(text).split(":"))
    except ValueError:
        raise ValueError("speed range must be LO:HI in integer percents, got %r" % (text,))
    if lo > hi:
        raise ValueError("empty speed range %r" % (text,))
    return parse_speeds(range(lo, hi + 1))


def speed_ratio(pct):
    """(up, down) = 100 / pct in lowest terms: a source replayed at pct % of its speed."""
    pct = int(pct)
    g = math.gcd(100, pct)
    return 100 // g, pct // g


def need(segment_len, pct):
    """ceil(segment_len * pct / 100): the input samples a segment at pct % spans."""
    return (int(segment_len) * int(pct) + 99) // 100


def eligible_len(segment_len, speeds):
    """The utterance length the sampler's tables are built for: need() at the largest percent."""
    return need(segment_len, max(speeds))


def span(up, down, W, chunk=CHUNK):
    """LDS floats of the input span of `chunk` consecutive outputs (ctn_resample_span)."""
    return (up - 1 + (chunk - 1) * down) // up + 2 * W


class SpeedBanks:
    """The filter banks of a set of speed percents in one flat device buffer, with the (up, down, W, offset) table of
    ctn_dynmix_speed_segments (row pct - 50; W = 0: not configured; 100 needs no bank)."""

    def __init__(self, speeds, device):
        self.speeds = parse_speeds(speeds)
        tab = np.zeros((PCT_HI - PCT_LO + 1, 4), dtype=np.int32)
        flat, at, spans, padded = [], 0, [1], []
        for p in self.speeds:
            if p == 100:
                continue
            up, down = speed_ratio(p)
            h, W = _host_filter(up, down)
            tab[p - PCT_LO] = (up, down, W, at)
            flat.append(h.reshape(-1))
            at += h.size
            spans.append(span(up, down, W))
            padded.append(up * (2 * W + 1))
        self.table_host = tab
        self.span_cap = max(spans)
        room = LDS_BYTES // 4 - self.span_cap
        fits = [n for n in padded if n <= room]         # a bank that does not fit beside the span is read through the cache
        self.bank_cap = max(fits) if fits else 0
        banks = np.concatenate(flat) if flat else np.zeros(1, dtype=np.float32)
        self.banks = torch.from_numpy(banks).to(device)
        self.table = torch.from_numpy(tab).to(device)


_HOST_FILTERS, _DEVICE_FILTERS, _SPEED_BANKS = {}, {}, {}


def _host_filter(up, down):
    if (up, down) not in _HOST_FILTERS:
        _HOST_FILTERS[(up, down)] = design_filter(up, down)
    return _HOST_FILTERS[(up, down)]


def device_filter(up, down, device):
    """(h on the device, W), cached per device and ratio."""
    device = torch.device(device)
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device(), up, down)
    if key not in _DEVICE_FILTERS:
        h, W = _host_filter(up, down)
        _DEVICE_FILTERS[key] = (torch.from_numpy(h).to(device), W)
    return _DEVICE_FILTERS[key]


def speed_banks(speeds, device):
    """SpeedBanks, cached per device and set of percents."""
    device = torch.device(device)
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device(), parse_speeds(speeds))
    if key not in _SPEED_BANKS:
        _SPEED_BANKS[key] = SpeedBanks(key[2], device)
    return _SPEED_BANKS[key]


# ---- the device path ----------------------------------------------------------------------------------------------------
def _need_gpu(t, name):
    if not torch.is_tensor(t) or t.device.type != "cuda":
        raise ValueError("%s must be a tensor on the GPU: there is no CPU path" % name)
    if t.dtype != torch.float32:
        raise ValueError("%s must be float32, got %s" % (name, t.dtype))


def resample_rows(x, in_offsets, in_lens, up, down, y, out_offsets):
    """Rows of the flat device buffer x into rows of the flat device buffer y (both float32, contiguous), by up / down in lowest
    terms; the tables are host integer sequences.  -> out_lens (numpy int64).  Raises CtnError on a row outside a buffer."""
    _need_gpu(x, "x")
    _need_gpu(y, "y")
    if y.device != x.device or not x.is_contiguous() or not y.is_contiguous():
        raise ValueError("x and y must be contiguous and on one device")
    in_offsets = np.asarray(in_offsets, dtype=np.int64).reshape(-1)
    in_lens = np.asarray(in_lens, dtype=np.int64).reshape(-1)
    out_offsets = np.asarray(out_offsets, dtype=np.int64).reshape(-1)
    if not (len(in_offsets) == len(in_lens) == len(out_offsets)) or len(in_lens) == 0:
        raise ValueError("row tables of %d, %d and %d entries" % (len(in_offsets), len(in_lens), len(out_offsets)))
    out_lens = (in_lens * up + down - 1) // down
    host = np.ascontiguousarray(np.stack([in_offsets, in_lens, out_offsets, out_lens]))
    dev = torch.from_numpy(host).to(x.device)
    h, W = device_filter(up, down, x.device)
    U = len(in_lens)
    lib.call("ctn_resample_ragged", x.data_ptr(), x.numel(), dev[0].data_ptr(), dev[1].data_ptr(), U, up, down, h.data_ptr(), W,
             y.data_ptr(), y.numel(), dev[2].data_ptr(), dev[3].data_ptr(), host.ctypes.data, 0,
             torch.cuda.current_stream(x.device).cuda_stream)
    return out_lens


def resample_ragged(flat, offsets, lens, orig_sr, new_sr):
    """Rows (offsets, lens: host integer sequences) of the flat float32 GPU tensor `flat` from orig_sr to new_sr.
    -> (flat_out on the same device, the rows back to back; out_offsets, out_lens numpy int64)."""
    _need_gpu(flat, "flat")
    up, down = ratio(orig_sr, new_sr)
    flat = flat.contiguous().reshape(-1)
    lens = np.asarray(lens, dtype=np.int64).reshape(-1)
    offsets = np.asarray(offsets, dtype=np.int64).reshape(-1)
    if len(lens) == 0 or int(lens.min()) < 1:
        raise ValueError("resample_ragged needs at least one row and no empty row")
    if up == down:
        out_offsets = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64)
        if ((offsets < 0) | (offsets + lens > flat.numel())).any():
            raise ValueError("a row lies outside the buffer of %d samples" % flat.numel())
        return torch.cat([flat[int(o):int(o) + int(n)] for o, n in zip(offsets, lens)]), out_offsets, lens.copy()
    out_lens = (lens * up + down - 1) // down
    out_offsets = np.concatenate(([0], np.cumsum(out_lens)[:-1])).astype(np.int64)
    y = torch.empty(int(out_lens.sum()), dtype=torch.float32, device=flat.device)
    resample_rows(flat, offsets, lens, up, down, y, out_offsets)
    return y, out_offsets, out_lens


def resample(x, orig_sr, new_sr):
    """GPU float32 tensor [..., T] at orig_sr -> [..., ceil(T * new_sr / orig_sr)] at new_sr; every row on its own (zeros
    beyond its ends).  Equal rates give a copy."""
    _need_gpu(x, "x")
    up, down = ratio(orig_sr, new_sr)
    if x.dim() < 1 or x.shape[-1] < 1 or x.numel() == 0:
        raise ValueError("resample needs a non-empty last dimension, got shape %s" % (tuple(x.shape),))
    if up == down:
        return x.clone()
    T = int(x.shape[-1])
    rows = x.numel() // T
    flat = x.contiguous().reshape(-1)
    n_out = out_len(T, up, down)
    y = torch.empty(rows * n_out, dtype=torch.float32, device=x.device)
    resample_rows(flat, np.arange(rows, dtype=np.int64) * T, np.full(rows, T, dtype=np.int64), up, down, y,
                  np.arange(rows, dtype=np.int64) * n_out)
    return y.reshape(tuple(x.shape[:-1]) + (n_out,))
