"""Long-recording separation (csrc/ctn_longform.hip): a meeting or a podcast through a model trained on 4-second segments.

    est = separate_long(model, x, segment=32000)                  # x [T] on the GPU -> [C, T]
    ests = separate_long(model, [x0, x1, x2], 32000, hop=16000)   # a list: their segments share the forward batches

The recording is cut into overlapping segments of the training length, the segments are separated as a batch, every
segment's speakers are brought into the order of its predecessor by comparing the overlaps (PIT leaves the order arbitrary
per segment), and the segments are cross-faded.  Framing, the C * C overlap costs, the chain of permutations and the
assembly are HIP kernels over ragged tables in device memory (include/ctn_hip.h has the contract, the tests
restate it in numpy): the host knows every length and fills the tables itself, so nothing is read back and nothing
synchronises.  Every sum has a stated order with one rounding per operation, so the output is a bitwise function of the
estimates.  There is no CPU path: a CPU tensor raises.

    segs, seg_ptr = frame_ragged(flat, offsets, lens, seg, hop)   # [Nseg, seg], numpy int64 [R + 1]
    outs = stitch_ragged(est, seg_ptr, lens, hop)                 # est [Nseg, C, seg] -> list of [C, T_r]
"""
import math

import numpy as np
import torch

from ._lib import lib

MAX_C = 4
WINDOWS = ("linear", "hann")


def check_geometry(seg, hop):
    """1 <= seg - hop <= hop: never more than two segments over one sample.  -> (seg, hop) as ints."""
    if isinstance(seg, bool) or isinstance(hop, bool) or int(seg) != seg or int(hop) != hop:
        raise ValueError("segment and hop are integer sample counts, got %r and %r" % (seg, hop))
    seg, hop = int(seg), int(hop)
    if hop < 1 or seg - hop < 1:
        raise ValueError("segment (%d) must exceed hop (%d >= 1): the overlap is what the speaker orders are compared on" % (seg, hop))
    if seg > 2 * hop:
        raise ValueError("segment (%d) above 2 * hop (%d): more than two segments over one sample is not supported" % (seg, hop))
    if seg > 1 << 30:
        raise ValueError("segment (%d) above 2^30" % seg)
    return seg, hop


def plan_segments(T, seg, hop):
    """The segments of a recording of T >= 1 samples: 1 if T <= seg, else 1 + ceil((T - seg) / hop)."""
    seg, hop = check_geometry(seg, hop)
    T = int(T)
    if T < 1:
        raise ValueError("a recording needs at least one sample, got %d" % T)
    return 1 if T <= seg else 1 + -((seg - T) // hop)


def fade_tables(ov, window="linear"):
    """(fi, fo) float32 [ov]: the cross-fade weights of an overlap of ov samples, designed in float64 and rounded once.
    'linear': fi = (u + 0.5) / ov; 'hann': fi = sin^2(pi (u + 0.5) / (2 ov)); fo = 1 - fi."""
    ov = int(ov)
    if ov < 1:
        raise ValueError("the overlap must be at least one sample, got %d" % ov)
    if window not in WINDOWS:
        raise ValueError("window must be one of %s, got %r" % (WINDOWS, window))
    u = (np.arange(ov, dtype=np.float64) + 0.5) / ov
    fi = u if window == "linear" else np.sin(0.5 * np.pi * u) ** 2
    return fi.astype(np.float32), (1.0 - fi).astype(np.float32)


def _seg_ptr(lens, seg, hop):
    lens = np.asarray(lens, dtype=np.int64).reshape(-1)
    if len(lens) == 0 or int(lens.min()) < 1:
        raise ValueError("at least one recording and no empty recording expected")
    n = np.where(lens <= seg, 1, 1 + -((seg - lens) // hop)).astype(np.int64)
    return lens, np.concatenate(([0], np.cumsum(n))).astype(np.int64)


def _need_gpu(t, name):
    if not torch.is_tensor(t) or t.device.type != "cuda":
        raise ValueError("%s must be a tensor on the GPU: there is no CPU path" % name)
    if t.dtype != torch.float32:
        raise ValueError("%s must be float32, got %s" % (name, t.dtype))


def _upload(host, device):
    """A host int64 / float32 array to the device through pinned memory: no synchronisation (the pinned block is returned to
    torch's host allocator, which keeps it until the copy has run)."""
    return torch.from_numpy(host).pin_memory().to(device, non_blocking=True)


_FADES = {}


def _device_fades(ov, window, device):
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device(), ov, window)
    if key not in _FADES:
        fi, fo = fade_tables(ov, window)
        _FADES[key] = (_upload(fi, device), _upload(fo, device))
    return _FADES[key]


def _tables(seg_ptr, lens, offsets):
    """seg_ptr [R + 1], T [R], offsets [R] back to back: the host_tables of ctn_longform_frame / _assemble."""
    return np.ascontiguousarray(np.concatenate([seg_ptr, lens, offsets]).astype(np.int64))


def frame_ragged(flat, offsets, lens, seg, hop):
    """Recordings (offsets, lens: host integer sequences) of the flat float32 GPU tensor `flat` cut into segments of `seg` samples
    every `hop`, zeros beyond a recording's end.  -> (segs [Nseg, seg] on the same device, seg_ptr numpy int64 [R + 1])."""
    seg, hop = check_geometry(seg, hop)
    _need_gpu(flat, "flat")
    flat = flat.contiguous().reshape(-1)
    lens, seg_ptr = _seg_ptr(lens, seg, hop)
    offsets = np.asarray(offsets, dtype=np.int64).reshape(-1)
    if len(offsets) != len(lens):
        raise ValueError("tables of %d offsets and %d lengths" % (len(offsets), len(lens)))
    R, Nseg = len(lens), int(seg_ptr[-1])
    host = _tables(seg_ptr, lens, offsets)
    dev = _upload(host, flat.device)
    segs = torch.empty((Nseg, seg), dtype=torch.float32, device=flat.device)
    lib.call("ctn_longform_frame", flat.data_ptr(), flat.numel(), dev.data_ptr(), dev[R + 1:].data_ptr(), dev[2 * R + 1:].data_ptr(), R, Nseg,
             seg, hop, segs.data_ptr(), host.ctypes.data, 0, torch.cuda.current_stream(flat.device).cuda_stream)
    return segs, seg_ptr


def _check_est(est, seg_ptr):
    _need_gpu(est, "est")
    if est.dim() != 3 or not est.is_contiguous():
        raise ValueError("est must be a contiguous [Nseg, C, seg] tensor, got shape %s" % (tuple(est.shape),))
    Nseg, C, seg = (int(v) for v in est.shape)
    if not 2 <= C <= MAX_C:
        raise ValueError("C = %d speakers: the stitch compares all C! orders, 2 <= C <= %d" % (C, MAX_C))
    seg_ptr = np.ascontiguousarray(np.asarray(seg_ptr, dtype=np.int64).reshape(-1))
    if len(seg_ptr) < 2 or int(seg_ptr[0]) != 0 or int(seg_ptr[-1]) != Nseg or (np.diff(seg_ptr) < 1).any():
        raise ValueError("seg_ptr must ascend from 0 to the %d rows of est" % Nseg)
    return Nseg, C, seg, seg_ptr


def segment_costs(est, seg_ptr, hop, _dev_seg_ptr=None):
    """cost [Nseg, C, C] of est [Nseg, C, seg]: cost[s, a, b] = the squared difference between speaker a of the predecessor's last
    seg - hop samples and speaker b of segment s's first ones; rows of first segments are zeros."""
    Nseg, C, seg, seg_ptr = _check_est(est, seg_ptr)
    seg, hop = check_geometry(seg, hop)
    dsp = _upload(seg_ptr, est.device) if _dev_seg_ptr is None else _dev_seg_ptr
    cost = torch.empty((Nseg, C, C), dtype=torch.float32, device=est.device)
    lib.call("ctn_longform_costs", est.data_ptr(), dsp.data_ptr(), len(seg_ptr) - 1, Nseg, C, seg, hop, cost.data_ptr(), seg_ptr.ctypes.data,
             torch.cuda.current_stream(est.device).cuda_stream)
    return cost


def segment_order(cost, seg_ptr, _dev_seg_ptr=None):
    """g [Nseg, C] int32 from cost [Nseg, C, C]: g[s][a] = the local channel of segment s that carries output channel a."""
    Nseg, C, _, seg_ptr = _check_est(cost, seg_ptr)
    dsp = _upload(seg_ptr, cost.device) if _dev_seg_ptr is None else _dev_seg_ptr
    g = torch.empty((Nseg, C), dtype=torch.int32, device=cost.device)
    lib.call("ctn_longform_order", cost.data_ptr(), dsp.data_ptr(), len(seg_ptr) - 1, Nseg, C, g.data_ptr(), seg_ptr.ctypes.data, 0,
             torch.cuda.current_stream(cost.device).cuda_stream)
    return g


def stitch_ragged(est, seg_ptr, lens, hop, window="linear", return_order=False):
    """The estimates est [Nseg, C, seg] of the segments of R recordings (seg_ptr, lens: host integer sequences, as frame_ragged
    gives them) back into recordings: speaker orders chained over the overlaps, overlaps cross-faded with `window`.
    -> a list of [C, T_r] tensors (views of one device buffer); with return_order also g [Nseg, C] int32.
    Three launches, no read-back, no synchronisation."""
    Nseg, C, seg, seg_ptr = _check_est(est, seg_ptr)
    seg, hop = check_geometry(seg, hop)
    lens, want = _seg_ptr(lens, seg, hop)
    if not np.array_equal(want, seg_ptr):
        raise ValueError("seg_ptr does not hold the segment counts of recordings of these lengths at segment %d, hop %d" % (seg, hop))
    R = len(lens)
    rows = (C * lens + 3) // 4 * 4                                   # every recording starts on a 16-byte boundary
    out_off = np.concatenate(([0], np.cumsum(rows)[:-1])).astype(np.int64)
    host = _tables(seg_ptr, lens, out_off)
    dev = _upload(host, est.device)
    fi, fo = _device_fades(seg - hop, window, est.device)
    cost = segment_costs(est, seg_ptr, hop, _dev_seg_ptr=dev)
    g = segment_order(cost, seg_ptr, _dev_seg_ptr=dev)
    out = torch.empty(int(rows.sum()), dtype=torch.float32, device=est.device)
    lib.call("ctn_longform_assemble", est.data_ptr(), g.data_ptr(), dev.data_ptr(), dev[R + 1:].data_ptr(), dev[2 * R + 1:].data_ptr(), R, Nseg,
             C, seg, hop, fi.data_ptr(), fo.data_ptr(), out.data_ptr(), out.numel(), host.ctypes.data, 0,
             torch.cuda.current_stream(est.device).cuda_stream)
    outs = [out[int(o):int(o) + C * int(n)].view(C, int(n)) for o, n in zip(out_off, lens)]
    return (outs, g) if return_order else outs


@torch.no_grad()
def separate_long(model, signals, segment, hop=None, batch_size=8, window="linear"):
    """Separate recordings of any length with a model trained on `segment` samples.

    signals: one [T] float32 GPU tensor or a list of them (-> one [C, T] tensor or a list).  model: a ConvTasNet, or any callable
    [B, segment] -> [B, C, segment].  hop defaults to segment // 2; 1 <= segment - hop <= hop, and with a ConvTasNet both are
    multiples of L / 2, so that a segment's estimate has the segment's length.

    The segments of ALL recordings longer than `segment` fill the forward batches of `batch_size` rows together, in list order;
    their estimates are stitched on the device (stitch_ragged).  A recording with T <= segment is one forward pass over its own
    T samples and comes back as the bits of that pass.  Between the first forward pass and the return there is no device-to-host
    copy and no synchronisation.

    The estimates of all segments stay on the device until the stitch: Nseg * C * segment * 4 bytes, 460 MB for an hour at 8 kHz
    with C = 2 (next to the model's own activations for one batch).  No autograd."""
    hop = int(segment) // 2 if hop is None else hop
    seg, hop = check_geometry(segment, hop)
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError("batch_size must be positive, got %d" % batch_size)
    if window not in WINDOWS:
        raise ValueError("window must be one of %s, got %r" % (WINDOWS, window))
    from .conv_tasnet import ConvTasNet
    if isinstance(model, ConvTasNet):
        if (2 * seg) % model.L or (2 * hop) % model.L:
            raise ValueError("segment (%d) and hop (%d) must be multiples of L / 2 = %g" % (seg, hop, model.L / 2))
        if not 2 <= model.C <= MAX_C:
            raise ValueError("C = %d speakers: the stitch compares all C! orders, 2 <= C <= %d" % (model.C, MAX_C))
    single = torch.is_tensor(signals)
    signals = [signals] if single else list(signals)
    if not signals:
        raise ValueError("no recording given")
    for x in signals:
        _need_gpu(x, "every recording")
        if x.dim() != 1 or x.numel() < 1 or x.device != signals[0].device:
            raise ValueError("every recording must be a non-empty [T] tensor, all on one device")
    lens = [int(x.numel()) for x in signals]
    long_ids = [k for k, n in enumerate(lens) if n > seg]
    outs = [None] * len(signals)
    for k, x in enumerate(signals):
        if lens[k] <= seg:
            y = model(x[None])
            if y.dim() != 3 or y.shape[0] != 1 or y.shape[2] != lens[k]:
                raise ValueError("the model gave shape %s for a [1, %d] input" % (tuple(y.shape), lens[k]))
            outs[k] = y[0]
    if long_ids:
        long_lens = np.array([lens[k] for k in long_ids], dtype=np.int64)
        offsets = np.concatenate(([0], np.cumsum(long_lens)[:-1])).astype(np.int64)
        flat = signals[long_ids[0]].contiguous() if len(long_ids) == 1 else torch.cat([signals[k] for k in long_ids])
        segs, seg_ptr = frame_ragged(flat, offsets, long_lens, seg, hop)
        Nseg, est = segs.shape[0], None
        for b0 in range(0, Nseg, batch_size):
            y = model(segs[b0:b0 + batch_size])
            if y.dim() != 3 or y.shape[0] != min(batch_size, Nseg - b0) or y.shape[2] != seg:
                raise ValueError("the model gave shape %s for a [%d, %d] batch" % (tuple(y.shape), min(batch_size, Nseg - b0), seg))
            if est is None:
                est = torch.empty((Nseg, int(y.shape[1]), seg), dtype=torch.float32, device=segs.device)
            est[b0:b0 + batch_size].copy_(y)
        for k, y in zip(long_ids, stitch_ragged(est, seg_ptr, long_lens, hop, window)):
            outs[k] = y
    return outs[0] if single else outs
