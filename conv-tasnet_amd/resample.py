"""On-device sinc resampling (csrc/ctn_resample.hip): a Kaiser-windowed-sinc polyphase resampler for ragged batches in
device memory -- what `librosa.load(path, sr=sample_rate)` does for the reference's loaders, and the primitive behind the
dynamic mixer's speed perturbation.

    y = resample(x, 16000, 8000)                                              # GPU tensor [..., T] -> [..., ceil(T / 2)]
    flat, offsets, lens = resample_ragged(flat, offsets, lens, 16000, 8000)   # rows of one flat device buffer
    r = StreamResampler(rows, 16000, 8000, max_chunk=160)                     # the same sum push by push, per-row history

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


# ---- streaming: the same sum over signals that arrive push by push ------------------------------------------------------
STAB = 8     # int64 entries per row of a ctn_stream_resample table (CTN_STREAM_RS_TAB): n_old, n_new, t0, n_out, src, dst, parity, spare


def plan_stream_resample(n_old, n_new, up, down, W, final=False):
    """(t0, n_out): the outputs a push of n_new samples emits on a row that holds n_old (pure host arithmetic, no GPU).

    After N samples E(N) = ceil((N - W) * up / down) outputs are computable for N > W and none before: output t reads input
    up to floor(t * down / up) + W.  A push emits [E(n_old), E(n_old + n_new)); with `final` it emits up to
    ceil((n_old + n_new) * up / down), the future reading as zero."""
    n_old, n_new, up, down, W = int(n_old), int(n_new), int(up), int(down), int(W)
    if n_old < 0 or n_new < 0:
        raise ValueError("sample counts must not be negative, got %d and %d" % (n_old, n_new))

    def ready(N):
        return out_len(N - W, up, down) if N > W else 0
    t0, N = ready(n_old), n_old + n_new
    return t0, (out_len(N, up, down) if final else ready(N)) - t0


class StreamResampler:
    """`rows` independent streams through the sinc resampler, push by push (ctn_stream_resample):

        r = StreamResampler(rows, 16000, 8000, max_chunk=160)
        r.open(row)                     # a new stream on `row`: its history is reset on the device
        y, lengths = r.push(chunk, counts)      # chunk [rows, n] on the GPU: row m delivers its first counts[m] samples
        tail = r.close(row)             # what the missing future holds back, with zeros for it; the row is free again
    counts may be any mix of values, 0 included; a count above `max_chunk` is split inside `push`.  y is [rows, max(lengths)]
    with zeros beyond lengths[m]; what lies beyond counts[m] in a chunk row, or in rows that deliver nothing, is never read.  Every
    y[m, :lengths[m]] of a row and its `close()` tail, concatenated, are BITWISE `resample()` of the row's whole signal, whatever
    the cuts and whatever the other rows do.  ``groups=C``: C consecutive rows share one count, `open` / `close` take the group's
    index, counts and lengths have rows / C entries and the tail is [C, n] (the sources of one stream).

    A row keeps its last 2W - 1 samples on the device; the counting is host arithmetic (`plan_stream_resample`) and goes to the
    device as a table through pinned memory: a push reads nothing back and does not synchronise.

    `zeros` sets the algorithmic latency: an output needs W = ceil(zeros / (0.95 * min(1, new_sr / orig_sr))) input samples of
    look-ahead, W / orig_sr seconds, about zeros / (0.95 * min(rate)).  At zeros = 32 that is 4.25 ms each way for 16 kHz <-> 8 kHz
    and 4.23 ms for 48 kHz -> 8 kHz; at zeros = 8 it is 1.06 ms.  The offline `resample()` always uses zeros = 32.
    Equal rates pass the samples through with the same interface.  There is no CPU path.
    """

    def __init__(self, rows, orig_sr, new_sr, max_chunk, zeros=ZEROS, groups=1, device="cuda"):
        rows, groups, max_chunk = int(rows), int(groups), int(max_chunk)
        self.up, self.down = ratio(orig_sr, new_sr)
        if rows < 1 or groups < 1 or rows % groups or max_chunk < 1:
            raise ValueError("rows (%d) must be a positive multiple of groups (%d) and max_chunk (%d) positive" % (rows, groups, max_chunk))
        if isinstance(zeros, bool) or int(zeros) != zeros or zeros < 1:
            raise ValueError("zeros must be a positive integer, got %r" % (zeros,))
        self.rows, self.groups, self.n_groups, self.max_chunk, self.zeros = rows, groups, rows // groups, max_chunk, int(zeros)
        self.identity = self.up == self.down
        self.h_host, self.W = (None, 0) if self.identity else (
            _host_filter(self.up, self.down) if self.zeros == ZEROS else design_filter(self.up, self.down, zeros=self.zeros))
        self.n = [0] * self.n_groups            # samples received per group
        self.parity = [0] * self.n_groups
        self.is_open = [False] * self.n_groups
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("StreamResampler needs a GPU device: there is no CPU path")
        self.tab = None                         # device state is allocated at the first use: the checks above need no GPU

    def _alloc(self):
        if self.tab is not None:
            return
        dev, rows = self.device, self.rows
        if not self.identity:
            self.h = device_filter(self.up, self.down, dev)[0] if self.zeros == ZEROS else torch.from_numpy(self.h_host).to(dev)
            self.hist = torch.zeros((2, rows, 2 * self.W - 1), dtype=torch.float32, device=dev)
        self.tab = torch.zeros((rows, STAB), dtype=torch.int64, device=dev)
        self._none = torch.zeros(1, dtype=torch.float32, device=dev)         # stands in for an empty chunk or output
        # pinned staging for the table upload: a ring, each entry with the event of its last copy (FusedStreamPool._upload)
        self._stage = [[torch.zeros((rows, STAB), dtype=torch.int64).pin_memory(), None] for _ in range(4)]
        self._stage_i = 0

    # ---- host bookkeeping ----
    def _group(self, g):
        g = int(g)
        if not 0 <= g < self.n_groups:
            raise ValueError("row %d is outside 0..%d" % (g, self.n_groups - 1))
        return g

    def open(self, row):
        """A new stream on `row` (a group's index with groups > 1): counters and device history back to the start."""
        g = self._group(row)
        if self.is_open[g]:
            raise ValueError("row %d is already open" % g)
        if not self.identity and self.tab is not None:      # (a fresh allocation is zero already)
            self.hist[:, g * self.groups:(g + 1) * self.groups].zero_()
        self.n[g], self.parity[g], self.is_open[g] = 0, 0, True
        return g

    def out_total(self, n_in):
        """ceil(n_in * up / down): the outputs of a whole stream of n_in samples."""
        return out_len(n_in, self.up, self.down)

    def _check_counts(self, counts):
        counts = [int(c) for c in counts]
        if len(counts) != self.n_groups:
            raise ValueError("counts must have one entry per row (%d), got %d" % (self.n_groups, len(counts)))
        for g, c in enumerate(counts):
            if c < 0:
                raise ValueError("counts[%d] is negative" % g)
            if c and not self.is_open[g]:
                raise ValueError("row %d is not open but counts[%d] = %d" % (g, g, c))
        return counts

    def _ready(self, N):
        """E(N) for an int64 array: the outputs computable after N samples."""
        return np.where(N > self.W, -((-(N - self.W) * self.up) // self.down), 0)

    def _ends(self, N, flush):
        """The outputs a row has emitted once it holds N samples (`flush`: and was closed)."""
        if self.identity:
            return N
        return np.where(flush, (N * self.up + self.down - 1) // self.down, self._ready(N))

    def _final_mask(self, final):
        mask = np.zeros(self.n_groups, dtype=bool)
        for g in final:
            mask[self._group(g)] = True
        return mask

    def plan(self, counts, final=()):
        """The outputs every group emits for `counts` new samples (groups in `final` are flushed): host arithmetic only."""
        n = np.asarray(self.n, dtype=np.int64)
        none = np.zeros(self.n_groups, dtype=bool)
        return (self._ends(n + np.asarray(counts, dtype=np.int64), self._final_mask(final)) - self._ends(n, none)).tolist()

    def _upload(self, table):
        buf = self._stage[self._stage_i]
        self._stage_i = (self._stage_i + 1) % len(self._stage)
        if buf[1] is not None:
            buf[1].synchronize()                 # its previous copy has completed (long ago, as a rule)
        else:
            buf[1] = torch.cuda.Event()
        buf[0].copy_(torch.from_numpy(table))
        self.tab.copy_(buf[0], non_blocking=True)
        buf[1].record()
        return buf[0]

    # ---- the device path ----
    def run(self, chunk, counts, y, yld, yoff, final=(), spare=None):
        """`counts[g]` new samples per group from the rows of `chunk` [rows, n]; group g's outputs go to y[row, yoff[g] ..] of the
        float32 device tensor y whose rows are yld samples apart.  Groups in `final` are flushed as well and start afresh at their
        next `open`.  spare[g] goes into the table's spare entry.  -> the outputs written per group.  (The building block of
        `push` / `close`, and of ResamplingStreamPool, which lets the rows land behind its carried remainders.)"""
        counts, C, dev = self._check_counts(counts), self.groups, self.device
        for g in final:
            if not self.is_open[self._group(g)]:
                raise ValueError("row %r is not open" % (g,))
        lengths = self.plan(counts, final)
        n_cols = int(chunk.shape[1]) if chunk is not None else 0
        if max(counts) > n_cols:
            raise ValueError("chunk rows hold %d samples, counts ask for %d" % (n_cols, max(counts)))
        for g, n in enumerate(lengths):
            if n and yoff[g] + n > yld:
                raise ValueError("row %d: %d outputs at offset %d do not fit rows of %d" % (g, n, yoff[g], yld))
        if max(counts) > 0:
            _need_gpu(chunk, "chunk")
        self._alloc()
        if max(counts) > 0:
            if chunk.dim() != 2 or chunk.shape[0] != self.rows or chunk.device != dev:
                raise ValueError("chunk must be [%d, n] on %s" % (self.rows, dev))
            if self.identity or chunk.stride(1) != 1 or (self.rows > 1 and chunk.stride(0) < n_cols):
                chunk = chunk.contiguous()
            cld = chunk.stride(0) if self.rows > 1 else n_cols       # rows of a wider tensor are read in place
            extent = (self.rows - 1) * cld + n_cols
        else:
            chunk, cld, extent = self._none, 0, 1
        G = self.n_groups
        n, par, want = np.asarray(self.n, dtype=np.int64), np.asarray(self.parity, dtype=np.int64), np.asarray(counts, dtype=np.int64)
        flush, none = self._final_mask(final), np.zeros(G, dtype=bool)
        done, written = np.zeros(G, dtype=np.int64), np.zeros(G, dtype=np.int64)
        yoff = np.asarray(yoff, dtype=np.int64)
        row = np.arange(self.rows, dtype=np.int64)
        table = np.zeros((self.rows, STAB), dtype=np.int64)
        while True:
            k = np.minimum(want - done, self.max_chunk)
            last = bool((want - done <= self.max_chunk).all())
            t0 = self._ends(n, none)
            n_out = self._ends(n + k, flush if last else none) - t0
            busy = bool(k.any() or n_out.any())
            per_group = np.stack([n, k, t0, n_out, done, yoff + written, par, np.zeros(G, dtype=np.int64) if spare is None
                                  else np.asarray(spare, dtype=np.int64)], axis=1)
            table[:] = np.repeat(per_group, C, axis=0) if C > 1 else per_group
            table[:, 4] += row * cld
            table[:, 5] += row * yld
            n, done, written = n + k, done + k, written + n_out
            if not self.identity:
                par = par ^ (k > 0)
            if busy or spare is not None:
                host = self._upload(table)
            if busy and self.identity:
                self._copy_through(chunk, n_cols, y, yld)
            elif busy:
                lib.call("ctn_stream_resample", chunk.data_ptr(), extent, self.hist.data_ptr(), self.rows, self.up, self.down,
                         self.h.data_ptr(), self.W, y.data_ptr(), y.numel(), self.tab.data_ptr(), host.data_ptr(), 0,
                         torch.cuda.current_stream(dev).cuda_stream)
            if last:
                break
        self.n, self.parity, written = n.tolist(), par.tolist(), written.tolist()
        assert written == lengths
        for g in final:
            self.is_open[g] = False
        return lengths

    def _copy_through(self, chunk, n_cols, y, yld):
        """Equal rates: y[dst + k] = chunk[src + k], k < n_new, by the table on the device (no per-row launch)."""
        flat = y.view(-1)[: self.rows * yld].view(self.rows, yld)
        k = torch.arange(self.rows * yld, device=self.device).view(self.rows, yld) - self.tab[:, 5:6]
        live = (k >= 0) & (k < self.tab[:, 1:2])
        src = (self.tab[:, 4:5] + k).clamp_(0, max(chunk.numel() - 1, 0))
        flat.copy_(torch.where(live, chunk.view(-1)[src], flat))

    @torch.no_grad()
    def push(self, chunk, counts):
        counts = self._check_counts(counts)
        _need_gpu(chunk, "chunk")
        self._alloc()
        lengths = self.plan(counts)
        width = max(lengths)
        y = torch.zeros((self.rows, width), dtype=torch.float32, device=self.device)
        self.run(chunk, counts, y if width else self._none, width, [0] * self.n_groups)
        return y, lengths

    @torch.no_grad()
    def close(self, row):
        """The row's last outputs (zeros for the future they would need): [n], or [C, n] with groups = C.  The row is free again."""
        g = self._group(row)
        if not self.is_open[g]:
            raise ValueError("row %d is not open" % g)
        counts = [0] * self.n_groups
        width = self.plan(counts, (g,))[g]
        self._alloc()
        y = torch.zeros((self.rows, width), dtype=torch.float32, device=self.device)
        self.run(None, counts, y if width else self._none, width, [0] * self.n_groups, final=(g,))
        tail = y[g * self.groups:(g + 1) * self.groups]
        return tail[0] if self.groups == 1 else tail
