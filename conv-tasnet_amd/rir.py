"""Room impulse responses for the reverberant dynamic mixing (dynmix.DynamicMixLoader(rirs=...), csrc/ctn_dynmix_aug.hip).

    bank = RirBank.from_manifest("rirs.json", 8000, "cuda:0")                      # [[wav_path, n_samples], ...]
    bank = RirBank.from_arrays(synthetic_bank(32, 8000), "cuda:0", early_ms=50.0)  # no RIR data set at hand
    loader = DynamicMixLoader(corpus, 8, 32000, rirs=bank, noise=noise_corpus, snr_db=(-6, 3))
    bank = RirBank.from_rooms(draw_rooms(64, 4, 8000), "cuda:0")                   # simulated shoebox rooms, 4 positions in each
    loader = DynamicMixLoader(corpus, 8, 32000, rirs=bank, same_room=True,         # the talkers of a mixture share a room, and
                              room_schedule=lambda e: draw_rooms(64, 4, 8000, epoch=e))   # every epoch brings new rooms

A bank is R responses of 1 .. 8192 taps (about 1 s at 8 kHz) back to back in one flat float32 device buffer, with three
numbers per response taken on the host in float64 (include/ctn_hip.h has the contract, the tests restate it in numpy):
the direct path `direct[r]` = the first index of max |h|, and `early[r]` = the number of leading taps that make the training
target: the direct path and the reflections of the first `early_ms` behind it (early_ms=None: all of them, the target is the
fully reverberant source; 0: the direct path alone).

normalize=True divides every response by sqrt(sum h^2) before the single rounding to float32, so that the reverberant source
keeps roughly the level the plan gave it.  A deliberate approximation (and one of the RMS: a corpus built with
level="active" sees its active level move with the tail as well): it is exact for a white source only, and the early-taps target lies below that level by the energy of the late taps.
"""
import json

import numpy as np
import torch

from . import data as _data
from ._lib import lib

MAX_TAPS = 8192


def build_tables(arrays, sample_rate=8000, early_ms=50.0, normalize=True):
    """The bank's host tables (pure host function, float64 until the one rounding).
    -> dict(bank float32 [sum n_r], offsets int64 [R], lens, direct, early int32 [R])."""
    if len(arrays) == 0:
        raise ValueError("a RIR bank needs at least one response")
    if int(sample_rate) < 1:
        raise ValueError("sample_rate must be positive, got %r" % (sample_rate,))
    if early_ms is not None and not (np.isfinite(early_ms) and early_ms >= 0):
        raise ValueError("early_ms must be None or a non-negative number of milliseconds, got %r" % (early_ms,))
    extra = None if early_ms is None else int(round(float(early_ms) * int(sample_rate) / 1000.0))
    taps, lens, direct, early = [], [], [], []
    for r, a in enumerate(arrays):
        h = np.asarray(a, dtype=np.float64).reshape(-1)
        n = h.shape[0]
        if n < 1:
            raise ValueError("response %d is empty" % r)
        if n > MAX_TAPS:
            raise ValueError("response %d has %d taps, at most %d are supported (truncate it)" % (r, n, MAX_TAPS))
        if not np.all(np.isfinite(h)):
            raise ValueError("response %d holds values that are not finite" % r)
        if normalize:
            energy = float(np.sum(h * h))
            if not energy > 0:
                raise ValueError("response %d is all zeros and cannot be normalised" % r)
            h = h / np.sqrt(energy)
        d = int(np.argmax(np.abs(h)))                       # the first index of the maximum
        taps.append(h.astype(np.float32))
        lens.append(n)
        direct.append(d)
        early.append(n if extra is None else min(n, d + 1 + extra))
    lens = np.asarray(lens, dtype=np.int32)
    offsets = np.concatenate(([0], np.cumsum(lens.astype(np.int64))[:-1])).astype(np.int64)
    return dict(bank=np.concatenate(taps), offsets=offsets, lens=lens, direct=np.asarray(direct, dtype=np.int32),
                early=np.asarray(early, dtype=np.int32))


def synthetic_bank(n, sample_rate=8000, rt60=(0.2, 0.6), seed=0):
    """n synthetic responses (float64 arrays, pure numpy, a function of the arguments alone): a unit direct-path spike at a
    delay of up to 2 ms, behind it Gaussian noise under the exponential envelope 10^(-3 t / RT60) of an RT60 drawn uniformly
    from `rt60` (seconds), truncated where the envelope reaches -60 dB or at 8192 taps.  The tail starts 12 dB below the
    spike, so the spike is the largest tap."""
    lo, hi = float(rt60[0]), float(rt60[1])
    if n < 1 or not 0 < lo <= hi:
        raise ValueError("synthetic_bank(n=%r, rt60=%r): n >= 1 and 0 < rt60[0] <= rt60[1]" % (n, rt60))
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(int(n)):
        delay = int(rng.randint(0, int(0.002 * sample_rate) + 1))
        t60 = float(rng.uniform(lo, hi))
        tail = min(int(np.ceil(t60 * sample_rate)), MAX_TAPS - delay - 1)
        h = np.zeros(delay + 1 + tail, dtype=np.float64)
        h[delay] = 1.0
        t = np.arange(1, tail + 1, dtype=np.float64) / sample_rate
        h[delay + 1:] = np.clip(0.25 * rng.randn(tail), -0.9, 0.9) * 10.0 ** (-3.0 * t / t60)
        out.append(h)
    return out


# ---- simulated rooms: the shoebox image-source method on the device (csrc/ctn_ism.hip) --------------------------------------
C_SOUND = 343.0             # m/s
MIN_SOURCE_GAP = 0.3        # metres between any two source positions of a room
_ROOM_DOUBLES, _RESP_DOUBLES = 16, 4


def draw_rooms(n_rooms, positions, sample_rate, rt60=(0.2, 0.6), dims=((3, 3, 2.5), (10, 8, 4)), distance=(0.5, 3.0), margin=0.5,
               seed=0, epoch=0):
    """n_rooms shoebox rooms with one microphone and `positions` source positions each (pure numpy, a function of the arguments
    alone): dimensions uniform between dims[0] and dims[1] (metres), the microphone and the sources uniform at least `margin`
    from every wall, every source-microphone distance within `distance` and the sources pairwise at least 0.3 m apart (by
    rejection; a ValueError after 1000 tries for one position).  One absorption coefficient per room from the Eyring formula,
    alpha = 1 - exp(-0.161 V / (S * rt60)) for an rt60 drawn uniformly from `rt60` (seconds), beta = sqrt(1 - alpha) on all six walls.
    rt60 is a DESIGN TARGET, not what the response will measure: the Schroeder T60 of a shoebox image-method response comes out
    longer than the Eyring value it was designed for (DESIGN.md has measured figures), a known property of the method.
    -> dict(L [G,3], mic [G,3], beta [G,6], src [G,P,3], rt60 [G] float64, sample_rate, positions)."""
    G, P = int(n_rooms), int(positions)
    lo, hi = float(rt60[0]), float(rt60[1])
    dlo, dhi = float(distance[0]), float(distance[1])
    d0, d1 = np.asarray(dims[0], np.float64), np.asarray(dims[1], np.float64)
    margin = float(margin)
    if G < 1 or P < 1 or int(sample_rate) < 1:
        raise ValueError("draw_rooms(n_rooms=%r, positions=%r, sample_rate=%r): all at least 1" % (n_rooms, positions, sample_rate))
    if not 0 < lo <= hi or not 1e-3 <= dlo <= dhi or not margin > 0:
        raise ValueError("draw_rooms: 0 < rt60[0] <= rt60[1], 1e-3 <= distance[0] <= distance[1], margin > 0; got %r, %r, %r"
                         % (rt60, distance, margin))
    if d0.shape != (3,) or d1.shape != (3,) or np.any(d0 > d1) or np.any(d0 <= 2 * margin):
        raise ValueError("draw_rooms: dims = (smallest, largest) room, every dimension above twice the margin; got %r" % (dims,))
    if not (0 <= int(seed) < 1 << 48 and 0 <= int(epoch) < 1 << 32):
        raise ValueError("draw_rooms: seed in [0, 2^48) and epoch in [0, 2^32), got %r, %r" % (seed, epoch))
    rng = np.random.RandomState(np.array([int(seed) & 0xffffffff, int(seed) >> 32, int(epoch)], dtype=np.uint32))
    out = dict(L=np.zeros((G, 3)), mic=np.zeros((G, 3)), beta=np.zeros((G, 6)), src=np.zeros((G, P, 3)), rt60=np.zeros(G),
               sample_rate=int(sample_rate), positions=P)
    for g in range(G):
        L = rng.uniform(d0, d1)
        mic = rng.uniform(margin, L - margin)
        t60 = float(rng.uniform(lo, hi))
        for p in range(P):
            for _ in range(1000):
                s = rng.uniform(margin, L - margin)
                dist = np.sqrt(np.sum((s - mic) ** 2))
                if dlo <= dist <= dhi and all(np.sqrt(np.sum((s - o) ** 2)) >= MIN_SOURCE_GAP for o in out["src"][g, :p]):
                    break
            else:
                raise ValueError("draw_rooms: no place for position %d of room %d (%.2f x %.2f x %.2f m) after 1000 tries"
                                 % (p, g, L[0], L[1], L[2]))
            out["src"][g, p] = s
        V, S = L[0] * L[1] * L[2], 2.0 * (L[0] * L[1] + L[1] * L[2] + L[0] * L[2])
        alpha = 1.0 - np.exp(-0.161 * V / (S * t60))
        out["L"][g], out["mic"][g], out["beta"][g], out["rt60"][g] = L, mic, np.sqrt(1.0 - alpha), t60
    return out


def design_fractional_delay(Q=1024, W=8):
    """frac [Q][2W] float64: the Hann-windowed sinc of half-width W taps at the Q delays q / Q of a sample.  With
    tau = (j - W + 1) - q / Q: frac[q][j] = sinc(tau) * 0.5 * (1 + cos(pi tau / W)), 0 where |tau| >= W."""
    Q, W = int(Q), int(W)
    if not (1 <= Q <= 4096 and 1 <= W <= 32):
        raise ValueError("design_fractional_delay(Q=%r, W=%r): 1 <= Q <= 4096, 1 <= W <= 32" % (Q, W))
    tau = (np.arange(2 * W, dtype=np.float64)[None, :] - W + 1) - np.arange(Q, dtype=np.float64)[:, None] / Q
    return np.ascontiguousarray(np.where(np.abs(tau) < W, np.sinc(tau) * 0.5 * (1.0 + np.cos(np.pi * tau / W)), 0.0))


def default_taps(rooms):
    """min(8192, ceil(max rt60 * fs)): the taps that hold the designed decay of every room."""
    return int(min(MAX_TAPS, np.ceil(float(np.max(rooms["rt60"])) * rooms["sample_rate"])))


def ism_tables(rooms, n_taps=None, Q=1024, W=8, c=C_SOUND, frac=None):
    """The simulator's host tables for ctn_ism_simulate (include/ctn_hip.h has the layout), all float64.
    -> dict(tables float64 [ctn_ism_table_doubles], G, R, K, Q, W, n_taps, fs_over_c, four_pi)."""
    L, mic, beta, src = (np.asarray(rooms[k], np.float64) for k in ("L", "mic", "beta", "src"))
    G, P = src.shape[0], src.shape[1]
    fs = int(rooms["sample_rate"])
    n_taps = default_taps(rooms) if n_taps is None else int(n_taps)
    Q, W, c = int(Q), int(W), float(c)
    if L.shape != (G, 3) or mic.shape != (G, 3) or beta.shape != (G, 6) or src.shape != (G, P, 3) or G < 1 or P < 1:
        raise ValueError("rooms: L [G,3], mic [G,3], beta [G,6], src [G,P,3]")
    if not (1 <= n_taps <= MAX_TAPS and c > 0 and np.all(np.isfinite(L)) and np.all(L > 0)):
        raise ValueError("1 <= n_taps <= %d, c > 0 and positive room dimensions; got n_taps = %r, c = %r" % (MAX_TAPS, n_taps, c))
    frac = design_fractional_delay(Q, W) if frac is None else np.ascontiguousarray(frac, dtype=np.float64)
    if frac.shape != (Q, 2 * W):
        raise ValueError("frac must be [Q, 2W] = [%d, %d]" % (Q, 2 * W))
    N = np.array([[int(np.ceil(n_taps / fs * c / (2.0 * float(L[g, a])))) + 1 for a in range(3)] for g in range(G)], dtype=np.int64)
    K = int(N.max()) + 2
    room = np.zeros((G, _ROOM_DOUBLES))
    room[:, 0:3], room[:, 3:6], room[:, 6:12], room[:, 12:15] = L, mic, beta, N
    pw = np.ones((G, 6, K))
    for k in range(1, K):
        pw[:, :, k] = pw[:, :, k - 1] * beta                      # the repeated product, one rounding per power
    resp = np.zeros((G * P, _RESP_DOUBLES))
    resp[:, 0] = np.repeat(np.arange(G), P)
    resp[:, 1:4] = src.reshape(G * P, 3)
    tables = np.ascontiguousarray(np.concatenate([room.reshape(-1), pw.reshape(-1), resp.reshape(-1), frac.reshape(-1)]))
    return dict(tables=tables, G=G, R=G * P, K=K, Q=Q, W=W, n_taps=n_taps, fs_over_c=np.float64(fs) / np.float64(c),
                four_pi=4.0 * np.pi)


def simulate_tables(tb, device, tables_dev=None, out=None, stats=None):
    """ctn_ism_simulate over the tables of ism_tables() -> (h [R, n_taps] float64, status [R] int32) on the device.  tables_dev:
    the device copy (default: uploaded here); out: an h to fill; stats: an int64 [2] device tensor the caller zeroed."""
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("the room simulator runs on the GPU: got device %s" % device)
    host = tb["tables"]
    if host.dtype != np.float64 or not host.flags["C_CONTIGUOUS"] or \
            host.size != lib.ctn_ism_table_doubles(tb["G"], tb["R"], tb["K"], tb["Q"], tb["W"]):
        raise ValueError("tables: %d contiguous float64 values do not fit (G, R, K, Q, W) = %r"
                         % (host.size, (tb["G"], tb["R"], tb["K"], tb["Q"], tb["W"])))
    if tables_dev is None:
        tables_dev = torch.from_numpy(host).to(device)
    h = torch.empty(tb["R"], tb["n_taps"], dtype=torch.float64, device=device) if out is None else out
    if tuple(h.shape) != (tb["R"], tb["n_taps"]) or h.dtype != torch.float64 or not h.is_contiguous() or h.device != device:
        raise ValueError("out must be a contiguous float64 [%d, %d] tensor on %s" % (tb["R"], tb["n_taps"], device))
    status = torch.empty(tb["R"], dtype=torch.int32, device=device)
    lib.call("ctn_ism_simulate", host.ctypes.data, tables_dev.data_ptr(), tb["G"], tb["R"], tb["K"], tb["Q"], tb["W"], tb["n_taps"],
             float(tb["fs_over_c"]), float(tb["four_pi"]), h.data_ptr(), status.data_ptr(), 0 if stats is None else stats.data_ptr(),
             torch.cuda.current_stream(device).cuda_stream)
    return h, status


def simulate(rooms, device, n_taps=None, Q=1024, W=8, c=C_SOUND):
    """The responses of `rooms` (draw_rooms, or a dict of the same arrays) by the image-source method on the device:
    h [G * P, n_taps] float64, response g * P + pos.  n_taps=None: min(8192, ceil(max rt60 * fs))."""
    h, _ = simulate_tables(ism_tables(rooms, n_taps, Q, W, c), device)      # the host checked every row: no status to read back
    return h


class RirBank:
    """R room impulse responses in device memory: bank (flat float32), offsets [R] int64, lens / direct / early [R] int32."""

    positions_per_room = None       # from_rooms: response g * P + pos is position pos of room g
    _ism = None                     # from_rooms: the simulator's arguments, kept for refresh()

    def __init__(self, arrays, device, sample_rate=8000, early_ms=50.0, normalize=True):
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("RirBank lives on the GPU: got device %s" % device)
        self.host = build_tables(arrays, sample_rate, early_ms, normalize)
        self.device, self.sample_rate, self.early_ms, self.normalize = device, int(sample_rate), early_ms, bool(normalize)
        self.bank = torch.from_numpy(self.host["bank"]).to(device)
        self.offsets = torch.from_numpy(self.host["offsets"]).to(device)
        self.lens = torch.from_numpy(self.host["lens"]).to(device)
        self.direct = torch.from_numpy(self.host["direct"]).to(device)
        self.early = torch.from_numpy(self.host["early"]).to(device)

    @classmethod
    def from_arrays(cls, arrays, device, sample_rate=8000, early_ms=50.0, normalize=True):
        return cls(arrays, device, sample_rate, early_ms, normalize)

    @classmethod
    def from_manifest(cls, json_path, sample_rate, device, early_ms=50.0, normalize=True, reader=None):
        """json list of (wav_path, n_samples): every file is read once.  A file at another rate is a ValueError."""
        with open(json_path, "r") as f:
            infos = json.load(f)
        reader = _data.read_wav if reader is None else reader
        arrays = []
        for info in infos:
            path, n = info[0], info[1]
            x = reader(path, sample_rate)
            if x.shape[0] != int(n):
                raise ValueError("%s has %d samples, the manifest says %d" % (path, x.shape[0], int(n)))
            arrays.append(x)
        return cls(arrays, device, sample_rate, early_ms, normalize)

    @classmethod
    def from_rooms(cls, rooms, device, early_ms=50.0, normalize=True, n_taps=None, Q=1024, W=8, c=C_SOUND):
        """Simulated rooms (draw_rooms): the responses are computed on the device (simulate), read back once, and finished by
        build_tables like any other bank.  Records positions_per_room for DynamicMixLoader(same_room=True)."""
        n_taps = default_taps(rooms) if n_taps is None else int(n_taps)
        h = simulate(rooms, device, n_taps, Q, W, c).cpu().numpy()
        self = cls(list(h), device, int(rooms["sample_rate"]), early_ms, normalize)
        self.positions_per_room = int(rooms["positions"])
        self._ism = dict(n_taps=n_taps, Q=int(Q), W=int(W), c=float(c))
        return self

    def refresh(self, rooms):
        """Refill the bank from other rooms of the same count, positions and sample rate, with the taps and the simulator
        arguments of from_rooms: the device tensors are written in place (their data pointers stay), so loaders that hold the bank
        see the new rooms.  Raises before anything is written if `full_targets` would change (a loader has sized its buffers by it)."""
        if self._ism is None:
            raise ValueError("refresh() needs a bank made by RirBank.from_rooms")
        R = self.num_responses
        if int(rooms["positions"]) != self.positions_per_room or len(rooms["L"]) * self.positions_per_room != R or \
                int(rooms["sample_rate"]) != self.sample_rate:
            raise ValueError("refresh(): the bank holds %d responses, %d per room, at %d Hz; the new rooms differ"
                             % (R, self.positions_per_room, self.sample_rate))
        h = simulate(rooms, self.device, **self._ism).cpu().numpy()
        host = build_tables(list(h), self.sample_rate, self.early_ms, self.normalize)
        if bool(np.all(host["early"] == host["lens"])) != self.full_targets:
            raise ValueError("refresh(): full_targets would change (early_ms = %r against %d taps)" % (self.early_ms, self._ism["n_taps"]))
        self.host = host
        for name in ("bank", "offsets", "lens", "direct", "early"):
            getattr(self, name).copy_(torch.from_numpy(host[name]))

    num_responses = property(lambda self: len(self.host["lens"]))
    # True where no response has late taps: the targets are the reverberant sources themselves, no second set of rows
    full_targets = property(lambda self: bool(np.all(self.host["early"] == self.host["lens"])))

    def device_bytes(self):
        return sum(t.numel() * t.element_size() for t in (self.bank, self.offsets, self.lens, self.direct, self.early))
