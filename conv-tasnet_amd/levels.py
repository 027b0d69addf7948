"""ITU-T P.56 active speech level (method B) of ragged utterances on the device (csrc/ctn_levels.hip).

    out = active_level_ragged(flat, offsets, lens, 8000)        # flat: float32 device tensor, utterances anywhere in it
    out["level"], out["level_db"], out["long_term"], out["activity"]

The active level is the energy of the band-limited signal divided by the time speech is active: the 0-dB reference the
wsj0-2mix recipe normalises every source to before its +-q dB weights (tools/matlab-code/create_wav_2speakers.m:89-97,
`activlev(s, fs, 'n')`).  The computation is the default mode of that meter, restated in include/ctn_hip.h ("active speech
level") and in numpy under tests/: 0.35 s of appended zeros, a 200 Hz 5th-order Chebyshev-II high-pass (and its
5.5 kHz low-pass mirror from 12.1 kHz up), a 30 ms double-pole envelope, octave bins of the squared envelope held for 0.2 s, and
the level at which the active-level curve crosses the 15.9 dB margin above the bin edges.

The device produces the integer and fixed-order part, (ssq, ns, emax, counts[20]) per utterance, as a bitwise function of the
utterance's own samples, the rate and the chunk length; `level_from_counts` finishes on the host in fp64.
There is no CPU fallback.
"""
import math

import numpy as np
import torch

from ._lib import lib

NBIN = 20               # octave bins of the squared envelope: 60 dB at 3 dB per bin
MARGIN_DB = 15.9        # P.56: the threshold lies this far below the active level
EMPTY = -32768          # the exponent of an envelope sample whose square is zero (stands for -inf)
TABLE_DOUBLES = 131     # the table ctn_active_level reads (include/ctn_hip.h has the layout)
MAX_CHUNKS = (1 << 24) - 1      # chunks per ctn_active_level call

# 5th-order Chebyshev-II high-pass in the s-plane, 50 dB stop band, -0.25 dB at w = 1:
# scipy.signal.cheby2(5, 50, W0, 'high', analog=True) (tests/test_levels_cpu.py re-derives these)
W0 = 0.39790951457558527
PROTO_ZEROS = (0.0, 0.3784344367329518j, 0.2338853444143859j)                # the real zero, then one of each conjugate pair
PROTO_POLES = (-0.6679326883376755, -0.20640255179488695 + 0.739421859068245j, -0.5403688959637246 + 0.45698784092881006j)


def _band_step(sec, x, z):
    """One sample through the band filter, every section direct form II transposed, every product and sum rounded once.
    x: scalar or array; z: list of the 5 (10 with the low-pass) state values or arrays.  -> (y, new z)"""
    b0, b1, a1 = sec["hp1"]
    y = b0 * x + z[0]
    nz = [b1 * x - a1 * y]
    for name, k in (("bq1", 1), ("bq2", 3)):
        b0, b1, b2, a1, a2 = sec[name]
        u = y
        y = b0 * u + z[k]
        nz.append((b1 * u + z[k + 1]) - a1 * y)
        nz.append(b2 * u - a2 * y)
    if sec["lp"] is not None:
        c = sec["lp"]                               # b0 .. b5, a1 .. a5
        u = y
        y = c[0] * u + z[5]
        for k in range(1, 5):
            nz.append((c[k] * u + z[5 + k]) - c[5 + k] * y)
        nz.append(c[5] * u - c[10] * y)
    return y, nz


def _env_step(env, x, z):
    """One sample through the envelope's double pole (numerator b0 only).  -> (s, new z)"""
    b0, a1, a2 = env
    s = b0 * x + z[0]
    return s, [z[1] - a1 * s, -(a2 * s)]


def _transition(step, nstate, chunk):
    """T = A^chunk of a filter: column k is the state `chunk` zero-input samples after the unit state e_k."""
    z = [np.array([1.0 if r == k else 0.0 for k in range(nstate)]) for r in range(nstate)]
    zero = np.zeros(nstate)
    for _ in range(chunk):
        _, z = step(zero, z)
    return np.stack(z)


def design(sample_rate, chunk=None):
    """The fp64 tables of the meter at one rate: dict(sample_rate, chunk, nz, nh, use_lp, sections = dict(hp1 [b0,b1,a1],
    bq1 / bq2 [b0,b1,b2,a1,a2], lp [b0..b5, a1..a5] or None, env [b0,a1,a2]), t_band [S,S] with S = 5 or 10, t_env [2,2],
    table [131] = what ctn_active_level reads)."""
    fs = int(sample_rate)
    if not 8000 <= fs <= 48000:
        raise ValueError("the active-level meter takes 8000 <= sample_rate <= 48000, got %r" % (sample_rate,))
    chunk = int(lib.ctn_active_level_chunk()) if chunk is None else int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be positive, got %d" % chunk)
    zeros, poles = np.array(PROTO_ZEROS, dtype=np.complex128), np.array(PROTO_POLES, dtype=np.complex128)
    t = math.tan(math.pi * 200.0 / fs)
    zz, zp = 2.0 / (1.0 - zeros * t) - 1.0, 2.0 / (1.0 - poles * t) - 1.0
    hp1 = [1.0, -zz[0].real, -zp[0].real]
    bq = [[1.0, -2.0 * zz[k].real, abs(zz[k]) ** 2, -2.0 * zp[k].real, abs(zp[k]) ** 2] for k in (1, 2)]
    # gain at Nyquist (z = -1) of the three sections; the first numerator takes its inverse
    num = (1.0 - hp1[1]) * (1.0 - bq[0][1] + bq[0][2]) * (1.0 - bq[1][1] + bq[1][2])
    den = (1.0 - hp1[2]) * (1.0 - bq[0][3] + bq[0][4]) * (1.0 - bq[1][3] + bq[1][4])
    hp1[0], hp1[1] = hp1[0] * den / num, hp1[1] * den / num
    use_lp = fs >= 2.2 * 5500
    lp = None
    if use_lp:
        tl = math.tan(math.pi * 5500.0 / fs)
        full = lambda r: np.concatenate(([r[0]], r[1:], np.conj(r[1:])))
        ah = np.real(np.poly(2.0 / (full(poles) / tl - 1.0) + 1.0))
        bh = np.real(np.poly(2.0 / (full(zeros) / tl - 1.0) + 1.0))
        bh = bh * ah.sum() / bh.sum()
        lp = np.concatenate((bh, ah[1:]))
    g = math.exp(-1.0 / (0.03 * fs))
    sec = dict(hp1=np.array(hp1), bq1=np.array(bq[0]), bq2=np.array(bq[1]), lp=lp, env=np.array([(1.0 - g) ** 2, -2.0 * g, g * g]))
    nstate = 10 if use_lp else 5
    t_band = _transition(lambda x, z: _band_step(sec, x, z), nstate, chunk)
    t_env = _transition(lambda x, z: _env_step(sec["env"], x, z), 2, chunk)
    table = np.zeros(TABLE_DOUBLES)
    table[0:3], table[3:8], table[8:13], table[24:27] = sec["hp1"], sec["bq1"], sec["bq2"], sec["env"]
    if use_lp:
        table[13:24] = lp
    table[27:27 + nstate * nstate] = t_band.reshape(-1)
    table[127:131] = t_env.reshape(-1)
    return dict(sample_rate=fs, chunk=chunk, nz=int(math.ceil(0.35 * fs)), nh=int(math.ceil(0.2 * fs)) + 1, use_lp=bool(use_lp),
                sections=sec, t_band=t_band, t_env=t_env, table=table)


def level_from_counts(ssq, ns, emax, counts):
    """The level from the device's statistics, in fp64 on the host: ssq [U] the energy of the filtered signal, ns [U] its
    samples, emax [U] one above the largest held exponent, counts [U, 20] the samples per bin (bin j = min(emax - h, 20)).
    -> dict(level (power), level_db, long_term (power), activity); silence (ssq == 0) gives level 0, -inf dB, activity 0."""
    ssq = np.atleast_1d(np.asarray(ssq, dtype=np.float64))
    ns = np.atleast_1d(np.asarray(ns, dtype=np.float64))
    emax = np.atleast_1d(np.asarray(emax, dtype=np.float64))
    kc = np.cumsum(np.asarray(counts, dtype=np.float64).reshape(len(ssq), NBIN), axis=1)
    live = (ssq > 0) & (ns > 0) & (emax > EMPTY + 1)
    rows = np.arange(len(ssq))
    with np.errstate(divide="ignore", invalid="ignore"):
        aj = 10.0 * np.log10(ssq[:, None] / kc)
        cj = 10.0 * math.log10(2.0) * (emax[:, None] - np.arange(1, NBIN + 1)[None, :] - 1.0)      # lower edge of bin j in dB
        mj = aj - cj - MARGIN_DB
        cross = (mj[:, :-1] < 0) & (mj[:, 1:] >= 0)
        has = cross.any(axis=1)
        below = mj[:, -1] <= 0                      # never crossing: all below -> bottom of the last bin; all above -> top bin
        jj = np.where(has, np.argmax(cross, axis=1), np.where(below, NBIN - 2, 0))
        jf = np.where(has, 1.0 / (1.0 - mj[rows, jj + 1] / mj[rows, jj]), np.where(below, 1.0, 0.0))
        step = np.where(jf == 0.0, 0.0, jf * (aj[rows, jj + 1] - aj[rows, jj]))
        lev = aj[rows, jj] + step
        lp = np.where(live, 10.0 ** (lev / 10.0), 0.0)
        level_db = np.where(live, lev, -np.inf)
        long_term = np.where(ns > 0, ssq / ns, 0.0)
        activity = np.where(live, ssq / (ns * lp), 0.0)
    return dict(level=lp, level_db=level_db, long_term=long_term, activity=activity)


_DESIGNS = {}


def _device_design(sample_rate, device):
    key = (int(sample_rate), str(device))
    if key not in _DESIGNS:
        d = design(sample_rate)
        _DESIGNS[key] = (d, torch.from_numpy(d["table"]).to(device))
    return _DESIGNS[key]


def _groups(nchunks, workspace_bytes):
    """Consecutive utterances per launch group: as many as the workspace bound (and the call's chunk limit) holds, at least one."""
    out, first, used = [], 0, 0
    for u, n in enumerate(nchunks):
        need = int(lib.ctn_active_level_workspace(used + int(n), u + 1 - first))
        if u > first and (need > workspace_bytes or used + int(n) > MAX_CHUNKS):
            out.append((first, u))
            first, used = u, 0
        used += int(n)
    out.append((first, len(nchunks)))
    return out


def active_level_ragged(flat, offsets, lens, sample_rate, workspace_bytes=256 << 20):
    """flat: contiguous float32 device tensor; offsets, lens: [U] int64 (host), utterance u is flat[offsets[u] : offsets[u] + lens[u]].
    Utterances are processed in groups sized to `workspace_bytes` (one utterance always fits: the bound then grows to it); the
    grouping does not change a bit of the result.  -> dict of numpy arrays [U]: level (power), level_db, long_term, activity,
    and the device's statistics ssq, ns (-1: an entry outside `flat`, never read; its levels are 0), emax, counts [U, 20]."""
    if flat.device.type != "cuda" or flat.dtype != torch.float32 or not flat.is_contiguous() or flat.dim() != 1 or flat.numel() < 1:
        raise ValueError("flat must be a contiguous 1-d float32 tensor on the GPU")
    offsets = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).reshape(-1))
    lens = np.ascontiguousarray(np.asarray(lens, dtype=np.int64).reshape(-1))
    if len(offsets) != len(lens) or len(lens) == 0:
        raise ValueError("%d offsets with %d lengths" % (len(offsets), len(lens)))
    dev = flat.device
    d, table = _device_design(sample_rate, dev)
    ch, nz, U = d["chunk"], d["nz"], len(lens)
    nchunks = (np.maximum(lens, 0) + nz + ch - 1) // ch
    groups = _groups(nchunks, int(workspace_bytes))
    chunk_ptr = np.concatenate([np.concatenate(([0], np.cumsum(nchunks[a:b]))) for a, b in groups]).astype(np.int64)
    off_d, len_d, cp_d = (torch.from_numpy(a).to(dev) for a in (offsets, lens, chunk_ptr))
    ssq = torch.zeros(U, dtype=torch.float64, device=dev)
    ns = torch.zeros(U, dtype=torch.int64, device=dev)
    emax = torch.zeros(U, dtype=torch.int32, device=dev)
    counts = torch.zeros(U, NBIN, dtype=torch.int64, device=dev)
    ws_bytes = max(int(lib.ctn_active_level_workspace(int(nchunks[a:b].sum()), b - a)) for a, b in groups)
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    at = 0
    for a, b in groups:
        lib.call("ctn_active_level", flat.data_ptr(), flat.numel(), off_d[a:].data_ptr(), len_d[a:].data_ptr(), cp_d[at:].data_ptr(),
                 b - a, int(nchunks[a:b].sum()), table.data_ptr(), int(d["use_lp"]), nz, d["nh"], ssq[a:].data_ptr(), ns[a:].data_ptr(),
                 emax[a:].data_ptr(), counts[a:].data_ptr(), ws.data_ptr(), ws.numel(), stream)
        at += b - a + 1
    stats = dict(ssq=ssq.cpu().numpy(), ns=ns.cpu().numpy(), emax=emax.cpu().numpy(), counts=counts.cpu().numpy())
    out = level_from_counts(stats["ssq"], np.maximum(stats["ns"], 0), stats["emax"], stats["counts"])
    out.update(stats)
    return out


def active_level(x, lengths, sample_rate):
    """Padded batches on the device: x [R, T] float32, lengths [R] (the first lengths[r] samples of row r count).
    -> the dict of active_level_ragged."""
    if x.dim() != 2:
        raise ValueError("x must be [R, T], got %s" % (tuple(x.shape),))
    R, T = x.shape
    lens = np.asarray(lengths.cpu() if torch.is_tensor(lengths) else lengths, dtype=np.int64).reshape(-1)
    if len(lens) != R or (R and (int(lens.min()) < 0 or int(lens.max()) > T)):
        raise ValueError("lengths must hold %d values in [0, %d]" % (R, T))
    return active_level_ragged(x.contiguous().reshape(-1), np.arange(R, dtype=np.int64) * T, lens, sample_rate)
