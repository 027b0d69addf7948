"""ITU-R BS.1770-4 integrated loudness (mono) of ragged utterances on the device (csrc/ctn_loudness.hip).

    out = integrated_loudness_ragged(flat, offsets, lens, 16000)    # flat: float32 device tensor, utterances anywhere in it
    out["lufs"], out["power"], out["ungated"], out["n_blocks"], out["n_abs"], out["n_rel"]

The level the LibriMix recipe (Cosentino et al. 2020) brings every source and noise file to before it mixes them: the mean power
of the K-weighted signal over 400 ms blocks at 75 % overlap, of the blocks that pass the absolute gate (-70 LUFS) and the
relative gate (10 LU below the mean of the absolute-gated blocks).  The computation is restated in include/ctn_hip.h
("integrated loudness") and in numpy under tests/: two biquads (a high shelf and a high-pass, designed for any rate from the
analog prototype by the bilinear transform), blocks of exactly 4 h samples every h = fs / 10, both gates as strict comparisons of
powers.  Nothing is appended, a trailing partial block is dropped.

The device produces the block counts and the three gated sums per utterance as a bitwise function of the utterance's own samples,
the rate and the chunk length; `loudness_from_stats` finishes on the host in fp64.  There is no CPU fallback.
"""
import math

import numpy as np
import torch

from ._lib import lib

TABLE_DOUBLES = 27              # the table ctn_loudness reads (include/ctn_hip.h has the layout)
MAX_CHUNKS = (1 << 31) - 65     # chunks per ctn_loudness call
ABS_GATE_LUFS = -70.0
OFFSET_DB = -0.691              # lufs = OFFSET_DB + 10 log10(power)
REL_GATE = 10.0                 # the relative gate lies 10 LU below the absolute-gated mean: its power over 10.0

# the analog prototypes of the K-weighting (at 48 kHz they give the Recommendation's table to 9e-16)
SHELF_F0, SHELF_GAIN_DB, SHELF_Q, SHELF_VB_EXP = 1681.974450955533, 3.999843853973347, 0.7071752369554196, 0.4996667741545416
HP_F0, HP_Q = 38.13547087602444, 0.5003270373238773


def _biquad_step(c, v, z):
    """One sample through a biquad [b0, b1, b2, a1, a2], direct form II transposed, every product and sum rounded once."""
    y = c[0] * v + z[0]
    return y, [(c[1] * v + z[1]) - c[3] * y, c[2] * v - c[4] * y]


def _k_step(shelf, hp, x, z):
    y, za = _biquad_step(shelf, x, z[0:2])
    y, zb = _biquad_step(hp, y, z[2:4])
    return y, za + zb


def _check_rate(sample_rate):
    fs = int(sample_rate)
    if fs != sample_rate or not 8000 <= fs <= 48000 or fs % 10:
        raise ValueError("the loudness meter takes 8000 <= sample_rate <= 48000 with sample_rate %% 10 == 0 (the 100 ms hop is a "
                         "whole number of samples), got %r" % (sample_rate,))
    return fs


def design(sample_rate, chunk=None):
    """The fp64 tables of the meter at one rate: dict(sample_rate, chunk, hop = fs / 10, block = 4 hop, shelf / hp
    [b0, b1, b2, a1, a2], t [4,4] = A^chunk, abs_gate (a power), table [27] = what ctn_loudness reads)."""
    fs = _check_rate(sample_rate)
    chunk = int(lib.ctn_loudness_chunk()) if chunk is None else int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be positive, got %d" % chunk)
    K = math.tan(math.pi * SHELF_F0 / fs)
    Vh = 10.0 ** (SHELF_GAIN_DB / 20.0)
    Vb = Vh ** SHELF_VB_EXP
    a0 = 1.0 + K / SHELF_Q + K * K
    shelf = np.array([(Vh + Vb * K / SHELF_Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / SHELF_Q + K * K) / a0,
                      2.0 * (K * K - 1.0) / a0, (1.0 - K / SHELF_Q + K * K) / a0])
    K = math.tan(math.pi * HP_F0 / fs)
    a0 = 1.0 + K / HP_Q + K * K
    hp = np.array([1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / HP_Q + K * K) / a0])
    z = [np.array([1.0 if r == k else 0.0 for k in range(4)]) for r in range(4)]       # column k: the state after the unit state e_k
    zero = np.zeros(4)
    for _ in range(chunk):
        _, z = _k_step(shelf, hp, zero, z)
    t = np.stack(z)
    abs_gate = 10.0 ** ((ABS_GATE_LUFS - OFFSET_DB) / 10.0)
    table = np.zeros(TABLE_DOUBLES)
    table[0:5], table[5:10], table[10:26], table[26] = shelf, hp, t.reshape(-1), abs_gate
    return dict(sample_rate=fs, chunk=chunk, hop=fs // 10, block=4 * (fs // 10), shelf=shelf, hp=hp, t=t, abs_gate=abs_gate, table=table)


def loudness_from_stats(n_blocks, n_abs, n_rel, sum_all, sum_abs, sum_rel):
    """The loudness from the device's statistics, in fp64 on the host.  -> dict(power = sum_rel / n_rel (the gated K-weighted
    power), lufs = -0.691 + 10 log10(power), ungated (lufs of sum_all / n_blocks), n_blocks, n_abs, n_rel); an utterance without a
    complete block, or without a block above the gates, has power 0 and lufs -inf."""
    n_blocks, n_abs, n_rel = (np.atleast_1d(np.asarray(a, dtype=np.int64)) for a in (n_blocks, n_abs, n_rel))
    sum_all, sum_rel = (np.atleast_1d(np.asarray(a, dtype=np.float64)) for a in (sum_all, sum_rel))
    power, mean_all = np.zeros(len(n_rel)), np.zeros(len(n_rel))
    power[n_rel > 0] = sum_rel[n_rel > 0] / n_rel[n_rel > 0]
    mean_all[n_blocks > 0] = sum_all[n_blocks > 0] / n_blocks[n_blocks > 0]
    with np.errstate(divide="ignore"):
        lufs = np.where(power > 0, OFFSET_DB + 10.0 * np.log10(power), -np.inf)
        ungated = np.where(mean_all > 0, OFFSET_DB + 10.0 * np.log10(mean_all), -np.inf)
    power[~(power > 0)] = 0.0
    return dict(power=power, lufs=lufs, ungated=ungated, n_blocks=n_blocks, n_abs=n_abs, n_rel=n_rel)


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
        need = int(lib.ctn_loudness_workspace(used + int(n), u + 1 - first))
        if u > first and (need > workspace_bytes or used + int(n) > MAX_CHUNKS):
            out.append((first, u))
            first, used = u, 0
        used += int(n)
    out.append((first, len(nchunks)))
    return out


def integrated_loudness_ragged(flat, offsets, lens, sample_rate, workspace_bytes=256 << 20):
    """flat: contiguous float32 device tensor; offsets, lens: [U] int64 (host), utterance u is flat[offsets[u] : offsets[u] + lens[u]].
    Utterances are processed in groups sized to `workspace_bytes` (one utterance always fits: the bound then grows to it); the
    grouping does not change a bit of the result.  -> dict of numpy arrays [U]: power, lufs, ungated, and the device's statistics
    ns (the samples; -1: an entry outside `flat`, never read; its power is 0), n_blocks, n_abs, n_rel, sum_all, sum_abs, sum_rel."""
    if flat.device.type != "cuda" or flat.dtype != torch.float32 or not flat.is_contiguous() or flat.dim() != 1 or flat.numel() < 1:
        raise ValueError("flat must be a contiguous 1-d float32 tensor on the GPU")
    offsets = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).reshape(-1))
    lens = np.ascontiguousarray(np.asarray(lens, dtype=np.int64).reshape(-1))
    if len(offsets) != len(lens) or len(lens) == 0:
        raise ValueError("%d offsets with %d lengths" % (len(offsets), len(lens)))
    dev = flat.device
    d, table = _device_design(sample_rate, dev)
    ch, U = d["chunk"], len(lens)
    nchunks = (np.maximum(lens, 0) + ch - 1) // ch
    groups = _groups(nchunks, int(workspace_bytes))
    chunk_ptr = np.concatenate([np.concatenate(([0], np.cumsum(nchunks[a:b]))) for a, b in groups]).astype(np.int64)
    off_d, len_d, cp_d = (torch.from_numpy(a).to(dev) for a in (offsets, lens, chunk_ptr))
    counts = torch.zeros(4, U, dtype=torch.int64, device=dev)           # ns, n_blocks, n_abs, n_rel
    sums = torch.zeros(3, U, dtype=torch.float64, device=dev)           # sum_all, sum_abs, sum_rel
    ws_bytes = max(int(lib.ctn_loudness_workspace(int(nchunks[a:b].sum()), b - a)) for a, b in groups)
    ws = torch.zeros(max(8, ws_bytes), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    at = 0
    for a, b in groups:
        lib.call("ctn_loudness", flat.data_ptr(), flat.numel(), off_d[a:].data_ptr(), len_d[a:].data_ptr(), cp_d[at:].data_ptr(),
                 b - a, int(nchunks[a:b].sum()), table.data_ptr(), d["hop"], counts[0, a:].data_ptr(), counts[1, a:].data_ptr(),
                 counts[2, a:].data_ptr(), counts[3, a:].data_ptr(), sums[0, a:].data_ptr(), sums[1, a:].data_ptr(),
                 sums[2, a:].data_ptr(), ws.data_ptr(), ws.numel(), stream)
        at += b - a + 1
    counts, sums = counts.cpu().numpy(), sums.cpu().numpy()
    stats = dict(ns=counts[0], n_blocks=counts[1], n_abs=counts[2], n_rel=counts[3], sum_all=sums[0], sum_abs=sums[1], sum_rel=sums[2])
    out = loudness_from_stats(stats["n_blocks"], stats["n_abs"], stats["n_rel"], stats["sum_all"], stats["sum_abs"], stats["sum_rel"])
    out.update(stats)
    return out


def integrated_loudness(x, lengths, sample_rate):
    """Padded batches on the device: x [R, T] float32, lengths [R] (the first lengths[r] samples of row r count).
    -> the dict of integrated_loudness_ragged."""
    if x.dim() != 2:
        raise ValueError("x must be [R, T], got %s" % (tuple(x.shape),))
    R, T = x.shape
    lens = np.asarray(lengths.cpu() if torch.is_tensor(lengths) else lengths, dtype=np.int64).reshape(-1)
    if len(lens) != R or (R and (int(lens.min()) < 0 or int(lens.max()) > T)):
        raise ValueError("lengths must hold %d values in [0, %d]" % (R, T))
    return integrated_loudness_ragged(x.contiguous().reshape(-1), np.arange(R, dtype=np.int64) * T, lens, sample_rate)
