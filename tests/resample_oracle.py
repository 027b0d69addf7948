"""Oracle for the on-device sinc resampling (csrc/ctn_resample.hip) and the dynamic mixer's speed perturbation: the contract
of include/ctn_hip.h restated in pure numpy, written from that contract.  No GPU, no import of the package.

    design_filter(up, down)                                     -> h float32 [up, 2W], W
    resample_f32(x, up, down, h, W, n_out=None, start=0)        -> float32, sequential: one rounding per product and per add
    resample_f64(x, up, down, h, W, n_out=None, start=0)        -> float64 sum of the float32 table's taps
    tap_abs_sum(x, up, down, h, W, n_out=None, start=0)         -> float64 sum_j |h_j| |x_j| per output (the rounding bound)
    plan_speed(seed, rank, epoch, step, B, C, seg_len, tables, speeds) -> plan_utt, plan_start, plan_q, gain, plan_pct
    speed_segments(corpus, offsets, lens, plan_utt, plan_start, plan_pct, T) -> seg float32 [B, C, T]

x outside [0, len(x)) reads as zero; `start` moves output sample 0 to input sample `start` (the speed-perturbed segments).
"""
import math

import numpy as np

import dynmix_oracle as DO


def design_filter(up, down, zeros=32, rolloff=0.95, beta=14.77):
    assert up >= 1 and down >= 1 and math.gcd(up, down) == 1
    fc = rolloff * min(1.0, up / down)
    W = int(math.ceil(zeros / fc))
    h = np.zeros((up, 2 * W), dtype=np.float64)
    for p in range(up):
        tau = (np.arange(2 * W, dtype=np.float64) - W + 1) - p / up
        live = np.abs(tau) < W
        win = np.zeros(2 * W, dtype=np.float64)
        win[live] = np.i0(beta * np.sqrt(1.0 - (tau[live] / W) ** 2)) / np.i0(beta)
        row = fc * np.sinc(fc * tau) * win
        h[p] = row / row.sum()
    return h.astype(np.float32), W


def out_len(n_in, up, down):
    return -((-int(n_in) * int(up)) // int(down))


def need(seg_len, pct):
    return -((-int(seg_len) * int(pct)) // 100)


def speed_ratio(pct):
    g = math.gcd(100, int(pct))
    return 100 // g, int(pct) // g


def _indices(n_in, up, down, W, n_out, start):
    """(padded-array index of tap 0, phase) of every output; the padded array holds `front` zeros before the row."""
    t = np.arange(n_out, dtype=np.int64)
    pos = t * down
    i, phase = pos // up + int(start), pos % up
    first = i - W + 1
    front = max(0, -int(first.min())) if n_out else 0
    back = max(0, int(first.max()) + 2 * W - n_in) if n_out else 0
    return first + front, phase, front, back


def _run(x, up, down, h, W, n_out, start, dtype, table):
    x = np.asarray(x)
    n_out = out_len(len(x), up, down) if n_out is None else int(n_out)
    first, phase, front, back = _indices(len(x), up, down, W, n_out, start)
    xp = np.concatenate([np.zeros(front, dtype), x.astype(dtype), np.zeros(back, dtype)])
    y = np.zeros(n_out, dtype=dtype)
    for j in range(2 * W):
        y = y + table[phase, j] * xp[first + j]                     # one rounding for the product, one for the add
    assert y.dtype == dtype
    return y


def resample_f32(x, up, down, h, W, n_out=None, start=0):
    assert h.dtype == np.float32
    return _run(np.asarray(x, dtype=np.float32), up, down, h, W, n_out, start, np.float32, h)


def resample_f64(x, up, down, h, W, n_out=None, start=0):
    return _run(x, up, down, h, W, n_out, start, np.float64, h.astype(np.float64))


def tap_abs_sum(x, up, down, h, W, n_out=None, start=0):
    return _run(np.abs(np.asarray(x, dtype=np.float64)), up, down, h, W, n_out, start, np.float64, np.abs(h.astype(np.float64)))


def plan_speed(seed, rank, epoch, step, B, C, seg_len, tables, speeds):
    """DO.plan with one more Philox block per source, counter (c + 256, b, step, epoch): word 0 picks the percent; the start is
    drawn over need = ceil(seg_len * pct / 100) samples.  Speaker, utterance and level draws are DO.plan's."""
    assert 0 <= seed < 1 << 48 and 0 <= rank < 1 << 16 and 2 <= C <= 4
    spk_ptr, utt_ids, lens = tables["spk_ptr"], tables["utt_ids"], tables["lens"]
    inv_rms, w = tables["inv_rms"], tables["w"]
    S = len(spk_ptr) - 1
    key = (seed & DO.MASK, (seed >> 32) | (rank << 16))
    plan_utt = np.zeros((B, C), np.int32)
    plan_start = np.zeros((B, C), np.int64)
    plan_q = np.zeros((B, C), np.int32)
    plan_pct = np.zeros((B, C), np.int32)
    gain = np.zeros((B, C), np.float32)
    for b in range(B):
        taken = []
        for c in range(C):
            r = DO.philox4x32((c, b, step, epoch), key)
            rs = DO.philox4x32((c + 256, b, step, epoch), key)
            pct = int(speeds[DO.below(rs[0], len(speeds))])
            s = DO.below(r[0], S - c)
            for t in sorted(taken):
                if s >= t:
                    s += 1
            taken.append(s)
            first, count = int(spk_ptr[s]), int(spk_ptr[s + 1] - spk_ptr[s])
            u = int(utt_ids[first + DO.below(r[1], count)])
            start = DO.below(r[2], int(lens[u]) - need(seg_len, pct) + 1)
            if c == 0:
                q = 1 + DO.below(r[3], 249)
            elif c == 1:
                q = -int(plan_q[b, 0])
            else:
                v = DO.below(r[3], 498)
                q = 1 + v if v < 249 else -(1 + v - 249)
            plan_utt[b, c], plan_start[b, c], plan_q[b, c], plan_pct[b, c] = u, start, q, pct
            gain[b, c] = np.float32(w[q + 249]) * np.float32(inv_rms[u])
    return plan_utt, plan_start, plan_q, gain, plan_pct


_FILTERS = {}


def speed_segments(corpus, offsets, lens, plan_utt, plan_start, plan_pct, T):
    corpus = np.asarray(corpus, dtype=np.float32)
    B, C = plan_utt.shape
    seg = np.zeros((B, C, T), np.float32)
    for b in range(B):
        for c in range(C):
            u, st, pct = int(plan_utt[b, c]), int(plan_start[b, c]), int(plan_pct[b, c])
            x = corpus[int(offsets[u]):int(offsets[u]) + int(lens[u])]
            assert 0 <= st and st + need(T, pct) <= len(x)
            if pct == 100:
                seg[b, c] = x[st:st + T]
                continue
            up, down = speed_ratio(pct)
            if (up, down) not in _FILTERS:
                _FILTERS[(up, down)] = design_filter(up, down)
            h, W = _FILTERS[(up, down)]
            seg[b, c] = resample_f32(x, up, down, h, W, n_out=T, start=st)
    return seg


def mix_segments(seg, gain):
    """DO.mix over the segment buffer as a corpus of B * C utterances of T samples."""
    B, C, T = seg.shape
    utt = np.arange(B * C, dtype=np.int32).reshape(B, C)
    return DO.mix(seg.reshape(-1), np.arange(B * C, dtype=np.int64) * T, utt, np.zeros((B, C), np.int64), gain, T)
