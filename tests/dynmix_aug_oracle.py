"""Oracle for the noisy and reverberant dynamic mixing (csrc/ctn_dynmix_aug.hip): the contract of include/ctn_hip.h ("noisy
and reverberant dynamic mixing") restated in pure numpy, written from that text.  No GPU, no import of the package.

    rir_tables(arrays, rate, early_ms, normalize)             -> dict(bank f32, offsets i64, lens, direct, early i32)
    snr_table(lo10, hi10)                                     -> wn float32
    plan_aug(seed, rank, epoch, step, B, C, seg_len, R=None, noise=None) -> plan_rir, noise_utt, noise_start, snr10, ngain
    reverb_f32(x, h, d, e)                                    -> (wet, tgt) float32, one rounding per product and per add
    reverb_f64(x, h, d, e)                                    -> (wet, tgt) float64 sums of the float32 taps
    tap_abs_sum(x, h, d)                                      -> float64 sum_j |h_j| |x_j| per output (the rounding bound)
    reverb_rows(corpus, offsets, plan_utt, plan_start, T, tables, plan_rir) -> wet, tgt float32 [N, T]
    mix_aug(corpus, offsets, plan_utt, plan_start, gain, T, tgt_corpus=None, noise=None, ...) -> mixture, sources, peak

`noise` of plan_aug is a dict: noise_ids, lens [Un], inv_rms [Un] float32, wn float32, lo10.  x outside [0, len(x)) reads as zero.
"""
import numpy as np

import dynmix_oracle as DO

MAX_TAPS = 8192


def rir_tables(arrays, rate=8000, early_ms=50.0, normalize=True):
    taps, lens, direct, early = [], [], [], []
    for a in arrays:
        h = np.asarray(a, dtype=np.float64).reshape(-1)
        n = len(h)
        assert 1 <= n <= MAX_TAPS and np.all(np.isfinite(h))
        if normalize:
            h = h / np.sqrt(np.sum(h * h))
        d = int(np.argmax(np.abs(h)))
        e = n if early_ms is None else min(n, d + 1 + int(round(early_ms * rate / 1000.0)))
        taps.append(h.astype(np.float32))
        lens.append(n)
        direct.append(d)
        early.append(e)
    offsets = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64)
    return dict(bank=np.concatenate(taps), offsets=offsets, lens=np.array(lens, np.int32), direct=np.array(direct, np.int32),
                early=np.array(early, np.int32))


def snr_table(lo10, hi10):
    """wn[i] = 10^(-(lo10 + i) / 200), float32 rounded from float64."""
    return np.array([10.0 ** (-(lo10 + i) / 200.0) for i in range(hi10 - lo10 + 1)], dtype=np.float64).astype(np.float32)


def plan_aug(seed, rank, epoch, step, B, C, seg_len, R=None, noise=None):
    assert 0 <= seed < 1 << 48 and 0 <= rank < 1 << 16
    key = (seed & DO.MASK, (seed >> 32) | (rank << 16))
    plan_rir = noise_utt = noise_start = snr10 = ngain = None
    if R is not None:
        plan_rir = np.zeros((B, C), np.int32)
        for b in range(B):
            for c in range(C):
                plan_rir[b, c] = DO.below(DO.philox4x32((c + 512, b, step, epoch), key)[0], R)
    if noise is not None:
        ids, lens, inv_rms, wn, lo10 = noise["noise_ids"], noise["lens"], noise["inv_rms"], noise["wn"], noise["lo10"]
        noise_utt, noise_start = np.zeros(B, np.int32), np.zeros(B, np.int64)
        snr10, ngain = np.zeros(B, np.int32), np.zeros(B, np.float32)
        for b in range(B):
            r = DO.philox4x32((768, b, step, epoch), key)
            v = int(ids[DO.below(r[0], len(ids))])
            k = DO.below(r[2], len(wn))
            noise_utt[b] = v
            noise_start[b] = DO.below(r[1], int(lens[v]) - seg_len + 1)
            snr10[b] = lo10 + k
            ngain[b] = np.float32(wn[k]) * np.float32(inv_rms[v])
    return plan_rir, noise_utt, noise_start, snr10, ngain


def _reverb(x, h, d, e, dtype):
    """acc = +0; j ascending: acc = acc + h[j] * x[t + d - j], every product and every add rounded once to `dtype`."""
    x, h = np.asarray(x, dtype=dtype), np.asarray(h, dtype=dtype)
    T, n = len(x), len(h)
    assert 0 <= d < n and 0 <= e <= n
    xp = np.concatenate([np.zeros(n, dtype), x, np.zeros(n, dtype)])          # xp[n + g] = x[g], zeros outside [0, T)
    t = np.arange(T)
    acc = np.zeros(T, dtype)
    tgt = acc.copy()
    for j in range(n):
        acc = acc + h[j] * xp[n + t + d - j]
        if j + 1 == e:
            tgt = acc.copy()
    assert acc.dtype == dtype
    return acc, tgt


def reverb_f32(x, h, d, e):
    assert np.asarray(h).dtype == np.float32
    return _reverb(np.asarray(x, dtype=np.float32), h, d, e, np.float32)


def reverb_f64(x, h, d, e):
    return _reverb(x, np.asarray(h, dtype=np.float32), d, e, np.float64)


def tap_abs_sum(x, h, d):
    return _reverb(np.abs(np.asarray(x, dtype=np.float64)), np.abs(np.asarray(h, dtype=np.float32)), d, len(h), np.float64)[0]


def reverb_rows(corpus, offsets, plan_utt, plan_start, T, tables, plan_rir):
    """wet, tgt [N, T] of N = plan_utt.size rows at unit gain: the dry segment is the T samples from offsets[u] + start on."""
    corpus = np.asarray(corpus, dtype=np.float32)
    utt, start, rir = np.reshape(plan_utt, -1), np.reshape(plan_start, -1), np.reshape(plan_rir, -1)
    wet, tgt = np.zeros((len(utt), T), np.float32), np.zeros((len(utt), T), np.float32)
    for i in range(len(utt)):
        o, r = int(offsets[utt[i]]) + int(start[i]), int(rir[i])
        h = tables["bank"][int(tables["offsets"][r]):int(tables["offsets"][r]) + int(tables["lens"][r])]
        wet[i], tgt[i] = reverb_f32(corpus[o:o + T], h, int(tables["direct"][r]), int(tables["early"][r]))
    return wet, tgt


def mix_aug(corpus, offsets, plan_utt, plan_start, gain, T, tgt_corpus=None, noise=None, noise_offsets=None, noise_utt=None,
            noise_start=None, ngain=None):
    """r_c = gain * corpus[..], g_c = gain * tgt_corpus[..] (r_c when None), n = ngain * noise[..];
    mix = (((r_0 + r_1) + ...) + n); a = max(|mix|, |g_c|); everything times 0.9f / a.  An entry with plan_utt < 0 or
    noise_utt < 0 reads as silence and gives peak = -1."""
    corpus = np.asarray(corpus, dtype=np.float32)
    gain = np.asarray(gain, dtype=np.float32)
    B, C = plan_utt.shape
    mixture, sources, peak = np.zeros((B, T), np.float32), np.zeros((B, C, T), np.float32), np.zeros(B, np.float32)
    for b in range(B):
        r, g, bad = [], [], False
        for c in range(C):
            if plan_utt[b, c] < 0:
                bad = True
                r.append(np.zeros(T, np.float32))
                g.append(np.zeros(T, np.float32))
                continue
            o = int(offsets[plan_utt[b, c]]) + int(plan_start[b, c])
            r.append(gain[b, c] * corpus[o:o + T])
            g.append(r[-1] if tgt_corpus is None else gain[b, c] * np.asarray(tgt_corpus, dtype=np.float32)[o:o + T])
        m = r[0] + r[1]
        for c in range(2, C):
            m = m + r[c]
        if noise is not None:
            if noise_utt[b] < 0:
                bad = True
                m = m + np.zeros(T, np.float32)
            else:
                o = int(noise_offsets[noise_utt[b]]) + int(noise_start[b])
                m = m + np.float32(ngain[b]) * np.asarray(noise, dtype=np.float32)[o:o + T]
        a = np.float32(max(float(np.abs(m).max()), max(float(np.abs(x).max()) for x in g)))
        scale = np.float32(0.9) / a if a > 0 else np.float32(1.0)
        assert np.asarray(scale).dtype == np.float32 and m.dtype == np.float32
        mixture[b] = scale * m
        for c in range(C):
            sources[b, c] = scale * g[c]
        peak[b] = np.float32(-1.0) if bad else a
    return mixture, sources, peak


def mix_rows(wet, tgt, gain, **noise):
    """mix_aug over wet / tgt [N, T] as corpora of N utterances of T samples (plan_utt = arange, plan_start = 0)."""
    B, C = gain.shape
    T = wet.shape[1]
    utt = np.arange(B * C, dtype=np.int32).reshape(B, C)
    return mix_aug(wet.reshape(-1), np.arange(B * C, dtype=np.int64) * T, utt, np.zeros((B, C), np.int64), gain, T,
                   tgt_corpus=None if tgt is None else tgt.reshape(-1), **noise)
