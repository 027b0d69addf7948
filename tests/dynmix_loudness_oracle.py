"""Oracle for the LibriMix-recipe levels of the dynamic mixer (csrc/ctn_dynmix_loudness.hip and the peak rule of the gathers): the
contract of include/ctn_hip.h ("LibriMix-recipe mixing") restated in pure Python / numpy on top of the Philox block and the
integer draw of dynmix_oracle.py and the noise draw of dynmix_aug_oracle.py.  No GPU, no import of the package.

    loudness_table(lo10, hi10)                                   -> wl float32
    plan_loudness(seed, rank, epoch, step, plan_utt, inv_rms, wl, lo10)   -> plan_l10 [B,C] int32, gain [B,C] float32
    noise_plan(seed, rank, epoch, step, B, C, seg_len, noise)    -> AO.plan_aug's noise half with the loudness table as `wn`
    mix(corpus, offsets, plan_utt, plan_start, gain, T, peak, noise...)   -> mixture, sources, peak under either peak rule
    other_words(C)                                               -> the Philox c0 words of every other draw of a minibatch
"""
import numpy as np

import dynmix_aug_oracle as AO
import dynmix_oracle as DO

LOUDNESS_WORD = 1280                # c0 = 1280 + c
OFFSET_DB = 0.691


def other_words(C):
    """c0 of the plan (c), the speed draw (256 + c), the RIR draw (512 + c), the noise draw (768) and the count draw (1024)."""
    return sorted(set(range(C)) | {256 + c for c in range(C)} | {512 + c for c in range(C)} | {768, 1024})


def loudness_table(lo10, hi10):
    """wl[i] = 10^(((lo10 + i) / 10 + 0.691) / 20), float32 rounded from float64."""
    return np.array([10.0 ** (((lo10 + i) / 10.0 + OFFSET_DB) / 20.0) for i in range(hi10 - lo10 + 1)], dtype=np.float64).astype(np.float32)


def plan_loudness(seed, rank, epoch, step, plan_utt, inv_rms, wl, lo10):
    """`step` is the minibatch's step (the device reads the advanced step word and takes one off)."""
    assert 0 <= seed < 1 << 48 and 0 <= rank < 1 << 16
    key = (seed & DO.MASK, (seed >> 32) | (rank << 16))
    B, C = plan_utt.shape
    plan_l10, gain = np.zeros((B, C), np.int32), np.zeros((B, C), np.float32)
    for b in range(B):
        for c in range(C):
            i = DO.below(DO.philox4x32((LOUDNESS_WORD + c, b, step, epoch), key)[0], len(wl))
            u = int(plan_utt[b, c])
            plan_l10[b, c] = lo10 + i
            gain[b, c] = np.float32(wl[i]) * np.float32(inv_rms[u]) if 0 <= u < len(inv_rms) else np.float32(0.0)
    return plan_l10, gain


def noise_plan(seed, rank, epoch, step, B, C, seg_len, noise_ids, noise_lens, noise_inv_rms, lo10, hi10):
    """-> (noise_utt, noise_start, l10, ngain): the word that chooses the SNR chooses the noise loudness."""
    noise = dict(noise_ids=noise_ids, lens=noise_lens, inv_rms=noise_inv_rms, wn=loudness_table(lo10, hi10), lo10=lo10)
    return AO.plan_aug(seed, rank, epoch, step, B, C, seg_len, noise=noise)[1:]


def peak_scale(a, peak):
    a = np.float32(a)
    over = np.float32(0.9) if peak == "clip" else np.float32(0.0)
    assert peak in ("always", "clip")
    return np.float32(0.9) / a if a > over else np.float32(1.0)


def mix(corpus, offsets, plan_utt, plan_start, gain, T, peak="always", noise=None, noise_offsets=None, noise_utt=None, noise_start=None,
        ngain=None):
    """s_c = gain * corpus[..], n = ngain * noise[..]; mix = (((s_0 + s_1) + ...) + n); a = max(|mix|, |s_c|); everything times
    peak_scale(a); one float32 rounding per operation."""
    corpus = np.asarray(corpus, dtype=np.float32)
    gain = np.asarray(gain, dtype=np.float32)
    B, C = plan_utt.shape
    mixture, sources, pk = np.zeros((B, T), np.float32), np.zeros((B, C, T), np.float32), np.zeros(B, np.float32)
    for b in range(B):
        s = []
        for c in range(C):
            o = int(offsets[plan_utt[b, c]]) + int(plan_start[b, c])
            s.append(gain[b, c] * corpus[o:o + T])
        m = s[0] + s[1]
        for c in range(2, C):
            m = m + s[c]
        if noise is not None:
            o = int(noise_offsets[noise_utt[b]]) + int(noise_start[b])
            m = m + np.float32(ngain[b]) * np.asarray(noise, dtype=np.float32)[o:o + T]
        a = np.float32(max(float(np.abs(m).max()), max(float(np.abs(x).max()) for x in s)))
        scale = peak_scale(a, peak)
        assert np.asarray(scale).dtype == np.float32 and m.dtype == np.float32
        mixture[b] = scale * m
        for c in range(C):
            sources[b, c] = scale * s[c]
        pk[b] = a
    return mixture, sources, pk


def mix_segments(seg, gain, peak="always"):
    """mix() over a segment buffer [B,C,T] as a corpus of B * C utterances of T samples."""
    B, C, T = seg.shape
    utt = np.arange(B * C, dtype=np.int32).reshape(B, C)
    return mix(seg.reshape(-1), np.arange(B * C, dtype=np.int64) * T, utt, np.zeros((B, C), np.int64), gain, T, peak)
