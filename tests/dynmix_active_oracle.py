"""Oracle for the dynamic mixer's speaker-count draw (csrc/ctn_dynmix_active.hip): the contract of include/ctn_hip.h ("variable
speaker counts in the dynamic mixer") restated in pure Python on top of the Philox block and the integer draw of dynmix_oracle.py.
No GPU, no import of the package.

    counts(seed, rank, epoch, step, B, C, m)    -> n_active [B] int32 in [m, C]
    masked(gain, n_active)                      -> gain with the entries c >= n_active[b] set to +0
    other_words(C)                              -> the Philox c0 words of every other draw of a minibatch
"""
import numpy as np

import dynmix_oracle as DO

COUNT_WORD = 1024


def other_words(C):
    """c0 of the plan (c), the speed draw (256 + c), the RIR draw (512 + c) and the noise draw (768)."""
    return sorted(set(range(C)) | {256 + c for c in range(C)} | {512 + c for c in range(C)} | {768})


def counts(seed, rank, epoch, step, B, C, m):
    assert 0 <= seed < 1 << 48 and 0 <= rank < 1 << 16 and 1 <= m <= C
    key = (seed & DO.MASK, (seed >> 32) | (rank << 16))
    out = np.zeros(B, np.int32)
    for b in range(B):
        r = DO.philox4x32((COUNT_WORD, b, step, epoch), key)
        out[b] = m + DO.below(r[0], C - m + 1)
    return out


def masked(gain, n_active):
    gain = np.array(gain, dtype=np.float32, copy=True)
    for b in range(gain.shape[0]):
        gain[b, int(n_active[b]):] = 0.0
    return gain
