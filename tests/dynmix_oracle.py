"""Oracle for the on-device dynamic mixing (csrc/ctn_dynmix.hip): the contract of include/ctn_hip.h restated in pure Python /
numpy, written from that contract and from the published Philox definition (Salmon et al., "Parallel random numbers: as easy
as 1, 2, 3", SC'11).  No GPU, no import of the package.

    philox4x32(counter, key)                                  -> four 32-bit words, ten rounds
    plan(seed, rank, epoch, step, B, C, seg_len, tables)      -> plan_utt, plan_start, plan_q, gain
    mix(corpus, offsets, plan_utt, plan_start, gain, T)       -> mixture, sources, peak   (numpy float32, one rounding per operation)
    meansq(corpus, offsets, lens)                             -> float64

`tables` is a dict of numpy arrays: spk_ptr [S+1], utt_ids, lens [U], inv_rms [U] float32, w [499] float32.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32(counter, key, rounds=10):
    c0, c1, c2, c3 = (int(v) & MASK for v in counter)
    k0, k1 = (int(v) & MASK for v in key)
    for _ in range(rounds):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def below(r, n):
    """Integer in [0, n) from the 32-bit word r."""
    return (int(r) * int(n)) >> 32


def level_table():
    """w[q + 249] = 10^(q / 2000) for q = -249 .. 249, float32 rounded from float64."""
    return np.array([10.0 ** (q / 2000.0) for q in range(-249, 250)], dtype=np.float64).astype(np.float32)


def plan(seed, rank, epoch, step, B, C, seg_len, tables):
    assert 0 <= seed < 1 << 48 and 0 <= rank < 1 << 16 and 2 <= C <= 4
    spk_ptr, utt_ids, lens = tables["spk_ptr"], tables["utt_ids"], tables["lens"]
    inv_rms, w = tables["inv_rms"], tables["w"]
    S = len(spk_ptr) - 1
    key = (seed & MASK, (seed >> 32) | (rank << 16))
    plan_utt = np.zeros((B, C), np.int32)
    plan_start = np.zeros((B, C), np.int64)
    plan_q = np.zeros((B, C), np.int32)
    gain = np.zeros((B, C), np.float32)
    for b in range(B):
        taken = []
        for c in range(C):
            r = philox4x32((c, b, step, epoch), key)
            s = below(r[0], S - c)
            for t in sorted(taken):
                if s >= t:
                    s += 1
            taken.append(s)
            first, count = int(spk_ptr[s]), int(spk_ptr[s + 1] - spk_ptr[s])
            u = int(utt_ids[first + below(r[1], count)])
            start = below(r[2], int(lens[u]) - seg_len + 1)
            if c == 0:
                q = 1 + below(r[3], 249)
            elif c == 1:
                q = -int(plan_q[b, 0])
            else:
                v = below(r[3], 498)
                q = 1 + v if v < 249 else -(1 + v - 249)
            plan_utt[b, c], plan_start[b, c], plan_q[b, c] = u, start, q
            gain[b, c] = np.float32(w[q + 249]) * np.float32(inv_rms[u])
    return plan_utt, plan_start, plan_q, gain


def mix(corpus, offsets, plan_utt, plan_start, gain, T):
    corpus = np.asarray(corpus, dtype=np.float32)
    gain = np.asarray(gain, dtype=np.float32)
    B, C = plan_utt.shape
    mixture = np.zeros((B, T), np.float32)
    sources = np.zeros((B, C, T), np.float32)
    peak = np.zeros(B, np.float32)
    for b in range(B):
        s = []
        for c in range(C):
            o = int(offsets[plan_utt[b, c]]) + int(plan_start[b, c])
            s.append(gain[b, c] * corpus[o:o + T])                     # float32 * float32 array: one rounding each
        m = s[0] + s[1]
        for c in range(2, C):
            m = m + s[c]
        a = np.float32(max(float(np.abs(m).max()), max(float(np.abs(x).max()) for x in s)))
        scale = np.float32(0.9) / a if a > 0 else np.float32(1.0)
        assert np.asarray(scale).dtype == np.float32
        mixture[b] = scale * m
        for c in range(C):
            sources[b, c] = scale * s[c]
        peak[b] = a
    return mixture, sources, peak


def meansq(corpus, offsets, lens):
    x = np.asarray(corpus, dtype=np.float64)
    return np.array([np.sum(x[int(o):int(o) + int(n)] ** 2) / int(n) for o, n in zip(offsets, lens)], dtype=np.float64)
