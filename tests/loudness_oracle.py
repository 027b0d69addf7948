"""Oracle for the integrated loudness meter (csrc/ctn_loudness.hip): ITU-R BS.1770-4, mono, as include/ctn_hip.h states it
("integrated loudness"), restated in numpy from that contract and from the Recommendation.  No GPU, no import of the package.

    design(fs, chunk)                 -> the fp64 tables: the two biquads, the transition matrix, the hop, the absolute gate
    k_weight(x, fs, chunk)            -> the K-weighted signal in the device's form: chunks from zero state, the carry, chunks from
                                         their true states (vectorised over the chunks of the utterance)
    stats(x, fs, chunk)               -> dict(ns, n_blocks, n_abs, n_rel, sum_all, sum_abs, sum_rel, z [n_blocks], y)
    loudness(st)                      -> dict(power, lufs, ungated) of one utterance from its statistics
    scipy_k_weight(x, fs)             -> the same filters as a scipy.signal.lfilter chain
    cases(fs, chunk)                  -> the utterances the GPU tests use
"""
import math

import numpy as np

SHELF_F0, SHELF_GAIN_DB, SHELF_Q, SHELF_VB_EXP = 1681.974450955533, 3.999843853973347, 0.7071752369554196, 0.4996667741545416
HP_F0, HP_Q = 38.13547087602444, 0.5003270373238773
OFFSET_DB = -0.691
LANES = 64                          # the device sums block j in lane j % 64, then the lanes in ascending order


def biquad_step(c, v, z0, z1):
    """One sample (or one sample of many chunks at once: arrays) through [b0, b1, b2, a1, a2].  -> (y, z0, z1)"""
    y = c[0] * v + z0
    return y, (c[1] * v + z1) - c[3] * y, c[2] * v - c[4] * y


def k_step(d, x, z):
    y, a, b = biquad_step(d["shelf"], x, z[0], z[1])
    y, c, e = biquad_step(d["hp"], y, z[2], z[3])
    return y, [a, b, c, e]


def design(fs, chunk):
    fs, chunk = int(fs), int(chunk)
    assert 8000 <= fs <= 48000 and fs % 10 == 0
    K = math.tan(math.pi * SHELF_F0 / fs)
    Vh = 10.0 ** (SHELF_GAIN_DB / 20.0)
    Vb = Vh ** SHELF_VB_EXP
    a0 = 1.0 + K / SHELF_Q + K * K
    shelf = np.array([(Vh + Vb * K / SHELF_Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / SHELF_Q + K * K) / a0,
                      2.0 * (K * K - 1.0) / a0, (1.0 - K / SHELF_Q + K * K) / a0])
    K = math.tan(math.pi * HP_F0 / fs)
    a0 = 1.0 + K / HP_Q + K * K
    hp = np.array([1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / HP_Q + K * K) / a0])
    d = dict(sample_rate=fs, chunk=chunk, hop=fs // 10, shelf=shelf, hp=hp, abs_gate=10.0 ** ((-70.0 - OFFSET_DB) / 10.0))
    z = [np.array([1.0 if r == k else 0.0 for k in range(4)]) for r in range(4)]
    zero = np.zeros(4)
    for _ in range(chunk):
        _, z = k_step(d, zero, z)
    d["t"] = np.stack(z)
    return d


def _carry(T, z_end):
    """z_end [nch, 4] (end states from zero) -> the true start states: s_0 = 0, s_(c+1) = T s_c + z_c, row r summed k ascending,
    z_c last."""
    nch, S = z_end.shape
    start = np.zeros((nch, S))
    s = [0.0] * S
    for c in range(nch):
        start[c] = s
        nxt = []
        for r in range(S):
            acc = float(T[r][0]) * s[0]
            for k in range(1, S):
                acc = acc + float(T[r][k]) * s[k]
            nxt.append(acc + float(z_end[c][r]))
        s = nxt
    return start


def _chunks(x, ch):
    x = np.asarray(x, dtype=np.float32).reshape(-1).astype(np.float64)
    N = len(x)
    nch = (N + ch - 1) // ch
    return np.concatenate((x, np.zeros(nch * ch - N))).reshape(nch, ch), N, nch


def k_weight(x, fs, chunk, d=None):
    """-> (Y [nch, chunk], N): the K-weighted chunks (what lies behind sample N in the last one is not the device's business)."""
    d = design(fs, chunk) if d is None else d
    X, N, nch = _chunks(x, d["chunk"])
    z = [np.zeros(nch) for _ in range(4)]
    for i in range(d["chunk"]):
        _, z = k_step(d, X[:, i], z)
    start = _carry(d["t"], np.stack(z, axis=1)) if nch else np.zeros((0, 4))
    z, Y = [start[:, k].copy() for k in range(4)], np.zeros((nch, d["chunk"]))
    for i in range(d["chunk"]):
        Y[:, i], z = k_step(d, X[:, i], z)
    return Y, N


def stats(x, fs, chunk):
    d = design(fs, chunk)
    ch, h = d["chunk"], d["hop"]
    Y, N = k_weight(x, fs, chunk, d)
    nch = Y.shape[0]
    # the pieces: chunk c meets sub-blocks (c ch) // h + k, k = 0, 1, 2; every piece is summed from 0 in sample order
    n = np.arange(nch * ch).reshape(nch, ch)
    piece = n // h - (n[:, :1] // h)
    live = n < N
    assert nch == 0 or int(piece.max()) <= 2
    P = np.zeros((nch, 3))
    for i in range(ch):
        sq = Y[:, i] * Y[:, i]
        for k in range(3):
            take = live[:, i] & (piece[:, i] == k)
            P[:, k] = np.where(take, P[:, k] + sq, P[:, k])
    nsub = N // h
    nb = max(0, nsub - 3)
    S = np.zeros(nsub)
    for i in range(nsub if nb else 0):                       # sub-block i: its pieces, chunks ascending, from 0
        s = 0.0
        for c in range(i * h // ch, ((i + 1) * h - 1) // ch + 1):
            s = s + float(P[c, i - c * ch // h])
        S[i] = s
    z = (((S[0:nb] + S[1:nb + 1]) + S[2:nb + 2]) + S[3:nb + 3]) / float(4 * h) if nb else np.zeros(0)

    def ordered(mask):
        lanes = [0.0] * LANES
        for j in range(nb):
            if mask[j]:
                lanes[j % LANES] = lanes[j % LANES] + float(z[j])
        t = lanes[0]
        for k in range(1, LANES):
            t = t + lanes[k]
        return t

    m_abs = z > d["abs_gate"]
    n_abs = int(m_abs.sum())
    sum_all, sum_abs = ordered(np.ones(nb, dtype=bool)), ordered(m_abs)
    m_rel = np.zeros(nb, dtype=bool)
    if n_abs > 0:
        m_rel = m_abs & (z > (sum_abs / float(n_abs)) / 10.0)
    return dict(ns=N, n_blocks=nb, n_abs=n_abs, n_rel=int(m_rel.sum()), sum_all=sum_all, sum_abs=sum_abs, sum_rel=ordered(m_rel),
                z=z, y=Y.reshape(-1)[:N])


def loudness(st):
    power = st["sum_rel"] / st["n_rel"] if st["n_rel"] > 0 else 0.0
    mean_all = st["sum_all"] / st["n_blocks"] if st["n_blocks"] > 0 else 0.0
    db = lambda p: OFFSET_DB + 10.0 * math.log10(p) if p > 0 else -math.inf
    return dict(power=power if power > 0 else 0.0, lufs=db(power), ungated=db(mean_all))


def scipy_k_weight(x, fs):
    from scipy.signal import lfilter
    d = design(fs, 1)
    y = np.asarray(x, dtype=np.float32).astype(np.float64)
    for c in (d["shelf"], d["hp"]):
        y = lfilter(c[:3], [1.0, c[3], c[4]], y)
    return y


def tone(fs, freq, seconds, amp):
    return (amp * np.sin(2.0 * np.pi * freq * np.arange(int(round(seconds * fs))) / fs)).astype(np.float32)


def cases(fs, chunk):
    """-> list of (name, float32 array): the block edges, the scan's seams, both gates, silence."""
    h, ch = fs // 10, int(chunk)
    n = 4 * h
    rng = np.random.default_rng(fs + 1)
    noise = lambda m, amp=0.1: (amp * rng.standard_normal(m)).astype(np.float32)
    loud = noise(3 * fs + 123, 0.2)
    loud[len(loud) // 2:] *= np.float32(0.1)                 # the second half 20 dB down: below the relative gate
    k = (n + h) // ch + 2                                     # chunks of the seam cases: a few blocks at every rate
    return [
        ("n-1", noise(n - 1)), ("n", noise(n)), ("n+h-1", noise(n + h - 1)), ("n+h", noise(n + h)),
        ("kch-1", noise(k * ch - 1)), ("kch", noise(k * ch, 0.02)), ("kch+1", noise(k * ch + 1)),
        ("loud_quiet", loud), ("zeros", np.zeros(n + h + 5, dtype=np.float32)), ("below_abs", tone(fs, 440.0, 0.7, 1e-5)),
        ("len1", noise(1)), ("tone", tone(fs, 997.0, 0.9, 0.5)),
    ]
