"""Oracle for the active speech level meter (csrc/ctn_levels.hip): ITU-T P.56 method B as include/ctn_hip.h states it
("active speech level"), restated in numpy from that contract and from the Recommendation.  No GPU, no import of the package.

    design(fs, chunk)                 -> the fp64 tables: sections, transition matrices, nz, nh
    stats_sequential(x, fs)           -> form (a): one plain per-sample loop over the whole padded utterance
    stats_chunked(x, fs, chunk)       -> form (b): chunks from zero state, the carry, chunks from their true states, in exactly
                                         the header's operation order (vectorised over the chunks of the utterance)
    level(ssq, ns, emax, counts)      -> level (power), level_db, long_term, activity of one utterance
    scipy_band(x, fs), scipy_envelope(y, fs)  -> the same filters as scipy.signal.lfilter chains
    cases(fs, chunk)                  -> the utterances the CPU and GPU tests share

Both stats_* return dict(ssq, ns, emax, counts [20] int64, y, e).  -inf exponents are EMPTY = -32768.
"""
import math

import numpy as np

NBIN = 20
MARGIN_DB = 15.9
EMPTY = -32768
W0 = 0.39790951457558527
# scipy.signal.cheby2(5, 50, W0, 'high', analog=True): the real root, then one of each conjugate pair
PROTO_ZEROS = (0.0, 0.3784344367329518j, 0.2338853444143859j)
PROTO_POLES = (-0.6679326883376755, -0.20640255179488695 + 0.739421859068245j, -0.5403688959637246 + 0.45698784092881006j)


def band_step(sec, x, z):
    """One sample (or one sample of many chunks at once: arrays) through the band filter.  -> (y, new state list)"""
    b0, b1, a1 = sec["hp1"]
    y = b0 * x + z[0]
    out = [b1 * x - a1 * y]
    for name, k in (("bq1", 1), ("bq2", 3)):
        b0, b1, b2, a1, a2 = sec[name]
        v = y
        y = b0 * v + z[k]
        out.append((b1 * v + z[k + 1]) - a1 * y)
        out.append(b2 * v - a2 * y)
    if sec["lp"] is not None:
        c = sec["lp"]
        v = y
        y = c[0] * v + z[5]
        for k in range(1, 5):
            out.append((c[k] * v + z[5 + k]) - c[5 + k] * y)
        out.append(c[5] * v - c[10] * y)
    return y, out


def env_step(env, x, z):
    b0, a1, a2 = env
    s = b0 * x + z[0]
    return s, [z[1] - a1 * s, -(a2 * s)]


def transition(step, nstate, chunk):
    z = [np.array([1.0 if r == k else 0.0 for k in range(nstate)]) for r in range(nstate)]
    zero = np.zeros(nstate)
    for _ in range(chunk):
        _, z = step(zero, z)
    return np.stack(z)


def design(fs, chunk):
    fs, chunk = int(fs), int(chunk)
    zeros, poles = np.array(PROTO_ZEROS, dtype=np.complex128), np.array(PROTO_POLES, dtype=np.complex128)
    t = math.tan(math.pi * 200.0 / fs)
    zz, zp = 2.0 / (1.0 - zeros * t) - 1.0, 2.0 / (1.0 - poles * t) - 1.0
    hp1 = [1.0, -zz[0].real, -zp[0].real]
    bq = [[1.0, -2.0 * zz[k].real, abs(zz[k]) ** 2, -2.0 * zp[k].real, abs(zp[k]) ** 2] for k in (1, 2)]
    num = (1.0 - hp1[1]) * (1.0 - bq[0][1] + bq[0][2]) * (1.0 - bq[1][1] + bq[1][2])        # the sections at z = -1
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
    return dict(sample_rate=fs, chunk=chunk, nz=int(math.ceil(0.35 * fs)), nh=int(math.ceil(0.2 * fs)) + 1, use_lp=bool(use_lp),
                sections=sec, t_band=transition(lambda x, z: band_step(sec, x, z), nstate, chunk),
                t_env=transition(lambda x, z: env_step(sec["env"], x, z), 2, chunk))


def exponents(s):
    """frexp exponent of s * s per sample (fp64, denormals kept), EMPTY where the square is zero."""
    sq = s * s
    e = np.frexp(sq)[1].astype(np.int64)
    e[sq == 0] = EMPTY
    return e


def hangover(e, nh):
    """h[n] = max e[n - nh + 1 .. n], indices below 0 absent."""
    h, span = e.copy(), 1
    while span < nh and span < len(h):
        step = min(span, nh - span, len(h) - 1)
        h[step:] = np.maximum(h[step:], h[:-step].copy())
        span += step
    return h


def occupancy(e, nh):
    h = hangover(e, nh)
    emax = int(h.max()) + 1
    return emax, np.bincount(np.minimum(emax - h, NBIN) - 1, minlength=NBIN).astype(np.int64)


def _padded(x, d):
    x = np.asarray(x, dtype=np.float32).reshape(-1).astype(np.float64)
    return np.concatenate((x, np.zeros(d["nz"])))


def stats_sequential(x, fs):
    d = design(fs, 1)
    sec = {k: (None if v is None else [float(c) for c in v]) for k, v in d["sections"].items()}
    xp = _padded(x, d)
    y, s = np.zeros(len(xp)), np.zeros(len(xp))
    z, ze, ssq = [0.0] * (10 if d["use_lp"] else 5), [0.0, 0.0], 0.0
    for n, v in enumerate(xp.tolist()):
        y[n], z = band_step(sec, v, z)
        ssq = ssq + y[n] * y[n]
        s[n], ze = env_step(sec["env"], abs(float(y[n])), ze)
    e = exponents(s)
    emax, counts = occupancy(e, d["nh"])
    return dict(ssq=float(ssq), ns=len(xp), emax=emax, counts=counts, y=y, e=e)


def _carry(T, z_end):
    """z_end [nch, S] (end states from zero) -> the true start states [nch, S]: s_0 = 0, s_(c+1) = T s_c + z_c, row r summed
    k ascending, z_c last."""
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


def stats_chunked(x, fs, chunk):
    d = design(fs, chunk)
    sec, ch = d["sections"], d["chunk"]
    xp = _padded(x, d)
    N = len(xp)
    nch = (N + ch - 1) // ch
    X = np.concatenate((xp, np.zeros(nch * ch - N))).reshape(nch, ch)
    live = (np.arange(nch * ch).reshape(nch, ch) < N)                          # the last chunk stops at N
    S = 10 if d["use_lp"] else 5
    # band pass 1
    z = [np.zeros(nch) for _ in range(S)]
    for i in range(ch):
        _, z = band_step(sec, X[:, i], z)
    start = _carry(d["t_band"], np.stack(z, axis=1))
    # band pass 2, energy, envelope pass 1
    z, ze = [start[:, k].copy() for k in range(S)], [np.zeros(nch), np.zeros(nch)]
    Y, part = np.zeros((nch, ch)), np.zeros(nch)
    for i in range(ch):
        Y[:, i], z = band_step(sec, X[:, i], z)
        part = np.where(live[:, i], part + Y[:, i] * Y[:, i], part)
        _, ze = env_step(sec["env"], np.abs(Y[:, i]), ze)
    ssq = 0.0
    for c in range(nch):
        ssq = ssq + float(part[c])
    estart = _carry(d["t_env"], np.stack(ze, axis=1))
    # envelope pass 2 (the band filter's second run repeats Y bit for bit)
    ze, Sg = [estart[:, 0].copy(), estart[:, 1].copy()], np.zeros((nch, ch))
    for i in range(ch):
        Sg[:, i], ze = env_step(sec["env"], np.abs(Y[:, i]), ze)
    e = exponents(Sg.reshape(-1)[:N])
    emax, counts = occupancy(e, d["nh"])
    return dict(ssq=float(ssq), ns=N, emax=emax, counts=counts, y=Y.reshape(-1)[:N], e=e)


def level(ssq, ns, emax, counts):
    """The level of one utterance from its statistics: the first crossing of the 15.9 dB margin, interpolated."""
    long_term = ssq / ns if ns > 0 else 0.0
    if not ssq > 0 or emax <= EMPTY + 1:
        return dict(level=0.0, level_db=-math.inf, long_term=long_term, activity=0.0)
    kc = np.cumsum(np.asarray(counts, dtype=np.float64))
    aj = [10.0 * math.log10(ssq / k) if k > 0 else math.inf for k in kc]
    mj = [aj[j] - 10.0 * math.log10(2.0) * (emax - (j + 1) - 1) - MARGIN_DB for j in range(NBIN)]
    jj = next((j for j in range(NBIN - 1) if mj[j] < 0 <= mj[j + 1]), None)
    if jj is None:
        jj, jf = (NBIN - 2, 1.0) if mj[-1] <= 0 else (0, 0.0)
    else:
        jf = 1.0 / (1.0 - mj[jj + 1] / mj[jj])
    lev = aj[jj] + (jf * (aj[jj + 1] - aj[jj]) if jf != 0.0 else 0.0)
    lp = 10.0 ** (lev / 10.0)
    return dict(level=lp, level_db=lev, long_term=long_term, activity=ssq / (ns * lp))


def scipy_band(x, fs):
    """The band filter as scipy.signal.lfilter sections over the padded utterance."""
    from scipy.signal import lfilter
    d = design(fs, 1)
    sec = d["sections"]
    y = lfilter(sec["hp1"][:2], [1.0, sec["hp1"][2]], _padded(x, d))
    for name in ("bq1", "bq2"):
        y = lfilter(sec[name][:3], [1.0, sec[name][3], sec[name][4]], y)
    if sec["lp"] is not None:
        y = lfilter(sec["lp"][:6], np.concatenate(([1.0], sec["lp"][6:])), y)
    return y


def scipy_envelope(y, fs):
    from scipy.signal import lfilter
    b0, a1, a2 = design(fs, 1)["sections"]["env"]
    return lfilter([b0], [1.0, a1, a2], np.abs(y))


def bursts(rng, n, amp=0.1):
    """Seeded noise in bursts of 40 .. 400 ms-at-8-kHz with pauses between them."""
    x, at, on = np.zeros(n), 0, True
    while at < n:
        run = int(rng.integers(300, 3200))
        if on:
            x[at:at + run] = amp * rng.standard_normal(len(x[at:at + run]))
        at, on = at + run, not on
    return x.astype(np.float32)


def cases(fs, chunk):
    """-> list of (name, float32 array): every length at which the device takes another path, and the contents the issue lists
    (plus one row that starts with 2 nh zeros: -inf exponents under a finite emax, which the 1e-30 row does not reach in fp64)."""
    d = design(fs, 1)
    nz, nh, ch = d["nz"], d["nh"], int(chunk)
    rng = np.random.default_rng(fs)
    noise = lambda n: (0.1 * rng.standard_normal(n)).astype(np.float32)
    base = bursts(rng, 3 * nh)
    lead = np.concatenate((np.zeros(2 * nh, dtype=np.float32), noise(700)))
    return [
        ("len1", noise(1)), ("len2", noise(2)), ("ch-1", bursts(rng, ch - 1)), ("ch_zero", np.zeros(ch, dtype=np.float32)),
        ("ch+1_dc", np.full(ch + 1, 0.25, dtype=np.float32)),
        ("pad0_tiny", (1e-30 * np.sign(rng.standard_normal((-nz) % ch + ch))).astype(np.float32)),
        ("pad1_int16", np.round(32768.0 * np.clip(0.3 * rng.standard_normal((1 - nz) % ch), -1, 1)).astype(np.float32)),
        ("pad-1", noise((-1 - nz) % ch)), ("3nh", base), ("3nh_x1024", (base * np.float32(1024.0)).astype(np.float32)),
        ("long", bursts(rng, 20000)), ("lead_zeros", lead),
    ]
