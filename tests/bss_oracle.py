"""Oracle for the GPU BSS Eval: a float64 numpy/scipy restatement of BSS Eval v3 as mir_eval.separation.bss_eval_sources
computes it (v0.7, compute_permutation=True, 512-tap distortion filters), written from its published definition.

Form "fft" is mir_eval's own: correlations by scipy.fftpack FFTs, G c = D by np.linalg.solve (LU; lstsq if that raises),
projections by scipy.signal.fftconvolve, energies from the decomposition signals of _bss_decomp_mtifilt.  Form "direct"
restates the same numbers another way: direct fp64 correlations, a Cholesky solve, explicit time-domain residuals.
Also speech-like test signals (AR(2)-filtered noise under an amplitude envelope)."""
import itertools

import numpy as np
import scipy.fftpack
import scipy.linalg
import scipy.signal

FLEN = 512


def _project_fft(refs, e, flen=FLEN):
    nsrc, n = refs.shape
    refs = np.hstack((refs, np.zeros((nsrc, flen - 1))))
    e = np.hstack((e, np.zeros(flen - 1)))
    n_fft = int(2 ** np.ceil(np.log2(n + flen - 1.0)))
    sf = scipy.fftpack.fft(refs, n=n_fft, axis=1)
    sef = scipy.fftpack.fft(e, n=n_fft)
    G = np.zeros((nsrc * flen, nsrc * flen))
    for i in range(nsrc):
        for j in range(nsrc):
            ssf = np.real(scipy.fftpack.ifft(sf[i] * np.conj(sf[j])))
            ss = scipy.linalg.toeplitz(np.hstack((ssf[0], ssf[-1:-flen:-1])), r=ssf[:flen])
            G[i * flen:(i + 1) * flen, j * flen:(j + 1) * flen] = ss
            G[j * flen:(j + 1) * flen, i * flen:(i + 1) * flen] = ss.T
    D = np.zeros(nsrc * flen)
    for i in range(nsrc):
        ssef = np.real(scipy.fftpack.ifft(sf[i] * np.conj(sef)))
        D[i * flen:(i + 1) * flen] = np.hstack((ssef[0], ssef[-1:-flen:-1]))
    try:
        C = np.linalg.solve(G, D).reshape(flen, nsrc, order="F")
    except np.linalg.LinAlgError:
        C = np.linalg.lstsq(G, D, rcond=None)[0].reshape(flen, nsrc, order="F")
    sproj = np.zeros(n + flen - 1)
    for i in range(nsrc):
        sproj += scipy.signal.fftconvolve(C[:, i], refs[i])[:n + flen - 1]
    return sproj


def corr(a, b, flen=FLEN):
    """r(tau) = sum_t a[t] b[t+tau], tau in [0, flen): direct fp64 sums."""
    n = len(a)
    return np.array([np.dot(a[:n - tau], b[tau:]) if tau < n else 0.0 for tau in range(flen)])


def gram(refs, flen=FLEN):
    """G[iF+a, kF+b] = r_ik(a-b) from direct correlations."""
    nsrc = refs.shape[0]
    G = np.zeros((nsrc * flen, nsrc * flen))
    lag = np.arange(flen)[:, None] - np.arange(flen)[None, :]
    for i in range(nsrc):
        for k in range(nsrc):
            rik, rki = corr(refs[i], refs[k], flen), corr(refs[k], refs[i], flen)
            G[i * flen:(i + 1) * flen, k * flen:(k + 1) * flen] = np.where(lag >= 0, rik[np.clip(lag, 0, None)],
                                                                           rki[np.clip(-lag, 0, None)])
    return G


def _project_direct(refs, e, flen=FLEN):
    nsrc, n = refs.shape
    G = gram(refs, flen)
    D = np.concatenate([corr(refs[i], e, flen) for i in range(nsrc)])
    c = scipy.linalg.cho_solve(scipy.linalg.cho_factor(G, lower=True), D).reshape(nsrc, flen)
    sproj = np.zeros(n + flen - 1)
    for i in range(nsrc):
        sproj += np.convolve(c[i], refs[i])
    return sproj


def _safe_db(num, den):
    return np.inf if den == 0 else 10 * np.log10(num / den)


def bss_matrices(ref, est, form="fft"):
    """ref [C,n], est [E,n] -> sdr, sir, sar [E,C] (row jest of est against reference jtrue)."""
    ref, est = np.asarray(ref, np.float64), np.asarray(est, np.float64)
    C, n = ref.shape
    E = est.shape[0]
    proj = _project_fft if form == "fft" else _project_direct
    out = np.zeros((3, E, C))
    for jest in range(E):
        e = est[jest]
        pall = proj(ref, e)
        for jtrue in range(C):
            s_true = np.hstack((ref[jtrue], np.zeros(FLEN - 1)))
            if form == "fft":
                e_spat = proj(ref[jtrue, np.newaxis, :], e) - s_true
                e_interf = pall - s_true - e_spat
                e_artif = -s_true - e_spat - e_interf
                e_artif[:n] += e
                s_filt = s_true + e_spat
                out[0, jest, jtrue] = _safe_db(np.sum(s_filt ** 2), np.sum((e_interf + e_artif) ** 2))
                out[1, jest, jtrue] = _safe_db(np.sum(s_filt ** 2), np.sum(e_interf ** 2))
                out[2, jest, jtrue] = _safe_db(np.sum((s_filt + e_interf) ** 2), np.sum(e_artif ** 2))
            else:
                pj = proj(ref[jtrue, np.newaxis, :], e)
                ep = np.hstack((e, np.zeros(FLEN - 1)))
                out[0, jest, jtrue] = _safe_db(np.sum(pj ** 2), np.sum((ep - pj) ** 2))
                out[1, jest, jtrue] = _safe_db(np.sum(pj ** 2), np.sum((pall - pj) ** 2))
                out[2, jest, jtrue] = _safe_db(np.sum(pall ** 2), np.sum((ep - pall) ** 2))
    return out[0], out[1], out[2]


def bss_eval_sources(ref, est, form="fft"):
    """-> sdr, sir, sar, popt as mir_eval.separation.bss_eval_sources returns them."""
    sdr, sir, sar = bss_matrices(ref, est, form)
    nsrc = sdr.shape[1]
    perms = list(itertools.permutations(list(range(nsrc))))
    dum = np.arange(nsrc)
    mean_sir = np.array([np.mean(sir[list(p), dum]) for p in perms])
    popt = perms[int(np.argmax(mean_sir))]
    idx = (list(popt), dum)
    return sdr[idx], sir[idx], sar[idx], np.asarray(popt)


def cal_SDRi(src_ref, src_est, mix, form="fft"):
    """src/evaluate.py:76-91."""
    src_anchor = np.stack([mix, mix], axis=0)
    sdr, _, _, _ = bss_eval_sources(src_ref, src_est, form)
    sdr0, _, _, _ = bss_eval_sources(src_ref, src_anchor, form)
    return ((sdr[0] - sdr0[0]) + (sdr[1] - sdr0[1])) / 2


def speech_like(seed, C, n, pole=0.9, sr=8000):
    """C speech-like signals [C,n] fp32: AR(2) noise (complex pole pair of radius `pole`) under a syllable-rate envelope."""
    rng = np.random.RandomState(seed)
    out = np.zeros((C, n))
    t = np.arange(n) / sr
    for c in range(C):
        th = rng.uniform(0.05, 0.6)
        a1, a2 = 2 * pole * np.cos(th), -pole * pole
        x = scipy.signal.lfilter([1.0], [1.0, -a1, -a2], rng.randn(n))
        env = 0.6 + 0.4 * np.sin(2 * np.pi * rng.uniform(2, 6) * t + rng.uniform(0, 6.28)) ** 2
        out[c] = x * env
        out[c] /= np.abs(out[c]).max()
    return out.astype(np.float32)


def mixtures(seed, C, n, pole=0.9, leak=0.2, noise=0.05):
    """(ref [C,n], est [C,n]) fp32: each estimate = its reference, a leak of the others, filtered a little, plus noise."""
    ref = speech_like(seed, C, n, pole)
    rng = np.random.RandomState(seed + 1000)
    est = np.zeros_like(ref, dtype=np.float64)
    for c in range(C):
        x = ref[c] + leak * sum(ref[k] for k in range(C) if k != c)
        x = scipy.signal.lfilter([0.9, 0.1], [1.0], x)
        est[c] = x + noise * rng.randn(n)
    return ref, est.astype(np.float32)
