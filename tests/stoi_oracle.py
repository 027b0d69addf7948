"""Oracle for the GPU STOI / ESTOI (csrc/ctn_stoi.hip, stoi.py): the short-time objective intelligibility measure of
C. H. Taal, R. C. Hendriks, R. Heusdens and J. Jensen, "An Algorithm for Intelligibility Prediction of Time-Frequency Weighted
Noisy Speech", IEEE TASLP 19(7), 2011, and its extension of J. Jensen and C. H. Taal, "An Algorithm for Predicting the
Intelligibility of Speech Masked by Modulated Noise Maskers", IEEE/ACM TASLP 24(11), 2016, restated in float64 numpy from the
published algorithm with the conventions of the authors' MATLAB code and of pystoi (strict framing, hanning(258)[1:-1],
silent-frame removal by the clean signal's frame energies, 1e-5 for fewer than 30 frames).  No GPU, no import of the package.

    stoi(x, y, fs_sig, extended=False, form="fft") -> float
    details(x, y, fs_sig, form="fft")              -> dict: stoi, estoi, M, K, frames, energies, threshold, keep, index,
                                                      env_x, env_y [15, M], clipped (share of clipped cells), margin (dB)

form "fft" takes the 512-point spectra with np.fft.rfft, form "dft" with an explicit cos / sin DFT-matrix product.  Signals at
another rate are first brought to 10 kHz by the project's own resampler (resample_oracle.resample_f32 with design_filter(up,
down) at its defaults: float32 out, widened to float64), which is the only place where this differs from pystoi.
"""
import math

import numpy as np

import resample_oracle as RO

FS = 10000
N_FRAME = 256
HOP = 128
NFFT = 512
NUMBAND = 15
MINFREQ = 150
N = 30
BETA = -15.0
DYN_RANGE = 40
EPS = np.finfo(np.float64).eps
WINDOW = np.hanning(N_FRAME + 2)[1:-1]
TOO_SHORT = 1e-5


def band_table():
    """[(first bin, width)] of the 15 third-octave bands over the bins f = k * FS / NFFT, k = 0 .. NFFT / 2."""
    f = np.linspace(0, FS, NFFT + 1)[:NFFT // 2 + 1]
    k = np.arange(NUMBAND, dtype=np.float64)
    lo = MINFREQ * 2.0 ** ((2 * k - 1) / 6)
    hi = MINFREQ * 2.0 ** ((2 * k + 1) / 6)
    out = []
    for a, b in zip(lo, hi):
        i0, i1 = int(np.argmin(np.square(f - a))), int(np.argmin(np.square(f - b)))
        out.append((i0, i1 - i0))
    return out


def resample_10k(x, fs_sig):
    """float32 [n] at fs_sig -> float64 [ceil(n * 10000 / fs_sig)] holding the float32 outputs of the project's resampler."""
    x = np.asarray(x, dtype=np.float32)
    if int(fs_sig) == FS:
        return x.astype(np.float64)
    g = math.gcd(int(fs_sig), FS)
    up, down = FS // g, int(fs_sig) // g
    h, W = RO.design_filter(up, down)
    return RO.resample_f32(x, up, down, h, W).astype(np.float64)


def frame_count(n):
    """Frames start at i = 0, 128, ... with i < n - 256, strictly: the frame that ends exactly at the last sample is dropped."""
    return len(range(0, int(n) - N_FRAME, HOP))


def frames_of(x):
    """-> [frame_count(len(x)), 256] windowed frames."""
    starts = range(0, len(x) - N_FRAME, HOP)
    if len(starts) == 0:
        return np.zeros((0, N_FRAME))
    return np.stack([WINDOW * x[i:i + N_FRAME] for i in starts])


def frame_energies(x):
    """20 log10(||windowed frame||_2 + EPS) of every first-pass frame."""
    return 20 * np.log10(np.linalg.norm(frames_of(x), axis=1) + EPS)


def remove_silent(x, y):
    """-> (x', y', kept frame indices, energies, threshold): frames whose clean energy is not above max - 40 dB are dropped
    from both signals, the rest overlap-added at hop 128."""
    xf, yf = frames_of(x), frames_of(y)
    if len(xf) == 0:
        return np.zeros(0), np.zeros(0), np.zeros(0, np.int64), np.zeros(0), -np.inf
    en = 20 * np.log10(np.linalg.norm(xf, axis=1) + EPS)
    thr = np.max(en) - DYN_RANGE
    idx = np.nonzero(en > thr)[0]
    K = len(idx)
    xs, ys = np.zeros((K - 1) * HOP + N_FRAME), np.zeros((K - 1) * HOP + N_FRAME)
    for j, i in enumerate(idx):
        xs[j * HOP:j * HOP + N_FRAME] += xf[i]
        ys[j * HOP:j * HOP + N_FRAME] += yf[i]
    return xs, ys, idx, en, thr


_DFT = {}


def _spectra_power(fr, form):
    """[M, 256] windowed frames -> |X|^2 [M, 257] of the 512-point DFT."""
    if form == "fft":
        X = np.fft.rfft(fr, n=NFFT, axis=1)
        return X.real ** 2 + X.imag ** 2
    if "cs" not in _DFT:
        ang = 2 * np.pi * ((np.arange(NFFT // 2 + 1)[:, None] * np.arange(N_FRAME)[None, :]) % NFFT) / NFFT
        _DFT["cs"] = (np.cos(ang), np.sin(ang))
    c, s = _DFT["cs"]
    re, im = fr @ c.T, fr @ s.T
    return re ** 2 + im ** 2


def envelopes(x, form="fft"):
    """Third-octave band envelopes [15, M] of a (compacted) 10 kHz signal."""
    fr = frames_of(x)
    if len(fr) == 0:
        return np.zeros((NUMBAND, 0))
    p = _spectra_power(fr, form)
    return np.stack([np.sqrt(p[:, a:a + w].sum(axis=1)) for a, w in band_table()])


def _segments(e):
    """[15, M] -> [M - 29, 15, 30]"""
    return np.stack([e[:, m:m + N] for m in range(e.shape[1] - N + 1)])


def _stoi_d(ex, ey):
    xs, ys = _segments(ex), _segments(ey)
    scale = np.linalg.norm(xs, axis=2, keepdims=True) / (np.linalg.norm(ys, axis=2, keepdims=True) + EPS)
    yn = ys * scale
    clip = 10 ** (-BETA / 20)
    bound = xs * (1 + clip)
    yp = np.minimum(yn, bound)
    clipped = float(np.mean(yn > bound))
    yp = yp - yp.mean(axis=2, keepdims=True)
    xc = xs - xs.mean(axis=2, keepdims=True)
    yp = yp / (np.linalg.norm(yp, axis=2, keepdims=True) + EPS)
    xc = xc / (np.linalg.norm(xc, axis=2, keepdims=True) + EPS)
    return float(np.sum(yp * xc) / (xs.shape[0] * NUMBAND)), clipped


def _row_col_normalize(s):
    s = s - s.mean(axis=2, keepdims=True)
    s = s / (np.linalg.norm(s, axis=2, keepdims=True) + EPS)
    s = s - s.mean(axis=1, keepdims=True)
    return s / (np.linalg.norm(s, axis=1, keepdims=True) + EPS)


def _estoi_d(ex, ey):
    xn, yn = _row_col_normalize(_segments(ex)), _row_col_normalize(_segments(ey))
    return float(np.sum(xn * yn / N) / xn.shape[0])


def details(x, y, fs_sig, form="fft"):
    x, y = np.asarray(x), np.asarray(y)
    if x.shape != y.shape or x.ndim != 1:
        raise ValueError("x and y should be 1-D and have the same length, got %s and %s" % (x.shape, y.shape))
    x10, y10 = resample_10k(x, fs_sig), resample_10k(y, fs_sig)
    xs, ys, idx, en, thr = remove_silent(x10, y10)
    ex, ey = envelopes(xs, form), envelopes(ys, form)
    out = {"frames": frame_count(len(x10)), "K": len(idx), "M": ex.shape[1], "index": idx, "energies": en, "threshold": thr,
           "keep": en > thr, "env_x": ex, "env_y": ey, "n10": len(x10),
           "margin": float(np.min(np.abs(en - thr))) if len(en) else np.inf}
    if ex.shape[1] < N:
        out.update(stoi=TOO_SHORT, estoi=TOO_SHORT, clipped=0.0)
    else:
        d, clipped = _stoi_d(ex, ey)
        out.update(stoi=d, estoi=_estoi_d(ex, ey), clipped=clipped)
    return out


def stoi(x, y, fs_sig, extended=False, form="fft"):
    """pystoi's call form: x the clean signal, y the processed one, both 1-D at fs_sig -> d."""
    return details(x, y, fs_sig, form)["estoi" if extended else "stoi"]


# ---- test signals ---------------------------------------------------------------------------------------------------------
def case_signals(n, kind, seed, C=2):
    """(ref [C,n], est [C,n]) fp32 from bss_oracle.mixtures.  'pause': a span of n/6 samples from n/3 scaled by 1e-4 in every
    row (frames inside it are silent and removed); 'dips': the reference scaled by 0.03 over 400-sample spans every n/5
    samples while the estimate comes from the undipped signal (its cells there exceed the clipping bound); 'plain': as is."""
    import bss_oracle as BO
    ref, est = BO.mixtures(seed, C, n)
    ref, est = ref.copy(), est.copy()
    if kind == "pause":
        a, b = n // 3, n // 3 + n // 6
        ref[:, a:b] *= np.float32(1e-4)
        est[:, a:b] *= np.float32(1e-4)
    elif kind == "dips":
        for a in range(n // 10, n - 400, n // 5):
            ref[:, a:a + 400] *= np.float32(0.03)
    elif kind != "plain":
        raise ValueError(kind)
    return ref, est


# (fs, n, kind, seed) of the end-to-end cases shared by the CPU and the GPU tests
CASES = [(10000, 7000, "pause", 1), (8000, 8000, "pause", 7), (8000, 8000, "dips", 1), (16000, 12000, "pause", 1),
         (8000, 16003, "dips", 7), (8000, 3300, "plain", 1), (8000, 3100, "plain", 1)]
