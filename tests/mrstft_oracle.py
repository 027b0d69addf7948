"""numpy float64 restatement of the multi-resolution STFT loss (conv_tasnet_amd.mrstft, csrc/ctn_mrstft.hip): the three terms of
one (reference, estimate) pair at one resolution through np.fft.rfft on the gathered frames, the analytic gradient with respect
to the estimate, and the conditions on a test's inputs that keep it away from the two kinks of the loss.

A resolution is (n_fft, hop, win_length).  The frames are torch.stft's with center=True, pad_mode='reflect' on the row's own n
samples: frame f covers padded samples f hop .. f hop + n_fft - 1, f = 0 .. n // hop; the periodic Hann window of win_length points
sits (n_fft - win_length) // 2 taps into the frame."""
import numpy as np

EPS = 1e-7
DEFAULT_RESOLUTIONS = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))


def window(n_fft, win):
    w = np.zeros(n_fft)
    off = (n_fft - win) // 2
    w[off:off + win] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win) / win)
    return w


def frame_index(n, n_fft, hop):
    """-> [F, n_fft] int64: the sample under every tap of every frame, reflected about samples 0 and n - 1 (n > n_fft / 2)."""
    F = 1 + n // hop
    j = np.arange(F)[:, None] * hop + np.arange(n_fft)[None, :] - n_fft // 2
    j = np.where(j < 0, -j, j)
    j = np.where(j >= n, 2 * (n - 1) - j, j)
    assert j.min() >= 0 and j.max() < n
    return j


def spectra(x, res):
    """x [n] -> the complex spectrogram [F, n_fft/2+1] of the row"""
    n_fft, hop, win = res
    x = np.asarray(x, dtype=np.float64)
    return np.fft.rfft(x[frame_index(x.shape[0], n_fft, hop)] * window(n_fft, win)[None, :], axis=1)


def run(ref, est, res, g=(1.0, 1.0, 0.0), eps=EPS):
    """ref, est [n] -> dict: terms (sc, logmag, linmag), grad [n] = d (g . terms) / d est, and the margins of conditions().
    n <= n_fft / 2: everything zero."""
    n_fft, hop, win = res
    ref, est = np.asarray(ref, dtype=np.float64), np.asarray(est, dtype=np.float64)
    n = ref.shape[0]
    if n <= n_fft // 2:
        return dict(terms=np.zeros(3), grad=np.zeros(n), clamp_margin=np.inf, equal_margin=np.inf, clamped=0, frames=0)
    idx = frame_index(n, n_fft, hop)
    w = window(n_fft, win)
    S, Y = np.fft.rfft(ref[idx] * w, axis=1), np.fft.rfft(est[idx] * w, axis=1)
    ps, py = S.real ** 2 + S.imag ** 2, Y.real ** 2 + Y.imag ** 2
    a, b = np.sqrt(np.maximum(ps, eps)), np.sqrt(np.maximum(py, eps))
    D, A, M = ((a - b) ** 2).sum(), (a ** 2).sum(), a.size
    sc = np.sqrt(D) / np.sqrt(A) if D > 0 else 0.0
    terms = np.array([sc, np.abs(np.log(a) - np.log(b)).mean(), np.abs(a - b).mean()])
    # d / d|S^| per bin, through the clamp (a clamped bin passes nothing), then d|S^| / dS^ = S^ / |S^|
    sg = np.sign(b - a)
    c = (g[0] * (b - a) / (np.sqrt(D) * np.sqrt(A)) if D > 0 else 0.0) + sg * (g[1] / (M * b) + g[2] / M)
    G = np.where(py >= eps, c / b, 0.0) * Y
    # real-input adjoint: y[m] = Re sum_{k <= N/2} G[k] exp(+2 pi i k m / N) = N irfft(G') with the inner bins halved
    Gh = G.copy()
    Gh[:, 1:n_fft // 2] *= 0.5
    gf = n_fft * np.fft.irfft(Gh, n=n_fft, axis=1) * w[None, :]
    grad = np.zeros(n)
    np.add.at(grad, idx.ravel(), gf.ravel())
    clamp_margin = min(np.abs(ps / eps - 1.0).min(), np.abs(py / eps - 1.0).min())
    equal_margin = (np.abs(a - b) / a).min()
    return dict(terms=terms, grad=grad, clamp_margin=clamp_margin, equal_margin=equal_margin,
                clamped=int((ps < eps).sum() + (py < eps).sum()), frames=idx.shape[0])


def conditions(runs):
    """The inputs of every test case keep away from the kinks: no bin's power within a relative 1e-6 of eps, no bin with
    | |S| - |S^| | < 1e-9 |S|, so a clamp or sign decision cannot differ between two correct computations."""
    cm, em = min(r["clamp_margin"] for r in runs), min(r["equal_margin"] for r in runs)
    assert cm >= 1e-6 and em >= 1e-9, (cm, em)
    return cm, em


def signals(seed, C, E, T):
    """Independent Gaussian references [C,T] and estimates [E,T] = 0.7 ref[e % C] + 0.5 noise, at unit scale, fp32."""
    rng = np.random.RandomState(seed)
    ref = rng.randn(C, T)
    est = np.stack([0.7 * ref[e % C] + 0.5 * rng.randn(T) for e in range(E)])
    return ref.astype(np.float32), est.astype(np.float32)


# ---- the shared cases of the GPU tests: (resolutions, lengths, C, E, T, est_of_ref, seed) ------------------------------------------
ALL_FFT = ((64, 16, 48), (128, 32, 128), (256, 50, 240), (512, 50, 240), (1024, 120, 600), (2048, 240, 1200))
CASES = {
    # every n_fft; win = n_fft, win < n_fft, an odd win; hop > win; R = 8.  Lengths: a multiple of the hops 16, 32 and 64; one more
    # than a multiple of 16, 120 and 240; n_fft / 2 + 1 of 2048, the shortest valid length; n_fft / 2 of 2048 (an empty cell beside
    # seven live ones).  E != C: two references on one estimate row, a row nobody chose.
    "seams": (ALL_FFT + ((256, 64, 255), (128, 200, 100)), (4096, 4081, 1025, 1024), 2, 3, 4096,
              ((2, 0), (1, 1), (0, 2), (2, 2)), 11),
    # hop = 1 with win = 64 (64 frames over every sample), R = 1; the shortest valid length, n = n_fft / 2 and n = 0
    "hop1": (((64, 1, 64),), (600, 33, 32, 0), 1, 1, 600, ((0,), (0,), (0,), (0,)), 12),
    # the default resolutions on ragged rows
    "default": (DEFAULT_RESOLUTIONS, (4000, 2881), 2, 2, 4000, ((1, 0), (0, 1)), 13),
}
_RUNS = {}


def case_inputs(name):
    """-> (ref [B,C,T], est [B,E,T]) fp32 of a shared case, Gaussian beyond the lengths too (the tests overwrite that part)"""
    res, lens, C, E, T, eo, seed = CASES[name]
    pairs = [signals(seed + 100 * b, C, E, T) for b in range(len(lens))]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def case_runs(name, g=(1.0, 1.0, 0.0)):
    """-> {(b, c, r): run(...)} of a shared case under upstream weights g, computed once"""
    if (name, g) not in _RUNS:
        res, lens, C, E, T, eo, seed = CASES[name]
        ref, est = case_inputs(name)
        _RUNS[name, g] = {(b, c, r): run(ref[b, c, :n], est[b, eo[b][c], :n], rr, g)
                          for b, n in enumerate(lens) for c in range(C) for r, rr in enumerate(res)}
    return _RUNS[name, g]


def case_expected(name, g=(1.0, 1.0, 0.0)):
    """-> (terms [B,C,R,3], grad [B,E,T] fp64 of sum over cells of g . terms) of a shared case"""
    res, lens, C, E, T, eo, seed = CASES[name]
    runs = case_runs(name, g)
    terms = np.zeros((len(lens), C, len(res), 3))
    grad = np.zeros((len(lens), E, T))
    for (b, c, r), out in runs.items():
        terms[b, c, r] = out["terms"]
        grad[b, eo[b][c], :lens[b]] += out["grad"]
    return terms, grad


def loss(terms, w_sc=1.0, w_log=1.0, w_lin=0.0):
    """terms [..., R, 3] -> the mean over pairs of the mean over resolutions of the weighted sum"""
    terms = np.asarray(terms)
    return float((w_sc * terms[..., 0] + w_log * terms[..., 1] + w_lin * terms[..., 2]).mean())
