"""Oracle for the image-source room simulator (csrc/ctn_ism.hip) and the same-room RIR draw: the contract of include/ctn_hip.h
("image-source room simulator") restated in pure numpy, written from that text.  No GPU, no import of the package.

    lattice_bounds(L, n_taps, fs, c)                  -> N[3]
    power_table(beta, K)                              -> pw [6][K] by the repeated product
    fractional_delay(Q, W)                            -> frac [Q][2W]
    images(room, src, n_taps, fs, c, Q)               -> dict(amp, i, q, tau) of the lattice in index order (all of it)
    simulate(room, src, n_taps, fs, ...)              -> h [n_taps] float64, additions in ascending image index (vectorised)
    simulate_loop(...)                                -> the same, one Python loop over images and taps (tiny cases)
    simulate_exact(room, src, n_taps, fs, c, W)       -> (h, bound_sum): exact delays, no table; sum |amp| of the images touching a tap
    plan_rooms(seed, rank, epoch, step, B, C, G, P)   -> plan_rir [B, C] int32

A room is a dict(L [3], mic [3], beta [6]); every array is float64.
"""
import numpy as np

import dynmix_oracle as DO

C_SOUND = 343.0
FOUR_PI = 4.0 * np.pi


def lattice_bounds(L, n_taps, fs, c=C_SOUND):
    return [int(np.ceil(n_taps / fs * c / (2.0 * float(L[a])))) + 1 for a in range(3)]


def power_table(beta, K):
    pw = np.ones((6, K), np.float64)
    for w in range(6):
        for k in range(1, K):
            pw[w, k] = pw[w, k - 1] * np.float64(beta[w])
    return pw


def window(x, W):
    """sinc(x) * 0.5 * (1 + cos(pi x / W)), 0 where |x| >= W."""
    x = np.asarray(x, np.float64)
    return np.where(np.abs(x) < W, np.sinc(x) * 0.5 * (1.0 + np.cos(np.pi * x / W)), 0.0)


def fractional_delay(Q, W):
    j = np.arange(2 * W, dtype=np.float64)[None, :]
    q = np.arange(Q, dtype=np.float64)[:, None]
    return np.ascontiguousarray(window((j - W + 1) - q / Q, W))


def images(room, src, n_taps, fs, c=C_SOUND, Q=1024):
    """Every lattice entry in index order: nx outermost, then ny, nz, p = 4 px + 2 py + pz innermost."""
    L, mic, beta = (np.asarray(room[k], np.float64) for k in ("L", "mic", "beta"))
    src = np.asarray(src, np.float64)
    N = lattice_bounds(L, n_taps, fs, c)
    pw = power_table(beta, max(N) + 2)
    fs_over_c = np.float64(fs) / np.float64(c)
    nx, ny, nz, p = np.meshgrid(np.arange(-N[0], N[0] + 1), np.arange(-N[1], N[1] + 1), np.arange(-N[2], N[2] + 1), np.arange(8),
                                indexing="ij")
    n = [nx.reshape(-1), ny.reshape(-1), nz.reshape(-1)]
    p = p.reshape(-1)
    par = [p >> 2, (p >> 1) & 1, p & 1]
    Rv = [((1.0 - 2.0 * par[a]) * src[a] - mic[a]) + (2.0 * n[a]) * L[a] for a in range(3)]
    d2 = (Rv[0] * Rv[0] + Rv[1] * Rv[1]) + Rv[2] * Rv[2]
    d = np.sqrt(d2)
    b = [pw[2 * a][np.abs(n[a] - par[a])] * pw[2 * a + 1][np.abs(n[a])] for a in range(3)]
    amp = ((b[0] * b[1]) * b[2]) / (d * FOUR_PI)
    tau = d * fs_over_c
    i = np.floor(tau)
    q = np.floor((tau - i) * np.float64(Q)).astype(np.int64)
    assert q.max() < Q
    return dict(amp=amp, i=i.astype(np.int64), q=q, tau=tau, N=N)


def simulate(room, src, n_taps, fs, c=C_SOUND, Q=1024, W=8, frac=None):
    frac = fractional_delay(Q, W) if frac is None else np.asarray(frac, np.float64)
    assert frac.shape == (Q, 2 * W)
    im = images(room, src, n_taps, fs, c, Q)
    live = im["i"] < n_taps
    amp, i, q = im["amp"][live], im["i"][live], im["q"][live]
    k = i[:, None] + np.arange(2 * W)[None, :] - W + 1                       # [images, 2W], row-major = image order per tap
    v = amp[:, None] * frac[q]
    ok = (k >= 0) & (k < n_taps)
    h = np.zeros(n_taps, np.float64)
    np.add.at(h, k[ok], v[ok])                                               # unbuffered, in the order of the index array
    return h


def simulate_loop(room, src, n_taps, fs, c=C_SOUND, Q=1024, W=8, frac=None):
    frac = fractional_delay(Q, W) if frac is None else np.asarray(frac, np.float64)
    im = images(room, src, n_taps, fs, c, Q)
    h = np.zeros(n_taps, np.float64)
    for amp, i, q in zip(im["amp"], im["i"], im["q"]):
        if i >= n_taps:
            continue
        for j in range(2 * W):
            k = int(i) + j - W + 1
            if 0 <= k < n_taps:
                h[k] = h[k] + amp * frac[q, j]
    return h


def simulate_exact(room, src, n_taps, fs, c=C_SOUND, W=8):
    """Exact delays: tap k receives amp * sinc(k - tau) * window(k - tau).  Also sum |amp| over the images touching each tap."""
    im = images(room, src, n_taps, fs, c, 1)
    live = im["i"] < n_taps
    amp, i, tau = im["amp"][live], im["i"][live], im["tau"][live]
    k = i[:, None] + np.arange(2 * W)[None, :] - W + 1
    v = amp[:, None] * window(k - tau[:, None], W)
    ok = (k >= 0) & (k < n_taps)
    h, s = np.zeros(n_taps, np.float64), np.zeros(n_taps, np.float64)
    np.add.at(h, k[ok], v[ok])
    np.add.at(s, k[ok], np.broadcast_to(np.abs(amp)[:, None], k.shape)[ok])
    return h, s


def plan_rooms(seed, rank, epoch, step, B, C, G, P):
    assert 0 <= seed < 1 << 48 and 0 <= rank < 1 << 16 and C <= P <= 64
    key = (seed & DO.MASK, (seed >> 32) | (rank << 16))
    plan = np.zeros((B, C), np.int32)
    for b in range(B):
        g = DO.below(DO.philox4x32((512, b, step, epoch), key)[0], G)
        free = list(range(P))
        for c in range(C):
            kc = DO.below(DO.philox4x32((c + 512, b, step, epoch), key)[1], P - c)
            plan[b, c] = g * P + free.pop(kc)
    return plan
