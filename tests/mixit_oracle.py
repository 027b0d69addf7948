"""numpy fp64 restatement of the MixIT loss (include/ctn_hip.h, "mixture invariant training loss") in the DIRECT form: every one
of the 2^M remixes is built and its error summed sample by sample; no moments.  `moment_form` is the algebra the kernels use
(Gram matrix of the estimates, the assignment decided on scalars), kept here so that the two can be compared in fp64 on the CPU.

    A_n(a) = {i : bit i of a == n}          err_n = sum_{t < len} (sum_{i in A_n} e_i[t] - x_n[t])^2       Xx_n = sum_{t < len} x_n[t]^2
    l_n(a) = 10 log10((err_n + tau Xx_n + EPS) / (Xx_n + EPS))         L(a) = (l_0 + l_1) / 2              tau = 10^(-snr_max / 10)
    assign = the first a (ascending) attaining min L;  per_utt = L(assign);  loss = mean_b per_utt;  snr[n] = -l_n(assign)
    dL/de_i[t] = [t < len] c_n (sum_{k in A_n} e_k[t] - x_n[t]),   c_n = (10 / ln 10) / (err_n + tau Xx_n + EPS),  n = bit i of assign
"""
import numpy as np

EPS = 1e-8
C10 = 10.0 / np.log(10.0)

# (B, M, T) of the GPU cases: odd T (no 16-byte rows), the register-heaviest M = 8, an exact chunk fit, B above a workgroup
SHAPES = [(3, 2, 4133), (3, 3, 4133), (3, 4, 4133), (2, 8, 4133), (5, 4, 8192), (257, 2, 64), (3, 6, 777)]


def threshold(snr_max):
    return 0.0 if snr_max is None else 10.0 ** (-float(snr_max) / 10.0)


def assign_matrices(M):
    """[2^M, 2, M] of 0 / 1: row (a, n) selects the sources of mixture n under assignment a."""
    a = np.arange(1 << M)[:, None]
    bits = (a >> np.arange(M)[None, :]) & 1
    return np.stack((1 - bits, bits), axis=1).astype(np.float64)


def unpack(assign, M):
    return (np.asarray(assign, np.int64)[:, None] >> np.arange(M)[None, :]) & 1


def _clamp(lens, T):
    return np.clip(np.asarray(lens, np.int64), 0, T)


def _pick(L):
    """First minimum in ascending a (strict <), and the margin to the second-best value."""
    a = int(np.argmin(L))                 # numpy returns the first occurrence
    rest = np.delete(L, a)
    return a, float(rest.min() - L[a])


def direct(x, e, lens, snr_max=30.0, g_loss=None, g_per=None):
    """x [B,2,T], e [B,M,T] (any float dtype; computed in fp64), lens [B] -> dict of
    per_utt [B], assign [B], margin [B] (dB, best against second best), snr [B,2], coef [B,2], loss, L [B,2^M],
    grad [B,M,T]: the gradient of g_loss * loss + sum_b g_per[b] * per_utt[b] (g_loss = 1, g_per = 0 when both are None)."""
    x, e = np.asarray(x, np.float64), np.asarray(e, np.float64)
    B, M, T = e.shape
    lens, tau, A = _clamp(lens, T), threshold(snr_max), assign_matrices(M)
    if g_loss is None and g_per is None:
        g_loss = 1.0
    out = dict(per_utt=np.zeros(B), assign=np.zeros(B, np.int64), margin=np.zeros(B), snr=np.zeros((B, 2)), coef=np.zeros((B, 2)),
               L=np.zeros((B, 1 << M)), grad=np.zeros((B, M, T)))
    for b in range(B):
        n = int(lens[b])
        xb, eb = x[b, :, :n], e[b, :, :n]
        res = np.einsum("anm,mt->ant", A, eb) - xb[None]              # every remix, minus its mixture
        err = (res * res).sum(-1)                                     # [2^M, 2]
        xx = (xb * xb).sum(-1)                                        # [2]
        l = 10.0 * np.log10((err + tau * xx + EPS) / (xx + EPS))
        L = l.mean(-1)
        a, margin = _pick(L)
        c = C10 / (err[a] + tau * xx + EPS)
        scale = (0.0 if g_loss is None else float(g_loss) / B) + (0.0 if g_per is None else float(np.asarray(g_per)[b]))
        bits = (a >> np.arange(M)) & 1
        out["grad"][b, :, :n] = scale * c[bits][:, None] * res[a][bits]
        out["per_utt"][b], out["assign"][b], out["margin"][b], out["snr"][b], out["L"][b] = L[a], a, margin, -l[a], L
        out["coef"][b] = c
    out["loss"] = float(out["per_utt"].mean())
    return out


def moments(x, e, lens):
    """fp64 second-order moments over t < len: G [B,M,M] = e e^T, Xe [B,2,M] = x e^T, Xx [B,2]."""
    x, e = np.asarray(x, np.float64), np.asarray(e, np.float64)
    B, M, T = e.shape
    keep = (np.arange(T)[None, :] < _clamp(lens, T)[:, None]).astype(np.float64)[:, None, :]
    xm, em = x * keep, e * keep
    return np.einsum("bit,bkt->bik", em, em), np.einsum("bnt,bit->bni", xm, em), np.einsum("bnt,bnt->bn", xm, xm)


def moment_form(x, e, lens, snr_max=30.0):
    """The kernels' algebra in fp64: err_n(a) = Xx_n - 2 sum_{i in A_n} Xe[n][i] + sum_{i,k in A_n} G[i][k], clamped at 0."""
    G, Xe, Xx = moments(x, e, lens)
    B, M = G.shape[:2]
    tau, A = threshold(snr_max), assign_matrices(M)
    err = Xx[:, None, :] - 2.0 * np.einsum("anm,bnm->ban", A, Xe) + np.einsum("ani,bik,ank->ban", A, G, A)
    err = np.maximum(err, 0.0)
    l = 10.0 * np.log10((err + tau * Xx[:, None, :] + EPS) / (Xx[:, None, :] + EPS))
    L = l.mean(-1)
    assign = np.array([_pick(L[b])[0] for b in range(B)], np.int64)
    per_utt = L[np.arange(B), assign]
    return dict(per_utt=per_utt, assign=assign, snr=-l[np.arange(B), assign], L=L, loss=float(per_utt.mean()))


def make_case(B, M, T, seed, noise=0.03):
    """A planted assignment: e Gaussian with a row scale in [0.05, 0.5], x_n = the planted group's sum + noise * randn, lens in
    [T/2, T] with lens[0] = T.  -> x [B,2,T] f32, e [B,M,T] f32, lens [B] i64, planted [B] (packed; both groups non-empty)."""
    rng = np.random.default_rng(seed)
    e = (rng.standard_normal((B, M, T)) * rng.uniform(0.05, 0.5, (B, M, 1))).astype(np.float32)
    planted = rng.integers(1, (1 << M) - 1, B)                     # neither 0 nor 2^M - 1: both mixtures get a source
    bits = unpack(planted, M).astype(np.float64)
    groups = np.stack((1.0 - bits, bits), axis=1)                  # [B,2,M]
    x = np.einsum("bnm,bmt->bnt", groups, e.astype(np.float64)) + noise * rng.standard_normal((B, 2, T))
    lens = rng.integers(T // 2, T + 1, B).astype(np.int64)
    lens[0] = T
    return x.astype(np.float32), e, lens, planted.astype(np.int64)


def grad_fp32(x, e, lens, assign, coef32, g_loss=None, g_per=None):
    """numpy fp32 emulation of the backward kernel's stated order: both remixes added in ascending source index with one
    rounding per add, one subtraction, w_n = scale_b * coef[b][n] rounded once, d = w_n * r_n."""
    x, e = np.asarray(x, np.float32), np.asarray(e, np.float32)
    B, M, T = e.shape
    lens = _clamp(lens, T)
    out = np.zeros((B, M, T), np.float32)
    for b in range(B):
        scale = np.float32(0.0)
        if g_loss is not None:
            scale = np.float32(np.float32(g_loss) / np.float32(B))
        if g_per is not None:
            scale = np.float32(scale + np.float32(np.asarray(g_per)[b]))
        bits = (int(assign[b]) >> np.arange(M)) & 1
        n = int(lens[b])
        for m in range(2):
            mix = np.zeros(n, np.float32)
            for k in range(M):
                if bits[k] == m:
                    mix = (mix + e[b, k, :n]).astype(np.float32)
            w = np.float32(scale * np.float32(coef32[b][m]))
            r = (mix - x[b, m, :n]).astype(np.float32)
            for i in range(M):
                if bits[i] == m:
                    out[b, i, :n] = (w * r).astype(np.float32)
    return out


def grad_bound(x, e, lens, assign, coef, g_loss=None, g_per=None):
    """(M + 6) 2^-24 |scale_b c_n| (sum_{k in A_n} |e_k[t]| + |x_n[t]|): M - 1 fp32 adds and one subtraction (each at most half
    an ulp of a partial sum bounded by the sum of magnitudes), the rounding of c_n to fp32, of g_loss / B, of the scale sum, of
    scale * c_n and of the final product: M + 5 half-ulps, M + 6 with the second-order terms covered."""
    x, e = np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(e, np.float64))
    B, M, T = e.shape
    out = np.zeros((B, M, T))
    for b in range(B):
        scale = (0.0 if g_loss is None else float(g_loss) / B) + (0.0 if g_per is None else float(np.asarray(g_per)[b]))
        bits = (int(assign[b]) >> np.arange(M)) & 1
        for i in range(M):
            m = bits[i]
            mag = e[b][bits == m].sum(0) + x[b, m]
            out[b, i] = (M + 6) * 2.0 ** -24 * abs(scale * coef[b][m]) * mag
    return out
