"""Closed forms of the cumulative LayerNorm entry points (csrc/ctn_cumln.hip: ctn_cumln_fwd, ctn_cumln_bwd, ctn_cumln_stats_frame,
ctn_cumln_bwd_frame), in plain torch / numpy on the CPU.  Conventions, limits and helpers are tests/norm_oracle.py's (imported, not
copied): tensors are [M, Ch, Kp] WITH the pad frames, fp64 is the reference and fp32 a model of what fp32 arithmetic can reach, every
sum comes with "<name>|abs" and "<name>|terms", PReLU has slope 1 at exactly 0.

    forward :  s1_k = sum_c a[c,k]   s2_k = sum_c a[c,k]^2   n_k = Ch (k0 + k + 1)      (a = prelu(Y); k0 frames came before this call)
               mean_k = C1_k / n_k,  rstd_k = 1 / sqrt(max(C2_k / n_k - mean_k^2, 0) + eps)   (C: prefix sums, carried across calls)
               out = gamma (a - mean_k) rstd_k + beta ;  pad frames: out 0, mean 0, rstd 1 / sqrt(eps)
    backward:  t = gamma dOut, xh = (a - mean_k) rstd_k, p1_k = sum_c t, p2_k = sum_c t xh, u_k = rstd_k p1_k / n_k, v_k = rstd_k^2 p2_k / n_k
               (U, V, W)_j = sum_{j <= k < K} (u_k, v_k, v_k mean_k) ;  da = rstd_j t - U_j + W_j - a V_j ;  dY = da prelu'(Y)
               dgamma = sum dOut xh, dbeta = sum dOut, dalpha = sum_{Y < 0} da Y  over the valid frames
    fc form :  fc = (rstd, mean rstd, U - W + mean V, V / rstd):  xh = a fc0 - fc1,  da = gamma fc0 dOut - fc2 - xh fc3
"""
import collections
import contextlib
import functools
import types

import numpy as np
import torch

import norm_oracle as N
from norm_oracle import ALPHA, EPS, F64, LIMIT, RSTD_PAD, rel_err, sum_err  # noqa: F401  (shared, not copied)

SCAN_BLOCK = 64

# ---- the cases of tests/test_gpu_cumln.py --------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "Ch K Kp M prelu mis alias seed")
WIDTHS, FRAMES = (3, 64, 65, 512), (1, 63, 64, 65, 130, 200)       # frames: either side of the 64-frame scan block, 2 and 3 blocks, ragged


def cases():
    out, n = [], 0
    for Ch in WIDTHS:
        for K in FRAMES:
            out.append(Case(Ch, K, N.padded(K), 2, n % 2 == 0, False, False, N.CHECKED_SEEDS.get(Ch, 0)))
            n += 1
    out.append(Case(65, 130, 192, 3, True, False, False, 0))       # three utterances
    out.append(Case(64, 61, 64, 2, True, True, False, 0))          # rows one float off a 16-byte boundary: the scalar kernels
    out.append(Case(65, 61, 68, 2, False, False, False, 0))        # Kp % 16 != 0: the scalar kernels
    out.append(Case(64, 130, 192, 2, True, False, True, 0))        # dY written over dOut
    return out


# ---- deliberately wrong models ---------------------------------------------------------------------------------------------------
_DEFECT = {}
DEFECTS = ("suffix_j1", "n_chk", "pads_in_suffix", "count_ignored", "var_per_frame")


@contextlib.contextmanager
def defect(name):
    """suffix_j1: the suffix sums start at j + 1.  n_chk: n_k = Ch k.  pads_in_suffix: the pad frames of dOut enter the suffix sums.
    count_ignored: n_k counts this call's frames only (the carried frame count dropped).  var_per_frame: the mean is cumulative, the
    second moment is the frame's own."""
    assert name in DEFECTS
    _DEFECT[name] = True
    try:
        yield
    finally:
        _DEFECT.clear()


def _suffix(t):
    return t.flip(-1).cumsum(-1).flip(-1)


def _n(Ch, Kp, k0, dtype):
    k = torch.arange(Kp, dtype=dtype) + k0
    return Ch * (k.clamp_min(1) if "n_chk" in _DEFECT else k + 1)


# ---- forward -----------------------------------------------------------------------------------------------------------------------
def cumln_fwd(Y, K, gamma, beta, alpha=None, dtype=F64, carry=None):
    """ctn_cumln_fwd -> {out [M,Ch,Kp], mean, rstd [M,Kp], carry}.  carry = (C1 [M], C2 [M], frames) of the calls before, or None."""
    Y, gamma, beta = N._c(dtype, Y, gamma, beta)
    M, Ch, Kp = Y.shape
    ok = N._frames(Y, K)
    a = N._act(Y, alpha)
    s1, s2 = N._sel(ok, a.sum(1)), N._sel(ok, (a * a).sum(1))
    c1, c2, k0 = (torch.zeros(M, dtype=dtype), torch.zeros(M, dtype=dtype), 0) if carry is None else carry
    C1, C2 = s1.cumsum(-1) + c1[:, None].to(dtype), s2.cumsum(-1) + c2[:, None].to(dtype)
    n = _n(Ch, Kp, 0 if "count_ignored" in _DEFECT else k0, dtype)
    mu = C1 / n
    var = ((s2 / Ch if "var_per_frame" in _DEFECT else C2 / n) - mu * mu).clamp_min(0)
    rstd = 1.0 / torch.sqrt(var + EPS)
    out = N._ch(gamma) * ((a - N._frm(mu)) * N._frm(rstd)) + N._ch(beta)
    return {"out": N._sel(ok, out), "mean": N._sel(ok, mu), "rstd": torch.where(ok, rstd, torch.full_like(rstd, RSTD_PAD)),
            "carry": (C1[:, K - 1], C2[:, K - 1], k0 + K)}


def cumln_autograd(y, gamma, beta, alpha=None):
    """The norm as torch.cumsum arithmetic on un-padded [M,Ch,K] tensors: what autograd differentiates.  alpha: tensor or None."""
    Ch, K = y.shape[1], y.shape[2]
    a = y if alpha is None else torch.where(y >= 0, y, alpha * y)
    n = Ch * torch.arange(1, K + 1, dtype=y.dtype)
    mu = a.sum(1).cumsum(-1) / n
    var = ((a * a).sum(1).cumsum(-1) / n - mu * mu).clamp_min(0)
    return gamma.view(1, -1, 1) * (a - mu[:, None]) / torch.sqrt(var[:, None] + EPS) + beta.view(1, -1, 1)


# ---- backward ----------------------------------------------------------------------------------------------------------------------
def frame_sums(dOut, Y, mean, rstd, K, gamma, alpha=None, dtype=F64):
    """(p1, p2) [M,Kp] -- what ctn_pw_dgrad_cln's column partials add up to -- with |abs companions; 0 on the pad frames."""
    dOut, Y, mean, rstd, gamma = N._c(dtype, dOut, Y, mean, rstd, gamma)
    ok = N._frames(Y, K)
    t = N._ch(gamma) * N._sel(ok, dOut)
    tx = t * ((N._act(Y, alpha) - N._frm(mean)) * N._frm(rstd))
    return {"p1": t.sum(1), "p2": tx.sum(1), "p1|abs": t.abs().sum(1), "p2|abs": tx.abs().sum(1)}


def suffix_sums(p1, p2, mean, rstd, K, Ch):
    """(U, V, W) [M,Kp] from the per-frame sums; 0 contributions from the pad frames."""
    ok = N._frames(p1, K)
    n = _n(Ch, p1.shape[-1], 0, p1.dtype)
    u, v = rstd * p1 / n, rstd * rstd * p2 / n
    if "pads_in_suffix" not in _DEFECT:
        u, v = N._sel(ok, u), N._sel(ok, v)
    w = v * mean
    U, V, W = _suffix(u), _suffix(v), _suffix(w)
    if "suffix_j1" in _DEFECT:
        U, V, W = U - u, V - v, W - w
    return U, V, W


def cumln_fc(p1, p2, mean, rstd, K, Ch, dtype=F64):
    """ctn_cumln_bwd_frame -> fc [M,4,Kp]; pad frames: (rstd, 0, 0, 0)."""
    p1, p2, mean, rstd = N._c(dtype, p1, p2, mean, rstd)
    ok = N._frames(p1, K)
    U, V, W = suffix_sums(p1, p2, mean, rstd, K, Ch)
    return torch.stack([rstd, N._sel(ok, mean * rstd), N._sel(ok, U - W + mean * V), N._sel(ok, V / rstd)], 1)


def cumln_bwd(dOut, Y, mean, rstd, K, gamma, alpha=None, dtype=F64, form="closed"):
    """ctn_cumln_bwd + ctn_cln_bwd_finalize -> {dY, dgamma, dbeta [Ch], dalpha [1] (with alpha)} and per sum "|abs" / "|terms".
    form "fc": da through the four per-frame constants, as ctn_dw_bwd_cln and the apply pass compute it."""
    dOut, Y, mean, rstd, gamma = N._c(dtype, dOut, Y, mean, rstd, gamma)
    Ch = Y.shape[1]
    ok = N._frames(Y, K)
    a = N._act(Y, alpha)
    xh = (a - N._frm(mean)) * N._frm(rstd)
    d = N._sel(ok, dOut)
    t = N._ch(gamma) * d
    ts = N._ch(gamma) * dOut.clamp(-1e30, 1e30) if "pads_in_suffix" in _DEFECT else t
    p1, p2 = ts.sum(1), (ts * xh).sum(1)
    if form == "fc":
        fc = cumln_fc(p1, p2, mean, rstd, K, Ch, dtype)
        x2 = a * N._frm(fc[:, 0]) - N._frm(fc[:, 1])
        da = N._ch(gamma) * N._frm(fc[:, 0]) * d - N._frm(fc[:, 2]) - x2 * N._frm(fc[:, 3])
    else:
        U, V, W = suffix_sums(p1, p2, mean, rstd, K, Ch)
        da = N._frm(rstd) * t - N._frm(U) + N._frm(W) - a * N._frm(V)
    out = {"dY": N._sel(ok, da * N._slope(Y, alpha))}
    N._sum3(out, "dgamma", d * xh)
    N._sum3(out, "dbeta", d)
    if alpha is not None:
        N._sum3(out, "dalpha", N._sel(ok, torch.where(Y < 0, da * Y, torch.zeros_like(Y))), dims=(0, 1, 2))
        for n in ("dalpha", "dalpha|abs"):
            out[n] = out[n].reshape(1)
    return out


# ---- the canonical order of the forward scan ---------------------------------------------------------------------------------------
def scan_state():
    return {"P": np.zeros(2), "q": np.zeros(2), "a": 0}


def canonical_scan(s, state=None):
    """s [K,2] fp64 per-frame sums -> C [K,2] in the canonical order: q runs sequentially inside an aligned block of 64 ABSOLUTE frames,
    a finished block is folded into the block prefix P when the next one starts, C = P + q.  state (scan_state(), advanced in place)
    carries (P, q, frames so far) from call to call: the statement the kernel's carry record follows."""
    st = scan_state() if state is None else state
    C = np.empty_like(s)
    for k in range(s.shape[0]):
        if st["a"] % SCAN_BLOCK == 0:
            st["P"] = st["P"] + st["q"]
            st["q"] = np.zeros(2)
        st["q"] = st["q"] + s[k]
        C[k] = st["P"] + st["q"]
        st["a"] += 1
    return C


def blocked_scan(s, state=None):
    """The same values the way the kernel forms them: every touched block's chain on its own (the first continues the carried q), then
    the block totals' prefix in block order."""
    st = scan_state() if state is None else state
    K, a0 = s.shape[0], st["a"]
    o = a0 % SCAN_BLOCK
    P, cq = (st["P"] + st["q"], np.zeros(2)) if o == 0 else (st["P"], st["q"])
    nb = (o + K + SCAN_BLOCK - 1) // SCAN_BLOCK
    q, tot = np.zeros_like(s), []
    for b in range(nb):
        r = cq.copy() if b == 0 else np.zeros(2)
        for i in range(SCAN_BLOCK):
            k = b * SCAN_BLOCK + i - o
            if 0 <= k < K:
                r = r + s[k]
                q[k] = r
        tot.append(r)
    C, p = np.empty_like(s), P
    for b in range(nb):
        lo, hi = max(b * SCAN_BLOCK - o, 0), min((b + 1) * SCAN_BLOCK - o, K)
        C[lo:hi] = p + q[lo:hi]
        if hi == K:
            st["P"], st["q"] = p, q[K - 1].copy()
        p = p + tot[b]
    st["a"] = a0 + K
    return C


def stats_of_scan(C, Ch, a0=0):
    """(mean, rstd) fp64 [K] of prefix sums C [K,2] whose first frame is absolute frame a0."""
    n = Ch * (np.arange(C.shape[0], dtype=np.float64) + a0 + 1)
    mu = C[:, 0] / n
    return mu, 1.0 / np.sqrt(np.maximum(C[:, 1] / n - mu * mu, 0.0) + EPS)


# ---- the inputs --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make_inputs(Ch, K, Kp, M=2, seed=0):
    """norm_oracle.make_inputs' tensors (pad frames of Y exact zeros, of dOut 1e30, a few exact zeros among the valid values, the second
    utterance 20 times quieter) with stats[prelu] = the fp64 CUMULATIVE (mean, rstd), rounded to fp32.  Read-only (cached)."""
    i = types.SimpleNamespace(**vars(N.make_inputs(Ch, K, Kp, M, seed)))
    i.stats = {}
    for pre in (False, True):
        f = cumln_fwd(i.Y, K, i.gamma, i.beta, ALPHA if pre else None)
        i.stats[pre] = (N.r32(f["mean"]), N.r32(f["rstd"]))
    return i


def run_fwd(i, pre, dtype=F64):
    return cumln_fwd(i.Y, i.K, i.gamma, i.beta, i.alpha if pre else None, dtype=dtype)


def run_bwd(i, pre, dtype=F64, form="closed"):
    return cumln_bwd(i.dOut, i.Y, *i.stats[pre], i.K, i.gamma, i.alpha if pre else None, dtype=dtype, form=form)


def errors(got, ref, K):
    """norm_oracle.cln_errors: {figure: (error, limit)} of whatever of out / mean / rstd / dY / dgamma / dbeta / dalpha `got` holds."""
    return N.cln_errors(got, ref, K)


def fc_errors(got, ref):
    """Each of the four fc rows against fp64, relative to the row's largest magnitude (per utterance)."""
    return {"fc%d" % r: (rel_err(got[:, r], ref[:, r], "utt"), LIMIT["mean"]) for r in range(4)}


# ---- a TemporalBlock with the cumulative norm, from oracle.ctn_oracle's pieces ---------------------------------------------------------
def temporal_block(O, cfg, x, sd, xi):
    """oracle.ctn_oracle.temporal_block with cumln_autograd in place of norm()."""
    k = O.block_keys(cfg, 0, xi)
    h = O.pointwise(x, sd[k["w1"]])
    h = cumln_autograd(O.prelu(h, sd[k["a1"]]), sd[k["g1"]], sd[k["b1"]])
    h = O.depthwise(h, sd[k["dw"]], 2 ** xi, cfg.causal)
    h = cumln_autograd(O.prelu(h, sd[k["a2"]]), sd[k["g2"]], sd[k["b2"]])
    return x + O.pointwise(h, sd[k["w2"]])
