"""numpy fp64 restatement of PIT with inactive sources (include/ctn_hip.h, "PIT with inactive sources") in three forms.

`direct` builds every pair's difference e_i - s_j and sums its square sample by sample: no moments.  `moment_form` is the algebra
the kernels use (err_ij = Ss_j - 2 Es_ij + Ee_i, clamped at 0), kept here so that the two can be compared in fp64 on the CPU.
`direct` also returns the gradient, and `grad_bound` the elementwise limit of the fp32 backward pass.

    Ss_j = sum_{t < len} s_j^2     Ee_i = sum e_i^2     Xx = sum_t (sum_j s_j[t])^2  (ascending j)     active_j = Ss_j > 0
    active:    l_ij = 10 log10((err_ij + tau Ss_j + EPS) / (Ss_j + EPS)),   err_ij = sum (e_i - s_j)^2,   tau  = 10^(-snr_max / 10)
    inactive:  l_ij = 10 log10((Ee_i + tau0 Xx + EPS) / (Xx + EPS)),                                      tau0 = 10^(-inactive_snr_max / 10)
    L(p) = (sum_i l_{i,p(i)}) / C, added in ascending i;  idx = the first p of itertools.permutations(range(C)) attaining min L
    per_utt = L(idx);  loss = mean_b per_utt
    dL/de_i[t] = [t < len] (1 / C) c_i (e_i[t] - a_i s_j[t]),  j = p(i),  c_i = (20 / ln 10) / D_i,  D_i = the numerator argument
"""
import itertools

import numpy as np

EPS = 1e-8
C20 = 20.0 / np.log(10.0)

# (B, C, T) of the GPU cases: odd T (no 16-byte rows), more than two chunks, an exact chunk fit, the register-heaviest C = 6, B above
# one workgroup of waves
SHAPES = [(4, 2, 4133), (4, 3, 4133), (5, 4, 4133), (3, 6, 777), (2, 5, 2049), (5, 3, 8192), (257, 2, 64)]


def threshold(snr_max):
    return 0.0 if snr_max is None else 10.0 ** (-float(snr_max) / 10.0)


def perm_table(C):
    """[C!, C]: perm[i] = j pairs estimate i with reference j."""
    return np.array(list(itertools.permutations(range(C))), dtype=np.int64)


def _clamp(lens, T):
    return np.clip(np.asarray(lens, np.int64), 0, T)


def _mixture_energy(sb):
    mix = np.zeros(sb.shape[1])
    for j in range(sb.shape[0]):                                       # ascending j
        mix = mix + sb[j]
    return float((mix * mix).sum())


def _pair_losses(err, ss, ee, xx, tau, tau0):
    """err [C,C] (estimate i, reference j) -> l [C,C], D [C,C], active [C]."""
    active = ss > 0
    d_act = err + tau * ss[None, :] + EPS
    d_in = np.broadcast_to((ee + tau0 * xx + EPS)[:, None], err.shape)
    D = np.where(active[None, :], d_act, d_in)
    den = np.where(active, ss + EPS, xx + EPS)[None, :]
    return 10.0 * np.log10(D / den), D, active


def _totals(l, perms):
    C = l.shape[0]
    L = np.zeros(len(perms))
    for k, p in enumerate(perms):
        tot = 0.0
        for i in range(C):                                             # ascending i, one fp64 add each
            tot = tot + l[i, p[i]]
        L[k] = tot / C
    return L


def tie_key(p, active):
    """The tie class of a permutation: its mapping on active references and the set of outputs sent to inactive ones."""
    return tuple(int(j) if active[j] else -1 for j in p)


def _pick(L, perms, active):
    """First minimum in table order (strict <) and the margin to the best permutation outside the winner's tie class (inf when
    every permutation is in it)."""
    k = int(np.argmin(L))                                              # numpy returns the first occurrence
    key = tie_key(perms[k], active)
    others = [L[q] for q in range(len(perms)) if tie_key(perms[q], active) != key]
    return k, (float(min(others) - L[k]) if others else float("inf"))


def _scale(B, b, g_loss, g_per):
    return (0.0 if g_loss is None else float(g_loss) / B) + (0.0 if g_per is None else float(np.asarray(g_per)[b]))


def direct(s, e, lens, snr_max=30.0, inactive_snr_max=20.0, g_loss=None, g_per=None):
    """s, e [B,C,T] (any float dtype; computed in fp64), lens [B] -> dict of per_utt [B], idx [B], margin [B] (dB), pair [B,C,C],
    active [B,C], coef [B,C] (c_i), act_of [B,C] (a_i), ref_of [B,C] (j of estimate i), loss, L [B,C!],
    grad [B,C,T]: the gradient of g_loss * loss + sum_b g_per[b] * per_utt[b] (g_loss = 1, g_per = 0 when both are None)."""
    s, e = np.asarray(s, np.float64), np.asarray(e, np.float64)
    B, C, T = e.shape
    lens, tau, tau0, perms = _clamp(lens, T), threshold(snr_max), threshold(inactive_snr_max), perm_table(C)
    if g_loss is None and g_per is None:
        g_loss = 1.0
    out = dict(per_utt=np.zeros(B), idx=np.zeros(B, np.int64), margin=np.zeros(B), pair=np.zeros((B, C, C)),
               active=np.zeros((B, C), np.int32), coef=np.zeros((B, C)), act_of=np.zeros((B, C)), ref_of=np.zeros((B, C), np.int64),
               L=np.zeros((B, len(perms))), grad=np.zeros((B, C, T)))
    for b in range(B):
        n = int(lens[b])
        sb, eb = s[b, :, :n], e[b, :, :n]
        diff = eb[:, None, :] - sb[None, :, :]                         # [C,C,n]: every estimate minus every reference
        err = (diff * diff).sum(-1)
        ss, ee, xx = (sb * sb).sum(-1), (eb * eb).sum(-1), _mixture_energy(sb)
        l, D, active = _pair_losses(err, ss, ee, xx, tau, tau0)
        L = _totals(l, perms)
        k, margin = _pick(L, perms, active)
        p = perms[k]
        scale = _scale(B, b, g_loss, g_per)
        for i in range(C):
            j = p[i]
            c = C20 / D[i, j]
            a = 1.0 if active[j] else 0.0
            out["coef"][b, i], out["act_of"][b, i], out["ref_of"][b, i] = c, a, j
            out["grad"][b, i, :n] = scale / C * c * (eb[i] - a * sb[j])
        out["per_utt"][b], out["idx"][b], out["margin"][b], out["pair"][b], out["active"][b], out["L"][b] = L[k], k, margin, l, active, L
    out["loss"] = float(out["per_utt"].mean())
    return out


def moments(s, e, lens):
    """fp64 moments over t < len: Es [B,C,C] (estimate i, reference j), Ss [B,C], Ee [B,C], Xx [B]."""
    s, e = np.asarray(s, np.float64), np.asarray(e, np.float64)
    B, C, T = e.shape
    keep = (np.arange(T)[None, :] < _clamp(lens, T)[:, None]).astype(np.float64)[:, None, :]
    sm, em = s * keep, e * keep
    mix = np.zeros((B, T))
    for j in range(C):
        mix = mix + sm[:, j]
    return np.einsum("bit,bjt->bij", em, sm), (sm * sm).sum(-1), (em * em).sum(-1), (mix * mix).sum(-1)


def moment_form(s, e, lens, snr_max=30.0, inactive_snr_max=20.0):
    """The kernels' algebra in fp64: err_ij = max(Ss_j - 2 Es_ij + Ee_i, 0)."""
    Es, Ss, Ee, Xx = moments(s, e, lens)
    B, C = Ss.shape
    tau, tau0, perms = threshold(snr_max), threshold(inactive_snr_max), perm_table(C)
    out = dict(per_utt=np.zeros(B), idx=np.zeros(B, np.int64), pair=np.zeros((B, C, C)), L=np.zeros((B, len(perms))))
    for b in range(B):
        err = np.maximum(Ss[b][None, :] - 2.0 * Es[b] + Ee[b][:, None], 0.0)
        l, D, active = _pair_losses(err, Ss[b], Ee[b], Xx[b], tau, tau0)
        L = _totals(l, perms)
        k, _ = _pick(L, perms, active)
        out["per_utt"][b], out["idx"][b], out["pair"][b], out["L"][b] = L[k], k, l, L
    out["loss"] = float(out["per_utt"].mean())
    return out


def plain_snr_pit(s, e, lens):
    """Every reference active, no threshold, written without the active / inactive machinery: the best mean over the outputs of
    10 log10((Ss_j + EPS) / (err_ij + EPS)) over the permutations -> [B]."""
    s, e = np.asarray(s, np.float64), np.asarray(e, np.float64)
    B, C, T = e.shape
    lens, perms = _clamp(lens, T), perm_table(C)
    out = np.zeros(B)
    for b in range(B):
        n = int(lens[b])
        snr = np.zeros((C, C))
        for i in range(C):
            for j in range(C):
                snr[i, j] = 10.0 * np.log10(((s[b, j, :n] ** 2).sum() + EPS) / (((e[b, i, :n] - s[b, j, :n]) ** 2).sum() + EPS))
        out[b] = max(sum(snr[i, p[i]] for i in range(C)) / C for p in perms)
    return out


def make_case(B, C, T, seed, active_counts=None):
    """Planted: references Gaussian with a row scale in [0.1, 0.5]; utterance b keeps 1 + (b mod C) of them (a drawn subset; or
    active_counts[b]), the others are zeros.  The estimates are a drawn permutation of the references: output i is its reference
    plus noise of 0.03 (1 + i), or noise of 1e-3 (1 + i) alone when the reference is silent.  lens in [T/2, T], lens[0] = T.
    -> s [B,C,T] f32, e [B,C,T] f32, lens [B] i64, planted [B,C] (the reference of output i)."""
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((B, C, T)) * rng.uniform(0.1, 0.5, (B, C, 1))
    planted = np.zeros((B, C), np.int64)
    e = np.zeros((B, C, T))
    for b in range(B):
        n_act = 1 + (b % C) if active_counts is None else int(active_counts[b])
        keep = rng.permutation(C)[:n_act]
        silent = np.setdiff1d(np.arange(C), keep)
        s[b, silent] = 0.0
        planted[b] = rng.permutation(C)
        for i in range(C):
            j = planted[b, i]
            noise = (0.03 if j in keep else 1e-3) * (1 + i)
            e[b, i] = s[b, j] + noise * rng.standard_normal(T)
    lens = rng.integers(T // 2, T + 1, B).astype(np.int64)
    lens[0] = T
    return s.astype(np.float32), e.astype(np.float32), lens, planted


def grad_fp32(s, e, lens, ref, g_loss=None, g_per=None):
    """numpy fp32 emulation of the backward kernel's stated order: scale = g_loss / B (+ g_per[b]), / C, w_i = scale * c_i with c_i
    rounded to fp32, r = e_i - s_j (or e_i for an inactive pairing), d = w_i * r; one rounding each."""
    s, e = np.asarray(s, np.float32), np.asarray(e, np.float32)
    B, C, T = e.shape
    lens = _clamp(lens, T)
    out = np.zeros((B, C, T), np.float32)
    for b in range(B):
        scale = np.float32(0.0)
        if g_loss is not None:
            scale = np.float32(np.float32(g_loss) / np.float32(B))
        if g_per is not None:
            scale = np.float32(scale + np.float32(np.asarray(g_per)[b]))
        scale = np.float32(scale / np.float32(C))
        n = int(lens[b])
        for i in range(C):
            w = np.float32(scale * np.float32(ref["coef"][b, i]))
            r = e[b, i, :n]
            if ref["act_of"][b, i]:
                r = (r - s[b, ref["ref_of"][b, i], :n]).astype(np.float32)
            out[b, i, :n] = (w * r).astype(np.float32)
    return out


def grad_bound(s, e, lens, ref, g_loss=None, g_per=None):
    """8 * 2^-24 |scale_b / C c_i| (|e_i[t]| + a_i |s_j[t]|) from direct()'s result `ref`.  The fp32 backward pass rounds g_loss / B,
    the sum with g_per[b], the division by C, c_i (fp64 -> fp32), the product with c_i, the difference e_i - s_j (at most half an
    ulp of a value bounded by |e_i| + |s_j|) and the final product: 7 half-ulps, 8 with the second-order terms covered."""
    s, e = np.abs(np.asarray(s, np.float64)), np.abs(np.asarray(e, np.float64))
    B, C, T = e.shape
    out = np.zeros((B, C, T))
    if g_loss is None and g_per is None:
        g_loss = 1.0
    for b in range(B):
        scale = _scale(B, b, g_loss, g_per)
        for i in range(C):
            mag = e[b, i] + ref["act_of"][b, i] * s[b, ref["ref_of"][b, i]]
            out[b, i] = 8 * 2.0 ** -24 * abs(scale / C * ref["coef"][b, i]) * mag
    return out
