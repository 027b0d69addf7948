"""numpy fp64 restatement of optimal-assignment PIT (include/ctn_hip.h, "optimal-assignment PIT"), written from the algebra.

    over t < len:  sc_j = s_j - mean s_j,  ec_i = e_i - mean e_i,  dot = sum ec_i sc_j,  En = sum sc_j^2
    proj = dot sc_j / (En + EPS),  noise = ec_i - proj,  ratio = sum proj^2 / (sum noise^2 + EPS),  snr_ij = 10 log10(ratio + EPS)
    perm = argmax over the permutations p of sum_i snr_{i,p(i)};  max_snr = that sum / C;  loss = -mean_b max_snr

`solve` is the shortest-augmenting-path assignment solver the device runs, restated: rows in index order, the first column of
least slack, fp64 additions, subtractions and comparisons only, so that it returns the device's permutation bit for bit, ties
included.  `direct` builds proj and noise sample by sample (no moments), takes the optimum from scipy, and returns the gradient and
the MARGIN: the distance in mean SI-SNR to the best other assignment.  `moment_form` is the algebra the kernels use on raw moments,
kept here so that the two can be compared in fp64 on the CPU.  `grad_bound` is the elementwise limit of the fp32 backward pass.
"""
import numpy as np
from scipy.optimize import linear_sum_assignment

EPS = 1e-8
K10 = 10.0 / np.log(10.0)

# (B, C, T) of the GPU cases.  T = 4133: no row but the first is 16-byte aligned; T = 8192: aligned rows, several chunks; T = 129 =
# 32 * 4 + 1: a tail of one sample beyond the MFMA's k-step; T = 64 with len >= 32: one short chunk; C = 16: a full tile, C = 7, 11,
# 13: zero rows in the tile; B = 257: more utterances than one pass of waves
SHAPES = [(4, 2, 4133), (3, 7, 777), (2, 11, 2049), (3, 16, 4133), (2, 16, 8192), (5, 16, 129), (3, 13, 64), (257, 2, 64)]


def _clamp(lens, T):
    return np.clip(np.asarray(lens, np.int64), 0, T)


def solve(score, maximize=True):
    """score [C,C] or [N,C,C] -> perm [C] or [N,C] int64, perm[i] = the column of row i.  The device's solver step by step: every
    loop has a trip count fixed by C, and the first minimum is taken by a strict `<` in ascending column order."""
    score = np.asarray(score, np.float64)
    if score.ndim == 3:
        return np.stack([solve(m, maximize) for m in score]) if len(score) else np.zeros((0, score.shape[1]), np.int64)
    C = score.shape[0]
    c = -score if maximize else score
    u, v, p = np.zeros(C), np.zeros(C), -np.ones(C, np.int64)          # p[j]: the row matched to column j
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(C):
            minv, way = np.full(C, np.inf), -np.ones(C, np.int64)
            used, intree = np.zeros(C, bool), np.zeros(C, bool)
            intree[i] = True
            j0, i0, done = -1, i, False
            for _ in range(C):
                if done:
                    continue
                if j0 >= 0:
                    used[j0] = True
                best = -1
                for j in range(C):
                    if used[j]:
                        continue
                    cur = (c[i0, j] - u[i0]) - v[j]
                    if cur < minv[j]:
                        minv[j], way[j] = cur, j0
                    if best < 0 or minv[j] < minv[best]:
                        best = j
                delta = minv[best]
                u[intree] += delta
                v[used] -= delta
                minv[~used] -= delta
                j0 = best
                i0 = p[j0]
                done = i0 < 0
                if not done:
                    intree[i0] = True
            for _ in range(C):
                if j0 < 0:
                    continue
                j1 = way[j0]
                p[j0] = i if j1 < 0 else p[j1]
                j0 = j1
    perm = np.zeros(C, np.int64)
    perm[p] = np.arange(C)
    return perm


def is_permutation(perm):
    perm = np.asarray(perm)
    return perm.shape[-1] == 0 or bool((np.sort(perm, -1) == np.arange(perm.shape[-1])).all())


def _pair_direct(sb, eb):
    """sb, eb [C,n] fp64 -> snr [C,C] (estimate i, reference j) and the pieces of its gradient."""
    C = sb.shape[0]
    sc = sb - sb.mean(-1, keepdims=True)
    ec = eb - eb.mean(-1, keepdims=True)
    snr = np.zeros((C, C))
    for i in range(C):
        for j in range(C):
            proj = (ec[i] * sc[j]).sum() * sc[j] / ((sc[j] ** 2).sum() + EPS)
            noise = ec[i] - proj
            snr[i, j] = 10.0 * np.log10((proj ** 2).sum() / ((noise ** 2).sum() + EPS) + EPS)
    return snr, sc, ec


def _grad_direct(sc, ec):
    """d snr / d e[t] of one pair (sc, ec centred, [n]) by the chain rule on the vectors -> (gradient [n], A, B): the gradient is
    A sc + B ec once noise is written out."""
    dot, En = (ec * sc).sum(), (sc ** 2).sum()
    Enp = En + EPS
    proj = dot * sc / Enp
    noise = ec - proj
    P, Nz = (proj ** 2).sum(), (noise ** 2).sum()
    ratio = P / (Nz + EPS)
    k = K10 / (ratio + EPS)
    dP = 2.0 * (proj * sc).sum() / Enp * sc                            # d P / d ec
    dNz = 2.0 * noise - 2.0 * (noise * sc).sum() / Enp * sc            # d Nz / d ec
    g = k * (dP / (Nz + EPS) - P / (Nz + EPS) ** 2 * dNz)
    g = g - g.mean()                                                   # through the centring of e (sc and noise have mean 0)
    Bc = -2.0 * k * P / (Nz + EPS) ** 2
    A = k * (2.0 * dot * En / (Enp ** 2 * (Nz + EPS)) + P / (Nz + EPS) ** 2 * (2.0 * dot / Enp + 2.0 * (noise * sc).sum() / Enp))
    return g, A, Bc


def _optimum(snr):
    rows, cols = linear_sum_assignment(snr, maximize=True)
    perm = np.zeros(len(rows), np.int64)
    perm[rows] = cols
    return perm


def margin_of(snr, perm):
    """The smallest loss in mean SI-SNR when one matched edge is forbidden and the assignment solved again: the distance from the
    optimum to the best other assignment (every other assignment misses at least one of the optimum's edges)."""
    C = snr.shape[0]
    best = snr[np.arange(C), perm].sum()
    worst = np.inf
    for i in range(C):
        m = snr.copy()
        m[i, perm[i]] = -1e9
        other = _optimum(m)
        if C > 1:
            worst = min(worst, (best - snr[np.arange(C), other].sum()) / C)
    return float(worst)


def _scale(B, C, b, g_loss, g_max):
    return ((0.0 if g_loss is None else -float(g_loss) / B) + (0.0 if g_max is None else float(np.asarray(g_max).reshape(-1)[b]))) / C


def direct(s, e, lens, g_loss=None, g_max=None):
    """s, e [B,C,T] (computed in fp64), lens [B] -> dict of pair [B,C,C], perm [B,C] (the reference of estimate i), max_snr [B],
    loss, margin [B] (dB), A, Bc, me, ms [B,C] (the matched pairs' gradient coefficients and means) and grad [B,C,T]: the gradient
    of g_loss * loss + sum_b g_max[b] * max_snr[b] (g_loss = 1 when both are None)."""
    s, e = np.asarray(s, np.float64), np.asarray(e, np.float64)
    B, C, T = e.shape
    lens = _clamp(lens, T)
    if g_loss is None and g_max is None:
        g_loss = 1.0
    out = dict(pair=np.zeros((B, C, C)), perm=np.zeros((B, C), np.int64), max_snr=np.zeros(B), margin=np.zeros(B),
               A=np.zeros((B, C)), Bc=np.zeros((B, C)), me=np.zeros((B, C)), ms=np.zeros((B, C)), grad=np.zeros((B, C, T)))
    for b in range(B):
        n = int(lens[b])
        sb, eb = s[b, :, :n], e[b, :, :n]
        snr, sc, ec = _pair_direct(sb, eb)
        perm = _optimum(snr)
        out["pair"][b], out["perm"][b] = snr, perm
        out["max_snr"][b] = snr[np.arange(C), perm].sum() / C
        out["margin"][b] = margin_of(snr, perm)
        scale = _scale(B, C, b, g_loss, g_max)
        for i in range(C):
            j = perm[i]
            g, A, Bc = _grad_direct(sc[j], ec[i])
            out["grad"][b, i, :n] = scale * g
            out["A"][b, i], out["Bc"][b, i], out["me"][b, i], out["ms"][b, i] = A, Bc, eb[i].mean(), sb[j].mean()
    out["loss"] = float(-out["max_snr"].mean())
    return out


def moment_form(s, e, lens):
    """The kernels' algebra in fp64 on raw moments summed by numpy -> pair [B,C,C]."""
    s, e = np.asarray(s, np.float64), np.asarray(e, np.float64)
    B, C, T = e.shape
    lens = _clamp(lens, T)
    pair = np.zeros((B, C, C))
    for b in range(B):
        n = int(lens[b])
        sb, eb = s[b, :, :n], e[b, :, :n]
        ms, me = sb.sum(-1) / n, eb.sum(-1) / n
        En = np.maximum((sb * sb).sum(-1) - n * ms * ms, 0.0)
        Ee = np.maximum((eb * eb).sum(-1) - n * me * me, 0.0)
        dot = eb @ sb.T - n * me[:, None] * ms[None, :]
        Enp = En[None, :] + EPS
        P = dot * dot * En[None, :] / (Enp * Enp)
        Nz = np.maximum(Ee[:, None] - 2.0 * dot * dot / Enp + P, 0.0)
        pair[b] = 10.0 * np.log10(P / (Nz + EPS) + EPS)
    return pair


def make_case(B, C, T, seed):
    """Planted: references Gaussian with a row scale in [0.1, 0.5]; the estimates are a drawn permutation of the references, output i
    being its reference plus noise of 0.03 (1 + i).  lens in [T/2, T], lens[0] = T.
    -> s [B,C,T] f32, e [B,C,T] f32, lens [B] i64, planted [B,C] (the reference of output i)."""
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((B, C, T)) * rng.uniform(0.1, 0.5, (B, C, 1))
    planted = np.zeros((B, C), np.int64)
    e = np.zeros((B, C, T))
    for b in range(B):
        planted[b] = rng.permutation(C)
        for i in range(C):
            e[b, i] = s[b, planted[b, i]] + 0.03 * (1 + i) * rng.standard_normal(T)
    lens = rng.integers(T // 2, T + 1, B).astype(np.int64)
    lens[0] = T
    return s.astype(np.float32), e.astype(np.float32), lens, planted


def make_mixed_case(B, C, T, seed):
    """Harder matrices: every estimate is a random mixture of ALL references (weights uniform in [0, 1]), so that several outputs
    favour the same reference and the row-wise argmax is no permutation.  -> s, e [B,C,T] f32, lens [B] = T."""
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((B, C, T)) * rng.uniform(0.1, 0.5, (B, C, 1))
    mix = rng.uniform(0.0, 1.0, (B, C, C))
    e = np.einsum("bij,bjt->bit", mix, s)
    return s.astype(np.float32), e.astype(np.float32), np.full(B, T, np.int64)


def solver_matrices(C, count=200, seed=0):
    """The solver tests' matrices [count + 1, C, C] fp32: Gaussian, every fourth one rounded to integers in -3 .. 3 (many exact
    ties), and one all-equal matrix at the end."""
    rng = np.random.default_rng(1000 * seed + C)
    m = rng.standard_normal((count + 1, C, C)) * 2.0
    m[::4] = np.clip(np.round(m[::4]), -3, 3)
    m[-1] = 1.5
    return m.astype(np.float32)


def value(score, perm):
    """sum_i score[n, i, perm[n, i]] in fp64 -> [N]."""
    score, perm = np.asarray(score, np.float64), np.asarray(perm, np.int64)
    return np.take_along_axis(score, perm[..., None], -1)[..., 0].sum(-1)


def scipy_value(score, maximize=True):
    score = np.asarray(score, np.float64)
    out = np.zeros(len(score))
    for n, m in enumerate(score):
        r, c = linear_sum_assignment(m, maximize=maximize)
        out[n] = m[r, c].sum()
    return out


def grad_bound(s, e, lens, ref, g_loss=None, g_max=None):
    """10 * 2^-24 |scale_b| (|A| (|s_j[t]| + |mean s_j|) + |B| (|e_i[t]| + |mean e_i|)) from direct()'s result `ref`.

    The fp32 backward pass computes scale_b * (A (s_j - ms) + B (e_i - me)) with every operation rounded once.  In half-ulps
    (2^-24 relative) of the magnitudes above: the term A (s_j - ms) carries the roundings of A and of ms (fp64 -> fp32), of the
    difference and of the product: 4; the term with B likewise 4, and each only on its own magnitude, so together they are 4 on the
    sum of the two magnitudes; the sum of the two terms: 1; scale_b is g_loss / B, the sum with g_max[b] and the division by C: 3;
    the final product: 1.  That is 9 half-ulps; 10 with the second-order terms covered."""
    s, e = np.abs(np.asarray(s, np.float64)), np.abs(np.asarray(e, np.float64))
    B, C, T = e.shape
    out = np.zeros((B, C, T))
    if g_loss is None and g_max is None:
        g_loss = 1.0
    for b in range(B):
        scale = abs(_scale(B, C, b, g_loss, g_max))
        for i in range(C):
            j = ref["perm"][b, i]
            mag = abs(ref["A"][b, i]) * (s[b, j] + abs(ref["ms"][b, i])) + abs(ref["Bc"][b, i]) * (e[b, i] + abs(ref["me"][b, i]))
            out[b, i] = 10 * 2.0 ** -24 * scale * mag
    return out
