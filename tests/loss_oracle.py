"""Plain numpy model of the moment form of the PIT SI-SNR loss (csrc/ctn_loss.hip), and the case table its tests share.

The model is written from the algebra, not from the kernel.  With s0 = s_j - mean(s_j), e0 = e_i - mean(e_i) over t < len:

    En = sum s0^2, Ee = sum e0^2, dot = sum e0 s0             (from the raw fp64 moments sum s, sum e, sum s^2, sum e^2, sum e s)
    proj = dot s0 / (En + EPS)          =>  P  = sum proj^2  = dot^2 En / (En + EPS)^2
    noise = e0 - proj                   =>  Nz = sum noise^2 = Ee - 2 dot^2 / (En + EPS) + P
    snr = 10 log10(P / (Nz + EPS) + EPS)

Only dot and Ee depend on the estimate (d dot / d e0 = s0, d Ee / d e0 = 2 e0), and s0, e0 have zero mean, so the centring is
transparent to the gradient:  d snr / d e_i = A s0 + B e0  with
    A = snr'(ratio) * (P'(dot) / (Nz + EPS) - P / (Nz + EPS)^2 * Nz'(dot)),   B = snr'(ratio) * (-P / (Nz + EPS)^2) * 2.
The device keeps A, B and the two means in fp32 and evaluates scale * (A (s - mean s) + B (e - mean e)) in fp32, with
scale = (-g_loss / B + g_max[b]) / C; the model does the same (numpy fp32, no FMA contraction).

What the model does not reproduce: the order of the fp64 partial sums, FMA contraction, the device's log / log10.
"""
import itertools

import numpy as np
import torch

EPS = 1e-8
F32 = np.float32


def sisnr_pit_model(src, est, lens, g_loss=None, g_max=None):
    """src, est: [B,C,T] fp32 arrays; lens: [B] ints (clamped to T); g_loss: float or None; g_max: [B] or None.
    -> dict(snr [B,C,C] fp32, max_snr [B] fp32, idx [B] int64, loss fp32, d_est [B,C,T] fp32)."""
    src = np.asarray(src, dtype=F32)
    est = np.asarray(est, dtype=F32)
    Bn, C, T = src.shape
    perms = list(itertools.permutations(range(C)))
    snr = np.zeros((Bn, C, C), dtype=F32)
    max_snr = np.zeros((Bn,), dtype=F32)
    idx = np.zeros((Bn,), dtype=np.int64)
    d_est = np.zeros((Bn, C, T), dtype=F32)
    for b in range(Bn):
        n = int(min(int(lens[b]), T))
        s = src[b, :, :n].astype(np.float64)
        e = est[b, :, :n].astype(np.float64)
        ms, me = s.sum(1) / n, e.sum(1) / n
        En = np.maximum((s * s).sum(1) - n * ms * ms, 0.0)
        Ee = np.maximum((e * e).sum(1) - n * me * me, 0.0)
        dot = e @ s.T - n * np.outer(me, ms)                    # [i, j]
        Enp = En[None, :] + EPS
        P = dot * dot * En[None, :] / (Enp * Enp)
        Nz = np.maximum(Ee[:, None] - 2.0 * dot * dot / Enp + P, 0.0)
        ratio = P / (Nz + EPS)
        sn = 10.0 * np.log10(ratio + EPS)
        snr[b] = sn.astype(F32)
        dsnr = (10.0 / np.log(10.0)) / (ratio + EPS)
        dP = 2.0 * dot * En[None, :] / (Enp * Enp)
        dNz = -4.0 * dot / Enp + dP
        A = dsnr * (dP / (Nz + EPS) - P / (Nz + EPS) ** 2 * dNz)
        Bc = dsnr * (-P / (Nz + EPS) ** 2) * 2.0
        best, bestv = 0, F32(0)
        for p, perm in enumerate(perms):                        # fp32 sums in itertools order, the first maximum wins
            acc = F32(0)
            for i in range(C):
                acc = F32(acc + snr[b, i, perm[i]])
            if p == 0 or acc > bestv:
                best, bestv = p, acc
        max_snr[b] = F32(bestv / F32(C))
        idx[b] = best
        scale = F32(0)
        if g_loss is not None:
            scale = F32(scale - F32(F32(g_loss) / F32(Bn)))
        if g_max is not None:
            scale = F32(scale + F32(g_max[b]))
        scale = F32(scale / F32(C))
        for i in range(C):
            j = perms[best][i]
            a, bc, mei, msj = F32(A[i, j]), F32(Bc[i, j]), F32(me[i]), F32(ms[j])
            d_est[b, i, :n] = scale * (a * (src[b, j, :n] - msj) + bc * (est[b, i, :n] - mei))
    loss = F32(0.0 - max_snr.astype(np.float64).sum() / Bn)
    return dict(snr=snr, max_snr=max_snr, idx=idx, loss=loss, d_est=d_est)


# ----------------------------------------------------------------------------------------------------------- case table
# name -> (B, C, T, lengths, options).  The smallest shapes that still reach each code path of csrc/ctn_loss.hip.
def _table():
    t = {}
    for T in (1, 255, 2048, 2049, 4097):          # nchunk 1, 2, 3, an empty last chunk, T < the 256 threads of a workgroup
        t["chunk_T%d" % T] = (3, 2, T, (T, T - 1, 64) if T >= 64 else (T, T, T), {})
    # nchunk capped at 64 (chunk > 2048); the backward's grid is capped at 4096 workgroups, so its grid-stride loop wraps
    t["chunk_cap"] = (4, 2, 140001, (140001, 131073, 131072, 70000), {})
    for C in (1, 4, 5, 6):                        # the whole permutation table in registers; C = 1
        t["spk_C%d" % C] = (2, C, 1500, (1500, 777), {})
    t["batch_stride"] = (300, 2, 96, tuple(64 + (7 * b) % 33 for b in range(300)), {})   # b += 256 in the PIT kernel
    for db in (0, 20, 40, 60):                    # cancellation in Nz and in A, B
        t["snr_%d" % db] = (3, 2, 4000, (4000, 3877, 2000), {"snr": float(db)})
    for dc in (100, 1000):                        # raw moments rather than centred ones
        t["dc_%d" % dc] = (2, 2, 4000, (4000, 3877), {"dc": float(dc)})
    for name, amp in (("tiny_1e-4", 1e-4), ("tiny_1e-6", 1e-6)):   # the EPS terms dominate
        t[name] = (2, 2, 4000, (4000, 3877), {"amp": amp})
    t["silent_src"] = (2, 2, 1000, (1000, 1000), {"silent": "src"})     # En = 0
    t["silent_est"] = (2, 2, 1000, (1000, 1000), {"silent": "est"})     # Ee = 0
    t["tie_C2"] = (2, 2, 1000, (1000, 1000), {"tie": True})
    t["tie_C3"] = (2, 3, 1000, (1000, 1000), {"tie": True})
    t["len_gt_T"] = (2, 2, 1000, (1000, 5000), {})                      # clamped in forward, in backward and in the mask
    return t


TABLE = _table()
CASES = list(TABLE)
DEFAULT_SNR_DB = 20.0


def is_tie(name):
    """Every permutation scores the same: the exact-tie rows, and T = 1, where both centred signals vanish."""
    return bool(TABLE[name][4].get("tie")) or TABLE[name][2] == 1


def make_inputs(Bn, C, T, lens, seed, snr=DEFAULT_SNR_DB, dc=0.0, amp=1.0, silent=None, tie=False):
    """src = seeded randn, zero at t >= len; est = src + 10^(-snr/20) randn with the channels rolled so that the best
    permutation is not the identity.  -> (src, est, lengths) fp32, fp32, int64 CPU tensors."""
    g = torch.Generator().manual_seed(seed)
    src = torch.randn(Bn, C, T, generator=g) * amp + dc
    noise = torch.randn(Bn, C, T, generator=g) * (amp * 10.0 ** (-snr / 20.0))
    if tie:
        src = src[:, :1].expand(Bn, C, T).contiguous()
        noise = noise[:, :1].expand(Bn, C, T).contiguous()
    if silent == "src":
        src[:, C - 1] = 0.0
    lengths = torch.tensor(lens, dtype=torch.int64)
    mk = (torch.arange(T).view(1, 1, T) < lengths.view(-1, 1, 1)).float()
    src = src * mk
    est = src + noise
    if C > 1 and not tie:
        est = torch.stack([torch.roll(est[b], 1 + b % (C - 1), dims=0) for b in range(Bn)])
    if silent == "est":
        est[:, 0] = 0.0
    return src.contiguous(), est.contiguous(), lengths


def case_inputs(name):
    Bn, C, T, lens, opt = TABLE[name]
    return make_inputs(Bn, C, T, lens, seed=1000 + CASES.index(name), **opt)


G_LOSS = 1.3    # upstream gradient of the loss used by the tests (not 1, so that a dropped factor shows)


def g_max_weight(Bn):
    return torch.randn(Bn, generator=torch.Generator().manual_seed(77)) + 0.25


_REF = {}


def reference(name):
    """fp64 oracle with autograd, computed once per case and shared (treat as read-only):
    dict(snr [B,C,C], max_snr [B], idx [B], loss, est_masked, g_loss [B,C,T] = d(G_LOSS * loss)/d est,
    g_max = d (max_snr * wgt).sum() / d est, margin [B] = best minus runner-up permutation score / C in dB)."""
    if name in _REF:
        return _REF[name]
    from oracle import ctn_oracle as O
    src, est, lengths = case_inputs(name)
    Bn, C, T = src.shape
    lc = lengths.clamp(max=T)          # the kernel's contract: a length beyond T means T
    e = est.double().requires_grad_(True)
    loss, max_snr, est_m, _ = O.cal_loss(src.double(), e, lc)
    snr, _ = O.pairwise_si_snr(src.double(), e, lc)
    _, perms, idx, _ = O.si_snr_pit(src.double(), e, lc)
    wgt = g_max_weight(Bn).double()
    gl, = torch.autograd.grad(G_LOSS * loss, e, retain_graph=True)
    gm, = torch.autograd.grad((max_snr.view(-1) * wgt).sum(), e)
    score = torch.stack([snr.detach()[:, torch.arange(C), p].sum(1) for p in perms], dim=1) / C
    top = score.sort(dim=1, descending=True).values
    margin = (top[:, 0] - top[:, 1]) if top.shape[1] > 1 else torch.full((Bn,), float("inf"), dtype=torch.float64)
    _REF[name] = dict(snr=snr.detach(), max_snr=max_snr.detach().view(-1), idx=idx, loss=loss.detach(), est_masked=est_m.detach(),
                      g_loss=gl, g_max=gm, wgt=wgt, margin=margin, lengths=lc)
    return _REF[name]


def check_inputs(name):
    """Conditions on the inputs, from the reference alone: lengths >= 64 (the whole signal where T < 64), and the best
    permutation ahead of the runner-up by more than 0.05 dB except in the tie rows."""
    Bn, C, T, lens, _ = TABLE[name]
    assert min(lens) >= min(64, T), (name, min(lens))
    ref = reference(name)
    if is_tie(name):
        assert float(ref["margin"].abs().max()) == 0.0, (name, ref["margin"])
    else:
        assert float(ref["margin"].min()) > 0.05, (name, ref["margin"])
        if C > 1:
            assert bool((ref["idx"] != 0).all()), (name, ref["idx"])


def rel_err_per_utt(got, ref, lengths):
    """max |got - ref| / max |ref| over t < len, per utterance -> list of floats (0 where the reference is all zero and so is got)."""
    out = []
    for b in range(ref.shape[0]):
        n = int(lengths[b])
        g_, r_ = torch.as_tensor(got[b, :, :n]).double(), ref[b, :, :n].double()
        d, m = float((g_ - r_).abs().max()), float(r_.abs().max())
        out.append(d / m if m > 0 else (0.0 if d == 0 else float("inf")))
    return out
