"""BSS Eval v3 (SDR / SIR / SAR) on the GPU in fp64: mir_eval.separation.bss_eval_sources as cal_SDRi calls it
(src/evaluate.py:76-91).

``bss_eval_batch(ref, est, lengths)`` scores every estimate row of a padded batch against every reference with the HIP
kernels of csrc/ctn_bss.hip (correlations, Cholesky of the 512-tap Gram matrices, solves, projections; fp64 throughout) and
returns the full ``[B, E, C]`` matrices on the device.  ``bss_eval_sources`` is mir_eval's call form for one utterance.
An utterance whose Gram matrix does not factorise (a pivot not above n*eps*max diag) is redone on the host in fp64 the
way mir_eval does it (``torch.linalg.solve``, ``lstsq`` if that raises) and flagged: never silently wrong numbers.
"""
import itertools

import numpy as np
import torch
import torch.nn.functional as Fn

from ._lib import lib

FLEN = 512                     # distortion-filter length of bss_eval_sources
WORKSPACE_BUDGET = 1 << 30     # bytes of workspace per ctn_bss_eval call; larger batches are split


def _ptr(t):
    return t.data_ptr() if t is not None else 0


def _check_nonsilent(x, lengths, what):
    t = torch.arange(x.shape[-1], device=x.device)
    live = ((x != 0) & (t < lengths.view(-1, 1, 1))).any(-1)
    if not bool(live.all()):
        raise ValueError("All the %s sources should be non-silent (not all-zeros), but at least one of them is all 0s, "
                         "which introduces ambiguity to the evaluation." % what)


def _project_host(refs, e):
    """mir_eval's _project in fp64 on the host: refs [K,n], e [n] -> the n+F-1 samples of the projection of e onto the F
    delayed copies of every row of refs (G c = D by solve, lstsq if that raises)."""
    K, n = refs.shape
    pad = Fn.pad(refs, (0, FLEN - 1)).unsqueeze(1)                         # [K,1,n+F-1]
    r = Fn.conv1d(pad, refs.unsqueeze(1))                                  # r[k,i,tau] = sum_t s_i[t] s_k[t+tau]
    G = torch.empty(K * FLEN, K * FLEN, dtype=torch.float64)
    a = torch.arange(FLEN)
    lag = a.view(-1, 1) - a.view(1, -1)
    for i in range(K):
        for k in range(K):
            # G[iF+a, kF+b] = r_ik(a-b) for a >= b, r_ki(b-a) otherwise
            G[i * FLEN:(i + 1) * FLEN, k * FLEN:(k + 1) * FLEN] = torch.where(lag >= 0, r[k, i][lag.clamp(min=0)],
                                                                              r[i, k][(-lag).clamp(min=0)])
    D = Fn.conv1d(Fn.pad(e, (0, FLEN - 1)).view(1, 1, -1), refs.unsqueeze(1)).reshape(-1)   # D[iF+a] = sum_t s_i[t] e[t+a]
    try:
        c = torch.linalg.solve(G, D)
    except RuntimeError:                                                   # torch.linalg.LinAlgError: singular
        c = torch.linalg.lstsq(G, D.unsqueeze(1), driver="gelsd").solution[:, 0]
    c = c.view(K, FLEN)
    sp = Fn.conv1d(Fn.pad(refs, (FLEN - 1, FLEN - 1)).unsqueeze(0), c.flip(-1).unsqueeze(1), groups=K)
    return sp[0].sum(0)                                                    # [n+F-1]


def _safe_db(num, den):
    return float("inf") if den == 0 else 10.0 * np.log10(num / den)


def _bss_eval_host(ref, est):
    """ref [C,n], est [E,n] fp64 CPU tensors -> sdr, sir, sar [E,C] float64 numpy (mir_eval's _bss_decomp_mtifilt and
    _bss_source_crit)."""
    C, n = ref.shape
    E = est.shape[0]
    out = np.zeros((3, E, C))
    for e in range(E):
        ep = Fn.pad(est[e], (0, FLEN - 1))
        pall = _project_host(ref, est[e])
        for j in range(C):
            pj = _project_host(ref[j:j + 1], est[e])
            out[0, e, j] = _safe_db(float((pj ** 2).sum()), float(((ep - pj) ** 2).sum()))
            out[1, e, j] = _safe_db(float((pj ** 2).sum()), float(((pall - pj) ** 2).sum()))
            out[2, e, j] = _safe_db(float((pall ** 2).sum()), float(((ep - pall) ** 2).sum()))
    return out


def bss_eval_batch(ref, est, lengths):
    """ref [B,C,T], est [B,E,T] (fp32 on the GPU; other dtypes are cast), lengths [B] -> (sdr, sir, sar, fallback):
    sdr/sir/sar [B,E,C] fp64 on the device, row e of est scored against reference j over the first lengths[b] samples;
    fallback [B] bool: the utterance was redone on the host because a Gram matrix did not factorise.  2 <= C <= 4."""
    dev = ref.device
    if dev.type != "cuda":
        raise ValueError("bss_eval_batch runs on the GPU: got %s tensors" % dev)
    if ref.dim() != 3 or est.dim() != 3 or ref.shape[0] != est.shape[0] or ref.shape[2] != est.shape[2]:
        raise ValueError("ref [B,C,T] and est [B,E,T] do not match: %s vs %s" % (tuple(ref.shape), tuple(est.shape)))
    B, C, T = ref.shape
    E = est.shape[1]
    if not 2 <= C <= 4:
        raise ValueError("bss_eval_batch supports 2..4 reference sources, got %d" % C)
    ref = ref.to(device=dev, dtype=torch.float32).contiguous()
    est = est.to(device=dev, dtype=torch.float32).contiguous()
    lengths = torch.as_tensor(lengths).to(device=dev, dtype=torch.int64).clamp(0, T).contiguous()
    _check_nonsilent(ref, lengths, "reference")
    _check_nonsilent(est, lengths, "estimated")
    sdr = torch.empty(B, E, C, dtype=torch.float64, device=dev)
    sir, sar = torch.empty_like(sdr), torch.empty_like(sdr)
    status = torch.empty(B, C, dtype=torch.int32, device=dev)
    per = lib.ctn_bss_workspace(1, C, E, T)
    step = max(1, min(B, WORKSPACE_BUDGET // per))
    stream = torch.cuda.current_stream(dev).cuda_stream
    ws = torch.empty(lib.ctn_bss_workspace(step, C, E, T), dtype=torch.uint8, device=dev)
    for b0 in range(0, B, step):
        nb = min(step, B - b0)
        lib.call("ctn_bss_eval", _ptr(ref[b0:b0 + nb]), _ptr(est[b0:b0 + nb]), _ptr(lengths[b0:b0 + nb]), nb, C, E, T,
                 _ptr(sdr[b0:b0 + nb]), _ptr(sir[b0:b0 + nb]), _ptr(sar[b0:b0 + nb]), _ptr(status[b0:b0 + nb]),
                 _ptr(ws), ws.numel(), stream)
    fallback = (status != 0).any(1)
    bad = torch.nonzero(fallback).flatten().tolist()
    if bad:
        lens = lengths.cpu()
        for b in bad:
            n = int(lens[b])
            got = _bss_eval_host(ref[b, :, :n].double().cpu(), est[b, :, :n].double().cpu())
            for m, o in zip((sdr, sir, sar), got):
                m[b] = torch.from_numpy(o).to(dev)
    return sdr, sir, sar, fallback


def sir_permutation(sir):
    """sir [B,C(estimates),C(references)] -> popt [B,C] int64: the permutation of itertools.permutations(range(C)) order with
    the largest mean sir[b, perm[k], k], the first one on ties (mir_eval's np.argmax over mean_sir)."""
    B, C = sir.shape[0], sir.shape[2]
    perms = torch.tensor(list(itertools.permutations(range(C))), dtype=torch.int64, device=sir.device)
    best = torch.zeros(B, dtype=torch.int64, device=sir.device)
    bestv = None
    for p in range(perms.shape[0]):
        s = sir[:, int(perms[p, 0]), 0]
        for k in range(1, C):
            s = s + sir[:, int(perms[p, k]), k]
        m = s / C
        if bestv is None:
            bestv = m
        else:
            take = m > bestv
            bestv = torch.where(take, m, bestv)
            best = torch.where(take, torch.full_like(best, p), best)
    return perms[best]


def _as_tensor(x):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not torch.is_tensor(x):
        raise ValueError("expected a numpy array or a torch tensor, got %s" % type(x).__name__)
    if x.dim() == 1:
        x = x.unsqueeze(0)
    if x.dim() != 2:
        raise ValueError("expected [nsrc, nsampl], got shape %s" % (tuple(x.shape),))
    return x


def bss_eval_sources(reference_sources, estimated_sources):
    """mir_eval.separation.bss_eval_sources(reference_sources, estimated_sources) on the current GPU in fp64 from the fp32
    samples: [nsrc, nsampl] numpy or torch inputs -> numpy float64 (sdr, sir, sar, popt), with the SIR-maximising
    permutation popt already applied.  Same shape, non-silent sources and 2 <= nsrc <= 4, else ValueError."""
    ref, est = _as_tensor(reference_sources), _as_tensor(estimated_sources)
    if ref.shape != est.shape:
        raise ValueError("The shape of estimated sources and the true sources should match.  reference_sources.shape = %s, "
                         "estimated_sources.shape = %s" % (tuple(ref.shape), tuple(est.shape)))
    dev = torch.device("cuda", torch.cuda.current_device())
    ref, est = ref.to(dev, torch.float32), est.to(dev, torch.float32)
    C, n = ref.shape
    sdr, sir, sar, _ = bss_eval_batch(ref.unsqueeze(0), est.unsqueeze(0), torch.tensor([n], device=dev))
    popt = sir_permutation(sir)[0]
    k = torch.arange(C, device=dev)
    return (sdr[0, popt, k].cpu().numpy(), sir[0, popt, k].cpu().numpy(), sar[0, popt, k].cpu().numpy(),
            popt.cpu().numpy())


def sdr_improvement(sdr, sir):
    """sdr, sir [B,C+1,C] of the C estimates plus the mixture anchor as row C -> [B] fp64: the mean over references of
    sdr[popt[k], k] - sdr_anchor[k] (cal_SDRi's ((sdr[0]-sdr0[0]) + (sdr[1]-sdr0[1])) / 2 for two speakers; the anchor
    rows [mix, mix] of the reference are bitwise equal, so its permutation choice leaves sdr_anchor[k] = sdr[C, k])."""
    C = sdr.shape[2]
    popt = sir_permutation(sir[:, :C])
    k = torch.arange(C, device=sdr.device)
    got = sdr[:, :C][torch.arange(sdr.shape[0], device=sdr.device).view(-1, 1), popt, k.view(1, -1)]
    d = got - sdr[:, C]
    tot = d[:, 0]
    for j in range(1, C):
        tot = tot + d[:, j]
    return tot / C
