"""Oracle for the gradient of the GPU STOI / ESTOI loss (csrc/ctn_stoi_grad.hip, stoi.stoi_pairs): stoi_oracle.details restated in
float64 torch on the CPU, so that autograd gives d score / d estimate.  No GPU, no import of the package.

    run(x, y, fs, w_stoi=1.0, w_estoi=0.0, straight_through=True) -> dict:
        stoi, estoi (floats), M, K, index; env_x, env_y [15, M]; g_env [15, M], g10 [n10], g [n]: the gradients of
        w_stoi * stoi + w_estoi * estoi with respect to the estimate's envelopes, its 10 kHz samples and its samples at fs;
        clip_margin (smallest relative distance of a scaled cell to its clip bound), clipped (share of clipped cells), env_min
    stage_rows()                   the ragged 10 kHz pair rows of the stage tests (inputs only)
    resample_linear(y, up, down)   the resampler as the linear float64 map R of its float32 tap table (torch, differentiable)
    adjoint(g10, n, up, down)      R^T g10 -> [n]

What is differentiated (the semantics of include/ctn_hip.h): everything that depends on the reference alone is a constant, i.e.
the kept-index table, the reference's envelopes and the clip bound; the estimate is compacted by the reference's table.  At a rate
other than 10 kHz the forward VALUES are those of the float32 resampler and the gradient is R^T: y10 = R y + (resample_f32(y) -
R y).detach().  With straight_through=False the forward is R y itself (a function whose finite differences can be taken).
A pair with M < 30 scores 1e-5 and has gradient 0.
"""
import math

import numpy as np
import torch

import resample_oracle as RO
import stoi_oracle as SO

F64 = torch.float64
WINDOW = torch.from_numpy(SO.WINDOW.copy())
_FILTERS = {}


def _ratio(fs):
    g = math.gcd(int(fs), SO.FS)
    return SO.FS // g, int(fs) // g


def _filter(up, down):
    if (up, down) not in _FILTERS:
        _FILTERS[(up, down)] = RO.design_filter(up, down)
    return _FILTERS[(up, down)]


def resample_linear(y, up, down):
    """y torch float64 [n] -> [ceil(n up / down)]: sum_j h[(t down) % up, j] y[(t down) // up - W + 1 + j], zeros outside [0, n)."""
    h, W = _filter(up, down)
    n = y.shape[0]
    n_out = RO.out_len(n, up, down)
    first, phase, front, back = RO._indices(n, up, down, W, n_out, 0)
    yp = torch.cat([torch.zeros(front, dtype=F64), y, torch.zeros(back, dtype=F64)])
    table = torch.from_numpy(h.astype(np.float64))
    first, phase = torch.from_numpy(first), torch.from_numpy(phase)
    out = torch.zeros(n_out, dtype=F64)
    for j in range(2 * W):
        out = out + table[phase, j] * yp[first + j]
    return out


def adjoint(g10, n, up, down):
    y = torch.zeros(n, dtype=F64, requires_grad=True)
    (g,) = torch.autograd.grad(resample_linear(y, up, down), y, torch.as_tensor(g10, dtype=F64))
    return g.numpy()


def _sqrt0(s):
    """sqrt with gradient 0 at 0"""
    live = s > 0
    return torch.where(live, torch.sqrt(torch.where(live, s, torch.ones_like(s))), torch.zeros_like(s))


def _norm0(v, dim):
    return _sqrt0((v * v).sum(dim=dim, keepdim=True))


def compact(y10, idx):
    """The overlap-add at hop 128 of the windowed first-pass frames idx of y10."""
    K = len(idx)
    fr = y10.unfold(0, SO.N_FRAME, SO.HOP)[torch.from_numpy(np.asarray(idx, dtype=np.int64))] * WINDOW
    pos = (torch.arange(K)[:, None] * SO.HOP + torch.arange(SO.N_FRAME)[None, :]).reshape(-1)
    return torch.zeros((K - 1) * SO.HOP + SO.N_FRAME, dtype=F64).index_add(0, pos, fr.reshape(-1))


def envelopes(sig):
    """[L] -> [15, frame_count(L)]"""
    m = SO.frame_count(sig.shape[0])
    fr = sig.unfold(0, SO.N_FRAME, SO.HOP)[:m] * WINDOW
    X = torch.fft.rfft(fr, n=SO.NFFT, dim=1)
    p = X.real ** 2 + X.imag ** 2
    return torch.stack([_sqrt0(p[:, a:a + w].sum(dim=1)) for a, w in SO.band_table()])


def _segments(e):
    return e.unfold(1, SO.N, 1).permute(1, 0, 2)            # [M - 29, 15, 30]


def _stoi(ex, ey):
    xs, ys = _segments(ex), _segments(ey)
    scale = _norm0(xs, 2) / (_norm0(ys, 2) + SO.EPS)
    yn = ys * scale
    bound = xs * (1 + 10 ** (-SO.BETA / 20))
    clipped = yn > bound
    yp = torch.where(clipped, bound, yn)
    yp = yp - yp.mean(dim=2, keepdim=True)
    xc = xs - xs.mean(dim=2, keepdim=True)
    yp = yp / (_norm0(yp, 2) + SO.EPS)
    xc = xc / (_norm0(xc, 2) + SO.EPS)
    margin = float(((yn - bound).abs() / bound).min().detach())
    return (yp * xc).sum() / (xs.shape[0] * SO.NUMBAND), float(clipped.double().mean()), margin


def _row_col(s):
    s = s - s.mean(dim=2, keepdim=True)
    s = s / (_norm0(s, 2) + SO.EPS)
    s = s - s.mean(dim=1, keepdim=True)
    return s / (_norm0(s, 1) + SO.EPS)


def _estoi(ex, ey):
    xn, yn = _row_col(_segments(ex)), _row_col(_segments(ey))
    return (xn * yn / SO.N).sum() / xn.shape[0]


def run(x, y, fs, w_stoi=1.0, w_estoi=0.0, straight_through=True):
    x = np.asarray(x, dtype=np.float32)
    yt = torch.tensor(np.asarray(y, dtype=np.float64), dtype=F64, requires_grad=True)
    x10 = SO.resample_10k(x, fs)
    if int(fs) == SO.FS:
        y10 = yt * 1.0
    else:
        up, down = _ratio(fs)
        y10 = resample_linear(yt, up, down)
        if straight_through:
            y10 = y10 + (torch.from_numpy(SO.resample_10k(np.asarray(y, dtype=np.float32), fs)) - y10).detach()
    y10.retain_grad()
    xs, _, idx, en, thr = SO.remove_silent(x10, x10)
    out = {"K": len(idx), "index": idx, "n10": len(x10)}
    ex = torch.from_numpy(SO.envelopes(xs))
    out["M"] = ex.shape[1]
    if ex.shape[1] < SO.N:
        out.update(stoi=SO.TOO_SHORT, estoi=SO.TOO_SHORT, g=np.zeros(len(x)), g10=np.zeros(len(x10)), env_x=ex.numpy(),
                   g_env=np.zeros(tuple(ex.shape)), clipped=0.0, clip_margin=np.inf)
        return out
    ey = envelopes(compact(y10, idx))
    ey.retain_grad()
    d_stoi, clipped, margin = _stoi(ex, ey)
    d_estoi = _estoi(ex, ey)
    (w_stoi * d_stoi + w_estoi * d_estoi).backward()
    out.update(stoi=float(d_stoi.detach()), estoi=float(d_estoi.detach()), g=yt.grad.numpy(), g10=y10.grad.numpy(), g_env=ey.grad.numpy(),
               env_x=ex.numpy(), env_y=ey.detach().numpy(), clipped=clipped, clip_margin=margin, env_min=float(ey.detach().min()))
    return out


# ---- test signals ---------------------------------------------------------------------------------------------------------------
STAGE_LENS, STAGE_T = [4095, 4096, 4097, 7000, 12700], 12800


def stage_rows():
    """(ref [5, T], est [5, T]) fp32 pair rows at 10 kHz for the stage tests, garbage after each length: 29 frames left (no segment),
    exactly one segment, a row with removed frames, and a row whose segments cross the 64-segment workgroup of the score kernel."""
    import bss_oracle as BO
    rng = np.random.RandomState(17)
    ref = rng.randn(len(STAGE_LENS), STAGE_T).astype(np.float32)
    est = rng.randn(len(STAGE_LENS), STAGE_T).astype(np.float32)
    for p, n in enumerate(STAGE_LENS):
        x = BO.speech_like(40 + p, 2, n, sr=10000)
        if p == 3:
            x[0, 2000:3500] *= np.float32(1e-4)                          # removed frames
        ref[p, :n] = x[0]
        est[p, :n] = (0.7 * x[0] + 0.4 * x[1] + 0.05 * rng.randn(n)).astype(np.float32)
    return ref, est
