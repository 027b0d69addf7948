"""STOI / ESTOI training loss: forward plus backward of the HIP path (stoi.stoi_pairs, csrc/ctn_stoi_grad.hip) and of the Solver
criterion (stoi.StoiPitCriterion) against a torch restatement on the GPU, against the PIT SI-SNR loss (cal_loss) and the training
step (`step_share`: relative to the 9.9 - 10.6 ms the README quotes for bench.py, not measured here), with the shares of the stages and the cost of the validation read-back.

Inputs: B = 8 utterances of C = 2 speech-like sources, T = 32000 samples at 8 kHz (the training segment), estimates = sources with
leakage and noise.  One timed call = scores forward + the gradient with respect to the estimates.  Timing: warm-up calls, then per
iteration two device events around the call on its stream; the median is reported.  Peak memory: torch's peak of allocated bytes
over one call, above what was allocated before it.

The torch restatement is tests/stoi_grad_oracle.py's chain in fp64 on the device, one pair at a time: frames by unfold, compaction
by index_add with the kept-index table of ctn_stoi_frames, torch.fft.rfft (no torch.stft), band sums, segments by unfold, the
15 x 30 normalisations.  It starts from the 10 kHz signals (the resampler and its adjoint are left out of it, which favours it).
`stages` times the C entry points one by one on the same pairs (events around each call); `validation_ms` is the wall-clock time
of the non-silent check and the lengths' trip to the host, the only read-backs of the path.

    python benchmarks/stoi_loss_bench.py [--batch 8] [--samples 32000] [--iters 50] [--warmup 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import resample as rs  # noqa: E402
from conv_tasnet_amd.pit_criterion import cal_loss  # noqa: E402
import bss_oracle as BO  # noqa: E402
import stoi_oracle as SO  # noqa: E402

st = sys.modules["conv_tasnet_amd.stoi"]     # (ctn.stoi is the function)
STEP_MS = (9.9, 10.6)       # the range the README quotes for the flagship training step (bench.py); not measured here
F64 = torch.float64


def event_ms(fn, iters):
    out = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out)), float(min(out))


def peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


class TorchStoi:
    """The restatement: constants on the device, the kept-index tables given."""

    def __init__(self, dev):
        self.win = torch.from_numpy(SO.WINDOW.copy()).to(dev)
        self.bands = SO.band_table()
        self.offs = torch.arange(SO.N_FRAME, device=dev)
        self.dev = dev

    def envelopes(self, sig, m):
        fr = sig.unfold(0, SO.N_FRAME, SO.HOP)[:m] * self.win
        X = torch.fft.rfft(fr, n=SO.NFFT, dim=1)
        p = X.real ** 2 + X.imag ** 2
        return torch.stack([p[:, a:a + w].sum(dim=1).sqrt() for a, w in self.bands])

    def compact(self, y, idx):
        K = idx.shape[0]
        fr = y.unfold(0, SO.N_FRAME, SO.HOP)[idx] * self.win
        pos = (torch.arange(K, device=self.dev)[:, None] * SO.HOP + self.offs[None, :]).reshape(-1)
        return torch.zeros((K - 1) * SO.HOP + SO.N_FRAME, dtype=F64, device=self.dev).index_add(0, pos, fr.reshape(-1))

    def pair(self, x, y, idx, extended):
        M = idx.shape[0] - 1
        ex, ey = self.envelopes(self.compact(x, idx), M), self.envelopes(self.compact(y, idx), M)
        xs, ys = ex.unfold(1, SO.N, 1).permute(1, 0, 2), ey.unfold(1, SO.N, 1).permute(1, 0, 2)
        if extended:
            def norm(s):
                s = s - s.mean(dim=2, keepdim=True)
                s = s / (s.norm(dim=2, keepdim=True) + SO.EPS)
                s = s - s.mean(dim=1, keepdim=True)
                return s / (s.norm(dim=1, keepdim=True) + SO.EPS)
            return (norm(xs) * norm(ys) / SO.N).sum() / xs.shape[0]
        yn = ys * (xs.norm(dim=2, keepdim=True) / (ys.norm(dim=2, keepdim=True) + SO.EPS))
        yp = torch.minimum(yn, xs * (1 + 10 ** (-SO.BETA / 20)))
        yp = yp - yp.mean(dim=2, keepdim=True)
        xc = xs - xs.mean(dim=2, keepdim=True)
        yp = yp / (yp.norm(dim=2, keepdim=True) + SO.EPS)
        xc = xc / (xc.norm(dim=2, keepdim=True) + SO.EPS)
        return (yp * xc).sum() / (xs.shape[0] * SO.NUMBAND)

    def mean_score(self, ref10, est10, tables, extended):
        B, C, _ = ref10.shape
        tot = 0.0
        for b in range(B):
            for c in range(C):
                tot = tot + self.pair(ref10[b, c], est10[b, c], tables[b][c], extended)
        return tot / (B * C)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--samples", type=int, default=32000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stoi_loss_bench needs the GPU")
    dev = torch.device("cuda:0")
    lib = ctn.lib
    lib.load()
    B, C, T, fs = a.batch, 2, a.samples, 8000
    stream = torch.cuda.current_stream().cuda_stream

    def measure(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        med, best = event_ms(fn, a.iters)
        return med, best, peak_bytes(fn)

    pairs = [BO.mixtures(900 + b, C, T) for b in range(B)]
    ref = torch.from_numpy(np.stack([p[0] for p in pairs]) * np.float32(0.3)).to(dev)
    est = torch.from_numpy(np.stack([p[1] for p in pairs]) * np.float32(0.3)).to(dev).requires_grad_(True)
    lens = torch.full((B,), T, dtype=torch.int64, device=dev)
    eo = torch.arange(C, dtype=torch.int32, device=dev).repeat(B, 1)

    # the 10 kHz signals and the kept-index tables for the restatement and the stage calls
    up, down = rs.ratio(fs, st.FS)
    T10 = rs.out_len(T, up, down)
    lens_host = np.full(B, T, dtype=np.int64)
    with torch.no_grad():
        ref10, est10 = st._to_10k(ref, lens_host, up, down, T10), st._to_10k(est.detach(), lens_host, up, down, T10)
    lens10 = torch.full((B * C,), T10, dtype=torch.int64, device=dev)
    P = B * C
    NF = lib.ctn_stoi_max_frames(T10)
    MF = max(NF - 1, 1)
    energy = torch.empty(P, NF, dtype=F64, device=dev)
    idx = torch.empty(P, NF, dtype=torch.int32, device=dev)
    K = torch.empty(P, dtype=torch.int32, device=dev)
    env = torch.zeros(P, 2, 15, MF, dtype=F64, device=dev)
    d = [torch.empty(P, dtype=F64, device=dev) for _ in range(2)]
    g_env = torch.empty(P, 15, MF, dtype=F64, device=dev)
    g10 = torch.empty(P, T10, dtype=F64, device=dev)
    g_est = torch.empty(B, C, T, dtype=torch.float32, device=dev)
    one, zero = torch.ones(P, dtype=F64, device=dev), torch.zeros(P, dtype=F64, device=dev)
    h, W = rs.device_filter(up, down, dev)
    ws = [torch.empty(max(n, 1), dtype=torch.uint8, device=dev) for n in
          (lib.ctn_stoi_score_workspace(P, 1, 1, T10), lib.ctn_stoi_score_bwd_workspace(P, T10), lib.ctn_stoi_bands_bwd_workspace(P, T10))]
    p_ = torch.Tensor.data_ptr
    stage_calls = [
        ("resample_to_10k", lambda: st._to_10k(est.detach(), lens_host, up, down, T10)),
        ("frames", lambda: lib.call("ctn_stoi_frames", p_(ref10), p_(lens10), P, 1, T10, p_(energy), p_(idx), p_(K), stream)),
        ("bands", lambda: lib.call("ctn_stoi_bands", p_(ref10), p_(est10), p_(lens10), p_(idx), p_(K), P, 1, 1, T10, p_(env), stream)),
        ("score", lambda: lib.call("ctn_stoi_score", p_(env), p_(K), P, 1, 1, T10, p_(d[0]), p_(d[1]), 0, 0, p_(ws[0]), ws[0].numel(),
                                   stream)),
        ("score_bwd_stoi", lambda: lib.call("ctn_stoi_score_bwd", p_(env), p_(K), p_(one), p_(zero), P, T10, p_(g_env), p_(ws[1]),
                                            ws[1].numel(), stream)),
        ("score_bwd_estoi", lambda: lib.call("ctn_stoi_score_bwd", p_(env), p_(K), p_(zero), p_(one), P, T10, p_(g_env), p_(ws[1]),
                                             ws[1].numel(), stream)),
        ("bands_bwd", lambda: lib.call("ctn_stoi_bands_bwd", p_(est10), p_(lens10), p_(idx), p_(K), p_(env), p_(g_env), P, T10, p_(g10),
                                       p_(ws[2]), ws[2].numel(), stream)),
        ("resample_adjoint", lambda: lib.call("ctn_resample_rows_adjoint_f64", p_(g10), p_(eo), p_(lens), B, C, C, T, T10, up, down,
                                              p_(h), W, p_(g_est), 0, stream)),
    ]
    stages = {}
    for name, fn in stage_calls:
        stages[name] = measure(fn)[0]
    Kh, idxh = K.cpu().numpy(), idx.cpu()
    tables = [[idxh[b * C + c, :Kh[b * C + c]].long().to(dev) for c in range(C)] for b in range(B)]
    ref10d = ref10.double()
    est10d = est10.double().requires_grad_(True)
    restatement = TorchStoi(dev)

    def pit_step():
        e = est.clone()                                    # the loss masks its input in place: it refuses a leaf tensor
        torch.autograd.grad(cal_loss(ref, e, lens)[0], est)

    def validation():
        st._check_nonsilent(ref, lens)
        lens.cpu()

    for _ in range(a.warmup):
        validation()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.iters):
        validation()
    validation_ms = (time.perf_counter() - t0) / a.iters * 1e3
    pit_ms, pit_min, pit_peak = measure(pit_step)
    results = []
    for extended in (False, True):
        crit = st.StoiPitCriterion(fs, 10.0, extended)

        def hip():
            torch.autograd.grad(st.stoi_pairs(ref, est, lens, fs, eo, extended).mean(), est)

        def hip_fwd():
            with torch.no_grad():
                st.stoi_pairs(ref, est, lens, fs, eo, extended)

        def criterion():
            torch.autograd.grad(crit(ref, est.clone(), lens), est)

        def torch_ref():
            torch.autograd.grad(restatement.mean_score(ref10d, est10d, tables, extended), est10d)

        hip_ms, hip_min, hip_peak = measure(hip)
        fwd_ms = measure(hip_fwd)[0]
        crit_ms, crit_min, crit_peak = measure(criterion)
        ref_ms, ref_min, ref_peak = measure(torch_ref)
        score_hip = float(st.stoi_pairs(ref, est, lens, fs, eo, extended).mean().detach())
        score_ref = float(restatement.mean_score(ref10d, est10d, tables, extended).detach())
        res = {"metric": "stoi_loss_fwd_bwd", "measure": "estoi" if extended else "stoi", "batch": B, "sources": C, "samples": T,
               "sample_rate": fs, "hip_ms_median": hip_ms, "hip_ms_min": hip_min, "hip_fwd_ms_median": fwd_ms,
               "hip_peak_bytes": hip_peak, "criterion_ms_median": crit_ms, "criterion_ms_min": crit_min,
               "criterion_peak_bytes": crit_peak, "torch_ms_median": ref_ms, "torch_ms_min": ref_min, "torch_peak_bytes": ref_peak,
               "speedup_vs_torch": ref_ms / hip_ms, "peak_memory_ratio": ref_peak / max(hip_peak, 1),
               "cal_loss_ms_median": pit_ms, "cal_loss_ms_min": pit_min, "cal_loss_peak_bytes": pit_peak,
               "step_share": [hip_ms / STEP_MS[1], hip_ms / STEP_MS[0]], "step_share_of_quoted_ms": list(STEP_MS), "validation_ms": validation_ms, "stages_ms": stages,
               "mean_score_hip": score_hip, "mean_score_torch": score_ref, "iters": a.iters, "warmup": a.warmup}
        results.append(res)
        print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
