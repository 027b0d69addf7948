"""Multi-resolution STFT training loss: forward plus backward of the HIP path (mrstft.mrstft_pairs, csrc/ctn_mrstft.hip) and of
the Solver criterion (mrstft.MrStftPitCriterion) against a torch restatement on the same GPU (torch.stft per resolution, in fp32
and in fp64), against the PIT SI-SNR loss (cal_loss), the training step (`step_share`: relative to the 9.9 - 10.6 ms the README
quotes for bench.py, not measured here) and the floor of reading 2 B C T floats per resolution at 8 TB/s.

Inputs: B = 8 utterances of C = 2 Gaussian sources, T = 32000 samples, estimates = 0.7 source + 0.5 noise (tests/mrstft_oracle.py's
signals), the default resolutions.  One timed call = the terms forward + the gradient of their mean with respect to the estimates.
Timing: warm-up calls, then per iteration two device events around the call on its stream; the median is reported.  Peak memory:
torch's peak of allocated bytes over one call, above what was allocated before it.
`stages_ms` times the two C entry points on their own (events around each call: forward = tables + frames + terms, backward =
frame gradients + gather), all resolutions together and one resolution at a time; what the autograd node and the input checks add
is the difference to `hip_ms_median`; `stage_share` gives the three as fractions of it.

    python benchmarks/mrstft_bench.py [--batch 8] [--samples 32000] [--iters 50] [--warmup 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import mrstft as ms  # noqa: E402
from conv_tasnet_amd.pit_criterion import cal_loss  # noqa: E402
import mrstft_oracle as MO  # noqa: E402

STEP_MS = (9.9, 10.6)       # the range the README quotes for the flagship training step (bench.py); not measured here
HBM_BYTES_PER_S = 8e12


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


def torch_terms(ref, est, resolutions, eps=ms.EPS):
    """ref, est [P,T] of one dtype, full length -> [P,R,3]: torch.stft + clamp + sqrt + norms per resolution"""
    out = []
    for n_fft, hop, win in resolutions:
        w = torch.hann_window(win, dtype=ref.dtype, device=ref.device)
        a, b = (torch.sqrt(torch.clamp(X.real ** 2 + X.imag ** 2, min=eps)) for X in
                (torch.stft(x, n_fft, hop, win, w, center=True, pad_mode="reflect", return_complex=True) for x in (ref, est)))
        sc = torch.linalg.norm(a - b, dim=(1, 2)) / torch.linalg.norm(a, dim=(1, 2))
        out.append(torch.stack([sc, (a.log() - b.log()).abs().mean(dim=(1, 2)), (a - b).abs().mean(dim=(1, 2))], dim=1))
    return torch.stack(out, dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--samples", type=int, default=32000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mrstft_bench needs the GPU")
    dev = torch.device("cuda:0")
    lib = ctn.lib
    lib.load()
    B, C, T = a.batch, 2, a.samples
    res = ms.DEFAULT_RESOLUTIONS
    R = len(res)
    stream = torch.cuda.current_stream().cuda_stream

    def measure(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        med, best = event_ms(fn, a.iters)
        return med, best, peak_bytes(fn)

    pairs = [MO.signals(900 + b, C, C, T) for b in range(B)]
    ref = torch.from_numpy(np.stack([p[0] for p in pairs])).to(dev)
    est = torch.from_numpy(np.stack([p[1] for p in pairs])).to(dev).requires_grad_(True)
    lens = torch.full((B,), T, dtype=torch.int64, device=dev)
    eo = torch.arange(C, dtype=torch.int32, device=dev).repeat(B, 1)
    p_ = torch.Tensor.data_ptr

    def stage_pair(resolutions):
        ra = np.ascontiguousarray(np.array(resolutions, dtype=np.int32))
        n = len(resolutions)
        fw = torch.empty(lib.ctn_mrstft_workspace(B, C, T, n, ra.ctypes.data), dtype=torch.uint8, device=dev)
        bw = torch.empty(lib.ctn_mrstft_bwd_workspace(B, C, T, n, ra.ctypes.data), dtype=torch.uint8, device=dev)
        terms = torch.empty(B, C, n, 3, dtype=torch.float64, device=dev)
        gt = torch.full((B, C, n, 3), 1.0 / (B * C * n), dtype=torch.float64, device=dev)
        g = torch.empty(B, C, T, dtype=torch.float32, device=dev)
        e = est.detach()
        fwd = measure(lambda: lib.call("ctn_mrstft_pairs_fwd", p_(ref), p_(e), p_(lens), p_(eo), B, C, C, T, ra.ctypes.data, n, ms.EPS,
                                       p_(terms), p_(fw), fw.numel(), stream))[0]
        bwd = measure(lambda: lib.call("ctn_mrstft_pairs_bwd", p_(fw), fw.numel(), p_(ref), p_(e), p_(lens), p_(eo), B, C, C, T,
                                       ra.ctypes.data, n, ms.EPS, p_(gt), p_(g), p_(bw), bw.numel(), stream))[0]
        return {"forward": fwd, "backward": bwd, "forward_workspace_bytes": fw.numel(), "backward_workspace_bytes": bw.numel()}

    stages = {"all": stage_pair(res)}
    for r in res:
        stages["%d:%d:%d" % r] = stage_pair((r,))

    def hip():
        torch.autograd.grad(ms.mrstft_pairs(ref, est, lens, eo, res).mean(), est)

    def hip_fwd():
        with torch.no_grad():
            ms.mrstft_pairs(ref, est, lens, eo, res)

    crit = ms.MrStftPitCriterion(1.0, res)

    def criterion():
        torch.autograd.grad(crit(ref, est.clone(), lens), est)

    def pit_step():
        e = est.clone()                                    # the loss masks its input in place: it refuses a leaf tensor
        torch.autograd.grad(cal_loss(ref, e, lens)[0], est)

    hip_ms, hip_min, hip_peak = measure(hip)
    fwd_ms = measure(hip_fwd)[0]
    crit_ms, crit_min, crit_peak = measure(criterion)
    pit_ms, pit_min, pit_peak = measure(pit_step)
    terms_hip = ms.mrstft_pairs(ref, est, lens, eo, res).detach()
    g_hip = torch.autograd.grad(ms.mrstft_pairs(ref, est, lens, eo, res).mean(), est)[0]
    out = {"metric": "mrstft_loss_fwd_bwd", "batch": B, "sources": C, "samples": T, "resolutions": [list(r) for r in res],
           "hip_ms_median": hip_ms, "hip_ms_min": hip_min, "hip_fwd_ms_median": fwd_ms, "hip_peak_bytes": hip_peak,
           "criterion_ms_median": crit_ms, "criterion_ms_min": crit_min, "criterion_peak_bytes": crit_peak,
           "cal_loss_ms_median": pit_ms, "cal_loss_ms_min": pit_min, "cal_loss_peak_bytes": pit_peak,
           "step_share": [hip_ms / STEP_MS[1], hip_ms / STEP_MS[0]], "step_share_of_quoted_ms": list(STEP_MS),
           "read_floor_ms": 2.0 * B * C * T * 4 * R / HBM_BYTES_PER_S * 1e3, "read_floor_bytes_per_s": HBM_BYTES_PER_S,
           "stages_ms": stages, "iters": a.iters, "warmup": a.warmup}
    f_ms, b_ms = stages["all"]["forward"], stages["all"]["backward"]
    out["stage_share"] = {"forward": f_ms / hip_ms, "backward": b_ms / hip_ms, "autograd_node_and_checks": 1.0 - (f_ms + b_ms) / hip_ms}
    for name, dt in (("fp32", torch.float32), ("fp64", torch.float64)):
        rr = ref.reshape(B * C, T).to(dt)
        ee = est.detach().reshape(B * C, T).to(dt).requires_grad_(True)

        def torch_ref():
            torch.autograd.grad(torch_terms(rr, ee, res).mean(), ee)

        t_ms, t_min, t_peak = measure(torch_ref)
        tt = torch_terms(rr, ee, res)
        gg = torch.autograd.grad(tt.mean(), ee)[0].reshape(B, C, T)
        out["torch_%s" % name] = {"ms_median": t_ms, "ms_min": t_min, "peak_bytes": t_peak, "speedup": t_ms / hip_ms,
                                  "peak_memory_ratio": t_peak / max(hip_peak, 1),
                                  "largest_term_difference": float((tt.detach().reshape(B, C, R, 3).double() - terms_hip).abs().max()),
                                  "largest_gradient_difference_of_max": float((gg.double() - g_hip.double()).abs().max()
                                                                              / g_hip.double().abs().max())}
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
