"""MixIT loss: forward plus backward of the HIP kernels (mixit.py, csrc/ctn_mixit.hip) against a torch restatement that builds
every remix through the [2^M, 2, M] assignment matrices, and against the PIT SI-SNR loss (ops.SiSnrPit) at C = 4.

Inputs: the planted cases of tests/mixit_oracle.py at B = 8, T = 32000 (the training segment), M in {2, 4, 8}.  One timed call =
loss forward + the gradient with respect to the estimates.  Timing: warm-up calls, then per iteration two device events around
the call on its stream; the median over the iterations is reported.  Peak memory: torch's peak of allocated bytes over one call,
above what was allocated before it.  `step_share` relates the MixIT call to the 9.9 - 10.6 ms training step of bench.py.  One
JSON line per M, and all of them as a list into --out.

    python benchmarks/mixit_bench.py [--batch 8] [--samples 32000] [--outputs 2 4 8] [--iters 200] [--warmup 20] [--out FILE]
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
from conv_tasnet_amd import ops  # noqa: E402
import mixit_oracle as MO  # noqa: E402

STEP_MS = (9.9, 10.6)       # the flagship training step (README, bench.py)


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


def torch_mixit(x, e, lens, tau, A):
    """The textbook form in fp32: all 2^M remixes, their errors, the minimum."""
    T = e.shape[2]
    keep = (torch.arange(T, device=e.device)[None, None, :] < lens[:, None, None]).to(e.dtype)
    res = (torch.einsum("anm,bmt->bant", A, e) - x[:, None]) * keep[:, None]
    err = (res * res).sum(-1)
    xx = ((x * keep) ** 2).sum(-1)[:, None, :]
    L = (10.0 * torch.log10((err + tau * xx + MO.EPS) / (xx + MO.EPS))).mean(-1)
    return L.min(dim=1).values.mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--samples", type=int, default=32000)
    ap.add_argument("--outputs", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mixit_bench needs the GPU")
    dev = torch.device("cuda:0")
    ctn.lib.load()
    B, T = a.batch, a.samples
    tau = MO.threshold(30.0)

    def measure(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        med, best = event_ms(fn, a.iters)
        return med, best, peak_bytes(fn)

    # the PIT SI-SNR loss at C = 4 on the same kind of input
    xs, es, ls, _ = MO.make_case(B, 4, T, seed=1)
    src = torch.from_numpy(es).to(dev)
    est = (src + 0.03 * torch.randn_like(src)).requires_grad_(True)
    lens = torch.from_numpy(ls).to(dev)

    def pit_step():
        e = est.clone()                                    # the loss masks its input in place: it refuses a leaf tensor
        torch.autograd.grad(ops.SiSnrPit.apply(src, e, lens)[0], est)

    def clone_only():                                      # the copy alone, to be subtracted by the reader
        with torch.no_grad():
            est.clone()

    pit_ms, pit_min, pit_peak = measure(pit_step)
    clone_ms = measure(clone_only)[0]
    results = []
    for M in a.outputs:
        x, e, ln, _ = MO.make_case(B, M, T, seed=M)
        xd, ld = torch.from_numpy(x).to(dev), torch.from_numpy(ln).to(dev)
        ed = torch.from_numpy(e).to(dev).requires_grad_(True)
        A = torch.from_numpy(MO.assign_matrices(M)).to(device=dev, dtype=torch.float32)

        def hip():
            torch.autograd.grad(ctn.cal_mixit_loss(xd, ed, ld, 30.0)[0], ed)

        def ref():
            torch.autograd.grad(torch_mixit(xd, ed, ld, tau, A), ed)

        def hip_fwd():
            with torch.no_grad():
                ctn.cal_mixit_loss(xd, ed, ld, 30.0)

        hip_ms, hip_min, hip_peak = measure(hip)
        fwd_ms = measure(hip_fwd)[0]
        ref_ms, ref_min, ref_peak = measure(ref)
        lh = float(ctn.cal_mixit_loss(xd, ed, ld, 30.0)[0].detach())
        lr = float(torch_mixit(xd, ed, ld, tau, A).detach())
        gh = torch.autograd.grad(ctn.cal_mixit_loss(xd, ed, ld, 30.0)[0], ed)[0]
        gr = torch.autograd.grad(torch_mixit(xd, ed, ld, tau, A), ed)[0]
        hbm = 4 * B * T * ((M + 2) + (2 * M + 2))             # forward reads M + 2 rows; backward reads M + 2, writes M
        res = {"metric": "mixit_fwd_bwd", "batch": B, "samples": T, "M": M, "snr_max": 30.0,
               "hip_ms_median": hip_ms, "hip_ms_min": hip_min, "hip_fwd_ms_median": fwd_ms, "hip_peak_bytes": hip_peak,
               "torch_ms_median": ref_ms, "torch_ms_min": ref_min, "torch_peak_bytes": ref_peak,
               "speedup_vs_torch": ref_ms / hip_ms, "peak_memory_ratio": ref_peak / max(hip_peak, 1),
               "min_bytes_moved": hbm, "effective_gb_per_s": hbm / (hip_ms * 1e-3) / 1e9,
               "step_share": [hip_ms / STEP_MS[1], hip_ms / STEP_MS[0]],
               "pit_c4_ms_median": pit_ms, "pit_c4_ms_min": pit_min, "pit_c4_clone_ms": clone_ms, "pit_c4_peak_bytes": pit_peak,
               "loss_hip": lh, "loss_torch": lr, "grad_max_abs_diff": float((gh - gr).abs().max()),
               "grad_max_abs": float(gh.abs().max()), "iters": a.iters, "warmup": a.warmup}
        results.append(res)
        print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
