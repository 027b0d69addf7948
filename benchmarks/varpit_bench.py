"""PIT with inactive sources: forward plus backward of the HIP kernels (varpit.py, csrc/ctn_varpit.hip) against the PIT SI-SNR loss
(cal_loss) at the same C in the same process, and against a torch restatement that builds the [B, C, C, T] differences.

Inputs: the planted cases of tests/varpit_oracle.py at B = 8, T = 32000 (the training segment), C = 2 .. 6, active counts cycling
through 1 .. C.  One timed call = loss forward + the gradient with respect to the estimates.  cal_loss masks its input in place and
refuses a leaf tensor, so its call carries one clone of the estimates; the clone alone is timed too.  Timing: warm-up calls, then
per iteration two device events around the call on its stream; the median over the iterations is reported.  The forward alone
(moments + assignment kernels) is timed as well, so the backward kernel's share is the difference.  Peak memory: torch's peak of
allocated bytes over one call, above what was allocated before it.  One JSON line per C, and all of them as a list into --out.

    python benchmarks/varpit_bench.py [--batch 8] [--samples 32000] [--sources 2 3 4 5 6] [--iters 200] [--warmup 20] [--out FILE]
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
import varpit_oracle as VO  # noqa: E402


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


def torch_varpit(s, e, lens, tau, tau0, perms):
    """The textbook form in fp32: every estimate minus every reference, the pair losses, all C! totals, the minimum."""
    B, C, T = e.shape
    keep = (torch.arange(T, device=e.device)[None, None, :] < lens[:, None, None]).to(e.dtype)
    sm, em = s * keep, e * keep
    diff = em[:, :, None, :] - sm[:, None, :, :]                       # [B,C,C,T]
    err = (diff * diff).sum(-1)
    ss, ee = (sm * sm).sum(-1), (em * em).sum(-1)
    xx = (sm.sum(1) ** 2).sum(-1)
    act = 10.0 * torch.log10((err + tau * ss[:, None, :] + VO.EPS) / (ss[:, None, :] + VO.EPS))
    ina = 10.0 * torch.log10((ee + tau0 * xx[:, None] + VO.EPS) / (xx[:, None] + VO.EPS))[:, :, None].expand_as(act)
    pair = torch.where((ss > 0)[:, None, :], act, ina)
    L = pair[:, torch.arange(C, device=e.device)[None, :], perms].sum(-1) / C          # [B, C!]
    return L.min(dim=1).values.mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--samples", type=int, default=32000)
    ap.add_argument("--sources", type=int, nargs="+", default=[2, 3, 4, 5, 6])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("varpit_bench needs the GPU")
    dev = torch.device("cuda:0")
    ctn.lib.load()
    B, T = a.batch, a.samples
    tau, tau0 = VO.threshold(30.0), VO.threshold(20.0)

    def measure(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        med, best = event_ms(fn, a.iters)
        return med, best, peak_bytes(fn)

    results = []
    for C in a.sources:
        s, e, ln, _ = VO.make_case(B, C, T, seed=C)
        sd, ld = torch.from_numpy(s).to(dev), torch.from_numpy(ln).to(dev)
        ed = torch.from_numpy(e).to(dev).requires_grad_(True)
        perms = ops._perms(C, dev)[1]

        def hip():
            torch.autograd.grad(ctn.cal_varpit_loss(sd, ed, ld, 30.0, 20.0)[0], ed)

        def hip_fwd():
            with torch.no_grad():
                ctn.cal_varpit_loss(sd, ed, ld, 30.0, 20.0)

        def pit():
            x = ed.clone()                                     # the loss masks its input in place: it refuses a leaf tensor
            torch.autograd.grad(ops.SiSnrPit.apply(sd, x, ld)[0], ed)

        def pit_fwd():
            with torch.no_grad():
                ops.SiSnrPit.apply(sd, ed.clone(), ld)

        def clone_only():
            with torch.no_grad():
                ed.clone()

        def ref():
            torch.autograd.grad(torch_varpit(sd, ed, ld, tau, tau0, perms), ed)

        hip_ms, hip_min, hip_peak = measure(hip)
        fwd_ms = measure(hip_fwd)[0]
        pit_ms, pit_min, pit_peak = measure(pit)
        pit_fwd_ms = measure(pit_fwd)[0]
        clone_ms = measure(clone_only)[0]
        ref_ms, ref_min, ref_peak = measure(ref)
        lh = float(ctn.cal_varpit_loss(sd, ed, ld, 30.0, 20.0)[0].detach())
        lr = float(torch_varpit(sd, ed, ld, tau, tau0, perms).detach())
        gh = torch.autograd.grad(ctn.cal_varpit_loss(sd, ed, ld, 30.0, 20.0)[0], ed)[0]
        gr = torch.autograd.grad(torch_varpit(sd, ed, ld, tau, tau0, perms), ed)[0]
        hbm = 4 * B * T * (2 * C + 3 * C)                      # forward reads 2C rows; backward reads at most 2C, writes C
        res = {"metric": "varpit_fwd_bwd", "batch": B, "samples": T, "C": C, "snr_max": 30.0, "inactive_snr_max": 20.0,
               "hip_ms_median": hip_ms, "hip_ms_min": hip_min, "hip_fwd_ms_median": fwd_ms, "hip_bwd_ms": hip_ms - fwd_ms,
               "hip_peak_bytes": hip_peak,
               "pit_ms_median": pit_ms, "pit_ms_min": pit_min, "pit_fwd_ms_median": pit_fwd_ms, "pit_clone_ms": clone_ms,
               "pit_peak_bytes": pit_peak, "ratio_vs_pit": hip_ms / pit_ms, "ratio_vs_pit_without_clone": hip_ms / (pit_ms - clone_ms),
               "torch_ms_median": ref_ms, "torch_ms_min": ref_min, "torch_peak_bytes": ref_peak,
               "speedup_vs_torch": ref_ms / hip_ms, "peak_memory_ratio": ref_peak / max(hip_peak, 1),
               "min_bytes_moved": hbm, "effective_gb_per_s": hbm / (hip_ms * 1e-3) / 1e9,
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
