"""Optimal-assignment PIT: forward plus backward of the HIP kernels (assign.py, csrc/ctn_assign.hip) against
  * cal_loss (ops.SiSnrPit, the C! search) where it runs, C <= 6, in the same process;
  * a torch restatement for every C: the pairwise SI-SNR in the reference's form -- the dot products by einsum, the projections and
    the noise as [B,C,C,T] tensors --, a read-back, scipy.optimize.linear_sum_assignment on the host, and autograd.  This is what a
    user would write today;
  * the HBM floor: the forward reads the 2 B C T fp32 samples once (2 B C T 4 bytes), the backward reads them again and writes
    B C T 4 bytes of gradient: 5 B C T 4 bytes in all, at the 6.29 TB/s a float4 copy reaches on this chip.

Inputs: the planted cases of tests/assign_oracle.py at B = 8, T = 32000 (the training segment), C in {2, 4, 6, 8, 12, 16}.  One timed
call = loss forward + the gradient with respect to the estimates.  Timing: warm-up calls, then per iteration two device events
around the call on its stream, the forms under comparison taking turns in five rounds (the first measurement of the process is
thrown away); the median, the minimum and the 10th / 90th percentiles over the iterations are reported (the spread of this same
run is what a difference has to exceed).  Peak memory: torch's peak of allocated bytes over one call, above
what was allocated before it.  One JSON line per C, and all of them as a list into --out.

    python benchmarks/assign_bench.py [--batch 8] [--samples 32000] [--speakers 2 4 6 8 12 16] [--iters 100] [--warmup 10] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import ops  # noqa: E402
import assign_oracle as AO  # noqa: E402

EPS = 1e-8
ROUNDS = 5
COPY_BYTES_PER_S = 6.29e12      # measured float4 copy on the MI355X (8.0 TB/s spec)


def event_ms(fn, iters):
    out = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def summary(out):
    return {"median": float(np.median(out)), "min": float(min(out)), "p10": float(np.percentile(out, 10)),
            "p90": float(np.percentile(out, 90))}


def peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def torch_assign(s, e, lens):
    """The textbook form in fp32: every pair's projection and noise as [B,C,C,T] tensors, the assignment on the host."""
    T = e.shape[2]
    keep = (torch.arange(T, device=e.device)[None, None, :] < lens[:, None, None]).to(e.dtype)
    n = lens.view(-1, 1, 1).to(e.dtype)
    sc = (s - (s * keep).sum(-1, keepdim=True) / n) * keep
    ec = (e - (e * keep).sum(-1, keepdim=True) / n) * keep
    dot = torch.einsum("bit,bjt->bij", ec, sc).unsqueeze(-1)                         # [B,C,C,1]: estimate i, reference j
    energy = (sc * sc).sum(-1)[:, None, :, None] + EPS
    proj = dot * sc.unsqueeze(1) / energy                                            # [B,C,C,T]
    noise = ec.unsqueeze(2) - proj
    snr = 10.0 * torch.log10((proj * proj).sum(-1) / ((noise * noise).sum(-1) + EPS) + EPS)
    cols = np.stack([linear_sum_assignment(m, maximize=True)[1] for m in snr.detach().cpu().numpy()])
    idx = torch.from_numpy(cols).to(e.device)
    return -snr.gather(2, idx.unsqueeze(-1)).squeeze(-1).mean(1).mean(), idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--samples", type=int, default=32000)
    ap.add_argument("--speakers", type=int, nargs="+", default=[2, 4, 6, 8, 12, 16])
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("assign_bench needs the GPU")
    dev = torch.device("cuda:0")
    ctn.lib.load()
    B, T = a.batch, a.samples

    def measure(fns):
        """{name: fn} -> {name: timing summary}: every fn warmed up, then ROUNDS rounds that take the fns in turn, iters / ROUNDS
        timed calls each, so that a drift of the host or the clocks during the run meets all of them alike."""
        for fn in fns.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(ROUNDS):
            for k, fn in fns.items():
                times[k] += event_ms(fn, max(a.iters // ROUNDS, 1))
        return {k: summary(v) for k, v in times.items()}

    results = []
    for C in a.speakers:
        s, e, ln, _ = AO.make_case(B, C, T, seed=C)
        sd, ld = torch.from_numpy(s).to(dev), torch.from_numpy(ln).to(dev)
        ed = torch.from_numpy(e).to(dev).requires_grad_(True)

        def hip():
            torch.autograd.grad(ctn.cal_assign_loss(sd, ed, ld)[0], ed)

        def hip_fwd():
            with torch.no_grad():
                ctn.cal_assign_loss(sd, ed, ld)

        def ref():
            torch.autograd.grad(torch_assign(sd, ed, ld)[0], ed)

        def pit():
            c = ed.clone()                                     # cal_loss masks its input in place: it refuses a leaf tensor
            torch.autograd.grad(ops.SiSnrPit.apply(sd, c, ld)[0], ed)

        def clone_only():                                      # the copy alone, to be subtracted by the reader
            with torch.no_grad():
                ed.clone()

        fns = {"hip": hip, "fwd": hip_fwd, "ref": ref}
        if C <= 6:
            fns.update({"pit": pit, "clone": clone_only})
        if not results:
            measure(fns)                                       # the first measurement of a process runs slow: thrown away
        t = measure(fns)
        hip_t, fwd_t, ref_t = t["hip"], t["fwd"], t["ref"]
        hip_peak, ref_peak = peak_bytes(hip), peak_bytes(ref)
        loss_h, _, _, perm_h = ctn.cal_assign_loss(sd, ed, ld)
        loss_r, perm_r = torch_assign(sd, ed, ld)
        gh = torch.autograd.grad(loss_h, ed)[0]
        gr = torch.autograd.grad(loss_r, ed)[0]
        floor_bytes = 5 * B * C * T * 4
        res = {"metric": "assign_fwd_bwd", "batch": B, "samples": T, "C": C,
               "hip_ms": hip_t, "hip_fwd_ms": fwd_t, "hip_peak_bytes": hip_peak,
               "torch_ms": ref_t, "torch_peak_bytes": ref_peak,
               "speedup_vs_torch": ref_t["median"] / hip_t["median"], "peak_memory_ratio": ref_peak / max(hip_peak, 1),
               "floor_bytes": floor_bytes, "floor_ms": floor_bytes / COPY_BYTES_PER_S * 1e3,
               "effective_gb_per_s": floor_bytes / (hip_t["median"] * 1e-3) / 1e9,
               "loss_hip": float(loss_h.detach()), "loss_torch": float(loss_r.detach()),
               "perm_equal": bool(torch.equal(perm_h, perm_r)), "grad_max_abs_diff": float((gh - gr).abs().max()),
               "grad_max_abs": float(gh.abs().max()), "iters": a.iters, "warmup": a.warmup}
        if C <= 6:
            pit_t, clone_t, pit_peak = t["pit"], t["clone"], peak_bytes(pit)
            res.update({"cal_loss_ms": pit_t, "cal_loss_clone_ms": clone_t, "cal_loss_peak_bytes": pit_peak,
                        "hip_over_cal_loss": hip_t["median"] / pit_t["median"]})
        results.append(res)
        print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
