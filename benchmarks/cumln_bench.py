#!/usr/bin/env python
"""Time the cumulative LayerNorm against the per-frame channel-wise one of the same build, at the causal paper shape [8, 512, 3199]:
the two norms with passes of their own (ctn_cumln_fwd / _bwd vs ctn_cln_fwd / _bwd), the two per-frame kernels (the scans vs
ctn_cln_stats_frame / ctn_cln_bwd_frame), the two cumLN passes with the h3 maximum tracked (ctn_cumln_fwd_amax / _bwd_amax) against the
untracked pass and against the untracked pass followed by the ctn_absmax_rows pass that tracking replaces, and the causal paper-config
training step: norm_type cumLN and cLN, each block by block and through its composite stack (ops._COMPOSITE toggled per step).  The
variants of a group alternate inside one process; every figure is the median of `reps` windows, with the windows' range beside it.

usage: python benchmarks/cumln_bench.py [--no-step] [--json OUT]      (prints a table and, with --json, writes the figures)"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import ops  # noqa: E402
from conv_tasnet_amd.optim import FlatAdam  # noqa: E402
from conv_tasnet_amd.train import SyntheticLoader  # noqa: E402

M, H, K = 8, 512, 3199
Kp = ops.padded_frames(K)
dev = "cuda:0"
res = {"shape": [M, H, K], "Kp": Kp}


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3            # us per call


def pair(name, a, b, iters=50, reps=7):
    """Median us of a (cumLN) and b (cLN), measured in alternating windows."""
    for _ in range(5):
        a(); b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(window(a, iters))
        tb.append(window(b, iters))
    x, y = statistics.median(ta), statistics.median(tb)
    res[name] = {"cumln_us": round(x, 2), "cln_us": round(y, 2), "ratio": round(x / y, 3), "cumln_spread_us": [round(min(ta), 2), round(max(ta), 2)],
                 "cln_spread_us": [round(min(tb), 2), round(max(tb), 2)]}
    print("%-12s cumLN %8.1f us [%6.1f .. %6.1f]   cLN %8.1f us [%6.1f .. %6.1f]   ratio %.2f" % (name, x, min(ta), max(ta), y, min(tb), max(tb), x / y), flush=True)


def group(name, fns, iters=50, reps=7):
    """{label: median us} of the variants `fns` = {label: fn}, measured in alternating windows; res[name][label] = {us, spread_us}."""
    for _ in range(5):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t[k].append(window(fn, iters))
    res[name] = {k: {"us": round(statistics.median(v), 2), "spread_us": [round(min(v), 2), round(max(v), 2)]} for k, v in t.items()}
    for k, v in t.items():
        print("%-12s %-22s %9.1f us [%8.1f .. %8.1f]" % (name, k, statistics.median(v), min(v), max(v)), flush=True)
    return {k: statistics.median(v) for k, v in t.items()}


torch.manual_seed(0)
y = torch.randn(M, H, Kp, device=dev) + 0.3
y[..., K:] = 0
dout = torch.randn(M, H, Kp, device=dev)
dout[..., K:] = 0
g, b = 1 + 0.3 * torch.randn(H, device=dev), 0.3 * torch.randn(H, device=dev)
a = torch.full((1,), 0.25, device=dev)
nbytes = M * H * Kp * 4

_, mean_c, rstd_c = ops.cumln_fwd(y, g, b, a, K)
_, mean_f, rstd_f = ops.cln_fwd(y, g, b, a, K)
pair("fwd", lambda: ops.cumln_fwd(y, g, b, a, K), lambda: ops.cln_fwd(y, g, b, a, K))
pair("bwd", lambda: ops.cumln_bwd(dout, y, mean_c, rstd_c, g, a, K), lambda: ops.cln_bwd(dout, y, mean_f, rstd_f, g, a, K))
for k, passes in (("fwd", (3, 2)), ("bwd", (5, 3))):
    res[k]["cumln_TBps"] = round(passes[0] * nbytes / res[k]["cumln_us"] / 1e6, 2)
    res[k]["cln_TBps"] = round(passes[1] * nbytes / res[k]["cln_us"] / 1e6, 2)
    res[k]["byte_ratio"] = round(passes[0] / passes[1], 2)
nparts = ctn.lib.ctn_pw_col_parts(M, H, Kp, 3)                 # the row tiles of the h3 GEMM that feeds the frame kernels in the step
colp = torch.rand(M, nparts, Kp, 2, dtype=torch.float64, device=dev)
res["frame_nparts"] = nparts
pair("stats_frame", lambda: ops.cumln_stats_frame(colp, H, K), lambda: ops.cln_stats_frame(colp, H), iters=100)
pair("bwd_frame", lambda: ops.cumln_bwd_frame(colp, mean_c, rstd_c, H, K), lambda: ops.cln_bwd_frame(colp, mean_f, rstd_f, H), iters=100)

# the two passes with and without the tracked maximum, on buffers allocated once (the differences are a few us)
lib, p_ = ctn.lib, ops._p
out_, mean_, rstd_ = torch.empty_like(y), torch.empty(M, Kp, device=dev), torch.empty(M, Kp, device=dev)
work_ = torch.empty(lib.ctn_cumln_work_bytes(M, Kp), dtype=torch.uint8, device=dev)
pc_ = torch.empty(lib.ctn_cln_bwd_pc_floats(M, H, Kp), device=dev)
dap_ = torch.empty(lib.ctn_cln_bwd_blocks(M, Kp), device=dev)
amax_ = torch.zeros(M, ops.AMAX_SLOTS, dtype=torch.int32, device=dev)


def fwd_pass(amax):
    lib.call("ctn_cumln_fwd_amax", p_(y), p_(out_), p_(mean_), p_(rstd_), M, H, K, Kp, p_(g), p_(b), p_(a), 0, 0, p_(work_), p_(amax), ops._stream())


def bwd_pass(amax):
    lib.call("ctn_cumln_bwd_amax", p_(dout), p_(y), p_(out_), p_(mean_c), p_(rstd_c), M, H, K, Kp, p_(g), p_(a), p_(dap_), p_(pc_), p_(work_), p_(amax),
             ops._stream())


for k, fn in (("fwd_amax", fwd_pass), ("bwd_amax", bwd_pass)):
    t = group(k, {"untracked": lambda fn=fn: fn(None), "tracked": lambda fn=fn: fn(amax_),
                  "untracked+absmax_rows": lambda fn=fn: (fn(None), ops.absmax_rows(out_, amax_))}, iters=100)
    res[k]["tracking_cost_us"] = round(t["tracked"] - t["untracked"], 2)
    res[k]["absmax_rows_pass_us"] = round(t["untracked+absmax_rows"] - t["untracked"], 2)

if "--no-step" not in sys.argv:
    mix, lens, src = next(iter(SyntheticLoader(1, 8, samples=32000, C=2, sample_rate=8000)))
    mix, lens, src = mix.to(dev), lens.to(dev), src.to(dev)
    steps = {}
    for norm in ("cumLN", "cLN"):
        torch.manual_seed(0)
        m = ctn.ConvTasNet(256, 20, 256, 512, 3, 8, 4, 2, norm_type=norm, causal=True).to(dev)
        opt = FlatAdam(m.parameters(), lr=1e-3)

        def step(composite, m=m, opt=opt):
            ops._COMPOSITE = composite              # read by ConvTasNet.blocks() in the forward pass; the backward follows the node
            opt.zero_grad()
            ctn.cal_loss(src, m(mix), lens)[0].backward()
            opt.step(max_grad_norm=5.0)
        for composite in (False, True):
            steps["%s_%s" % (norm, "composite" if composite else "block")] = lambda step=step, composite=composite: step(composite)
    saved = ops._COMPOSITE
    try:
        t = group("step_variants", steps, iters=10, reps=7)
    finally:
        ops._COMPOSITE = saved
    sv = res["step_variants"]
    # block by block, cumLN against cLN (the figures this file has always reported), then the composite against the block path
    res["step"] = {"ratio": round(t["cumLN_block"] / t["cLN_block"], 3), "cumln_spread_us": sv["cumLN_block"]["spread_us"],
                   "cln_spread_us": sv["cLN_block"]["spread_us"], "cumln_ms": round(t["cumLN_block"] / 1e3, 3), "cln_ms": round(t["cLN_block"] / 1e3, 3)}
    res["step_composite"] = {"cumln_ms": round(t["cumLN_composite"] / 1e3, 3), "cln_ms": round(t["cLN_composite"] / 1e3, 3),
                             "cumln_block_over_composite": round(t["cumLN_block"] / t["cumLN_composite"], 3),
                             "cln_block_over_composite": round(t["cLN_block"] / t["cLN_composite"], 3),
                             "cumln_over_cln": round(t["cumLN_composite"] / t["cLN_composite"], 3)}

if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res))
