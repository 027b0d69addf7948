#!/usr/bin/env python
"""Parent library against the new one in ONE process, interleaved rounds: the h3 GEMM forms of benchmarks/gemm_only.py plus the cLN
input-gradient GEMM, paper shape.  usage: python benchmarks/ab_gemm_libs.py other/libctn_hip.so [rounds] [n]"""
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import ops  # noqa: E402
from conv_tasnet_amd.ops import _p  # noqa: E402

parent_path = sys.argv[1]
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 10
n = int(sys.argv[3]) if len(sys.argv) > 3 else 100
assert ctn.gemm_arith() == "h3"
new = ctn.lib.load()
parent = ctypes.CDLL(parent_path)
for name, (res, args, _) in ctn.lib.protos.items():
    fn = getattr(parent, name)
    fn.restype, fn.argtypes = res, args

dev = "cuda:0"
M, K = 8, 3199
Kp = ops.padded_frames(K)
B, H = 256, 512
torch.manual_seed(0)
xB = torch.randn(M, B, Kp, device=dev); xB[..., K:] = 0
xH = torch.randn(M, H, Kp, device=dev); xH[..., K:] = 0
w1 = torch.randn(H, B, device=dev) * 0.05
w2 = torch.randn(B, H, device=dev) * 0.05
a = torch.full((1,), 0.25, device=dev)
g = torch.randn(1, H, 1, device=dev)
b = torch.randn(1, H, 1, device=dev)
ms = torch.tensor([[0.1, 1.3]] * M, device=dev)
pre = torch.where(xH >= 0, xH, 0.25 * xH).double()
st2 = torch.stack([pre[..., :K].sum((1, 2)), (pre[..., :K] ** 2).sum((1, 2))], -1).reshape(M, 1, 2).contiguous()
cmean = pre.mean(1).float().contiguous()
crstd = (1.0 / torch.sqrt(pre.var(1, unbiased=False) + 1e-8)).float().contiguous()
outH = torch.empty(M, H, Kp, device=dev)
outB = torch.empty(M, B, Kp, device=dev)
part = torch.empty((M, new.ctn_pw_stats_parts(M, H, Kp), 2), dtype=torch.float64, device=dev)
col = torch.empty((M, new.ctn_pw_col_parts(M, H, Kp, 3), Kp, 2), dtype=torch.float64, device=dev)
sm = ops._stream()
P1, P2 = ops.h3_pieces(w1, H, B, False), ops.h3_pieces(w2, B, H, False)
Q2, Q1 = ops.h3_pieces(w2, H, B, True), ops.h3_pieces(w1, B, H, True)
axB, axH, gbm = ops.absmax_rows(xB), ops.absmax_rows(xH), ops.absmax_of(g, b)
oam = torch.zeros(M, ops.AMAX_SLOTS, dtype=torch.int32, device=dev)
N_ = None
forms = {
    "K1": ("ctn_pw_gemm_h3", (_p(P1), _p(xB), _p(outH), M, H, B, K, Kp, N_, 0, N_, N_, N_, N_, N_, _p(a), _p(part), _p(axB), N_, N_, sm)),
    "K3": ("ctn_pw_gemm_h3", (_p(P2), _p(xH), _p(outB), M, B, H, K, Kp, _p(st2), 1, _p(g), _p(b), _p(a), N_, _p(xB), N_, N_, _p(axH), _p(gbm), _p(oam), sm)),
    "B1": ("ctn_pw_dgrad_gln_h3", (_p(Q2), _p(xB), _p(outH), M, H, B, K, Kp, _p(xH), _p(g), _p(a), _p(ms), _p(part), _p(axB), sm)),
    "B5": ("ctn_pw_gemm_h3", (_p(Q1), _p(xH), _p(outB), M, B, H, K, Kp, N_, 0, N_, N_, N_, N_, _p(xB), N_, N_, _p(axH), N_, _p(oam), sm)),
    "C1": ("ctn_pw_dgrad_cln", (_p(Q2), 3, _p(xB), _p(outH), M, H, B, K, Kp, _p(xH), _p(g), _p(a), _p(cmean), _p(crstd), _p(col), _p(axB), sm)),
}


def timed(dll, name, args):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        rc = getattr(dll, name)(*args)
        assert rc == 0, (name, rc)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


for form, (name, args) in forms.items():
    res = {"parent": [], "new": []}
    for dll in (parent, new):
        timed(dll, name, args)
    for r in range(rounds):
        order = (("parent", parent), ("new", new)) if r % 2 == 0 else (("new", new), ("parent", parent))
        for label, dll in order:
            res[label].append(timed(dll, name, args))
    mp, mn = statistics.median(res["parent"]), statistics.median(res["new"])
    print("%s parent median %.2f min %.2f max %.2f | new median %.2f min %.2f max %.2f | new - parent %+.2f us (%+.1f %%)"
          % (form, mp, min(res["parent"]), max(res["parent"]), mn, min(res["new"]), max(res["new"]), mn - mp, 100 * (mn - mp) / mp), flush=True)
    print("   parent", " ".join("%.2f" % v for v in res["parent"]))
    print("   new   ", " ".join("%.2f" % v for v in res["new"]), flush=True)
