#!/usr/bin/env python
"""Launch only the gLN-1 / PReLU-1 backward (B4: ctn_gln_prelu_bwd) at the paper shape, for timing / rocprofv3 --pmc.  The stack
calls it in place; here the result goes to a buffer of its own, so every launch reads the same inputs (in place, the random sums
below would drive dn to inf within a few launches).  The traffic is the same 2 reads + 1 write.
usage: python benchmarks/gln_prelu_bwd_only.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import ops  # noqa: E402
from conv_tasnet_amd.ops import _p  # noqa: E402

M, H, K = 8, 512, 3199
Kp = ops.padded_frames(K)
dev = "cuda:0"
dn, y = torch.randn(M, H, Kp, device=dev), torch.randn(M, H, Kp, device=dev)
for t in (dn, y):
    t[..., K:] = 0
g = torch.randn(H, device=dev)
al = torch.full((1,), 0.25, device=dev)
ms = torch.tensor([[0.1, 1.2]] * M, device=dev)
nparts = H
sp = torch.randn(M, nparts, 2, device=dev, dtype=torch.float64)
dy = torch.empty_like(dn)
dap = torch.empty(M * H, device=dev)
amax = torch.zeros((M, ops.AMAX_SLOTS), dtype=torch.int32, device=dev)


def run():
    ctn.lib.call("ctn_gln_prelu_bwd", _p(dn), _p(y), _p(dy), M, H, K, Kp, _p(g), _p(al), _p(ms), _p(sp), nparts, _p(dap), _p(amax),
                 ops._stream())


for _ in range(5):
    run()
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(50):
    run()
e1.record()
torch.cuda.synchronize()
us = e0.elapsed_time(e1) / 50 * 1e3
print("gln_prelu_bwd: %.1f us  (%.2f TB/s on 3 x M*H*Kp*4 bytes)" % (us, 3 * M * H * Kp * 4 / us / 1e6))
