"""GPU: ctn_pw_wgrad on the skinny shapes of the front and back end (encoder and decoder bases, min(R, Cn) <= 32).

dW [R, Cn] = sum over utterances and frames of dOut [M, R, Kp] X [M, Cn, Kp]^T, without the operand prologue.  These shapes run the
128 x 128 fp32-MFMA tile with most of its columns (or rows) empty, a split-K partition and slab_reduce; a form made for them has to
give these gradients.  Shapes (R, Cn): (256, 20) and (20, 256) (the bases of the paper model at half its width), (64, 4), (4, 64),
(32, 32); K = 1, 31, 32, 33, 257 frames (one frame; either side of two k-tiles of 16; more than one 256-frame split-K chunk) in
Kp = ctn_padded_frames(K), pad frames zero in both operands; M = 1 and 3 utterances.

Against the fp64 product under the limit tests/test_gpu_gemm_seams.py holds dW to (tests/gemm_oracle.py: LIMIT["pro"] = 5e-6 of the
largest reference element, err_of's figure for a matrix), and bitwise from one call to the next: the slabs are summed in a fixed
order.  The workspace is filled with NaN before each call and dW carries a guard row on both sides.
"""
import pytest
import torch

import gemm_oracle as GO

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import ops  # noqa: E402

DEV = "cuda:0"
SHAPES = [(256, 20), (20, 256), (64, 4), (4, 64), (32, 32)]
FRAMES = (1, 31, 32, 33, 257)
LIMIT = GO.LIMIT["pro"]


def _wgrad(g, x, R, Cn, K, Kp):
    M = g.shape[0]
    nbytes = ctn.lib.ctn_pw_wgrad_workspace(M, R, Cn, Kp)
    ws = torch.full((max(nbytes // 4, 1),), float("nan"), device=DEV)
    out = torch.full((R + 2, Cn), float("nan"), device=DEV)
    ctn.lib.call("ctn_pw_wgrad", ops._p(g), ops._p(x), out[1:].data_ptr(), M, R, Cn, K, Kp, 0, 0, 0, 0, ops._p(ws), nbytes, ops._stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[0]).all()) and bool(torch.isnan(out[R + 1]).all()), "a guard row was written"
    return out[1:R + 1].cpu()


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("R,Cn", SHAPES)
def test_skinny_weight_gradient_vs_fp64_and_run_to_run(R, Cn, M):
    for K in FRAMES:
        Kp = ops.padded_frames(K)
        gen = torch.Generator().manual_seed(1000 * R + 10 * Cn + K + M)
        keep = (torch.arange(Kp) < K).float()
        g = torch.randn(M, R, Kp, generator=gen) * keep
        x = (torch.randn(M, Cn, Kp, generator=gen) + 0.3) * keep
        ref = torch.einsum("mrk,mck->rc", g.double(), x.double())
        g_d, x_d = g.to(DEV), x.to(DEV)
        a, b = _wgrad(g_d, x_d, R, Cn, K, Kp), _wgrad(g_d, x_d, R, Cn, K, Kp)
        assert bool(torch.isfinite(a).all()), (R, Cn, K, M)
        assert torch.equal(a, b), (R, Cn, K, M, "second call differs")
        e = float((a.double() - ref).abs().max() / ref.abs().max())
        print("SMALL WGRAD R=%-3d Cn=%-3d K=%-3d Kp=%-3d M=%d dW=%.2e (limit %.0e)" % (R, Cn, K, Kp, M, e, LIMIT))
        assert e < LIMIT, (R, Cn, K, M, e)
