"""GPU: the latency-bound kernels of the step outside the TemporalBlock stacks, at the sizes where their loops change path.

ctn_cln_bwd_finalize (csrc/ctn_cln.hip: cln_bwd_finalize_kernel).  A workgroup owns 64 channels of dgamma or dbeta; wave w adds
the partial rows w, w + 4, ... in row order -- 64 loads in flight per lane while more than 252 rows remain, then eight, then one
-- and the four wave sums are added in wave order.  Rows: 1 (three idle waves), 4, 5, 67 (eight-row batches and a tail), 253
(only wave 0 takes a 64-row batch), 256 (every wave exactly one), 300 (all three loops), 800 (the paper shape: three 64-row
batches).  Ch: 4, 64, 68 (a second, ragged channel block), 256.  Against the fp64 sum under tests/norm_oracle.py's LIMIT["sum"]
(error over the sum of the terms' magnitudes), and bitwise against a torch fp32 restatement that adds in the same order: the
batching must not move a bit.

ctn_mask_apply_bwd (csrc/ctn_codec.hip: mask_apply_bwd2_kernel for C = 2 and 3).  A thread takes two groups of four elements per
trip, the second one a whole grid further on.  All three modes, C = 2 and 3, with N * Kp / 4 groups that are no multiple of the
per-lane batch of two: 9 groups (one workgroup, no thread has a second group), 11 700 groups (23 workgroups: the last 76 threads
that hold a first group have no second), and, relu at C = 2, 2 363 904 groups (beyond the 4096-workgroup cap: a second trip, for part
of the grid).  Through tests/test_gpu_codec.py's check_mask: fp64 torch autograd, its limits (2e-6 of the largest reference element
for the backward, reasoned there), and in place over dsw bitwise the same as into a buffer of its own.

ctn_encoder_fwd (csrc/ctn_codec.hip: encoder_fwd_kernel<L>): w[m, n, k] = relu(sum_l U[n, l] mix[m, k L/2 + l]), zero for k >= K.
A workgroup takes 256 frames x 64 channels.  L = 16 and 20; N = 4, 64, 68 (a partial channel block, a full one, a second ragged
one); K = 1, 2, 255, 257 (one frame; the last lanes of a frame block idle; a second frame block of one frame), Kp =
ctn_padded_frames(K).  Against the fp64 restatement in torch (unfold, matmul, relu).  Limit per element, from the number format: the
kernel adds L products by L fused multiply-adds, each rounding once to within half an ulp of a partial sum that is at most
S = sum_l |U[n, l]| |mix[...]|, so |w - ref| <= L 2^-24 S, and relu does not widen a difference; the pad frames are exact zeros.
"""
import pytest
import torch

import norm_oracle as NO
from test_gpu_codec import check_mask, g

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import ops  # noqa: E402

DEV = "cuda:0"
# rows = M * ceil(Kp / 16) at the default ctn_tune("cln_fr")
FINALIZE_ROWS = {1: (1, 16), 4: (1, 64), 5: (5, 16), 67: (67, 16), 253: (253, 16), 256: (16, 256), 300: (300, 16), 800: (4, 3200)}
FINALIZE_CH = (4, 64, 68, 256)


def _finalize_order(pc):
    """[rows, Ch] fp32 -> [Ch]: wave w = rows w, w + 4, ... added in row order from 0.f, then ((w0 + w1) + w2) + w3."""
    rows, Ch = pc.shape
    part = torch.zeros(4, Ch, dtype=torch.float32)
    for r in range(rows):
        part[r % 4] = part[r % 4] + pc[r]
    return ((part[0] + part[1]) + part[2]) + part[3]


@pytest.mark.parametrize("rows", sorted(FINALIZE_ROWS))
def test_cln_bwd_finalize_rows_and_widths(rows):
    M, Kp = FINALIZE_ROWS[rows]
    assert ctn.lib.ctn_cln_bwd_blocks(M, Kp) == rows == NO.bwd_blocks(M, Kp)
    gen = torch.Generator().manual_seed(4000 + rows)
    for Ch in FINALIZE_CH:
        pc = torch.randn(2, rows, Ch, generator=gen) * torch.rand(1, rows, 1, generator=gen) * 10
        dap = torch.randn(rows, generator=gen)
        pcd, dapd = pc.to(DEV), dap.to(DEV)
        out = torch.full((3, Ch + 2), float("nan"), device=DEV)         # dgamma, dbeta, dalpha rows with a guard word on both sides
        ctn.lib.call("ctn_cln_bwd_finalize", ops._p(pcd), ops._p(dapd), M, Ch, Kp, out[0, 1:].data_ptr(), out[1, 1:].data_ptr(),
                     out[2, 1:].data_ptr(), ops._stream())
        torch.cuda.synchronize()
        o = out.cpu()
        assert bool(torch.isnan(o[:, 0]).all()) and bool(torch.isnan(o[:2, Ch + 1]).all()) and bool(torch.isnan(o[2, 2:]).all())
        for f in range(2):
            got = o[f, 1:Ch + 1]
            e = NO.sum_err(got, pc[f].double().sum(0), pc[f].double().abs().sum(0))
            print("finalize rows %d Ch %d output %d: sum error %.2e (limit %.0e)" % (rows, Ch, f, e, NO.LIMIT["sum"]))
            assert e < NO.LIMIT["sum"], (rows, Ch, f, e)
            assert torch.equal(got, _finalize_order(pc[f])), (rows, Ch, f)
        e = NO.sum_err(o[2, 1:2], dap.double().sum().reshape(1), dap.double().abs().sum().reshape(1))
        assert e < NO.LIMIT["sum"], (rows, "dalpha", e)


MASK_SHAPES = [(1, 3, 12), (3, 20, 260)]            # (M, N, Kp): 9 and 11 700 groups of four


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("C", [2, 3])
@pytest.mark.parametrize("M,N,Kp", MASK_SHAPES)
def test_mask_apply_bwd_two_groups_per_lane(M, N, Kp, C, mode):
    assert (M * N * Kp // 4) % 2 == 1 or (M * N * Kp // 4) % (2 * 256) != 0
    score = torch.randn(M, C, N, Kp, generator=g(11)) * 2.0
    w = torch.rand(M, N, Kp, generator=g(12)) + 0.1
    dsw = torch.randn(M, C, N, Kp, generator=g(13))
    check_mask(score, w, dsw, mode, "two-group")


def test_mask_apply_bwd_second_trip():
    """More groups than two per thread of the capped grid (4096 workgroups of 256 threads): part of the grid makes a second trip."""
    M, C, N, Kp = 9, 2, 512, 2052
    assert M * N * Kp // 4 > 2 * 4096 * 256 and (M * N * Kp // 4) % (2 * 4096 * 256) != 0
    score = torch.randn(M, C, N, Kp, generator=g(21)) * 2.0
    w = torch.rand(M, N, Kp, generator=g(22)) + 0.1
    dsw = torch.randn(M, C, N, Kp, generator=g(23))
    check_mask(score, w, dsw, 0, "second trip")


ENC_N, ENC_K = (4, 64, 68), (1, 2, 255, 257)


@pytest.mark.parametrize("N", ENC_N)
@pytest.mark.parametrize("L", [16, 20])
def test_encoder_fwd_frames_and_widths(L, N):
    M, S = 2, L // 2
    for K in ENC_K:
        T, Kp = (K - 1) * S + L, ops.padded_frames(K)
        gen = g(300 + 100 * L + N + K)
        mix = torch.randn(M, T, generator=gen)
        U = torch.randn(N, L, generator=gen) * 0.3
        fr = mix.double().unfold(1, L, S)                                   # [M, K, L]
        assert fr.shape[1] == K
        pre = torch.einsum("nl,mkl->mnk", U.double(), fr)
        mag = torch.einsum("nl,mkl->mnk", U.double().abs(), fr.abs())
        out = torch.full((M * N * Kp + 8,), float("nan"), device=DEV)       # four guard words on both sides
        mix_d, U_d = mix.to(DEV), U.to(DEV)
        ctn.lib.call("ctn_encoder_fwd", ops._p(mix_d), ops._p(U_d), out[4:].data_ptr(), M, T, N, L, K, Kp, ops._stream())
        torch.cuda.synchronize()
        o = out.cpu()
        assert bool(torch.isnan(o[:4]).all()) and bool(torch.isnan(o[-4:]).all()), "a guard word was written"
        w = o[4:-4].view(M, N, Kp)
        assert float(w[..., K:].abs().sum()) == 0.0 and not bool(torch.isnan(w).any()), (L, N, K)
        err = (w[..., :K].double() - torch.relu(pre)).abs()
        worst = float((err / (L * 2.0 ** -24 * mag).clamp_min(1e-300)).max())
        print("ENCODER L=%d N=%d K=%d Kp=%d: largest error over its bound %.2f" % (L, N, K, Kp, worst))
        assert worst <= 1.0, (L, N, K, worst)
