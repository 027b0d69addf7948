"""GPU: the weight operands that a composite gLN stack call prepares in one launch are, byte for byte, those of the per-kernel path.

prepare_weights (csrc/ctn_block.hip) writes, for the h3 arithmetic, both GEMM operands of every block and {max |gamma2|,
max |beta2|} with ONE launch of prep_h3_kernel (csrc/ctn_gemm_b3.h) per 32 blocks.  ctn_split_h3_batch and ctn_absmax_batch keep
their own kernels (one maximum launch, one split launch), so they are an independent statement of the same bytes: this module
runs one training step of a small model, reads the prepared region out of the stack's forward and backward workspaces and
compares it with what the two exported calls give for the same tensors, called matrix by matrix.

Where the region lies.  Both workspaces end with it (csrc/ctn_block.hip: fwd_ws, bwd_ws): forward
[... | nblocks x 2 operand slots | gb], backward [... | nblocks x 2 operand slots | gb | amax], a slot being the largest of the
fp32 matrix and its b3 / h3 piece forms rounded up to 256 bytes, gb = nblocks x 2 floats and amax = nblocks x 2 x M x AMAX_SLOTS
words, each rounded up to 256 bytes.  The offsets are taken from the END of the exported workspace sizes.  Slot 0 of a block is
the operand with H output rows (forward: w1 as stored; backward: w2 used transposed), slot 1 the one with B rows.

Compared: the piece bytes and the maximum word behind them (ctn_split_h3_bytes minus the 12 unused bytes of its 16-byte tail), and
gb.  Shapes (H, B) = (64, 64), (128, 64), (96, 160): one fragment-row tile and several, a row count that is no multiple of 32 with
a column count that is no multiple of 32 in the other operand; nblocks = 1, 2, 3 and 33 (a second launch: 32 blocks per launch,
below the 64-entry tables of the exported calls).  Block 0's w1 is all zeros (maximum 0: the scale of an empty range) and the
last block's w2 has one element of 1e30 (every other element underflows in the pieces); what the step computes from them is not
looked at.

The second test compares a whole step, composite against per-kernel, at the dims of tests/test_gpu_ops_trace.py: loss and
every gradient bitwise, gLN and cLN.
"""
import ctypes

import pytest
import torch

from oracle import ctn_oracle as O

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import ops  # noqa: E402

DEV = "cuda:0"
NARROW = (32, 20, 16, 32, 3, 4, 2, 2)           # tests/test_gpu_ops_trace.py
WIDE = (64, 20, 64, 128, 3, 3, 2, 2)
SHAPES = [(64, 64), (128, 64), (96, 160)]       # (R, Cn) of the H-row operand = (H, B)
NBLOCKS = {1: (1, 1), 2: (2, 1), 3: (3, 1), 33: (3, 11)}      # nblocks -> (X, R); dilations stay <= 4


def _align256(n):
    return (n + 255) // 256 * 256


def _slot(B, H):
    lib = ctn.lib
    return _align256(max(H * B * 4, lib.ctn_split_b3_bytes(H, B), lib.ctn_split_b3_bytes(B, H), lib.ctn_split_h3_bytes(H, B),
                         lib.ctn_split_h3_bytes(B, H)))


def _split_one(W, R, Cn, k_major):
    """ctn_split_h3_batch of one matrix -> its bytes without the unused tail."""
    nbytes = ctn.lib.ctn_split_h3_bytes(R, Cn)
    dst = torch.zeros((nbytes,), dtype=torch.uint8, device=DEV)
    ctn.lib.call("ctn_split_h3_batch", (ctypes.c_void_p * 1)(W.data_ptr()), (ctypes.c_void_p * 1)(dst.data_ptr()), 1, R, Cn, k_major,
                 ops._stream())
    return dst[:nbytes - 12]


def _absmax_one(v):
    out = torch.zeros((1,), dtype=torch.int32, device=DEV)
    ctn.lib.call("ctn_absmax_batch", (ctypes.c_void_p * 1)(v.data_ptr()), (ctypes.c_void_p * 1)(out.data_ptr()), 1, v.numel(), ops._stream())
    return out


@pytest.fixture()
def h3():
    saved = ops.gemm_arith()
    ops.set_gemm_arith("h3")
    ops._ws_cache.clear()
    yield
    ops.set_gemm_arith(saved)
    ops._ws_cache.clear()


@pytest.mark.parametrize("nblocks", sorted(NBLOCKS))
@pytest.mark.parametrize("H,B", SHAPES)
def test_prepared_operands_equal_the_per_kernel_calls(h3, H, B, nblocks):
    X, R = NBLOCKS[nblocks]
    torch.manual_seed(100 * H + B + nblocks)
    m = ctn.ConvTasNet(64, 20, B, H, 3, X, R, 2, norm_type="gLN", causal=False).to(DEV)
    blks = [blk for rep in m.separator.network[2] for blk in rep]
    params = [[p for p in blk.fused_params()] for blk in blks]
    assert len(params) == nblocks and all(len(p) == ops.NPARAM for p in params)
    with torch.no_grad():
        for i, p in enumerate(params):          # the norm parameters start as ones and zeros: give every block its own
            p[6].copy_(torch.randn_like(p[6]) * (1 + i))
            p[7].copy_(torch.randn_like(p[7]) * 0.1 * (1 + i))
        params[0][0].zero_()
        params[-1][8].view(-1)[5 * H + 3] = 1e30
    w1 = [p[0].view(H, B) for p in params]
    w2 = [p[8].view(B, H) for p in params]
    mix, lens, src = (t.to(DEV) for t in O.synth_batch(7, 2, 804))
    M, K = 2, (804 - 20) // 10 + 1
    Kp = ops.padded_frames(K)
    ctn.cal_loss(src, m(mix), lens)[0].backward()
    ops.join_side_stream()
    torch.cuda.synchronize()
    slot = _slot(B, H)
    gb_bytes = _align256(nblocks * 2 * 4)
    fwd = ops._ws_cache[(torch.device(DEV), "tcn_fwd")]
    bwd = ops._ws_cache[(torch.device(DEV), "tcn_bwd")]
    f_total = ctn.lib.ctn_tcn_gln_fwd_workspace(M, B, H, Kp, nblocks)
    b_total = ctn.lib.ctn_tcn_gln_bwd_workspace(M, B, H, Kp, 3, nblocks)
    assert fwd.numel() >= f_total and bwd.numel() >= b_total
    f_gb = f_total - gb_bytes
    b_gb = b_total - _align256(nblocks * 2 * M * ops.AMAX_SLOTS * 4) - gb_bytes
    for name, ws, gb_off, k_major in (("forward", fwd, f_gb, 0), ("backward", bwd, b_gb, 1)):
        reg = gb_off - nblocks * 2 * slot
        assert reg >= 0
        for i in range(nblocks):
            # slot 0: H rows (fwd w1 as stored, bwd w2 transposed); slot 1: B rows (fwd w2, bwd w1 transposed)
            ops_h, ops_b = (w1[i], w2[i]) if k_major == 0 else (w2[i], w1[i])
            for half, (W, Rr, Cn) in enumerate(((ops_h, H, B), (ops_b, B, H))):
                want = _split_one(W, Rr, Cn, k_major)
                o = reg + (2 * i + half) * slot
                got = ws[o:o + want.numel()]
                assert torch.equal(got, want), "%s: block %d operand %d differs from ctn_split_h3_batch" % (name, i, half)
                word = want[-4:].cpu().numpy().view("uint32")[0]
                assert word == W.detach().abs().max().view(torch.int32).item(), (name, i, half)
            for j, v in enumerate((params[i][6], params[i][7])):
                o = gb_off + (2 * i + j) * 4
                assert torch.equal(ws[o:o + 4].view(torch.int32), _absmax_one(v)), "%s: gb[%d][%d]" % (name, i, j)
    # the two special weights went through: maximum 0 and 1e30 behind their pieces
    assert _split_one(w1[0], H, B, 0)[-4:].cpu().numpy().view("uint32")[0] == 0
    assert _split_one(w2[-1], B, H, 0)[-4:].cpu().numpy().view("float32")[0] == torch.tensor(1e30).float().item()


def _step(dims, norm_type, causal, composite, mp):
    mp.setattr(ops, "_COMPOSITE", composite)
    torch.manual_seed(3)
    m = ctn.ConvTasNet(*dims, norm_type=norm_type, causal=causal).to(DEV)
    mix, lens, src = (t.to(DEV) for t in O.synth_batch(5, 3, 4007))
    loss = ctn.cal_loss(src, m(mix), lens)[0]
    loss.backward()
    ops.join_side_stream()
    torch.cuda.synchronize()
    return [loss.detach().cpu()] + [p.grad.cpu() for p in m.parameters()], [k for k, _ in m.named_parameters()]


@pytest.mark.parametrize("norm_type,causal", [("gLN", False), ("cLN", True)])
@pytest.mark.parametrize("dims", [NARROW, WIDE], ids=["narrow", "wide"])
def test_composite_step_equals_the_per_kernel_step(h3, dims, norm_type, causal, monkeypatch):
    a, names = _step(dims, norm_type, causal, True, monkeypatch)
    b, _ = _step(dims, norm_type, causal, False, monkeypatch)
    assert float(a[0]) == float(b[0]) and bool(torch.isfinite(a[0]))
    for k, x, y in zip(["loss"] + names, a, b):
        assert torch.equal(x, y), "%s differs between the composite and the per-kernel step" % k
