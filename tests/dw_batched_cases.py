"""What tests/test_gpu_depthwise_batched.py and tests/test_dw_batched_oracle_cpu.py share: the cases at which a batched or
pipelined load of dw_fwd_kernel / dw_bwd_kernel / gln_prelu_bwd_kernel (csrc/ctn_dw.hip) can go wrong, the guard-row layout
of the operands, a model of a kernel that reads past its row, and the fp64 definition of ctn_gln_prelu_bwd.

The kernels fill a segment's LDS image in batches of 256-frame chunks (one float4 per lane), all loads of a batch before the
first use, and the forward kernel issues the next segment's first batch before the current segment's taps.  A load that is
issued early no longer sits behind the branch that decides whether its frame exists, so what can go wrong is a load of a frame
left of 0 or right of Kp (the neighbouring row in memory), of a dead wave's row, of the segment after the last, or a register of
a batch that is used for the wrong chunk.

Frame counts per configuration, from the segment length `seg` of the direction that the form runs (dw_oracle.plan):
    two_seg_1    2 seg + 1          a third segment whose batch holds one valid frame               Kp - K = 3
    three_seg    3 seg + 67         three seams and a ragged float4 tail                            Kp - K = 1
    part1..3     seg + 256 j + 3    the second segment's batch has j whole chunks and a ragged one  Kp - K = 1
    full4        seg + 256 + 4      the last float4 of a partial batch is full                      Kp - K = 0
Kp is K rounded up to 4, the least that the entry points take: with Kp = K the frame right of the last one is the next row's
first.  Configurations (dw_oracle.CONFIGS): A, B backward patch S (scalar / float4 taps), Kc, C patch M, J, E patch L; the forward
patch is S for A, B, C and L for Kc, J, E.  M = 2, H = 6: the second workgroup of an utterance has two dead waves.
"""
import contextlib

import torch
import torch.nn.functional as F

import dw_oracle as DO

F32, F64 = torch.float32, torch.float64
TAGS = ("A", "B", "Kc", "C", "J", "E")
KINDS = ("two_seg_1", "three_seg", "part1", "part2", "part3", "full4")
GUARDS = {"nan": float("nan"), "big": 1e30}


def frames(kind, seg):
    return {"two_seg_1": 2 * seg + 1, "three_seg": 3 * seg + 67, "part1": seg + 259, "part2": seg + 515, "part3": seg + 771,
            "full4": seg + 260}[kind]


def kp_of(K):
    return (K + 3) // 4 * 4


def case_Ks(tag, kind):
    """-> (K of the forward forms, K of the backward forms)."""
    p = DO.plan(*DO.CONFIGS[tag])
    return frames(kind, p.fwd_seg), frames(kind, p.bwd_seg)


# ---- guard rows ---------------------------------------------------------------------------------------------------------------
def guarded(t, Kp, fill, dtype=F32):
    """Host tensor [..., K] -> (buffer [rows + 2, Kp], view [..., Kp] of its rows 1..rows): the rows as the kernels read them
    (zero pad frames up to Kp) between two guard rows that hold `fill` in every frame."""
    K = t.shape[-1]
    rows = t.reshape(-1, K).to(dtype)
    buf = torch.full((rows.shape[0] + 2, Kp), fill, dtype=dtype)
    buf[1:-1] = 0
    buf[1:-1, :K] = rows
    return buf, buf[1:-1].view(*t.shape[:-1], Kp)


# ---- a kernel that reads past its row --------------------------------------------------------------------------------------------
@contextlib.contextmanager
def reads_neighbour_rows(Kp, guard, side="both"):
    """Inside, the oracle's taps read memory instead of zeros outside [0, K): frame k + off of a row is the float at that
    address in the guarded [M H + 2, Kp] buffer -- the previous row's last frames left of frame 0, the row's own pad frames and
    then the next row's first frames right of K, the guard value `guard` before the first and behind the last row.
    side = "left" / "right": only the taps that reach left of frame 0 / right of frame K - 1 do so."""
    orig = DO._shift

    def shift(x, off):
        K = x.shape[-1]
        if abs(off) >= Kp or off == 0 or (side == "left" and off > 0) or (side == "right" and off < 0):
            return orig(x, off)         # (further than one row away: keep the zeros; no configuration here gets that far)
        flat = F.pad(x.reshape(-1, K), (0, Kp - K))
        g = torch.full((1, Kp), guard, dtype=x.dtype)
        flat = torch.cat([g, flat, g], 0).reshape(-1)
        n = x.reshape(-1, K).shape[0]
        idx = (torch.arange(1, n + 1)[:, None] * Kp + torch.arange(K)[None, :] + off).reshape(-1)
        return flat[idx].reshape(x.shape)

    DO._shift = shift
    try:
        yield
    finally:
        DO._shift = orig


# ---- ctn_gln_prelu_bwd ------------------------------------------------------------------------------------------------------------
GLN_KS = (1, 255, 257, 1023, 1027, 4 * 1024 + 3)          # before, at and after one batch of four 256-frame chunks


def gln_inputs(K, seed=0, M=DO.M_TEST, H=DO.H_TEST):
    """y, dN [M,H,K], gamma [H], alpha, (mean, rstd) [M], sums_part [M,3,2]: fp64 tensors that hold fp32 values (the fp64 partial
    sums stay fp64), the statistics and sums computed in fp64 from their definitions as the stack would hand them on."""
    gen = torch.Generator().manual_seed(4000 + seed + K)
    y = DO.r32(1.5 * torch.randn(M, H, K, generator=gen, dtype=F64) + 0.2)
    y[1:] = DO.r32(y[1:] * 0.05)
    g = DO.r32(1.0 + 0.3 * torch.randn(H, generator=gen, dtype=F64))
    dN = DO.r32(torch.randn(M, H, K, generator=gen, dtype=F64) + y)      # leans on y: dalpha is no remainder of a cancellation
    al = DO.ALPHA1
    ms = tuple(DO.r32(v) for v in DO.gln_stats(DO.row_sums(DO.prelu(y, al)), H * K))
    xh = (DO.prelu(y, al) - DO._utt(ms[0])) * DO._utt(ms[1])
    t = DO._ch(g) * dN
    rows = torch.stack([t.sum(2), (t * xh).sum(2)], 2)                   # [M,H,2]
    return dict(y=y, dN=dN, g=g, al=al, ms=ms, sums=DO.parts3(rows), K=K, M=M, H=H)


def gln_prelu_bwd(i, dtype=F64):
    """dY = rstd (g dN - S1/n - xh S2/n) prelu'(y), xh = (prelu(y) - mean) rstd; dalpha partial per row = sum_{y<0} da y."""
    y, dN, g = (v.to(dtype) for v in (i["y"], i["dN"], i["g"]))
    mean, rstd = (v.to(dtype) for v in i["ms"])
    n = i["H"] * i["K"]
    c = (i["sums"].double().sum(1) / n).to(dtype)                        # (fp64 sums divided in fp64, the quotient rounded)
    xh = (DO.prelu(y, i["al"]) - DO._utt(mean)) * DO._utt(rstd)
    da = DO._utt(rstd) * (DO._ch(g) * dN - DO._utt(c[:, 0]) - xh * DO._utt(c[:, 1]))
    return {"dY": da * DO.dprelu(y, i["al"]), "dalpha_part": torch.where(y < 0, da * y, torch.zeros_like(y)).sum(2)}


def reach(tag, output, side):
    """How many frames past the row's end the taps behind `output` read on `side`: the x image (Z, dD) is read at
    k + j dil - pad_left, the dd image (the backward forms' tensor output) at k - j dil + pad_left."""
    p = DO.plan(*DO.CONFIGS[tag])
    x_image = output in ("Z", "dD")
    return p.padl if (side == "left") == x_image else p.halo - p.padl
