"""GPU: ctn_sisnr_pit_fwd / _bwd with the moment sums of the PIT kernel spread over lanes (csrc/ctn_loss.hip).

sisnr_pit_kernel puts one (utterance, moment) pair on every lane, PIT_UB = 32 utterances per pass, loads each pair's chunk
partials eight at a time and adds them in chunk order; thread b % 256 then does utterance b's algebra.  The cases take every
path of that: B = 1, 3 (part of a pass) and 65 (two full passes and one utterance of a third), C = 2 (8 moments) and 3 (21 moments:
pairs straddle waves), nchunk = 1 (tail loop only), 2, 7 (tail only), 17 (two batches of eight and a tail).  Lengths are ragged,
with one utterance of length T and one of length 1 (nothing is left after centring: every permutation ties, index 0 wins).

Against fp64 (the oracle on .double() inputs, as tests/loss_oracle.py: reference() takes it) under the limits of
tests/test_gpu_loss.py: snr_out, max_snr, loss within 1e-4; the permutation index equal; d_est per utterance within
max(8 * e_model, 4e-6), e_model being the error of tests/loss_oracle.py: sisnr_pit_model on the same inputs.

Bitwise against a torch restatement of what the lanes add.  The chunk partials are read back from the workspace
([B][nchunk][4C + C*C] doubles) and added in chunk order on the host in fp64; from these sums the restatement takes the operations
that IEEE rounds exactly -- sum, division, conversion to fp32 -- so that it can ask for equal bits: the means coef[b,i,2] =
fp32(sum_e_i / n) and coef[b,i,3] = fp32(sum_s_j / n), j = jsel[b,i].  The rest of the algebra multiplies and adds in fp64, which
the device compiler may contract, and takes a device log10: there the restatement is held to 1e-4 dB instead.  The batch mean is
restated bitwise from max_snr: per-thread sums over b = t, t + 256, ..., the xor butterfly of a wave, the four waves in order.
That the order matters to these inputs is asserted too: for nchunk > 2 the partials added in reverse chunk order give at least one
different moment (with two chunks a + b = b + a).
"""
import numpy as np
import pytest
import torch

import loss_oracle as LO
from oracle import ctn_oracle as O

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import ops  # noqa: E402

DEV = "cuda:0"
FACTOR, FLOOR = 8.0, 4e-6           # tests/test_gpu_loss.py
T_OF_NCHUNK = {1: 1500, 2: 2049, 7: 12300, 17: 32771}
CASES = [(Bn, C, nch) for Bn in (1, 3, 65) for C in (2, 3) for nch in (1, 2, 7, 17)]


def _lengths(Bn, T):
    if Bn == 1:
        return (T - 37,)
    return (T, 1) + tuple(64 + (977 * k) % (T - 64) for k in range(Bn - 2))


def _fwd(src, est, lengths):
    Bn, C, T = src.shape
    p32, _ = ops._perms(C, src.device)
    o = dict(max_snr=torch.full((Bn,), float("nan"), device=DEV), idx=torch.full((Bn,), -1, dtype=torch.int64, device=DEV),
             loss=torch.full((1,), float("nan"), device=DEV), coef=torch.full((Bn, C, 4), float("nan"), device=DEV),
             jsel=torch.full((Bn, C), -1, dtype=torch.int32, device=DEV), snr=torch.full((Bn, C, C), float("nan"), device=DEV))
    nbytes = ctn.lib.ctn_sisnr_workspace(Bn, C, T)
    ws = torch.zeros((nbytes,), dtype=torch.uint8, device=DEV)
    ctn.lib.call("ctn_sisnr_pit_fwd", ops._p(src), ops._p(est), ops._p(lengths), ops._p(p32), p32.shape[0], Bn, C, T,
                 ops._p(o["max_snr"]), ops._p(o["idx"]), ops._p(o["loss"]), ops._p(o["snr"]), ops._p(o["coef"]), ops._p(o["jsel"]),
                 ops._p(ws), nbytes, ops._stream())
    torch.cuda.synchronize()
    o["partial"] = ws.cpu().numpy().view(np.float64).reshape(Bn, ctn.lib.ctn_sisnr_chunks(T), 4 * C + C * C)
    return o


def _block_sum_256(local):
    """block_sum<double, 256> of csrc/ctn_common.h on a [256] fp64 array: xor butterfly per wave, then the waves in order."""
    v = local.reshape(4, 64).copy()
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ o]
    return ((v[0, 0] + v[1, 0]) + v[2, 0]) + v[3, 0]


@pytest.mark.parametrize("Bn,C,nchunk", CASES)
def test_lane_sums_vs_fp64_and_bitwise_restatement(Bn, C, nchunk):
    T = T_OF_NCHUNK[nchunk]
    assert ctn.lib.ctn_sisnr_chunks(T) == nchunk
    lens = _lengths(Bn, T)
    src, est, lengths = LO.make_inputs(Bn, C, T, lens, seed=9000 + 100 * Bn + 10 * C + nchunk)
    # ---- fp64 oracle with autograd
    e64 = est.double().requires_grad_(True)
    loss, max_snr, _, _ = O.cal_loss(src.double(), e64, lengths)
    snr, _ = O.pairwise_si_snr(src.double(), e64, lengths)
    _, perms, idx, _ = O.si_snr_pit(src.double(), e64, lengths)
    wgt = LO.g_max_weight(Bn)
    gref, = torch.autograd.grad(LO.G_LOSS * loss + (max_snr.view(-1) * wgt.double()).sum(), e64)
    snr, max_snr = snr.detach(), max_snr.detach().view(-1)
    score = torch.stack([snr[:, torch.arange(C), p].sum(1) for p in perms], dim=1) / C
    top = score.sort(dim=1, descending=True).values
    margin = top[:, 0] - top[:, 1]
    for b in range(Bn):                         # conditions on the inputs, from the reference alone
        assert (float(margin[b]) == 0.0 and int(idx[b]) == 0) if lens[b] == 1 else float(margin[b]) > 0.05, (b, lens[b], float(margin[b]))

    src_d, est_d, len_d = src.to(DEV), est.to(DEV), lengths.to(DEV)
    o = _fwd(src_d, est_d, len_d)
    d_snr = float((o["snr"].double().cpu() - snr).abs().max())
    d_max = float((o["max_snr"].double().cpu() - max_snr).abs().max())
    d_loss = abs(float(o["loss"]) - float(loss))
    print("B%d C%d nchunk%d: |d snr_out| %.2e dB, |d max_snr| %.2e dB, |d loss| %.2e" % (Bn, C, nchunk, d_snr, d_max, d_loss))
    assert bool(torch.isfinite(o["snr"]).all())
    assert d_snr < 1e-4 and d_max < 1e-4 and d_loss < 1e-4
    assert torch.equal(o["idx"].cpu(), idx)
    jsel = o["jsel"].cpu()
    assert torch.equal(jsel.long(), perms[idx])

    # ---- backward
    d = torch.full_like(src_d, float("nan"))
    g_loss_d, wgt_d = torch.tensor([LO.G_LOSS], device=DEV), wgt.to(DEV)        # (held until the kernel has run)
    ctn.lib.call("ctn_sisnr_pit_bwd", ops._p(src_d), ops._p(est_d), ops._p(len_d), ops._p(o["coef"]), ops._p(o["jsel"]),
                 ops._p(g_loss_d), ops._p(wgt_d), Bn, C, T, ops._p(d), ops._stream())
    torch.cuda.synchronize()
    d = d.cpu()
    keep = torch.arange(T).view(1, 1, T) < lengths.view(-1, 1, 1)
    assert bool(torch.isfinite(d).all())
    assert float(d[(~keep).expand_as(d)].abs().sum()) == 0.0
    m = LO.sisnr_pit_model(src.numpy(), est.numpy(), lengths.tolist(), g_loss=LO.G_LOSS, g_max=wgt.numpy())
    e_model = LO.rel_err_per_utt(torch.from_numpy(m["d_est"]), gref, lengths)
    e_gpu = LO.rel_err_per_utt(d, gref, lengths)
    print("B%d C%d nchunk%d: e_gpu %.2e, e_model %.2e" % (Bn, C, nchunk, max(e_gpu), max(e_model)))
    for b in range(Bn):
        assert e_gpu[b] <= max(FACTOR * e_model[b], FLOOR), (b, e_gpu[b], e_model[b])

    # ---- bitwise: chunk partials added in chunk order, then only exactly rounded operations
    part = o["partial"]
    assert part.shape[1] == nchunk
    mo = np.zeros((Bn, part.shape[2]), np.float64)
    for ch in range(nchunk):
        mo = mo + part[:, ch, :]
    n = lengths.clamp(max=T).double().numpy()[:, None]
    ms, me = mo[:, 0:C] / n, mo[:, C:2 * C] / n
    coef = o["coef"].cpu().numpy()
    assert coef[:, :, 2].tobytes() == me.astype(np.float32).tobytes()
    assert coef[:, :, 3].tobytes() == np.take_along_axis(ms, jsel.numpy().astype(np.int64), axis=1).astype(np.float32).tobytes()
    if nchunk > 1 and Bn > 1:                   # the order matters to these inputs: the reversed sum moves at least one bit
        rev = np.zeros_like(mo)
        for ch in reversed(range(nchunk)):
            rev = rev + part[:, ch, :]
        print("moments that differ between chunk order and its reverse: %d of %d" % (int((rev != mo).sum()), mo.size))
        if nchunk > 2:                          # (two chunks: a + b = b + a) these inputs tell the two orders apart
            assert bool((rev != mo).any())
    # the rest of the algebra from the same sums, fp64 on the host: the fp32 outputs within 1e-4 dB
    En = np.maximum(mo[:, 2 * C:3 * C] - n * ms * ms, 0.0)
    Ee = np.maximum(mo[:, 3 * C:4 * C] - n * me * me, 0.0)
    dot = mo[:, 4 * C:].reshape(Bn, C, C) - n[:, :, None] * me[:, :, None] * ms[:, None, :]
    Enp = En[:, None, :] + LO.EPS
    P = dot * dot * En[:, None, :] / (Enp * Enp)
    Nz = np.maximum(Ee[:, :, None] - 2.0 * dot * dot / Enp + P, 0.0)
    sn = 10.0 * np.log10(P / (Nz + LO.EPS) + LO.EPS)
    assert float(np.abs(o["snr"].cpu().numpy().astype(np.float64) - sn).max()) < 1e-4
    # the batch mean in block_sum order, from the kernel's own max_snr
    local = np.zeros(256, np.float64)
    mx = o["max_snr"].cpu().numpy()
    for b in range(Bn):
        local[b % 256] = local[b % 256] + np.float64(mx[b])
    want = np.float32(0.0 - _block_sum_256(local) / np.float64(Bn))
    assert o["loss"].cpu().numpy().tobytes() == np.array([want], np.float32).tobytes()
