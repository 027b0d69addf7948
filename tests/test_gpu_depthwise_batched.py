"""The batched and early loads of dw_fwd_kernel, dw_bwd_kernel and gln_prelu_bwd_kernel (csrc/ctn_dw.hip) through the C ABI
against tests/dw_oracle.py in fp64, at the frame counts of tests/dw_batched_cases.py and between guard rows.

Every tensor and per-frame operand is rows 1..n of a buffer with one more row in front and one behind.  The guard rows hold NaN
in one variant, so a halo or an early load that reads a neighbour's data turns the result NaN, and 1e30 in the other, so a
leak cannot hide behind a `valid ? ... : 0` select either.  Kp is K rounded up to 4: at Kp = K the float right of a row's last
frame is the next row's first.  Per case and form (test_gpu_depthwise.check_form): nothing is left NaN in outputs that were
pre-filled with NaN, frames K..Kp are exactly 0, a second call gives the same bits, the tracked maximum is bitwise max |dY1[m]|,
and every output is within the project's limits of the fp64 oracle, as ceilings:
    3e-6 plain forms, 2e-5 fused tensors and sums, 1e-4 dalpha1 / dalpha2.
tests/test_dw_batched_oracle_cpu.py shows on these inputs that fp32 arithmetic stays 4x inside each and that a model which reads
the neighbouring row misses by 10x or more.

Largest figure per kind over the 36 guard-row cases (576 form checks), first MI355X run: plain Z / dY 1.0e-07 / 9.6e-08 (3e-6);
fused Z 1.9e-07, dN1 / dY1 5.6e-07, dD 5.9e-07, sums1_part 1.3e-06, dgamma / dbeta at most 5.6e-07 (2e-5); dalpha1 2.3e-06,
dalpha2 5.2e-07 (1e-4).

ctn_gln_prelu_bwd against its fp64 definition: K before, at and after one batch of four chunks, Kp = K rounded up to 4 and one
float4 more, dY in place (as the stack calls it) and out of place; dY within 2e-5, the dalpha partials within 1e-4, the tracked
maximum bitwise max |dY[m]|.  Largest over the 24 cases: dY 1.8e-07, dalpha partials 2.0e-07.
"""
import pytest
import torch

import dw_batched_cases as BC
import dw_oracle as DO
import test_gpu_depthwise as TG

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import ops  # noqa: E402

DEV = TG.DEV
F32, F64 = torch.float32, torch.float64


@pytest.fixture(autouse=True)
def _own_lines():
    print()
    yield


class GuardedCase:
    """Device buffers of one dw_oracle.make_inputs() case (the attributes of test_gpu_depthwise.Case), every tensor and
    per-frame operand between two guard rows."""

    def __init__(self, i, fill):
        self.i, self.K, self.Kp = i, i.K, BC.kp_of(i.K)
        Kp = self.Kp
        self.dims = (i.M, i.H, i.K, Kp, i.P, i.dil, int(i.causal))
        self.keep = []

        def g(t):
            buf, _ = BC.guarded(t, Kp, fill)
            buf = buf.to(DEV)
            self.keep.append(buf)
            return buf[1:-1].view(*t.shape[:-1], Kp)

        self.h1, self.dN2, self.dN2_c = g(i.h1), g(i.dN2), g(i.dN2_c)
        self.Dz_g, self.Dz_c, self.X1_c = g(i.Dz_g), g(i.Dz_c), g(i.X1_c)
        self.mean1, self.rstd1, self.fc = g(i.st1[0]), g(i.st1[1]), g(i.fc)                  # [M,Kp], [M,Kp], [M,4,Kp]
        self.D, self.g1, self.b1, self.g2 = TG.dev(i.D), TG.dev(i.g1), TG.dev(i.b1), TG.dev(i.g2)
        self.a1, self.a2 = TG.scalar(i.a1), TG.scalar(i.a2)
        self.ms1, self.ms2 = TG.dev(torch.stack(i.ms1, 1)), TG.dev(torch.stack(i.ms2, 1))
        self.part1 = TG.dev(DO.parts3(i.part1), dtype=F64)
        self.sums2 = TG.dev(DO.parts3(i.rows8[..., :2]), dtype=F64)
        self.sums8 = TG.dev(DO.parts3(i.rows8), dtype=F64)

    def guards_intact(self):
        for buf in self.keep:
            for row in (buf[0], buf[-1]):
                ok = torch.isnan(row).all() if bool(torch.isnan(row[0])) else (row == row[0]).all()
                assert bool(ok)


CASES = [(tag, kind) for tag in BC.TAGS for kind in BC.KINDS]


@pytest.mark.parametrize("tag,kind", CASES, ids=["%s-%s" % c for c in CASES])
def test_forms_between_guard_rows(tag, kind):
    Kf, Kb = BC.case_Ks(tag, kind)
    for K, forms in ((Kf, DO.FWD_FORMS), (Kb, DO.BWD_FORMS)):
        inp = DO.make_inputs(*DO.CONFIGS[tag], K)
        for gname, fill in BC.GUARDS.items():
            c = GuardedCase(inp, fill)
            assert c.Kp - K == {"two_seg_1": 3, "full4": 0}.get(kind, 1)
            for form in forms:
                TG.check_form("%s/%s/%s" % (tag, kind, gname), form, c)
            c.guards_intact()


GLN_CASES = [(K, extra, inplace) for K in BC.GLN_KS for extra in (0, 4) for inplace in (True, False)]


@pytest.mark.parametrize("K,extra,inplace", GLN_CASES, ids=["K%d-pad%d-%s" % (k, e, "inplace" if p else "outofplace") for k, e, p in GLN_CASES])
def test_gln_prelu_bwd_batches(K, extra, inplace):
    i = BC.gln_inputs(K)
    M, H, Kp = i["M"], i["H"], BC.kp_of(K) + extra
    ref = BC.gln_prelu_bwd(i)
    g, al, ms, sums = TG.dev(i["g"]), TG.scalar(i["al"]), TG.dev(torch.stack(i["ms"], 1)), TG.dev(i["sums"], dtype=F64)
    for gname, fill in BC.GUARDS.items():
        got = []
        for _ in range(2):
            bufN, bufY = BC.guarded(i["dN"], Kp, fill)[0].to(DEV), BC.guarded(i["y"], Kp, fill)[0].to(DEV)
            dN, Y = bufN[1:-1].view(M, H, Kp), bufY[1:-1].view(M, H, Kp)
            dY = dN if inplace else TG.nan(M, H, Kp)
            dap = TG.nan(M * H)
            amax = torch.zeros((M, ops.AMAX_SLOTS), dtype=torch.int32, device=DEV)
            ctn.lib.call("ctn_gln_prelu_bwd", TG.ptr(dN), TG.ptr(Y), TG.ptr(dY), M, H, K, Kp, TG.ptr(g), TG.ptr(al), TG.ptr(ms), TG.ptr(sums), 3,
                         TG.ptr(dap), TG.ptr(amax), 0)
            torch.cuda.synchronize()
            got.append((dY.clone(), dap, amax.view(F32).amax(1)))
            for buf in (bufN, bufY):
                for row in (buf[0], buf[-1]):
                    assert bool(torch.isnan(row).all() if gname == "nan" else (row == fill).all()), "a guard row was written"
        (dY, dap, amax), again = got
        assert not bool(torch.isnan(dY).any()) and not bool(torch.isnan(dap).any()), (K, Kp, gname, "NaN left")
        assert float(dY[..., K:].abs().sum()) == 0.0, (K, Kp, gname, "pad frames")
        assert all(torch.equal(a, b) for a, b in zip(got[0], again)), (K, Kp, gname, "second call differs")
        assert torch.equal(amax, dY.abs().flatten(1).amax(1)), (K, Kp, gname, "amax_out")
        e = DO.rel_err(dY[..., :K], ref["dY"], "utt")
        ea = DO.rel_err(dap.view(M, H), ref["dalpha_part"], "all")
        print("GLNB K=%-4d Kp=%-4d %-10s %-3s dY=%.2e dalpha_part=%.2e" % (K, Kp, "inplace" if inplace else "outofplace", gname, e, ea))
        assert e < 2e-5 and ea < 1e-4, (K, Kp, gname, e, ea)
