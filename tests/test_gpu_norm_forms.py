"""Every kernel form behind ctn_cln_fwd / ctn_cln_bwd / ctn_cln_bwd_finalize (csrc/ctn_cln.hip) and ctn_bn_fwd / ctn_bn_bwd
(csrc/ctn_bn.hip) through the C ABI against tests/norm_oracle.py in fp64, at the dispatch seams, on guarded buffers.

What runs (norm_oracle.fwd_cases / bwd_cases; test_cln_oracle_cpu.py checks against a mirror of the dispatch, itself tied to the
source, that they reach what they claim):
    v4 kernels, CPT 1 / 2 / 4 / 8, at cln_fr 16 and again under ctn_tune("cln_fr", 32): Ch 3, 64, 65, 128, 129, 256, 257, 511, 512;
      K = 1, 64 (= Kp), 65 (whole workgroups of pad frames) and two of 15, 16, 17, 61, 130 per width; M = 2, and M = 3 / M = 1 once per
      direction (grids of 12 and 4 workgroups under xcd_remap)
    LEAN (Ch = 512, PReLU, no add / relu_ref) at K = 1, 61, 64, 65, 130, bitwise against the general CPT 8 form (cln_lean 0)
    register-resident and generic fallbacks through Kp % 32 != 0: (K, Kp) = (37, 40), (97, 100), (68, 68), forward also (37, 37);
      and through alignment at Kp = 64, 128: mean (forward), dY or add (backward) one float off a 16-byte boundary.
      Forward Ch 3, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025; backward Ch 3, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513
      (with cln_bwd_params_kernel on that path)
    backward options {PReLU, none} x {plain, add, add + relu_ref}: run-time branches of every kernel, two of the six per (width, frames)
      in turn, all six per kernel label
    ctn_cln_bwd_finalize alone at 28, 32, 36 and 320 partial rows; Ch = 1 and Ch = 2 known answers; exact zeros under PReLU; refusals
    BatchNorm: Ch 1, 7, 257 x K 1, 3, 64, 255, 257 x M 1, 2 x {training with running statistics, training without, eval} x {PReLU, none}

Pad frames of the inputs.  cLN: Y holds exact ZEROS in frames K..Kp -- ctn_cln_fwd computes the pad frames' statistics from what is
there (recorded here: mean == 0 exactly, rstd = 1 / sqrt(eps) to 2e-5) and the v4 backward multiplies the pad frames' xhat by a zeroed
gradient; dOut, add and relu_ref hold 1e30 there: no kernel may let them into a result.  BatchNorm: Y and dOut both hold 1e30 there
(every BatchNorm kernel selects on k < K).

Per case: outputs are pre-filled with NaN inside an allocation with 4096 sentinel elements on either side -- afterwards the
sentinels are untouched, nothing is NaN, frames K..Kp of out / dY are exactly 0; a second call gives the same bits; utterance m of
an M > 1 call is bitwise the M = 1 call on that utterance alone (out, mean, rstd, dY).

Limits, the project's existing ones as ceilings (norm_oracle.LIMIT):
    2e-5   out, mean, rstd: of max |ref| per utterance over the valid frames          (test_cln_kernels_every_width)
    5e-5   dY per utterance; dgamma, dbeta of max |ref|                                (test_cln_kernels_every_width)
    1e-5   every sum (each dgamma[c], dbeta[c], dalpha): of the sum of its terms' absolute values   (test_gpu_gemm_seams.py)
           dalpha is judged by this rule alone (its terms cancel)
    1e-5   BatchNorm out, running statistics; 2e-5 BatchNorm dY                        (test_bn_kernels_vs_torch)
tests/test_cln_oracle_cpu.py shows on these inputs that fp32 arithmetic stays 4x inside each and that eight wrong models miss them
by 10x or more.

Largest figure per kind of output over all cases of this module, first MI355X run (the `NORM MAX` lines of -s).  These figures are
a record, not new limits.
    kind                             largest    limit  at (label, direction, Ch K Kp M, misaligned pointer, PReLU, mode)
    bn dY                            1.68e-07   2e-05  bn 257 64 1 train prelu
    bn dalpha sum                    3.00e-07   1e-05  bn 1 3 2 train prelu
    bn dbeta sum                     8.22e-08   1e-05  bn 257 3 2 train prelu
    bn dgamma sum                    1.37e-07   1e-05  bn 257 1 2 eval -
    bn mr                            1.46e-07   1e-05  bn 257 3 1 train -
    bn out                           1.52e-07   1e-05  bn 1 255 1 train prelu
    bn running_mean                  4.79e-08   1e-05  bn 7 64 2 train prelu
    bn running_var                   5.99e-08   1e-05  bn 257 3 2 train -
    ch2 (|dY| - exact) / slack       1.32e-01   1e+00  64 64 False
    ch2 mean                         5.52e-08   2e-05  ch2 61 64 False
    ch2 out                          1.41e-07   2e-05  ch2 61 64 True
    ch2 rstd                         1.03e-07   2e-05  ch2 61 64 False
    dxreg dY                         6.25e-07   5e-05  dxreg/2x512 bwd 3 68 68 2 - mask
    dxreg dalpha sum                 6.56e-08   1e-05  dxreg/2x512 bwd 3 61 64 2 dY prelu mask
    dxreg dbeta                      1.03e-07   5e-05  dxreg/2x512 bwd 3 61 64 2 dY prelu mask
    dxreg dbeta sum                  7.68e-08   1e-05  dxreg/16x512 bwd 256 37 40 2 prelu plain
    dxreg dgamma                     3.58e-07   5e-05  dxreg/2x512 bwd 3 128 128 2 dY prelu add
    dxreg dgamma sum                 6.77e-08   1e-05  dxreg/16x1024 bwd 512 37 40 2 - plain
    finalize sum                     8.85e-08   1e-05  36 64
    generic dY                       1.15e-07   5e-05  generic bwd 513 97 100 2 prelu add
    generic dalpha sum               5.80e-09   1e-05  generic bwd 513 68 68 2 prelu mask
    generic dbeta                    1.02e-07   5e-05  generic bwd 513 97 100 2 prelu add
    generic dbeta sum                6.56e-08   1e-05  generic bwd 513 37 40 2 prelu plain
    generic dgamma                   1.41e-07   5e-05  generic bwd 513 37 40 2 - add
    generic dgamma sum               6.83e-08   1e-05  generic bwd 513 37 40 2 - add
    generic mean                     3.98e-07   2e-05  generic fwd 1025 97 100 2 prelu
    generic out                      2.22e-07   2e-05  generic fwd 1025 37 40 2 -
    generic rstd                     2.13e-07   2e-05  generic fwd 1025 68 68 2 -
    lean dY                          1.24e-07   5e-05  lean bwd 512 1 64 2 prelu plain
    lean dalpha sum                  5.02e-09   1e-05  lean bwd 512 1 64 2 prelu plain
    lean dbeta                       1.11e-07   5e-05  lean bwd 512 61 64 2 prelu plain
    lean dbeta sum                   7.46e-08   1e-05  lean bwd 512 61 64 2 prelu plain
    lean dgamma                      1.39e-07   5e-05  lean bwd 512 64 64 2 prelu plain
    lean dgamma sum                  1.28e-07   1e-05  lean bwd 512 1 64 2 prelu plain
    reg mean                         3.03e-07   2e-05  reg/CPT32 fwd 513 97 100 2 prelu
    reg out                          3.58e-07   2e-05  reg/CPT2 fwd 3 37 40 2 -
    reg rstd                         1.93e-07   2e-05  reg/CPT8 fwd 256 61 64 2 mean -
    v4 dY                            5.24e-07   5e-05  v4/CPT1/fr16 bwd 3 65 128 2 prelu mask
    v4 dalpha sum                    5.41e-07   1e-05  v4/CPT1/fr16 bwd 3 1 64 2 prelu plain
    v4 dbeta                         1.47e-07   5e-05  v4/CPT4/fr32 bwd 256 65 128 2 prelu plain
    v4 dbeta sum                     9.19e-08   1e-05  v4/CPT8/fr16 bwd 511 15 64 2 prelu plain
    v4 dgamma                        1.49e-07   5e-05  v4/CPT1/fr32 bwd 64 64 64 2 prelu plain
    v4 dgamma sum                    1.67e-07   1e-05  v4/CPT2/fr16 bwd 128 1 64 2 - add
    v4 mean                          2.09e-07   2e-05  v4/CPT8/fr32 fwd 257 17 64 2 -
    v4 out                           3.06e-07   2e-05  v4/CPT1/fr16 fwd 3 15 64 2 -
    v4 rstd                          1.47e-07   2e-05  v4/CPT2/fr32 fwd 128 17 64 2 -
    BatchNorm rstd at n = M K = 1 (no limit applies: see test_batchnorm_every_form): 2.0e-2 off 1 / sqrt(eps) at Ch = 257
"""
import math

import numpy as np
import pytest
import torch

import norm_oracle as NO

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import ops  # noqa: E402

DEV = "cuda:0"
NAN = float("nan")
F32, F64, I32 = torch.float32, torch.float64, torch.int32
GUARD, SENT = 4096, -7777.0
WORST = {}
_REF = {}


@pytest.fixture(scope="module", autouse=True)
def _figures():
    yield
    print()
    for kind, (e, lim, where) in sorted(WORST.items()):
        print("NORM MAX %-22s %.2e  limit %.0e  at %s" % (kind, e, lim, where))


@pytest.fixture(autouse=True)
def _defaults():
    yield
    _REF.clear()
    ctn.lib.call("ctn_tune", b"cln_fr", NO.DEFAULT_FR)
    ctn.lib.call("ctn_tune", b"cln_lean", NO.DEFAULT_LEAN)


class Guarded:
    """An output buffer pre-filled with NaN (integers: 0) between two runs of GUARD sentinel elements of the same allocation;
    off = 1: the buffer starts one element off a 16-byte boundary."""

    def __init__(self, *shape, dtype=F32, off=0):
        self.n = math.prod(shape)
        self.flat = torch.full((self.n + off + 2 * GUARD,), int(SENT) if dtype == I32 else SENT, dtype=dtype, device=DEV)
        self.t = self.flat[GUARD + off:GUARD + off + self.n].view(shape)
        self.t.fill_(0 if dtype == I32 else NAN)
        self.off = off
        assert (self.t.data_ptr() % 16 == 0) == (off == 0)

    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        a = GUARD + self.off
        return bool((self.flat[:a] == SENT).all()) and bool((self.flat[a + self.n:] == SENT).all())

    def untouched(self):
        return self.intact() and bool(torch.isnan(self.t).all())


def dev(t, off=0, dtype=F32):
    """t on the device; off = 1: one element off a 16-byte boundary."""
    t = t.to(dtype).contiguous()
    buf = torch.empty(t.numel() + 8, dtype=dtype, device=DEV)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert (v.data_ptr() % 16 == 0) == (off == 0)
    return v


def ptr(t):
    return 0 if t is None else t.data_ptr()


def note(kind, e, lim, where):
    if e > WORST.get(kind, (-1.0,))[0]:
        WORST[kind] = (e, lim, where)


def cpu(d):
    return {k: (v.t if isinstance(v, Guarded) else v).detach().cpu() for k, v in d.items() if not k.startswith("_")}


class Case:
    """Device buffers of one norm_oracle.make_inputs() case."""

    def __init__(self, i, mis=None):
        self.i, self.mis = i, mis
        self.Y, self.dOut, self.relu_ref = dev(i.Y), dev(i.dOut), dev(i.relu_ref)
        self.add = dev(i.add, off=int(mis == "add"))
        self.gamma, self.beta, self.alpha = dev(i.gamma), dev(i.beta), dev(torch.tensor([i.alpha]))
        self.stats = {k: (dev(v[0]), dev(v[1])) for k, v in i.stats.items()}
        self._solo = {}

    def solo(self, m):
        if m not in self._solo:
            self._solo[m] = Case(NO.solo(self.i, m), self.mis)
        return self._solo[m]


def cln_fwd(c, pre, amax=False):
    i = c.i
    out = {"out": Guarded(i.M, i.Ch, i.Kp), "mean": Guarded(i.M, i.Kp, off=int(c.mis == "mean")), "rstd": Guarded(i.M, i.Kp)}
    if amax:
        out["_amax"] = Guarded(i.M, ops.AMAX_SLOTS, dtype=I32)
    ctn.lib.call("ctn_cln_fwd", ptr(c.Y), out["out"].ptr(), out["mean"].ptr(), out["rstd"].ptr(), i.M, i.Ch, i.K, i.Kp, ptr(c.gamma),
                 ptr(c.beta), ptr(c.alpha) if pre else 0, out["_amax"].ptr() if amax else 0, ops._stream())
    torch.cuda.synchronize()
    return out


def cln_bwd(c, pre, mode, amax=False, inplace=False):
    """ctn_cln_bwd + ctn_cln_bwd_finalize; the partial buffers are sized by the library (after any ctn_tune("cln_fr"))."""
    i, lib = c.i, ctn.lib.load()
    rows = lib.ctn_cln_bwd_blocks(i.M, i.Kp)
    assert lib.ctn_cln_bwd_pc_floats(i.M, i.Ch, i.Kp) == 2 * rows * i.Ch
    out = {"dY": Guarded(i.M, i.Ch, i.Kp, off=int(c.mis == "dY")), "_pc": Guarded(2, rows, i.Ch), "dgamma": Guarded(i.Ch), "dbeta": Guarded(i.Ch)}
    dOut = c.dOut
    if inplace:
        out["dY"].t.copy_(c.dOut)
        dOut = out["dY"].t
    if pre:
        out["_dap"], out["dalpha"] = Guarded(rows), Guarded(1)
    if amax:
        out["_amax"] = Guarded(i.M, ops.AMAX_SLOTS, dtype=I32)
    mean, rstd = c.stats[pre]
    dap = out["_dap"].ptr() if pre else 0
    ctn.lib.call("ctn_cln_bwd", ptr(dOut), ptr(c.Y), out["dY"].ptr(), ptr(mean), ptr(rstd), i.M, i.Ch, i.K, i.Kp, ptr(c.gamma),
                 ptr(c.alpha) if pre else 0, ptr(c.add) if mode != "plain" else 0, ptr(c.relu_ref) if mode == "mask" else 0, dap,
                 out["_pc"].ptr(), out["_amax"].ptr() if amax else 0, ops._stream())
    ctn.lib.call("ctn_cln_bwd_finalize", out["_pc"].ptr(), dap, i.M, i.Ch, i.Kp, out["dgamma"].ptr(), out["dbeta"].ptr(),
                 out["dalpha"].ptr() if pre else 0, ops._stream())
    torch.cuda.synchronize()
    return out


def reference(kind, i, *key):
    k = (kind, id(i)) + key
    if k not in _REF:
        _REF[k] = (i, NO.run_fwd(i, *key) if kind == "fwd" else NO.run_bwd(i, *key))
    return _REF[k][1]


def common_checks(where, got, again, K, tensor):
    for name, g in got.items():
        assert g.intact(), (where, name, "a guard element was written")
        assert not bool(torch.isnan(g.t).any()), (where, name, "NaN left")
        assert torch.equal(g.t, again[name].t), (where, name, "second call differs")
    assert float(got[tensor].t[..., K:].abs().sum()) == 0.0, (where, "pad frames of " + tensor)


def judge(where, label, errs):
    for name, (e, lim) in errs.items():
        note("%s %s" % (label.split("/")[0], name), e, lim, where)
        assert e < lim, (where, name, e, lim)


def check_fwd(c, pre, label):
    i = c.i
    where = (label, "fwd", i.Ch, i.K, i.Kp, i.M, c.mis, "prelu" if pre else "-")
    got = cln_fwd(c, pre)
    common_checks(where, got, cln_fwd(c, pre), i.K, "out")
    # the pad frames' statistics are those of the zeros that Y holds there: mean 0, rstd 1 / sqrt(eps)
    if i.Kp > i.K:
        assert float(got["mean"].t[:, i.K:].abs().max()) == 0.0, (where, "mean of the pad frames")
        assert float((got["rstd"].t[:, i.K:].double() / NO.RSTD_PAD - 1).abs().max()) < 2e-5, (where, "rstd of the pad frames")
    if i.M > 1:
        for m in range(i.M):
            alone = cln_fwd(c.solo(m), pre)
            for name, g in alone.items():
                assert g.intact(), (where, name, "M = 1: a guard element was written")
                assert torch.equal(g.t[0], got[name].t[m]), (where, name, "utterance %d differs from the M = 1 call" % m)
    errs = NO.cln_errors(cpu(got), reference("fwd", i, pre), i.K)
    judge(where, label, errs)
    return errs


def check_bwd(c, pre, mode, label):
    i = c.i
    where = (label, "bwd", i.Ch, i.K, i.Kp, i.M, c.mis, "prelu" if pre else "-", mode)
    got = cln_bwd(c, pre, mode)
    common_checks(where, got, cln_bwd(c, pre, mode), i.K, "dY")
    if i.M > 1:
        for m in range(i.M):
            alone = cln_bwd(c.solo(m), pre, mode)
            assert all(g.intact() for g in alone.values()), (where, "M = 1: a guard element was written")
            assert torch.equal(alone["dY"].t[0], got["dY"].t[m]), (where, "dY: utterance %d differs from the M = 1 call" % m)
    errs = NO.cln_errors(cpu(got), reference("bwd", i, pre, mode), i.K)
    judge(where, label, errs)
    return errs, got


def _inputs(c):
    return NO.make_inputs(c.Ch, c.K, c.Kp, c.M, c.seed)


def run_fwd_cases(fr, only_v4):
    n = 0
    for c in NO.fwd_cases():
        label = NO.fwd_label(c, fr)
        if only_v4 and not label.startswith("v4"):
            continue
        check_fwd(Case(_inputs(c), c.mis), c.prelu, label)
        n += 1
    return n


def run_bwd_cases(fr, which):
    n = 0
    for c in NO.bwd_cases():
        label = NO.bwd_label(c, fr)
        if (label.startswith("v4") or label == "lean") != (which == "v4"):
            continue
        assert ctn.lib.load().ctn_cln_bwd_blocks(c.M, c.Kp) == NO.bwd_blocks(c.M, c.Kp, fr)
        check_bwd(Case(_inputs(c), c.mis), c.prelu, c.mode, label)
        n += 1
    return n


# ---- the case tables ---------------------------------------------------------------------------------------------------------------
def test_cln_forward_every_form():
    assert run_fwd_cases(16, False) == len(NO.fwd_cases())


@pytest.mark.parametrize("which", ["v4", "fallback"])
def test_cln_backward_every_form(which):
    assert run_bwd_cases(16, which) > 40


def test_cln_v4_forms_at_32_frames():
    """The 512-thread, 32-frame v4 kernels of both directions; the partial buffers are sized after the switch."""
    try:
        ctn.lib.call("ctn_tune", b"cln_fr", 32)
        assert ctn.lib.load().ctn_cln_bwd_blocks(2, 64) == 4
        assert run_fwd_cases(32, True) > 40 and run_bwd_cases(32, "v4") > 40
    finally:
        ctn.lib.call("ctn_tune", b"cln_fr", NO.DEFAULT_FR)
        ctn.lib.call("ctn_tune", b"cln_lean", NO.DEFAULT_LEAN)
    assert ctn.lib.load().ctn_cln_bwd_blocks(2, 64) == 8


def test_lean_is_bitwise_the_general_form():
    """cln_bwd_v4_kernel<8, 256, 16, LEAN> against the general CPT 8 form on the same input: dY, pc, dalpha_part and the tracked maximum."""
    try:
        for K in (1, 61, 64, 130):
            c = Case(NO.make_inputs(512, K, NO.padded(K)))
            assert NO.plan_bwd(512, c.i.Kp) == "lean" and NO.plan_bwd(512, c.i.Kp, lean=0) == "v4/CPT8/fr16"
            res = {}
            for lean in (1, 0):
                ctn.lib.call("ctn_tune", b"cln_lean", lean)
                errs, _ = check_bwd(c, True, "plain", "lean" if lean else "v4/CPT8/fr16")
                res[lean] = cln_bwd(c, True, "plain", amax=True)
                assert res[lean]["_amax"].intact()
            for name in ("dY", "_pc", "_dap", "_amax", "dgamma", "dbeta", "dalpha"):
                assert torch.equal(res[1][name].t, res[0][name].t), (K, name, "LEAN differs from the general form")
            assert torch.equal(res[1]["_amax"].t.view(F32).amax(1), res[1]["dY"].t.abs().flatten(1).amax(1))
    finally:
        ctn.lib.call("ctn_tune", b"cln_lean", NO.DEFAULT_LEAN)


def test_tracked_maxima_on_v4_and_fallback():
    """amax_out: the slots' maximum is bitwise max |out[m]| / max |dY[m]| -- inside the v4 kernels, and after the fallback kernels
    (a ctn_absmax_rows pass)."""
    for Ch, K, Kp, mis in ((129, 61, 64, None), (257, 130, 192, None), (129, 37, 40, None), (40, 61, 64, "add"), (513, 68, 68, None)):
        c = Case(NO.make_inputs(Ch, K, Kp), mis)
        assert NO.plan_fwd(Ch, Kp).startswith("v4") == (Kp % 32 == 0 and Ch <= 512)
        f = cln_fwd(c, True, amax=True)
        assert f["_amax"].intact() and torch.equal(f["_amax"].t.view(F32).amax(1), f["out"].t.abs().flatten(1).amax(1)), (Ch, K, Kp, "out")
        assert torch.equal(f["out"].t, cln_fwd(c, True)["out"].t)
        mode = "mask" if mis else "plain"
        assert NO.plan_bwd(Ch, Kp, mis is None, add=bool(mis), relu_ref=bool(mis)).startswith("v4") == (Kp % 32 == 0 and Ch <= 512 and not mis)
        b = cln_bwd(c, True, mode, amax=True)
        assert b["_amax"].intact() and torch.equal(b["_amax"].t.view(F32).amax(1), b["dY"].t.abs().flatten(1).amax(1)), (Ch, K, Kp, "dY")
        assert torch.equal(b["dY"].t, cln_bwd(c, True, mode)["dY"].t)


def test_dY_may_alias_dOut():
    """In place (dY = dOut) gives the bits of the out-of-place call: a v4 form, a register-resident fallback and the generic kernel."""
    for Ch, K, Kp, want in ((129, 61, 64, "v4/CPT4/fr16"), (129, 97, 100, "dxreg/16x512"), (513, 37, 40, "generic")):
        c = Case(NO.make_inputs(Ch, K, Kp))
        assert NO.plan_bwd(Ch, Kp, add=True, relu_ref=True) == want
        for pre in (True, False):
            a, b = cln_bwd(c, pre, "mask"), cln_bwd(c, pre, "mask", inplace=True)
            for name in a:
                assert b[name].intact() and torch.equal(a[name].t, b[name].t), (want, pre, name, "in place differs")


# ---- ctn_cln_bwd_finalize alone ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,Kp", NO.FINALIZE_SHAPES)
def test_finalize_alone(M, Kp):
    rows = ctn.lib.load().ctn_cln_bwd_blocks(M, Kp)
    assert rows == NO.bwd_blocks(M, Kp)
    gen = torch.Generator().manual_seed(rows)
    for Ch in NO.FINALIZE_WIDTHS:
        pc = torch.randn(2, rows, Ch, generator=gen) * torch.rand(1, rows, 1, generator=gen) * 10
        dap = torch.randn(rows, generator=gen)
        pcd, dapd = dev(pc), dev(dap)
        for with_alpha in (True, False):
            dg, db, da = Guarded(Ch), Guarded(Ch), Guarded(1)
            ctn.lib.call("ctn_cln_bwd_finalize", ptr(pcd), ptr(dapd) if with_alpha else 0, M, Ch, Kp, dg.ptr(), db.ptr(), da.ptr(), ops._stream())
            torch.cuda.synchronize()
            assert dg.intact() and db.intact() and da.intact()
            for f, g in enumerate((dg, db)):
                e = NO.sum_err(g.t.cpu(), pc[f].double().sum(0), pc[f].double().abs().sum(0))
                note("finalize sum", e, NO.LIMIT["sum"], (rows, Ch))
                assert e < NO.LIMIT["sum"], (rows, Ch, f, e)
            if with_alpha:
                e = NO.sum_err(da.t.cpu(), dap.double().sum().reshape(1), dap.double().abs().sum().reshape(1))
                note("finalize sum", e, NO.LIMIT["sum"], (rows, "dalpha"))
                assert e < NO.LIMIT["sum"], (rows, "dalpha", e)
            else:
                assert da.untouched(), "dalpha written without dalpha_part"


# ---- known answers -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,Kp", [(61, 64), (37, 40)])
def test_one_channel(K, Kp):
    """Ch = 1: out == beta exactly, rstd == 1 / sqrt(eps) as fp32 rounds it, dY == add exactly (0 without add); v4 and fallback."""
    c = Case(NO.make_inputs(1, K, Kp))
    i = c.i
    want_rstd = float(np.float32(1.0) / np.sqrt(np.float32(NO.EPS)))
    for pre in (True, False):
        f = cln_fwd(c, pre)
        assert all(g.intact() for g in f.values())
        assert bool((f["out"].t[..., :K] == float(i.beta[0])).all()) and float(f["out"].t[..., K:].abs().sum()) == 0.0
        assert bool((f["rstd"].t == want_rstd).all()), (float(f["rstd"].t[0, 0]), want_rstd)
        assert torch.equal(f["mean"].t.cpu().double(), NO.run_fwd(i, pre)["mean"])
        for mode in ("plain", "add"):
            b = cln_bwd(c, pre, mode)
            want = torch.zeros_like(i.add) if mode == "plain" else torch.where(torch.arange(Kp) < K, i.add, torch.zeros_like(i.add))
            assert torch.equal(b["dY"].t.cpu().double(), want), (K, pre, mode)
            assert float(b["dgamma"].t.abs().max()) == 0.0
            assert NO.sum_err(b["dbeta"].t.cpu(), i.dOut[..., :K].sum((0, 2)), i.dOut[..., :K].abs().sum((0, 2))) < NO.LIMIT["sum"]


@pytest.mark.parametrize("K,Kp", [(1, 64), (61, 64), (64, 64), (37, 40)])
def test_two_channels(K, Kp):
    """Ch = 2 on a well-separated input: out by the 2e-5 rule; the exact dY is about 1e-8 of gamma dOut, so |dY| is bounded by
    norm_oracle.ch2_dy_bound()'s absolute figure instead of a relative error."""
    c = Case(NO.make_ch2_inputs(K, Kp))
    i = c.i
    for pre in (True, False):
        f = cln_fwd(c, pre)
        errs = NO.cln_errors(cpu(f), NO.run_fwd(i, pre), K)
        judge(("ch2", K, Kp, pre), "ch2", errs)
        b = cln_bwd(c, pre, "plain")
        assert all(g.intact() for g in b.values())
        exact, slack = NO.ch2_dy_bound(i.dOut, *i.stats[pre], i.gamma)
        over = (b["dY"].t.cpu().double().abs().amax(1) - exact)[:, :K] / slack[:, :K]
        note("ch2 (|dY| - exact) / slack", float(over.max()), 1.0, (K, Kp, pre))
        assert float(over.max()) <= 1.0, (K, Kp, pre, float(over.max()))
        assert float(b["dY"].t[..., K:].abs().sum()) == 0.0


@pytest.mark.parametrize("Kp", [64, 40])
def test_exact_zeros_under_prelu(Kp):
    """A quarter of the input exactly 0: the kernels take slope 1 there (v >= 0); the wrong convention misses the dY limit by
    more than 10x on this input (test_cln_oracle_cpu.py::test_limits_catch_defects)."""
    c = Case(NO.make_inputs(40, Kp - 3, Kp, zeros=0.25))
    assert float((c.i.Y[..., :Kp - 3] == 0).double().mean()) > 0.2
    for mode in ("plain", "mask"):
        check_bwd(c, True, mode, NO.plan_bwd(40, Kp, add=mode == "mask", relu_ref=mode == "mask") + " zeros")
    check_fwd(c, True, NO.plan_fwd(40, Kp) + " zeros")


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    lib = ctn.lib.load()
    i = NO.make_inputs(40, 61, 64)
    c = Case(i)
    M, Ch, K, Kp = i.M, i.Ch, i.K, i.Kp
    mean, rstd = c.stats[True]
    rows = lib.ctn_cln_bwd_blocks(M, Kp)
    st = ops._stream()

    def refused(name, args, bufs, what):
        rc = getattr(lib, name)(*args)
        torch.cuda.synchronize()
        assert rc != 0, what
        msg = lib.ctn_last_error().decode()
        assert name in msg, (what, msg)
        assert all(b.untouched() for b in bufs), (what, "a refused call wrote something")

    o, mo, ro = Guarded(M, Ch, Kp), Guarded(M, Kp), Guarded(M, Kp)
    refused("ctn_cln_fwd", (ptr(c.Y), o.ptr(), mo.ptr(), ro.ptr(), M, Ch, Kp + 1, Kp, ptr(c.gamma), ptr(c.beta), ptr(c.alpha), 0, st),
            (o, mo, ro), "Kp < K (forward)")
    dY, pc, dap = Guarded(M, Ch, Kp), Guarded(2, rows, Ch), Guarded(rows)
    bufs = (dY, pc, dap)

    def bwd(dOut=c.dOut, K_=K, Kp_=Kp, alpha=c.alpha, dap_=dap.ptr(), pc_=pc.ptr()):
        return (ptr(dOut), ptr(c.Y), dY.ptr(), ptr(mean), ptr(rstd), M, Ch, K_, Kp_, ptr(c.gamma), ptr(alpha), 0, 0, dap_, pc_, 0, st)

    refused("ctn_cln_bwd", bwd(K_=Kp + 1), bufs, "Kp < K (backward)")
    refused("ctn_cln_bwd", bwd(K_=61, Kp_=62), bufs, "Kp % 4 != 0")
    refused("ctn_cln_bwd", bwd(dOut=dev(i.dOut, off=1)), bufs, "misaligned dOut")
    refused("ctn_cln_bwd", bwd(dap_=0), bufs, "alpha without dalpha_part")
    refused("ctn_cln_bwd", bwd(pc_=0), bufs, "null pc")
    ctn.lib.call("ctn_cln_bwd", *bwd())                       # and the same arguments, unbroken, are accepted
    torch.cuda.synchronize()
    assert not bool(torch.isnan(dY.t).any()) and all(b.intact() for b in bufs)


# ---- BatchNorm -----------------------------------------------------------------------------------------------------------------------
def bn_fwd(i, d, stats, pre):
    Ch, M = i.Ch, i.M
    out = {"out": Guarded(M, Ch, i.Kp), "mr": Guarded(Ch, 2), "_part": Guarded(Ch * M * 2, dtype=F64)}
    run = stats != "train_norun"
    if run:
        out["running_mean"], out["running_var"] = Guarded(Ch), Guarded(Ch)
        out["running_mean"].t.copy_(i.running[0])
        out["running_var"].t.copy_(i.running[1])
    ctn.lib.call("ctn_bn_fwd", ptr(d["Y"]), out["out"].ptr(), ptr(d["alpha"]) if pre else 0, ptr(d["gamma"]), ptr(d["beta"]),
                 out["running_mean"].ptr() if run else 0, out["running_var"].ptr() if run else 0, int(stats != "eval"), NO.BN_EPS,
                 NO.BN_MOMENTUM, M, Ch, i.K, i.Kp, out["_part"].ptr(), out["mr"].ptr(), ops._stream())
    torch.cuda.synchronize()
    if stats == "eval":
        assert out.pop("_part").untouched()
    return out


def bn_bwd(i, d, stats, pre, inplace=False):
    Ch, M = i.Ch, i.M
    out = {"dY": Guarded(M, Ch, i.Kp), "_part": Guarded(Ch * M * 2, dtype=F64), "_coef": Guarded(Ch, 2), "dgamma": Guarded(Ch), "dbeta": Guarded(Ch)}
    if pre:
        out["_dap"] = Guarded(M * Ch)
    dOut = d["dOut"]
    if inplace:
        out["dY"].t.copy_(dOut)
        dOut = out["dY"].t
    ctn.lib.call("ctn_bn_bwd", ptr(dOut), ptr(d["Y"]), out["dY"].ptr(), ptr(d["alpha"]) if pre else 0, ptr(d["gamma"]), ptr(d["mr"][(stats, pre)]),
                 int(stats != "eval"), M, Ch, i.K, i.Kp, out["_part"].ptr(), out["_coef"].ptr(), out["dgamma"].ptr(), out["dbeta"].ptr(),
                 out["_dap"].ptr() if pre else 0, ops._stream())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("Ch", NO.BN_WIDTHS)
def test_batchnorm_every_form(Ch):
    """ctn_bn_fwd / ctn_bn_bwd: training with and without running statistics, eval, with and without PReLU; n = M K = 1 included
    (var = 0, out == beta, the running variance takes var itself)."""
    for K in NO.BN_FRAMES:
        for M in NO.BN_MS:
            i = NO.make_bn_inputs(Ch, K, M)
            d = {"Y": dev(i.Y), "dOut": dev(i.dOut), "gamma": dev(i.gamma), "beta": dev(i.beta), "alpha": dev(torch.tensor([i.alpha])),
                 "mr": {k: dev(v) for k, v in i.mr.items()}}
            for stats in NO.BN_STATS:
                for pre in (True, False):
                    where = ("bn", Ch, K, M, stats, "prelu" if pre else "-")
                    f = bn_fwd(i, d, stats, pre)
                    common_checks(where, f, bn_fwd(i, d, stats, pre), K, "out")
                    ref = NO.run_bn_fwd(i, stats, pre)
                    got = cpu(f)
                    judge(where, "bn", NO.bn_errors(got, ref, K))
                    # mr: mean and rstd each against its own largest.  At n = 1 only the mean: var is 0, and bn_finalize_kernel's
                    # one-pass E[p^2] - mean^2 leaves the rounding of p^2 (up to 1.5e-6 beside eps = 1e-5: rstd 2e-2 off, measured at
                    # Ch = 257) -- the one-pass variance is a known design question outside this suite, and at n = 1 rstd multiplies
                    # p - mean = 0 in every result (out == beta and dY == 0 are asserted)
                    rows = slice(0, 1) if M * K == 1 and stats != "eval" else slice(0, 2)
                    e = NO.rel_err(got["mr"].t()[rows], ref["mr"].t()[rows], "utt")
                    note("bn mr", e, NO.LIMIT["bn_run"], where)
                    assert e < NO.LIMIT["bn_run"], (where, "mr", e)
                    if stats == "eval":
                        assert torch.equal(got["running_mean"].double(), i.running[0]) and torch.equal(got["running_var"].double(), i.running[1])
                    if M * K == 1 and stats != "eval":          # the batch statistics of one element: mean = it, var = 0
                        assert torch.equal(got["out"][0, :, 0].double(), i.beta), (where, "out == beta")
                    b = bn_bwd(i, d, stats, pre)
                    common_checks(where, b, bn_bwd(i, d, stats, pre), K, "dY")
                    gb = cpu(b)
                    if pre:
                        gb["dalpha"] = b["_dap"].t.double().sum().reshape(1).cpu()          # "sum them in order"
                    judge(where, "bn", NO.bn_errors(gb, NO.run_bn_bwd(i, stats, pre), K))
                    if M * K == 1 and stats != "eval":
                        assert float(gb["dY"].abs().max()) == 0.0, (where, "dY == 0")
                    if K == 255:
                        bi = bn_bwd(i, d, stats, pre, inplace=True)
                        assert bi["dY"].intact() and torch.equal(bi["dY"].t, b["dY"].t), (where, "in place differs")
