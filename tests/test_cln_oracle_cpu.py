"""tests/norm_oracle.py itself, on the CPU: the mirror of the cLN dispatch against csrc/ctn_cln.hip, the case tables against that
mirror (every kernel label of both entry points at cln_fr 16 and 32), the fp64 closed forms of the cLN and BatchNorm entry points
against autograd, and the limits of tests/test_gpu_norm_forms.py against what fp32 arithmetic can reach on that test's inputs and
against eight deliberately wrong models."""
import os
import re

import pytest
import torch
import torch.nn.functional as Fn

import norm_oracle as NO
from conftest import ROOT

F64, F32 = torch.float64, torch.float32
CSRC = os.path.join(ROOT, "conv-tasnet_amd", "csrc")


# ---- the mirror ----------------------------------------------------------------------------------------------------------------
def test_mirror_matches_the_source():
    src = open(os.path.join(CSRC, "ctn_cln.hip")).read()
    assert "constexpr int CLN_NT = %d, CLN_FR = %d;" % (NO.CLN_NT, NO.CLN_FR) in src
    assert "constexpr int C4_NT = %d, C4_FR = %d, C4_NG = C4_NT / (C4_FR / 4);" % (NO.C4_NT, NO.C4_FR) in src
    assert NO.C4_NG == NO.C4_NT // (NO.C4_FR // 4) == 256 // (16 // 4)           # the 16-frame form has the same 64 channel groups
    assert "int g_ctn_cln_fr = %d;" % NO.DEFAULT_FR in src and "int g_ctn_cln_lean = %d;" % NO.DEFAULT_LEAN in src
    assert "int ctn_padded_frames(int K) { return (K + 63) / 64 * 64; }" in open(os.path.join(CSRC, "ctn_api.hip")).read()
    # the v4 gate and its width cap
    assert NO.V4_MAX_CH == 8 * NO.C4_NG
    assert src.count("return Ch <= 8 * C4_NG && Kp % C4_FR == 0 && ctn_aligned16(a) && ctn_aligned16(b) && ctn_aligned16(c);") == 1
    assert "if (cln_v4_ok(Ch, Kp, Y, Out, mean) && ctn_aligned16(rstd)) {" in src
    assert ("if (cln_v4_ok(Ch, Kp, dOut, Y, dY) && Kp % g_ctn_cln_fr == 0 && (!add || ctn_aligned16(add)) && (!relu_ref || "
            "ctn_aligned16(relu_ref))) {") in src
    assert len(re.findall(r"cln_v4_ok\(", src)) == 3
    # the four ladders
    assert "const int cpt = ctn_cdiv(Ch, C4_NG);" in src and "const int cpt = ctn_cdiv(Ch, CLN_NT / CLN_FR);" in src
    assert re.findall(r"cpt <= (\d+)\) CTN_CLN_FWD4\((\d+)\);", src) == [(str(c), str(c)) for c in NO.V4_CPT[:-1]]
    assert "else CTN_CLN_FWD4(%d);" % NO.V4_CPT[-1] in src
    assert re.findall(r"cpt <= (\d+)\) CTN_CLN_FWD\((\d+)\);", src) == [(str(c), str(c)) for c in NO.FWD_REG_CPT]
    assert re.findall(r"Ch <= (?:(\d+) \* )?C4_NG\) CTN_CLN_BWD4\((\d+)\);", src) == [("", "1"), ("2", "2"), ("4", "4")]
    assert "else CTN_CLN_BWD4(%d);" % NO.V4_CPT[-1] in src
    assert re.findall(r"Ch <= (\d+)\) CTN_CLN_BWD\((\d+), (\d+)\);", src) == [tuple(str(v) for v in row) for row in NO.BWD_REG]
    # no threshold that the mirror does not know: 1 (the gate) + 3 + 5 + 3 + 5
    assert len(re.findall(r"\b(?:cpt|Ch) <= ", src)) == 1 + len(NO.V4_CPT) - 1 + len(NO.FWD_REG_CPT) + len(NO.V4_CPT) - 1 + len(NO.BWD_REG)
    assert len(re.findall(r"\bhipLaunchKernelGGL\(\(?cln_(?:fwd|bwd_dx|bwd_v4)\w*kernel", src)) == 2 + 1 + 1 + 2 + 1 + 1 + 1
    # the LEAN condition, and the kernels behind the two frame counts
    assert "const bool lean = g_ctn_cln_lean && Ch == 8 * C4_NG && g_ctn_cln_fr == 16 && alpha && !add && !relu_ref;" in src
    assert "(cln_bwd_v4_kernel<8, 256, 16, true>)" in src
    assert "(cln_fwd_v4_kernel<CPT_, 256, 16>)" in src and "(cln_fwd_v4_kernel<CPT_>)" in src
    assert "(cln_bwd_v4_kernel<CPT_, 256, 16>)" in src and "(cln_bwd_v4_kernel<CPT_, C4_NT, C4_FR>)" in src
    assert "int ctn_cln_bwd_blocks(int M, int Kp) { return M * ctn_cdiv(Kp, g_ctn_cln_fr); }" in src
    assert "constexpr float" not in src and "#define CTN_EPS 1e-8f" in open(os.path.join(CSRC, "ctn_common.h")).read()


def test_plans_at_the_thresholds():
    f, b = NO.plan_fwd, NO.plan_bwd
    assert [f(c, 64) for c in (1, 64, 65, 128, 129, 256, 257, 512)] == ["v4/CPT%d/fr16" % c for c in (1, 1, 2, 2, 4, 4, 8, 8)]
    assert f(512, 64, fr=32) == "v4/CPT8/fr32" and f(513, 64) == "reg/CPT32" and f(1024, 64) == "reg/CPT32" and f(1025, 64) == "generic"
    assert [f(c, 40) for c in (3, 64, 65, 128, 129, 256, 257, 512)] == ["reg/CPT%d" % c for c in (2, 2, 4, 4, 8, 8, 16, 16)]
    assert f(64, 64, aligned=False) == "reg/CPT2" and f(64, 96) == "v4/CPT1/fr16" and f(64, 48) == "reg/CPT2"
    assert b(512, 64) == "lean" and b(512, 64, lean=0) == "v4/CPT8/fr16" and b(512, 64, fr=32) == "v4/CPT8/fr32"
    assert b(512, 64, alpha=False) == b(512, 64, add=True) == b(512, 64, add=True, relu_ref=True) == b(511, 64) == "v4/CPT8/fr16"
    assert [b(c, 68) for c in (32, 33, 64, 65, 128, 129, 256, 257, 512, 513)] == [
        "dxreg/2x512", "dxreg/4x512", "dxreg/4x512", "dxreg/8x512", "dxreg/8x512", "dxreg/16x512", "dxreg/16x512", "dxreg/16x1024",
        "dxreg/16x1024", "generic"]
    assert b(64, 64, aligned=False) == "dxreg/4x512" and b(513, 64) == "generic"
    assert all(NO.padded(K) % 64 == 0 and 0 <= NO.padded(K) - K < 64 for K in range(1, 300))


# ---- coverage --------------------------------------------------------------------------------------------------------------------
def _kinds(cases, label_of):
    by = {}
    for c in cases:
        by.setdefault(label_of(c), []).append(c)
    return by


@pytest.mark.parametrize("fr", [16, 32])
def test_case_tables_reach_every_label(fr):
    fwd = _kinds(NO.fwd_cases(), lambda c: NO.fwd_label(c, fr))
    bwd = _kinds(NO.bwd_cases(), lambda c: NO.bwd_label(c, fr))
    assert set(fwd) == set(NO.FWD_LABELS[fr]) and set(bwd) == set(NO.BWD_LABELS[fr])
    for d in (fwd, bwd):
        for label, cs in d.items():
            two = [c for c in cs if c.M == 2]
            if label.startswith("v4") or label == "lean":
                # the four kinds of K: one frame, no pad, a ragged frame quad, whole workgroups of pad frames
                assert all(c.Kp == NO.padded(c.K) and c.mis is None for c in cs), label
                ks = {c.K for c in two}
                assert 1 in ks and 64 in ks and any(k % 4 for k in ks - {1, 65}), (label, ks)
                assert 65 in ks, (label, ks)
                assert label != "lean" or ks >= {1, 61, 64, 130}
            else:
                frames = {(c.K, c.Kp) for c in two}
                assert frames >= set(NO.FALLBACK_FRAMES), (label, frames)
                assert all(c.Kp % 32 != 0 or c.mis is not None or c.Ch > NO.V4_MAX_CH for c in cs), label
                if d is bwd:
                    assert all(c.Kp % 4 == 0 for c in cs)
                else:
                    assert (37, 37) in frames
                if label != "generic" and not label.endswith("CPT32"):       # the alignment fallbacks, at Kp = 64 and 128
                    mis = {(c.mis, c.Kp) for c in cs if c.mis}
                    want = {("mean", 64), ("mean", 128)} if d is fwd else {("dY", 64), ("dY", 128), ("add", 64), ("add", 128)}
                    assert mis == want, (label, mis)
            assert {c.prelu for c in cs} == ({True} if label == "lean" else {True, False}), label
    for label, cs in bwd.items():                   # every pair of options per backward label
        opts = {(c.prelu, c.mode) for c in cs}
        assert opts == ({(True, "plain")} if label == "lean" else {(p, m) for p in (True, False) for m in NO.MODES}), (label, opts)
    # the widths on either side of every threshold, and the grids that are no multiple of 8
    assert {c.Ch for c in NO.fwd_cases() if NO.fwd_label(c).startswith("v4")} == set(NO.V4_WIDTHS)
    assert {c.Ch for c in NO.bwd_cases() if NO.bwd_label(c, lean=0).startswith("v4")} == set(NO.V4_WIDTHS)
    assert {c.Ch for c in NO.fwd_cases() if not NO.fwd_label(c).startswith("v4")} == set(NO.FWD_FALLBACK_WIDTHS) | {3}
    assert {c.Ch for c in NO.bwd_cases() if NO.bwd_label(c)[:2] in ("dx", "ge")} == set(NO.BWD_FALLBACK_WIDTHS)
    for cases, lab in ((NO.fwd_cases(), NO.fwd_label), (NO.bwd_cases(), NO.bwd_label)):
        grids = {c.M * c.Kp // 16 for c in cases if lab(c).startswith("v4") and c.M != 2}
        assert grids == {12, 4}
    assert max(c.Ch * c.Kp * c.M for c in NO.fwd_cases() + NO.bwd_cases()) <= 1100 * 130 * 3
    # ctn_cln_bwd_finalize: all tail, the unrolled loop exactly, loop + tail, more than 256 dalpha partials
    assert [NO.bwd_blocks(M, Kp) for M, Kp in NO.FINALIZE_SHAPES] == [28, 32, 36, 320]


# ---- the oracle against autograd -----------------------------------------------------------------------------------------------
def _close(got, ref, what):
    e = NO.rel_err(got, ref, "all")
    assert e < 1e-10, (what, e)


def _leaf(t):
    return t.clone().requires_grad_(True)


@pytest.mark.parametrize("Ch,K,Kp", [(1, 5, 8), (2, 7, 8), (5, 8, 8), (70, 13, 64)])
@pytest.mark.parametrize("pre", [True, False])
@pytest.mark.parametrize("mode", NO.MODES)
def test_cln_oracle_matches_autograd(Ch, K, Kp, pre, mode):
    i = NO.make_inputs(Ch, K, Kp, 2, zeros=0)
    u, g, b = _leaf(i.Y[..., :K]), _leaf(i.gamma), _leaf(i.beta)
    a = _leaf(torch.tensor([i.alpha], dtype=F64))
    dOut, add, R = i.dOut[..., :K], i.add[..., :K], i.relu_ref[..., :K]
    y = torch.where(R > 0, u, u.detach()) if mode == "mask" else u          # the gradient reaches u through the mask only
    p = torch.where(y >= 0, y, a * y) if pre else y
    mu = p.mean(1, keepdim=True)
    var = ((p - mu) ** 2).mean(1, keepdim=True)
    out = g.view(1, Ch, 1) * (p - mu) / torch.sqrt(var + NO.EPS) + b.view(1, Ch, 1)
    loss = (out * dOut).sum() + ((y * add).sum() if mode != "plain" else 0.0)
    loss.backward()
    f = NO.run_fwd(i, pre)
    _close(f["out"][..., :K], out.detach(), "out")
    assert float(f["out"][..., K:].abs().sum()) == 0.0
    _close(f["mean"][:, :K], mu.detach()[:, 0], "mean")
    _close(f["rstd"][:, :K], 1 / torch.sqrt(var.detach()[:, 0] + NO.EPS), "rstd")
    assert float(f["mean"][:, K:].abs().sum()) == 0.0 and bool((f["rstd"][:, K:] == 1 / torch.sqrt(torch.tensor(NO.EPS, dtype=F64))).all())
    o = NO.cln_bwd(i.dOut, i.Y, f["mean"], f["rstd"], K, i.gamma, i.alpha if pre else None, i.add if mode != "plain" else None,
                   i.relu_ref if mode == "mask" else None)
    scale = u.grad.abs().max() + o["dbeta"].abs().max()
    assert float((o["dY"][..., :K] - u.grad).abs().max()) < 1e-10 * float(scale)      # (Ch = 1, 2: the exact gradient is ~0)
    assert float(o["dY"][..., K:].abs().sum()) == 0.0
    _close(o["dbeta"], b.grad, "dbeta")
    if Ch > 1:
        _close(o["dgamma"], g.grad, "dgamma")
    if pre:
        assert float((o["dalpha"] - a.grad).abs()) < 1e-10 * float(o["dalpha|abs"] + 1e-300), "dalpha"
    for n in ("dgamma", "dbeta") + (("dalpha",) if pre else ()):
        t = o[n + "|terms"]
        assert torch.equal(t.abs().sum((0, 2) if n != "dalpha" else (0, 1, 2)).reshape(-1), o[n + "|abs"].reshape(-1))


@pytest.mark.parametrize("Ch,K,M", [(1, 3, 2), (7, 5, 1), (7, 64, 2), (3, 70, 2)])
@pytest.mark.parametrize("pre", [True, False])
@pytest.mark.parametrize("stats", ["train", "eval"])
def test_bn_oracle_matches_autograd(Ch, K, M, pre, stats):
    i = NO.make_bn_inputs(Ch, K, M)
    training = stats == "train"
    y, g, b = _leaf(i.Y[..., :K]), _leaf(i.gamma), _leaf(i.beta)
    a = _leaf(torch.tensor([i.alpha], dtype=F64))
    rm, rv = i.running[0].clone(), i.running[1].clone()
    out = Fn.batch_norm(torch.where(y >= 0, y, a * y) if pre else y,      # (torch's own prelu takes the slope at 0)
                         rm, rv, g, b, training, NO.BN_MOMENTUM, NO.BN_EPS)
    out.backward(i.dOut[..., :K])
    f = NO.run_bn_fwd(i, stats, pre)
    _close(f["out"][..., :K], out.detach(), "out")
    assert float(f["out"][..., K:].abs().sum()) == 0.0
    _close(f["running_mean"], rm, "running_mean")
    _close(f["running_var"], rv, "running_var")
    o = NO.bn_bwd(i.dOut, i.Y, f["mr"], K, i.gamma, i.alpha if pre else None, training)
    _close(o["dY"][..., :K], y.grad, "dY")
    assert float(o["dY"][..., K:].abs().sum()) == 0.0
    _close(o["dgamma"], g.grad, "dgamma")
    _close(o["dbeta"], b.grad, "dbeta")
    if pre:
        assert float((o["dalpha"] - a.grad).abs()) < 1e-10 * float(o["dalpha|abs"]), "dalpha"
    assert NO.run_bn_fwd(i, "train_norun", pre)["running_mean"] is None


def test_bn_single_element_closed_form():
    """n = M K = 1 (torch refuses it): var = 0, out = beta, and the running variance takes var itself."""
    i = NO.make_bn_inputs(7, 1, 1)
    f = NO.run_bn_fwd(i, "train", True)
    assert torch.equal(f["out"][0, :, 0], i.beta) and bool((f["mr"][:, 1] == NO.BN_EPS ** -0.5).all())
    assert torch.allclose(f["running_var"], (1 - NO.BN_MOMENTUM) * i.running[1], rtol=1e-15)
    assert torch.allclose(f["running_mean"], (1 - NO.BN_MOMENTUM) * i.running[0] + NO.BN_MOMENTUM * NO.prelu(i.Y[0, :, 0], i.alpha), rtol=1e-15)


# ---- the limits: reachable in fp32, and out of reach of a defect ------------------------------------------------------------------
def _worst(errs, where, worst):
    for name, (e, lim) in errs.items():
        if e / lim > worst.get(name, (0,))[0]:
            worst[name] = (e / lim, e, where)


def test_limits_are_reachable_in_fp32():
    """The oracle's own formulas in fp32 (torch's CPU kernels: another summation order than the HIP kernels', the same number format,
    the same two-pass variance) stay at least 4x inside every limit of tests/test_gpu_norm_forms.py on that test's inputs."""
    worst = {}
    for c in dict.fromkeys((c.Ch, c.K, c.Kp, c.M, c.prelu, c.seed) for c in NO.fwd_cases()):
        Ch, K, Kp, M, pre, seed = c
        i = NO.make_inputs(Ch, K, Kp, M, seed)
        _worst(NO.cln_errors(NO.run_fwd(i, pre, F32), NO.run_fwd(i, pre), K), c, worst)
    for c in dict.fromkeys((c.Ch, c.K, c.Kp, c.M, c.prelu, c.mode, c.seed) for c in NO.bwd_cases()):
        Ch, K, Kp, M, pre, mode, seed = c
        i = NO.make_inputs(Ch, K, Kp, M, seed)
        _worst(NO.cln_errors(NO.run_bwd(i, pre, mode, F32), NO.run_bwd(i, pre, mode), K), c, worst)
    for K, Kp in ((1, 64), (61, 64), (64, 64), (37, 40)):       # the known-answer inputs
        i = NO.make_ch2_inputs(K, Kp)
        _worst({"out": NO.cln_errors(NO.run_fwd(i, True, F32), NO.run_fwd(i, True), K)["out"]}, ("ch2", K), worst)
        for pre in (True, False):
            exact, slack = NO.ch2_dy_bound(i.dOut, *i.stats[pre], i.gamma)
            got = NO.run_bwd(i, pre, "plain", F32)["dY"].double().abs().amax(1)
            assert bool((got <= exact + 0.25 * slack)[:, :K].all()), (K, pre)
            ref = NO.run_bwd(i, pre, "plain")["dY"].abs().amax(1)
            assert bool((ref <= exact + 0.25 * slack)[:, :K].all()), (K, pre)       # (the handed statistics are rounded to fp32: in the slack)
    for Kp in (64, 40):
        i = NO.make_inputs(40, Kp - 3, Kp, zeros=0.25)
        _worst(NO.cln_errors(NO.run_fwd(i, True, F32), NO.run_fwd(i, True), Kp - 3), ("zeros", Kp), worst)
        for mode in ("plain", "mask"):
            _worst(NO.cln_errors(NO.run_bwd(i, True, mode, F32), NO.run_bwd(i, True, mode), Kp - 3), ("zeros", Kp, mode), worst)
    bad = {k: v for k, v in worst.items() if v[0] > 0.25}
    assert not bad, bad
    assert set(worst) == {"out", "mean", "rstd", "dY", "dgamma", "dbeta", "dgamma sum", "dbeta sum", "dalpha sum"}


def test_bn_limits_are_reachable_in_fp32():
    worst = {}
    for Ch, K, M, st, pre in NO.bn_cases():
        i = NO.make_bn_inputs(Ch, K, M)
        _worst(NO.bn_errors(NO.run_bn_fwd(i, st, pre, F32), NO.run_bn_fwd(i, st, pre), K), (Ch, K, M, st, pre), worst)
        _worst(NO.bn_errors(NO.run_bn_bwd(i, st, pre, F32), NO.run_bn_bwd(i, st, pre), K), (Ch, K, M, st, pre), worst)
    bad = {k: v for k, v in worst.items() if v[0] > 0.25}
    assert not bad, bad
    assert set(worst) == {"out", "dY", "running_mean", "running_var", "dgamma sum", "dbeta sum", "dalpha sum"}


def _ratio(errs, name):
    e, lim = errs[name]
    return e / lim


def test_limits_catch_defects():
    """Eight wrong fp64 models; each must miss a limit that it can affect by 10x or more, on a case of the tables."""
    seen = {}

    def cln(name, Ch, K, Kp, pre, mode, figure, fwd=False, zeros=1):
        i = NO.make_inputs(Ch, K, Kp, 2, NO.CHECKED_SEEDS.get(Ch, 0), zeros)
        run = (lambda: NO.run_fwd(i, pre)) if fwd else (lambda: NO.run_bwd(i, pre, mode))
        ref = run()
        with NO.defect(name):
            got = run()
        seen.setdefault(name, []).append((figure, _ratio(NO.cln_errors(got, ref, K), figure)))

    for Ch in (65, 129, 511):                                   # (at whole groups of 64 the padded count is the true one)
        cln("mean_padded", Ch, 17, 64, True, None, "out", fwd=True)
        cln("mean_padded", Ch, 17, 64, True, None, "mean", fwd=True)
    for Ch, K, Kp in ((3, 15, 64), (257, 65, 128), (513, 37, 40)):
        cln("frame_k", Ch, K, Kp, True, "plain", "dbeta")
        cln("dbeta_kp", Ch, K, Kp, False, "add", "dbeta sum")
    for Ch in (3, 65, 512):
        cln("drop_channel", Ch, 64, 64, True, None, "out", fwd=True)
        cln("drop_channel", Ch, 64, 64, False, "plain", "dY")
        cln("add_after_mask", Ch, 61, 64, True, "mask", "dY")
    cln("prelu_zero", 40, 61, 64, True, "mask", "dY", zeros=0.25)
    cln("prelu_zero", 40, 61, 64, True, "plain", "dY", zeros=0.25)
    for Ch, K, M in ((7, 3, 2), (257, 255, 2), (1, 257, 1)):
        i = NO.make_bn_inputs(Ch, K, M)
        ref = NO.run_bn_fwd(i, "train", True)
        for name, figure in (("bn_biased", "running_var"), ("bn_frame_k", "out")):
            with NO.defect(name):
                seen.setdefault(name, []).append((figure, _ratio(NO.bn_errors(NO.run_bn_fwd(i, "train", True), ref, K), figure)))
    assert set(seen) == set(NO.DEFECTS) and len(NO.DEFECTS) >= 6
    weak = {k: v for k, v in seen.items() if min(r for _, r in v) < 10}
    assert not weak, weak
