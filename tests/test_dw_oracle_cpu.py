"""tests/dw_oracle.py itself, on the CPU: the fp64 closed forms of the depthwise kernels against autograd, the limits of
tests/test_gpu_depthwise.py against what fp32 arithmetic can reach and against four deliberately wrong models, and the mirror of
the kernels' patch constants against csrc/ctn_dw.hip."""
import os
import re

import pytest
import torch

import dw_oracle as DO
from conftest import ROOT
from oracle import ctn_oracle as O

F64 = torch.float64
SOURCE = os.path.join(ROOT, "conv-tasnet_amd", "csrc", "ctn_dw.hip")


# ---- the constants mirror ------------------------------------------------------------------------------------------------------
def test_constants_match_the_source():
    src = open(SOURCE).read()
    for name in ("MAXP", "FWD_BUF_S", "FWD_BUF_L", "BWD_BUF_S", "BWD_BUF_M", "BWD_BUF_L"):
        m = re.search(r"constexpr int [^;]*\b%s = (\d+)[,;]" % name, src)
        assert m, name
        assert int(m.group(1)) == getattr(DO, name), name
    # the patch is chosen from the halo, in the one geometry helper that every depthwise entry point goes through:
    # forward small <= 192, backward small <= 128, medium <= 256
    t = [str(v) for v in (DO.FWD_SMALL_HALO, DO.BWD_SMALL_HALO, DO.BWD_MEDIUM_HALO)]
    assert re.findall(r"halo <= (\d+)", src) == t       # (no further threshold that the mirror does not know)
    assert "const bool small = halo <= %s;" % t[0] in src
    assert "const bool small = halo <= %s, medium = !small && halo <= %s;" % (t[1], t[2]) in src
    # seg = ((BUF - halo - 8) / 64) * 64, once per direction and nowhere else
    assert len(re.findall(r"(?<![.\w])seg = ", src)) == 2 and len(re.findall(r"\bdw_geometry\(\"ctn_dw_\w+\", (?:true|false),", src)) == 5
    assert src.count("seg = (((small ? FWD_BUF_S : FWD_BUF_L) - halo - 8) / 64) * 64;") == 1
    assert src.count("seg = (((small ? BWD_BUF_S : (medium ? BWD_BUF_M : BWD_BUF_L)) - halo - 8) / 64) * 64;") == 1
    assert src.count("const bool vec4 = (a.dil % 4 == 0) && (a.padl % 4 == 0);") == 2
    assert DO.seg_of(1024, 2) == 960 and DO.seg_of(1792, 512) == 1216


def test_configurations_reach_the_variants_they_are_for():
    """Every BUF x tap path x (kernel size compiled in | run time) combination that the table names, recomputed from the
    mirrored constants; the seam frame counts follow from the same numbers."""
    for tag, cfg in DO.CONFIGS.items():
        p = DO.plan(*cfg)
        assert (p.halo, p.vec4, p.fwd_buf, p.fwd_seg, p.bwd_buf, p.bwd_seg) == DO.EXPECTED_PLAN[tag], tag
        K = DO.long_K(tag)
        assert K % 4 == 3 and K > max(p.fwd_seg, p.bwd_seg) + 64 and K <= 3456
        assert all(k >= 1 for k in DO.fwd_Ks(tag)) and set(DO.bwd_Ks(tag)) <= set(DO.fwd_Ks(tag))
    seen_f = {(DO.plan(*c).fwd_buf, DO.plan(*c).vec4, DO.plan(*c).pt) for c in DO.CONFIGS.values()}
    seen_b = {(DO.plan(*c).bwd_buf, DO.plan(*c).vec4, DO.plan(*c).pt) for c in DO.CONFIGS.values()}
    for buf in "SL":
        for vec4 in (False, True):
            assert (buf, vec4, 3) in seen_f
    for buf in "SML":
        for vec4 in (False, True):
            assert (buf, vec4, 3) in seen_b
    for vec4 in (False, True):                      # the run-time-P kernels: both tap paths; large patches on the float4 path
        assert ("S", vec4, 0) in seen_f and ("S", vec4, 0) in seen_b
    assert ("L", True, 0) in seen_f and ("L", True, 0) in seen_b
    assert {c[0] for c in DO.CONFIGS.values()} >= {1, 2, 3, 5, DO.MAXP}
    assert set(DO.short_Ks("E")) == {1, 5, 256, 513} and set(DO.short_Ks("A")) == {1, 3, 5}


# ---- the oracle against autograd -----------------------------------------------------------------------------------------------
def _close(got, ref, what):
    e = DO.rel_err(got, ref, "all")
    assert e < 1e-10, (what, e)


def _leaf(t):
    return t.clone().requires_grad_(True)


@pytest.mark.parametrize("P", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("below", [True, False])
def test_oracle_matches_autograd(P, causal, below):
    dil = 3 if causal else 2
    halo = (P - 1) * dil
    K = max(2, halo - 1) if below else 2 * halo + 7
    M, H, a1v, a2v = 2, 5, 0.2, 0.3
    gen = torch.Generator().manual_seed(P * 10 + causal)

    def rn(*s):
        return torch.randn(*s, generator=gen, dtype=F64)

    h1_, D_, dN2 = 1.5 * rn(M, H, K) + 0.2, rn(H, P), rn(M, H, K)
    g1_, b1_, g2_, b2_ = 1 + 0.3 * rn(H), 0.3 * rn(H), 1 + 0.3 * rn(H), 0.3 * rn(H)
    n = H * K
    for norm in ("gLN", "cLN"):
        h1, D, g1, b1, g2, b2 = (_leaf(t) for t in (h1_, D_, g1_, b1_, g2_, b2_))
        a1, a2 = _leaf(torch.tensor([a1v], dtype=F64)), _leaf(torch.tensor([a2v], dtype=F64))
        nf = O.gln if norm == "gLN" else O.cln
        p1 = O.prelu(h1, a1)
        n1 = nf(p1, g1.view(1, H, 1), b1.view(1, H, 1))
        n1.retain_grad()
        d = O.depthwise(n1, D.view(H, 1, P), dil, causal)
        p2 = O.prelu(d, a2)
        (nf(p2, g2.view(1, H, 1), b2.view(1, H, 1)) * dN2).sum().backward()
        dz, p1, p2 = d.detach(), p1.detach(), p2.detach()
        if norm == "gLN":
            ms1, ms2 = DO.gln_stats(DO.row_sums(p1), n), DO.gln_stats(DO.row_sums(p2), n)
            f = DO.fwd(h1_, D_, dil, causal, gln=(*ms1, g1_, b1_, a1v), epi_alpha=a2v)
            _close(f["Z"], dz, "fwd gLN Z")
            _close(f["epi_part"].sum(1), DO.row_sums(p2).sum(1), "epi_part")
            rows8 = DO.gln2_row_sums(dN2, dz, D_, dil, causal, g1_, b1_, g2_, a2v, ms2)
            args = (dN2, dz, h1_, D_, dil, causal, g1_, b1_, a1v, ms1, g2_, a2v, ms2)
            o = DO.bwd_gln(*args, rows8[..., :2].sum(1))
            xh1 = (p1 - ms1[0][:, None, None]) * ms1[1][:, None, None]
            t = g1_[None, :, None] * n1.grad
            _close(o["sums1_part"], torch.stack([t.sum(2), (t * xh1).sum(2)], 2), "sums1_part")
            o2 = DO.bwd_gln2(*args, rows8.sum(1))
            _close(o2["dY1"], h1.grad, "dY1")
            _close(o2["dalpha1"], a1.grad, "dalpha1")
            for oo in (o, o2):
                _close(oo["dgamma1"], g1.grad, "dgamma1")
                _close(oo["dbeta1"], b1.grad, "dbeta1")
            outs = [o, o2]
        else:
            st1, st2 = DO.cln_stats(p1), DO.cln_stats(p2)
            _close(DO.fwd(h1_, D_, dil, causal, cln=(*st1, g1_, b1_, a1v))["Z"], dz, "fwd cLN Z")
            fc = DO.cln_fc(dN2, dz, g2_, a2v, *st2)
            o = DO.bwd_cln(dN2, dz, n1.detach(), D_, dil, causal, g2_, a2v, fc)
            outs = [o, DO.bwd_cln(dN2, dz, h1_, D_, dil, causal, g2_, a2v, fc, first=(g1_, b1_, a1v, *st1))]
        _close(o["dN1"], n1.grad, norm + " dN1")
        for oo in outs:
            _close(oo["dD"], D.grad, norm + " dD")
            _close(oo["dgamma2"], g2.grad, norm + " dgamma2")
            _close(oo["dbeta2"], b2.grad, norm + " dbeta2")
            _close(oo["dalpha2"], a2.grad, norm + " dalpha2")
        if norm == "cLN":
            _close(outs[1]["dN1"], n1.grad, "cLN recomputed dN1")
    y, D = _leaf(h1_), _leaf(D_)
    z = O.depthwise(y, D.view(H, 1, P), dil, causal)
    (z * dN2).sum().backward()
    _close(DO.fwd(h1_, D_, dil, causal)["Z"], z.detach(), "plain Z")
    o = DO.bwd_plain(dN2, h1_, D_, dil, causal)
    _close(o["dY"], y.grad, "plain dY")
    _close(o["dD"], D.grad, "plain dD")


def test_parts_and_helpers():
    rows = torch.arange(2 * 6 * 8, dtype=F64).reshape(2, 6, 8)
    assert DO.parts3(rows).shape == (2, 3, 8) and torch.equal(DO.parts3(rows).sum(1), rows.sum(1))
    rows = torch.arange(3 * 70 * 2, dtype=F64).reshape(3, 70, 2)
    assert torch.equal(DO.parts3(rows).sum(1), rows.sum(1))
    x = torch.tensor([-1.0, 0.0, 2.0], dtype=F64)
    assert DO.prelu(x, 0.25).tolist() == [-0.25, 0.0, 2.0] and DO.dprelu(x, 0.25).tolist() == [0.25, 1.0, 1.0]


# ---- the limits: reachable in fp32, and out of reach of a defect --------------------------------------------------------------------
def _cases(tag):
    cfg = DO.CONFIGS[tag]
    for K in DO.fwd_Ks(tag):
        forms = DO.FWD_FORMS + (DO.BWD_FORMS if K in DO.bwd_Ks(tag) else ())
        yield K, DO.make_inputs(*cfg, K), forms


@pytest.mark.parametrize("tag", list(DO.CONFIGS))
def test_limits_are_reachable_in_fp32(tag):
    """The oracle's own formulas in fp32 (torch's CPU kernels: another summation order than the HIP kernels', the same number
    format) stay at least 4x inside every limit of tests/test_gpu_depthwise.py on that test's inputs."""
    worst = {}
    for K, inp, forms in _cases(tag):
        for form in forms:
            ref, got = DO.run_form(form, inp), DO.run_form(form, inp, dtype=torch.float32)
            for name, r in ref.items():
                cls, how = DO.OUTPUTS[(form, name)]
                e = DO.rel_err(got[name], r, how) / DO.LIMIT[cls]
                if e > worst.get((form, name), (0, 0))[0]:
                    worst[(form, name)] = (e, K)
    bad = {k: v for k, v in worst.items() if v[0] > 0.25}
    assert not bad, bad


@pytest.mark.parametrize("mode", ["set", "taps"])
def test_zero_case_is_reachable_in_fp32(mode):
    inp = DO.make_inputs(*DO.CONFIGS["B"], 203, zeros=mode)
    assert float((inp.h1 == 0).sum()) >= 6 and float((inp.Dz_g == 0).sum()) >= 6 and float((inp.Dz_c == 0).sum()) >= 6
    assert inp.h1[0, 0, 0] == 0 and inp.h1[1, -1, -1] == 0 and bool((inp.Dz_g[..., 0] == 0).any() and (inp.Dz_g[..., -1] == 0).any())
    out = {}
    for form in DO.BWD_FORMS:
        ref, got = DO.run_form(form, inp), DO.run_form(form, inp, dtype=torch.float32)
        out[form] = ref
        for name, r in ref.items():
            cls, how = DO.OUTPUTS[(form, name)]
            assert DO.rel_err(got[name], r, how) <= 0.25 * DO.LIMIT[cls], (form, name)
    if mode == "taps":          # d is the conv of the first norm's output: the first norm's backward on dN1 is ctn_dw_bwd_gln2's dY1
        o, n = out["bwd_gln"], inp.H * inp.K
        xh1 = (DO.prelu(inp.h1, inp.a1) - inp.ms1[0][:, None, None]) * inp.ms1[1][:, None, None]
        c = o["sums1_part"].sum(1) / n
        da1 = inp.ms1[1][:, None, None] * (inp.g1[None, :, None] * o["dN1"] - c[:, 0, None, None] - xh1 * c[:, 1, None, None])
        assert DO.rel_err(da1 * DO.dprelu(inp.h1, inp.a1), out["bwd_gln2"]["dY1"], "utt") < 0.25 * 2e-5


def _tensor_out(form):
    return {"bwd_plain": "dY", "bwd_gln": "dN1", "bwd_gln2": "dY1", "bwd_cln": "dN1", "bwd_cln_x": "dN1"}.get(form, "Z")


@pytest.mark.parametrize("tag", list(DO.CONFIGS))
def test_limits_catch_defects(tag):
    """Four wrong fp64 models, on the long frame count of every configuration.  Each must miss every limit that it can
    affect by 10x or more.  What a defect can affect:
      * pad_left off by one shifts every tap: the tensor output of every form and every dD;
      * row c with the taps of row c+1: the tensor output of every form (the tap gradients do not read the taps);
      * an x image that is zero from the second segment's first halo frame on: Z from frame seg_f on, and the share of the
        frames from seg_b on in every dD;
      * frame K treated as valid: the normalised pad frame (prologue forms) reaches Z through the right-hand taps (non-causal,
        P > 1), and its dd (gLN forms: -rstd2 (c1 + xhat2(0) c2), not 0) reaches the last frames' input gradient (P > 1).
        Its own sums are 0 (dN2 = d = 0 there), and its share of dD is one frame's: not listed."""
    cfg = DO.CONFIGS[tag]
    P, dil, causal = cfg
    p = DO.plan(*cfg)
    inp = DO.make_inputs(*cfg, DO.long_K(tag))
    ref = {f: DO.run_form(f, inp) for f in DO.FWD_FORMS + DO.BWD_FORMS}
    checks = []

    def run(kw, affected):
        with DO.defect(**kw):
            for form, name in affected:
                checks.append((sorted(kw), form, name, DO.run_form(form, inp)[name]))

    every = DO.FWD_FORMS + DO.BWD_FORMS
    run({"padl": 1}, [(f, _tensor_out(f)) for f in every] + [(f, "dD") for f in DO.BWD_FORMS])
    run({"roll": 1}, [(f, _tensor_out(f)) for f in every])
    run({"xzero_fwd": p.fwd_seg, "xzero_bwd": p.bwd_seg}, [(f, "Z") for f in DO.FWD_FORMS] + [(f, "dD") for f in DO.BWD_FORMS])
    if P > 1:
        forms = ("bwd_gln", "bwd_gln2") + (() if causal else ("fwd_gln", "fwd_cln"))
        for form in forms:
            checks.append((["frame K"], form, _tensor_out(form), DO.with_frame_K(form, inp)[_tensor_out(form)]))
    weak = []
    for kw, form, name, got in checks:
        cls, how = DO.OUTPUTS[(form, name)]
        e = DO.rel_err(got, ref[form][name], how)
        if e < 10 * DO.LIMIT[cls]:
            weak.append((kw, form, name, e))
    assert not weak, weak
