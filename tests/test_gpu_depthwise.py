"""Every variant of dw_fwd_kernel / dw_bwd_kernel (csrc/ctn_dw.hip) through the C ABI against tests/dw_oracle.py in fp64, at the
kernels' seams.

The launchers pick a variant from halo = (P-1) dilation (the LDS patch: forward S / L, backward S / M / L), from the alignment
of dilation and pad_left (float4 or scalar taps) and from the kernel size (3 compiled in, any other at run time); the entry
point picks the form (plain, gLN / cLN prologue, statistics epilogue; five backward forms).  dw_oracle.CONFIGS holds eleven
(P, dilation, causal) that between them reach every patch x tap path, and the run-time kernel size at P = 1, 2, 5 and 8.  Each
runs every form at frame counts that put a segment seam at the end of the data (K = seg), leave a second segment with one valid
frame (seg + 1), cross a seam with a ragged float4 tail (max(seg_f, seg_b) + 67, K % 4 == 3) and, at four configurations, are
shorter than the receptive field (1, 5, dilation, halo + 1).  M = 2, H = 6: the second workgroup of an utterance has two dead
waves; the second utterance is 20 times quieter, so errors are taken per utterance.

The kernels are handed what they are handed in a training step, built by the test in fp64 from the definitions (statistics,
the S1 / S2 and the eight ctn_pw_dgrad_gln2 sums split over three parts, the per-frame constants fc) and rounded to the
buffers' formats; the oracle gets the same rounded values.  Outputs are pre-filled with NaN.  Per case: nothing is left NaN,
frames K..Kp are exactly 0, a second call gives the same bits, and the tracked maximum of ctn_dw_bwd_gln2 is bitwise max |dY1[m]|.

Limits (max |got - ref| / max |ref|), the project's existing ones, as ceilings:
    3e-6   Z, dY of the plain forms                                          (test_gpu_parity.py::test_dw_plain_fwd_bwd)
    2e-5   every fused tensor, dD, dgamma / dbeta, epi_part, sums1_part, ms_out   (the fused entry points in test_gpu_parity.py)
    1e-4   the scalars dalpha1, dalpha2                                      (test_temporal_block_fwd_bwd)
tests/test_dw_oracle_cpu.py shows on these inputs that fp32 arithmetic stays 4x inside each, and that four wrong models (pad_left
off by one, a zeroed x image in the second segment, frame K valid, the next row's taps) miss each by 10x or more.

Largest figure per kind of output over all cases of this module, first MI355X run (the `DW MAX` lines of -s).  Every one is
more than 4x below its ceiling; the ceilings stay where the project has them.
    kind                 largest    limit   at
    plain  Z             1.26e-07   3e-6    H K=961  fwd_plain
    plain  dY            1.06e-07   3e-6    H K=704  bwd_plain
    fused  Z             1.81e-07   2e-5    H K=1027 fwd_gln
    fused  epi_part      3.12e-07   2e-5    A K=1    fwd_gln
    fused  ms_out        0          2e-5    (the fp64 statistics rounded once)
    fused  dN1           6.40e-07   2e-5    A K=3    bwd_gln
    fused  dY1           3.23e-06   2e-5    I K=1    bwd_gln2 (test_tracked_maximum_ignores_dead_waves)
    fused  sums1_part    1.33e-06   2e-5    B K=1027 bwd_gln
    fused  dD            5.42e-07   2e-5    A K=705  bwd_gln
    fused  dgamma1       6.76e-07   2e-5    I K=705  bwd_gln
    fused  dbeta1        1.07e-06   2e-5    E K=513  bwd_gln
    fused  dgamma2       1.15e-07   2e-5    G K=5    bwd_gln
    fused  dbeta2        1.09e-07   2e-5    E K=256  bwd_cln
    scalar dalpha1       8.45e-06   1e-4    B K=1027 bwd_gln2
    scalar dalpha2       1.10e-05   1e-4    F K=1217 bwd_cln
    chain ctn_dw_bwd(1) + ctn_gln_prelu_bwd against ctn_dw_bwd_gln2 (test_prelu_at_exactly_zero): dY1 6.23e-08, dalpha1 1.45e-06
"""
import pytest
import torch

import dw_oracle as DO

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import ops  # noqa: E402

DEV = "cuda:0"
NAN = float("nan")
F32, F64 = torch.float32, torch.float64
WORST = {}


@pytest.fixture(autouse=True)
def _own_lines():
    print()                 # (-s: the DW lines start at the left margin, not behind the progress dots)
    yield


def nan(*shape, dtype=F32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def dev(t, Kp=None, dtype=F32):
    """A host tensor as the device buffer the kernels read: zero pad frames up to Kp, contiguous."""
    t = t.to(dtype)
    if Kp is not None:
        t = torch.nn.functional.pad(t, (0, Kp - t.shape[-1]))
    return t.contiguous().to(DEV)


def scalar(v):
    return torch.tensor([v], dtype=F32, device=DEV)


def ptr(t):
    return 0 if t is None else t.data_ptr()


class Case:
    """Device buffers of one dw_oracle.make_inputs() case."""

    def __init__(self, i):
        self.i, self.K, self.Kp = i, i.K, ops.padded_frames(i.K)
        Kp = self.Kp
        self.dims = (i.M, i.H, i.K, Kp, i.P, i.dil, int(i.causal))
        self.h1, self.dN2, self.dN2_c = dev(i.h1, Kp), dev(i.dN2, Kp), dev(i.dN2_c, Kp)
        self.Dz_g, self.Dz_c, self.X1_c = dev(i.Dz_g, Kp), dev(i.Dz_c, Kp), dev(i.X1_c, Kp)
        self.D, self.g1, self.b1, self.g2 = dev(i.D), dev(i.g1), dev(i.b1), dev(i.g2)
        self.a1, self.a2 = scalar(i.a1), scalar(i.a2)
        self.ms1, self.ms2 = dev(torch.stack(i.ms1, 1)), dev(torch.stack(i.ms2, 1))              # [M,2]
        self.mean1, self.rstd1 = dev(i.st1[0], Kp), dev(i.st1[1], Kp)                           # [M,Kp]
        self.fc = dev(i.fc, Kp)                                                                 # [M,4,Kp]
        self.part1 = dev(DO.parts3(i.part1), dtype=F64)                                         # [M,3,2]
        self.sums2 = dev(DO.parts3(i.rows8[..., :2]), dtype=F64)                                # [M,3,2]
        self.sums8 = dev(DO.parts3(i.rows8), dtype=F64)                                         # [M,3,8]


def run_gpu(form, c):
    """One form through the C ABI -> (outputs by the oracle's names, full-width tensors whose pad must be 0, pc or None)."""
    i, call = c.i, ctn.lib.call
    M, H, K, Kp, P = i.M, i.H, i.K, c.Kp, i.P
    T = nan(M, H, Kp)
    out, pc = {}, None
    if form == "fwd_plain":
        call("ctn_dw_fwd", ptr(c.h1), ptr(T), ptr(c.D), *c.dims, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
        out["Z"] = T
    elif form == "fwd_gln":
        ms, epi = nan(M, 2), nan(M, H, 2, dtype=F64)
        call("ctn_dw_fwd", ptr(c.h1), ptr(T), ptr(c.D), *c.dims, ptr(c.part1), 3, ptr(c.g1), ptr(c.b1), ptr(c.a1), ptr(ms),
             ptr(c.a2), ptr(epi), 0, 0)
        out.update(Z=T, ms_out=ms, epi_part=epi)
    elif form == "fwd_cln":
        call("ctn_dw_fwd_cln", ptr(c.h1), ptr(T), ptr(c.D), *c.dims, ptr(c.mean1), ptr(c.rstd1), ptr(c.g1), ptr(c.b1), ptr(c.a1), 0)
        out["Z"] = T
    elif form == "bwd_plain":
        pc, dD = nan(P, M, H), nan(H, P)
        call("ctn_dw_bwd", ptr(c.dN2), 0, ptr(c.h1), ptr(T), ptr(c.D), *c.dims, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, ptr(pc), 0, 0)
        call("ctn_dw_bwd_taps", ptr(pc), P, M, H, ptr(dD), 0)
        out.update(dY=T, dD=dD)
    elif form in ("bwd_gln", "bwd_gln2"):
        two = form == "bwd_gln2"
        pc = nan(P + (6 if two else 5), M, H)
        norms = (ptr(c.g1), ptr(c.b1), ptr(c.a1), ptr(c.ms1), ptr(c.g2), ptr(c.a2), ptr(c.ms2))
        v = {n: nan(H) for n in ("dgamma2", "dbeta2", "dgamma1", "dbeta1")}
        v.update(dD=nan(H, P), dalpha2=nan(1))
        if two:
            amax = torch.zeros((M, ops.AMAX_SLOTS), dtype=torch.int32, device=DEV)
            call("ctn_dw_bwd_gln2", ptr(c.dN2), ptr(c.Dz_g), ptr(c.h1), ptr(T), ptr(c.D), *c.dims, *norms, ptr(c.sums8), 3, ptr(pc),
                 ptr(amax), 0)
            v["dalpha1"] = nan(1)
            da1 = (ptr(pc[P + 5]), M * H, ptr(v["dalpha1"]))
            out.update(dY1=T, _amax=amax.view(F32).amax(1))
        else:
            s1 = nan(M, H, 2, dtype=F64)
            call("ctn_dw_bwd", ptr(c.dN2), ptr(c.Dz_g), ptr(c.h1), ptr(T), ptr(c.D), *c.dims, 1, *norms, ptr(c.sums2), 3, ptr(pc),
                 ptr(s1), 0)
            da1 = (0, 0, 0)
            out.update(dN1=T, sums1_part=s1)
        call("ctn_dw_bwd_finalize", ptr(pc), P, M, H, ptr(v["dD"]), ptr(v["dgamma2"]), ptr(v["dbeta2"]), ptr(v["dgamma1"]),
             ptr(v["dbeta1"]), ptr(v["dalpha2"]), *da1, 0)
        out.update(v)
    elif form in ("bwd_cln", "bwd_cln_x"):
        pc = nan(P + 3, M, H)
        first = (ptr(c.g1), ptr(c.b1), ptr(c.a1), ptr(c.mean1), ptr(c.rstd1)) if form == "bwd_cln_x" else (0, 0, 0, 0, 0)
        x1 = c.h1 if form == "bwd_cln_x" else c.X1_c
        v = dict(dD=nan(H, P), dgamma2=nan(H), dbeta2=nan(H), dalpha2=nan(1))
        call("ctn_dw_bwd_cln", ptr(c.dN2_c), ptr(c.Dz_c), ptr(x1), ptr(T), ptr(c.D), *c.dims, ptr(c.g2), ptr(c.a2), ptr(c.fc), *first,
             ptr(pc), 0)
        call("ctn_dw_bwd_cln_finalize", ptr(pc), P, M, H, ptr(v["dD"]), ptr(v["dgamma2"]), ptr(v["dbeta2"]), ptr(v["dalpha2"]), 0)
        out.update(dN1=T, **v)
    else:
        raise KeyError(form)
    torch.cuda.synchronize()
    return out, T, pc


def check_form(tag, form, c):
    """Runs the form twice and makes every per-case assertion; -> {output: error} and the kernel's outputs."""
    K = c.K
    got, T, pc = run_gpu(form, c)
    again, T2, pc2 = run_gpu(form, c)
    for name, t in list(got.items()) + ([("pc", pc)] if pc is not None else []):
        assert not bool(torch.isnan(t).any()), (tag, K, form, name, "NaN left")
    assert float(T[..., K:].abs().sum()) == 0.0, (tag, K, form, "pad frames")
    for name in got:
        assert torch.equal(got[name], again[name]), (tag, K, form, name, "second call differs")
    assert pc is None or torch.equal(pc, pc2), (tag, K, form, "pc: second call differs")
    if form == "bwd_gln2":
        assert torch.equal(got.pop("_amax"), T.abs().flatten(1).amax(1)), (tag, K, form, "amax_out")
    ref = DO.run_form(form, c.i)
    assert set(ref) == set(got)
    errs = {}
    for name, r in ref.items():
        cls, how = DO.OUTPUTS[(form, name)]
        g = got[name][..., :K] if got[name] is T else got[name]
        errs[name] = e = DO.rel_err(g, r, how)
        kind = "%s %s" % (cls, name)
        if e > WORST.get(kind, (-1.0,))[0]:
            WORST[kind] = (e, DO.LIMIT[cls], tag, K, form)
    print("DW %-2s K=%-4d %-9s " % (tag, K, form) + " ".join("%s=%.2e" % kv for kv in errs.items()))
    for name, e in errs.items():
        assert e < DO.LIMIT[DO.OUTPUTS[(form, name)][0]], (tag, K, form, name, e)
    return got


CASES = [(tag, K) for tag in DO.CONFIGS for K in DO.fwd_Ks(tag)]


@pytest.mark.parametrize("tag,K", CASES, ids=["%s-%d" % c for c in CASES])
def test_forms_at_the_seams(tag, K):
    """Forward forms at every frame count of the configuration; backward forms at all but the two forward-seam counts."""
    c = Case(DO.make_inputs(*DO.CONFIGS[tag], K))
    for form in DO.FWD_FORMS + (DO.BWD_FORMS if K in DO.bwd_Ks(tag) else ()):
        check_form(tag, form, c)


def test_prelu_at_exactly_zero():
    """h1 and d are 0.0 at known positions (a first and a last valid frame among them): the kernels' slope there is 1, as the
    oracle's.  "set" overwrites single elements of d; "taps" zeroes a channel's taps, which keeps d the depthwise conv of the
    first norm's output, as the identities behind ctn_dw_bwd_gln2's sums need: there the stand-alone chain ctn_dw_bwd(fused = 1) +
    ctn_gln_prelu_bwd must give the dY1 (and dalpha1) of ctn_dw_bwd_gln2."""
    for mode in ("set", "taps"):
        i = DO.make_inputs(*DO.CONFIGS["B"], 203, zeros=mode)
        assert i.h1[0, 0, 0] == 0 and i.h1[1, -1, -1] == 0 and int((i.Dz_g == 0).sum()) >= 6 and int((i.Dz_c == 0).sum()) >= 6
        assert bool((i.Dz_g[..., 0] == 0).any() and (i.Dz_g[..., -1] == 0).any())
        c = Case(i)
        got = {form: check_form("B0" + mode[0], form, c) for form in DO.BWD_FORMS}
    M, H, K, Kp = i.M, i.H, i.K, c.Kp
    dY, dap = nan(M, H, Kp), nan(M * H)
    ctn.lib.call("ctn_gln_prelu_bwd", ptr(got["bwd_gln"]["dN1"]), ptr(c.h1), ptr(dY), M, H, K, Kp, ptr(c.g1), ptr(c.a1), ptr(c.ms1),
                 ptr(got["bwd_gln"]["sums1_part"]), H, ptr(dap), 0, 0)
    e = DO.rel_err(dY, got["bwd_gln2"]["dY1"], "utt")
    e1 = DO.rel_err(dap.sum().reshape(1), got["bwd_gln2"]["dalpha1"], "all")
    print("DW B0t K=%d chain-vs-gln2 dY1=%.2e dalpha1=%.2e" % (K, e, e1))
    assert e < 2e-5 and e1 < 1e-4


@pytest.mark.parametrize("tag,seed", [("A", 17), ("I", 17)])
def test_tracked_maximum_ignores_dead_waves(tag, seed):
    """K = 1 with inputs at which rstd1 |S1'| / n, the value that ctn_dw_bwd_gln2's first-norm backward makes of a dead wave's
    all-zero row, is several times max |dY1[m]| (the oracle says so below): amax_out must still be the maximum of dY1."""
    i = DO.make_inputs(*DO.CONFIGS[tag], 1, seed)
    s8, n = DO.parts3(i.rows8).sum(1), i.H
    c1p = i.ms2[1] * (s8[:, 2] - s8[:, 0] / n * s8[:, 3] - s8[:, 1] / n * s8[:, 4]) / n
    ratio = (i.ms1[1] * c1p).abs() / DO.run_form("bwd_gln2", i)["dY1"].abs().flatten(1).amax(1)
    assert float(ratio.max()) > 3
    check_form(tag + "d", "bwd_gln2", Case(i))


def test_finalize_kernels_over_several_workgroups():
    """(P + 4) H = 840 and P H = 560 outputs: four and three workgroups of 256 with a ragged last one, against fp64 sums of the
    pc that the test wrote."""
    H, P, M = 70, 8, 3
    pc = torch.randn(P + 6, M, H, generator=torch.Generator().manual_seed(5)) + 0.5
    pcd, s = pc.to(DEV), pc.double().sum(1)                   # [F, H]
    ref = dict(dD=s[:P].t(), dgamma2=s[P], dbeta2=s[P + 1], dgamma1=s[P + 2], dbeta1=s[P + 3], dalpha2=s[P + 4].sum().reshape(1),
               dalpha1=s[P + 5].sum().reshape(1))
    v = {n: nan(*r.shape) for n, r in ref.items()}
    ctn.lib.call("ctn_dw_bwd_finalize", ptr(pcd), P, M, H, ptr(v["dD"]), ptr(v["dgamma2"]), ptr(v["dbeta2"]), ptr(v["dgamma1"]),
                 ptr(v["dbeta1"]), ptr(v["dalpha2"]), ptr(pcd[P + 5]), M * H, ptr(v["dalpha1"]), 0)
    refc = dict(dD=ref["dD"], dgamma2=ref["dgamma2"], dbeta2=ref["dbeta2"], dalpha2=s[P + 2].sum().reshape(1))
    vc = {n: nan(*r.shape) for n, r in refc.items()}
    ctn.lib.call("ctn_dw_bwd_cln_finalize", ptr(pcd), P, M, H, ptr(vc["dD"]), ptr(vc["dgamma2"]), ptr(vc["dbeta2"]), ptr(vc["dalpha2"]), 0)
    dD = nan(H, P)
    ctn.lib.call("ctn_dw_bwd_taps", ptr(pcd), P, M, H, ptr(dD), 0)
    torch.cuda.synchronize()
    errs = {}
    for pre, vv, rr in (("", v, ref), ("cln ", vc, refc), ("taps ", {"dD": dD}, {"dD": ref["dD"]})):
        for n, r in rr.items():
            assert not bool(torch.isnan(vv[n]).any()), pre + n
            errs[pre + n] = DO.rel_err(vv[n], r, "all")
    print("DW finalize H=70 P=8 M=3 " + " ".join("%s=%.2e" % kv for kv in errs.items()))
    for n, e in errs.items():
        assert e < (1e-4 if "dalpha" in n else 2e-5), (n, e)


def _refused(name, args, outs):
    lib = ctn.lib.load()
    rc = getattr(lib, name)(*args)
    msg = lib.ctn_last_error().decode()
    torch.cuda.synchronize()
    assert rc != 0, (name, "accepted")
    assert name in msg, (name, msg)
    for t in outs:
        assert bool(torch.isnan(t).all()), (name, "an output was written")


@pytest.mark.parametrize("what", ["odd_halo", "P9", "P0", "Kp_mod4", "Kp_lt_K", "halo_too_large", "missing_norm"])
def test_refusals(what):
    """Invalid arguments come back as a status and a message that names the entry point, before anything is launched."""
    M, H, K, Kp, P, dil, causal, fused = 2, 6, 70, 128, 3, 1, 0, 0
    g = torch.Generator().manual_seed(7)

    def rows(fill):
        """[M, H, 128] at the head of a buffer that would also hold the widest layout a refused call names."""
        flat = torch.full((M * H * 192,), fill, dtype=F32, device=DEV)
        return flat, flat[:M * H * 128].view(M, H, 128)

    (_, y), (_, dz), (Zf, Z), (dYf, dY) = rows(0.0), rows(0.0), rows(NAN), rows(NAN)
    y[..., :K], dz[..., :K] = torch.randn(M, H, K, generator=g).to(DEV), torch.randn(M, H, K, generator=g).to(DEV)
    Dflat = dev(torch.randn(H * 9, generator=g))            # [H, 3] at its head; room for the [H, 9] that P = 9 names
    pc, s1 = nan(16, M, H), nan(M, H, 2, dtype=F64)
    vec, ms, one, s2 = dev(torch.ones(H)), dev(torch.tensor([[0.0, 1.0]] * M)), scalar(0.25), dev(torch.ones(M, 1, 2), dtype=F64)
    ms1 = ms
    if what == "odd_halo":
        P, dil = 2, 3
    elif what == "P9":
        P = 9
    elif what == "P0":
        P = 0
    elif what == "Kp_mod4":
        Kp = 130
    elif what == "Kp_lt_K":
        Kp = 64
    elif what == "halo_too_large":
        dil = 1024
    elif what == "missing_norm":
        fused, ms1 = 1, None
    dims = (M, H, K, Kp, P, dil, causal)
    fwd = (ptr(y), ptr(Z), ptr(Dflat), *dims, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    bwd = (ptr(dz), ptr(dz), ptr(y), ptr(dY), ptr(Dflat), *dims, fused, ptr(vec), ptr(vec), ptr(one), ptr(ms1), ptr(vec), ptr(one),
           ptr(ms), ptr(s2), 1, ptr(pc), ptr(s1), 0)
    if what == "halo_too_large":        # the forward patch still holds a halo of 2048, the backward one does not
        ctn.lib.call("ctn_dw_fwd", *fwd)
        torch.cuda.synchronize()
        ref = DO.fwd(y[..., :K].cpu().double(), Dflat[:H * 3].view(H, 3).cpu().double(), dil, False)["Z"]
        e = DO.rel_err(Z[..., :K], ref, "utt")
        print("DW P=3 dil=1024 K=70 fwd_plain Z=%.2e" % e)
        assert e < 3e-6 and float(Z[..., K:].abs().sum()) == 0.0
    elif what != "missing_norm":
        _refused("ctn_dw_fwd", fwd, [Zf])
    _refused("ctn_dw_bwd", bwd, [dYf, pc, s1])


def test_zz_largest_figures():
    """Prints the largest figure per kind of output over the cases that ran before it (for the table in the docstring)."""
    for kind, (e, lim, tag, K, form) in sorted(WORST.items()):
        note = "" if e * 4 >= lim else "  (more than 4x below)"
        print("DW MAX %-18s %.2e  limit %.0e  at %s K=%d %s%s" % (kind, e, lim, tag, K, form, note))
