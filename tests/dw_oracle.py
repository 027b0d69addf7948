"""Closed forms of the depthwise-conv kernels of csrc/ctn_dw.hip (dw_fwd_kernel / dw_bwd_kernel), in plain torch on the CPU.

The functions take what the C entry points take (include/ctn_hip.h: ctn_dw_fwd, ctn_dw_fwd_cln, ctn_dw_bwd, ctn_dw_bwd_gln2,
ctn_dw_bwd_cln), already rounded to fp32 where the kernel receives fp32, without the K..Kp pad frames, and evaluate the
documented mathematics in `dtype` (float64: the reference; float32: a model of what fp32 arithmetic can reach).

Shapes: tensors [M, H, K]; taps D [H, P]; per-channel gamma / beta [H]; PReLU slopes are Python floats; gLN statistics
(mean, rstd) [M]; cLN statistics [M, K].  PReLU follows the kernels: slope 1 at exactly 0 (x >= 0 ? x : a x).

The module also holds what tests/test_dw_oracle_cpu.py and tests/test_gpu_depthwise.py share: the mirror of the kernels' patch
constants (checked against the source by the CPU test), the configurations and frame counts at the kernels' seams, the inputs,
the list of (form, output) pairs with their limits, and the deliberately wrong models that the CPU test uses to show that the
limits can tell a defect from rounding.
"""
import contextlib
import functools
import types

import torch
import torch.nn.functional as F

F64 = torch.float64
EPS = 1e-8                    # CTN_EPS

# ---- mirror of csrc/ctn_dw.hip (test_dw_oracle_cpu.py::test_constants_match_the_source reads the source) ------------------
MAXP = 8
FWD_BUF_S, FWD_BUF_L = 1024, 3584
BWD_BUF_S, BWD_BUF_M, BWD_BUF_L = 768, 1280, 1792
FWD_SMALL_HALO = 192          # forward: halo <= 192 takes FWD_BUF_S
BWD_SMALL_HALO, BWD_MEDIUM_HALO = 128, 256


def seg_of(buf, halo):
    return ((buf - halo - 8) // 64) * 64


def pad_left(P, dil, causal):
    halo = (P - 1) * dil
    return halo if causal else halo // 2


def plan(P, dil, causal):
    """-> namespace(halo, padl, vec4, pt, fwd_buf, fwd_seg, bwd_buf, bwd_seg): the kernel variant that the launchers pick."""
    halo, padl = (P - 1) * dil, pad_left(P, dil, causal)
    fb = "S" if halo <= FWD_SMALL_HALO else "L"
    bb = "S" if halo <= BWD_SMALL_HALO else ("M" if halo <= BWD_MEDIUM_HALO else "L")
    return types.SimpleNamespace(
        halo=halo, padl=padl, vec4=dil % 4 == 0 and padl % 4 == 0, pt=3 if P == 3 else 0,
        fwd_buf=fb, fwd_seg=seg_of({"S": FWD_BUF_S, "L": FWD_BUF_L}[fb], halo),
        bwd_buf=bb, bwd_seg=seg_of({"S": BWD_BUF_S, "M": BWD_BUF_M, "L": BWD_BUF_L}[bb], halo))


# tag -> (P, dilation, causal).  Between them: both tap paths x both forward patches x all three backward patches x
# kernel size compiled in / at run time (P = 1, 2, 5, MAXP).
CONFIGS = {
    "A": (3, 1, False), "B": (3, 4, True), "C": (3, 80, False), "D": (3, 128, True), "E": (3, 256, False),
    "F": (5, 128, True), "G": (2, 3, True), "H": (8, 2, True), "I": (1, 4, False), "J": (3, 150, False),
    "Kc": (3, 99, True),
}
# what each configuration is there for: (halo, float4 path, fwd patch, fwd seg, bwd patch, bwd seg)
EXPECTED_PLAN = {
    "A": (2, False, "S", 960, "S", 704), "B": (8, True, "S", 960, "S", 704), "C": (160, True, "S", 832, "M", 1088),
    "D": (256, True, "L", 3264, "M", 960), "E": (512, True, "L", 3008, "L", 1216), "F": (512, True, "L", 3008, "L", 1216),
    "G": (3, False, "S", 960, "S", 704), "H": (14, False, "S", 960, "S", 704), "I": (0, True, "S", 960, "S", 704),
    "J": (300, False, "L", 3264, "L", 1472), "Kc": (198, False, "L", 3328, "M", 1024),
}
SHORT_TAGS = ("A", "E", "G", "J")
M_TEST, H_TEST = 2, 6         # the second workgroup of an utterance has two dead waves
ALPHA1, ALPHA2 = 0.2, 0.3


def long_K(tag):
    """Two segments in both directions and a ragged float4 tail."""
    p = plan(*CONFIGS[tag])
    K = max(p.fwd_seg, p.bwd_seg) + 67
    while K % 4 != 3:
        K += 1
    return K


def short_Ks(tag):
    P, dil, causal = CONFIGS[tag]
    return sorted({k for k in (1, 5, dil, (P - 1) * dil + 1) if k >= 1})


def bwd_Ks(tag):
    """Frame counts at which every form runs: the long K, a backward seam at the end of the data, a second backward segment
    with one valid frame, and (at SHORT_TAGS) utterances shorter than the receptive field."""
    p = plan(*CONFIGS[tag])
    ks = [long_K(tag), p.bwd_seg, p.bwd_seg + 1]
    if tag in SHORT_TAGS:
        ks += [k for k in short_Ks(tag) if k not in ks]
    return ks


def fwd_Ks(tag):
    p = plan(*CONFIGS[tag])
    ks = bwd_Ks(tag)
    return ks + [k for k in (p.fwd_seg, p.fwd_seg + 1) if k not in ks]


# ---- limits (the project's existing ones; see the docstring of tests/test_gpu_depthwise.py) ---------------------------------
LIMIT = {"plain": 3e-6, "fused": 2e-5, "scalar": 1e-4}
# (form, output) -> (limit class, how the error is taken: "utt" per utterance, "col" per utterance and last-axis column, "all")
OUTPUTS = {
    ("fwd_plain", "Z"): ("plain", "utt"),
    ("fwd_gln", "Z"): ("fused", "utt"), ("fwd_gln", "epi_part"): ("fused", "col"), ("fwd_gln", "ms_out"): ("fused", "col"),
    ("fwd_cln", "Z"): ("fused", "utt"),
    ("bwd_plain", "dY"): ("plain", "utt"), ("bwd_plain", "dD"): ("fused", "all"),
    ("bwd_gln", "dN1"): ("fused", "utt"), ("bwd_gln", "sums1_part"): ("fused", "col"),
    ("bwd_gln2", "dY1"): ("fused", "utt"), ("bwd_gln2", "dalpha1"): ("scalar", "all"),
    ("bwd_cln", "dN1"): ("fused", "utt"), ("bwd_cln_x", "dN1"): ("fused", "utt"),
}
for _f in ("bwd_gln", "bwd_gln2"):
    for _o in ("dD", "dgamma2", "dbeta2", "dgamma1", "dbeta1"):
        OUTPUTS[(_f, _o)] = ("fused", "all")
    OUTPUTS[(_f, "dalpha2")] = ("scalar", "all")
for _f in ("bwd_cln", "bwd_cln_x"):
    for _o in ("dD", "dgamma2", "dbeta2"):
        OUTPUTS[(_f, _o)] = ("fused", "all")
    OUTPUTS[(_f, "dalpha2")] = ("scalar", "all")
FWD_FORMS = ("fwd_plain", "fwd_gln", "fwd_cln")
BWD_FORMS = ("bwd_plain", "bwd_gln", "bwd_gln2", "bwd_cln", "bwd_cln_x")


def rel_err(got, ref, how):
    """The project's max |got - ref| / max |ref|; per utterance ("utt") or per utterance and column ("col") where the two
    utterances' scales differ, and the largest of those."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    if how == "all":
        return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))
    if how == "utt":
        d, r = (got - ref).abs().flatten(1).amax(1), ref.abs().flatten(1).amax(1)
    else:
        nc = ref.shape[-1]
        d = (got - ref).abs().reshape(ref.shape[0], -1, nc).amax(1)
        r = ref.abs().reshape(ref.shape[0], -1, nc).amax(1)
    return float((d / (r + 1e-30)).max())


# ---- deliberately wrong models (test_dw_oracle_cpu.py::test_limits_catch_defects) -------------------------------------------
_DEFECT = {}


@contextlib.contextmanager
def defect(**kw):
    """padl=1: pad_left off by one.  roll=1: row c reads the taps of row c+1.  xzero_fwd=seg / xzero_bwd=seg: the x image is
    zero from the second segment's first halo frame on (everything a frame k >= seg reads of x).  count=n: the element count of an
    utterance is n whatever the tensors' length (with_frame_K: 'frame K treated as valid')."""
    _DEFECT.update(kw)
    try:
        yield
    finally:
        _DEFECT.clear()


# ---- primitives ---------------------------------------------------------------------------------------------------------------
def prelu(x, a):
    return torch.where(x >= 0, x, a * x)


def dprelu(x, a):
    return torch.where(x >= 0, torch.ones_like(x), torch.full_like(x, a))


def _shift(x, off):
    """x[..., k + off] for k in [0, K), zeros outside [0, K)."""
    K, m = x.shape[-1], abs(off)
    return F.pad(x, (m, m))[..., off + m: off + m + K]


def _padl(P, dil, causal):
    return pad_left(P, dil, causal) + _DEFECT.get("padl", 0)


def _taps(D):
    return D.roll(-_DEFECT["roll"], 0) if "roll" in _DEFECT else D


def dw(n, D, dil, causal):
    """z[m,c,k] = sum_j D[c,j] n[m,c,k + j dil - pad_left], zeros outside [0, K)."""
    P, padl, T = D.shape[1], _padl(D.shape[1], dil, causal), _taps(D)
    z = torch.zeros_like(n)
    for j in range(P):
        z = z + T[:, j, None] * _shift(n, j * dil - padl)
    if "xzero_fwd" in _DEFECT:
        z[..., _DEFECT["xzero_fwd"]:] = 0
    return z


def dw_adjoint(dd, D, dil, causal):
    """dN1[m,c,k] = sum_j D[c,j] dd[m,c,k - j dil + pad_left]."""
    P, padl, T = D.shape[1], _padl(D.shape[1], dil, causal), _taps(D)
    out = torch.zeros_like(dd)
    for j in range(P):
        out = out + T[:, j, None] * _shift(dd, padl - j * dil)
    return out


def dw_taps(dd, x, P, dil, causal):
    """dD[c,j] = sum_{m,k} dd[m,c,k] x[m,c,k + j dil - pad_left]."""
    padl = _padl(P, dil, causal)
    if "xzero_bwd" in _DEFECT:
        dd = dd.clone()
        dd[..., _DEFECT["xzero_bwd"]:] = 0
    return torch.stack([(dd * _shift(x, j * dil - padl)).sum((0, 2)) for j in range(P)], 1)


def tap_count(D, dil, causal, K):
    """V[c,k] = sum of the taps of frame k that stay inside [0, K)   (ctn_pw_dgrad_gln2 in the header)."""
    return dw(torch.ones((1, D.shape[0], K), dtype=D.dtype), D, dil, causal)[0]


def row_sums(p):
    """[M, H, 2] per-row (sum p, sum p^2): what a statistics epilogue leaves (epi_part)."""
    return torch.stack([p.sum(2), (p * p).sum(2)], 2)


def gln_stats(part, n):
    """finalize_stats of ctn_common.h: (mean, rstd) [M] from [M, parts, 2] partials over n = H K elements."""
    s = part.double().sum(1)
    mu = s[:, 0] / n
    var = (s[:, 1] / n - mu * mu).clamp_min(0)
    return mu, 1.0 / torch.sqrt(var + EPS)


def cln_stats(p):
    """cln_stats_frame_kernel: per-frame (mean, rstd) [M, K] over the channels, biased variance."""
    Ch = p.shape[1]
    mu = p.sum(1) / Ch
    var = ((p * p).sum(1) / Ch - mu * mu).clamp_min(0)
    return mu, 1.0 / torch.sqrt(var + EPS)


def _ch(v):
    return v[None, :, None]


def _utt(v):
    return v[:, None, None]


def _frm(v):
    return v[:, None, :]


def _count(t):
    """n = H K, the element count of an utterance."""
    return _DEFECT.get("count", t.shape[1] * t.shape[2])


def _conv(dtype, *ts):
    return [t if t is None or isinstance(t, (int, float)) else t.to(dtype) for t in ts]


def _norm1(h1, gln=None, cln=None):
    """(xhat1, n1) of the first norm; gln = (mean [M], rstd [M], g, b, alpha), cln = (mean [M,K], rstd [M,K], g, b, alpha)."""
    if gln is not None:
        mean, rstd, g, b, al = gln
        xh = (prelu(h1, al) - _utt(mean)) * _utt(rstd)
    else:
        mean, rstd, g, b, al = cln
        xh = (prelu(h1, al) - _frm(mean)) * _frm(rstd)
    return xh, _ch(g) * xh + _ch(b)


# ---- forward ------------------------------------------------------------------------------------------------------------------
def fwd(y, D, dil, causal, gln=None, cln=None, epi_alpha=None, dtype=F64):
    """ctn_dw_fwd / ctn_dw_fwd_cln.  -> dict: Z; with epi_alpha also epi_part [M,H,2]; with gln also ms_out [M,2] (the
    statistics that the prologue used, which the kernel hands on)."""
    y, D = _conv(dtype, y, D)
    out = {}
    if gln is not None:
        gln = _conv(dtype, *gln)
        n = _norm1(y, gln=gln)[1]
        out["ms_out"] = torch.stack([gln[0], gln[1]], 1)
    elif cln is not None:
        n = _norm1(y, cln=_conv(dtype, *cln))[1]
    else:
        n = y
    out["Z"] = dw(n, D, dil, causal)
    if epi_alpha is not None:
        out["epi_part"] = row_sums(prelu(out["Z"], epi_alpha))
    return out


# ---- backward -----------------------------------------------------------------------------------------------------------------
def bwd_plain(dZ, X, D, dil, causal, dtype=F64):
    dZ, X, D = _conv(dtype, dZ, X, D)
    return {"dY": dw_adjoint(dZ, D, dil, causal), "dD": dw_taps(dZ, X, D.shape[1], dil, causal)}


def _second_gln(dN2, Dz, g2, a2, ms2, sums2):
    """dd, xhat2, da2 of the comment block above dw_bwd_kernel; ms2 = (mean2, rstd2) [M], sums2 [M,2] = (S1, S2)."""
    n = _count(Dz)
    c = (sums2.double() / n).to(Dz.dtype)             # (the kernels divide the fp64 sums in fp64 and round the quotient)
    xh2 = (prelu(Dz, a2) - _utt(ms2[0])) * _utt(ms2[1])
    da2 = _utt(ms2[1]) * (_ch(g2) * dN2 - _utt(c[:, 0]) - xh2 * _utt(c[:, 1]))
    return da2 * dprelu(Dz, a2), xh2, da2


def _second_sums(out, dN2, Dz, xh2, da2):
    out["dgamma2"] = (dN2 * xh2).sum((0, 2))
    out["dbeta2"] = dN2.sum((0, 2))
    out["dalpha2"] = torch.where(Dz < 0, da2 * Dz, torch.zeros_like(Dz)).sum().reshape(1)


def bwd_gln(dN2, Dz, h1, D, dil, causal, g1, b1, a1, ms1, g2, a2, ms2, sums2, dtype=F64, _dn1=False):
    """ctn_dw_bwd(fused = 1) + ctn_dw_bwd_finalize.  ms1 / ms2 = (mean, rstd) [M] each; sums2 [M,2] the per-utterance (S1, S2)."""
    dN2, Dz, h1, D, g1, b1, g2 = _conv(dtype, dN2, Dz, h1, D, g1, b1, g2)
    ms1, ms2 = _conv(dtype, *ms1), _conv(dtype, *ms2)
    dd, xh2, da2 = _second_gln(dN2, Dz, g2, a2, ms2, sums2)
    xh1, n1 = _norm1(h1, gln=(ms1[0], ms1[1], g1, b1, a1))
    dN1 = dw_adjoint(dd, D, dil, causal)
    out = {"dN1": dN1, "dD": dw_taps(dd, n1, D.shape[1], dil, causal)}
    _second_sums(out, dN2, Dz, xh2, da2)
    out["dgamma1"] = (dN1 * xh1).sum((0, 2))
    out["dbeta1"] = dN1.sum((0, 2))
    t = _ch(g1) * dN1
    out["sums1_part"] = torch.stack([t.sum(2), (t * xh1).sum(2)], 2)
    if _dn1:
        out["_xh1"] = xh1
    return out


def gln2_row_sums(dN2, Dz, D, dil, causal, g1, b1, g2, a2, ms2, dtype=F64):
    """The eight sums of ctn_pw_dgrad_gln2 from their definitions, per row: [M, H, 8]; an utterance's sums are .sum(1).
    (S1, S2, sum u t g1V, sum u g1V, sum u xh2 g1V, sum u t e, sum u e, sum u xh2 e)  with u = prelu'(d), t = gamma2 dN2,
    g1V = gamma1 V, e = d - beta1 V, V = tap_count."""
    dN2, Dz, D, g1, b1, g2 = _conv(dtype, dN2, Dz, D, g1, b1, g2)
    ms2 = _conv(dtype, *ms2)
    xh2 = (prelu(Dz, a2) - _utt(ms2[0])) * _utt(ms2[1])
    V = tap_count(D, dil, causal, Dz.shape[2])[None]
    u, t, gv, e = dprelu(Dz, a2), _ch(g2) * dN2, _ch(g1) * V, Dz - _ch(b1) * V
    return torch.stack([q.sum(2) for q in (t, t * xh2, u * t * gv, u * gv, u * xh2 * gv, u * t * e, u * e, u * xh2 * e)], 2)


def bwd_gln2(dN2, Dz, h1, D, dil, causal, g1, b1, a1, ms1, g2, a2, ms2, sums8, dtype=F64):
    """ctn_dw_bwd_gln2 + ctn_dw_bwd_finalize with dalpha1_part = row P+5.  sums8 [M,8]: the per-utterance eight sums."""
    sums8 = sums8.double()                            # fp64 partials, combined in fp64 as in the kernel; the quotients are rounded
    out = bwd_gln(dN2, Dz, h1, D, dil, causal, g1, b1, a1, ms1, g2, a2, ms2, sums8[:, :2], dtype=dtype, _dn1=True)
    h1, g1 = _conv(dtype, h1, g1)
    n = _count(h1)
    c1, c2, r1, r2 = sums8[:, 0] / n, sums8[:, 1] / n, ms1[1].to(dtype), ms2[1].double()
    c1p = (r2 * (sums8[:, 2] - c1 * sums8[:, 3] - c2 * sums8[:, 4]) / n).to(dtype)
    c2p = (r2 * (sums8[:, 5] - c1 * sums8[:, 6] - c2 * sums8[:, 7]) / n).to(dtype)
    xh1 = out.pop("_xh1")
    da1 = _utt(r1) * (_ch(g1) * out.pop("dN1") - _utt(c1p) - xh1 * _utt(c2p))
    out.pop("sums1_part")
    out["dY1"] = da1 * dprelu(h1, a1)
    out["dalpha1"] = torch.where(h1 < 0, da1 * h1, torch.zeros_like(h1)).sum().reshape(1)
    return out


def cln_fc(dN2, Dz, g2, a2, mean2, rstd2, dtype=F64):
    """fc [M][4][K] = (rstd2, mean2 rstd2, rstd2 S1 / H, rstd2 S2 / H)[k] with S1[k] = sum_c gamma2 dN2, S2[k] = sum_c gamma2
    dN2 xhat2 (ctn_cln_bwd_frame)."""
    dN2, Dz, g2, mean2, rstd2 = _conv(dtype, dN2, Dz, g2, mean2, rstd2)
    H = Dz.shape[1]
    xh2 = (prelu(Dz, a2) - _frm(mean2)) * _frm(rstd2)
    t = _ch(g2) * dN2
    return torch.stack([rstd2, mean2 * rstd2, rstd2 * t.sum(1) / H, rstd2 * (t * xh2).sum(1) / H], 1)


def bwd_cln(dN2, Dz, X1, D, dil, causal, g2, a2, fc, first=None, dtype=F64):
    """ctn_dw_bwd_cln + ctn_dw_bwd_cln_finalize.  first = None: X1 is the first norm's output as stored; first = (g1, b1, a1,
    mean1 [M,K], rstd1 [M,K]): X1 is h1 and the first norm is recomputed."""
    dN2, Dz, X1, D, g2, fc = _conv(dtype, dN2, Dz, X1, D, g2, fc)
    f0, f1, f2, f3 = (_frm(fc[:, q]) for q in range(4))
    xh2 = prelu(Dz, a2) * f0 - f1
    da2 = _ch(g2) * f0 * dN2 - f2 - xh2 * f3
    dd = da2 * dprelu(Dz, a2)
    if first is not None:
        g1, b1, a1, mean1, rstd1 = _conv(dtype, *first)
        X1 = _norm1(X1, cln=(mean1, rstd1, g1, b1, a1))[1]
    out = {"dN1": dw_adjoint(dd, D, dil, causal), "dD": dw_taps(dd, X1, D.shape[1], dil, causal)}
    _second_sums(out, dN2, Dz, xh2, da2)
    return out


# ---- the inputs of tests/test_gpu_depthwise.py ----------------------------------------------------------------------------------
def r32(t):
    return t.float().double()


@functools.lru_cache(maxsize=8)
def make_inputs(P, dil, causal, K, seed=0, M=M_TEST, H=H_TEST, zeros=False):
    """Everything the entry points receive for one case, as fp64 tensors that hold fp32 values (fp64 partial sums stay fp64),
    without pad frames.  The statistics, sums and per-frame constants that the kernels are handed are computed here in fp64
    from their definitions and then rounded like the buffers that carry them.  Treat the result as read-only (it is cached).

    zeros: elements of h1 and of the depthwise outputs (Dz) are exactly 0.0 at known positions, a first and a last valid
    frame among them, where the kernels' PReLU slope is 1.  "set": single elements of Dz are overwritten (Dz is then no longer
    the depthwise conv of the first norm's output, which the identities behind ctn_pw_dgrad_gln2's sums assume: for comparing
    a form with its closed form only).  "taps": the taps of channel 2 are 0, so its whole row of Dz is 0 and still consistent."""
    gen = torch.Generator().manual_seed(1000 + seed)

    def rn(*s):
        return torch.randn(*s, generator=gen, dtype=F64)

    i = types.SimpleNamespace(P=P, dil=dil, causal=causal, K=K, M=M, H=H, a1=ALPHA1, a2=ALPHA2)
    h1 = 1.5 * rn(M, H, K) + 0.2
    h1[1:] *= 0.05                      # the second utterance's statistics differ from the first's
    i.D, i.g1, i.b1, i.g2, i.b2 = r32(rn(H, P)), r32(1.0 + 0.3 * rn(H)), r32(0.3 * rn(H)), r32(1.0 + 0.3 * rn(H)), r32(0.3 * rn(H))
    noise = rn(M, H, K)
    zpos = [(0, 0, 0), (1, H - 1, K - 1), (0, 2, K // 2), (1, 1, 0), (0, H - 1, K - 1), (1, 3, K // 3)]
    if zeros:
        for p in zpos:
            h1[p] = 0.0
    if zeros == "taps":
        i.D[2] = 0.0
    i.h1 = h1 = r32(h1)
    n = H * K
    # gLN chain
    i.part1 = row_sums(prelu(h1, i.a1))                                     # [M,H,2] fp64
    i.ms1 = tuple(r32(v) for v in gln_stats(i.part1, n))
    n1 = _norm1(h1, gln=(*i.ms1, i.g1, i.b1, i.a1))[1]
    Dz = dw(n1, i.D, dil, causal)
    if zeros == "set":
        for p in zpos[::-1]:
            Dz[p[0], (p[1] + 1) % H, p[2]] = 0.0
    i.Dz_g = Dz = r32(Dz)
    # the upstream gradient leans on d: with pure noise the two slope gradients (sums over the negative side of products whose
    # mean is 0) would be the small remainder of a cancellation, and their relative error a matter of luck
    i.dN2 = r32(noise + Dz)
    i.part2 = row_sums(prelu(Dz, i.a2))
    i.ms2 = tuple(r32(v) for v in gln_stats(i.part2, n))
    i.rows8 = gln2_row_sums(i.dN2, Dz, i.D, dil, causal, i.g1, i.b1, i.g2, i.a2, i.ms2)     # [M,H,8] fp64
    # cLN chain
    i.st1 = tuple(r32(v) for v in cln_stats(prelu(h1, i.a1)))
    n1c = _norm1(h1, cln=(*i.st1, i.g1, i.b1, i.a1))[1]
    i.X1_c = r32(n1c)
    Dz = dw(n1c, i.D, dil, causal)
    if zeros == "set":
        for p in zpos[::-1]:
            Dz[p[0], (p[1] + 1) % H, p[2]] = 0.0
    i.Dz_c = Dz = r32(Dz)
    i.dN2_c = r32(noise + Dz)
    i.st2 = tuple(r32(v) for v in cln_stats(prelu(Dz, i.a2)))
    i.fc = r32(cln_fc(i.dN2_c, Dz, i.g2, i.a2, *i.st2))
    return i


def parts3(rows):
    """[M, H, q] per-row sums -> [M, 3, q]: an utterance's partials split over three parts (channel groups)."""
    H = rows.shape[1]
    e = [0, (H + 2) // 3, (2 * H + 2) // 3, H]
    return torch.stack([rows[:, e[q]:e[q + 1]].sum(1) for q in range(3)], 1)


def run_form(form, i, dtype=F64):
    """One form of the oracle on make_inputs()' case -> {output name: tensor}."""
    a = (i.D, i.dil, i.causal)
    if form == "fwd_plain":
        return fwd(i.h1, *a, dtype=dtype)
    if form == "fwd_gln":
        return fwd(i.h1, *a, gln=(*i.ms1, i.g1, i.b1, i.a1), epi_alpha=i.a2, dtype=dtype)
    if form == "fwd_cln":
        return fwd(i.h1, *a, cln=(*i.st1, i.g1, i.b1, i.a1), dtype=dtype)
    if form == "bwd_plain":
        return bwd_plain(i.dN2, i.h1, *a, dtype=dtype)
    norms = (i.g1, i.b1, i.a1, i.ms1, i.g2, i.a2, i.ms2)
    if form == "bwd_gln":
        return bwd_gln(i.dN2, i.Dz_g, i.h1, *a, *norms, parts3(i.rows8[..., :2]).sum(1), dtype=dtype)
    if form == "bwd_gln2":
        return bwd_gln2(i.dN2, i.Dz_g, i.h1, *a, *norms, parts3(i.rows8).sum(1), dtype=dtype)
    if form == "bwd_cln":
        return bwd_cln(i.dN2_c, i.Dz_c, i.X1_c, *a, i.g2, i.a2, i.fc, dtype=dtype)
    if form == "bwd_cln_x":
        return bwd_cln(i.dN2_c, i.Dz_c, i.h1, *a, i.g2, i.a2, i.fc, first=(i.g1, i.b1, i.a1, *i.st1), dtype=dtype)
    raise KeyError(form)


def with_frame_K(form, i):
    """The wrong model 'frame K treated as valid': the case with one more frame whose inputs are the zero pad frame (per-frame
    statistics and constants of the pad: 0), the per-utterance statistics, sums and element count unchanged; outputs cut to K."""
    j = types.SimpleNamespace(**vars(i))
    for name in ("h1", "dN2", "dN2_c", "Dz_g", "Dz_c", "X1_c", "fc"):
        setattr(j, name, F.pad(getattr(i, name), (0, 1)))
    j.st1 = tuple(F.pad(v, (0, 1)) for v in i.st1)
    with defect(count=i.H * i.K):
        out = run_form(form, j)
    return {k: (v[..., :i.K] if v.dim() == 3 and v.shape[-1] == i.K + 1 else v) for k, v in out.items()}
