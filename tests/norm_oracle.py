"""Closed forms of the channel-wise LayerNorm and BatchNorm entry points (csrc/ctn_cln.hip: ctn_cln_fwd, ctn_cln_bwd,
ctn_cln_bwd_finalize; csrc/ctn_bn.hip: ctn_bn_fwd, ctn_bn_bwd), in plain torch on the CPU.

The functions take what the entry points take, already rounded to fp32 where the kernels receive fp32, WITH the K..Kp pad frames
(tensors are [M, Ch, Kp]), and evaluate the documented mathematics in `dtype` (float64: the reference; float32: a model of what
fp32 arithmetic can reach -- two-pass variance as in the kernels, torch's own summation order).  Every sum comes back with the sum
of its terms' absolute values under "<name>|abs" (the denominator of the limit on sums) and its per-element terms under
"<name>|terms".  PReLU follows the kernels: slope 1 at exactly 0 (v >= 0 ? v : a v).

The module also holds what tests/test_cln_oracle_cpu.py and tests/test_gpu_norm_forms.py share: the mirror of the dispatch of
ctn_cln_fwd / ctn_cln_bwd (checked against the source by the CPU test), the case tables at the dispatch seams, the inputs, the
limits, and the deliberately wrong models that the CPU test uses to show that the limits can tell a defect from rounding.
"""
import collections
import contextlib
import functools
import types

import torch
import torch.nn.functional as F

from dw_oracle import dprelu, prelu, r32, rel_err  # noqa: F401  (shared, not copied)

F64 = torch.float64
EPS = 1e-8                      # CTN_EPS
BN_EPS, BN_MOMENTUM = 1e-5, 0.1  # nn.BatchNorm1d's defaults, which the model passes
ALPHA = 0.25
PAD_FILL = 1e30                 # pad frames of dOut / add / relu_ref (cLN) and of Y / dOut (BatchNorm): see make_inputs()
RSTD_PAD = 1.0 / EPS ** 0.5     # what a zero pad frame's statistics are: mean 0, rstd 1 / sqrt(eps)

# ---- mirror of the dispatch in csrc/ctn_cln.hip (test_cln_oracle_cpu.py::test_mirror_matches_the_source reads the source) ------
C4_NT, C4_FR, C4_NG = 512, 32, 64          # v4: 64 channel groups; 16-frame form: 256 threads
CLN_NT, CLN_FR = 1024, 32                  # register-resident forward: 32 channel groups of 32 frames
V4_MAX_CH = 8 * C4_NG                      # cln_v4_ok
V4_CPT = (1, 2, 4, 8)                      # channels per thread of the v4 kernels: the first that holds cdiv(Ch, C4_NG)
FWD_REG_CPT = (2, 4, 8, 16, 32)            # cln_fwd_reg_kernel: the first that holds cdiv(Ch, CLN_NT / CLN_FR); above: generic
BWD_REG = ((32, 2, 512), (64, 4, 512), (128, 8, 512), (256, 16, 512), (512, 16, 1024))   # (Ch <=, CPT, NTB) of cln_bwd_dx_reg_kernel
DEFAULT_FR, DEFAULT_LEAN = 16, 1


def cdiv(a, b):
    return -(-a // b)


def padded(K):
    return cdiv(K, 64) * 64               # ctn_padded_frames


def v4_ok(Ch, Kp, aligned):
    return Ch <= V4_MAX_CH and Kp % C4_FR == 0 and aligned


def plan_fwd(Ch, Kp, aligned=True, fr=DEFAULT_FR):
    """The kernel that ctn_cln_fwd launches.  aligned: Y, Out, mean and rstd are all 16-byte aligned."""
    if v4_ok(Ch, Kp, aligned):
        return "v4/CPT%d/fr%d" % (next(c for c in V4_CPT if cdiv(Ch, C4_NG) <= c), fr)
    cpt = cdiv(Ch, CLN_NT // CLN_FR)
    return next(("reg/CPT%d" % c for c in FWD_REG_CPT if cpt <= c), "generic")


def plan_bwd(Ch, Kp, aligned=True, fr=DEFAULT_FR, lean=DEFAULT_LEAN, alpha=True, add=False, relu_ref=False):
    """The input-gradient kernel that ctn_cln_bwd launches.  aligned: dY, and add / relu_ref where given, are 16-byte aligned
    (dOut, Y, mean and rstd must be).  Every label but "v4/..." and "lean" also runs cln_bwd_params_kernel."""
    if v4_ok(Ch, Kp, aligned) and Kp % fr == 0:
        if lean and Ch == V4_MAX_CH and fr == 16 and alpha and not add and not relu_ref:
            return "lean"
        return "v4/CPT%d/fr%d" % (next(c for c in V4_CPT if Ch <= c * C4_NG), fr)
    return next(("dxreg/%dx%d" % (cpt, ntb) for lim, cpt, ntb in BWD_REG if Ch <= lim), "generic")


def bwd_blocks(M, Kp, fr=DEFAULT_FR):
    return M * cdiv(Kp, fr)               # ctn_cln_bwd_blocks


FWD_LABELS = {fr: ["v4/CPT%d/fr%d" % (c, fr) for c in V4_CPT] + ["reg/CPT%d" % c for c in FWD_REG_CPT] + ["generic"] for fr in (16, 32)}
BWD_LABELS = {fr: ["v4/CPT%d/fr%d" % (c, fr) for c in V4_CPT] + (["lean"] if fr == 16 else [])
              + ["dxreg/%dx%d" % (c, n) for _, c, n in BWD_REG] + ["generic"] for fr in (16, 32)}

# ---- the case tables ----------------------------------------------------------------------------------------------------------------
# mis: which pointer is one float off a 16-byte boundary (None: all aligned).  prelu: alpha given.  mode: "plain", "add" (an added
# gradient) or "mask" (add AND relu_ref).  seed: see CHECKED_SEEDS.
FwdCase = collections.namedtuple("FwdCase", "Ch K Kp M mis prelu seed")
BwdCase = collections.namedtuple("BwdCase", "Ch K Kp M mis prelu mode seed")
MODES = ("plain", "add", "mask")
V4_WIDTHS = (3, 64, 65, 128, 129, 256, 257, 511, 512)                # either side of the CPT steps at 64, 128, 256
BWD_FALLBACK_WIDTHS = (3, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513)
FWD_FALLBACK_WIDTHS = (64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025)
# v4 frames: every width runs K = 1, K = Kp = 64, K = 65 (64 valid frames' worth of workgroups, then whole workgroups of pad frames)
# and two of the other frame counts in turn; 15, 17, 61 and 130 end inside a frame quad
V4_K_FIXED, V4_K_TURN = (1, 64, 65), ((15, 16), (17, 130), (61, 15), (130, 17), (16, 61))
# fallback through Kp % 32 != 0: the last block is ragged for the 32-frame (register-resident) and 64-frame (generic) kernels
FALLBACK_FRAMES = ((37, 40), (97, 100), (68, 68))
# fallback through alignment, where v4 would otherwise run
ALIGN_FRAMES = ((61, 64), (128, 128))
# Narrow layers are badly conditioned (a frame's few values nearly equal: the normalised value is the remainder of a cancellation).
# Ch = 3 runs on a seed checked by test_cln_oracle_cpu.py::test_limits_are_reachable_in_fp32: with make_inputs()' offset, seeds 0 .. 7
# all stay below 0.1x of every limit in fp32 torch, seed 3 at 0.024x.  The limits are untouched.
CHECKED_SEEDS = {3: 3}


def _seed(Ch):
    return CHECKED_SEEDS.get(Ch, 0)


def _v4_frames(j):
    return V4_K_FIXED + V4_K_TURN[j % len(V4_K_TURN)]


def fwd_cases():
    """Every case of the forward: PReLU and none alternate (a run-time branch of every kernel: each label sees both)."""
    out, n = [], 0
    for j, Ch in enumerate(V4_WIDTHS):
        for K in _v4_frames(j):
            out.append(FwdCase(Ch, K, padded(K), 2, None, n % 2 == 0, _seed(Ch)))
            n += 1
    out.append(FwdCase(129, 61, 64, 3, None, True, 0))         # 12 workgroups of 16 frames: xcd_remap on a grid that is no multiple of 8
    out.append(FwdCase(65, 17, 64, 1, None, False, 0))         # 4 workgroups
    for Ch in (3,) + FWD_FALLBACK_WIDTHS:
        for K, Kp in FALLBACK_FRAMES + ((37, 37),):            # (37, 37): rows not 16-byte aligned
            out.append(FwdCase(Ch, K, Kp, 2, None, n % 2 == 0, _seed(Ch)))
            n += 1
        for K, Kp in ALIGN_FRAMES:
            if Ch <= V4_MAX_CH:
                out.append(FwdCase(Ch, K, Kp, 2, "mean", n % 2 == 0, _seed(Ch)))
                n += 1
    return out


def bwd_cases():
    """Every case of the backward.  {PReLU, none} x {plain, add, add + relu_ref} are run-time branches inside each kernel (alpha_p,
    add, relu_ref != nullptr; no kernel is selected by them but "lean"), so a (width, frames) pair runs two of the six in turn:
    (PReLU, MODES[n]) and (none, MODES[n + 1]); test_cln_oracle_cpu.py checks that every label still sees all six, and "lean" its one."""
    out, n = [], 0

    def two(Ch, K, Kp, M, mis):
        nonlocal n
        modes = ("add", "mask") if mis == "add" else MODES
        out.append(BwdCase(Ch, K, Kp, M, mis, True, modes[n % len(modes)], _seed(Ch)))
        out.append(BwdCase(Ch, K, Kp, M, mis, False, modes[(n + 1) % len(modes)], _seed(Ch)))
        n += 1

    for j, Ch in enumerate(V4_WIDTHS):
        for K in _v4_frames(j):
            two(Ch, K, padded(K), 2, None)
    for K in (1, 61, 64, 130):                                 # the LEAN form, and with cln_lean 0 the general CPT 8 form on the same input
        out.append(BwdCase(512, K, padded(K), 2, None, True, "plain", 0))
    two(129, 61, 64, 3, None)
    two(65, 17, 64, 1, None)
    for Ch in BWD_FALLBACK_WIDTHS:
        for K, Kp in FALLBACK_FRAMES:
            two(Ch, K, Kp, 2, None)
        if Ch <= V4_MAX_CH:
            for K, Kp in ALIGN_FRAMES:
                two(Ch, K, Kp, 2, "dY")
                two(Ch, K, Kp, 2, "add")
    return list(dict.fromkeys(out))


def fwd_label(c, fr=DEFAULT_FR):
    return plan_fwd(c.Ch, c.Kp, c.mis is None, fr)


def bwd_label(c, fr=DEFAULT_FR, lean=DEFAULT_LEAN):
    return plan_bwd(c.Ch, c.Kp, c.mis is None, fr, lean, c.prelu, c.mode != "plain", c.mode == "mask")


# ctn_cln_bwd_finalize alone: (M, Kp) -> rows 28 (all tail), 32 (the unrolled loop exactly), 36 (loop + tail), 320 (> 256 dalpha partials)
FINALIZE_SHAPES = ((7, 64), (2, 256), (3, 192), (5, 1024))
FINALIZE_WIDTHS = (1, 64, 65)

# BatchNorm: Ch 1, 7 (a ragged 4-row workgroup), 257 (a finalize over two workgroups); K 255 / 257: a second trip of the 256-frame
# lane loop, with a ragged quad; (M, K) = (1, 1): n = 1
BN_WIDTHS, BN_FRAMES, BN_MS = (1, 7, 257), (1, 3, 64, 255, 257), (1, 2)
BN_STATS = ("train", "train_norun", "eval")

# ---- limits (the project's existing ones; see the docstring of tests/test_gpu_norm_forms.py) ---------------------------------
LIMIT = {"out": 2e-5, "mean": 2e-5, "rstd": 2e-5, "dY": 5e-5, "dgamma": 5e-5, "dbeta": 5e-5, "sum": 1e-5,
         "bn_out": 1e-5, "bn_run": 1e-5, "bn_dY": 2e-5}


def sum_err(got, ref, mag):
    """max |got - ref| / (sum of the terms' absolute values)."""
    got, ref, mag = (t.detach().double().cpu().reshape(-1) for t in (got, ref, mag))
    return float(((got - ref).abs() / mag.clamp_min(1e-300)).max())


def cln_errors(got, ref, K):
    """{figure name: (error, limit)} of whatever of out / mean / rstd / dY / dgamma / dbeta / dalpha `got` holds, over the valid frames."""
    e = {}
    for n in ("out", "mean", "rstd", "dY"):
        if n in got:
            e[n] = (rel_err(got[n][..., :K], ref[n][..., :K], "utt"), LIMIT[n])
    for n in ("dgamma", "dbeta"):
        if n in got:
            e[n] = (rel_err(got[n], ref[n], "all"), LIMIT[n])
    for n in ("dgamma", "dbeta", "dalpha"):
        if n in got and got[n] is not None:
            e[n + " sum"] = (sum_err(got[n], ref[n], ref[n + "|abs"]), LIMIT["sum"])
    return e


def bn_errors(got, ref, K):
    e = {}
    for n, lim in (("out", "bn_out"), ("dY", "bn_dY"), ("running_mean", "bn_run"), ("running_var", "bn_run")):
        if n in got and got[n] is not None:
            g, r = (got[n][..., :K], ref[n][..., :K]) if n in ("out", "dY") else (got[n], ref[n])
            e[n] = (rel_err(g, r, "all"), LIMIT[lim])
    for n in ("dgamma", "dbeta", "dalpha"):
        if n in got and got[n] is not None:
            e[n + " sum"] = (sum_err(got[n], ref[n], ref[n + "|abs"]), LIMIT["sum"])
    return e


# ---- deliberately wrong models (test_cln_oracle_cpu.py::test_limits_catch_defects) ---------------------------------------------
_DEFECT = {}
DEFECTS = ("mean_padded", "frame_k", "drop_channel", "add_after_mask", "prelu_zero", "dbeta_kp", "bn_biased", "bn_frame_k")


@contextlib.contextmanager
def defect(name):
    """mean_padded: the mean divided by the channel count padded to whole groups of 64.  frame_k: frame K treated as valid.
    drop_channel: the last channel missing from the per-frame sums.  add_after_mask: `add` added after the ReLU mask's zero, not
    before.  prelu_zero: the PReLU slope applied at y == 0.  dbeta_kp: dbeta summed over all Kp frames.  bn_biased: the running
    variance updated with the biased variance.  bn_frame_k: BatchNorm's moments count frame K."""
    assert name in DEFECTS
    _DEFECT[name] = True
    try:
        yield
    finally:
        _DEFECT.clear()


# ---- primitives ----------------------------------------------------------------------------------------------------------------
def _ch(v):
    return v[None, :, None]


def _frm(v):
    return v[:, None, :]


def _c(dtype, *ts):
    return [t if t is None else t.to(dtype) for t in ts]


def _act(Y, alpha):
    return Y if alpha is None else prelu(Y, alpha)


def _slope(Y, alpha):
    if alpha is None:
        return torch.ones_like(Y)
    if "prelu_zero" in _DEFECT:
        return torch.where(Y > 0, torch.ones_like(Y), torch.full_like(Y, alpha))
    return dprelu(Y, alpha)


def _frames(t, K, extra=0):
    """[Kp] bool: the valid frames."""
    return torch.arange(t.shape[-1]) < K + extra


def _sel(ok, t):
    """t on the frames `ok`, 0 elsewhere -- a select as in the kernels, so that what the pad frames hold (1e30) never enters."""
    return torch.where(ok, t, torch.zeros_like(t))


def _sum3(out, name, terms, dims=(0, 2)):
    out[name], out[name + "|abs"], out[name + "|terms"] = terms.sum(dims), terms.abs().sum(dims), terms


# ---- channel-wise LayerNorm ------------------------------------------------------------------------------------------------------
def cln_fwd(Y, K, gamma, beta, alpha=None, dtype=F64):
    """ctn_cln_fwd -> {out [M,Ch,Kp] (0 on the frames >= K), mean, rstd [M,Kp] (every frame of Kp: the statistics of what Y holds
    there)}; alpha: a Python float or None."""
    Y, gamma, beta = _c(dtype, Y, gamma, beta)
    Ch = Y.shape[1]
    p = _act(Y, alpha)
    s = p[:, :-1].sum(1) if "drop_channel" in _DEFECT and Ch > 1 else p.sum(1)
    mu = s / (cdiv(Ch, C4_NG) * C4_NG if "mean_padded" in _DEFECT else Ch)
    d = p - _frm(mu)
    d2 = d * d
    var = (d2[:, :-1].sum(1) if "drop_channel" in _DEFECT and Ch > 1 else d2.sum(1)) / Ch
    rstd = 1.0 / torch.sqrt(var + EPS)
    out = _ch(gamma) * (d * _frm(rstd)) + _ch(beta)
    return {"out": _sel(_frames(Y, K, int("frame_k" in _DEFECT)), out), "mean": mu, "rstd": rstd}


def cln_bwd(dOut, Y, mean, rstd, K, gamma, alpha=None, add=None, relu_ref=None, dtype=F64):
    """ctn_cln_bwd + ctn_cln_bwd_finalize -> {dY [M,Ch,Kp], dgamma, dbeta [Ch], dalpha [1] (with alpha)} and per sum "|abs" and
    "|terms".  mean, rstd [M,Kp]: what the forward saved.
        t = gamma dOut,  xh = (prelu(Y) - mean) rstd,  da = rstd (t - mean_c t - xh mean_c (t xh))
        dY = [da prelu'(Y) + add] (relu_ref > 0),   dgamma = sum dOut xh,  dbeta = sum dOut,  dalpha = sum_{Y < 0} da Y
    over the frames < K; the ReLU mask does not enter dalpha (the PReLU sits behind the ReLU)."""
    dOut, Y, mean, rstd, gamma, add, relu_ref = _c(dtype, dOut, Y, mean, rstd, gamma, add, relu_ref)
    Ch = Y.shape[1]
    ok = _frames(Y, K, int("frame_k" in _DEFECT))
    xh = (_act(Y, alpha) - _frm(mean)) * _frm(rstd)
    d = _sel(ok, dOut)
    t = _ch(gamma) * d
    tx = t * xh
    if "drop_channel" in _DEFECT and Ch > 1:
        m1, m2 = t[:, :-1].sum(1) / Ch, tx[:, :-1].sum(1) / Ch
    else:
        m1, m2 = t.sum(1) / Ch, tx.sum(1) / Ch
    da = _frm(rstd) * (t - _frm(m1) - xh * _frm(m2))
    r = da * _slope(Y, alpha)
    if add is not None and "add_after_mask" not in _DEFECT:
        r = r + _sel(ok, add)
    if relu_ref is not None:
        r = torch.where(relu_ref > 0, r, torch.zeros_like(r))
    if add is not None and "add_after_mask" in _DEFECT:
        r = r + _sel(ok, add)
    out = {"dY": _sel(ok, r)}
    _sum3(out, "dgamma", d * xh)
    _sum3(out, "dbeta", dOut.clamp(-1e30, 1e30) if "dbeta_kp" in _DEFECT else d)
    if alpha is not None:
        _sum3(out, "dalpha", _sel(ok, torch.where(Y < 0, da * Y, torch.zeros_like(Y))), dims=(0, 1, 2))
        for n in ("dalpha", "dalpha|abs"):
            out[n] = out[n].reshape(1)
    return out


def ch2_dy_bound(dOut, mean, rstd, gamma):
    """Ch = 2: xh = (s, -s) with s^2 = 1 - eps rstd^2, so da = +-(t0 - t1) / 2 * eps rstd^3 exactly, t = gamma dOut -- about 1e-8 |t|
    on a well-separated frame.  What fp32 leaves is the rounding of  rstd (t - m1 - xh m2)  in units of u = 2^-24 rstd max |t|: the
    computed xh is off by up to (3 + |mean| rstd) u-fractions (the rounded mean against the separation 1 / rstd, the difference, the
    rounded rstd, the product) and enters twice (m2 is a mean of t xh), and t, m1, m2, xh m2, the two differences and the last
    product round once each: (13 + 2 |mean| rstd) u to first order, taken twice over (a worst case of independent roundings leaves no
    room for the 4x that the CPU test asks of fp32 torch: that uses 0.2 .. 0.33 of the single count; a wrong kernel is off by rstd |t|,
    1e6 times the slack).  -> (exact, slack) [M, Kp] each: |da| <= exact + slack (and so |dY| without `add`,
    for a slope <= 1); test_cln_oracle_cpu.py: fp32 torch stays within exact + slack / 4."""
    t, mean, rstd = _ch(gamma.double()) * dOut.double().clamp(-1e30, 1e30), mean.double(), rstd.double()
    return (t[:, 0] - t[:, 1]).abs() / 2 * EPS * rstd ** 3, 2 * (13 + 2 * mean.abs() * rstd) * 2.0 ** -24 * rstd * t.abs().amax(1)


# ---- BatchNorm -------------------------------------------------------------------------------------------------------------------
def bn_fwd(Y, K, gamma, beta, alpha=None, running=None, training=True, eps=BN_EPS, momentum=BN_MOMENTUM, dtype=F64):
    """ctn_bn_fwd -> {out, mr [Ch,2] = (mean, 1 / sqrt(var + eps)) used, running_mean, running_var (the updated ones; None without)}.
    Training: statistics over the n = M K valid elements of a channel, biased variance; the running variance takes var n / (n - 1),
    and var itself at n = 1 (the kernel's definition: torch refuses n = 1)."""
    Y, gamma, beta = _c(dtype, Y, gamma, beta)
    rm, rv = (None, None) if running is None else _c(dtype, *running)
    ok = _frames(Y, K, int("bn_frame_k" in _DEFECT))
    p = _act(_sel(ok, Y), alpha)
    n = Y.shape[0] * K
    if training:
        mu = p.sum((0, 2)) / n
        var = _sel(ok, (p - _ch(mu)) ** 2).sum((0, 2)) / n
        if rm is not None:
            unb = var if n == 1 or "bn_biased" in _DEFECT else var * n / (n - 1)
            rm, rv = (1 - momentum) * rm + momentum * mu, (1 - momentum) * rv + momentum * unb
    else:
        mu, var = rm, rv
    rstd = 1.0 / torch.sqrt(var + eps)
    out = (p - _ch(mu)) * _ch(rstd * gamma) + _ch(beta)
    return {"out": _sel(_frames(Y, K), out), "mr": torch.stack([mu, rstd], 1), "running_mean": rm, "running_var": rv}


def bn_bwd(dOut, Y, mr, K, gamma, alpha=None, training=True, dtype=F64):
    """ctn_bn_bwd -> {dY, dgamma, dbeta [Ch], dalpha [1] (with alpha)} (+ "|abs", "|terms").  Eval: the statistics are constants."""
    dOut, Y, mr, gamma = _c(dtype, dOut, Y, mr, gamma)
    ok = _frames(Y, K)
    Ys = _sel(ok, Y)
    n = Y.shape[0] * K
    xh = (_act(Ys, alpha) - _ch(mr[:, 0])) * _ch(mr[:, 1])
    d = _sel(ok, dOut)
    out = {}
    _sum3(out, "dgamma", _sel(ok, d * xh))
    _sum3(out, "dbeta", d)
    c1, c2 = (out["dbeta"] / n, out["dgamma"] / n) if training else (torch.zeros_like(gamma), torch.zeros_like(gamma))
    dp = _ch(gamma * mr[:, 1]) * (d - _ch(c1) - xh * _ch(c2))
    out["dY"] = _sel(ok, dp * _slope(Ys, alpha))
    if alpha is not None:
        _sum3(out, "dalpha", _sel(ok, torch.where(Ys < 0, dp * Ys, torch.zeros_like(Ys))), dims=(0, 1, 2))
        for k in ("dalpha", "dalpha|abs"):
            out[k] = out[k].reshape(1)
    return out


# ---- the inputs ------------------------------------------------------------------------------------------------------------------
UTT_SCALE = (1.0, 0.05, 0.3)          # the second utterance is 20 times quieter


def _nz(v):
    """Every element at least 0.1 away from 0 (the betas: a pad frame that passes through a norm shows up as a beta-sized error)."""
    return v + 0.1 * torch.where(v >= 0, 1.0, -1.0).to(v.dtype)


@functools.lru_cache(maxsize=None)
def make_inputs(Ch, K, Kp, M=2, seed=0, zeros=1):
    """Everything ctn_cln_fwd / ctn_cln_bwd receive for one case, as fp64 tensors that hold fp32 values.  Read-only (cached).

    Y [M,Ch,Kp]: exact zeros in the pad frames (the kernels compute the pad frames' statistics from what is there, and the v4
    backward multiplies their xh by a zero gradient), and at `zeros` valid positions per 64 (1: a handful).  dOut, add, relu_ref:
    1e30 in the pad frames, which no kernel may let into a result.  relu_ref holds zeros and negatives.  stats[prelu] = (mean, rstd)
    [M,Kp]: the fp64 forward's, rounded to fp32 -- what the backward is handed."""
    gen = torch.Generator().manual_seed(9000 + 131 * seed + Ch)

    def rn(*s):
        return torch.randn(*s, generator=gen, dtype=F64)

    scale = torch.tensor(UTT_SCALE[:M], dtype=F64).view(M, 1, 1)

    def utt(t):
        return t * scale

    def pad(t, fill=0.0):
        return F.pad(r32(t), (0, Kp - K), value=fill)

    i = types.SimpleNamespace(Ch=Ch, K=K, Kp=Kp, M=M, alpha=ALPHA)
    Y = utt(1.5 * rn(M, Ch, K) + 0.5)        # (an offset: a frame's mean over the channels is then no pure cancellation)
    if zeros == 1:
        for p in ((0, 0, 0), (M - 1, Ch - 1, K - 1), (0, Ch // 2, K // 2), (M - 1, Ch // 3, 0)):
            if Ch >= 16 or (Ch > 2 and K >= 4):         # (two zeros in a frame of three channels leave the third's gradient exactly 0)
                Y[p] = 0.0
    elif zeros:
        Y[torch.rand(M, Ch, K, generator=gen) < zeros] = 0.0
    i.Y = pad(Y)
    i.dOut = pad(rn(M, Ch, K) + 0.3, PAD_FILL)
    i.gamma, i.beta = r32(1.0 + 0.3 * rn(Ch)), r32(_nz(0.3 * rn(Ch)))
    i.add = pad(0.5 * rn(M, Ch, K) / scale, PAD_FILL)          # of the size of the norm's own input gradient (rstd ~ 1 / scale)
    rr = rn(M, Ch, K)
    rr[rr.abs() < 0.2] = 0.0
    i.relu_ref = pad(rr, PAD_FILL)
    i.stats = {}
    for pre in (False, True):
        f = cln_fwd(i.Y, K, i.gamma, i.beta, ALPHA if pre else None)
        i.stats[pre] = (r32(f["mean"]), r32(f["rstd"]))
    return i


@functools.lru_cache(maxsize=None)
def make_ch2_inputs(K, Kp, M=2):
    """Ch = 2 on a well-separated input: the two channels of a frame differ by 1 .. 3 times the utterance's scale, so the normalised
    value is +-1 to 1e-8 and the exact input gradient about 1e-8 |gamma dOut| (ch2_dy_bound)."""
    i = types.SimpleNamespace(**vars(make_inputs(2, K, Kp, M, zeros=0)))
    gen = torch.Generator().manual_seed(9100 + K)
    base = torch.randn(M, 1, K, generator=gen, dtype=F64)
    sep = (0.5 + torch.rand(M, 1, K, generator=gen, dtype=F64)) * torch.where(torch.rand(M, 1, K, generator=gen) < 0.5, -1.0, 1.0)
    Y = torch.cat([base + sep, base - sep], 1) * torch.tensor(UTT_SCALE[:M], dtype=F64).view(M, 1, 1)
    i.Y = F.pad(r32(Y), (0, Kp - K))
    i.stats = {}
    for pre in (False, True):
        f = cln_fwd(i.Y, K, i.gamma, i.beta, ALPHA if pre else None)
        i.stats[pre] = (r32(f["mean"]), r32(f["rstd"]))
    return i


def solo(i, m):
    """The case that holds utterance m alone (M = 1)."""
    j = types.SimpleNamespace(**vars(i))
    j.M = 1
    for name in ("Y", "dOut", "add", "relu_ref"):
        setattr(j, name, getattr(i, name)[m:m + 1])
    j.stats = {k: (v[0][m:m + 1], v[1][m:m + 1]) for k, v in i.stats.items()}
    return j


def run_fwd(i, pre, dtype=F64):
    return cln_fwd(i.Y, i.K, i.gamma, i.beta, i.alpha if pre else None, dtype=dtype)


def run_bwd(i, pre, mode, dtype=F64):
    return cln_bwd(i.dOut, i.Y, *i.stats[pre], i.K, i.gamma, i.alpha if pre else None, i.add if mode != "plain" else None,
                   i.relu_ref if mode == "mask" else None, dtype=dtype)


@functools.lru_cache(maxsize=None)
def make_bn_inputs(Ch, K, M, seed=0):
    """ctn_bn_fwd / ctn_bn_bwd: Y, dOut [M,Ch,Kp] with 1e30 in the pad frames (every BatchNorm kernel selects on k < K), the running
    statistics before the call, and mr [stats][prelu] = the fp64 forward's (mean, rstd), rounded to fp32."""
    gen = torch.Generator().manual_seed(9500 + 17 * seed + Ch + 1000 * M)
    Kp = padded(K)

    def rn(*s):
        return torch.randn(*s, generator=gen, dtype=F64)

    i = types.SimpleNamespace(Ch=Ch, K=K, Kp=Kp, M=M, alpha=ALPHA)
    Y = 1.7 * rn(M, Ch, K) + 0.3
    Y[1:] *= 0.05
    if 2 <= M * K <= 3:
        # two or three elements per channel: xhat is +-1 and the input gradient the remainder of a cancellation unless the variance is
        # of the size of eps (test_cln_oracle_cpu.py: fp32 reaches 0.5x of the dY limit at the scale of the other cases): scaled down
        Y *= 0.003
    Y[0, 0, 0] = 0.0
    i.Y, i.dOut = (F.pad(r32(t), (0, Kp - K), value=PAD_FILL) for t in (Y, rn(M, Ch, K) + 0.3))
    i.gamma, i.beta = r32(1.0 + 0.3 * rn(Ch)), r32(_nz(0.3 * rn(Ch)))
    # (a running mean of the batch mean's sign: at Ch = 1 the updated value is otherwise, on some seeds, the remainder of a cancellation)
    i.running = (r32(0.2 + 0.1 * rn(Ch)), r32(0.5 + torch.rand(Ch, generator=gen, dtype=F64)))
    i.mr = {(st, pre): r32(run_bn_fwd(i, st, pre)["mr"]) for st in BN_STATS for pre in (False, True)}
    return i


def run_bn_fwd(i, stats, pre, dtype=F64):
    return bn_fwd(i.Y, i.K, i.gamma, i.beta, i.alpha if pre else None, None if stats == "train_norun" else i.running, stats != "eval",
                  dtype=dtype)


def run_bn_bwd(i, stats, pre, dtype=F64):
    return bn_bwd(i.dOut, i.Y, i.mr[(stats, pre)], i.K, i.gamma, i.alpha if pre else None, stats != "eval", dtype=dtype)


def bn_cases():
    return [(Ch, K, M, st, pre) for Ch in BN_WIDTHS for K in BN_FRAMES for M in BN_MS for st in BN_STATS for pre in (True, False)]
