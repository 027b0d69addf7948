"""Closed forms of what the 1x1-conv GEMM entry points leave (csrc/ctn_gemm.hip, ctn_gemm_common.h, ctn_gemm_b3.h; include/ctn_hip.h:
ctn_pw_gemm, ctn_pw_dgrad_gln, ctn_pw_dgrad_gln2, ctn_pw_gemm_cln, ctn_pw_dgrad_cln, ctn_pw_wgrad and their h3 forms), in plain torch
on the CPU.

The functions take what the entry points take, already rounded to fp32 where the kernels receive fp32, WITH the K..Kp pad frames
(tensors are [M, rows, Kp]), and evaluate the documented mathematics in `dtype` (float64: the reference; float32: a model of what
fp32 arithmetic can reach).  Every GEMM is written on its effective operand A [R, Cn], Out[m] = A . f(X[m]); how A is stored
(trans_w 0 / 1, b6 or h3 pieces) is the caller's business.  Statistics come back the way the kernels leave them: per output tile
(part index ct * tiles_r + rt, the shared epilogue's) or per row tile and frame, each with the sum of its terms' absolute values
under "<name>|abs" -- the denominator of the limit on every sum.

The module also holds what tests/test_gemm_oracle_cpu.py and tests/test_gpu_gemm_seams.py share: the mirror of the tile tables
(checked against the sources by the CPU test), the shapes at the tiles' seams, the inputs, the limits, and the deliberately wrong
models that the CPU test uses to show that the limits can tell a defect from rounding.
"""
import contextlib
import functools
import types

import torch
import torch.nn.functional as F

import dw_oracle as DO
from dw_oracle import cln_stats, dprelu, gln2_row_sums, gln_stats, parts3, prelu, tap_count  # noqa: F401  (shared, not copied)

F64 = torch.float64
EPS = DO.EPS
M_TEST = 2
A_EPI, A_PRO = 0.2, 0.3         # slope of the PReLU behind a GEMM (K1, cLN forward; the norm of B1 / B1' / cLN backward uses A_PRO on y)
PAD_FILL = 1e30                 # pad frames of the prologue operand: pro_apply promises 0 for k >= K whatever is stored there

# ---- mirror of the tile tables (test_gemm_oracle_cpu.py::test_tile_tables_match_the_sources reads the sources) ---------------
TK, XK, WK = 16, 32, 16                                               # k-tile: fp32 forward, split forward / weight gradient, fp32 weight gradient
FP32_TILES = ((128, 128), (128, 64), (64, 128), (64, 64))             # tile_dims(), id by ctn_tune("pw_tile")
B3_TILES = ((128, 128), (128, 64), (256, 64), (256, 64))              # ctn_b3_tile_dims(), id by ctn_tune("b3_tile" / "b3_tile_k3")
WG_B3_TILE = 128                                                      # BM = BN of the split weight-gradient kernel
TUNE_DEFAULTS = {"pw_tile": -1, "b3_tile": 1, "b3_tile_k3": 3, "wgrad_blocks": 512, "b3_wgrad_blocks": 256}
DEFAULT_TILE = {"fp32": 3, "split": 1}


def cdiv(a, b):
    return -(-a // b)


def padded(K):
    return cdiv(K, 64) * 64


def tile_of(family, tile):
    return (FP32_TILES if family == "fp32" else B3_TILES)[tile]


def family_of(arith, R):
    """The kernel family of the plain entry points: layers with fewer than 64 rows always run the fp32-MFMA kernels."""
    return "fp32" if arith == "fp32" or R < 64 else "split"


def k3_tile_applies(R):
    """ctn_b3_pick_tile: the residual-on-pieces form at 128 < R <= 256 takes ctn_tune("b3_tile_k3")."""
    return 128 < R <= 256


def n_parts(R, Kp, tm, tn):
    return cdiv(R, tm) * cdiv(Kp, tn)


def wgrad_plan(split, M, R, Cn, Kp, blocks):
    """wgrad_plan / ctn_b3_wgrad_plan -> (output tile, chunk, chunks_per_m)."""
    wt = WG_B3_TILE if split else (64 if R >= 64 and Cn >= 64 else 128)
    cpm = max(1, min(cdiv(blocks, cdiv(R, wt) * cdiv(Cn, wt) * M), cdiv(Kp, 256)))
    kt = XK if split else WK
    chunk = cdiv(cdiv(Kp, cpm), kt) * kt
    return wt, chunk, cdiv(Kp, chunk)


def wgrad_split(arith, R, Cn):
    return arith != "fp32" and R >= 32 and Cn >= 32


# ---- the seams: the smallest shapes that reach them ------------------------------------------------------------------------------
K_ALL = (1, 61, 64, 65, 130, 191)                  # Kp 64, 64, 64, 128, 192, 192; K % 4 = 1, 1, 0, 1, 2, 3
K_EXTRA = (61, 65, 191, 61)                        # by tile id: with 130, 64 and 1 every K above appears over the ids of a form


def shapes(family, tile):
    """(R, Cn, K) of one (family, tile id): rows overhanging the tile with a ragged contraction at K = 130; everything exact at
    K = 64; K = 1; and one more K.  fp32: the two last shapes have R = 20, which runs the fp32 family under every arithmetic."""
    tm = tile_of(family, tile)[0]
    if family == "fp32":
        return [(132 if tm == 128 else 68, (20, 36, 4, 20)[tile], 130), (64, 64, 64), (20, 4, 1), (20, (36, 20, 64, 36)[tile], K_EXTRA[tile])]
    return [(260 if tm == 256 else 132, (20, 36, 4, 36)[tile], 130), (64, 64, 64), (68, 4, 1), ((260, 68, 68, 132)[tile], (36, 20, 64, 20)[tile], K_EXTRA[tile])]


def k3_shapes(tile):
    """The residual-on-pieces form in the range of ctn_tune("b3_tile_k3")."""
    return [(132, 20, 130), (132, 64, 64), (132, 4, 1), (132, 36, K_EXTRA[tile])]


GEOMS = ((3, 1, False), (3, 64, True), (3, 80, False), (8, 2, True), (1, 4, False), (2, 3, True))    # (P, dilation, causal) of ctn_pw_dgrad_gln2
GEOM_KS = (64, 65, 200, 5)
GEOM_SHAPE = (68, 20)                              # (R, Cn) of the geometry cases
GEOM_KS_WIDE, GEOM_WIDE_TILE = (200, 65), (128, 128)    # also under the 128-column tile id 0 of both families
# weight gradients: (R, Cn) x (Kp, K, intended chunks_per_m)
WGRAD_SHAPES = ((64, 64), (132, 20), (68, 36), (200, 132))
WGRAD_PLANS = ((64, 1, 1), (320, 257, 2), (832, 800, 3), (832, 769, 4))


def wgrad_blocks(split, R, Cn, cpm, M=M_TEST):
    """The ctn_tune("wgrad_blocks" | "b3_wgrad_blocks") value that asks for `cpm` chunks per utterance."""
    wt = WG_B3_TILE if split else (64 if R >= 64 and Cn >= 64 else 128)
    return cpm * cdiv(R, wt) * cdiv(Cn, wt) * M


# ---- limits (the project's existing ones; see the docstring of tests/test_gpu_gemm_seams.py) ---------------------------------
LIMIT = {"plain": 3e-6, "pro": 5e-6, "cln": 2e-5, "ms": 2e-6, "sum": 1e-5, "h3": 6e-7}
# output name -> limit class of the plain entry points (Out / dN / dW: by form, below)
OUT_CLASS = {"ms_out": "ms", "mean": "cln", "rstd": "cln", "fc": "cln", "part": "sum", "col": "sum"}
PRO_FORMS = ("pro", "k3", "wgrad_pro")


def limit_class(form, name):
    if name in OUT_CLASS:
        return OUT_CLASS[name]
    return "pro" if form in PRO_FORMS or form == "wgrad" else "plain"


def err_of(cls, got, ref, mag=None, K=None):
    """The figure that LIMIT[cls] bounds.  plain / pro: max |got - ref| / max |ref| per utterance over all Kp frames (dW: over the
    matrix); cln (mean, rstd [M, Kp], fc [M, 4, Kp]): the same over the frames < K, per utterance and row of fc (the pad frames
    hold constants, rstd's 1e4 among them: pad_constants()); ms: the largest relative error; sum and h3: max |got - ref| / mag,
    mag = the sum of the terms' absolute values (sum |a||b|)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    if cls in ("sum", "h3"):
        return float(((got - ref).abs() / mag.double().cpu().clamp_min(1e-300)).max())
    if cls == "ms":
        return float(((got - ref).abs() / ref.abs().clamp_min(1e-300)).max())
    if cls == "cln":
        return DO.rel_err(got[..., :K].reshape(-1, K), ref[..., :K].reshape(-1, K), "utt")
    if ref.dim() == 2 and ref.shape[0] != M_TEST:          # dW
        return DO.rel_err(got, ref, "all")
    return DO.rel_err(got, ref, "utt")


# ---- deliberately wrong models (test_gemm_oracle_cpu.py::test_limits_catch_defects) --------------------------------------------
_DEFECT = {}
DEFECTS = ("ghost_rows", "pro_pad", "v_kp", "v_left", "no_ok", "col_add", "w_t", "drop_chunk")


@contextlib.contextmanager
def defect(name):
    """ghost_rows: statistics count the rows >= R of the last row tile with the values a trans_w = 1 tile holds there (the next
    contraction row's).  pro_pad: the prologue's output is not zeroed for k >= K.  v_kp: V clipped to [0, Kp) instead of [0, K).
    v_left: V not clipped at the left edge.  no_ok: frames >= K counted in sums 4 and 7 of the eight.  col_add: the column partials
    of the second row tile are added to the first.  w_t: the weight used transposed (square shapes).  drop_chunk: the weight
    gradient drops its last chunk."""
    assert name in DEFECTS
    _DEFECT[name] = True
    try:
        yield
    finally:
        _DEFECT.clear()


# ---- primitives ----------------------------------------------------------------------------------------------------------------
def _ch(v):
    return v[None, :, None]


def _utt(v):
    return v[:, None, None]


def _frm(v):
    return v[:, None, :]


def _c(dtype, *ts):
    return [t.to(dtype) for t in ts]


def _valid(t, K):
    """t with its frames >= K zeroed."""
    t = t.clone()
    t[..., K:] = 0
    return t


def gemm(A, X):
    if "w_t" in _DEFECT and A.shape[0] == A.shape[1]:
        A = A.t()
    return torch.einsum("rc,mck->mrk", A, X)


def dot_mag(A, X, add=None):
    """sum |a||b| (+ |residual|): the scale of the h3 limit."""
    s = torch.einsum("rc,mck->mrk", A.abs(), X.abs())
    return s if add is None else s + add.abs()


def pro_stats(X, K, alpha, parts=3):
    """(pro_part [M, parts, 2] fp64, mean [M], rstd [M]) of the operand prologue's norm over the Cn K valid elements."""
    rows = DO.row_sums(prelu(X[..., :K].double(), alpha))
    part = parts3(rows) if parts == 3 else rows.sum(1, keepdim=True)
    mu, rs = gln_stats(part, X.shape[1] * K)
    return part, DO.r32(mu), DO.r32(rs)


def pro_apply(X, K, g, b, alpha, mean, rstd):
    """f(x)[i,k] = gamma[i] ((prelu(x, alpha) - mean_m) rstd_m) + beta[i] for k < K, 0 otherwise."""
    f = _ch(g) * ((prelu(X, alpha) - _utt(mean)) * _utt(rstd)) + _ch(b)
    return f if "pro_pad" in _DEFECT else _valid(f, K)


def tile_parts(terms, K, tm, tn):
    """[q][M, R, Kp] per-element terms -> [M, parts, q]: the sums over each output tile's rows < R and frames < K."""
    t = torch.stack([_valid(x, K) for x in terms], -1)
    M, R, Kp, q = t.shape
    tr, tc = cdiv(R, tm), cdiv(Kp, tn)
    out = t.new_zeros(M, tr * tc, q)
    for ct in range(tc):
        for rt in range(tr):
            out[:, ct * tr + rt] = t[:, rt * tm:(rt + 1) * tm, ct * tn:(ct + 1) * tn].sum((1, 2))
    return out


def col_parts(terms, tm):
    """[q][M, R, Kp] -> [M, row tiles, Kp, q]: per frame, the sums over each row tile's rows < R."""
    t = torch.stack(terms, -1)
    out = torch.stack([t[:, r0:r0 + tm].sum(1) for r0 in range(0, t.shape[1], tm)], 1)
    if "col_add" in _DEFECT and out.shape[1] > 1:
        out[:, 0] += out[:, 1]
    return out


def _with_abs(out, name, fn, terms, *a):
    out[name] = fn(terms, *a)
    out[name + "|abs"] = fn([x.abs() for x in terms], *a)


def _ghost(A, X, tm):
    """What the rows R .. tiles_r tm - 1 of a trans_w = 1 tile hold: the stored [Cn, R] matrix read past the end of its row,
    i.e. element (c, R + j) is element (c + 1, j); past the matrix: 0."""
    R, Cn = A.shape
    n = cdiv(R, tm) * tm - R
    flat = F.pad(A.t().contiguous().flatten(), (0, R + n))
    idx = torch.arange(Cn)[None, :] * R + R + torch.arange(n)[:, None]
    return torch.einsum("rc,mck->mrk", flat[idx], X)


def _stat_rows(A, X, out, tm):
    """The rows whose PReLU statistics are counted: Out's, and under the ghost_rows defect the last row tile's overhang too."""
    return torch.cat([out, _ghost(A, X, tm)], 1) if "ghost_rows" in _DEFECT and A.shape[0] % tm else out


def _V(D, dil, causal, K, Kp):
    """V [R, Kp]: the sum of the taps of frame k whose source frame lies in [0, K)   (frames >= K: what the epilogue computes there)."""
    P, padl = D.shape[1], DO.pad_left(D.shape[1], dil, causal)
    k = torch.arange(Kp)
    hi = Kp if "v_kp" in _DEFECT else K
    V = D.new_zeros(D.shape[0], Kp)
    for j in range(P):
        src = k + j * dil - padl
        ok = (src < hi) if "v_left" in _DEFECT else (src >= 0) & (src < hi)
        V = V + D[:, j, None] * ok.to(D.dtype)
    return V


def gln2_terms(dN, y, K, D, dil, causal, g1, b1, g2, a2, ms2):
    """The eight per-element terms of ctn_pw_dgrad_gln2 [M, R, Kp] (their row sums over k < K are dw_oracle.gln2_row_sums):
    (t, t xh2, u t g1V, u g1V, u xh2 g1V, u t e, u e, u xh2 e); the terms without t carry the `ok` mask of the frames < K."""
    Kp = y.shape[-1]
    xh2 = (prelu(y, a2) - _utt(ms2[0])) * _utt(ms2[1])
    V = _V(D, dil, causal, K, Kp)[None]
    ok = (torch.arange(Kp) < K).to(y.dtype)
    u = dprelu(y, a2) * ok
    t, gv, e = _ch(g2) * dN, _ch(g1) * V, y - _ch(b1) * V
    terms = [t, t * xh2, u * t * gv, u * gv, u * xh2 * gv, u * t * e, u * e, u * xh2 * e]
    if "no_ok" in _DEFECT:
        un = dprelu(y, a2)
        terms[3], terms[6] = un * gv, un * e
    return terms


# ---- the forms -------------------------------------------------------------------------------------------------------------------
FWD_FORMS = ("plain", "relu", "res", "k1", "pro", "k3", "b1", "gln2", "clnf", "clnb")


def run_form(form, i, tile=(64, 64), dtype=F64):
    """One form on make_inputs()' case -> {output: tensor} (+ "<sum>|abs", and "Out|dot" = sum |a||b| for the h3 limit).
    tile = (TM, TN) of the kernel that writes the statistics partials."""
    tm, tn = tile
    K = i.K
    A, X, G, res = _c(dtype, i.A, i.X, i.G, i.res)
    out = {}
    if form in ("plain", "relu", "res", "k1", "clnf"):
        o = gemm(A, X)
        out["Out|dot"] = dot_mag(A, X, res if form == "res" else None)
        if form == "relu":
            o = o.clamp_min(0)
        if form == "res":
            o = o + res
        out["Out"] = o
        if form in ("k1", "clnf"):
            p = prelu(_stat_rows(A, X, o, tm), A_EPI)
            if form == "k1":
                _with_abs(out, "part", tile_parts, [p, p * p], K, tm, tn)
            else:
                _with_abs(out, "col", col_parts, [p, p * p], tm)
                s = out["col"].double().sum(1)                      # ctn_cln_stats_frame: fp64 over the row tiles, every frame of Kp
                mu = s[..., 0] / i.R
                out["mean"], out["rstd"] = mu, 1.0 / torch.sqrt((s[..., 1] / i.R - mu * mu).clamp_min(0) + EPS)
    elif form in ("pro", "k3"):
        gp, bp, mean, rstd, Xp = _c(dtype, i.gp, i.bp, i.pro_mean, i.pro_rstd, i.Xp)
        f = pro_apply(Xp, K, gp, bp, A_PRO, mean, rstd)
        out["Out"] = gemm(A, f) + (res if form == "k3" else 0)
        out["Out|dot"] = dot_mag(A, _valid(f, K), res if form == "k3" else None)
        if form == "k3":
            out["ms_out"] = torch.stack([mean, rstd], 1)
    elif form in ("b1", "gln2", "clnb"):
        y, g2 = _c(dtype, i.y, i.g2)
        dN = gemm(A, G)
        out["Out"], out["Out|dot"] = dN, dot_mag(A, G)
        if form == "b1":
            ms2 = _c(dtype, *i.ms2)
            t = _ch(g2) * dN
            _with_abs(out, "part", tile_parts, [t, t * ((prelu(y, A_PRO) - _utt(ms2[0])) * _utt(ms2[1]))], K, tm, tn)
        elif form == "gln2":
            P, dil, causal = i.geom
            D, g1, b1 = _c(dtype, i.D, i.g1, i.b1)
            terms = gln2_terms(dN, y, K, D, dil, causal, g1, b1, g2, A_PRO, _c(dtype, *i.ms2))
            full = lambda ts, *a: tile_parts(ts, y.shape[-1], *a)  # noqa: E731  (the mask is in the terms: no_ok must show)
            _with_abs(out, "part", full, terms, tm, tn)
        else:
            mean, rstd = _c(dtype, i.cmean, i.crstd)
            t = _ch(g2) * dN
            _with_abs(out, "col", col_parts, [t, t * ((prelu(y, A_PRO) - _frm(mean)) * _frm(rstd))], tm)
            s = out["col"].double().sum(1)
            out["fc"] = torch.stack([rstd.double(), mean.double() * rstd.double(), rstd.double() * s[..., 0] / i.R,
                                     rstd.double() * s[..., 1] / i.R], 1)
    else:
        raise KeyError(form)
    return out


def run_wgrad(i, pro, dtype=F64, chunk=None):
    """ctn_pw_wgrad: dW [R, Cn] = sum_{m,k} G[m,r,k] f(X[m,c,k]); here the gradient operand is i.res [M, R, Kp] and f's operand
    i.Xp (pad frames 1e30) with the prologue, i.X without.  chunk: the plan's chunk, for the drop_chunk defect."""
    g, X = _c(dtype, i.res, i.Xp if pro else i.X)
    if pro:
        X = pro_apply(X, i.K, *_c(dtype, i.gp, i.bp), A_PRO, *_c(dtype, i.pro_mean, i.pro_rstd))
    if "drop_chunk" in _DEFECT:
        last = (cdiv(i.Kp, chunk) - 1) * chunk
        g, X = g[..., :last], X[..., :last]
    return {"dW": torch.einsum("mrk,mck->rc", g, X), "dW|dot": torch.einsum("mrk,mck->rc", g.abs(), _valid(X, i.K).abs()[..., :g.shape[-1]])}


# ---- the inputs ------------------------------------------------------------------------------------------------------------------
def _nz(v):
    """Every element at least 0.1 away from 0 (the betas: a pad frame that passes through a norm shows up as a beta-sized error)."""
    return v + 0.1 * torch.where(v >= 0, 1.0, -1.0).to(v.dtype)


@functools.lru_cache(maxsize=None)
def make_inputs(R, Cn, K, Kp=None, geom=GEOMS[0], seed=0, zeros=True, M=M_TEST):
    """Everything the entry points receive for one case, as fp64 tensors that hold fp32 values (fp64 partial sums stay fp64),
    Kp frames wide.  Treat the result as read-only (it is cached).

    A [R, Cn]: the effective weight operand; its second row is 0, so a whole row of Out is exactly 0.0 in the PReLU of K1 and of the
    cLN forward.  X [M, Cn, Kp]: activations, 0.0 at a few positions; Xp: the same with 1e30 in the pad frames (the prologue
    operand).  G [M, Cn, Kp]: the gradient operand of the input-gradient forms.  res [M, R, Kp]: the residual, and the gradient
    operand of the weight gradients.  y [M, R, Kp]: the input of the norm behind B1 / B1' / the cLN backward: the depthwise conv of
    gamma1 xhat1 + beta1 plus a share of dN (the eight sums are compared with their definitions, which hold for any y; the
    identities behind them need y to be that conv alone: test_gemm_oracle_cpu.py builds such a y); with `zeros` a few elements are 0.0.
    The second utterance is 20 times quieter.  Pad frames are exact zeros except Xp's."""
    Kp = padded(K) if Kp is None else Kp
    P, dil, causal = geom
    gen = torch.Generator().manual_seed(7000 + seed)

    def rn(*s):
        return torch.randn(*s, generator=gen, dtype=F64)

    def act(*s):
        t = 1.5 * rn(*s) + 0.2
        t[1:] *= 0.05
        return t

    def pad(t, fill=0.0):
        return F.pad(DO.r32(t), (0, Kp - K), value=fill)

    i = types.SimpleNamespace(R=R, Cn=Cn, K=K, Kp=Kp, M=M, geom=geom)
    A = (rn(R, Cn) + 0.5) / Cn ** 0.5             # (a mean: the per-frame sums over the rows of A . G are then no pure cancellation)
    A[1] = 0.0
    i.A = DO.r32(A)
    X = act(M, Cn, K)
    if zeros:
        for p in ((0, 0, 0), (1, Cn - 1, K - 1), (0, Cn // 2, K // 2), (1, 1, 0)):
            X[p] = 0.0
    i.X, i.Xp = pad(X), pad(X, PAD_FILL)
    i.G = pad(act(M, Cn, K) + 0.4)
    i.res = pad(act(M, R, K))
    i.gp, i.bp = DO.r32(1.0 + 0.3 * rn(Cn)), DO.r32(_nz(0.3 * rn(Cn)))
    i.pro_part, i.pro_mean, i.pro_rstd = pro_stats(i.X, K, A_PRO)
    # the norm behind the input-gradient forms
    i.g1, i.b1, i.g2, i.b2 = DO.r32(1.0 + 0.3 * rn(R)), DO.r32(_nz(0.3 * rn(R))), DO.r32(1.0 + 0.3 * rn(R)), DO.r32(_nz(0.3 * rn(R)))
    i.D = DO.r32(rn(R, P))
    i.h1 = DO.r32(act(M, R, K))
    i.ms1 = tuple(DO.r32(v) for v in gln_stats(DO.row_sums(prelu(i.h1, A_EPI)), R * K))
    n1 = _ch(i.g1) * ((prelu(i.h1, A_EPI) - _utt(i.ms1[0])) * _utt(i.ms1[1])) + _ch(i.b1)
    # y leans on dN = A . G: with an independent y the sums of dN xhat (per utterance, and per frame at K = 1 a single number) would
    # be the small remainder of a cancellation, and their relative error a matter of luck
    dN = torch.einsum("rc,mck->mrk", i.A, i.G[..., :K])
    y = DO.dw(n1, i.D, dil, causal) + 0.7 * dN / dN.pow(2).mean((1, 2), keepdim=True).sqrt()
    if zeros:
        for p in ((0, 0, 0), (1, R - 1, K - 1), (0, 2, K // 2), (1, 3, K // 3)):
            y[p] = 0.0
    i.y = pad(y)
    i.ms2 = tuple(DO.r32(v) for v in gln_stats(DO.row_sums(prelu(i.y[..., :K], A_PRO)), R * K))
    i.cmean, i.crstd = (DO.r32(v) for v in cln_stats(prelu(i.y, A_PRO)))              # every frame of Kp: the pad frames hold 0 and 1/sqrt(eps)
    return i


def solo(i, m):
    """The case that holds utterance m alone (M = 1)."""
    j = types.SimpleNamespace(**vars(i))
    j.M = 1
    for name, v in vars(i).items():
        if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == i.M and name not in ("A", "D", "gp", "bp", "g1", "b1", "g2", "b2"):
            setattr(j, name, v[m:m + 1])
    j.ms1, j.ms2 = tuple(v[m:m + 1] for v in i.ms1), tuple(v[m:m + 1] for v in i.ms2)
    return j


RSTD_PAD = 1.0 / EPS ** 0.5


def pad_constants_ok(name, t, K):
    """The pad frames of the per-frame cLN outputs: mean 0, rstd 1 / sqrt(eps) (to 2e-5), fc = (rstd, 0, 0, 0)."""
    p = t[..., K:].double().cpu()
    if p.numel() == 0:
        return True
    if name == "mean":
        return float(p.abs().max()) == 0.0
    if name == "rstd":
        return float((p / RSTD_PAD - 1).abs().max()) < 2e-5
    return float((p[:, 0] / RSTD_PAD - 1).abs().max()) < 2e-5 and float(p[:, 1:].abs().max()) == 0.0


def fwd_cases():
    """(family, tile id, (R, Cn, K)) of the tile tests of tests/test_gpu_gemm_seams.py; family "k3": the residual-on-pieces form."""
    for fam in ("fp32", "split"):
        for t in range(4):
            for s in shapes(fam, t):
                yield fam, t, s
    for t in range(4):
        for s in k3_shapes(t):
            yield "k3", t, s


def forms_of(family):
    return ("res", "k3") if family == "k3" else FWD_FORMS
