"""Every form of the 1x1-conv GEMMs (csrc/ctn_gemm.hip, ctn_gemm_common.h, ctn_gemm_b3.h) through the C ABI against tests/gemm_oracle.py
in fp64, at the tiles' seams, on guarded buffers, under all three arithmetics.

What runs.  The forward / input-gradient forms -- plain (trans_w 0 / 1 / pieces), ReLU, residual, K1 (PReLU statistics), the
operand prologue alone and with residual + ms_out (K3), B1 (ctn_pw_dgrad_gln / _planes), B1' (ctn_pw_dgrad_gln2), the cLN forward
(ctn_pw_gemm_cln + ctn_cln_stats_frame) and backward (ctn_pw_dgrad_cln + ctn_cln_bwd_frame), on every weight form the entry point
takes -- under every tile id: fp32 ids 0..3 through ctn_tune("pw_tile") (under fp32 arithmetic, and at R < 64 under every
arithmetic), split ids 0..3 through ctn_tune("b3_tile") (b6 kernels under the b6 / h3 arithmetics; the h3 entry points under all
three), and ids 0..3 of ctn_tune("b3_tile_k3") on the residual-on-pieces forms at R = 132.  The weight gradients (64x64 "w4"
kernel, 128-tile kernel, split kernels, h3 entry point) with and without the prologue on four split-K plans each.

Seams (gemm_oracle.shapes / k3_shapes / GEOMS / WGRAD_*; test_gemm_oracle_cpu.py checks that they are what they claim):
    R    fp32 family 20, 64, 68, 132; split family 64, 68, 132, 260 (68 / 132 / 260: one float4 row group over a 64 / 128 / 256-row tile)
    Cn   4 (below one k-tile), 20, 36, 64
    K    1, 61, 64, 65, 130, 191 (Kp 64, 64, 64, 128, 192, 192: no pad at 64, 63 pad frames at 65, a ragged 128-column tile at 192)
    per (family, tile id): (R over, Cn ragged, K = 130), (64, 64, K = 64), K = 1 and one more K, so that every K appears per form
    ctn_pw_dgrad_gln2 (P, dilation, causal): (3,1,n) (3,64,c) (3,80,n) (8,2,c) (1,4,n) (2,3,c) at K = 64, 65, 200, 5 under the default
      tiles, and at K = 200, 65 under the 128x128 tiles
    weight gradients (R, Cn): (64,64) (132,20) (68,36) (200,132) x (Kp, K, chunks_per_m): (64,1,1) (320,257,2) (832,800,3) (832,769,4)
      -- chunks_per_m 1, 2 and the maximum; 832 / 3 leaves a short last chunk (288, 288, 256); 832 / 4 is 13 k-tiles of 16 per chunk
      (fp32) or 224, 224, 224, 160 = 7, 7, 7, 5 k-tiles of 32 (split)

Per case: outputs are pre-filled with NaN inside an allocation with 4096 sentinel elements on either side -- afterwards the
sentinels are untouched, nothing is NaN, frames K..Kp of every activation output are exactly 0 (the prologue operand holds 1e30
there); a second call gives the same bits; utterance m of the M = 2 call is bitwise the M = 1 call on that utterance alone (every
form: tile decomposition and sum order do not depend on M); ctn_pw_stats_parts / ctn_pw_col_parts and, for weight gradients,
workspace bytes / (4 M R Cn) equal what the case intends; out_amax is bitwise max |Out[m]|.

Limits, the project's existing ones as ceilings (gemm_oracle.LIMIT):
    3e-6   of max |ref| per utterance: Out / dN of the plain, ReLU, residual and statistics forms     (test_pw_gemm_plain)
    5e-6   Out of the prologue forms, dW                          (test_pw_gemm_relu_and_stats_and_prologue, test_pw_wgrad)
    2e-5   cLN mean, rstd, fc over the valid frames (pad frames: constants)   (test_cln_forward_statistics..., test_cln_backward_entry_points...)
    2e-6   ms_out, relative                                                                            (test_gpu_h3.py)
    1e-5   every sum (statistics partials per TILE, S1 / S2, the eight sums, column partials per frame and row tile): of the sum of
           its terms' absolute values                                                           (test_gpu_h3.py, S1 / S2)
    6e-7   Out / dN / dW of the h3 entry points: of sum |a||b|, or 1.25x the fp32 MFMA's error on the same data   (test_gpu_h3.py)
tests/test_gemm_oracle_cpu.py shows on these inputs that fp32 arithmetic stays 4x inside each (the h3 rule, which is set against
fp32 arithmetic itself, excepted) and that eight wrong models miss them by 10x or more.

Largest figure per kind of output over all cases of this module and the three arithmetics, first MI355X run (the `GEMM MAX` lines
of -s; "at": arithmetic, test, form, weight form, R Cn K).  These figures are a record, not new limits.
    kind                 largest    limit   at
    plain Out / dN       3.62e-07   3e-6    fp32  fp32 tile 3     b1   w1  64 64 64
    pro   Out            3.39e-07   5e-6    fp32  fp32 tile 3     pro  w0  64 64 64
    h3    Out / dN       4.04e-07   6e-7    h3    split tile 2    pro  h3  260 4 130
    ms    ms_out         0          2e-6    (the fp64 statistics rounded once)
    sum   k1 part        2.93e-07   1e-5    h3    split tile 2    k1   h3  68 4 1
    sum   b1 part        7.63e-08   1e-5    h3    split tile 0    b1   h3  132 20 130
    sum   gln2 part      1.43e-07   1e-5    fp32  gln2 (3,64,c)   gln2 w1  68 20 65
    sum   clnf col       1.22e-06   1e-5    fp32  fp32 tile 1     clnf w0  132 36 130
    sum   clnb col       1.09e-06   1e-5    h3    split tile 0    clnb h3  260 36 61
    cln   mean           1.35e-07   2e-5    fp32  fp32 tile 0     clnf w0  64 64 64
    cln   rstd           1.72e-07   2e-5    h3    split tile 1    clnf h3  68 4 1
    cln   fc             2.76e-06   2e-5    h3    fp32 tile 0     clnb w1  20 4 1
    pro   dW             4.18e-07   5e-6    h3    ctn_pw_wgrad    132 20  Kp 832 K 800
    h3    dW             2.30e-05   6e-7    ctn_pw_wgrad_h3 with the prologue, 200 132 Kp 64 K 1: one frame, so dW = g f(x) with f the
                                            remainder of a cancellation in fp32; passes on the rule's second leg (1.25x the fp32 MFMA's
                                            error on the same data).  Without the prologue the largest is 5.36e-07.
"""
import contextlib
import math

import pytest
import torch

import gemm_oracle as GO
from conftest import ARITH

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gemm_arith")]

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import ops  # noqa: E402

DEV = "cuda:0"
NAN = float("nan")
F32, F64, I32 = torch.float32, torch.float64, torch.int32
GUARD, SENT = 4096, -7777.0
WORST = {}
_REF = {}


@pytest.fixture(autouse=True)
def _own_lines():
    print()                 # (-s: the GEMM lines start at the left margin, not behind the progress dots)
    yield
    _REF.clear()            # a reference is shared among the weight forms and calls of one test, not kept beyond it


@contextlib.contextmanager
def tuned(**kw):
    """ctn_tune switches for the enclosed calls; every switch this module touches goes back to its default afterwards."""
    try:
        for k, v in kw.items():
            ctn.lib.call("ctn_tune", k.encode(), v)
        ops._ws_cache.clear()
        yield
    finally:
        for k, v in GO.TUNE_DEFAULTS.items():
            ctn.lib.call("ctn_tune", k.encode(), v)
        ops._ws_cache.clear()


class Guarded:
    """An output buffer pre-filled with NaN (integers: 0) between two runs of GUARD sentinel elements of the same allocation."""

    def __init__(self, *shape, dtype=F32):
        self.n = math.prod(shape)
        self.flat = torch.full((self.n + 2 * GUARD,), int(SENT) if dtype == I32 else SENT, dtype=dtype, device=DEV)
        self.t = self.flat[GUARD:GUARD + self.n].view(shape)
        self.t.fill_(0 if dtype == I32 else NAN)

    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        return bool((self.flat[:GUARD] == SENT).all()) and bool((self.flat[GUARD + self.n:] == SENT).all())


def dev(t, dtype=F32):
    return t.to(dtype).contiguous().to(DEV)


def ptr(t):
    return 0 if t is None else t.data_ptr()


class Case:
    """Device buffers of one gemm_oracle.make_inputs() case."""

    def __init__(self, i):
        self.i = i
        self.A, self.At = dev(i.A), dev(i.A.t())
        self.X, self.Xp, self.G, self.res, self.y = dev(i.X), dev(i.Xp), dev(i.G), dev(i.res), dev(i.y)
        self.gp, self.bp, self.g1, self.b1, self.g2, self.D = dev(i.gp), dev(i.bp), dev(i.g1), dev(i.b1), dev(i.g2), dev(i.D)
        self.pro_part = dev(i.pro_part, F64)
        self.pro_ms = dev(torch.stack([i.pro_mean, i.pro_rstd], 1))
        self.ms2 = dev(torch.stack(i.ms2, 1))
        self.cmean, self.crstd = dev(i.cmean), dev(i.crstd)
        self.a_epi, self.a_pro = dev(torch.tensor([GO.A_EPI])), dev(torch.tensor([GO.A_PRO]))
        self._w, self._amax, self._solo = {}, {}, {}

    def weight(self, wf, k_major):
        """The weight operand A [R, Cn] in form wf: "w0" stored [R, Cn], "w1" stored [Cn, R], "b6" / "h3" pieces (k_major: split
        from the [Cn, R] matrix, as the input-gradient GEMMs of a layer do)."""
        if wf == "w0":
            return self.A
        if wf == "w1":
            return self.At
        key = (wf, k_major, ARITH["name"])
        if key not in self._w:
            fn = ops.h3_pieces if wf == "h3" else ops._b3_pieces
            self._w[key] = fn(self.At if k_major else self.A, self.i.R, self.i.Cn, k_major)
        return self._w[key]

    def amax(self, name):
        """The tracked maximum of an operand as its producer would have tracked it: over the tensor with zero pad frames (also for
        the prologue operand, whose 1e30 pad frames no kernel wrote)."""
        if name not in self._amax:
            self._amax[name] = ops.absmax_rows(getattr(self, name))
        return self._amax[name]

    def gbmax(self):
        if "gb" not in self._amax:
            self._amax["gb"] = ops.absmax_of(self.gp, self.bp)
        return self._amax["gb"]

    def solo(self, m):
        if m not in self._solo:
            self._solo[m] = Case(GO.solo(self.i, m))
        return self._solo[m]


W_FORM = {"w0": 0, "w1": 1, "b6": 2, "h3": 3}
DGRAD_FORMS = ("b1", "gln2", "clnb")


def run(form, wf, c, tile):
    """One form on one weight form through the C ABI -> {output name: Guarded}.  tile: (TM, TN) of the kernel that writes the
    statistics partials (sizes them)."""
    i, call, st = c.i, ctn.lib.call, ops._stream()
    M, R, Cn, K, Kp = i.M, i.R, i.Cn, i.K, i.Kp
    dims = (M, R, Cn, K, Kp)
    tm, tn = tile
    nparts, ncol = GO.n_parts(R, Kp, tm, tn), GO.cdiv(R, tm)
    h3 = wf == "h3"
    W = c.weight(wf, form in DGRAD_FORMS)
    out = {"Out": Guarded(M, R, Kp)}
    o = out["Out"].ptr()
    if form in ("plain", "relu", "res", "k1", "pro", "k3"):
        pro = form in ("pro", "k3")
        X = c.Xp if pro else c.X
        pa = (ptr(c.pro_part), 3, ptr(c.gp), ptr(c.bp), ptr(c.a_pro)) if pro else (0, 0, 0, 0, 0)
        resid = ptr(c.res) if form in ("res", "k3") else 0
        if form == "k3":
            out["ms_out"] = Guarded(M, 2)
        if form == "k1":
            out["part"] = Guarded(M, nparts, 2, dtype=F64)
        ms, part = (ptr(out[n].t) if n in out else 0 for n in ("ms_out", "part"))
        epi = ptr(c.a_epi) if form == "k1" else 0
        if h3:
            if resid:
                out["_amax"] = Guarded(M, ops.AMAX_SLOTS, dtype=I32)
            call("ctn_pw_gemm_h3", ptr(W), ptr(X), o, *dims, *pa, ms, resid, epi, part, ptr(c.amax("X")), ptr(c.gbmax()) if pro else 0,
                 ptr(out["_amax"].t) if resid else 0, st)
        else:
            call("ctn_pw_gemm", ptr(W), ptr(X), o, *dims, W_FORM[wf], *pa, ms, resid, epi, part, int(form == "relu"), st)
    elif form == "b1":
        out["part"] = Guarded(M, nparts, 2, dtype=F64)
        a = (ptr(W), ptr(c.G), o, *dims, ptr(c.y), ptr(c.g2), ptr(c.a_pro), ptr(c.ms2), out["part"].ptr())
        if h3:
            call("ctn_pw_dgrad_gln_h3", *a, ptr(c.amax("G")), st)
        else:
            call("ctn_pw_dgrad_gln_planes" if wf == "b6" else "ctn_pw_dgrad_gln", *a, st)
    elif form == "gln2":
        P, dil, causal = i.geom
        out["part"] = Guarded(M, nparts, 8, dtype=F64)
        call("ctn_pw_dgrad_gln2", ptr(W), W_FORM[wf], ptr(c.G), o, *dims, ptr(c.y), ptr(c.g2), ptr(c.a_pro), ptr(c.ms2), ptr(c.g1), ptr(c.b1),
             ptr(c.D), P, dil, int(causal), out["part"].ptr(), ptr(c.amax("G")) if h3 else 0, st)
    elif form == "clnf":
        out.update(col=Guarded(M, ncol, Kp, 2, dtype=F64), mean=Guarded(M, Kp), rstd=Guarded(M, Kp))
        call("ctn_pw_gemm_cln", ptr(W), W_FORM[wf], ptr(c.X), o, *dims, ptr(c.a_epi), out["col"].ptr(), ptr(c.amax("X")) if h3 else 0, st)
        call("ctn_cln_stats_frame", out["col"].ptr(), ncol, out["mean"].ptr(), out["rstd"].ptr(), M, R, Kp, st)
    elif form == "clnb":
        out.update(col=Guarded(M, ncol, Kp, 2, dtype=F64), fc=Guarded(M, 4, Kp))
        call("ctn_pw_dgrad_cln", ptr(W), W_FORM[wf], ptr(c.G), o, *dims, ptr(c.y), ptr(c.g2), ptr(c.a_pro), ptr(c.cmean), ptr(c.crstd),
             out["col"].ptr(), ptr(c.amax("G")) if h3 else 0, st)
        call("ctn_cln_bwd_frame", out["col"].ptr(), ncol, ptr(c.cmean), ptr(c.crstd), out["fc"].ptr(), M, R, Kp, st)
    else:
        raise KeyError(form)
    torch.cuda.synchronize()
    return out


def reference(form, i, tile):
    """The oracle's outputs, computed once per (case, form, tile) and shared."""
    key = (id(i), form, tile)
    if key not in _REF:
        _REF[key] = (i, GO.run_form(form, i, tile))
    return _REF[key][1]


def note(kind, e, cls, where):
    if e > WORST.get(kind, (-1.0,))[0]:
        WORST[kind] = (e, GO.LIMIT[cls], (ARITH["name"],) + tuple(where))


def h3_rule(e, fp32_err, where):
    """test_gpu_h3.py's check: 6e-7 of sum |a||b|, or where the fp32 MFMA itself is above that on this data, 1.25x its error."""
    if e >= GO.LIMIT["h3"]:
        prev = ARITH["name"]
        with ctn.gemm_arithmetic("fp32"):
            e32 = fp32_err()
        assert ctn.gemm_arith() == prev
        assert e <= 1.25 * e32, (where, e, e32)


def check(label, form, wf, c, tile):
    """Runs one form twice and once per utterance alone, and makes every per-case assertion; -> {output: error}."""
    i = c.i
    K, where = i.K, (label, form, wf, i.R, i.Cn, i.K)
    got, again = run(form, wf, c, tile), run(form, wf, c, tile)
    for name, g in got.items():
        assert g.intact(), (where, name, "a guard element was written")
        assert not bool(torch.isnan(g.t).any()), (where, name, "NaN left")
        assert torch.equal(g.t, again[name].t), (where, name, "second call differs")
    assert float(got["Out"].t[..., K:].abs().sum()) == 0.0, (where, "pad frames")
    for m in range(i.M):
        alone = run(form, wf, c.solo(m), tile)
        for name, g in alone.items():
            assert g.intact(), (where, name, "M = 1: a guard element was written")
            assert torch.equal(g.t[0], got[name].t[m]), (where, name, "utterance %d differs from the M = 1 call" % m)
    if "_amax" in got:
        assert torch.equal(got.pop("_amax").t.view(F32).amax(1), got["Out"].t.abs().flatten(1).amax(1)), (where, "out_amax")
    ref = reference(form, i, tile)
    errs = {}
    for name, r in ref.items():
        if "|" in name:
            continue
        g = got[name].t
        assert g.shape == r.shape, (where, name, g.shape, r.shape)
        if name in ("mean", "rstd", "fc"):
            assert GO.pad_constants_ok(name, g, K), (where, name, "pad frames")
        cls = "h3" if wf == "h3" and name == "Out" else GO.limit_class(form, name)
        mag = ref["Out|dot"] if cls == "h3" else ref.get(name + "|abs")
        errs[name] = e = GO.err_of(cls, g, r, mag, K)
        note("%s %s" % (cls, name if name in ("Out", "ms_out", "mean", "rstd", "fc") else form + " " + name), e, cls, where)
        if cls == "h3":
            h3_rule(e, lambda: GO.err_of("h3", run(form, "w1" if form in DGRAD_FORMS else "w0", c, GO.FP32_TILES[3])["Out"].t, r, mag), where)
        else:
            assert e < GO.LIMIT[cls], (where, name, e)
    print("GEMM %-14s %-5s %-2s R=%-3d Cn=%-2d K=%-3d " % (label, form, wf, i.R, i.Cn, K) + " ".join("%s=%.2e" % kv for kv in errs.items()))
    return errs


PLAIN_FORMS = [("plain", "w0"), ("plain", "w1"), ("relu", "w0"), ("res", "w0"), ("res", "w1"), ("k1", "w0"), ("k1", "w1"), ("pro", "w0"),
               ("pro", "w1"), ("k3", "w0"), ("k3", "w1"), ("b1", "w1"), ("gln2", "w1"), ("clnf", "w0"), ("clnf", "w1"), ("clnb", "w1")]
PIECE_FORMS = ["plain", "res", "k1", "pro", "k3", "b1", "gln2", "clnf", "clnb"]


def assert_parts(R, Kp, tile, family):
    """Coverage is asserted, not assumed: the library's own partial counts are those of the tile that the case intends."""
    lib = ctn.lib.load()
    if family == GO.family_of(ARITH["name"], R):
        assert lib.ctn_pw_stats_parts(GO.M_TEST, R, Kp) == GO.n_parts(R, Kp, *tile), (R, Kp, tile)
        assert lib.ctn_pw_col_parts(GO.M_TEST, R, Kp, 1) == GO.cdiv(R, tile[0])
    if family == "split":
        assert lib.ctn_pw_col_parts(GO.M_TEST, R, Kp, 3) == GO.cdiv(R, tile[0])


def run_fp32_tile(tid, first_plain):
    """Every form of the fp32-MFMA family under ctn_tune("pw_tile", tid): every shape under fp32 arithmetic, the R < 64 shapes under
    the other two."""
    tile = GO.FP32_TILES[tid]
    with tuned(pw_tile=tid):
        sh = [s for s in GO.shapes("fp32", tid) if GO.family_of(ARITH["name"], s[0]) == "fp32"]
        if first_plain:                                   # a never-run kernel: one small plain case first
            check("fp32 tile %d" % tid, "plain", "w0", Case(GO.make_inputs(*sh[-2])), tile)
        for R, Cn, K in sh:
            c = Case(GO.make_inputs(R, Cn, K))
            assert_parts(R, c.i.Kp, tile, "fp32")
            for form, wf in PLAIN_FORMS:
                check("fp32 tile %d" % tid, form, wf, c, tile)


def test_fp32_default_tile():
    assert GO.DEFAULT_TILE["fp32"] == 3
    run_fp32_tile(3, False)


@pytest.mark.parametrize("tid", [0, 1, 2])
def test_fp32_tiles_that_no_step_runs(tid):
    """128x128, 128x64 and 64x128: compiled for every form, reached only through ctn_tune("pw_tile") / CTN_PW_TILE.  Under fp32
    arithmetic the `ragged` branch of the shared epilogue (Kp = 192 under a 128-column tile) runs only here."""
    run_fp32_tile(tid, True)


@pytest.mark.parametrize("tid", [0, 1, 2, 3])
def test_split_tiles(tid):
    """ctn_tune("b3_tile", tid): the b6 kernels (fp32 weights split on the fly, and pieces) under the b6 / h3 arithmetics, the h3
    entry points under all three.  (The residual-on-pieces forms at R = 132 take ctn_tune("b3_tile_k3"): its default here.)"""
    tile = GO.B3_TILES[tid]
    arith = ARITH["name"]
    with tuned(b3_tile=tid):
        for R, Cn, K in GO.shapes("split", tid):
            c = Case(GO.make_inputs(R, Cn, K))
            assert_parts(R, c.i.Kp, tile, "split")
            forms = [(f, "h3") for f in PIECE_FORMS]
            if arith != "fp32":
                forms = PLAIN_FORMS + [(f, "b6") for f in PIECE_FORMS] + forms
            for form, wf in forms:
                check("split tile %d" % tid, form, wf, c, tile)


def run_k3_tile(tid, first_plain):
    stats_tile = GO.B3_TILES[GO.DEFAULT_TILE["split"]]
    arith = ARITH["name"]
    with tuned(b3_tile_k3=tid):
        sh = GO.k3_shapes(tid)
        forms = [(f, wf) for wf in (("b6", "h3") if arith != "fp32" else ("h3",)) for f in ("res", "k3")]
        if first_plain:
            check("k3 tile %d" % tid, "res", "h3", Case(GO.make_inputs(*sh[2])), stats_tile)
        for R, Cn, K in sh:
            assert GO.k3_tile_applies(R)
            c = Case(GO.make_inputs(R, Cn, K))
            for form, wf in forms:
                check("k3 tile %d" % tid, form, wf, c, stats_tile)


def test_k3_default_tile():
    assert GO.TUNE_DEFAULTS["b3_tile_k3"] == 3
    run_k3_tile(3, False)


@pytest.mark.parametrize("tid", [0, 1, 2])
def test_k3_tiles_that_no_step_runs(tid):
    """ctn_tune("b3_tile_k3", 0..2) on the residual-on-pieces forms (K3 and B5) at 128 < R <= 256: only id 3 runs in a step."""
    run_k3_tile(tid, True)


@pytest.mark.parametrize("geom", GO.GEOMS, ids=["P%d-d%d-%s" % (p, d, "c" if c else "n") for p, d, c in GO.GEOMS])
def test_dgrad_gln2_geometry(geom):
    """EPI_GLN_BWD2 on its own: the per-tile `interior` decision, the tap counts V clipped to [0, K), the `ok` mask of the frames >= K
    and the run-time kernel size, at K = 64 (one tile with both edges), 65, 200 (left-edge, interior and right-edge tiles) and 5
    (below the receptive field), under the default tiles (64 columns) and at K = 200 and 65 under the 128x128 tiles of both
    families.  The sums are compared per tile with their definitions."""
    R, Cn = GO.GEOM_SHAPE
    arith = ARITH["name"]
    fam = GO.family_of(arith, R)
    tile = GO.tile_of(fam, GO.DEFAULT_TILE[fam])
    for K in GO.GEOM_KS:
        c = Case(GO.make_inputs(R, Cn, K, geom=geom))
        assert_parts(R, c.i.Kp, tile, fam)
        for wf in (("w1",) if arith == "fp32" else ("w1", "b6")):
            check("gln2 %s" % (geom,), "gln2", wf, c, tile)
        check("gln2 %s" % (geom,), "gln2", "h3", c, GO.tile_of("split", GO.DEFAULT_TILE["split"]))
        if K in GO.GEOM_KS_WIDE:          # the same decisions under 128-column tiles (Kp = 256: two tiles; Kp = 128: one)
            with tuned(pw_tile=0, b3_tile=0):
                assert_parts(R, c.i.Kp, GO.GEOM_WIDE_TILE, fam)
                for wf in (("w1",) if arith == "fp32" else ("w1", "b6", "h3")):
                    check("gln2 %s wide" % (geom,), "gln2", wf, c, GO.GEOM_WIDE_TILE)


@pytest.mark.parametrize("what", ["P9", "odd_halo"])
def test_dgrad_gln2_refusals(what):
    R, Cn = GO.GEOM_SHAPE
    c = Case(GO.make_inputs(R, Cn, 65))
    i = c.i
    P, dil = (9, 1) if what == "P9" else (2, 3)
    D = dev(torch.ones(R, 9))
    dN, part = Guarded(i.M, R, i.Kp), Guarded(i.M, 64, 8, dtype=F64)
    lib = ctn.lib.load()
    rc = lib.ctn_pw_dgrad_gln2(ptr(c.At), 1, ptr(c.G), dN.ptr(), i.M, R, Cn, i.K, i.Kp, ptr(c.y), ptr(c.g2), ptr(c.a_pro), ptr(c.ms2), ptr(c.g1),
                               ptr(c.b1), ptr(D), P, dil, 0, part.ptr(), 0, ops._stream())
    msg = lib.ctn_last_error().decode()
    torch.cuda.synchronize()
    assert rc != 0 and "ctn_pw_dgrad_gln2" in msg, (rc, msg)
    assert bool(torch.isnan(dN.t).all()) and bool(torch.isnan(part.t).all()) and dN.intact() and part.intact()


def run_wgrad(c, pro, h3, nbytes):
    i = c.i
    dims = (i.M, i.R, i.Cn, i.K, i.Kp)
    dW, ws = Guarded(i.R, i.Cn), Guarded(nbytes // 4)
    pa = (ptr(c.gp), ptr(c.bp), ptr(c.a_pro), ptr(c.pro_ms)) if pro else (0, 0, 0, 0)
    X = c.Xp if pro else c.X
    if h3:
        ctn.lib.call("ctn_pw_wgrad_h3", ptr(c.res), ptr(X), dW.ptr(), *dims, *pa, ptr(c.amax("res")), ptr(c.amax("X")),
                     ptr(c.gbmax()) if pro else 0, ws.ptr(), nbytes, ops._stream())
    else:
        ctn.lib.call("ctn_pw_wgrad", ptr(c.res), ptr(X), dW.ptr(), *dims, *pa, ws.ptr(), nbytes, ops._stream())
    torch.cuda.synchronize()
    return dW, ws


@pytest.mark.parametrize("R,Cn", GO.WGRAD_SHAPES)
def test_weight_gradient_plans(R, Cn):
    """ctn_pw_wgrad (the 64x64 "w4" kernel at (64, 64) and the 128-tile kernel at (132, 20) under fp32 arithmetic -- the latter under
    every arithmetic --, the split kernels otherwise) and ctn_pw_wgrad_h3 on four split-K plans each, with and without the
    prologue; the plan that ran is read back from the workspace size."""
    arith = ARITH["name"]
    lib = ctn.lib.load()
    M = GO.M_TEST
    for Kp, K, want in GO.WGRAD_PLANS:
        c = Case(GO.make_inputs(R, Cn, K, Kp))
        with tuned(wgrad_blocks=GO.wgrad_blocks(False, R, Cn, want), b3_wgrad_blocks=GO.wgrad_blocks(True, R, Cn, want)):
            entries = [(False, lib.ctn_pw_wgrad_workspace(M, R, Cn, Kp), GO.wgrad_split(arith, R, Cn))]
            if R >= 32 and Cn >= 32:
                entries.append((True, lib.ctn_pw_wgrad_h3_workspace(M, R, Cn, Kp), True))
            for h3, nbytes, split in entries:
                plan = GO.wgrad_plan(split, M, R, Cn, Kp, GO.wgrad_blocks(split, R, Cn, want))
                assert nbytes == 4 * M * R * Cn * plan[2] and plan[2] == want, (R, Cn, Kp, h3, nbytes, plan)
                for pro in (False, True):
                    where = ("wgrad", "h3 entry" if h3 else arith, R, Cn, Kp, K, "pro" if pro else "")
                    (dW, ws), (dW2, ws2) = run_wgrad(c, pro, h3, nbytes), run_wgrad(c, pro, h3, nbytes)
                    for g in (dW, ws):
                        assert g.intact(), (where, "a guard element was written")
                        assert not bool(torch.isnan(g.t).any()), (where, "NaN left")
                    assert torch.equal(dW.t, dW2.t) and torch.equal(ws.t, ws2.t), (where, "second call differs")
                    key = (id(c.i), "wgrad", pro)
                    if key not in _REF:
                        _REF[key] = (c.i, GO.run_wgrad(c.i, pro))
                    ref = _REF[key][1]
                    cls = "h3" if h3 else "pro"
                    e = GO.err_of(cls, dW.t, ref["dW"], ref["dW|dot"])
                    note("%s dW" % cls, e, cls, where)
                    print("GEMM wgrad %-8s R=%-3d Cn=%-3d Kp=%-3d K=%-3d chunks_per_m=%d %s dW=%.2e" % (where[1], R, Cn, Kp, K, want, where[6], e))
                    if h3:
                        h3_rule(e, lambda: GO.err_of("h3", run_wgrad(c, pro, False, lib.ctn_pw_wgrad_workspace(M, R, Cn, Kp))[0].t, ref["dW"],
                                                     ref["dW|dot"]), where)
                    else:
                        assert e < GO.LIMIT[cls], (where, e)


def test_zz_largest_figures():
    """Prints the largest figure per kind of output over the cases that ran before it (for the table in the docstring)."""
    for kind, (e, lim, where) in sorted(WORST.items()):
        print("GEMM MAX %-18s %.2e  limit %.0e  at %s" % (kind, e, lim, " ".join(str(w) for w in where)))
    WORST.clear()           # (one table over the three arithmetics, printed by the first of the three runs of this function)
