"""GPU: csrc/ctn_optim.hip -- sumsq_kernel, clip_adam_kernel, clip_sgd_kernel<MOM, NEST>, clip_adam_l2_kernel -- through the
C ABI against tests/optim_oracle.py, the fp64 restatement of clip_grad_norm_ + torch.optim.Adam / SGD, element by element
under the oracle's own bound (2 x the fp32 roundings on the path, derived in the oracle's docstring; the reported norm under
3 x 2^-24 of itself).  tests/test_optim_oracle_cpu.py shows that the oracle is the torch rule in fp64, that fp32 arithmetic
with every rounding in place uses at most half of the bound on these very inputs, and that thirteen wrong rules exceed it.

Sizes are the smallest at which a loop changes path (optim_oracle.SIZES): a tail alone, one vector, the second workgroup,
the 257th partial, the second grid trip of each update kernel and of sumsq_kernel.  Besides the values: the gradient is
bitwise unchanged, the fp64 workspace beyond the partials in use keeps its fill, a second run is bitwise equal, and a step
without momentum leaves the buffer it is handed alone.

One choice of the kernels is pinned here that differs from clip_grad_norm_: a NaN in the gradient gives a NaN norm and,
by C's fminf, a clip coefficient of 1 -- only that element turns NaN -- where torch would scale every gradient by NaN.
An infinite element gives the norm inf and the coefficient 0: that element turns NaN (inf * 0), the rest see a zero gradient.

Measured on the MI355X (largest error / limit over all tests of the module, `-s` prints them as OPTIM lines; the limit of
the values is the oracle's 2 E per element, that of the norm 3 x 2^-24 of it):

    entry point               p       exp_avg   exp_avg_sq   momentum buffer   total norm
    ctn_clip_adam_step        0.499   0.250     0.255        -                 0.495
    ctn_clip_adam_l2_step     0.500   0.257     0.283        -                 0.495
    ctn_clip_sgd_step         0.494   -         -            0.488             0.415
    FlatAdam / FlatSGD.step   0.477   0.115     0.132        0.282             0.142

p sits at half the limit wherever the update is far below one ulp of the parameter: the one rounding of p - update is then
the whole error, and E counts it once.  The moments and the buffer use about half of what the fp32 model with every
rounding uses (0.49): the device contracts each a * b + c into one FMA.  The norm of n ones is float32(sqrt(n)) to 0 ulp at
every size and the norm of a lone element is that element at every seam index.  The device agrees with C's fminf on a NaN
norm (coefficient 1); no kernel was changed.
"""
import numpy as np
import pytest
import torch

import optim_oracle as OO
from oracle import ctn_oracle as O

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import ops  # noqa: E402
from conv_tasnet_amd.optim import FlatAdam, FlatSGD  # noqa: E402

DEV = "cuda:0"
F32 = np.float32
SENTINEL = -7.25
KERNELS = ("adam", "adam_l2", "sgd")
ADAM_HP = dict(OO.ADAM, wd=0.0, max_norm=5.0, grad_scale=1.0)
SGD_HP = OO._sgd_hp((0.9, 0.1, False, 1e-4, 5.0, 1.0))
WORST = {}      # (kernel, output) -> (error / limit, case)


def _note(kernel, key, ratio, where):
    if ratio >= WORST.get((kernel, key), (-1.0, ""))[0]:
        WORST[kernel, key] = (ratio, where)


def _bits(t):
    return t.view(torch.int32)


def _same(a, b):
    return all((a[k] is None and b[k] is None) or torch.equal(_bits(a[k]), _bits(b[k])) for k in ("p", "m", "v", "buf"))


def _partials(n):
    return min((n // 4 + 1 + 255) // 256, 1024)


def _run(kernel, p, g, state, hp, norm_out=True, null_buf=False):
    """One call of the entry point on fresh device copies.  state: (m, v, step) or (buf, first) as numpy / None.
    -> dict(p, m, v, buf: device tensors or None; total: the reported norm as float; g, g0: the gradient after and before)."""
    n = g.size
    dp, dg = torch.from_numpy(p).to(DEV), torch.from_numpy(g).to(DEV)
    g0 = dg.clone()
    ws = torch.full((ctn.lib.ctn_optim_parts(),), SENTINEL, dtype=torch.float64, device=DEV)
    norm = torch.full((1,), SENTINEL, dtype=torch.float32, device=DEV)
    nptr = norm.data_ptr() if norm_out else 0
    stream = torch.cuda.current_stream().cuda_stream
    out = dict(p=dp, m=None, v=None, buf=None)
    if kernel == "sgd":
        buf, first = state
        if buf is None:
            buf = np.full(n, SENTINEL, F32)             # momentum 0: must stay as it is
        db = torch.from_numpy(buf).to(DEV)
        out["buf"] = db
        ctn.lib.call("ctn_clip_sgd_step", dp.data_ptr(), dg.data_ptr(), 0 if null_buf else db.data_ptr(), n, hp["grad_scale"],
                     hp["max_norm"], hp["lr"], hp["momentum"], hp["dampening"], hp["wd"], int(hp["nesterov"]), int(first),
                     nptr, ws.data_ptr(), stream)
    else:
        m, v, step = state
        dm, dv = torch.from_numpy(m).to(DEV), torch.from_numpy(v).to(DEV)
        out["m"], out["v"] = dm, dv
        args = (dp.data_ptr(), dg.data_ptr(), dm.data_ptr(), dv.data_ptr(), n, hp["grad_scale"], hp["max_norm"], hp["lr"],
                hp["b1"], hp["b2"], hp["eps"], int(step))
        if kernel == "adam":
            assert hp["wd"] == 0
            ctn.lib.call("ctn_clip_adam_step", *args, nptr, ws.data_ptr(), stream)
        else:
            ctn.lib.call("ctn_clip_adam_l2_step", *args, hp["wd"], nptr, ws.data_ptr(), stream)
    torch.cuda.synchronize()
    assert torch.equal(_bits(dg), _bits(g0)), "the gradient was written"
    assert bool((ws[_partials(n):] == SENTINEL).all()), "workspace written beyond partial %d" % _partials(n)
    out["total"] = float(norm) if norm_out else None
    return out


def _host(out):
    return {k: (None if out[k] is None else out[k].cpu().numpy()) for k in ("p", "m", "v", "buf")}


def _check(kernel, got, ref, rule, hp, where, skip=None, quiet=False):
    """Every output of the step within the oracle's bound -> the worst ratio of error to bound (printed unless quiet)."""
    h = _host(got)
    worst = 0.0
    for k in OO.outputs(rule, hp):
        r = OO.worst_ratio(h, ref, k, skip=skip)
        _note(kernel, k, r, where)
        assert r <= 1.0, "%s %s: %s at %.3f of its bound" % (kernel, where, k, r)
        worst = max(worst, r)
    if rule == "sgd" and hp["momentum"] == 0:
        assert bool((got["buf"] == SENTINEL).all()), "a step without momentum wrote the buffer"
    if not quiet:
        print("OPTIM %-7s %.3f of the bound  %s" % (kernel, worst, where))
    return worst


def _check_norm(kernel, total, ref_total, where):
    lim = OO.norm_limit(ref_total)
    r = abs(total - ref_total) / lim if lim > 0 else float(total != ref_total)
    _note(kernel, "norm", r, where)
    assert r <= 1.0, "%s %s: norm %.9g against %.9g, %.3f of its limit" % (kernel, where, total, ref_total, r)
    return r


def _kernels_of(c):
    if c["rule"] == "sgd":
        return ("sgd",)
    return ("adam", "adam_l2") if c["hp"]["wd"] == 0 else ("adam_l2",)


def _state(kernel, n, amp=1.0, seed=0, step=10):
    """-> p, g, state for that kernel (a later step on non-zero state), drawn as the case table draws."""
    p, g, m, v, buf = OO.draw(n, amp, seed)
    return p, g, ((buf, False) if kernel == "sgd" else (m, v, step))


def _rule(kernel):
    return "sgd" if kernel == "sgd" else "adam"


def _hp(kernel, **over):
    hp = dict(SGD_HP if kernel == "sgd" else ADAM_HP)
    if kernel == "adam_l2":
        hp["wd"] = 1e-4
    hp.update(over)
    return hp


# ---- the case table -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", OO.SIZES)
def test_every_case_within_the_bound(n):
    ran, worst = 0, {}
    for c in OO.CASES:
        if c["n"] != n:
            continue
        p, g, state = OO.case_inputs(c)
        ref = OO.run_oracle(c["rule"], p, g, state, c["hp"])
        for kernel in _kernels_of(c):
            got = _run(kernel, p, g, state, c["hp"])
            r = _check(kernel, got, ref, c["rule"], c["hp"], c["name"], quiet=True)
            rn = _check_norm(kernel, got["total"], ref["total"], c["name"])
            worst[kernel] = tuple(max(a, b) for a, b in zip(worst.get(kernel, (0.0, 0.0)), (r, rn)))
            again = _run(kernel, p, g, state, c["hp"])
            assert _same(got, again) and got["total"] == again["total"], "%s %s: two runs differ" % (kernel, c["name"])
            ran += 1
    assert ran
    for kernel, (r, rn) in sorted(worst.items()):
        print("OPTIM %-7s n=%d  values %.3f of the bound, norm %.3f of its limit" % (kernel, n, r, rn))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n", [5, 1027])
def test_null_total_norm_out_gives_the_same_buffers(kernel, n):
    p, g, state = _state(kernel, n, amp=30.0, seed=11)
    hp = _hp(kernel)
    a, b = _run(kernel, p, g, state, hp), _run(kernel, p, g, state, hp, norm_out=False)
    assert _same(a, b)
    assert a["total"] != SENTINEL and b["total"] is None


def test_adam_l2_with_zero_weight_decay_is_bitwise_the_adam_kernel_beyond_both_grid_caps():
    n = 2097159
    p, g, state = _state("adam", n, amp=30.0, seed=12)
    a, b = _run("adam", p, g, state, ADAM_HP), _run("adam_l2", p, g, state, ADAM_HP)
    assert _same(a, b) and a["total"] == b["total"]
    ref = OO.run_oracle("adam", p, g, state, ADAM_HP)
    _check("adam_l2", b, ref, "adam", ADAM_HP, "wd=0 n=%d" % n)
    _check_norm("adam_l2", b["total"], ref["total"], "wd=0 n=%d" % n)


# ---- the norm counts every element once, with weight one ------------------------------------------------------------------
class _Resident:
    """Device buffers of one size that the norm probes reuse (only the reported norm is read)."""

    def __init__(self, kernel, n):
        self.kernel, self.n = kernel, n
        self.p, self.m, self.v = (torch.zeros(n, device=DEV) for _ in range(3))
        self.g = torch.zeros(n, device=DEV)
        self.ws = torch.empty(ctn.lib.ctn_optim_parts(), dtype=torch.float64, device=DEV)
        self.norm = torch.zeros(1, device=DEV)

    def total(self):
        s, n, stream = self, self.n, torch.cuda.current_stream().cuda_stream
        s.norm.fill_(SENTINEL)
        if s.kernel == "sgd":
            ctn.lib.call("ctn_clip_sgd_step", s.p.data_ptr(), s.g.data_ptr(), s.m.data_ptr(), n, 1.0, 5.0, 0.1, 0.9, 0.0, 0.0, 0, 0,
                         s.norm.data_ptr(), s.ws.data_ptr(), stream)
        elif s.kernel == "adam":
            ctn.lib.call("ctn_clip_adam_step", s.p.data_ptr(), s.g.data_ptr(), s.m.data_ptr(), s.v.data_ptr(), n, 1.0, 5.0, 1e-3,
                         0.9, 0.999, 1e-8, 1, s.norm.data_ptr(), s.ws.data_ptr(), stream)
        else:
            ctn.lib.call("ctn_clip_adam_l2_step", s.p.data_ptr(), s.g.data_ptr(), s.m.data_ptr(), s.v.data_ptr(), n, 1.0, 5.0,
                         1e-3, 0.9, 0.999, 1e-8, 1, 1e-4, s.norm.data_ptr(), s.ws.data_ptr(), stream)
        return float(s.norm)


@pytest.mark.parametrize("kernel", KERNELS)
def test_norm_of_ones_counts_each_element_once(kernel):
    """float32(sqrt(n)) is >= 2.8 ulp from that of n - 1 and n + 1 at every size (tests/test_optim_oracle_cpu.py)."""
    for n in OO.SIZES:
        r = _Resident(kernel, n)
        r.g.fill_(1.0)
        want = F32(np.sqrt(np.float64(n)))
        got = r.total()
        ulps = abs(got - float(want)) / float(np.spacing(want))
        print("OPTIM %-7s ones n=%d norm %.9g want %.9g (%.1f ulp)" % (kernel, n, got, float(want), ulps))
        assert ulps <= 1.0, (n, got, float(want))


def _seams(n):
    """Indices where a loop of the kernels starts or ends: first, last of the float4 body, last, the first element of the second
    grid trip of sumsq_kernel (4 x 256 x its workgroups), of clip_adam_kernel and of the float4 update kernels."""
    s = {0, 4 * (n // 4) - 1, n - 1, 4 * 256 * _partials(n), 2048 * 256, 4 * 2048 * 256}
    return sorted(i for i in s if 0 <= i < n)


@pytest.mark.parametrize("kernel", KERNELS)
def test_norm_of_one_element_is_that_element(kernel):
    x = -2.71875
    for n in OO.SIZES:
        r = _Resident(kernel, n)
        for i in _seams(n):
            r.g.zero_()
            r.g[i] = x
            got = r.total()
            assert got == abs(x), "n=%d: an element at %d is reported as %.9g" % (n, i, got)
    assert _seams(2097159) == [0, 524288, 1048576, 2097152, 2097155, 2097158]


# ---- edges ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("n", [5, 1027])
def test_first_sgd_step_does_not_read_the_buffer(n, nesterov):
    p, g, _ = _state("sgd", n, seed=20)
    hp = _hp("sgd", nesterov=nesterov, dampening=0.0 if nesterov else 0.1)
    got = _run("sgd", p, g, (np.full(n, np.nan, F32), True), hp)
    assert bool(torch.isfinite(got["p"]).all()) and bool(torch.isfinite(got["buf"]).all())
    ref = OO.sgd_step(p, g, None, True, **hp)
    _check("sgd", got, ref, "sgd", hp, "first step on a NaN buffer n=%d nesterov=%d" % (n, nesterov))
    d = g.astype(np.float64) * (ref["coef"] * OO._f(hp["grad_scale"])) + OO._f(hp["wd"]) * p.astype(np.float64)
    assert np.array_equal(ref["buf"], d)           # the oracle's buffer after a first step is the update itself


@pytest.mark.parametrize("n", [5, 1027])
def test_sgd_without_momentum_takes_a_null_buffer(n):
    p, g, _ = _state("sgd", n, seed=21)
    hp = _hp("sgd", momentum=0.0, dampening=0.0)
    a = _run("sgd", p, g, (None, True), hp)
    b = _run("sgd", p, g, (None, False), hp, null_buf=True)
    assert torch.equal(_bits(a["p"]), _bits(b["p"])) and a["total"] == b["total"]
    ref = OO.sgd_step(p, g, None, False, **hp)
    _check("sgd", b, ref, "sgd", hp, "momentum 0, null buffer n=%d" % n)


@pytest.mark.parametrize("kernel", KERNELS)
def test_max_norm_zero_and_negative_do_not_clip(kernel):
    n = 1027
    p, g, state = _state(kernel, n, amp=30.0, seed=22)
    a = _run(kernel, p, g, state, _hp(kernel, max_norm=0.0))
    b = _run(kernel, p, g, state, _hp(kernel, max_norm=-1.0))
    assert _same(a, b) and a["total"] == b["total"]
    hp = _hp(kernel, max_norm=-1.0)
    ref = OO.run_oracle(_rule(kernel), p, g, state, hp)
    assert ref["coef"] == 1.0 and ref["total"] > 100
    _check(kernel, b, ref, _rule(kernel), hp, "max_norm=-1")
    _check_norm(kernel, b["total"], ref["total"], "max_norm=-1")


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("gs", [1.0 / 3.0, -0.5])
def test_grad_scale_sign_and_size(kernel, gs):
    """The norm takes |grad_scale|, the update the signed value; the clip is active (total about 30 sqrt(n) |gs|)."""
    n = 1027
    p, g, state = _state(kernel, n, amp=30.0, seed=23)
    hp = _hp(kernel, grad_scale=gs)
    ref = OO.run_oracle(_rule(kernel), p, g, state, hp)
    assert ref["total"] > 0 and ref["coef"] < 1
    got = _run(kernel, p, g, state, hp)
    _check(kernel, got, ref, _rule(kernel), hp, "grad_scale=%.3g" % gs)
    _check_norm(kernel, got["total"], ref["total"], "grad_scale=%.3g" % gs)
    if gs < 0:                  # and the mirrored gradient with the mirrored scale is the same step, bit for bit
        assert _same(got, _run(kernel, p, -g, state, dict(hp, grad_scale=-gs)))


@pytest.mark.parametrize("kernel,momentum,first", [("adam", None, None), ("adam_l2", None, None), ("sgd", 0.9, True),
                                                   ("sgd", 0.9, False), ("sgd", 0.0, True)])
def test_zero_gradient_with_zero_state_moves_nothing(kernel, momentum, first):
    """wd = 0 and the clip switched on (coef = min(1, 5 / 1e-6) = 1): p bitwise unchanged, the state still zero, norm 0.0."""
    for n in (5, 1027):
        p = OO.draw(n, 1.0, 24)[0]
        zero = np.zeros(n, F32)
        if kernel == "sgd":
            hp, state = _hp("sgd", wd=0.0, momentum=momentum, dampening=0.0), (zero if momentum else None, first)
        else:
            hp, state = _hp(kernel, wd=0.0), (zero, zero, 1)
        got = _run(kernel, p, zero, state, hp)
        assert torch.equal(_bits(got["p"]), _bits(torch.from_numpy(p).to(DEV)))
        assert got["total"] == 0.0
        for k in OO.outputs(_rule(kernel), hp)[1:]:
            assert bool((got[k] == 0).all())


@pytest.mark.parametrize("kernel", KERNELS)
def test_total_norm_either_side_of_max_norm(kernel):
    """total = max_norm (1 - 2^-20), max_norm (1 + 2^-20), and max_norm = float32(total): the coefficient is capped on one side
    and 1 - 1e-6 on the other; min(., 1) is 1-Lipschitz, so the same bound holds across the cap."""
    n, mx = 1027, 5.0
    p, g, state = _state(kernel, n, seed=25)
    t0 = OO.clip(g)[0]
    for tag, f in (("below", 1 - 2.0 ** -20), ("above", 1 + 2.0 ** -20), ("at", None)):
        gg = g if f is None else (g.astype(np.float64) * (mx * f / t0)).astype(F32)
        hp = _hp(kernel, max_norm=mx if f is not None else float(F32(t0)))
        ref = OO.run_oracle(_rule(kernel), p, gg, state, hp)
        rel = ref["total"] / float(F32(hp["max_norm"])) - 1
        assert abs(rel - (0.0 if f is None else f - 1)) < 2.0 ** -24, rel
        got = _run(kernel, p, gg, state, hp)
        _check(kernel, got, ref, _rule(kernel), hp, "total %s max_norm" % tag)
        _check_norm(kernel, got["total"], ref["total"], "total %s max_norm" % tag)


def _non_finite(kernel, bad, coef, idx, n=1027):
    p, g, state = _state(kernel, n, seed=26)
    hp = _hp(kernel)
    gg = g.copy()
    gg[idx] = bad
    got = _run(kernel, p, gg, state, hp)
    g0 = g.copy()
    g0[idx] = 0.0
    ref = OO.run_oracle(_rule(kernel), p, g0, state, hp, coef=coef)
    h = _host(got)
    for k in OO.outputs(_rule(kernel), hp):
        nan = np.isnan(h[k])
        assert nan[idx] and nan.sum() == 1, "%s %s: %d NaN, element %d %r" % (kernel, k, nan.sum(), idx, h[k][idx])
    _check(kernel, got, ref, _rule(kernel), hp, "%r at %d" % (bad, idx), skip=idx)
    return got["total"]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("idx", [6, 1026])
def test_one_infinite_gradient_element(kernel, idx):
    """norm = inf, coef = max_norm / inf = 0: inf * 0 = NaN at that element, a zero gradient everywhere else."""
    assert _non_finite(kernel, np.inf, 0.0, idx) == float("inf")


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("idx", [6, 1026])
def test_one_nan_gradient_element(kernel, idx):
    """norm = NaN; fminf(NaN, 1) is 1 (the non-NaN operand), so coef = 1: only that element turns NaN.  clip_grad_norm_ would
    multiply every gradient by NaN."""
    assert np.isnan(_non_finite(kernel, np.nan, 1.0, idx))


# ---- through the Python layer ---------------------------------------------------------------------------------------------
def _tiny(norm_type, causal, seed):
    torch.manual_seed(seed)
    return ctn.ConvTasNet(8, 4, 4, 8, 3, 2, 1, 2, norm_type=norm_type, causal=causal).to(DEV)


def _backward(model, opt, first_utt):
    """One forward / loss / backward on batch 2 x 64 frames -> (flat gradient, fp64 norm of the concatenated .grad views)."""
    mix, lens, src = O.synth_batch(first_utt, 2, (64 + 1) * 4 // 2)
    opt.zero_grad()
    est = model(mix.to(DEV))
    assert est.shape[-1] == mix.shape[-1]
    ctn.cal_loss(src.to(DEV), est, lens.to(DEV))[0].backward()
    ops.join_side_stream(opt.flat_grads.device)
    torch.cuda.synchronize()
    views = torch.cat([p.grad.reshape(-1) for p in opt.param_groups[0]["params"]])
    return opt.flat_grads.clone(), float(torch.linalg.vector_norm(views.double()))


def _padding(opt):
    pad = torch.ones(opt.numel, dtype=torch.bool, device=DEV)
    for _, o, n in opt._segments():
        pad[o:o + n] = False
    assert int(pad.sum()) >= 1
    return pad


@pytest.mark.parametrize("norm_type,causal", [("gLN", False), ("cLN", True)])
@pytest.mark.parametrize("which", ["adam", "sgd"])
def test_flat_optimisers_keep_padding_zero_and_follow_the_oracle(which, norm_type, causal):
    model = _tiny(norm_type, causal, 30)
    if which == "adam":
        opt, hp, steps = FlatAdam(model.parameters(), lr=1e-3, direct_grads=True), dict(OO.ADAM, wd=0.0), 1
    else:
        opt = FlatSGD(model.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4, direct_grads=True)
        hp, steps = dict(lr=0.1, momentum=0.9, dampening=0.0, nesterov=False, wd=1e-4), 2
    hp.update(max_norm=5.0, grad_scale=1.0)
    pad = _padding(opt)
    state_names = ("exp_avg", "exp_avg_sq") if which == "adam" else ("momentum_buffer",)
    where = "%s %s" % (type(opt).__name__, norm_type)
    for step in range(steps):
        g, views_norm = _backward(model, opt, 50 + 2 * step)
        assert float(g.abs().max()) > 0
        assert bool((g[pad] == 0).all()), "%d padding slots of flat_grads hold a gradient" % int((g[pad] != 0).sum())
        p0 = opt.flat_params.cpu().numpy()
        if which == "adam":
            state = (opt.exp_avg.cpu().numpy(), opt.exp_avg_sq.cpu().numpy(), step + 1)
        else:
            state = (opt.momentum_buffer.cpu().numpy(), step == 0)
        ref = OO.run_oracle(which, p0, g.cpu().numpy(), state, hp)
        opt.step(max_grad_norm=5.0)
        torch.cuda.synchronize()
        _check_norm("python", float(opt.last_total_norm), views_norm, where)
        assert abs(ref["total"] - views_norm) <= 1e-12 * views_norm          # the padding adds nothing
        got = dict(p=opt.flat_params, m=None, v=None, buf=None)
        if which == "adam":
            got["m"], got["v"] = opt.exp_avg, opt.exp_avg_sq
        else:
            got["buf"] = opt.momentum_buffer
        _check("python", got, ref, which, hp, "%s step %d" % (where, step + 1))
        for name in ("flat_params",) + state_names:
            assert bool((getattr(opt, name)[pad] == 0).all()), "padding of %s at step %d" % (name, step + 1)
        assert bool((opt.flat_grads[pad] == 0).all())


def test_zz_largest_figures():
    """Prints the largest figure per kernel and output over the tests that ran before it (for the table in the docstring)."""
    for (kernel, key), (r, where) in sorted(WORST.items()):
        print("OPTIM MAX %-7s %-4s %.3f of its limit  at %s" % (kernel, key, r, where))
