"""tests/optim_oracle.py (the fp64 model of csrc/ctn_optim.hip, its error bound and its fp32 restatement) pinned on the CPU.

Three things make the oracle fit to judge the kernels in tests/test_gpu_optim_forms.py:
  * it IS the reference rule: equal to torch.optim.Adam / torch.optim.SGD / clip_grad_norm_ run in fp64, to 1e-12;
  * its bound is fair: on every entry of CASES the same rules evaluated in fp32 with every rounding in place stay within
    half of it (the limit is 2 E, see the oracle's docstring), and the fp32 norm within the norm limit;
  * its bound is sharp: each of thirteen wrong rules exceeds it on at least one entry of CASES.
"""
import numpy as np
import pytest
import torch

import optim_oracle as OO

F32 = np.float32


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _torch_side(p0, shapes):
    ps, o = [], 0
    for s in shapes:
        ps.append(torch.nn.Parameter(torch.from_numpy(p0[o:o + s].copy())))
        o += s
    return ps


def _torch_feed(ps, g, grad_scale, max_norm):
    """grad_scale and clip_grad_norm_ first, as the fused kernels do -> total norm."""
    o = 0
    for q in ps:
        q.grad = torch.from_numpy(g[o:o + q.numel()].copy()) * grad_scale
        o += q.numel()
    if max_norm > 0:
        return float(torch.nn.utils.clip_grad_norm_(ps, max_norm))
    return float(torch.linalg.vector_norm(torch.cat([q.grad for q in ps])))


SHAPES = (7, 15, 1, 64, 13)
STEPS = 5


def _grads(amp, seed):
    r = np.random.default_rng(seed)
    return [r.standard_normal(sum(SHAPES)) * amp for _ in range(STEPS)]


@pytest.mark.parametrize("wd", [0.0, 1e-4])
@pytest.mark.parametrize("max_norm,gs,amp", [(0.0, 1.0, 1.0), (5.0, 0.5, 30.0), (5.0, 1.0 / 3.0, 0.1), (5.0, 1.0, 1e-9)])
def test_oracle_adam_is_torch_adam_in_fp64(wd, max_norm, gs, amp):
    f = OO._f
    p = np.random.default_rng(1).standard_normal(sum(SHAPES))
    m, v = np.zeros_like(p), np.zeros_like(p)
    ps = _torch_side(p, SHAPES)
    ref = torch.optim.Adam(ps, lr=f(1e-3), betas=(f(0.9), f(0.999)), eps=f(1e-8), weight_decay=f(wd))
    for step, g in enumerate(_grads(amp, 2), 1):
        total = _torch_feed(ps, g, f(gs), f(max_norm))
        ref.step()
        o = OO.adam_step(p, g, m, v, step, wd=wd, grad_scale=gs, max_norm=max_norm, **OO.ADAM)
        p, m, v = o["p"], o["m"], o["v"]
        assert abs(o["total"] - total) <= 1e-12 * total
        assert _rel(p, torch.cat([q.detach() for q in ps]).numpy()) <= 1e-12
        assert _rel(m, torch.cat([ref.state[q]["exp_avg"] for q in ps]).numpy()) <= 1e-12
        assert _rel(v, torch.cat([ref.state[q]["exp_avg_sq"] for q in ps]).numpy()) <= 1e-12


@pytest.mark.parametrize("amp", [1.0, 30.0])
@pytest.mark.parametrize("row", OO.SGD_ROWS)
def test_oracle_sgd_is_torch_sgd_in_fp64(row, amp):
    f = OO._f
    mom, damp, nest, wd, max_norm, gs = row
    p = np.random.default_rng(3).standard_normal(sum(SHAPES))
    buf = np.full_like(p, np.nan)                      # the first step must not read it
    ps = _torch_side(p, SHAPES)
    ref = torch.optim.SGD(ps, lr=f(0.1), momentum=f(mom), dampening=f(damp), weight_decay=f(wd), nesterov=nest)
    for step, g in enumerate(_grads(amp, 4)):
        total = _torch_feed(ps, g, f(gs), f(max_norm))
        ref.step()
        o = OO.sgd_step(p, g, buf, step == 0, **OO._sgd_hp(row))
        p, buf = o["p"], o["buf"]
        assert abs(o["total"] - total) <= 1e-12 * total
        assert _rel(p, torch.cat([q.detach() for q in ps]).numpy()) <= 1e-12
        if mom != 0:
            assert _rel(buf, torch.cat([ref.state[q]["momentum_buffer"] for q in ps]).numpy()) <= 1e-12
        else:
            assert buf is None


@pytest.mark.parametrize("max_norm", [0.5, 5.0, 1e3])
def test_oracle_clip_is_clip_grad_norm_in_fp64(max_norm):
    g = np.random.default_rng(5).standard_normal(sum(SHAPES))
    ps = _torch_side(np.zeros_like(g), SHAPES)
    total = _torch_feed(ps, g, 1.0, max_norm)
    t, coef = OO.clip(g, 1.0, max_norm)
    assert abs(t - total) <= 1e-12 * total
    assert _rel(g * coef, torch.cat([q.grad for q in ps]).numpy()) <= 1e-12
    assert (coef < 1) == (total > max_norm)
    assert OO.clip(g, -0.5, 0.0) == (0.5 * t, 1.0) and OO.clip(g, 1.0, -1.0) == (t, 1.0)


# ---- the bound is fair --------------------------------------------------------------------------------------------------
_ORACLE = {}


def _oracle(i):
    """(inputs, oracle result) of CASES[i], computed once for the small cases."""
    if i in _ORACLE:
        return _ORACLE[i]
    c = OO.CASES[i]
    p, g, state = OO.case_inputs(c)
    out = (p, g, state, OO.run_oracle(c["rule"], p, g, state, c["hp"]))
    if c["n"] <= 1027:
        _ORACLE[i] = out
    return out


def _ratios(c, got, ref):
    r = {k: OO.worst_ratio(got, ref, k) for k in OO.outputs(c["rule"], c["hp"])}
    r["norm"] = abs(float(got["total"]) - ref["total"]) / OO.norm_limit(ref["total"])
    return r


@pytest.mark.parametrize("n", OO.SIZES)
def test_kernel_model_within_half_the_bound(n):
    worst = {}
    for i, c in enumerate(OO.CASES):
        if c["n"] != n:
            continue
        p, g, state, ref = _oracle(i)
        got = OO.kernel_model(c["rule"], p, g, state, c["hp"])
        for k, r in _ratios(c, got, ref).items():
            lim = 1.0 if k == "norm" else 0.5
            assert r <= lim, "%s: %s at %.3f of its limit" % (c["name"], k, r)
            worst[c["rule"], k] = max(worst.get((c["rule"], k), 0.0), r)
    assert worst
    print("OPTIM MODEL n=%d " % n + "  ".join("%s.%s %.3f" % (r, k, x) for (r, k), x in sorted(worst.items())))


def test_case_table_covers_what_it_lists():
    assert {c["n"] for c in OO.CASES} == set(OO.SIZES)
    for n in OO.PRODUCT_SIZES:
        adam = [c for c in OO.CASES if c["n"] == n and c["rule"] == "adam"]
        assert {c["step"] for c in adam} >= set(OO.STEPS) and {c["amp"] for c in adam} == set(OO.GRAD_SCALES)
        sgd = [c for c in OO.CASES if c["n"] == n and c["rule"] == "sgd"]
        for row in OO.SGD_ROWS:
            for first in (0, 1):
                assert any(c["hp"] == OO._sgd_hp(row) and c["first"] == first for c in sgd)
    for c in OO.CASES:                                   # the fp32 squares of the norm stay normal numbers
        g = np.abs(OO.case_inputs(c)[1]) if c["n"] <= 1027 else np.array([c["amp"] * 0.01, c["amp"] * 4])
        assert 1e-12 <= g.min() and g.max() <= 1e12


# ---- the bound is sharp -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", OO.MUTANTS)
def test_bound_rejects_wrong_rule(mutant):
    caught, worst = 0, 0.0
    for i, c in enumerate(OO.CASES):
        if c["n"] > 1027:
            continue
        p, g, state, ref = _oracle(i)
        r = max(_ratios(c, OO.kernel_model(c["rule"], p, g, state, c["hp"], mutant=mutant), ref).values())
        caught += r > 1.0
        worst = max(worst, r)
    print("OPTIM MUTANT %-26s exceeds the limit on %d cases, worst %.3g x" % (mutant, caught, worst))
    assert caught >= 1


# ---- the two norm probes of the GPU module ------------------------------------------------------------------------------
def test_norm_of_ones_tells_n_from_its_neighbours():
    """float32(sqrt(n)) is at least 2.8 ulp away from that of n - 1 and n + 1 at every size listed, so a norm held to one ulp
    of it sees a dropped or doubled element."""
    for n in OO.SIZES:
        x = float(F32(np.sqrt(float(n))))
        ulp = float(np.spacing(F32(x)))
        for k in (n - 1, n + 1):
            assert abs(float(F32(np.sqrt(float(k)))) - x) >= 2.8 * ulp, (n, k)


def test_norm_of_one_element_is_exact_in_the_model():
    """sqrt(fl32(x^2)) rounds back to |x|: the square is off by 2^-24 at most, its root by 2^-25, less than half an ulp of x."""
    x = np.random.default_rng(6).standard_normal(20000).astype(F32)
    x = x[x != 0]
    assert np.array_equal(np.sqrt((x * x).astype(np.float64)).astype(F32), np.abs(x))
