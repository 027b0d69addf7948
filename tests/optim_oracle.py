"""Plain numpy fp64 model of the flat optimiser step (csrc/ctn_optim.hip), an error bound per element, an fp32 restatement
of the same rules, and the case table the CPU and GPU tests share.

The rules are written from the algebra of torch.nn.utils.clip_grad_norm_, torch.optim.Adam and torch.optim.SGD, not from
the kernels.  All arrays are fp32 and are widened to fp64; every hyper-parameter is first rounded to fp32, as the C ABI
receives it (the 1e-6 of the clip too).

    clip       total = |grad_scale| sqrt(sum g^2);  coef = min(1, max_norm / (total + 1e-6)) if max_norm > 0 else 1
    gradient   gi = g grad_scale coef + wd p                 (the coupled weight decay joins AFTER the clip, outside the norm)
    Adam       m' = b1 m + (1 - b1) gi;  v' = b2 v + (1 - b2) gi^2;  bc1 = 1 - b1^step;  bc2 = 1 - b2^step
               p' = p - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps)
    SGD        buf' = gi on the first step, else momentum buf + (1 - dampening) gi      (momentum != 0; the first step does not
               read buf);  d = gi + momentum buf' with nesterov, buf' with momentum alone, gi with none;  p' = p - lr d

THE BOUND.  u = 2^-24 is the largest relative error of one fp32 rounding.  Beside every fp64 value X the oracle carries E_X,
a first-order bound on |fl32 evaluation - X|, through these rules (|.| everywhere, so a cancelling sum keeps the errors of
both operands):  a product or quotient rounds once, u |X|;  a sum rounds once, u |X|, and inherits E_a + E_b;  a product
inherits |a| E_b + |b| E_a;  a quotient a / b inherits E_a / |b| + |a| E_b / b^2;  sqrt inherits E / (2 sqrt) and rounds once.
The roundings, in the order of the formulas (a count in brackets is the roundings accumulated on that quantity):

    gs = grad_scale coef        max_norm <= 0: coef = 1 and gs = grad_scale, exact [0].  Otherwise [6]: the norm's three
                                (below), total + 1e-6, the division, grad_scale * coef.  min(., 1) is 1-Lipschitz, so the
                                same 6 u hold whichever side of the cap the fp32 coefficient falls.
    gi = g gs (+ wd p)          g * gs [7]; with wd != 0 also wd * p and the sum.
    1 - b1, 1 - b2, 1 - damp    one rounding each (exact by Sterbenz where the subtrahend is >= 0.5, counted all the same);
                                dampening == 0 gives exactly 1 and no rounding of the product either.
    m'                          b1 * m, (1 - b1) * gi, the sum: [7 + 1 + 2 + 1 = 11 on the gradient's share, 2 on m's].
    v'                          gi * gi, * (1 - b2), b2 * v, the sum: the gradient's share carries 2 x 7 + 1 + 1 + 1 + 1 = 18.
    sqrt(bc2), bc1              computed in fp64 by the host, rounded to fp32 once each.
    denom                       sqrt, / sqrt(bc2) (the operand's rounding and the division's), + eps.
    lr / bc1                    bc1's rounding and the division's.
    p'                          m' / denom, * (lr / bc1), p - (.): three more.
    buf'                        momentum * buf, (1 - dampening) * gi, the sum;  nesterov: momentum * buf', the sum.
    p' (SGD)                    lr * d, p - (.).

The limit the tests apply is 2 x E.  The factor 2 stands for what is not modelled: FMA contraction (it only removes
roundings) and the order of the fp64 partial sums of the norm (2^-53 each); nothing on the path can ADD an fp32 rounding,
so an evaluation with every rounding in place, kernel_model() below, must stay within E itself = half the limit
(tests/test_optim_oracle_cpu.py).  Two roundings of gs that a shorter count would miss, |grad_scale| * sqrt(s) and
grad_scale * coef, are exact when grad_scale is a power of two and are counted because 1/3 is a case.

THE NORM.  The device adds fp32 squares in pairs, (x^2 + y^2) in fp32, then accumulates in fp64: each pair is off by at
most (1 + u)^2 - 1 = 2 u relatively, so is the sum s (all terms positive), and sqrt halves it: u.  The fp64 accumulation
and sqrt add 2^-53 terms.  Rounding sqrt(s) to fp32 is one more u and the product with |grad_scale| a third:
|total_fp32 - total| <= NORM_ULPS * 2^-24 * total with NORM_ULPS = 3.  (The n % 4 tail is squared in fp64: exact.)
"""
import numpy as np

F32 = np.float32
U = 2.0 ** -24
NORM_ULPS = 3.0
CLIP_EPS = float(F32(1e-6))


def _f(x):
    """A hyper-parameter as the C ABI receives it: rounded to fp32, then exact in fp64."""
    return float(F32(x))


def norm_limit(total):
    return NORM_ULPS * U * total


# ------------------------------------------------------------------------------------------------------------ fp64 oracle
def clip(g, grad_scale=1.0, max_norm=0.0):
    """-> (total, coef) in fp64."""
    g = np.asarray(g, dtype=np.float64)
    total = abs(_f(grad_scale)) * float(np.sqrt(np.sum(g * g)))
    mx = _f(max_norm)
    coef = min(1.0, mx / (total + CLIP_EPS)) if mx > 0 else 1.0
    return total, coef


def _gradient(p, g, grad_scale, max_norm, wd, coef):
    """gi = g grad_scale coef + wd p and its error -> (total, coef, GI, E_gi)."""
    total, c = clip(g, grad_scale, max_norm)
    if coef is None:
        coef = c
    gs = _f(grad_scale) * coef
    e_gs = 6 * U * abs(gs) if _f(max_norm) > 0 else 0.0
    a = g * gs
    e = np.abs(g) * e_gs + U * np.abs(a)
    if wd != 0:
        w = wd * p
        gi = a + w
        e = e + U * np.abs(w) + U * np.abs(gi)
    else:
        gi = a
    return total, coef, gi, e


def adam_step(p, g, m, v, step, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, grad_scale=1.0, max_norm=0.0, coef=None):
    """One Adam step with the fused clip.  coef overrides the clip coefficient (the non-finite edge cases).
    -> dict(p, m, v: fp64 results; e_p, e_m, e_v: the limits 2 E per element; total, coef)."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    lr, b1, b2, eps, wd = _f(lr), _f(b1), _f(b2), _f(eps), _f(wd)
    total, coef, gi, e_gi = _gradient(p, g, grad_scale, max_norm, wd, coef)
    a, b = b1 * m, (1 - b1) * gi
    m1 = a + b
    e_m = U * np.abs(a) + (1 - b1) * e_gi + 2 * U * np.abs(b) + U * np.abs(m1)
    a, b = b2 * v, (1 - b2) * gi * gi
    v1 = a + b
    e_v = U * np.abs(a) + (1 - b2) * 2 * np.abs(gi) * e_gi + 3 * U * b + U * v1
    root = np.sqrt(v1)
    with np.errstate(divide="ignore", invalid="ignore"):
        e_root = np.where(v1 > 0, e_v / (2 * root), 0.0) + U * root
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    q = root / np.sqrt(bc2)
    e_q = e_root / np.sqrt(bc2) + 2 * U * q
    den = q + eps
    e_den = e_q + U * den
    st = lr / bc1
    e_st = 2 * U * st
    with np.errstate(divide="ignore", invalid="ignore"):
        r = m1 / den
        e_r = e_m / den + np.abs(m1) * e_den / (den * den) + U * np.abs(r)
    t = st * r
    e_t = e_st * np.abs(r) + st * e_r + U * np.abs(t)
    p1 = p - t
    e_p = e_t + U * np.abs(p1)
    return dict(p=p1, m=m1, v=v1, e_p=2 * e_p, e_m=2 * e_m, e_v=2 * e_v, total=total, coef=coef)


def sgd_step(p, g, buf, first, lr=0.1, momentum=0.0, dampening=0.0, wd=0.0, nesterov=False, grad_scale=1.0, max_norm=0.0,
             coef=None):
    """One SGD step with the fused clip; buf may be None when momentum == 0 and is not read when first.
    -> dict(p, buf (None without momentum), e_p, e_buf, total, coef)."""
    p, g = np.asarray(p, dtype=np.float64), np.asarray(g, dtype=np.float64)
    lr, mom, damp, wd = _f(lr), _f(momentum), _f(dampening), _f(wd)
    total, coef, d, e_d = _gradient(p, g, grad_scale, max_norm, wd, coef)
    b1 = e_b = None
    if mom != 0:
        if first:
            b1, e_b = d, e_d
        else:
            b0 = np.asarray(buf, dtype=np.float64)
            a, b = mom * b0, (1 - damp) * d
            b1 = a + b
            e_b = U * np.abs(a) + (1 - damp) * e_d + (2 * U * np.abs(b) if damp != 0 else 0.0) + U * np.abs(b1)
        if nesterov:
            a = mom * b1
            d, e_d = d + a, e_d + mom * e_b + U * np.abs(a) + U * np.abs(d + a)
        else:
            d, e_d = b1, e_b
    t = lr * d
    p1 = p - t
    e_p = lr * e_d + U * np.abs(t) + U * np.abs(p1)
    return dict(p=p1, buf=b1, e_p=2 * e_p, e_buf=None if e_b is None else 2 * e_b, total=total, coef=coef)


# ------------------------------------------------------------------------------------ the same rules with every fp32 rounding
MUTANTS = ("eps_inside_bc2", "bc2_not_rooted", "lr_without_bc1", "wd_before_clip", "wd_in_norm", "norm_without_grad_scale",
           "coef_without_1e-6", "coef_not_capped", "nesterov_old_buffer", "dampening_on_first_step", "first_step_decays_buffer",
           "tail_untouched", "element_counted_twice")


def _model_clip(p, g, grad_scale, max_norm, wd, mutant):
    """The norm as the device sums it (fp32 squares added in pairs, fp64 accumulation, an fp64 tail) -> (total, coef) fp32."""
    n = g.size
    x = g
    if mutant == "wd_in_norm":
        x = g + (wd / grad_scale) * p if grad_scale != 0 else g
    n4 = n // 4 * 4
    q = x[:n4].reshape(-1, 2)
    s = float(np.sum((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]).astype(np.float64)))
    s += float(np.sum(x[n4:].astype(np.float64) ** 2))
    if mutant == "element_counted_twice":
        s += float(x[n // 2]) ** 2
    total = F32(np.sqrt(s))
    if mutant != "norm_without_grad_scale":
        total = total * np.abs(grad_scale)
    coef = F32(1)
    if max_norm > 0:
        coef = max_norm / (total if mutant == "coef_without_1e-6" else total + F32(1e-6))
        if mutant != "coef_not_capped":
            coef = np.fmin(coef, F32(1))            # C's fminf: the non-NaN operand
    return F32(total), F32(coef)


def kernel_model(rule, p, g, state, hp, mutant=None):
    """rule "adam": state (m, v, step); "sgd": state (buf or None, first).  numpy fp32, every operation rounded, no FMA.
    mutant: one of MUTANTS, a deliberately wrong rule.  -> dict(p, m, v | buf, total)."""
    assert mutant is None or mutant in MUTANTS, mutant
    p, g = np.asarray(p, dtype=F32), np.asarray(g, dtype=F32)
    h = {k: (F32(x) if isinstance(x, float) else x) for k, x in hp.items()}
    gscale, mx, wd, lr = F32(h.get("grad_scale", 1.0)), F32(h.get("max_norm", 0.0)), F32(h.get("wd", 0.0)), F32(h["lr"])
    n = g.size
    with np.errstate(all="ignore"):
        total, coef = _model_clip(p, g, gscale, mx, wd, mutant)
        gs = gscale * coef
        gi = (g * gscale + wd * p) * coef if mutant == "wd_before_clip" else g * gs + wd * p
        if rule == "adam":
            m, v, step = state
            m, v = np.asarray(m, dtype=F32), np.asarray(v, dtype=F32)
            b1, b2, eps = F32(h.get("b1", 0.9)), F32(h.get("b2", 0.999)), F32(h.get("eps", 1e-8))
            bc1 = F32(1.0 - float(b1) ** step)
            bc2 = 1.0 - float(b2) ** step
            bc2s = F32(bc2) if mutant == "bc2_not_rooted" else F32(np.sqrt(bc2))
            st = lr if mutant == "lr_without_bc1" else lr / bc1
            m1 = m * b1 + gi * (F32(1) - b1)
            v1 = v * b2 + (gi * gi) * (F32(1) - b2)
            den = (np.sqrt(v1) + eps) / bc2s if mutant == "eps_inside_bc2" else np.sqrt(v1) / bc2s + eps
            p1 = p - st * (m1 / den)
            out = dict(p=p1, m=m1, v=v1)
        else:
            buf, first = state
            mom, damp, nest = F32(h.get("momentum", 0.0)), F32(h.get("dampening", 0.0)), bool(h.get("nesterov", False))
            d, b1 = gi, None
            if mom != 0:
                b0 = np.asarray(buf, dtype=F32)
                damp1 = F32(1) - damp
                if first and mutant == "dampening_on_first_step":
                    b1 = d * damp1
                elif first and mutant == "first_step_decays_buffer":
                    b1 = b0 * mom + d
                elif first:
                    b1 = d.copy()
                else:
                    b1 = b0 * mom + d * damp1
                if nest:
                    d = d + mom * (b0 if mutant == "nesterov_old_buffer" else b1)
                else:
                    d = b1
            out = dict(p=p - lr * d, buf=b1)
        if mutant == "tail_untouched" and n % 4:
            olds = dict(p=p, m=state[0], v=state[1]) if rule == "adam" else dict(p=p, buf=state[0])
            for k, old in olds.items():
                if out[k] is not None:
                    out[k][n // 4 * 4:] = np.asarray(old, dtype=F32)[n // 4 * 4:]
    for k in out:
        assert out[k] is None or out[k].dtype == F32, (k, out[k].dtype)
    out["total"] = total
    return out


# ------------------------------------------------------------------------------------------------------------ case table
# The sizes at which a loop of csrc/ctn_optim.hip changes path (256 threads, float4 vectors, sumsq partials capped at 1024
# workgroups, update grids capped at 2048):
#   1, 3, 4, 5            only a tail; one vector; vector plus tail
#   1021, 1027            the second sumsq / update workgroup appears at n/4 + 1 = 257
#   262141, 262147        256 -> 257 partials: the second trip of the partial-sum loop, with and without a tail
#   524293                the second grid trip of clip_adam_kernel (2048 x 256 threads)
#   1048583               1024 partials reached and the second grid trip of sumsq_kernel
#   2097159               the second grid trip of the float4 SGD and Adam + L2 kernels
SIZES = (1, 3, 4, 5, 1021, 1027, 262141, 262147, 524293, 1048583, 2097159)
PRODUCT_SIZES = (5, 1027)
STEPS = (1, 2, 10, 1000, 100000)
GRAD_SCALES = (1e-9, 1e-3, 1.0, 30.0)          # eps dominates; ordinary; ordinary; the clip at 5 is active
SGD_ROWS = (  # momentum, dampening, nesterov, weight_decay, max_norm, grad_scale: SGD_CASES of tests/test_gpu_optim.py
    (0.0, 0.0, False, 0.0, 0.0, 1.0),
    (0.0, 0.0, False, 1e-4, 1.0, 0.5),
    (0.9, 0.0, False, 0.0, 1.0, 1.0),
    (0.9, 0.1, False, 1e-4, 0.0, 0.5),
    (0.9, 0.1, False, 0.0, 1.0, 1.0),
    (0.9, 0.0, True, 1e-4, 1.0, 1.0),
    (0.9, 0.0, True, 0.0, 0.0, 0.5),
)
ADAM = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)


def _sgd_hp(row):
    mom, damp, nest, wd, mx, gs = row
    return dict(lr=0.1, momentum=mom, dampening=damp, nesterov=nest, wd=wd, max_norm=mx, grad_scale=gs)


def _cases():
    """Each case: dict(name, rule "adam" | "sgd", n, amp (the gradient's magnitude), step | first, hp)."""
    out = []
    for n in PRODUCT_SIZES:
        for wd in (0.0, 1e-4):
            for mx in (0.0, 5.0):
                for gs in (1.0, 0.5, 1.0 / 3.0):
                    for step in STEPS:
                        for amp in GRAD_SCALES:
                            out.append(dict(rule="adam", n=n, amp=amp, step=step, hp=dict(ADAM, wd=wd, max_norm=mx, grad_scale=gs)))
        for row in SGD_ROWS:
            for first in (1, 0):
                for amp in GRAD_SCALES:
                    out.append(dict(rule="sgd", n=n, amp=amp, first=first, hp=_sgd_hp(row)))
        out.append(dict(rule="adam", n=n, amp=1.0, step=3, hp=dict(lr=1e-3, b1=0.5, b2=0.9, eps=1e-3, wd=0.0, max_norm=5.0, grad_scale=1.0)))
        # a total norm far below 1 with the clip active: the 1e-6 of the coefficient is a part in 10^3 of it
        out.append(dict(rule="adam", n=n, amp=1e-3, step=2, hp=dict(ADAM, wd=0.0, max_norm=1e-3, grad_scale=1.0)))
        out.append(dict(rule="sgd", n=n, amp=1e-3, first=0, hp=_sgd_hp((0.9, 0.0, False, 0.0, 1e-3, 1.0))))
    for n in SIZES:
        if n in PRODUCT_SIZES:
            continue
        for wd in (0.0, 1e-4):          # one setting per kernel: ctn_clip_adam_step takes wd = 0 only
            out.append(dict(rule="adam", n=n, amp=30.0, step=10, hp=dict(ADAM, wd=wd, max_norm=5.0, grad_scale=1.0 / 3.0)))
        out.append(dict(rule="sgd", n=n, amp=1.0, first=0, hp=_sgd_hp(SGD_ROWS[3])))
        out.append(dict(rule="sgd", n=n, amp=30.0, first=0, hp=_sgd_hp(SGD_ROWS[5])))
    for i, c in enumerate(out):
        c["seed"] = 7000 + i
        key = "step%d" % c["step"] if c["rule"] == "adam" else "first%d" % c["first"]
        c["name"] = "%s-n%d-amp%g-%s-%s" % (c["rule"], c["n"], c["amp"], key,
                                            ",".join("%s=%.4g" % (k, float(x)) for k, x in sorted(c["hp"].items())))
    return out


CASES = _cases()


def draw(n, amp, seed, zero_state=False):
    """-> p, g, m, v, buf: fp32 arrays.  p ~ N(0, 1); |g| in amp x [0.01, 4] with a random sign, so that the fp32 squares of
    the norm stay normal numbers; m and buf at the gradient's scale, v >= 0 at its square; zero_state: m = v = 0."""
    r = np.random.default_rng(seed)
    p = r.standard_normal(n).astype(F32)
    x = r.standard_normal(n)
    g = (np.sign(x) * np.clip(np.abs(x), 0.01, 4.0) * amp).astype(F32)
    m = (r.standard_normal(n) * 0.5 * amp).astype(F32)
    v = ((r.standard_normal(n) * amp) ** 2).astype(F32)
    buf = (r.standard_normal(n) * amp).astype(F32)
    if zero_state:
        m, v = np.zeros(n, F32), np.zeros(n, F32)
    return p, g, m, v, buf


def case_inputs(c):
    """-> (p, g, state) for kernel_model / run_oracle: Adam at step 1 starts from zero moments; an SGD first step is given a
    non-zero buffer that it must not read."""
    p, g, m, v, buf = draw(c["n"], c["amp"], c["seed"], zero_state=c["rule"] == "adam" and c["step"] == 1)
    if c["rule"] == "adam":
        return p, g, (m, v, c["step"])
    return p, g, (buf if c["hp"]["momentum"] != 0 else None, bool(c["first"]))


def run_oracle(rule, p, g, state, hp, coef=None):
    if rule == "adam":
        m, v, step = state
        return adam_step(p, g, m, v, step, coef=coef, **hp)
    buf, first = state
    return sgd_step(p, g, buf, first, coef=coef, **hp)


def outputs(rule, hp):
    """Names of the arrays a step writes, p first."""
    if rule == "adam":
        return ("p", "m", "v")
    return ("p", "buf") if hp["momentum"] != 0 else ("p",)


def worst_ratio(got, ref, key, skip=None):
    """max over elements of |got - ref| / limit (0 / 0 counts as 0, x / 0 as inf); skip: an index left out."""
    d = np.abs(np.asarray(got[key], dtype=np.float64) - ref[key])
    lim = ref["e_" + key]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0, 0.0, d / lim)
    if skip is not None:
        r = np.delete(r, skip)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0
