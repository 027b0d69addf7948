"""tests/dw_batched_cases.py on the CPU, on exactly the inputs of tests/test_gpu_depthwise_batched.py: the oracle's formulas in
fp32 stay at least 4x inside every ceiling of that test, so the limits hide no failure, and a model of a kernel whose halo or
early loads read the neighbouring row's data in memory, on either side, misses them by 10x or more."""
import pytest
import torch

import dw_batched_cases as BC
import dw_oracle as DO

F64 = torch.float64
TENSOR_OUT = {"bwd_plain": "dY", "bwd_gln": "dN1", "bwd_gln2": "dY1", "bwd_cln": "dN1", "bwd_cln_x": "dN1"}


def _cases(tag, kind):
    Kf, Kb = BC.case_Ks(tag, kind)
    return ((DO.make_inputs(*DO.CONFIGS[tag], Kf), DO.FWD_FORMS), (DO.make_inputs(*DO.CONFIGS[tag], Kb), DO.BWD_FORMS))


def test_frame_counts_and_guard_layout():
    for tag in BC.TAGS:
        p = DO.plan(*DO.CONFIGS[tag])
        assert p.halo > 0 and p.padl > 0
        for seg in (p.fwd_seg, p.bwd_seg):
            ks = [BC.frames(kind, seg) for kind in BC.KINDS]
            assert ks == [2 * seg + 1, 3 * seg + 67, seg + 259, seg + 515, seg + 771, seg + 260]
            assert [BC.kp_of(k) - k for k in ks] == [3, 1, 1, 1, 1, 0]
    assert {DO.plan(*DO.CONFIGS[t]).bwd_buf + str(DO.plan(*DO.CONFIGS[t]).vec4) for t in BC.TAGS} == {b + v for b in "SML" for v in ("True", "False")}
    assert {DO.plan(*DO.CONFIGS[t]).fwd_buf + str(DO.plan(*DO.CONFIGS[t]).vec4) for t in BC.TAGS} == {b + v for b in "SL" for v in ("True", "False")}
    t = torch.arange(2 * 3 * 5, dtype=F64).reshape(2, 3, 5) + 1
    buf, view = BC.guarded(t, 8, 1e30)
    assert buf.shape == (8, 8) and view.shape == (2, 3, 8) and view.data_ptr() == buf[1].data_ptr()
    assert bool((buf[0] == 1e30).all() and (buf[-1] == 1e30).all()) and torch.equal(view[..., :5], t.float()) and float(view[..., 5:].abs().sum()) == 0
    # the model reads what lies in that buffer: frame -1 of row 0 is the guard, frame -1 of row 1 is row 0's last pad frame
    # (0), frame K + 3 of row 0 is row 1's first frame
    with BC.reads_neighbour_rows(8, 1e30):
        left, right = DO._shift(t, -1), DO._shift(t, 4)
    assert left[0, 0, 0] == 1e30 and left[0, 1, 0] == 0 and left[0, 0, 1] == t[0, 0, 0]
    assert right[0, 0, 4] == t[0, 1, 0] and right[0, 0, 0] == t[0, 0, 4] and right[1, 2, 4] == 1e30 and right[0, 0, 1] == 0
    assert torch.equal(DO._shift(t, -1)[..., 1:], t[..., :-1]) and float(DO._shift(t, -1)[..., 0].abs().sum()) == 0


@pytest.mark.parametrize("tag", BC.TAGS)
def test_limits_are_reachable_in_fp32(tag):
    bad = {}
    for kind in BC.KINDS:
        for inp, forms in _cases(tag, kind):
            for form in forms:
                ref, got = DO.run_form(form, inp), DO.run_form(form, inp, dtype=torch.float32)
                for name, r in ref.items():
                    cls, how = DO.OUTPUTS[(form, name)]
                    e = DO.rel_err(got[name], r, how) / DO.LIMIT[cls]
                    if e > 0.25:
                        bad[(kind, form, name)] = e
    assert not bad, bad


@pytest.mark.parametrize("tag", BC.TAGS)
def test_limits_catch_a_read_of_the_neighbouring_row(tag):
    """Guard value 0, so only the neighbouring rows' own data leak, one side at a time, at every frame count.  Left of frame 0
    lie the previous row's Kp - K pad frames (zeros) and then its data; right of frame K - 1 the row's own pad frames and then
    the next row's data.  So a side leaks data exactly when the taps reach further than Kp - K frames (dw_batched_cases.reach):
    then the output must miss its limit by 10x or more, and otherwise the model must give the oracle's result exactly.  Which
    (side, output, Kp - K) leak is asserted below for every configuration; guard value 1e30 at one frame count shows that the
    first and the last row do reach a guard row."""
    weak, leaks = [], set()
    for kind in BC.KINDS:
        for inp, forms in _cases(tag, kind):
            pad = BC.kp_of(inp.K) - inp.K
            ref = {form: DO.run_form(form, inp) for form in forms}
            for side in ("left", "right"):
                for form in forms:
                    with BC.reads_neighbour_rows(BC.kp_of(inp.K), 0.0, side):
                        got = DO.run_form(form, inp)
                    for name in (TENSOR_OUT.get(form, "Z"),) + (("dD",) if form in DO.BWD_FORMS else ()):
                        cls, how = DO.OUTPUTS[(form, name)]
                        e = DO.rel_err(got[name], ref[form][name], how)
                        if BC.reach(tag, name, side) > pad:
                            leaks.add((side, "x" if name in ("Z", "dD") else "dd", pad))
                            if not e >= 10 * DO.LIMIT[cls]:
                                weak.append((kind, side, form, name, e))
                        elif e != 0.0:
                            weak.append((kind, side, form, name, e, "no leak expected"))
    assert not weak, weak
    p = DO.plan(*DO.CONFIGS[tag])
    # every configuration leaks on the left of the x image and on the right of the dd image at every pad but A's (reach 1:
    # only at Kp = K); the non-causal ones (A, C, J, E) also on the other two sides
    expect = {(side, img, pad) for side in ("left", "right") for img in ("x", "dd") for pad in (0, 1, 3)
              if (p.padl if (side == "left") == (img == "x") else p.halo - p.padl) > pad}
    assert leaks == expect and {("left", "x", 0), ("right", "dd", 0)} <= leaks, (leaks, expect)
    inp, forms = list(_cases(tag, "three_seg"))[1]
    for form in forms:
        ref = DO.run_form(form, inp)
        with BC.reads_neighbour_rows(BC.kp_of(inp.K), 1e30):
            got = DO.run_form(form, inp)
        name = TENSOR_OUT[form]
        assert DO.rel_err(got[name], ref[name], DO.OUTPUTS[(form, name)][1]) > 1e20, (form, name)


@pytest.mark.parametrize("K", BC.GLN_KS)
def test_gln_prelu_bwd_limits_are_reachable_in_fp32(K):
    i = BC.gln_inputs(K)
    ref, got = BC.gln_prelu_bwd(i), BC.gln_prelu_bwd(i, dtype=torch.float32)
    assert DO.rel_err(got["dY"], ref["dY"], "utt") <= 0.25 * 2e-5
    assert DO.rel_err(got["dalpha_part"], ref["dalpha_part"], "all") <= 0.25 * 1e-4
    # the definition against autograd: d/dy, d/dalpha of sum(gLN(prelu(y)) dN) without the affine part's beta
    y = i["y"].clone().requires_grad_(True)
    al = torch.tensor([i["al"]], dtype=F64, requires_grad=True)
    p = torch.where(y >= 0, y, al * y)
    mu = p.mean((1, 2), keepdim=True)
    xh = (p - mu) / torch.sqrt(((p - mu) ** 2).mean((1, 2), keepdim=True) + DO.EPS)
    (DO._ch(i["g"]) * xh * i["dN"]).sum().backward()
    # (the kernel is handed statistics and sums that were rounded to fp32: 1e-5 is what that rounding leaves)
    assert DO.rel_err(ref["dY"], y.grad, "utt") < 1e-5
    assert abs(float(ref["dalpha_part"].sum()) - float(al.grad)) < 1e-5 * abs(float(al.grad)) + 1e-12
