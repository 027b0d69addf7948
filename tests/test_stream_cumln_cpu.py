"""CPU-only checks of the cumulative fused streaming path: tests/stream_cumln_oracle.py against a restatement on
cumln_oracle.cumln_fwd and against itself in other cuts, the fp32 model and the deliberate defects against LIMIT, the new entry
points' ABI surface and argument errors (in front of the first launch), and the host side of the three classes."""
import ctypes

import pytest
import torch

import conv_tasnet_amd as ctn
from conv_tasnet_amd import _lib
from conv_tasnet_amd.streaming import (CUM_STEP, FusedStreamingSeparator, FusedStreamPool, ResamplingStreamPool, check_fused_model,
                                       plan_steps)

import cumln_oracle as CL
import stream_cumln_oracle as CO

F64 = torch.float64
CASES = range(len(CO.CASES))


@pytest.fixture(autouse=True)
def _own_lines():
    print()


def restated(ci):
    """The stack of a case on the whole signal, block by block, with cumln_oracle.cumln_fwd as the norm and conv1d as the taps."""
    p, y = CO.stack_inputs(ci)
    y = y.to(F64)
    T = y.shape[2]
    for b in p.blocks:
        H, P = b.D.shape
        h = torch.matmul(b.W1.to(F64), y)
        n1 = CL.cumln_fwd(h, T, b.g1, b.b1, float(b.a1))["out"]
        pad = torch.nn.functional.pad(n1, ((P - 1) * b.d, 0))
        z = torch.nn.functional.conv1d(pad, b.D.to(F64).view(H, 1, P), dilation=b.d, groups=H)
        n2 = CL.cumln_fwd(z, T, b.g2, b.b2, float(b.a2))["out"]
        y = y + torch.matmul(b.W2.to(F64), n2)
    return y


@pytest.mark.parametrize("ci", CASES, ids=CO.CASE_IDS)
def test_fp64_whole_signal_is_the_restatement_on_cumln_fwd(ci):
    e = CO.rel_err(CO.stack_reference(ci), restated(ci))
    print("case %d: oracle against the restatement %.2e" % (ci, e))
    assert e < 1e-12


@pytest.mark.parametrize("ci", CASES, ids=CO.CASE_IDS)
def test_fp64_chunked_equals_whole(ci):
    for name, plan in CO.plans(ci).items():
        long = name == "long"
        e = CO.rel_err(CO.stack_model(ci, plan, F64, long=long), CO.stack_reference(ci, long))
        print("case %d %-4s %3d calls: chunked against whole %.2e" % (ci, name, len(plan), e))
        assert e < 1e-12, (ci, name)


def test_plans_are_what_the_module_says():
    for ci, c in enumerate(CO.CASES):
        assert c.max_frames == 16
        ps = CO.plans(ci)
        assert sum(ps["cut0"]) == sum(ps["cut1"]) >= 3 * max(CO.ring_len(c.P, d, 16) for d in c.dil) and ps["cut0"] != ps["cut1"]
        assert {1, 15, 16} <= set(ps["cut0"]) and max(ps["cut0"] + ps["cut1"]) == 16
        _, y = CO.stack_inputs(ci)
        amp = y.abs().amax((1, 2))
        assert y.shape[0] == 3 and amp[1] < 0.05 < 1 < amp[0] < 10 < 100 < amp[2]
    assert sum(CO.plans(0)["long"]) == CO.LONG_FRAMES == 4096 and set(CO.plans(0)["long"]) == {16}


def test_fp32_model_stays_four_times_inside():
    fig = CO.model_figures(torch.float32)
    for (ci, name), e in sorted(fig.items()):
        print("case %d %-4s fp32 model %.3e" % (ci, name, e))
    worst = max(fig.values())
    print("largest %.3e  FP32_FIGURE %.3e  LIMIT %.0e" % (worst, CO.FP32_FIGURE["stack_y_cum"], CO.LIMIT["stack_y_cum"]))
    assert worst <= CO.LIMIT["stack_y_cum"] / 4
    assert worst <= CO.FP32_FIGURE["stack_y_cum"] * 1.01           # the recorded figure is this machine-independent arithmetic's
    assert 4 * CO.FP32_FIGURE["stack_y_cum"] <= CO.LIMIT["stack_y_cum"] < 8 * CO.FP32_FIGURE["stack_y_cum"]


@pytest.mark.parametrize("wrong", CO.WRONG)
def test_every_defect_exceeds_the_limit(wrong):
    fig = CO.model_figures(F64, wrong)
    over = {k: e for k, e in fig.items() if e > CO.LIMIT["stack_y_cum"]}
    print("%-20s over the limit in %d of %d runs, largest %.2e, smallest %.2e" % (wrong, len(over), len(fig), max(fig.values()), min(fig.values())))
    assert over, (wrong, fig)
    if wrong != "pad_columns_counted":                                # (the long plan has no call below 16 frames)
        assert len(over) == len(fig), (wrong, fig)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
NEW = ["ctn_stream_cum_bytes", "ctn_stream_tcn_cumln", "ctn_stream_tcn_cumln_ragged", "ctn_stream_cum_reset_slots"]


def test_header_declares_the_cumulative_entry_points():
    protos = _lib.parse_header()
    assert not [n for n in NEW if n not in protos]
    assert protos["ctn_stream_cum_bytes"][0] is ctypes.c_size_t and protos["ctn_stream_cum_bytes"][2] == ["M", "nblocks"]
    plain, rag = protos["ctn_stream_tcn_cln"][2], protos["ctn_stream_tcn_cln_ragged"][2]
    assert protos["ctn_stream_tcn_cumln"][2] == plain[:5] + ["cum"] + plain[5:]
    assert protos["ctn_stream_tcn_cumln_ragged"][2] == rag[:5] + ["cum"] + rag[5:]
    assert protos["ctn_stream_cum_reset_slots"][2] == ["cum", "slots", "nslots", "M", "nblocks", "stream"]
    assert ctn.lib.ctn_stream_cum_bytes(3, 2) == 2 * 3 * 2 * 2 * 32 and ctn.lib.ctn_stream_cum_bytes(0, 2) == 0


def test_bad_arguments_return_error_codes_and_launch_nothing():
    # every check sits in front of the first launch, so this is safe without a GPU (fake non-null pointers are never read)
    lib, err = ctn.lib, ctn.lib.ctn_last_error
    d, p = (ctypes.c_int * 2)(1, 2), 4096
    assert lib.ctn_stream_tcn_cumln(p, d, 2, p, p, p, 1, 16, 32, 3, 17, 32, 0) == -1 and b"at most 16 frames" in err()
    assert lib.ctn_stream_tcn_cumln(p, d, 2, p, p, 0, 1, 16, 32, 3, 16, 16, 0) == -1 and b"cum" in err()
    assert lib.ctn_stream_tcn_cumln(p, d, 2, p, p, p + 8, 1, 16, 32, 3, 16, 16, 0) == -1 and b"16-byte aligned" in err()
    assert lib.ctn_stream_tcn_cumln(p, d, 2, p, p, p, 1, 16, 32, 3, 9, 8, 0) == -1 and b"max_frames" in err()
    assert lib.ctn_stream_tcn_cumln(p, d, 2, 0, p, p, 1, 16, 32, 3, 8, 16, 0) == -1 and b"null" in err()
    assert lib.ctn_stream_tcn_cumln(p, d, 2, p, p, p, 1, 16, 40, 3, 8, 16, 0) == -1 and b"multiples of 16" in err()
    # the cumulative LDS bound: (B + H) * 64 + 4480 bytes; B + H = 944 fits (64896 bytes), 960 does not, though the cLN call takes it
    assert lib.ctn_stream_tcn_cumln(p, d, 2, p, p, p, 1, 512, 448, 3, 8, 16, 0) == -1 and b"fp64 partial sums" in err()
    assert lib.ctn_stream_tcn_cumln_ragged(p, d, 2, p, p, p, 0, p, 1, 16, 32, 3, 8, 16, 0) == -1 and b"tab" in err()
    assert lib.ctn_stream_tcn_cumln_ragged(p, d, 2, p, p, p, p, 0, 1, 16, 32, 3, 8, 16, 0) == -1 and b"pos" in err()
    assert lib.ctn_stream_tcn_cumln_ragged(p, d, 2, p, p, p, p, p, 1, 16, 32, 3, 17, 32, 0) == -1 and b"at most 16 frames" in err()
    assert lib.ctn_stream_tcn_cumln_ragged(p, d, 2, p, p, 0, p, p, 1, 16, 32, 3, 8, 16, 0) == -1 and b"cum" in err()
    one = (ctypes.c_int * 1)
    assert lib.ctn_stream_cum_reset_slots(0, one(0), 1, 4, 2, 0) == -1 and b"null" in err()
    assert lib.ctn_stream_cum_reset_slots(p, one(4), 1, 4, 2, 0) == -1 and b"outside 0..3" in err()
    assert lib.ctn_stream_cum_reset_slots(p, one(0), 5, 4, 2, 0) == -1 and b"nslots" in err()
    assert lib.ctn_stream_cum_reset_slots(p + 4, one(0), 1, 4, 2, 0) == -1 and b"aligned" in err()


# ---- the host side of the classes ------------------------------------------------------------------------------------------------------
def _rows(steps):
    return [(f, h, [r[:5] for r in rows]) for f, h, rows in steps]


def test_plan_steps_cuts_at_sixteen_frames():
    F = CUM_STEP
    assert F == 16
    # one slot, not fresh: 1, 16, 17, 40 hops
    assert _rows(plan_steps([1], [False], F)) == [(1, 1, [[1, 1, 0, 1, 0]])]
    assert _rows(plan_steps([16], [False], F)) == [(16, 16, [[16, 16, 0, 1, 0]])]
    assert _rows(plan_steps([17], [False], F)) == [(16, 16, [[16, 16, 0, 1, 0]]), (1, 1, [[1, 1, 16, 1, 16]])]
    assert _rows(plan_steps([40], [False], F)) == [(16, 16, [[16, 16, 0, 1, 0]]), (16, 16, [[16, 16, 16, 1, 16]]), (8, 8, [[8, 8, 32, 1, 32]])]
    # fresh: the first hop only primes the carry
    assert _rows(plan_steps([1], [True], F)) == [(0, 1, [[0, 1, 0, 0, 0]])]
    assert _rows(plan_steps([16], [True], F)) == [(15, 16, [[15, 16, 0, 0, 0]])]
    assert _rows(plan_steps([17], [True], F)) == [(16, 17, [[16, 17, 0, 0, 0]])]
    assert _rows(plan_steps([40], [True], F)) == [(16, 17, [[16, 17, 0, 0, 0]]), (16, 16, [[16, 16, 17, 1, 16]]), (7, 7, [[7, 7, 33, 1, 32]])]
    # all four at once, two of them fresh: no step above 16 frames, every slot's frames add up
    steps = plan_steps([1, 16, 17, 40], [True, False, True, False], F)
    assert [s[0] for s in steps] == [16, 16, 8] and all(r[0] <= F for _, _, rows in steps for r in rows)
    assert [sum(rows[m][0] for _, _, rows in steps) for m in range(4)] == [0, 16, 16, 40]


def _model(norm, causal=True):
    torch.manual_seed(0)
    return ctn.ConvTasNet(32, 20, 16, 32, 3, 2, 1, 2, norm_type=norm, causal=causal)


MAKERS = (lambda m, **k: FusedStreamingSeparator(m, batch=2, **k), lambda m, **k: FusedStreamPool(m, slots=2, **k),
          lambda m, **k: ResamplingStreamPool(m, slots=2, input_rate=16000, **k))


def test_constructors_refuse_a_mode_that_does_not_fit_the_model():
    """The checks come before any device allocation: the models live on the CPU and nothing is built."""
    cum, cln, gln = _model("cumLN"), _model("cLN"), _model("gLN", causal=False)
    for make in MAKERS:
        with pytest.raises(ValueError, match="cumLN") as e:
            make(cum)
        assert "cumulative=True" in str(e.value) and "carry record" in str(e.value) and "16 frames" in str(e.value)
        with pytest.raises(ValueError, match="cumulative=True is for norm_type 'cumLN'"):
            make(cln, cumulative=True)
        with pytest.raises(ValueError, match="cumulative=True is for norm_type 'cumLN'|causal"):
            make(gln, cumulative=True)
        with pytest.raises(ValueError, match="causal"):
            make(gln)
    assert check_fused_model(cum, True) is True and check_fused_model(cln, False) is False
