"""No GPU: tests/stream_oracle.py is the operation the project means, its cases reach the seams of csrc/ctn_stream.hip that they are
listed for, and its limits tell fp32 rounding from a defect.

oracle.ctn_oracle expresses every config asked of it here (P = 2 / 3, L = 16 / 20, C = 1 / 3, both mask non-linearities, two
repeats); what it cannot express is a dilation list other than 1, 2, 4, ... per repeat, so the dilations of the GPU cases (5, 40,
8 twice, ...) are checked through the shared depthwise definition only.
"""
import pytest
import torch

import stream_oracle as SO
from oracle import ctn_oracle as O

F64 = torch.float64


# ---- the oracle against the model oracle ---------------------------------------------------------------------------------------------
CONFIGS = [
    O.Config(N=16, L=16, B=16, H=32, P=2, X=2, R=2, C=1, norm_type="cLN", causal=True, mask_nonlinear="relu"),
    O.Config(N=16, L=20, B=32, H=16, P=3, X=3, R=2, C=3, norm_type="cLN", causal=True, mask_nonlinear="softmax"),
    O.Config(N=32, L=20, B=16, H=32, P=3, X=2, R=3, C=1, norm_type="cLN", causal=True, mask_nonlinear="softmax"),
    O.Config(N=16, L=16, B=16, H=16, P=2, X=3, R=2, C=3, norm_type="cLN", causal=True, mask_nonlinear="relu"),
]


@pytest.mark.parametrize("cfg", CONFIGS, ids=["P%d-L%d-C%d-%s-R%d" % (c.P, c.L, c.C, c.mask_nonlinear, c.R) for c in CONFIGS])
def test_chained_calls_equal_the_model_oracle(cfg):
    """front -> tcn -> back over uneven chunks, then the carry as flush == ctn_oracle.forward of the whole signal, to 1e-12."""
    g = torch.Generator().manual_seed(11 + cfg.P + cfg.L + cfg.C)
    sd = {}
    for k, shape in O.param_shapes(cfg).items():
        if shape == (1,):
            sd[k] = torch.tensor([SO.A1 if ".net.1." in k and ".net.3." not in k else SO.A2], dtype=F64)
        elif k.endswith("gamma"):
            sd[k] = 0.5 + torch.rand(shape, generator=g, dtype=F64)
        elif k.endswith("beta"):
            sd[k] = 0.3 * torch.randn(shape, generator=g, dtype=F64)
        else:
            sd[k] = torch.randn(shape, generator=g, dtype=F64) / shape[1] ** 0.5
    S, M, plan = cfg.L // 2, 2, (1, 5, 16, 2, 17, 3, 1, 9)
    K = sum(plan)
    mix = torch.randn(M, (K + 1) * S, generator=g, dtype=F64)
    ref = O.forward(cfg, sd, mix)
    s, outs, t0 = SO.Stream(SO.params_from_state_dict(cfg, sd), M), [], 0
    for n in plan:
        w, y = s.front(mix[:, t0 * S:(t0 + n + 1) * S], n)
        out, carry = s.back(s.tcn(y, n), w)
        outs.append(out)
        t0 += n
    got = torch.cat(outs + [carry], 2)
    assert got.shape == ref.shape
    err = float((got - ref).abs().max() / ref.abs().max())
    print("chained oracle against ctn_oracle.forward: %.2e of max |ref|" % err)
    assert err <= 1e-12


# ---- the seams are real ----------------------------------------------------------------------------------------------------------------
# the constants of csrc/ctn_stream.hip, as plain integers
TC, NT, NW = 16, 1024, 16           # frame columns per tile, threads per workgroup, waves per workgroup
MAX_LDS = 64 * 1024


def batches(G, ntile):
    """gemm_rows: the k groups of one chain in batches of 16 (one row tile per wave only) / 8 / 4 / 2 / 1."""
    out, g = [], 0
    if ntile == 1:
        while g + 16 <= G:
            out.append(16)
            g += 16
    while g + 8 <= G:
        out.append(8)
        g += 8
    for nb in (4, 2, 1):
        if g + nb <= G:
            out.append(nb)
            g += nb
    assert g == G
    return tuple(out)


def gemm_forms(Rt, G):
    """tile_gemm -> [(row tiles per wave, batch decomposition)]: pairs (and a lone last tile if the count is odd) from 32 row tiles on."""
    if Rt >= 2 * NW:
        return [(2, batches(G, 2))] + ([(1, batches(G, 1))] if Rt % 2 else [])
    return [(1, batches(G, 1))]


def dw_elements(H):
    """-> (elements per thread, the NI of tile_dw_to, whether a thread's last element is clamped)."""
    ni = -(-H * TC // NT)
    NI = 1 if ni <= 1 else 4 if ni <= 4 else 8 if ni <= 8 else 16
    return ni, NI, NI * NT > H * TC


def split(Rt, M):
    """tcn_cln_launch + stream_rows_a / _b -> (nsplit, empty slices)."""
    nsplit = max(1, min(Rt, 16, 256 // M))
    per = -(-Rt // nsplit)
    return nsplit, nsplit - -(-Rt // per)


def stack_seams(c, M=SO.M_TEST):
    """Everything that the listed seams of a stack case are asserted from, computed from the case's numbers alone."""
    s = set()
    g1, g2, rt1, rt2 = c.B // 16, c.H // 16, c.H // 16, c.B // 16          # W1 [H, B], W2 [B, H]
    rows = [batches(g1, 1), batches(g2, 1)]                                # the row-split form: one row tile per wave
    stage = gemm_forms(rt1, g1) + gemm_forms(rt2, g2)                      # the stage form
    for G in (g1, g2):
        s.add("G%d" % G)
    if rt1 == 1 and rt2 == 1:
        s.add("one_tile")
    for nt, dec in stage:
        if nt == 2 and len(dec) > 1:
            s.add("two_tile_mixed")
    if (rt1 >= 2 * NW and rt1 % 2) or (rt2 >= 2 * NW and rt2 % 2):
        s.add("two_tile_odd")
    ni, NI, clamp = dw_elements(c.H)
    s.add("NI%d" % NI)
    if clamp:
        s.add("NI%d_clamp" % NI)
    s.add("NI%d_%s_per_thread" % (NI, {1: "one", 2: "two", 3: "three", 4: "four"}.get(ni, str(ni))))
    if c.P != 3:
        s.add("P%d" % c.P)
    if c.P == 8 and (c.P - 1) * max(c.dil) == 14:
        s.add("P8_fourteen_back")
    if any(0 < (c.P - 1 - t) * d < TC for d in c.dil for t in range(c.P)):
        s.add("tap_inside_tile")
    if TC in c.dil:
        s.add("dilation_one_tile")
    if any(d > c.max_frames for d in c.dil):
        s.add("dilation_beyond_max_frames")
    if any(SO.ring_len(c.P, d, c.max_frames) == (c.P - 1) * d + c.max_frames for d in c.dil):
        s.add("ring_no_slack")
    if split(rt1, M)[1] or split(rt2, M)[1]:
        s.add("empty_slices")
    return s, {"rows": rows, "stage": stage, "dw": (ni, NI, clamp), "split": (split(rt1, M), split(rt2, M)),
               "rings": [SO.ring_len(c.P, d, c.max_frames) for d in c.dil]}


def stack_lds(c):
    return ((c.B + c.H) * TC + (NT // TC) * TC) * 4


def front_lds(N, L, B):
    return ((-(-L // 16) * 16 + N + B) * TC + (NT // TC) * TC) * 4


def back_lds(N, L, B, C):
    return (B + C * N + C * (-(-L // 16) * 16)) * TC * 4


def test_every_stack_case_reaches_the_seams_it_is_listed_for():
    decs = set()
    for ci, c in enumerate(SO.STACK_CASES):
        have, detail = stack_seams(c)
        print("stack %d %s: %s" % (ci, tuple(c[:5]), detail))
        assert set(c.seams) <= have, (ci, set(c.seams) - have)
        assert stack_lds(c) <= MAX_LDS and c.B % 16 == 0 and c.H % 16 == 0 and 1 <= c.P <= 8
        decs |= set(detail["rows"]) | {d for _, d in detail["stage"]}
        plan = SO.stack_plan(c)
        assert {1, 15, 16}.issubset(plan) and c.max_frames in plan and max(plan) <= c.max_frames
        assert (17 in plan) == (c.max_frames >= 17)               # a chunk of 17 is one call where max_frames allows it, else 16 + 1
        assert sum(plan) >= 3 * max(detail["rings"]) and sum(SO.stack_plan(c, 1)) == sum(plan) and SO.stack_plan(c, 1) != plan
        assert max(SO.stack_plan(c, 1)) <= c.max_frames and min(SO.stack_plan(c, 1)) >= 1
    # each value of the issue's list appears in at least one case
    assert {(1,), (2, 1), (4, 1), (4, 2, 1), (8, 4, 2, 1), (16, 8, 4, 2, 1), (16, 16, 1)} <= decs, decs
    listed = set().union(*(c.seams for c in SO.STACK_CASES))
    assert {"two_tile_odd", "two_tile_mixed", "NI1", "NI1_clamp", "NI4", "NI4_clamp", "NI16", "NI16_clamp", "P1", "P2", "P8",
            "ring_no_slack", "empty_slices"} <= listed
    # the case with the lone last tile: 33 row tiles of W1 in pairs + 1, its W2 chain 16 + 16 + 1, 5 of 16 slices empty, ring 32
    c = SO.STACK_CASES[4]
    d = stack_seams(c)[1]
    assert gemm_forms(33, 1) == [(2, (1,)), (1, (1,))] and d["rows"][1] == (16, 16, 1) and d["split"][0] == (16, 5) and d["rings"] == [32, 32]
    assert (c.P - 1) * c.dil[0] + c.max_frames == 32
    # the 32-row-tile W2 in the two-tile form at G = 15
    assert gemm_forms(SO.STACK_CASES[5].B // 16, SO.STACK_CASES[5].H // 16)[0] == (2, (8, 4, 2, 1))
    # the forms of the bitwise tests: 129 streams leave no room for two workgroups per stream; 100 streams leave room for exactly two
    assert 256 // 129 < 2 and split(33, 100) == (2, 0) and split(1, 100) == (1, 0) and split(33, 1) == (16, 5)


def test_front_and_back_cases_reach_their_seams_inside_the_lds_limit():
    for N, L, B in SO.FRONT_CASES:
        assert front_lds(N, L, B) <= MAX_LDS and N % 16 == 0 and B % 16 == 0 and L % 4 == 0, (N, L, B)
    assert {L for _, L, _ in SO.FRONT_CASES} == {4, 16, 20, 40}
    N, L, B = SO.FRONT_CASES[3]
    Lp = -(-L // 16) * 16
    assert Lp == 48 and gemm_forms(N // 16, Lp // 16) == [(2, (2, 1)), (1, (2, 1))] and gemm_forms(B // 16, N // 16) == [(1, (16, 16, 1))]
    assert -(-16 // 16) * 16 == 16                                  # L = 16: no zero rows in the packed U
    assert {1, 16, 17, 33} == set(SO.FRONT_FRAMES)
    for N, L, B, C, soft in SO.BACK_CASES:
        assert back_lds(N, L, B, C) <= MAX_LDS and 1 <= C <= 8 and N % 16 == 0 and B % 16 == 0 and L % 4 == 0, (N, L, B, C)
    assert {C for _, _, _, C, _ in SO.BACK_CASES} == {1, 2, 3, 8} and {s for *_, s in SO.BACK_CASES} == {True, False}
    N, L, B, C, soft = SO.BACK_CASES[2]
    assert soft and gemm_forms(C * N // 16, B // 16) == [(2, (1,)), (1, (1,))]           # the mask GEMM: 33 row tiles
    assert len(SO.BACK_FRAMES) >= 4 and {1, 16, 17, 33} == set(SO.BACK_FRAMES)
    N, L, B, C, soft = SO.RAGGED_ENDS
    assert front_lds(N, L, B) <= MAX_LDS and back_lds(N, L, B, C) <= MAX_LDS
    assert SO.ragged_counts(17) == [17, 0, 1, 7, 22, -3]


def test_inputs_are_distinguishable_and_away_from_eps():
    """alpha1 != alpha2; the norms' parameters away from 1 / 0 and from each other; taps not symmetric; every cLN column's variance
    at least 1e-2 -- a million eps -- except the quiet stream of FRONT_QUIET, which is there for the eps-outside-the-root model: its
    smallest variance is 2.3e-6, 225 eps (eps moves 1 / sqrt(var + eps) by 0.2 % there, 2000x the limit; fp32 rounding of the
    variance itself is 1e-7 relative as everywhere)."""
    assert SO.A1 != SO.A2
    smallest, quiet = float("inf"), float("inf")
    for ci, c in enumerate(SO.STACK_CASES):
        p, y = SO.stack_inputs(ci)
        for b in p.blocks:
            assert float((b.g1 - b.g2).abs().min()) > 0.1 and float((b.g1 - 1).abs().min()) > 0.05 and float((b.g2 - 1).abs().min()) > 0.15
            assert float((b.b1 - b.b2).abs().mean()) > 0.2
            if c.P > 1:
                assert float((b.D - b.D.flip(1)).abs().amax(1).median()) > 0.3     # (a reversal is caught: test_limits_catch_defects)
        _, s = SO.stack_model(ci, F64)
        smallest = min(smallest, float(s.min_var.min()))
    for case in SO.FRONT_CASES:
        p, x = SO.front_inputs(*case)
        s = SO.Stream(p, x.shape[0])
        s.front(x, max(SO.FRONT_FRAMES))
        if case == SO.FRONT_QUIET:
            quiet = float(s.min_var[1])
            smallest = min(smallest, float(s.min_var[0]))
        else:
            smallest = min(smallest, float(s.min_var.min()))
    print("smallest cLN column variance: %.3e; quiet stream: %.3e = %.0f eps" % (smallest, quiet, quiet / SO.EPS))
    assert smallest >= 1e-2
    assert 100 * SO.EPS <= quiet <= 1e-4


def test_softmax_cases_hold_the_edge_columns():
    for case in SO.BACK_CASES:
        p, y, w, _ = SO.back_inputs(*case)
        if not p.softmax:
            continue
        N, C = case[0], case[3]
        score = torch.matmul(p.Wm.double(), y.double()).view(y.shape[0], C, N, -1)
        assert set(score[0, :, :, 0].abs().unique().tolist()) == {80.0}
        assert float(score[0, :, :, 1].abs().max()) == 0.0
        if C > 1:
            assert float(score[0, :, :, 0].amax(0).min()) == 80.0 and float(score[0, :, :, 0].amin(0).max()) == -80.0
        ref = SO.back_reference(case)
        assert float((ref[0][0][0, :, :, 1] * C).sub(torch.matmul(p.V.double(), w[0, :, 1].double())).abs().max()) < 1e-12


# ---- the limits hold for the right reason -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fp32_figures():
    return SO.model_figures(torch.float32)


def test_limits_are_four_times_the_fp32_model(fp32_figures):
    """LIMIT[kind] = 4 x the fp32 model's largest figure, rounded up to one significant digit; the model stays inside LIMIT / 4."""
    for kind, per_case in sorted(fp32_figures.items()):
        worst = max(per_case.values())
        print("fp32 model %-8s largest %.3e (recorded %.2e)  limit %.0e" % (kind, worst, SO.FP32_FIGURE[kind], SO.LIMIT[kind]))
        assert worst <= SO.LIMIT[kind] / 4, (kind, per_case)
        assert abs(worst - SO.FP32_FIGURE[kind]) <= 0.05 * SO.FP32_FIGURE[kind], (kind, worst)
        q = 4 * SO.FP32_FIGURE[kind]
        digit = 10.0 ** torch.tensor(q, dtype=F64).log10().floor().item()
        assert abs(SO.LIMIT[kind] - -(-q // digit) * digit) < 1e-12 * digit, (kind, q)
    assert set(fp32_figures) == set(SO.LIMIT)


@pytest.mark.parametrize("wrong", SO.WRONG)
def test_limits_catch_defects(wrong):
    """Every wrong model misses a limit by 10x or more on at least one case of the GPU lists."""
    fig = SO.model_figures(F64, wrong)
    worst = max((max(per_case.values()) / SO.LIMIT[kind], kind) for kind, per_case in fig.items())
    print("%-20s misses %s by %.1ex" % (wrong, worst[1], worst[0]))
    assert worst[0] >= 10.0, fig
