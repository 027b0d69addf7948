"""The STOI / ESTOI training loss on the GPU (csrc/ctn_stoi_grad.hip, stoi.stoi_pairs, cal_stoi_loss, StoiPitCriterion) against
the float64 torch oracle of stoi_grad_oracle.py: the stages through the C ABI (envelope gradients, 10 kHz sample gradients, the
resampler's adjoint), est.grad end to end at 10, 8 and 16 kHz, the forward bits, exact zeros, batch invariance, a pairing that is
no permutation, the PIT pairing at C = 3 and the Solver criterion.

The limits.  Stages: both sides are fp64 and differ by summation order only: LIMIT_STAGE = 1e-11 of the row maximum (the
project's LIMIT_ENV).  Largest deviations observed on an MI355X: g_env 8.3e-15, g10 4.7e-15, the adjoint's sum 6.8e-16.  End to
end, per element: 2^-23 |g| + LIMIT_STAGE max |g| (the one rounding to fp32 plus the fp64 reordering); observed 0.50 of it.  Every test prints the largest deviation it
saw before it asserts.  The conditions on the shared inputs (clip margin, no zero envelope) are asserted in test_stoi_grad_cpu.py."""
import warnings

import numpy as np
import pytest
import torch

import bss_oracle as BO
import resample_oracle as RO
import stoi_grad_oracle as GO
import stoi_oracle as SO

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd.resample import device_filter  # noqa: E402
from conv_tasnet_amd.stoi import StoiPitCriterion, cal_stoi_loss, stoi_both, stoi_pairs  # noqa: E402

DEV = "cuda:0"
LIMIT_STAGE = 1e-11
LIMIT_D = 1e-10
NB = 15
KEYS = {"stoi": (1.0, 0.0), "estoi": (0.0, 1.0)}


def _ptr(t):
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- the ragged 10 kHz pair rows of the stage tests: computed once, never modified ----------------------------------------------
STAGE = {}


def _stage_rows():
    """Pair rows at the seams: 29 frames left (no segment, beside live rows), exactly one segment, and a row whose 68 segments
    cross the 64-segment workgroup of the score kernel."""
    if STAGE:
        return STAGE
    lens, T = GO.STAGE_LENS, GO.STAGE_T
    ref, est = GO.stage_rows()
    want = {k: [GO.run(ref[p, :n], est[p, :n], 10000, *w) for p, n in enumerate(lens)] for k, w in KEYS.items()}
    STAGE.update(lens=lens, T=T, ref=ref, est=est, want=want)
    return STAGE


def _conditions(runs):
    """On the oracle's side (asserted without a GPU in test_stoi_grad_cpu.py too): no cell within 1e-6 of its clip bound, where
    forward and backward could decide differently from the oracle, and no zero envelope."""
    margin, env_min = min(r["clip_margin"] for r in runs), min(r["env_min"] for r in runs)
    print("smallest clip margin %.3g, smallest envelope %.3g" % (margin, env_min))
    assert margin >= 1e-6 and env_min > 0


def _forward_stages(s):
    P, T = len(s["lens"]), s["T"]
    NF = ctn.lib.ctn_stoi_max_frames(T)
    MF = max(NF - 1, 1)
    rt, et = torch.from_numpy(s["ref"]).to(DEV), torch.from_numpy(s["est"]).to(DEV)
    lt = torch.tensor(s["lens"], dtype=torch.int64, device=DEV)
    en = torch.empty(P, NF, dtype=torch.float64, device=DEV)
    idx = torch.empty(P, NF, dtype=torch.int32, device=DEV)
    K = torch.empty(P, dtype=torch.int32, device=DEV)
    env = torch.zeros(P, 2, NB, MF, dtype=torch.float64, device=DEV)
    ctn.lib.call("ctn_stoi_frames", _ptr(rt), _ptr(lt), P, 1, T, _ptr(en), _ptr(idx), _ptr(K), _stream())
    ctn.lib.call("ctn_stoi_bands", _ptr(rt), _ptr(et), _ptr(lt), _ptr(idx), _ptr(K), P, 1, 1, T, _ptr(env), _stream())
    return et, lt, idx, K, env, MF


def _score_bwd(K, env, w_stoi, w_estoi, P, T, MF):
    ws = torch.empty(ctn.lib.ctn_stoi_score_bwd_workspace(P, T), dtype=torch.uint8, device=DEV)
    g_env = torch.full((P, NB, MF), 7.0, dtype=torch.float64, device=DEV)
    a, b = (torch.tensor(w, dtype=torch.float64, device=DEV) for w in (w_stoi, w_estoi))
    ctn.lib.call("ctn_stoi_score_bwd", _ptr(env), _ptr(K), _ptr(a), _ptr(b), P, T, _ptr(g_env), _ptr(ws), ws.numel(), _stream())
    return g_env


def _bands_bwd(et, lt, idx, K, env, g_env, P, T):
    ws = torch.empty(ctn.lib.ctn_stoi_bands_bwd_workspace(P, T), dtype=torch.uint8, device=DEV)
    g10 = torch.full((P, T), 7.0, dtype=torch.float64, device=DEV)
    ctn.lib.call("ctn_stoi_bands_bwd", _ptr(et), _ptr(lt), _ptr(idx), _ptr(K), _ptr(env), _ptr(g_env), P, T, _ptr(g10), _ptr(ws),
                 ws.numel(), _stream())
    return g10


def test_stage_gradients_of_envelopes_and_samples_through_the_c_abi():
    """g_env of ctn_stoi_score_bwd and g10 of ctn_stoi_bands_bwd, each measure alone and a blend with per-pair weights, against the
    oracle; zeros for the rows without a segment, beyond frame M and beyond each length."""
    s = _stage_rows()
    lens, T, want = s["lens"], s["T"], s["want"]
    P = len(lens)
    Ms = [w["M"] for w in want["stoi"]]
    _conditions([w for w in want["stoi"] if w["M"] >= 30])
    assert Ms[:3] == [29, 29, 30] and 30 <= Ms[3] < 52 and Ms[4] >= 94          # row 3 has removed frames, row 4 more than 64 segments
    et, lt, idx, K, env, MF = _forward_stages(s)
    blend_s, blend_e = [0.25, 1.0, -2.0, 0.5, 3.0], [0.75, 1.0, 0.5, -1.5, 0.125]
    runs = {"stoi": ([1.0] * P, [0.0] * P), "estoi": ([0.0] * P, [1.0] * P), "blend": (blend_s, blend_e)}
    worst_env = worst_g10 = 0.0
    for name, (ws_, we_) in runs.items():
        g_env = _score_bwd(K, env, ws_, we_, P, T, MF)
        g10 = _bands_bwd(et, lt, idx, K, env, g_env, P, T).cpu().numpy()
        g_env = g_env.cpu().numpy()
        for p, n in enumerate(lens):
            if name == "blend":
                exp_env = ws_[p] * want["stoi"][p]["g_env"] + we_[p] * want["estoi"][p]["g_env"]
                exp_g10 = ws_[p] * want["stoi"][p]["g10"] + we_[p] * want["estoi"][p]["g10"]
            else:
                exp_env, exp_g10 = want[name][p]["g_env"], want[name][p]["g10"]
            M = want["stoi"][p]["M"]
            assert (g_env[p, :, M:] == 0).all() and (g10[p, n:] == 0).all()
            if M < 30:
                assert (g_env[p] == 0).all() and (g10[p] == 0).all()
                continue
            assert np.abs(exp_env).max() > 0 and np.abs(exp_g10).max() > 0
            worst_env = max(worst_env, (np.abs(g_env[p, :, :M] - exp_env).max(axis=1) / np.abs(exp_env).max(axis=1)).max())
            worst_g10 = max(worst_g10, np.abs(g10[p, :n] - exp_g10).max() / np.abs(exp_g10).max())
    print("largest g_env deviation / row maximum %.3g, largest g10 deviation / row maximum %.3g" % (worst_env, worst_g10))
    assert worst_env <= LIMIT_STAGE and worst_g10 <= LIMIT_STAGE


@pytest.mark.parametrize("fs,n", [(8000, 8000), (8000, 16003), (16000, 12000)])
def test_resample_adjoint_is_the_transpose_of_the_tap_table(fs, n):
    """ctn_resample_rows_adjoint_f64's fp64 sum against the oracle's R^T, rows shorter than T, two references summed into one
    estimate in c order, and the plain sum at equal rates."""
    up, down = GO._ratio(fs)
    T = n + 9
    T10 = RO.out_len(T, up, down)
    lens = [n, n - 1234]
    rng = np.random.RandomState(n)
    g10 = rng.randn(2, 2, T10)
    eo = np.array([[1, 0], [1, 1]], dtype=np.int32)
    h, W = device_filter(up, down, torch.device(DEV))
    gt, eot, lt = torch.from_numpy(g10).to(DEV), torch.from_numpy(eo).to(DEV), torch.tensor(lens, device=DEV)
    out = torch.full((2, 2, T), 7.0, dtype=torch.float32, device=DEV)
    acc = torch.full((2, 2, T), 7.0, dtype=torch.float64, device=DEV)
    ctn.lib.call("ctn_resample_rows_adjoint_f64", _ptr(gt), _ptr(eot), _ptr(lt), 2, 2, 2, T, T10, up, down, _ptr(h), W, _ptr(out),
                 _ptr(acc), _stream())
    got, got32 = acc.cpu().numpy(), out.cpu().numpy()
    assert np.array_equal(got32, got.astype(np.float32))                 # one rounding
    worst = 0.0
    for b, m in enumerate(lens):
        m10 = RO.out_len(m, up, down)
        exp = np.zeros((2, m))
        for c in range(2):                                               # the references of one estimate, in c order
            exp[eo[b, c]] += GO.adjoint(g10[b, c, :m10], m, up, down)
        assert (got[b, :, m:] == 0).all()
        worst = max(worst, np.abs(got[b, :, :m] - exp).max() / np.abs(exp).max())
    assert (got[1, 0] == 0).all()                                        # an estimate that no reference is paired with
    print("largest adjoint deviation / row maximum %.3g" % worst)
    assert worst <= LIMIT_STAGE
    # equal rates: the sum over the references of an estimate alone
    g1 = rng.randn(2, 2, T)
    g1t = torch.from_numpy(g1).to(DEV)
    ctn.lib.call("ctn_resample_rows_adjoint_f64", _ptr(g1t), _ptr(eot), _ptr(lt), 2, 2, 2, T, T, 1, 1, 0, 0, _ptr(out), _ptr(acc), _stream())
    got = acc.cpu().numpy()
    assert np.array_equal(got[1, 1, :lens[1]], g1[1, 0, :lens[1]] + g1[1, 1, :lens[1]]) and (got[1, 1, lens[1]:] == 0).all()
    assert np.array_equal(got[0, 1, :n], g1[0, 0, :n]) and np.array_equal(got[0, 0, :n], g1[0, 1, :n]) and (got[1, 0] == 0).all()


# ---- end to end -------------------------------------------------------------------------------------------------------------------
WANT = {}


def _case(fs, n, kind, seed, name):
    key = (fs, n, kind, seed, name)
    if key not in WANT:
        ref, est = SO.case_signals(n, kind, seed)
        WANT[key] = (ref, est, [GO.run(ref[c], est[1 - c], fs, *KEYS[name]) for c in range(2)])
    return WANT[key]


def _grad(ref, est, lens, fs, eo, extended, weights=None):
    """(scores, est.grad) of sum(weights * scores) on the GPU; numpy in, numpy out"""
    rt = torch.from_numpy(np.ascontiguousarray(ref)).to(DEV)
    et = torch.from_numpy(np.ascontiguousarray(est)).to(DEV).requires_grad_(True)
    d = stoi_pairs(rt, et, torch.tensor(lens, device=DEV), fs, torch.tensor(eo, dtype=torch.int32, device=DEV), extended)
    (d if weights is None else d * torch.tensor(weights, dtype=torch.float64, device=DEV)).sum().backward()
    return d.detach().cpu().numpy(), et.grad.cpu().numpy()


def _within(got, exp):
    """largest |got - exp| / (2^-23 |exp| + LIMIT_STAGE max |exp|): the end-to-end limit is 1"""
    return float((np.abs(got - exp) / (2.0 ** -23 * np.abs(exp) + LIMIT_STAGE * np.abs(exp).max())).max())


@pytest.mark.parametrize("name", ["stoi", "estoi"])
@pytest.mark.parametrize("fs,n,kind,seed", SO.CASES)
def test_gradient_matches_the_oracle_end_to_end(fs, n, kind, seed, name):
    """est.grad of stoi_pairs with the estimates crossed over (reference c against estimate 1 - c) at 10, 8 and 16 kHz; the
    3100-sample case has no segment: score 1e-5, gradient exactly zero."""
    ref, est, want = _case(fs, n, kind, seed, name)
    d, g = _grad(ref[None], est[None], [n], fs, [[1, 0]], name == "estoi")
    assert g.dtype == np.float32 and g.shape == (1, 2, n)
    dev = max(abs(d[0, c] - want[c][name]) for c in range(2))
    print("largest |d - oracle| %.3g" % dev)
    assert dev <= LIMIT_D
    if n == 3100:
        assert (d == 1e-5).all() and not g.any()
        return
    _conditions(want)
    worst = max(_within(g[0, 1 - c].astype(np.float64), want[c]["g"]) for c in range(2))
    print("largest deviation / limit %.3g" % worst)
    assert worst <= 1.0


# ---- batches ----------------------------------------------------------------------------------------------------------------------
def _ragged(C, E, lens, T, seed, nan=False):
    rng = np.random.RandomState(seed)
    ref = rng.randn(len(lens), C, T).astype(np.float32)
    est = rng.randn(len(lens), E, T).astype(np.float32)
    for b, n in enumerate(lens):
        ref[b, :, :n] = BO.speech_like(seed + b, C, n)
        est[b, :, :n] = 0.5 * ref[b, :, :n].sum(0) + 0.3 * rng.randn(E, n)
        if nan:
            ref[b, :, n:] = np.nan
            est[b, :, n:] = np.nan
    return ref, est


def test_forward_scores_are_bitwise_those_of_stoi_both():
    C, E, T = 2, 3, 8000
    lens = [8000, 3100, 5003, 6000]
    ref, est = _ragged(C, E, lens, T, 8)
    rt, et = torch.from_numpy(ref).to(DEV), torch.from_numpy(est).to(DEV)
    lt = torch.tensor(lens, device=DEV)
    eo = torch.tensor([[2, 0], [1, 1], [0, 2], [2, 2]], dtype=torch.int32, device=DEV)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        both = stoi_both(rt, et, lt, 8000)
        both10 = stoi_both(rt, et, lt, 10000)
    pick = eo.long().unsqueeze(1)                                        # [B,1,C]: entry (b, eo[b,c], c)
    for fs, b in ((8000, both), (10000, both10)):
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)               # the training path reads nothing back to warn about
            for ext in (False, True):
                d = stoi_pairs(rt, et, lt, fs, eo, extended=ext)
                assert d.dtype == torch.float64 and torch.equal(d, b[1 if ext else 0].gather(1, pick)[:, 0])
    assert (both[0][1] == 1e-5).all() and (both[0][[0, 2, 3]] != 1e-5).all()
    with pytest.raises(ValueError):
        stoi_pairs(rt.requires_grad_(True), et, lt, 8000, eo)


@pytest.mark.parametrize("fs", [10000, 8000])
def test_gradient_is_exactly_zero_beyond_lengths_and_for_rows_without_a_segment(fs):
    """NaN beyond every length in both inputs: never read, so nothing but finite numbers and exact zeros come back."""
    lens = [4095, 4096, 4097, 7000] if fs == 10000 else [3100, 3400, 5003, 7990]
    T = 7100 if fs == 10000 else 8000
    ref, est = _ragged(2, 2, lens, T, 31, nan=True)
    for ext in (False, True):
        d, g = _grad(ref, est, lens, fs, [[0, 1], [1, 0], [0, 1], [1, 1]], ext)
        assert np.isfinite(d).all() and np.isfinite(g).all()
        for b, n in enumerate(lens):
            assert not g[b, :, n:].any()
        short = [0, 1] if fs == 10000 else [0]
        assert (d[short] == 1e-5).all() and not g[short].any()
        live = [b for b in range(4) if b not in short]
        assert (d[live] != 1e-5).all() and all(g[b, 1, :lens[b]].any() for b in live)
        assert not g[3, 0].any()                                         # an estimate that no reference is paired with


def test_gradient_is_bitwise_per_utterance_and_reproducible():
    C, T = 2, 8000
    lens = [8000, 3100, 5003, 6000]
    ref, est = _ragged(C, C, lens, T, 8)
    eo = [[1, 0], [0, 1], [1, 0], [0, 1]]
    for fs, ext in ((8000, False), (8000, True), (10000, False), (10000, True)):
        d, g = _grad(ref, est, lens, fs, eo, ext)
        d2, g2 = _grad(ref, est, lens, fs, eo, ext)
        assert np.array_equal(d, d2) and np.array_equal(g, g2)
        assert all(g[u].any() for u in (0, 2, 3))
        for u, pos in ((2, 0), (0, 3)):
            n = lens[u]
            one = _grad(ref[u:u + 1, :, :n], est[u:u + 1, :, :n], [n], fs, [eo[u]], ext)
            assert np.array_equal(one[0][0], d[u]) and np.array_equal(one[1][0], g[u, :, :n])
            order = [v for v in range(4) if v != u]
            order.insert(pos, u)
            moved = _grad(ref[order], est[order], [lens[v] for v in order], fs, [eo[v] for v in order], ext)
            assert np.array_equal(moved[0][pos], d[u]) and np.array_equal(moved[1][pos], g[u])


def test_two_references_paired_with_one_estimate_sum_in_c_order():
    fs, n, kind, seed = SO.CASES[1]
    ref, est = SO.case_signals(n, kind, seed)
    wts = [1.0, -0.5]
    want = [GO.run(ref[c], est[0], fs, 1.0, 0.0) for c in range(2)]
    _conditions(want)
    d, g = _grad(ref[None], est[None], [n], fs, [[0, 0]], False, weights=[wts])
    assert max(abs(d[0, c] - want[c]["stoi"]) for c in range(2)) <= LIMIT_D
    worst = _within(g[0, 0].astype(np.float64), wts[0] * want[0]["g"] + wts[1] * want[1]["g"])
    print("largest deviation / limit %.3g" % worst)
    assert worst <= 2.0 and not g[0, 1].any()
    # ... and it is the sum in c order of the two single-pair fp64 gradients: reference 1 alone, paired with estimate 0
    only1 = _grad(ref[None], est[None], [n], fs, [[1, 0]], False, weights=[[0.0, wts[1]]])[1]
    only0 = _grad(ref[None], est[None], [n], fs, [[0, 1]], False, weights=[[wts[0], 0.0]])[1]
    o0, o1 = only0[0, 0].astype(np.float64), only1[0, 0].astype(np.float64)
    assert (np.abs(g[0, 0] - (o0 + o1)) <= 2.0 ** -23 * (np.abs(o0) + np.abs(o1)) + 1e-30).all()      # three fp32 roundings


def test_forward_and_backward_are_graph_capturable_and_replay_bitwise():
    """ctn_stoi_pairs_fwd / _bwd read nothing back and do not synchronise: captured in a graph, a replay over new samples in the
    same buffers gives the bits of the plain calls."""
    B, C, E, T, fs = 2, 2, 2, 6000, 8000
    lens = [6000, 4500]
    ref, est = _ragged(C, E, lens, T, 51)
    ref2, est2 = _ragged(C, E, lens, T, 52)
    up, down = GO._ratio(fs)
    T10 = RO.out_len(T, up, down)
    h, W = device_filter(up, down, torch.device(DEV))
    lt = torch.tensor(lens, dtype=torch.int64, device=DEV)
    l10 = torch.tensor([RO.out_len(n, up, down) for n in lens], dtype=torch.int64, device=DEV)
    eo = torch.tensor([[1, 0], [0, 0]], dtype=torch.int32, device=DEV)
    r10 = torch.zeros(B, C, T10, dtype=torch.float32, device=DEV)
    e10 = torch.zeros(B, E, T10, dtype=torch.float32, device=DEV)
    fw = torch.empty(ctn.lib.ctn_stoi_pairs_workspace(B, C, T10), dtype=torch.uint8, device=DEV)
    bw = torch.empty(ctn.lib.ctn_stoi_pairs_bwd_workspace(B, C, T10), dtype=torch.uint8, device=DEV)
    d = [torch.zeros(B, C, dtype=torch.float64, device=DEV) for _ in range(2)]
    w = [torch.tensor([[1.0, 0.5], [0.25, 2.0]], dtype=torch.float64, device=DEV), torch.tensor([[0.5, 1.0], [1.0, 0.0]], dtype=torch.float64, device=DEV)]
    g = torch.zeros(B, E, T, dtype=torch.float32, device=DEV)

    def load(r, e):
        r10.copy_(ctn.resample.resample(torch.from_numpy(r).to(DEV), fs, 10000))
        e10.copy_(ctn.resample.resample(torch.from_numpy(e).to(DEV), fs, 10000))

    def run():
        st = _stream()
        ctn.lib.call("ctn_stoi_pairs_fwd", _ptr(r10), _ptr(e10), _ptr(l10), _ptr(eo), B, C, E, T10, _ptr(d[0]), _ptr(d[1]), 0, _ptr(fw),
                     fw.numel(), st)
        ctn.lib.call("ctn_stoi_pairs_bwd", _ptr(fw), fw.numel(), _ptr(w[0]), _ptr(w[1]), _ptr(eo), _ptr(lt), B, C, E, T, T10, up, down,
                     _ptr(h), W, _ptr(g), _ptr(bw), bw.numel(), st)
    load(ref, est)
    run()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    load(ref2, est2)
    graph.replay()
    torch.cuda.synchronize()
    replayed = [x.clone() for x in d + [g]]
    run()
    torch.cuda.synchronize()
    for x, y in zip(replayed, d + [g]):
        assert torch.equal(x, y)
    assert g[1, 0].abs().max() > 0 and not g[1, 1].any() and not g[1, :, lens[1]:].any()


# ---- pairing ----------------------------------------------------------------------------------------------------------------------
def test_pairing_at_three_sources_is_the_inverse_permutation():
    """Estimates that are a three-cycle of the references: estimate e carries reference CYC[e].  The SI-SNR PIT pairing and the
    best-score search both pair reference c with the estimate that carries it; reorder_source's un-inverted rule would not."""
    n, fs, C = 6000, 8000, 3
    CYC = [1, 2, 0]
    ref = BO.speech_like(77, C, n)
    rng = np.random.RandomState(78)
    est = np.stack([ref[CYC[e]] + 0.05 * rng.randn(n) for e in range(C)]).astype(np.float32)
    right = [CYC.index(c) for c in range(C)]                             # [2, 0, 1]
    assert right != CYC
    good = [SO.details(ref[c], est[right[c]], fs) for c in range(C)]
    wrong = [SO.details(ref[c], est[CYC[c]], fs) for c in range(C)]
    mix = ref.sum(0).astype(np.float32)
    anchor = [SO.details(ref[c], mix, fs) for c in range(C)]
    for key in ("stoi", "estoi"):
        assert all(good[c][key] > anchor[c][key] and good[c][key] > wrong[c][key] for c in range(C)), key
    rt, lt = torch.from_numpy(ref[None]).to(DEV), torch.tensor([n], device=DEV)
    anchor_gpu = stoi_both(rt, torch.from_numpy(mix[None, None]).to(DEV), lt, fs)                     # [1,1,C] each
    for perm in ("sisnr", "stoi", torch.tensor([right], device=DEV)):
        for ext in (False, True):
            et = torch.from_numpy(est[None]).to(DEV).requires_grad_(True)
            loss, scores, eo = cal_stoi_loss(rt, et, lt, fs, extended=ext, perm=perm)
            assert eo.dtype == torch.int32 and eo.tolist() == [right]
            key = "estoi" if ext else "stoi"
            assert max(abs(float(scores[0, c].detach()) - good[c][key]) for c in range(C)) <= LIMIT_D
            assert (scores[0].detach() > anchor_gpu[1 if ext else 0][0, 0]).all()
            assert abs(float(loss.detach()) - (1.0 - np.mean([good[c][key] for c in range(C)]))) <= LIMIT_D
            assert torch.equal(et.detach(), torch.from_numpy(est[None]).to(DEV))          # not masked, not modified
            loss.backward()
            assert torch.isfinite(et.grad).all() and all(et.grad[0, e].abs().max() > 0 for e in range(C))


# ---- the criterion ------------------------------------------------------------------------------------------------------------------
def _train_batches(n_batches, B=2, T=4000):
    out = []
    for k in range(n_batches):
        src = np.stack([BO.speech_like(300 + 10 * k + b, 2, T) for b in range(B)]) * np.float32(0.3)
        src = torch.from_numpy(src.astype(np.float32))
        out.append((src.sum(1), torch.tensor([T, T - 500][:B]), src))
    return out


def _model():
    torch.manual_seed(0)
    return ctn.ConvTasNet(32, 20, 16, 32, 3, 2, 1, 2).to(DEV)


def test_criterion_with_weight_zero_is_cal_loss_bitwise():
    from conv_tasnet_amd.pit_criterion import cal_loss
    mixture, lengths, src = _train_batches(1)[0]
    got = []
    for crit in (None, StoiPitCriterion(8000, 0.0)):
        m = _model()
        est = m(mixture.to(DEV))
        loss = cal_loss(src.to(DEV), est, lengths.to(DEV))[0] if crit is None else crit(src.to(DEV), est, lengths.to(DEV))
        loss.backward()
        got.append([loss.detach().clone()] + [p.grad.clone() for p in m.parameters()])
    for a, b in zip(*got):
        assert torch.equal(a, b)


@pytest.mark.parametrize("ext", [False, True])
def test_criterion_is_cal_loss_plus_the_weighted_stoi_loss_under_the_pit_pairing_at_three_sources(ext):
    """Estimates that are a three-cycle of the references (a permutation that is not its own inverse), one utterance shorter than
    the tensor: the criterion equals cal_loss + weight * cal_stoi_loss(perm="sisnr"), in value and in the gradient, which pins
    its inversion of the permutation row and the path through the length-masked estimate.  Both sides add the same two fp32
    gradients (the SI-SNR term's and the score term's under the same upstream weight), so they agree to the last bit or, at the
    most, to one fp32 rounding of the sum."""
    from conv_tasnet_amd.pit_criterion import cal_loss
    n, fs, C, w = 6000, 8000, 3, 7.5
    CYC = [1, 2, 0]
    lens = [6000, 5000]
    rng = np.random.RandomState(91)
    refs, ests = [], []
    for b in range(2):
        r = BO.speech_like(80 + b, C, n)
        refs.append(r)
        ests.append(np.stack([r[CYC[e]] + 0.05 * rng.randn(n) for e in range(C)]).astype(np.float32))
    src, lt = torch.from_numpy(np.stack(refs)).to(DEV), torch.tensor(lens, device=DEV)
    ea = torch.from_numpy(np.stack(ests)).to(DEV).requires_grad_(True)
    eb = ea.detach().clone().requires_grad_(True)
    got = StoiPitCriterion(fs, w, extended=ext)(src, ea.clone(), lt)
    got.backward()
    sisnr = cal_loss(src, eb.clone(), lt)[0]
    stoi_loss, scores, eo = cal_stoi_loss(src, eb, lt, fs, extended=ext, perm="sisnr")
    assert eo.tolist() == [[CYC.index(c) for c in range(C)]] * 2
    exp = sisnr + (w * stoi_loss).to(sisnr.dtype)
    exp.backward()
    assert torch.equal(got.detach(), exp.detach())
    dev = float((ea.grad - eb.grad).abs().max() / eb.grad.abs().max())
    print("largest gradient difference / max |gradient| %.3g" % dev)
    assert torch.allclose(ea.grad, eb.grad, rtol=2.0 ** -23, atol=0.0)
    only = torch.autograd.grad(cal_loss(src, eb.clone(), lt)[0], eb)[0]
    assert not torch.equal(only, ea.grad) and not ea.grad[1, :, lens[1]:].any()
    # the un-inverted row would score every reference against another speaker's estimate
    wrong = stoi_pairs(src, eb.detach(), lt, fs, torch.tensor([CYC] * 2, dtype=torch.int32, device=DEV), ext)
    assert (scores.detach() > wrong).all()


def test_solver_trains_with_the_criterion_and_its_gradient_reaches_the_encoder(tmp_path):
    from conv_tasnet_amd.optim import FlatAdam
    from conv_tasnet_amd.solver import Solver
    mixture, lengths, src = _train_batches(1)[0]
    grads = {}
    for w in (0.0, 10.0):
        m = _model()
        loss = StoiPitCriterion(8000, w)(src.to(DEV), m(mixture.to(DEV)), lengths.to(DEV))
        loss.backward()
        grads[w] = next(m.parameters()).grad.clone()
        assert torch.isfinite(loss) and torch.isfinite(grads[w]).all() and grads[w].abs().max() > 0
    assert not torch.equal(grads[0.0], grads[10.0])
    for ext in (False, True):
        m = _model()
        opt = FlatAdam(m.parameters(), lr=1e-3)
        batches = _train_batches(2)
        args = (1, 1, 0, 0, 5, str(tmp_path / str(ext)), 0, "", "final.pth.tar", 1000, 0, 0, "stoi")
        before = next(m.parameters()).detach().clone()
        s = Solver({"tr_loader": batches, "cv_loader": batches[:1]}, m, opt, args, criterion=StoiPitCriterion(8000, 10.0, extended=ext))
        s.train()
        assert np.isfinite(float(s.tr_loss[0])) and np.isfinite(float(s.cv_loss[0]))
        assert not torch.equal(before, next(m.parameters()).detach())
