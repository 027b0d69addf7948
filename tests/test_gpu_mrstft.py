"""The multi-resolution STFT loss on the GPU (csrc/ctn_mrstft.hip, mrstft.mrstft_pairs, cal_mrstft_loss, MrStftPitCriterion) against
the numpy fp64 oracle of mrstft_oracle.py: the terms and est.grad at every supported n_fft and at the seams of the framing, exact
zeros, isolation from what lies beyond the lengths, batch invariance, the PIT pairing at C = 3, the Solver criterion and train.py.

The limits.  Terms: |gpu - oracle| <= 1e-9 max(1, |v|).  The fp64 FFT's error is about log2(n_fft) 2^-53 of the frame's norm:
<~ 3e-14 absolute per magnitude for unit-scale input and 1200 taps; on the log of a magnitude at the clamp floor sqrt(eps) = 3.2e-4
that is amplified to <~ 1e-10; the limit carries a 10x margin over that bound.  Gradient: every entry within one fp32 ulp of the
oracle's fp64 gradient rounded to fp32 (the device rounds an fp64 sum once) plus 1e-9 of the row's largest entry.  Observed on an
MI355X: terms within 2.4e-15, every gradient entry equal to the rounded oracle's.  Every test
prints the largest deviation it saw before it asserts.  The conditions on the shared inputs are asserted here and, without a GPU,
in test_mrstft_cpu.py."""
import numpy as np
import pytest
import torch

import bss_oracle as BO
import mrstft_oracle as MO

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd.mrstft import MrStftPitCriterion, cal_mrstft_loss, combine, mrstft_pairs  # noqa: E402
from conv_tasnet_amd.stoi import cal_stoi_loss  # noqa: E402

DEV = "cuda:0"
LIMIT_TERM = 1e-9
LIMIT_GRAD = 1e-9
G = (1.0, 0.75, 0.5)           # upstream weights of (sc, logmag, linmag): every term takes part in the gradient


def _run(ref, est, lens, eo, res, g=G):
    """(terms [B,C,R,3], est.grad [B,E,T]) of sum(g . terms) on the GPU; numpy in, numpy out"""
    rt = torch.from_numpy(np.ascontiguousarray(ref)).to(DEV)
    et = torch.from_numpy(np.ascontiguousarray(est)).to(DEV).requires_grad_(True)
    t = mrstft_pairs(rt, et, torch.tensor(lens, device=DEV), torch.tensor(eo, dtype=torch.int32, device=DEV), res)
    (t * torch.tensor(g, dtype=torch.float64, device=DEV)).sum().backward()
    return t.detach().cpu().numpy(), et.grad.cpu().numpy()


def _term_dev(got, want):
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())


def _grad_dev(got, want):
    """largest |got - fp32(want)| / (ulp(fp32(want)) + LIMIT_GRAD max |row|) over [.., T] rows: the limit is 1"""
    w32 = want.astype(np.float32)
    lim = np.spacing(np.abs(w32)).astype(np.float64) + LIMIT_GRAD * np.abs(want).max(axis=-1, keepdims=True)
    return float((np.abs(got.astype(np.float64) - w32.astype(np.float64)) / np.maximum(lim, 1e-300)).max())


@pytest.mark.parametrize("name", sorted(MO.CASES))
def test_terms_and_gradient_match_the_oracle_at_every_seam(name):
    """Every n_fft from 64 to 2048, win = n_fft, win < n_fft, an odd win, hop > win, hop = 1, R = 1 and R = 8, lengths at the
    framing's seams, E != C with two references on one estimate row and a row nobody chose: see mrstft_oracle.CASES."""
    res, lens, C, E, T, eo, seed = MO.CASES[name]
    MO.conditions([r for r in MO.case_runs(name, G).values() if r["frames"]])
    ref, est = MO.case_inputs(name)
    want_t, want_g = MO.case_expected(name, G)
    terms, g = _run(ref, est, lens, eo, res)
    assert terms.dtype == np.float64 and terms.shape == (len(lens), C, len(res), 3) and g.dtype == np.float32 and g.shape == est.shape
    dt, dg = _term_dev(terms, want_t), _grad_dev(g, want_g)
    print("%s: largest term deviation %.3g (limit %.0e), largest gradient deviation / limit %.3g" % (name, dt, LIMIT_TERM, dg))
    assert dt <= LIMIT_TERM and dg <= 1.0
    for b, n in enumerate(lens):
        assert not g[b, :, n:].any()                                     # exactly zero beyond the length
        chosen = {eo[b][c] for c in range(C)}
        for e in range(E):
            live = e in chosen and any(n > r[0] // 2 for r in res)
            assert g[b, e, :n].any() == live                             # ... and for a row nobody chose
        for r, rr in enumerate(res):
            if n <= rr[0] // 2:                                          # an empty cell, beside live ones of the same call
                assert not terms[b, :, r].any()
            else:
                assert (terms[b, :, r] > 0).all()
    if name == "seams":
        # hop > win_length (resolution 7): samples under no frame get nothing from it.  Alone, its gradient is exactly zero there.
        only = ((128, 200, 100),)
        _, g7 = _run(ref[:1], est[:1], lens[:1], eo[:1], only)
        covered = np.zeros(T + 128, dtype=bool)
        for f in range(1 + lens[0] // 200):
            covered[f * 200 + 14:f * 200 + 114] = True                   # padded positions, window offset (128 - 100) / 2
        direct = covered[64:64 + T]
        hit = direct.copy()
        hit[1:65] |= covered[63::-1][:64]                                # mirror images before sample 0
        tail = covered[64 + T:]                                          # padded positions beyond sample n - 1, n = T
        hit[T - 2:T - 2 - tail.shape[0]:-1] |= tail
        assert (~hit).sum() > 1000 and not g7[0, 2][~hit].any() and (g7[0, 2][hit] != 0).mean() > 0.95


def test_empty_cells_and_a_silent_batch_give_exact_zeros():
    """n = n_fft / 2 and n = 0 for every resolution of the call: terms and gradient all zero, nothing faults."""
    ref, est = MO.signals(21, 1, 1, 256)
    terms, g = _run(ref[None], est[None], [32], [[0]], ((64, 16, 48), (128, 32, 100)))
    assert not terms.any() and not g.any()
    terms, g = _run(ref[None], est[None], [0], [[0]], ((64, 16, 48),))
    assert not terms.any() and not g.any()


def test_nothing_beyond_the_lengths_is_read_and_the_estimate_is_not_modified():
    res, lens, C, E, T, eo, seed = MO.CASES["seams"]
    ref, est = MO.case_inputs("seams")
    clean = _run(ref, est, lens, eo, res)
    rn, en = ref.copy(), est.copy()
    for b, n in enumerate(lens):
        rn[b, :, n:] = np.nan
        en[b, :, n:] = np.nan
    rt, et = torch.from_numpy(rn).to(DEV), torch.from_numpy(en).to(DEV).requires_grad_(True)
    keep = et.detach().clone()
    t = mrstft_pairs(rt, et, torch.tensor(lens, device=DEV), torch.tensor(eo, dtype=torch.int32, device=DEV), res)
    (t * torch.tensor(G, dtype=torch.float64, device=DEV)).sum().backward()
    assert torch.equal(et.detach().isnan(), keep.isnan()) and torch.equal(et.detach().nan_to_num(), keep.nan_to_num())
    terms, g = t.detach().cpu().numpy(), et.grad.cpu().numpy()
    assert np.isfinite(terms).all() and np.isfinite(g).all()
    assert np.array_equal(terms, clean[0]) and np.array_equal(g, clean[1])
    with pytest.raises(ValueError):
        mrstft_pairs(rt.requires_grad_(True), et, torch.tensor(lens, device=DEV), torch.tensor(eo, dtype=torch.int32, device=DEV), res)


def test_a_pair_is_bitwise_the_same_alone_in_a_batch_and_run_to_run():
    res, lens, C, E, T, eo, seed = MO.CASES["seams"]
    ref, est = MO.case_inputs("seams")
    terms, g = _run(ref, est, lens, eo, res)
    again = _run(ref, est, lens, eo, res)
    assert np.array_equal(terms, again[0]) and np.array_equal(g, again[1])
    for u, at in ((1, 3), (0, 2), (3, 0)):
        n = lens[u]
        if n:
            one = _run(ref[u:u + 1, :, :n], est[u:u + 1, :, :n], [n], [eo[u]], res)
            assert np.array_equal(one[0][0], terms[u]) and np.array_equal(one[1][0], g[u, :, :n])
        order = [v for v in range(4) if v != u]
        order.insert(at, u)
        moved = _run(ref[order], est[order], [lens[v] for v in order], [eo[v] for v in order], res)
        assert np.array_equal(moved[0][at], terms[u]) and np.array_equal(moved[1][at], g[u])


def test_forward_and_backward_are_graph_capturable_and_replay_bitwise():
    res, lens, C, E, T, eo, seed = MO.CASES["default"]
    B, R = len(lens), len(res)
    ra = np.ascontiguousarray(np.array(res, dtype=np.int32))
    ref, est = (torch.from_numpy(x).to(DEV) for x in MO.case_inputs("default"))
    ref2, est2 = (torch.from_numpy(np.stack([p[k] for p in [MO.signals(90 + b, C, E, T) for b in range(B)]])).to(DEV) for k in range(2))
    lt, eot = torch.tensor(lens, dtype=torch.int64, device=DEV), torch.tensor(eo, dtype=torch.int32, device=DEV)
    fw = torch.empty(ctn.lib.ctn_mrstft_workspace(B, C, T, R, ra.ctypes.data), dtype=torch.uint8, device=DEV)
    bw = torch.empty(ctn.lib.ctn_mrstft_bwd_workspace(B, C, T, R, ra.ctypes.data), dtype=torch.uint8, device=DEV)
    rbuf, ebuf = ref.clone(), est.clone()
    terms = torch.zeros(B, C, R, 3, dtype=torch.float64, device=DEV)
    gt = torch.tensor(G, dtype=torch.float64, device=DEV).expand(B, C, R, 3).contiguous()
    g = torch.zeros(B, E, T, dtype=torch.float32, device=DEV)

    def run():
        st = torch.cuda.current_stream().cuda_stream
        ctn.lib.call("ctn_mrstft_pairs_fwd", rbuf.data_ptr(), ebuf.data_ptr(), lt.data_ptr(), eot.data_ptr(), B, C, E, T, ra.ctypes.data,
                     R, 1e-7, terms.data_ptr(), fw.data_ptr(), fw.numel(), st)
        ctn.lib.call("ctn_mrstft_pairs_bwd", fw.data_ptr(), fw.numel(), rbuf.data_ptr(), ebuf.data_ptr(), lt.data_ptr(), eot.data_ptr(),
                     B, C, E, T, ra.ctypes.data, R, 1e-7, gt.data_ptr(), g.data_ptr(), bw.data_ptr(), bw.numel(), st)
    run()
    torch.cuda.synchronize()
    first = terms.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    rbuf.copy_(ref2)
    ebuf.copy_(est2)
    graph.replay()
    torch.cuda.synchronize()
    replayed = [terms.clone(), g.clone()]
    run()
    torch.cuda.synchronize()
    assert torch.equal(replayed[0], terms) and torch.equal(replayed[1], g) and not torch.equal(first, terms)


# ---- pairing ----------------------------------------------------------------------------------------------------------------------
RES_SMALL = ((256, 64, 256), (512, 128, 400))


def test_sisnr_pairing_at_three_sources_is_that_of_cal_stoi_loss():
    """Estimates that are a three-cycle of the references: estimate e carries reference CYC[e].  cal_mrstft_loss pairs reference c
    with the estimate that carries it, the inverse of the permutation row, exactly as cal_stoi_loss does; the loss is the oracle's."""
    n, C = 4000, 3
    CYC = [1, 2, 0]
    ref = BO.speech_like(77, C, n)
    rng = np.random.RandomState(78)
    est = np.stack([ref[CYC[e]] + 0.05 * rng.randn(n) for e in range(C)]).astype(np.float32)
    right = [CYC.index(c) for c in range(C)]                             # [2, 0, 1]
    assert right != CYC
    want = [[MO.run(ref[c], est[right[c]], r) for r in RES_SMALL] for c in range(C)]
    MO.conditions([w for row in want for w in row])
    want_t = np.array([[w["terms"] for w in row] for row in want])
    rt, lt = torch.from_numpy(ref[None]).to(DEV), torch.tensor([n], device=DEV)
    et = torch.from_numpy(est[None]).to(DEV)
    _, _, eo_stoi = cal_stoi_loss(rt, et, lt, 8000)
    for perm in ("sisnr", torch.tensor([right], device=DEV)):
        e = et.clone().requires_grad_(True)
        loss, terms, eo = cal_mrstft_loss(rt, e, lt, RES_SMALL, w_sc=1.0, w_log=0.5, w_lin=0.25, perm=perm)
        assert eo.dtype == torch.int32 and eo.tolist() == [right] == eo_stoi.tolist()
        assert _term_dev(terms[0].detach().cpu().numpy(), want_t) <= LIMIT_TERM
        assert abs(float(loss.detach()) - MO.loss(want_t, 1.0, 0.5, 0.25)) <= LIMIT_TERM
        assert torch.equal(e.detach(), et)                               # not masked, not modified
        loss.backward()
        assert torch.isfinite(e.grad).all() and all(e.grad[0, k].abs().max() > 0 for k in range(C))
    wrong = mrstft_pairs(rt, et, lt, torch.tensor([CYC], dtype=torch.int32, device=DEV), RES_SMALL)
    assert (terms.detach()[..., :2] < wrong[..., :2]).all()               # the un-inverted row pairs every reference with another speaker


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
    for crit in (None, MrStftPitCriterion(0.0)):
        m = _model()
        est = m(mixture.to(DEV))
        loss = cal_loss(src.to(DEV), est, lengths.to(DEV))[0] if crit is None else crit(src.to(DEV), est, lengths.to(DEV))
        loss.backward()
        got.append([loss.detach().clone()] + [p.grad.clone() for p in m.parameters()])
    for a, b in zip(*got):
        assert torch.equal(a, b)


def test_criterion_is_cal_loss_plus_the_weighted_spectral_loss_under_the_pit_pairing():
    """Three sources in a three-cycle, one utterance shorter than the tensor: the criterion equals cal_loss + weight *
    cal_mrstft_loss(perm="sisnr") in value, and in the gradient to one fp32 rounding of the sum of the two fp32 gradients."""
    from conv_tasnet_amd.pit_criterion import cal_loss
    n, C, w = 4000, 3, 2.5
    CYC = [1, 2, 0]
    lens = [4000, 3300]
    rng = np.random.RandomState(91)
    refs, ests = [], []
    for b in range(2):
        r = BO.speech_like(80 + b, C, n)
        refs.append(r)
        ests.append(np.stack([r[CYC[e]] + 0.05 * rng.randn(n) for e in range(C)]).astype(np.float32))
    src, lt = torch.from_numpy(np.stack(refs)).to(DEV), torch.tensor(lens, device=DEV)
    ea = torch.from_numpy(np.stack(ests)).to(DEV).requires_grad_(True)
    eb = ea.detach().clone().requires_grad_(True)
    got = MrStftPitCriterion(w, RES_SMALL, w_lin=0.5)(src, ea.clone(), lt)
    got.backward()
    sisnr = cal_loss(src, eb.clone(), lt)[0]
    spec, terms, eo = cal_mrstft_loss(src, eb, lt, RES_SMALL, w_lin=0.5, perm="sisnr")
    assert eo.tolist() == [[CYC.index(c) for c in range(C)]] * 2
    assert torch.equal(spec.detach(), combine(terms.detach(), 1.0, 1.0, 0.5))
    exp = sisnr + (w * spec).to(sisnr.dtype)
    exp.backward()
    assert torch.equal(got.detach(), exp.detach())
    print("largest gradient difference / max |gradient| %.3g" % float((ea.grad - eb.grad).abs().max() / eb.grad.abs().max()))
    assert torch.allclose(ea.grad, eb.grad, rtol=2.0 ** -23, atol=0.0)
    only = torch.autograd.grad(cal_loss(src, eb.clone(), lt)[0], eb)[0]
    assert not torch.equal(only, ea.grad) and not ea.grad[1, :, lens[1]:].any()


def test_solver_step_with_the_criterion_changes_the_parameters(tmp_path):
    from conv_tasnet_amd.optim import FlatAdam
    from conv_tasnet_amd.solver import Solver
    mixture, lengths, src = _train_batches(1)[0]
    grads = {}
    for w in (0.0, 1.0):
        m = _model()
        loss = MrStftPitCriterion(w)(src.to(DEV), m(mixture.to(DEV)), lengths.to(DEV))
        loss.backward()
        grads[w] = next(m.parameters()).grad.clone()
        assert torch.isfinite(loss) and torch.isfinite(grads[w]).all() and grads[w].abs().max() > 0
    assert not torch.equal(grads[0.0], grads[1.0])
    m = _model()
    opt = FlatAdam(m.parameters(), lr=1e-3)
    batches = _train_batches(1)
    args = (1, 1, 0, 0, 5, str(tmp_path / "exp"), 0, "", "final.pth.tar", 1000, 0, 0, "mrstft")
    before = next(m.parameters()).detach().clone()
    s = Solver({"tr_loader": batches, "cv_loader": batches}, m, opt, args, criterion=MrStftPitCriterion(1.0))
    s.train()
    assert np.isfinite(float(s.tr_loss[0])) and np.isfinite(float(s.cv_loss[0]))
    assert not torch.equal(before, next(m.parameters()).detach())


def test_train_cli_with_the_loss_runs_one_epoch(tmp_path, monkeypatch):
    """train.py --loss pit_mrstft --mrstft-weight 1 --tiny on the fixture batches in place of the synthetic loader."""
    from conv_tasnet_amd import train
    batches = _train_batches(2)
    monkeypatch.setattr(train, "SyntheticLoader", lambda n, *a, **k: batches[:n])
    solver = train.main(["--loss", "pit_mrstft", "--mrstft-weight", "1", "--tiny", "--batches", "2", "--batch-size", "2", "--epochs", "1",
                         "--save-folder", str(tmp_path / "exp"), "--model-path", "final.pth.tar"])
    assert isinstance(solver.criterion, MrStftPitCriterion) and solver.criterion.weight == 1.0
    assert solver.criterion.resolutions == MO.DEFAULT_RESOLUTIONS
    assert np.isfinite(float(solver.tr_loss[0])) and np.isfinite(float(solver.cv_loss[0]))
    solver = train.main(["--loss", "pit_mrstft", "--mrstft-weight", "0.5", "--mrstft-resolutions", "256:64:256,512:128:400", "--tiny",
                         "--batches", "1", "--batch-size", "2", "--epochs", "1", "--save-folder", str(tmp_path / "exp2")])
    assert solver.criterion.resolutions == RES_SMALL and np.isfinite(float(solver.tr_loss[0]))
