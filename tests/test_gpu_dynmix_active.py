"""GPU: variable speaker counts in the dynamic mixer (ctn_dynmix_plan_active, ctn_dynmix_mask_active; DynamicMixLoader's
min_speakers) against the count draw restated in dynmix_active_oracle.py, the loader without the argument and the gather of a
caller-written plan; then the pieces together: Solver steps with VarPitCriterion and evaluate_variable on such a loader.

World: 12 speakers with 3 short utterances each, B = 64, C = 3, T = 2000."""
import numpy as np
import pytest
import torch

import dynmix_active_oracle as AO

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import dynmix, rir  # noqa: E402

DEV = "cuda:0"
B, C, T, STEPS = 64, 3, 2000, 4
SEED, RANK = 77, 3


@pytest.fixture(scope="module")
def world():
    rng = np.random.RandomState(5)
    arrays, speakers = [], []
    for u in range(36):
        n = int(rng.randint(2500, 5000))
        x = (rng.randn(n) * rng.uniform(0.02, 0.3)).astype(np.float32)
        arrays.append(x * (1.0 + 0.5 * np.sin(np.arange(n) / 300.0)).astype(np.float32))
        speakers.append("spk%02d" % (u % 12))
    noise = [(rng.randn(n) * 0.1).astype(np.float32) for n in (2600, 4000, 3100)]
    bank = ctn.RirBank.from_arrays(rir.synthetic_bank(4, 8000, rt60=(0.03, 0.08), seed=2), DEV, 8000, early_ms=10.0)
    return dict(corpus=ctn.DeviceCorpus.from_arrays(arrays, speakers, DEV),
                noise=ctn.DeviceCorpus.from_arrays(noise, ["n"] * len(noise), DEV), bank=bank)


def _loader(world, m, **kw):
    return ctn.DynamicMixLoader(world["corpus"], B, T, num_speakers=C, steps_per_epoch=STEPS, seed=SEED, rank=RANK, min_speakers=m, **kw)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                     b.view(torch.int32) if b.dtype == torch.float32 else b)


@pytest.mark.parametrize("m", [1, 2])
def test_counts_plans_and_minibatches(world, m):
    with_m, plain = _loader(world, m), _loader(world, None)
    with_m.dataset.set_epoch(2)
    plain.dataset.set_epoch(2)
    seen = set()
    it_m, it_p = iter(with_m), iter(plain)
    for step in range(STEPS):
        mixture, lengths, sources = next(it_m)
        next(it_p)
        n = with_m.last_active()
        want = AO.counts(SEED, RANK, 2, step, B, C, m)
        assert n.dtype == torch.int32 and np.array_equal(n.cpu().numpy(), want), step
        seen |= set(want.tolist())
        utt, start, q, gain = with_m.last_plan()
        p_utt, p_start, p_q, p_gain = plain.last_plan()
        assert torch.equal(utt, p_utt) and torch.equal(start, p_start) and torch.equal(q, p_q)
        masked = torch.from_numpy(AO.masked(p_gain.cpu().numpy(), want)).to(DEV)
        assert _same(gain, masked)
        silent = torch.arange(C, device=DEV).view(1, C) >= n.view(B, 1)
        assert float((sources.double() ** 2).sum(-1)[silent].sum()) == 0.0
        assert ((sources.double() ** 2).sum(-1)[~silent] > 0).all()
        g_mix, g_src, g_peak = dynmix.gather(world["corpus"], utt, start, masked, T)
        assert _same(mixture, g_mix) and _same(sources, g_src) and _same(with_m.last_peak(), g_peak)
        assert (lengths == T).all()
    assert seen == set(range(m, C + 1))
    with pytest.raises(ValueError, match="min_speakers"):
        plain.last_active()


def test_min_speakers_equal_to_the_speakers_gives_the_bits_of_the_plain_loader(world):
    full, plain = _loader(world, C), _loader(world, None)
    for (m1, _, s1), (m2, _, s2) in zip(full, plain):
        assert _same(m1, m2) and _same(s1, s2)
        assert (full.last_active() == C).all() and _same(full.last_peak(), plain.last_peak())
        assert all(_same(a, b) for a, b in zip(full.last_plan(), plain.last_plan()))


def test_with_speed_perturbation(world):
    speeds = tuple(range(95, 106))
    loader = _loader(world, 1, speeds=speeds)
    for step, (mixture, _, sources) in enumerate(loader):
        if step == 2:
            break
        n = loader.last_active()
        assert np.array_equal(n.cpu().numpy(), AO.counts(SEED, RANK, 0, step, B, C, 1))
        utt, start, q, gain, pct = loader.last_plan()
        assert (gain[torch.arange(C, device=DEV).view(1, C) >= n.view(B, 1)] == 0).all()
        g_mix, g_src, g_peak = dynmix.gather(world["corpus"], utt, start, gain, T, plan_pct=pct)
        assert _same(mixture, g_mix) and _same(sources, g_src) and _same(loader.last_peak(), g_peak)
        assert float((sources.double() ** 2).sum(-1)[gain == 0].sum()) == 0.0


def test_with_noise_and_reverberation(world):
    loader = _loader(world, 1, rirs=world["bank"], noise=world["noise"], snr_db=(0, 10))
    plain = _loader(world, None, rirs=world["bank"], noise=world["noise"], snr_db=(0, 10))
    for step, ((mixture, _, sources), _) in enumerate(zip(loader, plain)):
        if step == 2:
            break
        n = loader.last_active()
        assert np.array_equal(n.cpu().numpy(), AO.counts(SEED, RANK, 0, step, B, C, 1))
        utt, start, q, gain = loader.last_plan()
        assert all(_same(a, b) for a, b in zip((utt, start, q), plain.last_plan()[:3]))
        assert all(_same(a, b) for a, b in zip(loader.last_aug_plan(), plain.last_aug_plan()))     # the other draws are untouched
        plan_rir, noise_utt, noise_start, snr10, ngain = loader.last_aug_plan()
        g_mix, g_src, g_peak = dynmix.gather_aug(world["corpus"], utt, start, gain, T, rirs=world["bank"], plan_rir=plan_rir,
                                                 noise=world["noise"], noise_utt=noise_utt, noise_start=noise_start, ngain=ngain)
        assert _same(mixture, g_mix) and _same(sources, g_src) and _same(loader.last_peak(), g_peak)
        assert float((sources.double() ** 2).sum(-1)[gain == 0].sum()) == 0.0


# ---- end to end --------------------------------------------------------------------------------------------------------------
TINY = dict(N=64, L=20, B=32, H=64, P=3, X=2, R=2)


def _model():
    torch.manual_seed(0)
    return ctn.ConvTasNet(TINY["N"], TINY["L"], TINY["B"], TINY["H"], TINY["P"], TINY["X"], TINY["R"], C).to(DEV)


def test_solver_steps_with_the_varpit_criterion(world, tmp_path):
    """Three steps on one fixed minibatch (reshuffle=False, one step per epoch): the training loss must not go up."""
    from conv_tasnet_amd.optim import FlatAdam
    from conv_tasnet_amd.solver import Solver
    model = _model()
    opt = FlatAdam(model.parameters(), lr=1e-3)
    kw = dict(num_speakers=C, steps_per_epoch=1, rank=0, reshuffle=False, min_speakers=1)
    tr = ctn.DynamicMixLoader(world["corpus"], B, T, seed=31, **kw)
    cv = ctn.DynamicMixLoader(world["corpus"], B, T, seed=32, **kw)
    args = (1, 3, 0, 0, 5, str(tmp_path), 0, "", "final.pth.tar", 1000, 0, 0, "varpit")
    solver = Solver({"tr_loader": tr, "cv_loader": cv}, model, opt, args, criterion=ctn.VarPitCriterion(30.0, 20.0))
    solver.train()
    got = list(solver.iter_losses)
    print("losses (train, validation per epoch):", got)
    assert len(got) == 6 and all(np.isfinite(got))
    assert all(-30.0 - 1e-4 <= v <= 64.0 for v in got), got
    assert got[0] >= got[2] >= got[4], got
    assert np.array_equal(tr.last_active().cpu().numpy(), AO.counts(31, 0, 0, 0, B, C, 1))


def test_evaluate_variable_counts_every_utterance(world, capsys):
    loader = _loader(world, 1)
    confusion, sisnri, inactive_db = ctn.evaluate_variable(_model(), loader, threshold_db=-20.0)
    assert confusion.shape == (C + 1, C + 1) and confusion.dtype == np.int64
    assert int(confusion.sum()) == STEPS * B and int(confusion[0].sum()) == 0
    want = np.bincount(np.concatenate([AO.counts(SEED, RANK, 0, k, B, C, 1) for k in range(STEPS)]), minlength=C + 1)
    assert confusion.sum(1).tolist() == want.tolist()
    assert np.isfinite(sisnri) and np.isfinite(inactive_db)
    out = capsys.readouterr().out
    assert "Speaker count" in out and "Average SISNR improvement" in out and "inactive references" in out
    est = torch.zeros(2, C, 50, device=DEV)
    est[0, 0] = 1.0
    est[1] = 0.5
    assert ctn.count_sources(est, torch.ones(2, 50, device=DEV), torch.tensor([50, 50], device=DEV)).tolist() == [1, 3]
