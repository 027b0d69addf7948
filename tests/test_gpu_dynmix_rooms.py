"""GPU: simulated rooms in the dynamic mixer -- ctn_dynmix_plan_rooms bitwise against the numpy Philox restatement
(ism_oracle.plan_rooms), same_room=True leaving every other draw of a seed alone, its minibatches bitwise gather_aug over the
plans it reports, a bank refilled in place by a room schedule at set_epoch, and train.py --rirs rooms:G:P --rooms-refresh end to
end with a resumed run.

World: 16 random utterances of 1 .. 2 s over 8 speakers, three noise files, banks of 3 small rooms with 3 or 4 positions at 400
taps (rir.draw_rooms with short reverberation times, so that a bank simulates in milliseconds)."""
import numpy as np
import pytest
import torch

import ism_oracle as IO

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import dynmix, rir  # noqa: E402

DEV = "cuda:0"
SR = 8000
T = 2000
TAPS = 400


def draw(epoch=0, positions=3, seed=5):
    return rir.draw_rooms(3, positions, SR, rt60=(0.05, 0.1), dims=((3, 3, 2.5), (5, 4, 3)), seed=seed, epoch=epoch)


@pytest.fixture(scope="module")
def world():
    rng = np.random.RandomState(3)
    arrays, speakers = [], []
    for u in range(16):
        x = (rng.randn(int(rng.randint(SR, 2 * SR))) * rng.uniform(0.02, 0.3)).astype(np.float32)
        arrays.append(x)
        speakers.append("spk%d" % (u % 8))
    noise_arrays = [(rng.randn(n) * 0.1).astype(np.float32) for n in (5000, 9000, 2500)]
    return dict(corpus=ctn.DeviceCorpus.from_arrays(arrays, speakers, DEV),
                noise=ctn.DeviceCorpus.from_arrays(noise_arrays, ["n"] * 3, DEV),
                bank=ctn.RirBank.from_rooms(draw(), DEV, early_ms=10.0, n_taps=TAPS))


def bits_equal(a, b):
    a, b = (t.cpu().numpy() if torch.is_tensor(t) else t for t in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("B,C,G,P", [(300, 3, 5, 3), (300, 2, 4, 5), (64, 4, 1, 64), (64, 4, 1, 4)])
def test_plan_rooms_is_the_philox_restatement(B, C, G, P):
    seed, rank, epoch, step = (1 << 40) + 12345, 3, 2, 7
    step_word = torch.tensor([step], dtype=torch.int32, device=DEV)
    plan = torch.full((B, C), -1, dtype=torch.int32, device=DEV)
    ctn.lib.call("ctn_dynmix_plan_rooms", seed, epoch, rank, step_word.data_ptr(), B, C, G, P, plan.data_ptr(),
                 torch.cuda.current_stream().cuda_stream)
    want = IO.plan_rooms(seed, rank, epoch, step, B, C, G, P)
    assert bits_equal(plan, want)
    assert int(step_word.item()) == step                                              # read, and left alone
    got = plan.cpu().numpy()
    assert np.all(got // P == (got // P)[:, :1]) and all(len(set(r)) == C for r in (got % P).tolist())


def test_from_rooms_is_the_simulated_bank(world):
    bank, rooms = world["bank"], draw()
    assert bank.positions_per_room == 3 and bank.num_responses == 9 and bank.sample_rate == SR
    h = rir.simulate(rooms, DEV, TAPS).cpu().numpy()
    want = rir.build_tables(list(h), SR, 10.0, True)
    for k in ("bank", "offsets", "lens", "direct", "early"):
        assert bits_equal(getattr(bank, k), want[k]), k
    assert not bank.full_targets and list(want["lens"]) == [TAPS] * 9
    # the direct path of every response is where the geometry puts it
    dist = np.sqrt(np.sum((rooms["src"] - rooms["mic"][:, None, :]) ** 2, axis=-1)).reshape(-1)
    assert np.all(np.abs(want["direct"] - dist * SR / 343.0) <= 1.0)


def test_same_room_needs_a_bank_of_rooms(world):
    flat = ctn.RirBank.from_arrays(rir.synthetic_bank(4, SR, rt60=(0.03, 0.05)), DEV, SR)
    with pytest.raises(ValueError, match="positions_per_room"):
        ctn.DynamicMixLoader(world["corpus"], 4, T, rirs=flat, same_room=True)
    with pytest.raises(ValueError, match="same_room"):
        ctn.DynamicMixLoader(world["corpus"], 4, T, same_room=True)
    with pytest.raises(ValueError, match="positions per room"):                       # four talkers, three positions
        ctn.DynamicMixLoader(world["corpus"], 4, T, num_speakers=4, rirs=world["bank"], same_room=True)
    with pytest.raises(ValueError, match="room_schedule"):
        ctn.DynamicMixLoader(world["corpus"], 4, T, rirs=flat, room_schedule=draw)
    with pytest.raises(ValueError, match="from_rooms"):
        flat.refresh(draw())


@pytest.mark.parametrize("with_noise", [False, True])
def test_same_room_leaves_the_other_draws_alone(world, with_noise):
    kw = dict(num_speakers=3, steps_per_epoch=4, seed=21, rank=1, speeds=range(95, 106), rirs=world["bank"],
              noise=world["noise"] if with_noise else None, snr_db=(-3, 6))
    a = ctn.DynamicMixLoader(world["corpus"], 6, T, **kw)
    b = ctn.DynamicMixLoader(world["corpus"], 6, T, same_room=True, **kw)
    for ld in (a, b):
        ld.set_epoch(2)
    mix, src = (torch.empty(6, T, device=DEV), torch.empty(6, 3, T, device=DEV))
    for step in range(3):
        a.fill(mix, src)
        b.fill(mix, src)
        for x, y, name in zip(a.last_plan(), b.last_plan(), ("utt", "start", "q", "gain", "pct")):
            assert bits_equal(x, y), (step, name)
        pa, pb = a.last_aug_plan(), b.last_aug_plan()
        for x, y, name in zip(pa[1:], pb[1:], ("noise_utt", "noise_start", "snr10", "ngain")):
            assert (x is None and y is None and not with_noise) or bits_equal(x, y), (step, name)
        assert bits_equal(pb[0], IO.plan_rooms(21, 1, 2, step, 6, 3, 3, 3))
        assert not bits_equal(pa[0], pb[0])


@pytest.mark.parametrize("with_noise", [False, True])
def test_same_room_minibatch_is_gather_aug_over_its_plans(world, with_noise):
    bank, noise = world["bank"], world["noise"] if with_noise else None
    ld = ctn.DynamicMixLoader(world["corpus"], 5, T, steps_per_epoch=3, seed=9, rank=0, rirs=bank, noise=noise, same_room=True)
    steps = 0
    for mixture, lengths, sources in ld:
        utt, start, _, gain = ld.last_plan()
        plan_rir, nutt, nstart, _, ngain = ld.last_aug_plan()
        assert bits_equal(plan_rir, IO.plan_rooms(9, 0, 0, steps, 5, 2, 3, 3))
        m, s, peak = dynmix.gather_aug(world["corpus"], utt, start, gain, T, rirs=bank, plan_rir=plan_rir, noise=noise, noise_utt=nutt,
                                       noise_start=nstart, ngain=ngain)
        assert bits_equal(mixture, m) and bits_equal(sources, s) and bits_equal(ld.last_peak(), peak)
        assert float(peak.min()) > 0 and lengths.tolist() == [T] * 5
        steps += 1
    assert steps == 3


def test_room_schedule_refills_the_bank_in_place(world):
    schedule = lambda e: draw(epoch=e, positions=4)
    bank = ctn.RirBank.from_rooms(schedule(0), DEV, early_ms=10.0, n_taps=TAPS)
    cv_bank = ctn.RirBank.from_rooms(schedule(0), DEV, early_ms=10.0, n_taps=TAPS)
    names = ("bank", "offsets", "lens", "direct", "early")
    ptrs = [getattr(bank, k).data_ptr() for k in names]
    before = {k: getattr(bank, k).clone() for k in names}
    tr = ctn.DynamicMixLoader(world["corpus"], 4, T, steps_per_epoch=2, seed=1, rank=0, rirs=bank, same_room=True, room_schedule=schedule)
    cv = ctn.DynamicMixLoader(world["corpus"], 4, T, steps_per_epoch=2, seed=2, rank=0, rirs=cv_bank, same_room=True,
                              room_schedule=schedule, reshuffle=False)
    tr.set_epoch(1)
    cv.set_epoch(1)
    fresh = ctn.RirBank.from_rooms(schedule(1), DEV, early_ms=10.0, n_taps=TAPS)
    for k in names:
        assert bits_equal(getattr(bank, k), getattr(fresh, k)), k
        assert bits_equal(getattr(bank, k), bank.host[k]), k
        assert bits_equal(getattr(cv_bank, k), before[k]), k                           # the fixed validation set keeps its rooms
    assert not bits_equal(bank.bank, before["bank"])
    assert [getattr(bank, k).data_ptr() for k in names] == ptrs
    mixture, _, sources = next(iter(tr))                                               # and the loader mixes with the new rooms
    utt, start, _, gain = tr.last_plan()
    m, s, _ = dynmix.gather_aug(world["corpus"], utt, start, gain, T, rirs=fresh, plan_rir=tr.last_aug_plan()[0])
    assert bits_equal(mixture, m) and bits_equal(sources, s)
    with pytest.raises(ValueError, match="differ"):
        bank.refresh(draw(epoch=1, positions=3))
    full = ctn.RirBank.from_rooms(schedule(0), DEV, early_ms=None, n_taps=TAPS)        # full targets stay full
    full.refresh(schedule(1))
    assert full.full_targets and bits_equal(full.bank, ctn.RirBank.from_rooms(schedule(1), DEV, early_ms=None, n_taps=TAPS).bank)


def test_train_cli_with_simulated_rooms_refreshes_and_resumes(world, tmp_path, monkeypatch):
    """train.py --rirs rooms:3:2 --rooms-refresh, two epochs of 2 steps on the tiny config: same_room on both loaders, the training
    bank holds the rooms of the last epoch, the validation bank rooms of its own that never change, and a run resumed from the
    first epoch's checkpoint draws the uninterrupted run's second epoch."""
    import json
    from scipy.io import wavfile
    from conv_tasnet_amd.train import main
    rng = np.random.RandomState(2)
    infos = []
    for u in range(6):
        x = rng.randn(2 * SR) * 0.1
        p = str(tmp_path / ("%d.wav" % u))
        wavfile.write(p, SR, np.round(x / np.abs(x).max() * 20000.0).astype(np.int16))
        infos.append([p, 2 * SR, "spk%d" % (u % 3)])
    (tmp_path / "tr.json").write_text(json.dumps(infos))
    first = []
    plain_iter = dynmix.DynamicMixLoader.__iter__

    def recorded(self):
        for k, batch in enumerate(plain_iter(self)):
            if k == 0 and self.reshuffle:
                first.append((self.epoch, batch[0].clone(), batch[2].clone(), self.last_aug_plan()[0].cpu()))
            yield batch

    monkeypatch.setattr(dynmix.DynamicMixLoader, "__iter__", recorded)
    flags = ["--dynamic-mix", str(tmp_path / "tr.json"), "--dynamic-mix-cv", str(tmp_path / "tr.json"), "--cv-steps", "1", "--seed", "3",
             "--rirs", "rooms:3:2", "--rt60", "0.05:0.1", "--rooms-refresh", "--rir-early-ms", "10", "--tiny", "--segment-len", "4000",
             "--batch-size", "2", "--steps-per-epoch", "2"]
    solver = main(flags + ["--epochs", "2", "--checkpoint", "--save-folder", str(tmp_path / "full")])
    tr, cv = solver.tr_loader, solver.cv_loader
    assert tr._aug.same_room and cv._aug.same_room and tr.room_schedule is not None and cv.room_schedule is None
    assert tr._aug.rirs is not cv._aug.rirs and tr._aug.rirs.positions_per_room == 2 and tr._aug.rirs.num_responses == 6
    rooms = lambda seed, epoch: rir.draw_rooms(3, 2, SR, rt60=(0.05, 0.1), seed=seed, epoch=epoch)
    assert bits_equal(tr._aug.rirs.bank, ctn.RirBank.from_rooms(rooms(3, 1), DEV, early_ms=10.0, n_taps=800).bank)
    assert bits_equal(cv._aug.rirs.bank, ctn.RirBank.from_rooms(rooms(4, 0), DEV, early_ms=10.0, n_taps=800).bank)
    assert all(np.isfinite(solver.iter_losses)) and [f[0] for f in first] == [0, 1]
    assert all(len(set((row // 2).tolist())) == 1 and len(set(row.tolist())) == 2 for f in first for row in f[3])
    ck = tmp_path / "full" / "checkpoint_models" / "epoch1.pth.tar"
    resumed = main(flags + ["--epochs", "0", "--continue-from", str(ck), "--save-folder", str(tmp_path / "resumed")])
    assert resumed.start_epoch == 1 and len(first) == 3 and first[2][0] == 1
    assert all(torch.equal(a, b) for a, b in zip(first[2][1:], first[1][1:]))
