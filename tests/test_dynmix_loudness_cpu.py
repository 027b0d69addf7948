"""CPU: the host side of the LibriMix recipe in the dynamic mixer (dynmix.py, train.py) and its restatement
(dynmix_loudness_oracle.py): the tables, the range parsing, what the loader refuses, the draws that must keep their bits."""
import types

import numpy as np
import pytest

import dynmix_aug_oracle as AO
import dynmix_loudness_oracle as XO
import dynmix_oracle as DO
import conv_tasnet_amd as ctn
from conv_tasnet_amd import _lib, dynmix

ENTRY_POINTS = ("ctn_dynmix_plan_loudness", "ctn_dynmix_gather_peak", "ctn_dynmix_gather_aug_peak")


def test_loudness_table_and_range():
    assert dynmix.loudness_range((-33, -25)) == (-330, -250) and dynmix.loudness_range((-30.5, -30.5)) == (-305, -305)
    w = dynmix.loudness_table(-330, -250)
    assert w.dtype == np.float32 and w.shape == (81,) and np.array_equal(w.view(np.uint32), XO.loudness_table(-330, -250).view(np.uint32))
    assert w[0] == np.float32(10.0 ** ((-33.0 + 0.691) / 20.0)) and w[-1] == np.float32(10.0 ** ((-25.0 + 0.691) / 20.0))
    # unit gated power reads -0.691 LUFS: times wl[i] it reads (lo10 + i) / 10
    assert abs(-0.691 + 20.0 * np.log10(float(dynmix.loudness_table(-230, -230)[0])) - (-23.0)) < 1e-6
    for bad in ((-25, -33), (-110, -7.6), "x", (1,), None):
        with pytest.raises(ValueError):
            dynmix.loudness_range(bad)
    assert dynmix.loudness_range((-102.3, 0)) == (-1023, 0)
    assert dynmix.peak_mode("always") == 0 and dynmix.peak_mode("clip") == 1
    for bad in ("never", None, 1):
        with pytest.raises(ValueError, match="peak"):
            dynmix.peak_mode(bad)


def test_loader_refuses_what_the_recipe_cannot_mean():
    """The checks come before anything touches the device: a stand-in corpus is enough."""
    rms, loud = types.SimpleNamespace(level="rms"), types.SimpleNamespace(level="loudness")
    with pytest.raises(ValueError, match="level='loudness'"):
        ctn.DynamicMixLoader(rms, 2, 100, rank=0, loudness_db=(-33, -25))
    with pytest.raises(ValueError, match="level='loudness'"):
        ctn.DynamicMixLoader(types.SimpleNamespace(level="active"), 2, 100, rank=0, loudness_db=(-33, -25))
    with pytest.raises(ValueError, match="noise_loudness_db"):
        ctn.DynamicMixLoader(loud, 2, 100, rank=0, loudness_db=(-33, -25), noise_loudness_db=(-38, -30))          # no noise corpus
    with pytest.raises(ValueError, match="noise_loudness_db"):
        ctn.DynamicMixLoader(loud, 2, 100, rank=0, noise=rms, noise_loudness_db=(-38, -30))                          # an rms one
    with pytest.raises(ValueError, match="peak"):
        ctn.DynamicMixLoader(rms, 2, 100, rank=0, peak="never")
    with pytest.raises(ValueError):
        ctn.DynamicMixLoader(loud, 2, 100, rank=0, loudness_db=(-25, -33))
    with pytest.raises(ValueError, match="GPU"):
        ctn.DeviceCorpus.from_arrays([np.ones(10, np.float32)], ["a"], "cpu", level="loudness", sample_rate=8000)
    with pytest.raises(ValueError, match="sample rate"):
        ctn.DeviceCorpus.from_arrays([np.ones(10, np.float32)], ["a"], "cuda:0", level="loudness")


def _tables(rng, U=9, S=4, seg=100):
    lens = rng.integers(seg, 4 * seg, size=U)
    spk = [u % S for u in range(U)]
    order = sorted(range(U), key=lambda u: (spk[u], u))
    spk_ptr = np.concatenate(([0], np.cumsum(np.bincount(spk, minlength=S)))).astype(np.int32)
    return dict(spk_ptr=spk_ptr, utt_ids=np.array(order, np.int32), lens=lens, inv_rms=rng.uniform(0.5, 20.0, size=U).astype(np.float32),
                w=DO.level_table())


def test_the_loudness_draw_uses_words_of_its_own_and_leaves_the_plan_alone():
    rng = np.random.default_rng(2)
    t = _tables(rng)
    B, C, seg = 6, 3, 100
    assert not set(XO.LOUDNESS_WORD + c for c in range(4)) & set(XO.other_words(4))
    wl = XO.loudness_table(-330, -250)
    seen = set()
    for step in range(30):
        utt, start, q, gain = DO.plan(5, 1, 2, step, B, C, seg, t)
        l10, lgain = XO.plan_loudness(5, 1, 2, step, utt, t["inv_rms"], wl, -330)
        again = DO.plan(5, 1, 2, step, B, C, seg, t)
        assert all(np.array_equal(a, b) for a, b in zip((utt, start, q, gain), again))                 # the plan is a pure function
        assert l10.min() >= -330 and l10.max() <= -250
        assert np.array_equal(lgain.view(np.uint32), (wl[l10 + 330] * t["inv_rms"][utt]).astype(np.float32).view(np.uint32))
        assert not np.array_equal(lgain, gain)
        seen.update(l10.reshape(-1).tolist())
    assert len(seen) > 70                                                                              # of 81 tenths
    a = XO.plan_loudness(5, 1, 2, 3, utt, t["inv_rms"], wl, -330)[0]
    for change in (dict(seed=6), dict(rank=2), dict(epoch=1), dict(step=4)):
        k = dict(dict(seed=5, rank=1, epoch=2, step=3), **change)
        assert not np.array_equal(XO.plan_loudness(k["seed"], k["rank"], k["epoch"], k["step"], utt, t["inv_rms"], wl, -330)[0], a), change
    # a flagged entry keeps gain 0
    bad = utt.copy()
    bad[0, 0] = -1
    assert XO.plan_loudness(5, 1, 2, 3, bad, t["inv_rms"], wl, -330)[1][0, 0] == 0.0


def test_the_noise_loudness_keeps_the_noise_entry_and_start():
    ids, lens = np.array([0, 2, 3], np.int32), np.array([500, 10, 100, 101])
    inv = np.array([2.0, 1.0, 4.0, 0.5], np.float32)
    snr = dict(noise_ids=ids, lens=lens, inv_rms=inv, wn=AO.snr_table(-60, 30), lo10=-60)
    for step in range(10):
        _, v0, s0, _, _ = AO.plan_aug(7, 1, 0, step, 8, 2, 100, noise=snr)
        v, s, l10, g = XO.noise_plan(7, 1, 0, step, 8, 2, 100, ids, lens, inv, -380, -300)
        assert np.array_equal(v, v0) and np.array_equal(s, s0)
        assert l10.min() >= -380 and l10.max() <= -300
        assert np.array_equal(g.view(np.uint32), (XO.loudness_table(-380, -300)[l10 + 380] * inv[v]).astype(np.float32).view(np.uint32))


def test_peak_rule_on_a_toy_case():
    f = np.float32
    corpus = np.array([0.5, -0.25, 0.125, 1.0, 2.0, -4.0], dtype=np.float32)
    utt, start = np.array([[0, 1]], np.int32), np.zeros((1, 2), np.int64)
    quiet, loud = np.array([[0.5, 0.125]], np.float32), np.array([[2.0, 0.5]], np.float32)
    # quiet: s_0 = [.25, -.125, .0625], s_1 = [.125, .25, -.5]: mix = [.375, .125, -.4375], peak .5: left alone under "clip"
    m, s, p = XO.mix(corpus, [0, 3], utt, start, quiet, 3, "clip")
    assert p[0] == f(0.5) and np.array_equal(m[0], np.array([0.375, 0.125, -0.4375], np.float32))
    assert np.array_equal(s[0, 1], np.array([0.125, 0.25, -0.5], np.float32))
    always = XO.mix(corpus, [0, 3], utt, start, quiet, 3, "always")
    assert all(np.array_equal(a, b) for a, b in zip(always, DO.mix(corpus, [0, 3], utt, start, quiet, 3)))
    assert abs(float(np.abs(always[0]).max()) - 0.9 * 0.4375 / 0.5) < 1e-6
    # loud: peak 2 > 0.9: both rules rescale, to the same bits
    a, b = XO.mix(corpus, [0, 3], utt, start, loud, 3, "clip"), XO.mix(corpus, [0, 3], utt, start, loud, 3, "always")
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and a[2][0] == f(2.0)
    assert max(float(np.abs(a[0]).max()), float(np.abs(a[1]).max())) <= 0.9 * (1 + 2.0 ** -23)
    assert XO.peak_scale(f(0.9), "clip") == f(1.0) and XO.peak_scale(np.nextafter(f(0.9), f(1.0)), "clip") < f(1.0)      # strict
    assert XO.peak_scale(f(0.0), "always") == f(1.0) and XO.peak_scale(f(0.0), "clip") == f(1.0)
    with pytest.raises(AssertionError):
        XO.peak_scale(f(1.0), "never")


def test_train_parser_takes_the_recipe_flags_and_keeps_the_defaults():
    from conv_tasnet_amd.train import build_parser, main, recipe_args
    a = build_parser().parse_args([])
    assert (a.level, a.loudness, a.noise_loudness, a.peak, a.librimix) == ("rms", None, None, None, False)
    assert recipe_args(a) == ("rms", None, None, "always")
    a = build_parser().parse_args(["--dynamic-mix", "tr.json", "--level", "loudness", "--loudness=-33:-25", "--noise", "n.json",
                                   "--noise-loudness=-38:-30", "--peak", "clip"])
    assert recipe_args(a) == ("loudness", (-33.0, -25.0), (-38.0, -30.0), "clip")
    a = build_parser().parse_args(["--dynamic-mix", "tr.json", "--librimix"])
    assert recipe_args(a) == ("loudness", (-33.0, -25.0), None, "clip")
    a = build_parser().parse_args(["--dynamic-mix", "tr.json", "--librimix", "--noise", "n.json"])
    assert recipe_args(a) == ("loudness", (-33.0, -25.0), (-38.0, -30.0), "clip")
    a = build_parser().parse_args(["--dynamic-mix", "tr.json", "--librimix", "--loudness=-30:-28", "--peak", "always"])
    assert recipe_args(a) == ("loudness", (-30.0, -28.0), None, "always")
    for flags, text in ((["--dynamic-mix", "tr.json", "--loudness=-33:-25"], "--level loudness"),
                        (["--dynamic-mix", "tr.json", "--noise-loudness=-38:-30"], "--noise"),
                        (["--dynamic-mix", "tr.json", "--level", "loudness", "--loudness=x"], "LO:HI")):
        with pytest.raises(SystemExit, match=text):
            recipe_args(build_parser().parse_args(flags))
    for flags in (["--librimix"], ["--peak", "clip"], ["--loudness=-33:-25"]):
        with pytest.raises(SystemExit, match="dynamic-mix"):
            main(flags)


def test_train_refuses_the_recipe_for_loaders_that_are_built():
    from conv_tasnet_amd.train import SyntheticLoader, train
    data = dict(tr_loader=SyntheticLoader(1, 1, samples=800), cv_loader=SyntheticLoader(1, 1, samples=800))
    with pytest.raises(ValueError, match="dict"):
        train(data, 1, "x.pth", level="loudness", loudness_db=(-33, -25), peak="clip")


def test_entry_points_are_declared_and_exported():
    import subprocess
    protos = _lib.parse_header()
    assert not [n for n in ENTRY_POINTS if n not in protos]
    out = subprocess.run(["nm", "-D", "--defined-only", ctn.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert not [n for n in ENTRY_POINTS + ("ctn_loudness",) if n not in exported]
    assert protos["ctn_dynmix_gather_peak"][2] == protos["ctn_dynmix_gather"][2][:-1] + ["peak_mode", "stream"]
    assert protos["ctn_dynmix_gather_aug_peak"][2] == protos["ctn_dynmix_gather_aug"][2][:-1] + ["peak_mode", "stream"]
    assert protos["ctn_dynmix_plan_loudness"][2] == ["plan_utt", "inv_rms", "U", "wl", "nl", "lo10", "seed", "epoch", "rank", "step", "B",
                                                     "C", "plan_l10", "gain", "stream"]
