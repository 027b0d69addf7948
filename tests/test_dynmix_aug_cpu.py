"""CPU-only checks of the noisy and reverberant dynamic mixing: the RIR bank's host tables and the SNR table against the
oracle (dynmix_aug_oracle.py), the synthetic bank, the oracle's own reverberation against float64 within the rounding bound,
the train.py flags, the exported symbols, and the argument checks of the three entry points (csrc/ctn_dynmix_aug.hip), which
sit in front of every launch."""
import subprocess

import numpy as np
import pytest

import dynmix_aug_oracle as AO

import conv_tasnet_amd as ctn
from conv_tasnet_amd import _lib, dynmix, rir

AUG_ENTRY_POINTS = ["ctn_dynmix_plan_aug", "ctn_dynmix_reverb", "ctn_dynmix_gather_aug"]


def _responses():
    rng = np.random.RandomState(3)
    tie = np.array([0.0, -0.5, 0.25, 0.5, 0.1])                     # |h| has its maximum twice: the first index counts
    late = np.concatenate([0.01 * rng.randn(300), [2.0], 0.05 * rng.randn(900)])
    short = np.array([0.3, -0.7])
    edge = np.concatenate([0.1 * rng.randn(399), [1.5]])           # the direct path on the last tap
    return [tie, late, short, edge, np.array([1.0]), rng.randn(rir.MAX_TAPS)]


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("early_ms", [None, 0, 50.0])
def test_bank_host_tables_equal_the_oracle(early_ms, normalize):
    arrays = _responses()
    got = rir.build_tables(arrays, 8000, early_ms, normalize)
    want = AO.rir_tables(arrays, 8000, early_ms, normalize)
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k].view(np.uint32) if got[k].dtype == np.float32 else got[k],
                              want[k].view(np.uint32) if want[k].dtype == np.float32 else want[k]), k
    n = [len(a) for a in arrays]
    assert list(got["lens"]) == n and list(got["offsets"]) == list(np.cumsum([0] + n[:-1]))
    assert got["offsets"].dtype == np.int64 and got["lens"].dtype == got["direct"].dtype == got["early"].dtype == np.int32
    assert list(got["direct"][:5]) == [1, 300, 1, 399, 0]           # the tie goes to the first maximum
    if early_ms is None:
        assert list(got["early"]) == n
    elif early_ms == 0:
        assert list(got["early"]) == [d + 1 for d in got["direct"]]  # the direct path alone
    else:
        assert list(got["early"][:5]) == [5, 701, 2, 400, 1]        # d + 1 + 400, clipped at n_r
    first = got["bank"][:5].astype(np.float64)
    if normalize:
        for r in range(len(arrays)):
            h = got["bank"][got["offsets"][r]:got["offsets"][r] + n[r]].astype(np.float64)
            assert abs(np.sum(h * h) - 1.0) < 1e-6
    else:
        assert np.array_equal(first, arrays[0].astype(np.float32).astype(np.float64))


def test_bank_refuses_what_it_cannot_hold():
    ok = np.array([1.0, 0.5])
    for bad in ([], [ok, np.zeros(0)], [np.ones(rir.MAX_TAPS + 1)], [np.array([1.0, np.nan])], [np.array([np.inf])]):
        with pytest.raises(ValueError):
            rir.build_tables(bad, 8000, 50.0, False)
    with pytest.raises(ValueError, match="zeros"):
        rir.build_tables([np.zeros(4)], 8000, 50.0, True)
    assert rir.build_tables([np.zeros(4)], 8000, 50.0, False)["direct"][0] == 0
    with pytest.raises(ValueError):
        rir.build_tables([ok], 8000, -1.0, True)
    with pytest.raises(ValueError, match="GPU"):
        rir.RirBank.from_arrays([ok], "cpu")
    assert ctn.RirBank is rir.RirBank and ctn.rir is rir


def test_bank_manifest_refuses_a_file_at_another_rate(tmp_path):
    import json
    from scipy.io import wavfile
    wavfile.write(str(tmp_path / "a.wav"), 16000, (np.arange(40) * 100).astype(np.int16))
    (tmp_path / "rirs.json").write_text(json.dumps([[str(tmp_path / "a.wav"), 40]]))
    with pytest.raises(ValueError, match="16000"):
        rir.RirBank.from_manifest(str(tmp_path / "rirs.json"), 8000, "cuda:0")


def test_synthetic_bank_is_deterministic_and_within_its_limits():
    a, b = rir.synthetic_bank(12, 8000, seed=4), rir.synthetic_bank(12, 8000, seed=4)
    assert len(a) == 12 and all(np.array_equal(x, y) for x, y in zip(a, b))
    assert not np.array_equal(a[0][:50], rir.synthetic_bank(1, 8000, seed=5)[0][:50])
    for h in a:
        d = int(np.argmax(np.abs(h)))
        assert h.dtype == np.float64 and np.all(np.isfinite(h))
        assert h[d] == 1.0 and d <= 16 and not h[:d].any()           # a unit spike at a delay of 2 ms at most, nothing before it
        tail = len(h) - d - 1
        assert 0.2 * 8000 <= tail <= 0.6 * 8000 + 1                  # truncated where the envelope reaches -60 dB
        assert np.abs(h[d + 1:]).max() < 1.0 and np.abs(h[-1]) <= 0.9e-3 * 1.001
    long = rir.synthetic_bank(3, 8000, rt60=(1.5, 1.5), seed=0)
    assert all(len(h) == rir.MAX_TAPS for h in long)                 # or at 8192 taps
    t = rir.build_tables(a, 8000, 50.0, True)
    assert np.array_equal(t["early"], np.minimum(t["lens"], t["direct"] + 401))
    with pytest.raises(ValueError):
        rir.synthetic_bank(0)


def test_snr_table_and_range():
    assert dynmix.snr_range((-6, 3)) == (-60, 30) and dynmix.snr_range((2.5, 2.5)) == (25, 25)
    w = dynmix.snr_table(-60, 30)
    assert w.dtype == np.float32 and w.shape == (91,) and np.array_equal(w.view(np.uint32), AO.snr_table(-60, 30).view(np.uint32))
    assert w[0] == np.float32(10.0 ** 0.3) and w[-1] == np.float32(10.0 ** -0.15) and w[60] == 1.0
    for bad in ((3, -6), (0, 102.4), "x", (1,)):
        with pytest.raises(ValueError):
            dynmix.snr_range(bad)
    assert dynmix.snr_range((0, 102.3)) == (0, 1023)
    ids = dynmix.noise_table([100, 50, 300, 120], [0.1, 0.1, 0.0, 0.2], 100)
    assert ids.dtype == np.int32 and list(ids) == [0, 3]
    with pytest.raises(ValueError, match="noise"):
        dynmix.noise_table([100, 50], [0.0, 0.1], 100)


def test_plan_aug_oracle_draws():
    noise = dict(noise_ids=np.array([0, 2, 3], np.int32), lens=np.array([500, 10, 100, 101]), inv_rms=np.array([2.0, 1.0, 4.0, 0.5], np.float32),
                 wn=AO.snr_table(-30, 60), lo10=-30)
    seen_r, seen_v, seen_s = set(), set(), set()
    for step in range(40):
        rirp, v, st, snr, g = AO.plan_aug(7, 1, 0, step, 8, 3, 100, R=5, noise=noise)
        assert rirp.shape == (8, 3) and rirp.min() >= 0 and rirp.max() < 5
        assert set(v) <= {0, 2, 3} and np.all(st >= 0) and np.all(st <= noise["lens"][v] - 100) and np.all(st[v == 2] == 0)
        assert np.all(snr >= -30) and np.all(snr <= 60)
        assert np.array_equal(g, noise["wn"][snr + 30] * noise["inv_rms"][v])
        seen_r.update(rirp.reshape(-1)); seen_v.update(v); seen_s.update(snr)
    assert seen_r == set(range(5)) and seen_v == {0, 2, 3} and len(seen_s) > 50
    again = AO.plan_aug(7, 1, 0, 3, 8, 3, 100, R=5, noise=noise)
    assert all(np.array_equal(a, b) for a, b in zip(again, AO.plan_aug(7, 1, 0, 3, 8, 3, 100, R=5, noise=noise)))
    assert AO.plan_aug(7, 1, 0, 3, 8, 3, 100, noise=noise)[0] is None and AO.plan_aug(7, 1, 0, 3, 8, 3, 100, R=5)[1] is None
    for change in (dict(seed=8), dict(rank=2), dict(epoch=1), dict(step=4)):
        a = dict(dict(seed=7, rank=1, epoch=0, step=3), **change)
        other = AO.plan_aug(a["seed"], a["rank"], a["epoch"], a["step"], 8, 3, 100, R=5, noise=noise)
        assert not np.array_equal(other[0], again[0]), change


@pytest.mark.parametrize("n,d,e,T", [(1, 0, 1, 50), (2, 1, 1, 7), (257, 100, 180, 300), (1000, 0, 1, 64), (1000, 999, 1000, 1300),
                                     (8192, 4000, 4401, 700)])
def test_reverb_f32_is_within_the_rounding_bound_of_float64(n, d, e, T):
    """n products and n adds, one rounding each: |f32 - f64| <= (n + 1) * 2^-24 * sum_j |h_j| |x_j| per output."""
    rng = np.random.RandomState(n + T)
    x = (0.1 * rng.randn(T)).astype(np.float32)
    h = (rng.randn(n) * np.exp(-np.arange(n) / (0.2 * n + 1.0))).astype(np.float32)
    wet, tgt = AO.reverb_f32(x, h, d, e)
    wet64, tgt64 = AO.reverb_f64(x, h, d, e)
    assert wet.dtype == tgt.dtype == np.float32 and wet64.dtype == np.float64
    bound = (n + 1) * 2.0 ** -24 * AO.tap_abs_sum(x, h, d)
    assert np.all(np.abs(wet.astype(np.float64) - wet64) <= bound)
    assert np.all(np.abs(tgt.astype(np.float64) - tgt64) <= bound)
    # against the textbook convolution: wet[t] = (h * x)[t + d]
    full = np.convolve(h.astype(np.float64), x.astype(np.float64))
    ref = np.concatenate([full, np.zeros(T)])[d:d + T]
    assert np.allclose(wet64, ref, rtol=0, atol=1e-12 * max(1.0, np.abs(ref).max()))
    assert np.allclose(tgt64, np.concatenate([np.convolve(h[:e].astype(np.float64), x.astype(np.float64)), np.zeros(T + d)])[d:d + T],
                       rtol=0, atol=1e-12 * max(1.0, np.abs(ref).max()))
    if e == n:
        assert np.array_equal(wet, tgt)


def test_mix_aug_oracle_on_a_toy_case():
    f = np.float32
    corpus = np.array([0.5, -0.25, 0.125, 1.0, 2.0, -4.0], dtype=np.float32)
    tgt = np.array([0.25, 0.0, 0.125, 1.0, 1.0, -1.0], dtype=np.float32)
    noise = np.array([9.0, 1.0, -1.0, 2.0], dtype=np.float32)
    utt, start = np.array([[0, 1]], np.int32), np.zeros((1, 2), np.int64)
    gain = np.array([[2.0, 0.5]], np.float32)
    mixture, sources, peak = AO.mix_aug(corpus, [0, 3], utt, start, gain, 3, tgt_corpus=tgt, noise=noise, noise_offsets=[0], noise_utt=[0],
                                        noise_start=[1], ngain=[0.5])
    # r_0 = [1, -.5, .25], r_1 = [.5, 1, -2], n = [.5, -.5, 1]: mix = [2, 0, -.75]; g_0 = [.5, 0, .25], g_1 = [.5, .5, -.5]; a = 2
    scale = f(0.9) / f(2.0)
    assert peak[0] == f(2.0)
    assert np.array_equal(mixture[0], np.array([scale * f(2.0), scale * f(0.0), scale * f(-0.75)], np.float32))
    assert np.array_equal(sources[0, 0], np.array([scale * f(0.5), f(0.0), scale * f(0.25)], np.float32))
    assert np.array_equal(sources[0, 1], np.array([scale * f(0.5), scale * f(0.5), scale * f(-0.5)], np.float32))
    # without targets and noise it is the plain mix
    a = AO.mix_aug(corpus, [0, 3], utt, start, gain, 3)
    b = AO.DO.mix(corpus, [0, 3], utt, start, gain, 3)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    flagged = AO.mix_aug(corpus, [0, 3], np.array([[0, -1]], np.int32), start, gain, 3)
    assert flagged[2][0] == -1 and not flagged[1][0, 1].any() and flagged[1][0, 0].any()


def test_train_parser_accepts_the_noise_and_rir_flags_and_keeps_the_defaults():
    from conv_tasnet_amd.train import build_parser, main, parse_snr
    a = build_parser().parse_args([])
    assert (a.epochs, a.batches, a.batch_size, a.data_dir, a.optimizer, a.lr) == (1, 10, 8, None, "adam", 1e-3)
    assert (a.dynamic_mix, a.dynamic_mix_cv, a.speed_perturb, a.corpus_rate, a.steps_per_epoch, a.segment_len) == (None, None, None, "8000",
                                                                                                                   1000, 32000)
    assert (a.noise, a.snr, a.rirs, a.rir_early_ms, a.checkpoint, a.continue_from) == (None, "-6:3", None, "50", False, "")
    a = build_parser().parse_args(["--dynamic-mix", "tr.json", "--noise", "n.json", "--snr=-3:6", "--rirs", "synthetic:8",
                                   "--rir-early-ms", "full"])
    assert (a.noise, a.snr, a.rirs, a.rir_early_ms) == ("n.json", "-3:6", "synthetic:8", "full")
    assert parse_snr(a.snr) == (-3.0, 6.0) and parse_snr("0.5:2") == (0.5, 2.0)
    with pytest.raises(ValueError):
        parse_snr("3")
    for flags in (["--noise", "n.json"], ["--rirs", "synthetic:4"], ["--rirs", "r.json", "--dynamic-mix-cv", "cv.json"]):
        with pytest.raises(SystemExit, match="dynamic-mix only"):
            main(flags)


def test_package_exports_and_library_symbols():
    protos = _lib.parse_header()
    assert not [n for n in AUG_ENTRY_POINTS if n not in protos]
    out = subprocess.run(["nm", "-D", "--defined-only", ctn.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert not [n for n in AUG_ENTRY_POINTS if n not in exported]
    assert protos["ctn_dynmix_reverb"][2] == ["corpus", "offsets", "lens", "U", "plan_utt", "plan_start", "N", "T", "bank", "bank_floats",
                                              "rir_offsets", "rir_lens", "rir_direct", "rir_early", "R", "plan_rir", "wet", "tgt", "out_utt",
                                              "stream"]
    assert protos["ctn_dynmix_gather_aug"][2][10:18] == ["tgt_corpus", "noise", "noise_offsets", "noise_lens", "Un", "noise_utt",
                                                         "noise_start", "ngain"]
    assert callable(dynmix.gather_aug) and hasattr(dynmix.DynamicMixLoader, "last_aug_plan")


def test_bad_arguments_return_error_codes_and_launch_nothing():
    # every check sits in front of the first launch, so this is safe without a GPU (fake non-null pointers are never read)
    lib, err = ctn.lib, ctn.lib.ctn_last_error
    p = 4096

    def plan(step=p, B=8, C=2, seg=100, seed=0, rank=0, epoch=0, R=4, rirp=p, ids=p, Nn=3, nlens=p, Un=5, inv=p, wn=p, nsnr=91, utt=p,
             start=p, snr=p, ng=p):
        return lib.ctn_dynmix_plan_aug(seed, epoch, rank, step, B, C, seg, R, rirp, ids, Nn, nlens, Un, inv, wn, nsnr, -60, utt, start, snr, ng, 0)

    assert plan(step=0) == -1 and b"null" in err()
    assert plan(rirp=0, ids=0, nlens=0, inv=0, wn=0, utt=0, start=0, snr=0, ng=0) == -1 and b"null" in err()
    for half in ("ids", "nlens", "inv", "wn", "utt", "start", "snr", "ng"):
        assert plan(**{half: 0}) == -1 and b"null" in err(), half
    assert plan(C=5) == -1 and b"sources per mixture" in err()
    assert plan(C=1) == -1 and b"sources per mixture" in err()
    assert plan(B=0) == -1 and b"mixtures" in err()
    assert plan(seg=0) == -1 and b"seg_len" in err()
    assert plan(seed=1 << 48) == -1 and b"seed" in err()
    assert plan(seed=-1) == -1 and b"seed" in err()
    assert plan(rank=1 << 16) == -1 and b"rank" in err()
    assert plan(epoch=-1) == -1 and b"epoch" in err()
    assert plan(R=0) == -1 and b"responses" in err()
    assert plan(Nn=0) == -1 and b"eligible" in err()
    assert plan(Un=0) == -1 and b"noise utterances" in err()
    assert plan(nsnr=0) == -1 and b"SNR" in err()
    assert plan(nsnr=1025) == -1 and b"SNR" in err()

    def reverb(corpus=p, N=4, T=100, U=9, bank=p, floats=1000, R=3, rirp=p, wet=p, tgt=p, out=p, early=p):
        return lib.ctn_dynmix_reverb(corpus, p, p, U, p, p, N, T, bank, floats, p, p, p, early, R, rirp, wet, tgt, out, 0)

    for name in ("corpus", "bank", "rirp", "wet", "out", "early"):
        assert reverb(**{name: 0}) == -1 and b"null" in err(), name
    assert reverb(N=0) == -1 and b"rows" in err()
    assert reverb(N=65536) == -1 and b"rows" in err()
    assert reverb(T=0) == -1 and b"seg_len" in err()
    assert reverb(T=(1 << 30) + 1) == -1 and b"seg_len" in err()
    assert reverb(U=0) == -1 and b"utterances" in err()
    assert reverb(R=0) == -1 and b"responses" in err()
    assert reverb(floats=0) == -1 and b"bank_floats" in err()
    assert reverb(wet=p + 4) == -1 and b"aligned" in err()
    assert reverb(tgt=p + 8) == -1 and b"aligned" in err()

    def gather(corpus=p, peak=p, ws=p, wsb=1 << 20, B=8, C=2, T=100, mix=p, U=4, noise=p, nutt=p, Un=3):
        return lib.ctn_dynmix_gather_aug(corpus, p, p, U, p, p, p, B, C, T, p, noise, p, p, Un, nutt, p, p, mix, p, peak, ws, wsb, 0)

    assert gather(corpus=0) == -1 and b"null" in err()
    assert gather(peak=0) == -1 and b"null" in err()
    assert gather(nutt=0) == -1 and b"noise tables" in err()
    assert gather(Un=0) == -1 and b"noise utterances" in err()
    assert gather(C=5) == -1 and b"sources per mixture" in err()
    assert gather(T=0) == -1 and b"seg_len" in err()
    assert gather(B=0) == -1 and b"mixtures" in err()
    assert gather(B=65536) == -1 and b"mixtures" in err()
    assert gather(U=0) == -1 and b"utterances" in err()
    assert gather(mix=p + 4) == -1 and b"aligned" in err()
    assert gather(ws=0) == -1 and b"workspace" in err()
    assert gather(wsb=4, T=32000) == -3 and b"workspace" in err()
    with pytest.raises(ctn.CtnError, match="sources per mixture"):
        ctn.lib.call("ctn_dynmix_gather_aug", p, p, p, 4, p, p, p, 8, 5, 100, 0, 0, 0, 0, 0, 0, 0, 0, p, p, p, p, 1 << 20, 0)
