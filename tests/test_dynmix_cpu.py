"""CPU-only checks of the dynamic mixing: the oracle itself (Philox known answers, plan invariants, the mix arithmetic on a
toy case), the host-side table building, the manifest writer, the train.py flags, and the argument checks of the three entry
points (csrc/ctn_dynmix.hip), which sit in front of every launch."""
import json
import subprocess

import numpy as np
import pytest

import dynmix_oracle as DO

import conv_tasnet_amd as ctn
from conv_tasnet_amd import _lib, dynmix

DYNMIX_ENTRY_POINTS = ["ctn_dynmix_levels", "ctn_dynmix_plan", "ctn_dynmix_gather_workspace", "ctn_dynmix_gather"]
SEG = 100


def test_philox_known_answers():
    """The Random123 known-answer vectors of philox4x32_10."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for counter, key, want in kat:
        assert DO.philox4x32(counter, key) == want


def _corpus_tables(C):
    """16 speakers with 1 .. 9 utterances each; some utterances shorter than SEG, one of zero energy; speaker 'only' has one
    eligible utterance of SEG + 1 samples (and a short one), speaker 'none' has no eligible utterance at all."""
    rng = np.random.RandomState(5)
    lens, msq, spk = [], [], []
    for s in range(14):
        for k in range(1 + (s * 4) % 9):
            n = SEG + 1 + int(rng.randint(0, 400)) if (k + s) % 4 != 3 or k == 0 else int(rng.randint(1, SEG))
            lens.append(n)
            msq.append(0.0 if (s, k) == (6, 0) else float(rng.uniform(1e-4, 1e-1)))
            spk.append("spk%02d" % s)
    lens += [SEG + 1, SEG - 1]
    msq += [0.01, 0.01]
    spk += ["only", "only"]
    lens += [SEG - 1, SEG + 50]
    msq += [0.01, 0.0]
    spk += ["none", "none"]
    return np.array(lens), np.array(msq), spk, dynmix.build_tables(lens, msq, spk, SEG, C)


@pytest.mark.parametrize("C", [2, 3])
def test_plan_invariants_over_4096_mixtures(C):
    lens, msq, spk, tb = _corpus_tables(C)
    assert len(set(spk)) == 16 and "none" not in tb["speakers"] and len(tb["speakers"]) == 15
    S = len(tb["speakers"])
    owner = {}
    for s in range(S):
        for u in tb["utt_ids"][tb["spk_ptr"][s]:tb["spk_ptr"][s + 1]]:
            owner[int(u)] = s
    assert all(lens[u] >= SEG and msq[u] > 0 for u in owner)                       # the table holds eligible utterances only
    seen, only_starts = set(), set()
    only_u = [u for u in owner if spk[u] == "only"]
    assert len(only_u) == 1 and lens[only_u[0]] == SEG + 1
    B = 64
    for step in range(4096 // B):
        utt, start, q, gain = DO.plan(1234, 0, 0, step, B, C, SEG, tb)
        for b in range(B):
            speakers = [owner[int(u)] for u in utt[b]]                              # KeyError = not eligible / not in the table
            assert len(set(speakers)) == C
            seen.update(speakers)
            for c in range(C):
                u = int(utt[b, c])
                assert 0 <= start[b, c] <= lens[u] - SEG
                if u == only_u[0]:
                    only_starts.add(int(start[b, c]))
                assert 1 <= abs(int(q[b, c])) < 250
                assert gain[b, c] == np.float32(tb["w"][q[b, c] + 249]) * np.float32(tb["inv_rms"][u])
            assert 1 <= q[b, 0] < 250 and q[b, 1] == -q[b, 0]
    assert seen == set(range(S))          # a speaker is missed by 4096 C = 2 mixtures with probability (13/15)^4096
    assert only_starts == {0, 1}


def test_plan_is_a_function_of_seed_rank_epoch_step():
    _, _, _, tb = _corpus_tables(2)
    base = dict(seed=7, rank=0, epoch=0, step=0)

    def draw(**kw):
        a = dict(base, **kw)
        return DO.plan(a["seed"], a["rank"], a["epoch"], a["step"], 16, 2, SEG, tb)

    ref = draw()
    for a, b in zip(ref, draw()):
        assert np.array_equal(a, b)
    for change in (dict(seed=8), dict(seed=7 + (1 << 32)), dict(rank=1), dict(epoch=1), dict(step=1)):
        other = draw(**change)
        assert not (np.array_equal(ref[0], other[0]) and np.array_equal(ref[1], other[1])), change


def test_mix_oracle_on_a_toy_case():
    f = np.float32
    corpus = np.array([0.5, -0.25, 0.125, 1.0, 2.0, -4.0, 0.0, 0.0, 0.0, 0.0], dtype=np.float32)
    offsets = np.array([0, 3, 6])                    # utterances: [0.5 -0.25 0.125], [1 2 -4], [0 0 0 0]
    utt = np.array([[0, 1], [2, 2]], dtype=np.int32)
    start = np.array([[0, 0], [0, 1]], dtype=np.int64)
    gain = np.array([[2.0, 0.5], [3.0, 5.0]], dtype=np.float32)
    mixture, sources, peak = DO.mix(corpus, offsets, utt, start, gain, 3)
    # s_0 = [1, -0.5, 0.25], s_1 = [0.5, 1, -2], mix = [1.5, 0.5, -1.75]; a = 2 (|s_1[2]|), scale = fl(0.9f / 2)
    scale = f(0.9) / f(2.0)
    assert peak[0] == f(2.0)
    assert np.array_equal(mixture[0], np.array([scale * f(1.5), scale * f(0.5), scale * f(-1.75)], dtype=np.float32))
    assert np.array_equal(sources[0, 0], np.array([scale * f(1.0), scale * f(-0.5), scale * f(0.25)], dtype=np.float32))
    assert np.array_equal(sources[0, 1], np.array([scale * f(0.5), scale * f(1.0), scale * f(-2.0)], dtype=np.float32))
    assert sources[0, 1, 2] == f(-0.9)               # 0.45f * 2 is exact
    # the all-zero segment: scale = 1, everything stays zero
    assert peak[1] == 0 and not mixture[1].any() and not sources[1].any()
    assert mixture.dtype == sources.dtype == peak.dtype == np.float32


def test_meansq_oracle():
    x = np.array([1, 2, 3, 0.5, 0.5], dtype=np.float32)
    assert np.array_equal(DO.meansq(x, [0, 3], [3, 2]), np.array([14.0 / 3.0, 0.25]))


def test_level_table_and_inverse_rms():
    w = dynmix.level_table()
    assert w.dtype == np.float32 and w.shape == (499,) and w[249] == 1.0 and np.array_equal(w, DO.level_table())
    assert w[249 + 200] == np.float32(10.0 ** 0.1) and w[0] == np.float32(10.0 ** (-249 / 2000.0))
    r = dynmix.inverse_rms([4.0, 0.0, 0.25])
    assert r.dtype == np.float32 and list(r) == [0.5, 0.0, 2.0]


def test_table_building():
    lens = [200, 50, 300, 120, 80, 100]
    msq = [0.1, 0.1, 0.0, 0.2, 0.3, 0.4]
    spk = ["b", "b", "a", "a", "c", "b"]
    tb = dynmix.build_tables(lens, msq, spk, 100, 2)
    # 'a': utterance 2 is silent, 3 stays; 'b': 1 is short, 0 and 5 stay (len == seg_len is eligible); 'c' has none and is dropped
    assert tb["speakers"] == ["a", "b"]
    assert list(tb["spk_ptr"]) == [0, 1, 3] and list(tb["utt_ids"]) == [3, 0, 5]
    assert tb["spk_ptr"].dtype == np.int32 and tb["utt_ids"].dtype == np.int32 and tb["lens"].dtype == np.int64
    with pytest.raises(ValueError, match="speaker"):
        dynmix.build_tables(lens, msq, spk, 100, 3)
    with pytest.raises(ValueError, match="speaker"):
        dynmix.build_tables(lens, msq, spk, 150, 2)          # only 'b' keeps an utterance
    with pytest.raises(ValueError):
        dynmix.build_tables(lens, msq, spk, 0, 2)


def test_preprocess_sources_writes_the_speaker_manifest(tmp_path):
    from scipy.io import wavfile
    from conv_tasnet_amd.preprocess import preprocess_sources
    for spk, name, n in (("01t", "01to030v", 30), ("01t", "01to0310", 45), ("02a", "02ac0201", 12)):
        d = tmp_path / "si_tr_s" / spk
        d.mkdir(parents=True, exist_ok=True)
        wavfile.write(str(d / (name + ".wav")), 8000, (np.arange(n) * 100).astype(np.int16))
    (tmp_path / "si_tr_s" / "02a" / "notes.txt").write_text("x")
    out = tmp_path / "json" / "tr_sources.json"
    infos = preprocess_sources(str(tmp_path / "si_tr_s"), str(out), 8000)
    got = json.loads(out.read_text())
    assert [tuple(i) for i in got] == [tuple(i) for i in infos]
    assert [(i[0].split("/")[-1], i[1], i[2]) for i in got] == [("01to030v.wav", 30, "01t"), ("01to0310.wav", 45, "01t"),
                                                                 ("02ac0201.wav", 12, "02a")]
    with pytest.raises(ValueError):
        preprocess_sources(str(tmp_path / "si_tr_s"), str(out), 16000)


def test_train_parser_accepts_the_dynamic_mix_flags_and_keeps_the_defaults():
    from conv_tasnet_amd.train import build_parser
    a = build_parser().parse_args([])
    assert (a.epochs, a.batches, a.batch_size, a.data_dir, a.optimizer, a.lr) == (1, 10, 8, None, "adam", 1e-3)
    assert a.dynamic_mix is None and a.dynamic_mix_cv is None
    a = build_parser().parse_args(["--dynamic-mix", "tr.json", "--steps-per-epoch", "250", "--dynamic-mix-cv", "cv.json"])
    assert (a.dynamic_mix, a.steps_per_epoch, a.dynamic_mix_cv, a.data_dir) == ("tr.json", 250, "cv.json", None)


def test_package_exports_and_library_symbols():
    protos = _lib.parse_header()
    assert not [n for n in DYNMIX_ENTRY_POINTS if n not in protos]
    out = subprocess.run(["nm", "-D", "--defined-only", ctn.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert not [n for n in DYNMIX_ENTRY_POINTS if n not in exported]
    assert ctn.DeviceCorpus is dynmix.DeviceCorpus and ctn.DynamicMixLoader is dynmix.DynamicMixLoader
    assert protos["ctn_dynmix_plan"][2] == ["spk_ptr", "utt_ids", "S", "lens", "inv_rms", "w", "seed", "epoch", "rank", "step", "B",
                                            "C", "seg_len", "plan_utt", "plan_start", "plan_q", "gain", "stream"]


def test_bad_arguments_return_error_codes_and_launch_nothing():
    # every check sits in front of the first launch, so this is safe without a GPU (fake non-null pointers are never read)
    lib, err = ctn.lib, ctn.lib.ctn_last_error
    p = 4096
    assert lib.ctn_dynmix_levels(0, 10, p, p, 1, p, 0) == -1 and b"null" in err()
    assert lib.ctn_dynmix_levels(p, 10, p, p, 1, 0, 0) == -1 and b"null" in err()
    assert lib.ctn_dynmix_levels(p, 10, p, p, 0, p, 0) == -1 and b"utterances" in err()
    assert lib.ctn_dynmix_levels(p, 0, p, p, 1, p, 0) == -1 and b"num_samples" in err()

    def plan(spk_ptr=p, step=p, S=8, B=8, C=2, seg=100, seed=0, rank=0, epoch=0, gain=p):
        return lib.ctn_dynmix_plan(spk_ptr, p, S, p, p, p, seed, epoch, rank, step, B, C, seg, p, p, p, gain, 0)

    assert plan(spk_ptr=0) == -1 and b"null" in err()
    assert plan(step=0) == -1 and b"null" in err()
    assert plan(gain=0) == -1 and b"null" in err()
    assert plan(C=5) == -1 and b"sources per mixture" in err()
    assert plan(C=1) == -1 and b"sources per mixture" in err()
    assert plan(seg=0) == -1 and b"seg_len" in err()
    assert plan(seg=-4) == -1 and b"seg_len" in err()
    assert plan(S=2, C=3) == -1 and b"speakers" in err()
    assert plan(B=0) == -1 and b"mixtures" in err()
    assert plan(seed=1 << 48) == -1 and b"seed" in err()
    assert plan(seed=-1) == -1 and b"seed" in err()
    assert plan(rank=1 << 16) == -1 and b"rank" in err()
    assert plan(epoch=-1) == -1 and b"epoch" in err()

    def gather(corpus=p, peak=p, ws=p, wsb=1 << 20, B=8, C=2, T=100, mode=0, mix=p):
        return lib.ctn_dynmix_gather(corpus, p, p, 4, p, p, p, B, C, T, mix, p, peak, ws, wsb, mode, 0)

    assert gather(corpus=0) == -1 and b"null" in err()
    assert gather(peak=0) == -1 and b"null" in err()
    assert gather(C=5) == -1 and b"sources per mixture" in err()
    assert gather(T=0) == -1 and b"seg_len" in err()
    assert gather(T=-1) == -1 and b"seg_len" in err()
    assert gather(B=0) == -1 and b"mixtures" in err()
    assert gather(mode=2) == -1 and b"mode" in err()
    assert gather(mix=p + 4) == -1 and b"aligned" in err()
    assert gather(ws=0) == -1 and b"workspace" in err()
    assert gather(wsb=4, T=32000) == -3 and b"workspace" in err()
    assert lib.ctn_dynmix_gather_workspace(8, 32000) == 4 * 8 * 32 and lib.ctn_dynmix_gather_workspace(0, 5) == 0
    with pytest.raises(ctn.CtnError, match="sources per mixture"):
        ctn.lib.call("ctn_dynmix_gather", p, p, p, 4, p, p, p, 8, 5, 100, p, p, p, p, 1 << 20, 0, 0)


def test_loader_and_corpus_refuse_the_cpu():
    with pytest.raises(ValueError, match="GPU"):
        dynmix.DeviceCorpus.from_arrays([np.ones(10, np.float32)], ["a"], "cpu")
