"""STOI / ESTOI on the GPU (csrc/ctn_stoi.hip, stoi.py) against the float64 numpy restatement in stoi_oracle.py: the frame
stage (energies, keep mask, kept-index table), the band envelopes after compaction, the scores end to end at 10, 8 and 16 kHz,
batch invariance, properties, validation, and evaluate_loader(calc_stoi=True).

The limit: everything between the fp32 10 kHz samples and d is fp64 on both sides and the resampling is bitwise, so GPU and
oracle differ by summation order only: 1e-10 absolute on d, 1e-11 of the row maximum on the envelopes (the oracle's own two
forms differ by <= 5e-15).  Every test prints the largest deviation it saw before it asserts."""
import json
import warnings

import numpy as np
import pytest
import torch

import bss_oracle as BO
import stoi_oracle as SO
from oracle import ctn_oracle as O

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd.stoi import stoi, stoi_batch, stoi_both, stoi_improvement  # noqa: E402

DEV = "cuda:0"
LIMIT_D = 1e-10
LIMIT_ENV = 1e-11
NB = 15


def _ptr(t):
    return t.data_ptr()


# ---- the ragged 10 kHz batch of the stage tests: computed once, never modified -----------------------------------------------
STAGE = {}


def _stage_batch():
    if STAGE:
        return STAGE
    C, E, T, lens = 2, 1, 7100, [4095, 4096, 4097, 7000]
    rng = np.random.RandomState(11)
    ref = rng.randn(len(lens), C, T).astype(np.float32)                 # garbage after each length
    est = rng.randn(len(lens), E, T).astype(np.float32)
    for b, n in enumerate(lens):
        x = BO.speech_like(11 + b, C, n, sr=10000)
        if b == 3:
            x[0, 2000:3500] *= np.float32(1e-4)                          # a pause in one row of the long utterance ...
        if b == 1:
            x[1, 1000:2200] *= np.float32(1e-4)                          # ... and in one row of the exact-fit one
        ref[b, :, :n] = x
        est[b, 0, :n] = (0.7 * x[0] + 0.4 * x[1] + 0.05 * rng.randn(n)).astype(np.float32)
    want = {}
    for b, n in enumerate(lens):
        for c in range(C):
            r = ref[b, c, :n].astype(np.float64)
            xs, ys, idx, en, thr = SO.remove_silent(r, est[b, 0, :n].astype(np.float64))
            want[b, c] = {"en": en, "thr": thr, "idx": idx, "env_ref": SO.envelopes(xs), "env_est": SO.envelopes(ys)}
    STAGE.update(C=C, E=E, T=T, lens=lens, ref=ref, est=est, want=want)
    return STAGE


def _frames_gpu(ref, lens):
    B, C, T = ref.shape
    NF = ctn.lib.ctn_stoi_max_frames(T)
    rt = torch.from_numpy(ref).to(DEV)
    lt = torch.tensor(lens, dtype=torch.int64, device=DEV)
    en = torch.full((B, C, NF), 7.0, dtype=torch.float64, device=DEV)
    idx = torch.full((B, C, NF), -7, dtype=torch.int32, device=DEV)
    K = torch.full((B, C), -7, dtype=torch.int32, device=DEV)
    ctn.lib.call("ctn_stoi_frames", _ptr(rt), _ptr(lt), B, C, T, _ptr(en), _ptr(idx), _ptr(K), torch.cuda.current_stream().cuda_stream)
    return en, idx, K


def test_frames_energies_mask_and_index_table():
    s = _stage_batch()
    C, T, lens, want = s["C"], s["T"], s["lens"], s["want"]
    NF = ctn.lib.ctn_stoi_max_frames(T)
    assert NF == SO.frame_count(T) == 54
    # the conditions, on the oracle's side: no frame near the threshold, a frame removed somewhere, a row that keeps all
    margin = min(float(np.abs(w["en"] - w["thr"]).min()) for w in want.values())
    print("smallest |energy - threshold| %.3g dB" % margin)
    assert margin >= 1e-6
    assert any(len(w["idx"]) < len(w["en"]) for w in want.values()) and any(len(w["idx"]) == len(w["en"]) for w in want.values())
    assert [len(want[b, 0]["en"]) for b in range(4)] == [30, 30, 31, 53]            # the strict rule at the exact-fit lengths
    en, idx, K = (x.cpu().numpy() for x in _frames_gpu(s["ref"], lens))
    worst = 0.0
    for (b, c), w in want.items():
        nf, k = len(w["en"]), len(w["idx"])
        dev = np.abs(en[b, c, :nf] - w["en"]).max() / np.abs(w["en"]).max()
        worst = max(worst, dev)
        assert dev <= 1e-12, (b, c, dev)
        assert np.array_equal(en[b, c, :nf] > en[b, c, :nf].max() - 40, w["en"] > w["thr"])
        assert K[b, c] == k, (b, c, K[b, c], k)
        assert np.array_equal(idx[b, c, :k], w["idx"]), (b, c)
        assert (idx[b, c, k:] == -1).all() and (en[b, c, nf:] == 0).all()
    print("largest energy deviation / max |energy| %.3g" % worst)
    ref2 = s["ref"].copy()
    for b, n in enumerate(lens):
        ref2[b, :, n:] = -3.0
    for x, y in zip(_frames_gpu(ref2, lens), (en, idx, K)):
        assert np.array_equal(x.cpu().numpy(), y)                                  # the padding is never read: bitwise


def _bands_gpu(ref, est, lens):
    B, C, T = ref.shape
    E = est.shape[1]
    NF = ctn.lib.ctn_stoi_max_frames(T)
    MF = max(NF - 1, 1)
    _, idx, K = _frames_gpu(ref, lens)
    rt, et = torch.from_numpy(ref).to(DEV), torch.from_numpy(est).to(DEV)
    lt = torch.tensor(lens, dtype=torch.int64, device=DEV)
    env = torch.full((B, C + E * C, NB, MF), -1.0, dtype=torch.float64, device=DEV)
    ctn.lib.call("ctn_stoi_bands", _ptr(rt), _ptr(et), _ptr(lt), _ptr(idx), _ptr(K), B, C, E, T, _ptr(env),
                 torch.cuda.current_stream().cuda_stream)
    return env.cpu().numpy(), K.cpu().numpy()


def test_band_envelopes_after_compaction():
    s = _stage_batch()
    C, lens, want = s["C"], s["lens"], s["want"]
    env, K = _bands_gpu(s["ref"], s["est"], lens)
    worst = 0.0
    for (b, c), w in want.items():
        M = w["env_ref"].shape[1]
        assert M == K[b, c] - 1
        for got, exp in ((env[b, c], w["env_ref"]), (env[b, C + c], w["env_est"])):       # E = 1: set C + 0 * C + c
            dev = (np.abs(got[:, :M] - exp).max(axis=1) / exp.max(axis=1)).max()
            worst = max(worst, dev)
            assert dev <= LIMIT_ENV, (b, c, dev)
            assert (got[:, M:] == -1.0).all()                                           # nothing beyond frame M is written
    print("largest envelope deviation / row maximum %.3g" % worst)
    # the estimate under the two references' masks: different tables (on the oracle's side), so different envelopes
    assert len(want[3, 0]["idx"]) != len(want[3, 1]["idx"])
    m = min(want[3, 0]["env_est"].shape[1], want[3, 1]["env_est"].shape[1])
    assert not np.array_equal(env[3, C + 0, :, :m], env[3, C + 1, :, :m])
    ref2, est2 = s["ref"].copy(), s["est"].copy()
    for b, n in enumerate(lens):
        ref2[b, :, n:] = 5.0
        est2[b, :, n:] = -2.0
    assert np.array_equal(_bands_gpu(ref2, est2, lens)[0], env)


# ---- end to end -------------------------------------------------------------------------------------------------------------
WANT = {}


def _case(fs, n, kind, seed):
    key = (fs, n, kind, seed)
    if key not in WANT:
        ref, est = SO.case_signals(n, kind, seed)
        WANT[key] = (ref, est, {(e, c): SO.details(ref[c], est[e], fs) for e in range(2) for c in range(2)})
    return WANT[key]


def _gpu_both(ref, est, n, fs):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        out = stoi_both(torch.from_numpy(ref[None]).to(DEV), torch.from_numpy(est[None]).to(DEV), torch.tensor([n], device=DEV), fs)
    return [x[0].cpu().numpy() for x in out]


@pytest.mark.parametrize("fs,n,kind,seed", SO.CASES)
def test_scores_match_the_oracle_end_to_end(fs, n, kind, seed):
    """STOI and ESTOI of all four pairs, M and K against the oracle fed the same fp32 inputs.  Conditions, on the oracle's side:
    in the dips cases 5 % .. 50 % of the cells are clipped (measured 7 .. 17 %); in the pause cases none where estimate and
    reference belong together -- against the other speaker's reference a stray 0.1 .. 0.4 % are, so those pairs are held to
    below 1 % rather than to 0."""
    ref, est, want = _case(fs, n, kind, seed)
    shares = [w["clipped"] for w in want.values()]
    print("clipped cells: %s, threshold margin %.3g dB" % (["%.3f" % v for v in shares], min(w["margin"] for w in want.values())))
    assert min(w["margin"] for w in want.values()) >= 1e-6
    if kind == "dips":                       # the min() of the clipping is exercised
        assert all(0.05 <= v <= 0.5 for v in shares), shares
    if kind == "pause":                      # none where estimate and reference belong together (a stray cell with the other speaker's)
        assert want[0, 0]["clipped"] == 0 and want[1, 1]["clipped"] == 0 and max(shares) < 0.01, shares
        assert all(w["K"] < w["frames"] for w in want.values())
    if n == 3300:
        assert all(w["M"] == 30 for w in want.values())                  # exactly one segment
    if n == 3100:
        assert all(w["frames"] == 29 and w["stoi"] == 1e-5 and w["estoi"] == 1e-5 for w in want.values())
    d_stoi, d_estoi, M, K = _gpu_both(ref, est, n, fs)
    worst = 0.0
    for (e, c), w in want.items():
        assert (M[e, c], K[e, c]) == (w["M"], w["K"]), (e, c, M[e, c], K[e, c], w["M"], w["K"])
        worst = max(worst, abs(d_stoi[e, c] - w["stoi"]), abs(d_estoi[e, c] - w["estoi"]))
    print("largest |d - oracle| %.3g" % worst)
    assert worst <= LIMIT_D
    if n == 3100:
        assert (d_stoi == 1e-5).all() and (d_estoi == 1e-5).all()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for ext, d in ((False, d_stoi), (True, d_estoi)):
            a = stoi(ref[0], est[1], fs, extended=ext)
            b = stoi(torch.from_numpy(ref[0]), torch.from_numpy(est[1]), fs, extended=ext)
            assert isinstance(a, float) and a == b == d[1, 0]


# ---- batches ------------------------------------------------------------------------------------------------------------------
def _ragged(C, E, lens, T, seed):
    rng = np.random.RandomState(seed)
    ref = rng.randn(len(lens), C, T).astype(np.float32)
    est = rng.randn(len(lens), E, T).astype(np.float32)
    for b, n in enumerate(lens):
        ref[b, :, :n] = BO.speech_like(seed + b, C, n)
        est[b, :, :n] = 0.5 * ref[b, :, :n].sum(0) + 0.3 * rng.randn(E, n)
    return ref, est


def test_batch_is_bitwise_per_utterance_and_reproducible():
    C, E, T = 2, 3, 8000
    lens = [8000, 3100, 5003, 6000]
    ref, est = _ragged(C, E, lens, T, 8)
    rt, et = torch.from_numpy(ref).to(DEV), torch.from_numpy(est).to(DEV)
    lt = torch.tensor(lens, device=DEV)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        a = stoi_both(rt, et, lt, 8000)
        b = stoi_both(rt, et, lt, 8000)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        assert (a[0][1] == 1e-5).all() and (a[1][1] == 1e-5).all() and (a[2][1] < 30).all()
        assert (a[2][[0, 2, 3]] >= 30).all() and torch.isfinite(a[0]).all() and (a[0][[0, 2, 3]] != 1e-5).all()
        for u, n in enumerate(lens):
            one = stoi_both(rt[u:u + 1, :, :n].contiguous(), et[u:u + 1, :, :n].contiguous(), torch.tensor([n], device=DEV), 8000)
            for x, y in zip(a, one):
                assert torch.equal(x[u], y[0]), u


def test_large_batch_equals_single_utterance_calls():
    B, C, n = 48, 2, 6000
    ref = np.stack([BO.mixtures(500 + b, C, n)[0] for b in range(B)])
    est = np.concatenate([np.stack([BO.mixtures(500 + b, C, n)[1] for b in range(B)]), ref.sum(1, keepdims=True)], 1)
    rt, et = torch.from_numpy(ref).to(DEV), torch.from_numpy(est).to(DEV)
    got = stoi_both(rt, et, torch.full((B,), n, device=DEV), 8000)
    assert (got[2] >= 30).all()
    for u in range(0, B, 5):
        one = stoi_both(rt[u:u + 1], et[u:u + 1], torch.tensor([n], device=DEV), 8000)
        for x, y in zip(got, one):
            assert torch.equal(x[u], y[0]), u
    w = SO.details(ref[5, 1], est[5, 2], 8000)                       # the mixture row against reference 1
    assert abs(float(got[0][5, 2, 1]) - w["stoi"]) <= LIMIT_D and abs(float(got[1][5, 2, 1]) - w["estoi"]) <= LIMIT_D


# ---- properties ---------------------------------------------------------------------------------------------------------------
def test_identity_and_scale_invariance_on_the_device():
    """stoi_batch(ref, ref) has a diagonal of 1 within the limit.  Scaling an estimate leaves d within 1e-9 (not bitwise: the
    eps terms do not scale) when the scaling is one of the signal: by 0.125 every fp32 sample scales exactly.  By 0.1 the
    fp32 product rounds every sample anew (2^-24 relative), which is a different signal: that moves the ORACLE's d by up to
    2e-8 on these inputs, so for 0.1 the device is held to the oracle of the scaled samples (1e-10) and to 1e-9 beyond the
    movement of the oracle itself."""
    n, fs = 8000, 8000
    ref, est = SO.case_signals(n, "plain", 3)
    rt, et = torch.from_numpy(ref[None]).to(DEV), torch.from_numpy(est[None]).to(DEV)
    lt = torch.tensor([n], device=DEV)
    for ext in (False, True):
        d = stoi_batch(rt, rt, lt, fs, extended=ext)[0]
        print("identity: |d - 1| %.3g %.3g" % (abs(float(d[0, 0]) - 1), abs(float(d[1, 1]) - 1)))
        assert abs(float(d[0, 0]) - 1) <= LIMIT_D and abs(float(d[1, 1]) - 1) <= LIMIT_D
        assert float(d[0, 1]) < 0.9
        base = stoi_batch(rt, et, lt, fs, extended=ext)[0].cpu().numpy()
        exact = stoi_batch(rt, et * 0.125, lt, fs, extended=ext)[0].cpu().numpy()
        print("scaled by 0.125: %.3g" % np.abs(exact - base).max())
        assert np.abs(exact - base).max() <= 1e-9
        tenth = (est * np.float32(0.1)).astype(np.float32)
        got = stoi_batch(rt, torch.from_numpy(tenth[None]).to(DEV), lt, fs, extended=ext)[0].cpu().numpy()
        key = "estoi" if ext else "stoi"
        for e in range(2):
            for c in range(2):
                moved = abs(SO.details(ref[c], tenth[e], fs)[key] - SO.details(ref[c], est[e], fs)[key])
                assert abs(got[e, c] - SO.details(ref[c], tenth[e], fs)[key]) <= LIMIT_D
                assert abs(got[e, c] - base[e, c]) <= 1e-9 + moved, (e, c, got[e, c] - base[e, c], moved)


# ---- validation ---------------------------------------------------------------------------------------------------------------
def test_validation_and_the_too_short_row():
    ref, est = SO.case_signals(5000, "plain", 2)
    rt, et = torch.from_numpy(ref[None]).to(DEV), torch.from_numpy(est[None]).to(DEV)
    lt = torch.tensor([5000], device=DEV)
    with pytest.raises(ValueError):
        stoi_batch(rt.cpu(), et.cpu(), lt.cpu(), 8000)
    with pytest.raises(ValueError):
        stoi_batch(rt, et.cpu(), lt, 8000)
    with pytest.raises(ValueError):
        stoi_batch(rt, et[:, :, :4999], lt, 8000)
    with pytest.raises(ValueError):
        stoi_batch(rt, et[0], lt, 8000)
    with pytest.raises(ValueError):
        stoi_batch(rt, et, torch.tensor([5000, 5000], device=DEV), 8000)
    for bad in (0, -8000):
        with pytest.raises(ValueError):
            stoi_batch(rt, et, lt, bad)
    z = rt.clone()
    z[0, 1, :4000] = 0
    with pytest.raises(ValueError):
        stoi_batch(z, et, torch.tensor([4000], device=DEV), 8000)          # all zeros over its length (not beyond it)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                     # (its silent frames may leave fewer than 30)
        assert torch.isfinite(stoi_batch(z, et, lt, 8000)).all()
    with pytest.raises(ValueError):
        stoi(ref[0], est[0][:4999], 8000)
    with pytest.warns(RuntimeWarning, match="Not enough"):
        d = stoi_batch(rt, et, torch.tensor([3100], device=DEV), 8000)
    assert (d == 1e-5).all()
    with pytest.warns(RuntimeWarning):
        assert stoi(ref[0][:3100], est[0][:3100], 8000, extended=True) == 1e-5
    e0 = torch.zeros_like(et)                                              # a silent estimate is scored, not rejected
    assert torch.isfinite(stoi_batch(rt, e0, lt, 8000)).all()


# ---- evaluate_loader ------------------------------------------------------------------------------------------------------------
def test_evaluate_loader_calc_stoi(tmp_path, capsys):
    from scipy.io import wavfile
    from conv_tasnet_amd.data import AudioDataLoader, AudioDataset
    from conv_tasnet_amd.evaluate import evaluate_loader
    from conv_tasnet_amd.pit_criterion import cal_loss
    torch.manual_seed(3)
    m = ctn.ConvTasNet(32, 20, 16, 32, 3, 2, 1, 2).to(DEV)
    mix, lens, src = O.synth_batch(11, 3, 6200)
    src = src / src.abs().max() * 0.4
    manifests = {"mix": [], "s1": [], "s2": []}
    for u in range(3):
        n = 6200 - 500 * u                                                  # >= 5000 samples: every utterance has segments
        sig = {"s1": src[u, 0, :n], "s2": src[u, 1, :n]}
        sig["mix"] = sig["s1"] + sig["s2"]
        for k, v in sig.items():
            p = str(tmp_path / ("%s_%d.wav" % (k, u)))
            wavfile.write(p, 8000, (v.numpy() * 32767).astype(np.int16))
            manifests[k].append([p, n])
    for k, v in manifests.items():
        (tmp_path / (k + ".json")).write_text(json.dumps(v))

    def loader():
        return AudioDataLoader(AudioDataset(str(tmp_path), 2, sample_rate=8000, segment=-1))
    plain = evaluate_loader(m, loader(), verbose=False)
    capsys.readouterr()
    got = evaluate_loader(m, loader(), calc_stoi=True, sample_rate=8000)
    out = capsys.readouterr().out
    assert isinstance(got, tuple) and len(got) == 4
    assert got[0] == plain
    assert out.count("\tSTOI=") == 3 and " ESTOI=" in out and "Average STOI: " in out and "Average ESTOI: " in out
    assert "Average SISNR improvement" in out
    want = []
    with torch.no_grad():
        for pm, ml, ps in loader():
            est = m(pm.to(DEV))
            _, _, _, reord = cal_loss(ps.to(DEV), est, ml.to(DEV))
            for b, n in enumerate(ml.tolist()):
                r, e, x = ps[b, :, :n].numpy(), reord[b, :, :n].cpu().numpy(), pm[b, :n].numpy()
                d = [SO.details(r[k], e[k], 8000) for k in range(2)]
                a = [SO.details(r[k], x, 8000) for k in range(2)]
                assert all(v["M"] >= 30 for v in d)
                want.append((np.mean([v["stoi"] for v in d]), np.mean([v["estoi"] for v in d]),
                             np.mean([v["stoi"] - w["stoi"] for v, w in zip(d, a)])))
    assert len(want) == 3
    dev = np.abs(np.asarray(got[1:]) - np.mean(np.asarray(want), axis=0)).max()
    print("largest |average - oracle| %.3g" % dev)
    assert dev <= LIMIT_D
    both = evaluate_loader(m, loader(), calc_sdr=True, calc_stoi=True, verbose=False)
    assert len(both) == 5 and both[0] == plain and both[2:] == got[1:]
    d = torch.tensor([[[0.9, 0.1], [0.2, 0.8], [0.5, 0.6]]], dtype=torch.float64, device=DEV)
    assert abs(float(stoi_improvement(d)[0]) - 0.3) <= 1e-15


def test_eval_is_graph_capturable_and_replays_bitwise():
    """ctn_stoi_eval reads nothing back and does not synchronise: captured in a graph, a replay over new samples in the same
    buffers gives the bits of the plain call."""
    C, E, T = 2, 3, 7100
    lens = [7000, 4097, 3000]
    ref, est = _ragged(C, E, lens, T, 21)
    ref2, est2 = _ragged(C, E, lens, T, 22)
    B = len(lens)
    rt, et = torch.from_numpy(ref).to(DEV), torch.from_numpy(est).to(DEV)
    lt = torch.tensor(lens, dtype=torch.int64, device=DEV)
    ws = torch.empty(ctn.lib.ctn_stoi_workspace(B, C, E, T), dtype=torch.uint8, device=DEV)
    out = [torch.zeros(B, E, C, dtype=torch.float64, device=DEV) for _ in range(2)]
    cnt = [torch.zeros(B, E, C, dtype=torch.int32, device=DEV) for _ in range(2)]

    def run():
        ctn.lib.call("ctn_stoi_eval", _ptr(rt), _ptr(et), _ptr(lt), B, C, E, T, _ptr(out[0]), _ptr(out[1]), _ptr(cnt[0]), _ptr(cnt[1]),
                     _ptr(ws), ws.numel(), torch.cuda.current_stream().cuda_stream)
    run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    rt.copy_(torch.from_numpy(ref2))
    et.copy_(torch.from_numpy(est2))
    g.replay()
    torch.cuda.synchronize()
    replayed = [x.clone() for x in out + cnt]
    run()
    torch.cuda.synchronize()
    for x, y in zip(replayed, out + cnt):
        assert torch.equal(x, y)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        want = stoi_both(rt, et, lt, 10000)
    for x, y in zip(replayed, want):
        assert torch.equal(x, y)
    assert (want[2][2] < 30).all() and (want[0][2] == 1e-5).all() and (want[2][:2] >= 30).all()
