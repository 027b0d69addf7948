"""BSS Eval v3 on the GPU (csrc/ctn_bss.hip, bss_eval.py) against the float64 numpy/scipy restatement in bss_oracle.py:
correlations, Cholesky + solves, SDR/SIR/SAR and the permutation, cal_SDRi, batch invariance, validation, and
evaluate_loader(calc_sdr=True)."""
import json

import numpy as np
import pytest
import torch

import bss_oracle as BO
from oracle import ctn_oracle as O

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd.bss_eval import bss_eval_batch, bss_eval_sources  # noqa: E402
from conv_tasnet_amd.evaluate import cal_SDRi  # noqa: E402

DEV = "cuda:0"
F = 512


def _ptr(t):
    return t.data_ptr()


def _ragged(C, E, lens, T, seed):
    """[B,C,T] refs and [B,E,T] estimates with garbage after each length."""
    rng = np.random.RandomState(seed)
    ref = rng.randn(len(lens), C, T).astype(np.float32)
    est = rng.randn(len(lens), E, T).astype(np.float32)
    for b, n in enumerate(lens):
        ref[b, :, :n] = BO.speech_like(seed + b, C, n)
        est[b, :, :n] = 0.5 * ref[b, :, :n].sum(0) + 0.3 * rng.randn(E, n)
    return ref, est


def _corr_gpu(ref, est, lens):
    B, C, T = ref.shape
    E = est.shape[1]
    rt, et = torch.from_numpy(ref).to(DEV), torch.from_numpy(est).to(DEV)
    lt = torch.tensor(lens, dtype=torch.int64, device=DEV)
    r = torch.empty(B, C, C, F, dtype=torch.float64, device=DEV)
    d = torch.empty(B, E, C, F, dtype=torch.float64, device=DEV)
    en = torch.empty(B, E, dtype=torch.float64, device=DEV)
    ws = torch.empty(ctn.lib.ctn_bss_corr_workspace(B, C, E, T), dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    ctn.lib.call("ctn_bss_corr", _ptr(rt), _ptr(et), _ptr(lt), B, C, E, T, _ptr(r), _ptr(d), _ptr(en), _ptr(ws), ws.numel(), st)
    return r, d, en


def test_correlations_match_numpy_fp64_and_ignore_the_padding():
    C, E, T = 2, 3, 5200
    lens = [300, 5000, 2049, 2048]
    ref, est = _ragged(C, E, lens, T, 3)
    r, d, en = (x.cpu().numpy() for x in _corr_gpu(ref, est, lens))
    for b, n in enumerate(lens):
        s = ref[b, :, :n].astype(np.float64)
        e = est[b, :, :n].astype(np.float64)
        for i in range(C):
            for k in range(C):
                scale = np.linalg.norm(s[i]) * np.linalg.norm(s[k])
                assert np.abs(r[b, i, k] - BO.corr(s[i], s[k])).max() <= 1e-12 * scale
            for q in range(E):
                scale = np.linalg.norm(s[i]) * np.linalg.norm(e[q])
                assert np.abs(d[b, q, i] - BO.corr(s[i], e[q])).max() <= 1e-12 * scale
        assert np.abs(en[b] - (e ** 2).sum(1)).max() <= 1e-12 * (e ** 2).sum(1).max()
    ref2, est2 = ref.copy(), est.copy()
    for b, n in enumerate(lens):
        ref2[b, :, n:] = 7.0
        est2[b, :, n:] = -3.0
    for x, y in zip(_corr_gpu(ref2, est2, lens), (r, d, en)):
        assert np.array_equal(x.cpu().numpy(), y)


def test_cholesky_and_solves_match_numpy_solve():
    C, E, T = 3, 2, 6000
    lens = [6000, 4100]
    rng = np.random.RandomState(4)
    ref = rng.randn(2, C, T).astype(np.float32)                   # white references: well-conditioned G
    est = rng.randn(2, E, T).astype(np.float32)
    r, d, _ = _corr_gpu(ref, est, lens)
    B = 2
    fac = torch.empty(ctn.lib.ctn_bss_factor_doubles(B, C), dtype=torch.float64, device=DEV)
    status = torch.full((B, C), -7, dtype=torch.int32, device=DEV)
    ca = torch.empty(B, E, C * F, dtype=torch.float64, device=DEV)
    co = torch.empty(B, E, C, F, dtype=torch.float64, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    ctn.lib.call("ctn_bss_factor", _ptr(r), B, C, _ptr(fac), _ptr(status), st)
    ctn.lib.call("ctn_bss_solve", _ptr(fac), _ptr(d), B, C, E, _ptr(ca), _ptr(co), st)
    assert status.cpu().numpy().tolist() == [[0] * C] * B
    rn, dn, can, con = (x.cpu().numpy() for x in (r, d, ca, co))
    lag = np.arange(F)[:, None] - np.arange(F)[None, :]
    for b in range(B):
        G = np.zeros((C * F, C * F))
        for i in range(C):
            for k in range(C):
                G[i * F:(i + 1) * F, k * F:(k + 1) * F] = np.where(lag >= 0, rn[b, i, k][np.clip(lag, 0, None)],
                                                                   rn[b, k, i][np.clip(-lag, 0, None)])
        for e in range(E):
            want = np.linalg.solve(G, dn[b, e].reshape(-1))
            assert np.abs(can[b, e] - want).max() <= 1e-9 * np.abs(want).max()
            for j in range(C):
                Gj = G[j * F:(j + 1) * F, j * F:(j + 1) * F]
                want = np.linalg.solve(Gj, dn[b, e, j])
                assert np.abs(con[b, e, j] - want).max() <= 1e-9 * np.abs(want).max()
    # the G_00 factor is chol(G)'s leading block: L L^T reproduces G
    L = np.tril(fac[: (C * F) ** 2].view(C * F, C * F).cpu().numpy())
    assert np.abs(L @ L.T - G_first(rn, C)).max() <= 1e-11 * np.abs(G_first(rn, C)).max()


def G_first(rn, C):
    lag = np.arange(F)[:, None] - np.arange(F)[None, :]
    G = np.zeros((C * F, C * F))
    for i in range(C):
        for k in range(C):
            G[i * F:(i + 1) * F, k * F:(k + 1) * F] = np.where(lag >= 0, rn[0, i, k][np.clip(lag, 0, None)],
                                                               rn[0, k, i][np.clip(-lag, 0, None)])
    return G


def _signals(kind, C, n, seed):
    if kind == "ar":
        return BO.mixtures(seed, C, n, 0.9)
    if kind == "lowpass":
        return BO.mixtures(seed, C, n, 0.98, leak=0.1, noise=0.002)     # strongly low-passed, high SAR
    _, _, src = O.synth_batch(seed, 1, n, C=C)
    ref = src[0].numpy()
    rng = np.random.RandomState(seed)
    est = ref + 0.15 * ref[::-1].copy() + 0.01 * rng.randn(C, n).astype(np.float32)
    return ref, est.astype(np.float32)


# C = 3 starts at n = 16000: at n = 1000 its 3*512 delayed copies outnumber the n+511 samples they live in, G is singular
# and the projection spans the whole padded signal -- SDR / SAR are rounding noise (150+ dB) in any implementation.
CASES = [(2, 1000, "ar", False), (2, 1000, "synth", True), (2, 16000, "lowpass", False), (2, 32003, "synth", True),
         (2, 32003, "lowpass", True), (3, 16000, "lowpass", True), (3, 16000, "synth", False), (3, 32003, "ar", True)]


@pytest.mark.parametrize("C,n,kind,swap", CASES)
def test_bss_eval_sources_matches_the_restatement(C, n, kind, swap):
    ref, est = _signals(kind, C, n, 20 + C + n % 7)
    if swap:
        est = est[::-1].copy()
    got = bss_eval_sources(ref, est)
    want = BO.bss_eval_sources(ref, est, "fft")
    assert list(got[3]) == list(want[3])
    if swap:
        assert list(got[3]) != list(range(C))
    for g, w in zip(got[:3], want[:3]):
        assert g.dtype == np.float64
        np.testing.assert_allclose(g, w, rtol=0, atol=1e-6)
    tref = torch.from_numpy(ref)
    assert np.array_equal(bss_eval_sources(tref, torch.from_numpy(est))[0], got[0])      # torch input, same numbers


@pytest.mark.parametrize("n,kind", [(8000, "ar"), (32003, "lowpass")])
def test_cal_sdri_matches_the_restatement(n, kind):
    ref, est = _signals(kind, 2, n, 31)
    mix = ref.sum(0)
    got = cal_SDRi(ref, est, mix)
    want = BO.cal_SDRi(ref, est, mix)
    assert abs(got - want) <= 1e-6, (got, want)


def test_batch_is_bitwise_per_utterance_and_reproducible():
    C, E, T = 2, 3, 9000
    lens = [9000, 511, 4097, 1000]
    ref, est = _ragged(C, E, lens, T, 8)
    rt, et = torch.from_numpy(ref).to(DEV), torch.from_numpy(est).to(DEV)
    lt = torch.tensor(lens, device=DEV)
    a = bss_eval_batch(rt, et, lt)
    b = bss_eval_batch(rt, et, lt)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # n = 511: the 2*512 delayed copies outnumber the 1022 samples they live in, so G is singular -> host fallback, flagged
    assert a[3].tolist() == [False, True, False, False]
    for u, n in enumerate(lens):
        one = bss_eval_batch(rt[u:u + 1, :, :n].contiguous(), et[u:u + 1, :, :n].contiguous(), torch.tensor([n], device=DEV))
        for x, y in zip(a[:3], one[:3]):
            assert torch.equal(x[u], y[0]), u
        assert torch.isfinite(a[0][u]).all()


def test_validation_and_the_singular_fallback():
    rng = np.random.RandomState(2)
    ref = rng.randn(2, 3000).astype(np.float32)
    est = rng.randn(2, 3000).astype(np.float32)
    z = ref.copy()
    z[1] = 0
    with pytest.raises(ValueError):
        bss_eval_sources(z, est)
    z = est.copy()
    z[0] = 0
    with pytest.raises(ValueError):
        bss_eval_sources(ref, z)
    with pytest.raises(ValueError):
        bss_eval_sources(ref, est[:, :2999])
    # two identical unit impulses: G = [[I, I], [I, I]], its Schur complement is exactly zero
    imp = np.zeros((1, 2, 3000), np.float32)
    imp[0, :, 0] = 1.0
    sdr, sir, sar, fb = bss_eval_batch(torch.from_numpy(imp).to(DEV), torch.from_numpy(est[None]).to(DEV),
                                       torch.tensor([3000], device=DEV))
    torch.cuda.synchronize()
    assert bool(fb[0])
    assert torch.isfinite(sdr).all()
    want = BO.bss_matrices(imp[0], est, "fft")[0]
    np.testing.assert_allclose(sdr[0].cpu().numpy(), want, rtol=0, atol=1e-6)


def test_evaluate_loader_calc_sdr(tmp_path, capsys):
    from scipy.io import wavfile
    from conv_tasnet_amd.data import AudioDataLoader, AudioDataset
    from conv_tasnet_amd.evaluate import evaluate_loader
    from conv_tasnet_amd.pit_criterion import cal_loss
    torch.manual_seed(3)
    m = ctn.ConvTasNet(32, 20, 16, 32, 3, 2, 1, 2).to(DEV)
    mix, lens, src = O.synth_batch(11, 3, 2400)
    src = src / src.abs().max() * 0.4
    manifests = {"mix": [], "s1": [], "s2": []}
    for u in range(3):
        n = 2400 - 300 * u
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
    sisnri, sdri = evaluate_loader(m, loader(), calc_sdr=True)
    out = capsys.readouterr().out
    assert sisnri == plain
    assert "\tSDRi=" in out and "Average SDR improvement" in out and "Average SISNR improvement" in out
    want = []
    with torch.no_grad():
        for pm, ml, ps in loader():
            est = m(pm.to(DEV))
            _, _, _, reord = cal_loss(ps.to(DEV), est, ml.to(DEV))
            for b, n in enumerate(ml.tolist()):
                want.append(BO.cal_SDRi(ps[b, :, :n].double().numpy(), reord[b, :, :n].double().cpu().numpy(),
                                        pm[b, :n].double().numpy()))
    assert len(want) == 3
    assert abs(sdri - np.mean(want)) <= 1e-6, (sdri, np.mean(want))


def test_large_batch_equals_single_utterance_calls():
    """48 utterances: many panel workgroups in flight at once; each must still score bitwise as it does alone."""
    B, C, E, n = 48, 2, 3, 6000
    ref = np.stack([BO.mixtures(500 + b, C, n)[0] for b in range(B)])
    est = np.concatenate([np.stack([BO.mixtures(500 + b, C, n)[1] for b in range(B)]), ref.sum(1, keepdims=True)], 1)
    rt, et = torch.from_numpy(ref).to(DEV), torch.from_numpy(est).to(DEV)
    sdr, sir, sar, fb = bss_eval_batch(rt, et, torch.full((B,), n, device=DEV))
    assert not bool(fb.any())
    for u in range(0, B, 5):
        one = bss_eval_batch(rt[u:u + 1], et[u:u + 1], torch.tensor([n], device=DEV))
        for x, y in zip((sdr, sir, sar), one[:3]):
            assert torch.equal(x[u], y[0]), u
