"""SI-SNRi evaluation (src/evaluate.py:21-130): forward + PIT reorder on the GPU, the numpy SI-SNR metric on host.

``evaluate(model_path, data_dir, calc_sdr, use_cuda, sample_rate, batch_size)`` is the reference's entry point
(src/evaluate.py:21): it loads the checkpoint, reads data_dir/{mix,s1,s2}.json through data.AudioDataset (full
utterances, scipy wav reader) and prints per-utterance and average SI-SNRi.  ``evaluate_loader(model, data_loader)`` is
the same loop over any iterable of (padded_mixture, mixture_lengths, padded_source) batches.  SDRi (cal_SDRi, :76-91) is
BSS Eval v3 on the GPU in fp64 (bss_eval.py): ``cal_SDRi`` for one utterance, ``evaluate_loader(..., calc_sdr=True)`` for
a whole loader, one bss_eval_batch call per batch with the mixture as an extra estimate row.  ``calc_stoi=True`` adds STOI and
ESTOI (stoi.py, csrc/ctn_stoi.hip) the same way: one stoi_both call per batch, the mixture row giving the anchor.
"""
import numpy as np
import torch

from .assign import cal_assign_loss, reorder_estimate
from .bss_eval import bss_eval_batch, sdr_improvement
from .conv_tasnet import ConvTasNet
from .pit_criterion import cal_loss
from .stoi import stoi_both, stoi_improvement
from .utils import remove_pad

PIT_MAX_SOURCES = 6          # cal_loss enumerates C! permutations up to here; beyond, evaluate_loader pairs with assign.py

def cal_SISNR(ref_sig, out_sig, eps=1e-8):
    """Scale-invariant SNR in dB of one signal pair, float64 numpy (src/evaluate.py:114-130)."""
    assert len(ref_sig) == len(out_sig)
    ref = ref_sig - np.mean(ref_sig)
    out = out_sig - np.mean(out_sig)
    proj = np.sum(ref * out) * ref / (np.sum(ref ** 2) + eps)
    noise = out - proj
    ratio = np.sum(proj ** 2) / (np.sum(noise ** 2) + eps)
    return 10 * np.log(ratio + eps) / np.log(10.0)


def cal_SISNRi(src_ref, src_est, mix):
    """Mean SI-SNR improvement over using the mixture itself; two speakers, like src/evaluate.py:94-111."""
    gains = [cal_SISNR(src_ref[c], src_est[c]) - cal_SISNR(src_ref[c], mix) for c in range(2)]
    return (gains[0] + gains[1]) / 2


def cal_SISNRi_all(src_ref, src_est, mix):
    """Mean SI-SNR improvement over all C speakers of src_ref, src_est [C, n] (cal_SISNRi is the reference's two)."""
    return float(np.mean([cal_SISNR(r, o) - cal_SISNR(r, mix) for r, o in zip(src_ref, src_est)]))


def cal_SDRi(src_ref, src_est, mix):
    """SDR improvement over using the mixture itself; two speakers, like src/evaluate.py:76-91.  src_ref, src_est [2, n],
    mix [n] (numpy or torch) -> float: ((sdr[0]-sdr0[0]) + (sdr[1]-sdr0[1])) / 2 with sdr from bss_eval_sources(src_ref,
    src_est) and sdr0 from bss_eval_sources(src_ref, [mix, mix]), both in one GPU call (the anchor is one extra row)."""
    ref, est, mx = (torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x) for x in (src_ref, src_est, mix))
    if ref.shape != est.shape or ref.dim() != 2 or mx.shape != ref.shape[1:]:
        raise ValueError("cal_SDRi: src_ref %s, src_est %s and mix %s do not match" % (tuple(ref.shape), tuple(est.shape),
                                                                                   tuple(mx.shape)))
    dev = torch.device("cuda", torch.cuda.current_device())
    rows = torch.cat([est.reshape(ref.shape), mx.reshape(1, -1)], 0).to(dev, torch.float32)
    sdr, sir, _, _ = bss_eval_batch(ref.to(dev, torch.float32).unsqueeze(0), rows.unsqueeze(0),
                                    torch.tensor([ref.shape[1]], device=dev))
    return float(sdr_improvement(sdr, sir)[0])


def evaluate(model_path, data_dir, calc_sdr=0, use_cuda=1, sample_rate=8000, batch_size=1, calc_stoi=0):
    """The reference's signature (src/evaluate.py:21-73).  -> average SI-SNRi over data_dir's utterances; with calc_stoi what
    evaluate_loader(calc_stoi=True) returns."""
    if calc_sdr:
        raise NotImplementedError("evaluate(calc_sdr=1) is not switched on: SDRi is computed by "
                                  "evaluate_loader(..., calc_sdr=True) and cal_SDRi (GPU BSS Eval, bss_eval.py)")
    from .data import AudioDataLoader, AudioDataset
    model = ConvTasNet.load_model(model_path)
    print(model)
    dataset = AudioDataset(data_dir, batch_size, sample_rate=sample_rate, segment=-1)
    data_loader = AudioDataLoader(dataset, batch_size=1, num_workers=2)
    return evaluate_loader(model, data_loader, use_cuda=bool(use_cuda), calc_stoi=bool(calc_stoi), sample_rate=sample_rate)


def evaluate_loader(model, data_loader, use_cuda=True, verbose=True, calc_sdr=False, calc_stoi=False, sample_rate=8000):
    """-> average SI-SNRi over every utterance of the loader; with calc_sdr (src/evaluate.py:62-72) -> (average SI-SNRi,
    average SDRi), every batch scored by one bss_eval_batch call (the mixture is an extra estimate row, so its anchor
    SDRs come out of the same call).  With calc_stoi the return value is followed by (average STOI, average ESTOI, average
    STOI improvement over the mixture): every batch scored by one stoi_both call at `sample_rate` on the reordered estimates
    plus the mixture row, an utterance's STOI / ESTOI being the mean over its speakers.  `model` is a ConvTasNet or a checkpoint
    path.  Up to 6 speakers the pairing is cal_loss's, as ever; for more it comes from assign.cal_assign_loss, the estimates are put
    into their references' order by assign.reorder_estimate (the inverse permutation), and an utterance's SI-SNRi is the mean over
    all its speakers; calc_sdr and calc_stoi keep their own limits on C."""
    if isinstance(model, str):
        model = ConvTasNet.load_model(model)
    model.eval()
    if use_cuda:
        model.cuda()
    dev = next(model.parameters()).device
    total, count = 0.0, 0
    total_sdri = 0.0
    total_stoi, total_estoi, total_stoii = 0.0, 0.0, 0.0
    with torch.no_grad():
        for padded_mixture, mixture_lengths, padded_source in data_loader:
            padded_mixture = padded_mixture.to(dev)
            mixture_lengths = mixture_lengths.to(dev)
            padded_source = padded_source.to(dev)
            estimate_source = model(padded_mixture)
            many = padded_source.size(1) > PIT_MAX_SOURCES
            if many:                                         # beyond cal_loss's C! search: the assignment solver, and its inverse
                _, _, _, perm = cal_assign_loss(padded_source, estimate_source, mixture_lengths)
                reorder = reorder_estimate(estimate_source, perm)
            else:
                _, _, _, reorder = cal_loss(padded_source, estimate_source, mixture_lengths)
            mixture = remove_pad(padded_mixture, mixture_lengths)
            source = remove_pad(padded_source, mixture_lengths)
            est = remove_pad(reorder, mixture_lengths)       # NOTE: the reordered estimate, as the reference does
            sdri = None
            if calc_sdr:
                rows = torch.cat([reorder, padded_mixture.unsqueeze(1)], 1)
                sdr, sir, _, _ = bss_eval_batch(padded_source, rows, mixture_lengths)
                sdri = sdr_improvement(sdr, sir).tolist()
            scores = None
            if calc_stoi:
                rows = torch.cat([reorder, padded_mixture.unsqueeze(1)], 1)
                d_stoi, d_estoi, _, _ = stoi_both(padded_source, rows, mixture_lengths, sample_rate)
                C = padded_source.shape[1]
                scores = (torch.diagonal(d_stoi[:, :C], dim1=1, dim2=2).mean(1).tolist(),
                          torch.diagonal(d_estoi[:, :C], dim1=1, dim2=2).mean(1).tolist(), stoi_improvement(d_stoi).tolist())
            for u, (mix, ref, out) in enumerate(zip(mixture, source, est)):
                if sdri is not None:
                    total_sdri += sdri[u]
                    if verbose:
                        print("\tSDRi=%.2f" % sdri[u])
                if scores is not None:
                    total_stoi += scores[0][u]
                    total_estoi += scores[1][u]
                    total_stoii += scores[2][u]
                    if verbose:
                        print("\tSTOI=%.3f ESTOI=%.3f" % (scores[0][u], scores[1][u]))
                ref, out, mix = ref.astype(np.float64), out.astype(np.float64), mix.astype(np.float64)
                v = cal_SISNRi_all(ref, out, mix) if many else cal_SISNRi(ref, out, mix)
                if verbose:
                    print("Utt %d\tSI-SNRi=%.2f" % (count + 1, v))
                total += v
                count += 1
    avg = total / max(count, 1)
    if calc_stoi:
        stoi_avgs = tuple(t / max(count, 1) for t in (total_stoi, total_estoi, total_stoii))
        if verbose:
            print("Average STOI: {0:.3f}".format(stoi_avgs[0]))
            print("Average ESTOI: {0:.3f}".format(stoi_avgs[1]))
            print("Average STOI improvement: {0:.3f}".format(stoi_avgs[2]))
    if calc_sdr:
        avg_sdri = total_sdri / max(count, 1)
        if verbose:
            print("Average SDR improvement: {0:.2f}".format(avg_sdri))
            print("Average SISNR improvement: {0:.2f}".format(avg))
        return (avg, avg_sdri) + stoi_avgs if calc_stoi else (avg, avg_sdri)
    if verbose:
        print("Average SISNR improvement: {0:.2f}".format(avg))
    return (avg,) + stoi_avgs if calc_stoi else avg
