"""separate(): same signature and output naming as the reference (src/separate.py:17-57).

Writes <base>.wav (the mixture) and <base>_s{c}.wav per speaker into out_dir.  The forward pass is the HIP path.
wav IO uses scipy (librosa is not a dependency here; the reference's librosa.output.write_wav no longer exists
upstream).  File-name quirk kept: ``basename.strip('.wav')`` strips CHARACTERS from both ends (:52-53).

``file_rate=R`` (not in the reference): the files are at R Hz instead of `sample_rate`.  Every mixture is resampled on the device to
`sample_rate` (resample.resample), separated, and its estimates are resampled back; the mixture and the _s{c} files are written at R
with the file's own length.  A file at any other rate raises ValueError.

``segment=S`` (not in the reference; samples at `sample_rate`): every file goes through longform.separate_long -- cut into overlapping
segments of S samples every `hop` (default S // 2), the segments of the files of one batch separated `segment_batch` at a time,
their speaker orders chained and the overlaps cross-faded on the device.  It composes with file_rate (resample -> long-form ->
resample back).  With segment=None the function is the path above, unchanged.
"""
import os

import numpy as np
import torch

from .conv_tasnet import ConvTasNet
from .data import EvalDataLoader, EvalDataset, read_wav_native
from .utils import remove_pad


def _write_wav(path, x, sample_rate):
    from scipy.io import wavfile
    wavfile.write(path, sample_rate, np.asarray(x, dtype=np.float32))


def _reader_at(file_rate):
    def read(path, _sample_rate):
        x, sr = read_wav_native(path)
        if sr != file_rate:
            raise ValueError("%s is at %d Hz, expected file_rate = %d" % (path, sr, file_rate))
        return x
    return read


def separate(model_path, mix_dir, mix_json, out_dir, use_cuda, sample_rate, batch_size, file_rate=None, segment=None, hop=None,
             segment_batch=8):
    if mix_dir is None and mix_json is None:
        print("Must provide mix_dir or mix_json! When providing mix_dir, mix_json is ignored.")
    model = ConvTasNet.load_model(model_path)
    model.eval()
    if use_cuda:
        model.cuda()
    dev = next(model.parameters()).device
    if segment is not None:
        from . import longform
        hop = int(segment) // 2 if hop is None else hop
        longform.check_geometry(segment, hop)
    if file_rate is None or int(file_rate) == int(sample_rate):
        dataset = EvalDataset(mix_dir, mix_json, batch_size=batch_size, sample_rate=sample_rate)
        file_rate = None
    else:
        from . import resample as rs
        file_rate = int(file_rate)
        rs.ratio(file_rate, sample_rate)
        dataset = EvalDataset(mix_dir, mix_json, batch_size=batch_size, sample_rate=sample_rate, reader=_reader_at(file_rate))
    eval_loader = EvalDataLoader(dataset)
    os.makedirs(out_dir, exist_ok=True)
    with torch.no_grad():
        for mixture, lens, filenames in eval_loader:
            mixture, lens = mixture.to(dev), lens.to(dev)
            if segment is not None:                              # every file on its own through the long-form path
                n_file = [int(n) for n in lens]
                files = [mixture[i, :n].contiguous() for i, n in enumerate(n_file)]
                low = files if file_rate is None else [rs.resample(x, file_rate, sample_rate) for x in files]
                est = longform.separate_long(model, low, segment, hop, batch_size=segment_batch)
                if file_rate is not None:
                    est = [rs.resample(e.contiguous(), sample_rate, file_rate)[:, :n] for e, n in zip(est, n_file)]
                flat_estimate = [e.cpu().numpy() for e in est]
                mixture_np = remove_pad(mixture, lens)
                out_rate = sample_rate if file_rate is None else file_rate
            elif file_rate is None:
                estimate_source = model(mixture)                 # [B, C, T]
                flat_estimate = remove_pad(estimate_source, lens)
                mixture_np = remove_pad(mixture, lens)
                out_rate = sample_rate
            else:                                                # every file on its own through the device resampler, both ways
                n_file = [int(n) for n in lens]
                low = [rs.resample(mixture[i, :n].contiguous(), file_rate, sample_rate) for i, n in enumerate(n_file)]
                batch = torch.zeros((len(low), max(x.shape[0] for x in low)), device=dev)
                for i, x in enumerate(low):
                    batch[i, :x.shape[0]] = x
                estimate_source = model(batch)
                flat_estimate = [rs.resample(estimate_source[i, :, :x.shape[0]].contiguous(), sample_rate, file_rate)[:, :n_file[i]]
                                 .cpu().numpy() for i, x in enumerate(low)]
                mixture_np = remove_pad(mixture, lens)
                out_rate = file_rate
            for i, path in enumerate(filenames):
                filename = os.path.join(out_dir, os.path.basename(path).strip('.wav'))
                _write_wav(filename + '.wav', mixture_np[i], out_rate)
                for c in range(flat_estimate[i].shape[0]):
                    _write_wav(filename + '_s{}.wav'.format(c + 1), flat_estimate[i][c], out_rate)


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="separate the wav files of a directory (or of a json list) with a trained Conv-TasNet")
    ap.add_argument("--model-path", required=True)
    ap.add_argument("--mix-dir", default=None)
    ap.add_argument("--mix-json", default=None)
    ap.add_argument("--out-dir", required=True)
    ap.add_argument("--use-cuda", type=int, default=1)
    ap.add_argument("--sample-rate", type=int, default=8000, help="the model's rate")
    ap.add_argument("--batch-size", type=int, default=1)
    ap.add_argument("--file-rate", type=int, default=None,
                    help="the files' rate when it is not --sample-rate: resampled on the device both ways, outputs written at this rate")
    ap.add_argument("--segment-s", type=float, default=None,
                    help="long recordings: separate in overlapping segments of this many seconds (the training length) and stitch them "
                         "on the device; default: every file in one pass")
    ap.add_argument("--hop-s", type=float, default=None, help="seconds between segment starts (default: half of --segment-s)")
    ap.add_argument("--segment-batch", type=int, default=8, help="segments per forward pass with --segment-s")
    a = ap.parse_args(argv)
    if a.hop_s is not None and a.segment_s is None:
        ap.error("--hop-s needs --segment-s")
    segment = None if a.segment_s is None else int(round(a.segment_s * a.sample_rate))
    hop = None if a.hop_s is None else int(round(a.hop_s * a.sample_rate))
    separate(a.model_path, a.mix_dir, a.mix_json, a.out_dir, a.use_cuda, a.sample_rate, a.batch_size, file_rate=a.file_rate,
             segment=segment, hop=hop, segment_batch=a.segment_batch)


if __name__ == "__main__":
    main()
