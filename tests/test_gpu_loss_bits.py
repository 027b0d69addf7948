"""GPU: the MixIT and the inactive-source PIT losses give, byte for byte, what tests/golden/loss_bits.npz recorded.

The two losses share their skeleton (csrc/ctn_moment_loss.h): the time partition, the reductions, the first-minimum rule, the load
and store paths.  A change to it must not move one bit of either loss, so this module compares bytes, not tolerances: loss,
per_utt, snr / pair, assign / perm_idx, active, and the SHA-256 of the gradient's bytes for g_loss = 0.75 and
g_per = linspace(0.5, 2.5, B).  The cases take every template instantiation (M = 2 .. 8, C = 2 .. 6; T = 4133: three chunks, two
passes per lane, the scalar path, a partial last quad), the 16-byte path (T = 8192), more utterances than the assignment kernel
has waves (B = 257), whole tie classes spread over more than 64 permutations (C = 6 with 1, 2 and 3 active references), and rows
of length 0, -7 and T + 5000 (every moment zero: every candidate ties and index 0 wins).

The fixture pins ONE toolchain: it was recorded from the commit before the skeleton was shared, and it stores torch.version.hip.
Another compiler may contract or schedule the fp64 arithmetic differently and move bits without anything being wrong; a failure
therefore names both versions.  To re-record, check out a commit known good (one whose tests/test_gpu_mixit.py and
tests/test_gpu_varpit.py pass against their fp64 oracles), build it, and run there
    python tests/test_gpu_loss_bits.py --record tests/golden/loss_bits.npz
never from a tree whose loss kernels are the ones under review.
"""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  puts the repository root on sys.path, also when this file runs as a script
import mixit_oracle as MO
import varpit_oracle as VO

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402

DEV = "cuda:0"
G_LOSS = 0.75
FIXTURE = os.path.join(conftest.GOLDEN, "loss_bits.npz")
CLAMPED = "clamped"                   # lens = 0, -7, T + 5000

# (loss, shape, variant): variant None = make_case as it is, a tuple = VarPIT active counts, CLAMPED = the lengths above
CASES = [("mixit", (3, M, 4133), None) for M in range(2, 9)] + \
        [("varpit", (C + 1, C, 4133), None) for C in range(2, 7)] + \
        [("mixit", (5, 4, 8192), None), ("varpit", (5, 3, 8192), None),
         ("mixit", (257, 2, 64), None), ("varpit", (257, 2, 64), None),
         ("varpit", (3, 6, 777), (1, 2, 3)),
         ("mixit", (3, 3, 777), CLAMPED), ("varpit", (3, 3, 777), CLAMPED)]


def _name(which, shape, variant):
    tag = "" if variant is None else "_" + (variant if isinstance(variant, str) else "act" + "".join(str(c) for c in variant))
    return "%s_%dx%dx%d%s" % ((which,) + tuple(shape) + (tag,))


def _compute(which, shape, variant):
    """-> {field: numpy array} of one case, the gradient as the 32 bytes of its SHA-256."""
    B, _, T = shape
    if which == "mixit":
        ref, e, lens, _ = MO.make_case(*shape, seed=0)
    else:
        ref, e, lens, _ = VO.make_case(*shape, seed=0, active_counts=None if variant in (None, CLAMPED) else variant)
    if variant == CLAMPED:
        lens = np.array([0, -7, T + 5000], np.int64)
    ref, e, lens = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (ref, e, lens))
    g_per = torch.linspace(0.5, 2.5, B, dtype=torch.float32).to(DEV)
    e.requires_grad_(True)
    if which == "mixit":
        loss, per_utt, snr, assign = ctn.cal_mixit_loss(ref, e, lens)
        out = dict(snr=snr, assign=assign)
    else:
        loss, per_utt, pair, perm_idx, active = ctn.cal_varpit_loss(ref, e, lens)
        out = dict(pair=pair, perm_idx=perm_idx, active=active)
    (grad,) = torch.autograd.grad(loss * G_LOSS + (per_utt * g_per).sum(), e)
    out = {k: v.detach().cpu().numpy() for k, v in dict(out, loss=loss, per_utt=per_utt).items()}
    out["grad_sha256"] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(grad.cpu().numpy()).tobytes()).digest(), np.uint8)
    return out


def record(path):
    arrays = {"hip_version": np.array(str(torch.version.hip))}
    for which, shape, variant in CASES:
        for field, a in _compute(which, shape, variant).items():
            arrays["%s__%s" % (_name(which, shape, variant), field)] = a
    np.savez_compressed(path, **arrays)
    print("recorded %d arrays of %d cases under HIP %s -> %s (%d bytes)"
          % (len(arrays), len(CASES), torch.version.hip, path, os.path.getsize(path)))


@pytest.fixture(scope="module")
def recorded():
    return dict(np.load(FIXTURE, allow_pickle=False))


@pytest.mark.parametrize("which,shape,variant", CASES, ids=[_name(*c) for c in CASES])
def test_bytes_equal_the_recorded_ones(recorded, which, shape, variant):
    name = _name(which, shape, variant)
    got = _compute(which, shape, variant)
    note = "recorded under HIP %s, running under HIP %s" % (str(recorded["hip_version"]), torch.version.hip)
    assert sorted(k for k in recorded if k.startswith(name + "__")) == sorted("%s__%s" % (name, f) for f in got), note
    for field, a in got.items():
        want = recorded["%s__%s" % (name, field)]
        assert a.dtype == want.dtype and a.shape == want.shape, "%s %s: %s" % (name, field, note)
        assert a.tobytes() == want.tobytes(), "%s %s differs from the recorded bytes (%s)" % (name, field, note)
    if variant == CLAMPED:                      # rows 0 and 1 are empty: every candidate ties, the first one wins
        idx = got["assign"] if which == "mixit" else got["perm_idx"]
        assert (idx[:2] == 0).all() and (got["per_utt"][:2] == 0).all()


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit("usage: python tests/test_gpu_loss_bits.py --record PATH.npz   (on a build of a commit known good)")
    record(sys.argv[2])
